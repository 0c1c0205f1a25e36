"""Supervised classification, host side (no GPU): the header and the built library, the wrappers' refusals, the AUROC reducers
against brute-force pair loops, the two experiments and the module's `model.classifier` block, the launches of Engine.classify_step
against the stub library of tools/text_launch_trace.py, and the refusals."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import classify_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
ENTRIES = ("medmoe_cls_head_logits", "medmoe_cls_head_step", "medmoe_cls_head_scratch", "medmoe_auroc_counts")


# ------------------------------------------------------------------------------------------------------------------------------------------
# header, library, signature table
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    from medmoe_amd import lib_path, ops
    lib = ctypes.CDLL(lib_path())
    for name in ENTRIES:
        m = re.search(r"^(int|long long) %s\((.*)\);" % name, hdr, re.M)
        assert m, name
        assert hasattr(lib, name), name
        short = name[len("medmoe_"):]
        if short in ops._SIGS:
            assert len(m.group(2).split(",")) == len(ops._SIGS[short]) + 1, name                  # + the stream
            assert m.group(2).endswith("hipStream_t stream"), name
    src = open(os.path.join(ROOT, "medmoe_amd", "csrc", "classify.hip")).read()
    # no fp32 atomics: every atomicAdd of the file adds an integer (counts are int / unsigned long long)
    for line in src.splitlines():
        if "atomicAdd(" in line and not line.lstrip().startswith("//"):
            assert re.search(r"atomicAdd\((counts|o) ?\+? ?\d?,|atomicAdd\(counts,", line), line
    assert "mm_launch_det_sum" in src and "g_mm_nondet" not in src


# ------------------------------------------------------------------------------------------------------------------------------------------
# the wrappers refuse bad arguments before any launch (CPU tensors: a call that got through would raise the "GPU" RuntimeError)
# ------------------------------------------------------------------------------------------------------------------------------------------
def _args(N=4, D=64, C=3):
    return torch.zeros(N, D), torch.zeros(C, D), torch.zeros(C), torch.zeros(N, dtype=torch.int32), torch.zeros(C, D), torch.zeros(C)


def test_wrappers_refuse_bad_shapes_and_dtypes():
    from medmoe_amd import ops
    x, W, b, t, dW, db = _args()
    with pytest.raises(ValueError, match="x has D = 96"):
        ops.cls_head_step(torch.zeros(4, 96), torch.zeros(3, 96), b, t, torch.zeros(3, 96), db)
    with pytest.raises(ValueError, match="x has D = 96"):
        ops.cls_head_logits(torch.zeros(4, 96), torch.zeros(3, 96), b)
    with pytest.raises(ValueError, match="W has C = 0"):
        ops.cls_head_step(x, torch.zeros(0, 64), torch.zeros(0), t, torch.zeros(0, 64), torch.zeros(0))
    with pytest.raises(ValueError, match="W has C = 65"):
        ops.cls_head_step(x, torch.zeros(65, 64), torch.zeros(65), t, torch.zeros(65, 64), torch.zeros(65))
    with pytest.raises(ValueError, match="W has C = 65"):
        ops.cls_head_logits(x, torch.zeros(65, 64), torch.zeros(65))
    with pytest.raises(ValueError, match="x must be contiguous"):
        ops.cls_head_step(torch.zeros(4, 128)[:, ::2], W, b, t, dW, db)
    with pytest.raises(ValueError, match="W must be contiguous"):
        ops.cls_head_logits(x, torch.zeros(64, 3).t(), b)
    with pytest.raises(ValueError, match="targets must be torch.int32"):
        ops.cls_head_step(x, W, b, t.long(), dW, db)
    with pytest.raises(ValueError, match="targets must be torch.int8"):
        ops.cls_head_step(x, W, b, torch.zeros(4, 3, dtype=torch.int32), dW, db, task="multilabel")
    with pytest.raises(ValueError, match="targets must be contiguous with shape"):
        ops.cls_head_step(x, W, b, torch.zeros(5, dtype=torch.int32), dW, db)
    with pytest.raises(ValueError, match="x must be an fp32 tensor"):
        ops.cls_head_step(x.double(), W, b, t, dW, db)
    with pytest.raises(ValueError, match="dW must have shape"):
        ops.cls_head_step(x, W, b, t, torch.zeros(3, 128), db)
    with pytest.raises(ValueError, match="dx must have shape"):
        ops.cls_head_step(x, W, b, t, dW, db, dx=torch.zeros(4, 128))
    with pytest.raises(ValueError, match="task"):
        ops.cls_head_step(x, W, b, t, dW, db, task="binary")
    with pytest.raises(ValueError, match="pos_weight"):
        ops.cls_head_step(x, W, b, t, dW, db, pos_weight=torch.ones(3))
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.cls_head_step(x, W, b, t, dW, db, label_smoothing=1.0)
    with pytest.raises(RuntimeError, match="GPU"):                   # everything in order: the launch itself has no CPU form
        ops.cls_head_logits(x, W, b)
    s, tg = torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int8)
    with pytest.raises(ValueError, match="targets must be int8"):
        ops.auroc_counts(s, tg.long())
    with pytest.raises(ValueError, match="shaped like scores"):
        ops.auroc_counts(s, tg[:3])
    with pytest.raises(ValueError, match="scores must be contiguous"):
        ops.auroc_counts(torch.zeros(3, 4).t(), tg)
    with pytest.raises(ValueError, match=r"scores must be \[N, C\]"):
        ops.auroc_counts(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int8))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.auroc_counts(s, tg)
    from medmoe_amd.classify import ClassifierHead
    for kw in (dict(d=96, num_classes=3), dict(d=64, num_classes=0), dict(d=64, num_classes=65), dict(d=64, num_classes=3, task="binary"),
               dict(d=64, num_classes=3, task="multilabel", label_smoothing=0.1), dict(d=64, num_classes=3, pos_weight=torch.ones(3))):
        with pytest.raises(ValueError):
            ClassifierHead(device="cpu", **kw)


# ------------------------------------------------------------------------------------------------------------------------------------------
# reducers against brute force
# ------------------------------------------------------------------------------------------------------------------------------------------
def _midrank_auroc_loops(s, t):
    """AUROC of one class by the definition: the share of (positive, negative) pairs ranked correctly, a tie counting one half."""
    pos, neg = [v for v, y in zip(s, t) if y == 1], [v for v, y in zip(s, t) if y == 0]
    if not pos or not neg:
        return float("nan")
    return sum(1.0 if p > n else 0.5 if p == n else 0.0 for p in pos for n in neg) / (len(pos) * len(neg))


def test_auroc_reducers_match_brute_force_with_ties_and_one_sided_classes(monkeypatch):
    from medmoe_amd import classify, ops
    g = torch.Generator().manual_seed(5)
    N, C = 61, 4
    scores = torch.randint(-3, 4, (N, C), generator=g).float() / 4.0                 # seven distinct values: ties everywhere
    targets = (torch.rand(N, C, generator=g) < 0.5).to(torch.int8)
    targets[torch.rand(N, C, generator=g) < 0.2] = -1
    targets[:, 2] = torch.where(targets[:, 2] == 0, torch.tensor(-1, dtype=torch.int8), targets[:, 2])      # class 2: no negative
    counts = torch.from_numpy(R.auroc_counts_reference(scores.numpy(), targets.numpy()))
    assert int(counts[:, 3].sum()) > 0 and int(counts[2, 1]) == 0
    per, mean = classify.auroc_from_counts(counts)
    want = [_midrank_auroc_loops(scores[:, c].tolist(), targets[:, c].tolist()) for c in range(C)]
    assert per.dtype == torch.float64 and per[2] != per[2] and want[2] != want[2]
    for c in (0, 1, 3):
        assert abs(float(per[c]) - want[c]) < 1e-15
    assert abs(mean - np.mean([want[c] for c in (0, 1, 3)])) < 1e-15          # the one-sided class is left out of the mean
    none, nomean = classify.auroc_from_counts(torch.zeros(3, 4, dtype=torch.int64))
    assert bool(torch.isnan(none).all()) and nomean != nomean
    # the bank and the metrics dict on top of the counts (the launch replaced by the brute-force counts)
    monkeypatch.setattr(ops, "auroc_counts", lambda s, t: torch.from_numpy(R.auroc_counts_reference(s.numpy(), t.numpy())))
    bank = classify.ScoreBank(3, "cpu", task="multiclass", capacity=2)
    z = torch.tensor([[2.0, 1.0, 0.0], [0.0, 3.0, 3.0], [0.0, 0.0, 1.0], [5.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    y = torch.tensor([0, 2, 2, 1, -1])
    bank.add(z[:2], y[:2]); bank.add(z[2:], y[2:])                                  # grows past its capacity
    assert len(bank) == 5 and torch.equal(bank.scores, z) and bank.labels.tolist() == y.tolist()
    assert bank.targets.tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 1, 0], [-1, -1, -1]]
    m = classify.classification_metrics(bank, ["a", "b", "c"])
    assert m["acc"] == 2 / 4                                                         # row 1 ties towards class 1, row 3 is wrong, row 4 not counted
    assert sorted(m) == ["acc", "auroc/a", "auroc/b", "auroc/c", "auroc_mean"]
    assert m["auroc/a"] == _midrank_auroc_loops(z[:4, 0].tolist(), [1, 0, 0, 0])
    ml = classify.ScoreBank(2, "cpu", task="multilabel")
    ml.add(torch.tensor([[0.5, 0.1], [0.2, 0.9]]), torch.tensor([[1, -1], [0, 1]]))
    mm = classify.classification_metrics(ml)
    assert "acc" not in mm and mm["auroc/0"] == 1.0 and mm["auroc/1"] != mm["auroc/1"] and mm["auroc_mean"] == 1.0
    with pytest.raises(ValueError):
        ml.add(torch.zeros(2, 3), torch.zeros(2, 3))


# ------------------------------------------------------------------------------------------------------------------------------------------
# experiments and the module's block
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_both_experiments_compose_and_their_keys_reach_the_module(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from src.models.classifier_module import MedMoEClassifierLightningModule as M, classifier_block
    for exp, mode in (("linear_probe_medmoe_cfg2", "linear_probe"), ("finetune_medmoe_cfg2", "finetune")):
        cfg = compose(CONFIGS, "train.yaml", [f"experiment={exp}", "model.classifier.num_classes=14", "model.classifier.task=multilabel",
                                              "model.classifier.label_key=findings"])
        assert cfg.model._target_ == "src.models.classifier_module.MedMoEClassifierLightningModule" and cfg.model.fused_step is True
        assert cfg.data._target_.endswith("UnimedDataModule") and cfg.model.model.vision.arch == "vit_b16"
        blk = classifier_block(cfg.model.classifier)
        assert (blk["mode"], blk["num_classes"], blk["task"], blk["label_key"]) == (mode, 14, "multilabel", "findings")
        assert blk["pos_weight"] is None and blk["class_names"] is None and blk["label_smoothing"] == 0.0
    with pytest.raises(KeyError, match="n_classes"):
        M(torch.nn.Identity(), classifier={"num_classes": 5, "n_classes": 5})
    with pytest.raises(KeyError, match="num_classes"):
        M(torch.nn.Identity(), classifier={"task": "multiclass"})
    with pytest.raises(KeyError, match="model.classifier is missing"):
        M(torch.nn.Identity())
    with pytest.raises(ValueError, match="mode"):
        M(torch.nn.Identity(), classifier={"num_classes": 5, "mode": "probe"})
    with pytest.raises(ValueError, match="class_names"):
        M(torch.nn.Identity(), classifier={"num_classes": 5, "class_names": ["a"]})
    with pytest.raises(NotImplementedError, match="fused_step"):
        M(torch.nn.Identity(), classifier={"num_classes": 5}, fused_step=False)
    with pytest.raises(NotImplementedError, match="HIP engine"):
        M(torch.nn.Identity(), classifier={"num_classes": 5})
    # absent model.classifier: the pretraining experiments and their module are what they were
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert "classifier" not in dict(base.model) and base.model._target_ == "src.models.medmoe_module.MedMoEPretrainingLightningModule"
    import inspect
    from src.models.medmoe_module import MedMoEPretrainingLightningModule as P
    assert "classifier" not in inspect.signature(P.__init__).parameters


# ------------------------------------------------------------------------------------------------------------------------------------------
# launch sequences against the stub library
# ------------------------------------------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("text_launch_trace", os.path.join(ROOT, "tools", "text_launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trace(fn, **cfg_over):
    """The launches `fn(engine, head, batch)` makes on a fresh tiny2 engine and a fresh head against the stub library."""
    tool = _tool()
    import medmoe_oracle as O
    from medmoe_amd.classify import ClassifierHead
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    lib = tool._TraceLib()
    with tool._installed(lib, {}):
        cfg = config_by_name("tiny2")
        for k, v in cfg_over.items():
            setattr(cfg, k, v)
        eng = Engine(cfg, "cpu")
        head = ClassifierHead(cfg.d_out, 5, "cpu")
        batch = O.synthetic_batch(O.config_by_name("tiny2"), 8, min_len=4)
        batch = {"image": batch["image"], "label": batch["label"] % 5}
        lib.eng = eng
        fn(eng, head, batch)
    return lib.trace


_name = lambda l: l.split("(")[0]


def test_probe_step_issues_no_backward_or_optimiser_launch_of_the_engines_stores():
    fwd = _trace(lambda e, h, b: e.embed_image(b["image"]))
    tr = _trace(lambda e, h, b: e.classify_step(b, h, train_tower=False))
    assert len(fwd) > 10 and tr[:len(fwd)] == fwd                                   # the evaluation form of the image pass, launch for launch
    rest = tr[len(fwd):]
    assert [_name(l) for l in rest] == ["medmoe_cls_head_step", "medmoe_sumsq_det", "medmoe_adam_step"]
    for l in rest[1:]:                                                               # the head's own arena: nothing of the engine's stores
        assert "params." not in l and "ws." not in l, l
    assert "ws.img_g+0" in rest[0] and "params." not in rest[0] and "ws.d_img_g" not in rest[0]
    for l in tr:
        assert not _name(l).startswith(("medmoe_gemm_tn", "medmoe_layernorm_bwd", "medmoe_attn_bwd", "medmoe_scale_attn_bwd", "medmoe_router_bwd",
                                        "medmoe_drop_path_scales")), l
    quiet = _trace(lambda e, h, b: e.classify_step(b, h, train_tower=False, optimizer=False))
    assert quiet == tr[:len(fwd) + 1]
    ev = _trace(lambda e, h, b: e.classify_eval(b, h))
    assert [_name(l) for l in ev] == [_name(l) for l in quiet] and "tmp" in ev[-1]


def test_finetune_step_issues_the_backward_none_sequence():
    def parts(e, h, b):
        e.params.zero_grad()
        e._forward_image_train(b["image"])
        e.ws["d_img_l"].zero_()
        e.backward(None)
    ref = _trace(parts)
    fwd = _trace(lambda e, h, b: e._forward_image_train(b["image"]))
    tr = _trace(lambda e, h, b: e.classify_step(b, h, train_tower=True, optimizer=False))
    assert ref[:len(fwd)] == fwd and len(ref) > len(fwd) + 10
    assert tr[:len(fwd)] == fwd and _name(tr[len(fwd)]) == "medmoe_cls_head_step" and "ws.d_img_g+0" in tr[len(fwd)]
    assert tr[len(fwd) + 1:] == ref[len(fwd):]                                      # backward(None), launch for launch, argument for argument
    full = _trace(lambda e, h, b: e.classify_step(b, h, train_tower=True))
    assert full[:len(tr)] == tr
    # ONE clip norm over the head and the image arena, then Adam on each (the image arena's derived copies follow its launch)
    opt = [_name(l) for l in full[len(tr):]]
    assert [n for n in opt if n in ("medmoe_sumsq_det", "medmoe_adam_step")] == ["medmoe_sumsq_det", "medmoe_sumsq_det", "medmoe_adam_step",
                                                                                 "medmoe_adam_step"]
    assert "params.g32" in full[len(tr) + 1] and "params.normsq" in [l for l in full if _name(l) == "medmoe_adam_step"][-1]
    # drop path: the scales are drawn by the fine-tuning step and by no probe step
    dp = _trace(lambda e, h, b: e.classify_step(b, h, train_tower=True, optimizer=False), vit_drop_path=0.1)
    assert _name(dp[0]) == "medmoe_drop_path_scales"
    dpp = _trace(lambda e, h, b: e.classify_step(b, h, train_tower=False, optimizer=False), vit_drop_path=0.1)
    assert not any(_name(l) == "medmoe_drop_path_scales" for l in dpp)


def test_dropout_step_advances_under_finetuning_only():
    steps = {}

    def run(train_tower):
        def fn(e, h, b):
            e.classify_step(b, h, train_tower=train_tower)
            steps[train_tower] = e.dropout_step
        return fn
    _trace(run(True)); _trace(run(False))
    assert steps == {True: 1, False: 0}


# ------------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_keys():
    def dist(e, h, b):
        e.dist = True
        with pytest.raises(NotImplementedError, match="self.dist"):
            e.classify_step(b, h, train_tower=False)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            e.classify_eval(b, h)
    _trace(dist)

    def ema(e, h, b):
        with pytest.raises(NotImplementedError, match="ema_decay.*model.ema.decay"):
            e.classify_step(b, h, train_tower=True)
        e.classify_step(b, h, train_tower=False)                                    # the probe writes no store of the engine: allowed
    _trace(ema, ema_decay=0.999)
    from medmoe_amd.swin_engine import SwinEngine
    eng = SwinEngine.__new__(SwinEngine)
    for call in (lambda: eng.classify_step({}, None, True), lambda: eng.classify_eval({}, None)):
        with pytest.raises(NotImplementedError, match="swin_t"):
            call()

    class SwinNet(torch.nn.Module):
        swin, engine = object(), object()

    from src.models.classifier_module import MedMoEClassifierLightningModule as M
    with pytest.raises(NotImplementedError, match="swin_t"):
        M(SwinNet(), classifier={"num_classes": 5})
