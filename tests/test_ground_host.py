"""Phrase grounding, host side (no GPU): the header and the built library, the wrappers' refusals, the float64 restatement
against the oracle's attention maps, the metrics against brute force, word_spans, prepare_boxes, the synthetic annotations, the experiment and
the module's `model.grounding` block."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import ground_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
ENTRIES = ("medmoe_ground_maps", "medmoe_ground_score")


def test_header_declares_the_entries_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    from medmoe_amd import lib_path, ops
    lib = ctypes.CDLL(lib_path())
    for name in ENTRIES:
        m = re.search(r"^int %s\((.*)\);" % name, hdr, re.M)
        assert m, name
        assert hasattr(lib, name), name
        assert len(m.group(1).split(",")) == len(ops._SIGS[name[len("medmoe_"):]]) + 1, name                  # + the stream
        assert m.group(1).endswith("hipStream_t stream"), name
    src = open(os.path.join(ROOT, "medmoe_amd", "csrc", "ground.hip")).read()
    assert "atomic" not in src.lower() and "g_mm_nondet" not in src
    assert '#include "seg_plan.h"' in src and "seg_src(" in src and "mfma_f32_16x16x32_bf16" in src
    # seg_plan.h is included, not changed: the map of the segmentation head
    assert "SEG_HD SegSrc seg_src(int dst, float scale, int g)" in open(os.path.join(ROOT, "medmoe_amd", "csrc", "seg_plan.h")).read()


def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


def test_wrappers_refuse_bad_shapes_dtypes_and_tables():
    from medmoe_amd import ops
    ctx, words, lens = _bf(2, 64, 64), _bf(3, 16, 64), torch.tensor([4, 16, 1], dtype=torch.int32)
    ent = [[0, 0, 0, 4], [1, 1, 3, 16], [1, 2, 0, 1]]
    with pytest.raises(ValueError, match="ctx must be a torch.bfloat16"):
        ops.ground_maps(ctx.float(), words, lens, ent)
    with pytest.raises(ValueError, match="words must be a torch.bfloat16"):
        ops.ground_maps(ctx, words.float(), lens, ent)
    with pytest.raises(ValueError, match="cap_lens must be a torch.int32"):
        ops.ground_maps(ctx, words, lens.long(), ent)
    with pytest.raises(ValueError, match="entries must be an integer table"):
        ops.ground_maps(ctx, words, lens, torch.tensor(ent, dtype=torch.float32))
    with pytest.raises(ValueError, match=r"entries must be \[n, 4\]"):
        ops.ground_maps(ctx, words, lens, [[0, 0, 1]])
    with pytest.raises(ValueError, match="ctx has D = 96"):
        ops.ground_maps(_bf(2, 64, 96), _bf(3, 16, 96), lens, ent)
    with pytest.raises(ValueError, match="words has D = 128"):
        ops.ground_maps(ctx, _bf(3, 16, 128), lens, ent)
    with pytest.raises(ValueError, match="P = 1089 regions"):                       # g = 33
        ops.ground_maps(_bf(1, 33 * 33, 64), words, lens, ent)
    with pytest.raises(ValueError, match="P = 63 regions"):
        ops.ground_maps(_bf(2, 63, 64), words, lens, ent)
    with pytest.raises(ValueError, match="words has T = 81"):
        ops.ground_maps(ctx, _bf(3, 81, 64), lens, ent)
    with pytest.raises(ValueError, match=r"entries\[1\] has the word span \[3, 17\)"):      # past cap_lens
        ops.ground_maps(ctx, words, lens, [[0, 0, 0, 4], [1, 1, 3, 17]])
    with pytest.raises(ValueError, match=r"entries\[0\] has the word span \[2, 5\).*cap_lens\[0\] = 4"):
        ops.ground_maps(ctx, words, lens, [[0, 0, 2, 5]])
    with pytest.raises(ValueError, match=r"entries\[0\] has the word span \[2, 2\)"):       # empty
        ops.ground_maps(ctx, words, lens, [[0, 0, 2, 2]])
    with pytest.raises(ValueError, match=r"entries\[0\] has the word span \[-1, 2\)"):
        ops.ground_maps(ctx, words, lens, [[0, 0, -1, 2]])
    with pytest.raises(ValueError, match=r"names an image outside \[0, 2\)"):
        ops.ground_maps(ctx, words, lens, [[2, 0, 0, 1]])
    with pytest.raises(ValueError, match=r"names a caption outside \[0, 3\)"):
        ops.ground_maps(ctx, words, lens, [[0, -1, 0, 1]])
    with pytest.raises(ValueError, match=r"cap_lens of a listed caption lies outside \[1, 16\]"):
        ops.ground_maps(ctx, words, torch.tensor([4, 17, 1], dtype=torch.int32), [[0, 1, 0, 1]])
    with pytest.raises(ValueError, match="temp1 = 65"):
        ops.ground_maps(ctx, words, lens, ent, temp1=65.0)
    with pytest.raises(ValueError, match="mode must be one of"):
        ops.ground_maps(ctx, words, lens, ent, mode="softmax")
    with pytest.raises(ValueError, match="cap_lens holds 2 lengths"):
        ops.ground_maps(ctx, words, lens[:2], ent)
    with pytest.raises(RuntimeError, match="GPU"):                                  # everything in order: the launch itself has no CPU form
        ops.ground_maps(ctx, words, lens, ent)
    h, bx = torch.zeros(3, 64), torch.zeros(3, 2, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="h must be a torch.float32"):
        ops.ground_score(h.double(), bx, (32, 32))
    with pytest.raises(ValueError, match="boxes must be an int32 or int64"):
        ops.ground_score(h, bx.float(), (32, 32))
    with pytest.raises(ValueError, match=r"boxes must be \[3, NB, 4\]"):
        ops.ground_score(h, bx[:2], (32, 32))
    with pytest.raises(ValueError, match="NB = 9"):
        ops.ground_score(h, torch.zeros(3, 9, 4, dtype=torch.int32), (32, 32))
    with pytest.raises(ValueError, match="NTH = 5"):
        ops.ground_score(h, bx, (32, 32), thetas=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match="H = 7 is smaller than the region grid g = 8"):
        ops.ground_score(h, bx, (7, 32))
    with pytest.raises(ValueError, match="W = 5 is smaller"):
        ops.ground_score(h, bx, (32, 5))
    with pytest.raises(ValueError, match="P = 1089"):
        ops.ground_score(torch.zeros(1, 1089), bx[:1], (64, 64))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ground_score(h, bx, (32, 32), thetas=(0.5,))


def test_reference_attention_equals_the_oracles_att_maps():
    """One-word spans on the matched pairs: a row of the reference's att_maps (losses.py:993-995), float64, to 1e-12."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import medmoe_oracle as O
    g = torch.Generator().manual_seed(5)
    B, D, T, lens = 3, 16, 7, [7, 2, 5]
    img_l = torch.randn(B, D, 3, 3, generator=g, dtype=torch.float64)
    words = torch.randn(B, D, T, generator=g, dtype=torch.float64)
    _, _, maps = O.gloria_local(img_l, words, lens, temp1=4.0)
    ctx, w = img_l.reshape(B, D, 9).permute(0, 2, 1), words.permute(0, 2, 1)
    ent = [(i, i, t, t + 1) for i in range(B) for t in range(lens[i])]
    h = R.maps_reference(ctx, w, lens, ent, "attention", temp1=4.0)
    want = torch.cat([maps[i].reshape(lens[i], 9) for i in range(B)])
    assert float((h - want).abs().max()) < 1e-12 and float((h.sum(dim=1) - 1).abs().max()) < 1e-12
    # a span is the mean of its words' rows
    h2 = R.maps_reference(ctx, w, lens, [(0, 0, 2, 6)], "attention", temp1=4.0)
    assert float((h2[0] - maps[0].reshape(7, 9)[2:6].mean(dim=0)).abs().max()) < 1e-12
    # the cosine map by a loop
    hc = R.maps_reference(ctx, w, lens, [(1, 2, 1, 4)], "cosine")
    u = w[2, 1:4].sum(dim=0)
    for p in range(9):
        assert abs(float(hc[0, p]) - float(ctx[1, p] @ u) / (float(ctx[1, p].norm()) * float(u.norm()))) < 1e-12


def test_grounding_metrics_match_brute_force_with_the_nan_exclusions():
    from medmoe_amd.ground import GroundBank, entry_cnr, grounding_metrics
    rng = np.random.default_rng(3)
    H, W, thetas = 12, 10, (0.25, 0.5)
    bank, all_i, all_d = GroundBank(thetas, "cpu"), [], []
    assert grounding_metrics(bank) == {}
    for batch in range(3):
        n = 7
        hf = rng.normal(size=(n, H, W)).astype(np.float32)
        hf[2] = 0.25                                                              # a constant map: no contrast
        boxes = np.zeros((n, 2, 4), dtype=np.int64)
        for e in range(n):
            x0, y0 = rng.integers(0, W - 1), rng.integers(0, H - 1)
            boxes[e, 0] = (x0, y0, rng.integers(x0 + 1, W + 1), rng.integers(y0 + 1, H + 1))
        boxes[0, 0] = 0                                                           # no box
        boxes[1, 0] = (0, 0, W, H)                                                # the frame: no outside
        boxes[3, 1] = (2, 2, 6, 7)
        ref = R.records_reference(hf, boxes, thetas)
        rec_i = np.concatenate([np.stack([ref["y"], ref["x"], ref["hit"], ref["area"]], axis=1),
                                np.stack([ref["inter"], ref["pred"]], axis=2).reshape(n, -1)], axis=1)
        rec_d = np.stack([ref["S_in"], ref["Q_in"], ref["S_all"], ref["Q_all"]], axis=1)
        rec = {"rec_i": torch.from_numpy(rec_i).to(torch.int32), "rec_d": torch.from_numpy(rec_d), "size": (H, W), "thetas": thetas}
        cnr = entry_cnr(rec["rec_i"], rec["rec_d"], (H, W))
        assert bool(torch.isnan(cnr[0])) and bool(torch.isnan(cnr[1])) and bool(torch.isnan(cnr[2])) and bool(torch.isfinite(cnr[3:]).all())
        bank.add(rec)
        all_i.append(rec_i); all_d.append(rec_d)
    met, want = grounding_metrics(bank), R.metrics_reference(np.concatenate(all_i), np.concatenate(all_d), (H, W), 2)
    assert met["n_entries"] == 21 and want["n_boxed"] == 18 and want["n_cnr"] == 12 and len(bank) == 3
    assert abs(met["pg_acc"] - want["pg_acc"]) < 1e-15 and abs(met["cnr_mean"] - want["cnr_mean"]) < 1e-12
    for k, key in enumerate(("0.25", "0.5")):
        assert abs(met[f"iou@{key}"] - want["iou"][k]) < 1e-14 and abs(met[f"dice@{key}"] - want["dice"][k]) < 1e-14
    assert sorted(met) == sorted(["pg_acc", "cnr_mean", "n_entries", "iou@0.25", "iou@0.5", "dice@0.25", "dice@0.5"])
    with pytest.raises(ValueError, match="thresholds"):
        bank.add(dict(rec, thetas=(0.5,)))
    with pytest.raises(ValueError, match="rec_i int32"):
        bank.add(dict(rec, rec_i=rec["rec_i"][:, :6]))
    bank.reset()
    assert len(bank) == 0 and not bank.ints.any() and not bank.sums.any()
    # nothing boxed: every mean is NaN, the count stays
    none = GroundBank((), "cpu")
    none.add({"rec_i": torch.zeros(2, 4, dtype=torch.int32), "rec_d": torch.zeros(2, 4, dtype=torch.float64), "size": (4, 4), "thetas": ()})
    m = grounding_metrics(none)
    assert m["n_entries"] == 2 and m["pg_acc"] != m["pg_acc"] and m["cnr_mean"] != m["cnr_mean"]


def test_word_spans_match_a_loop_and_refuse_a_span_without_a_kept_token():
    from medmoe_amd.ground import word_spans
    g = torch.Generator().manual_seed(9)
    B, T = 6, 12
    seg = torch.full((B, T), -1, dtype=torch.int32)
    for b in range(B):
        n, w = int(torch.randint(4, T + 1, (1,), generator=g)), -1
        for t in range(1, n - 1):                                                # token 0 ([CLS]) and the tail are dropped
            w += int(t == 1 or torch.rand(1, generator=g) < 0.6)
            seg[b, t] = w
    lo = torch.tensor([1, 0, 2, 1, 1, 2])
    hi = torch.tensor([3, 2, 3, 12, 2, 12])
    got = word_spans(seg, lo, hi)
    for b in range(B):
        ws = [int(seg[b, t]) for t in range(int(lo[b]), int(hi[b])) if seg[b, t] >= 0]
        assert got[b].tolist() == [min(ws), max(ws) + 1], b
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, 2)
    with pytest.raises(ValueError, match="holds no kept token"):
        word_spans(seg, torch.tensor([0] * B), torch.tensor([1] * B))
    with pytest.raises(ValueError, match="empty or lies outside"):
        word_spans(seg, lo, lo)
    with pytest.raises(ValueError, match="empty or lies outside"):
        word_spans(seg, lo, hi + 1)
    with pytest.raises(ValueError, match="one token span per row"):
        word_spans(seg, lo[:2], hi[:2])


def test_prepare_boxes_rounds_outward_clips_rescales_and_pads():
    from medmoe_amd.ground import prepare_boxes
    b = torch.tensor([[[10.2, 5.0, 20.1, 9.9], [-3.0, -2.0, 4.5, 300.0], [7.0, 7.0, 7.0, 9.0]]])
    out = prepare_boxes(b, (100, 50), num_boxes=4)
    assert out.dtype == torch.int32 and tuple(out.shape) == (1, 4, 4) and out.is_contiguous()
    assert out[0].tolist() == [[10, 5, 21, 10], [0, 0, 5, 100], [0, 0, 0, 0], [0, 0, 0, 0]]       # outward; clipped; empty stays absent; padding
    assert prepare_boxes(torch.tensor([[10, 5, 10, 5]]), (100, 50), xywh=True)[0].tolist() == [[10, 5, 20, 10]]
    # from a 1024 x 2048 annotation frame to 224 x 224: scaled by 224 / 1024 down and 224 / 2048 across, then rounded outward
    r = prepare_boxes(torch.tensor([[[100, 100, 300, 500]]]), (224, 224), from_size=(1024, 2048))
    assert r[0, 0].tolist() == [int(np.floor(100 * 224 / 2048)), int(np.floor(100 * 224 / 1024)), int(np.ceil(300 * 224 / 2048)), int(np.ceil(500 * 224 / 1024))]
    assert prepare_boxes(torch.tensor([[[0.4, 0.4, 0.6, 0.6]]]), (8, 8))[0, 0].tolist() == [0, 0, 1, 1]     # a sliver keeps a pixel
    with pytest.raises(ValueError, match="num_boxes"):
        prepare_boxes(b, (100, 50), num_boxes=2)
    with pytest.raises(ValueError, match="num_boxes"):
        prepare_boxes(torch.zeros(1, 9, 4), (100, 50))
    with pytest.raises(ValueError, match=r"\[B, NB, 4\]"):
        prepare_boxes(torch.zeros(4), (100, 50))


def test_synthetic_boxes_are_seeded_and_leave_the_other_entries_alone():
    from src.data.components.unimed import SyntheticUnimed, collate_fn
    from src.data.unimed_datamodule import UnimedDataModule
    kw = dict(n=8, max_len=16, vocab=97, n_classes=5, seed=7, min_side=20, max_side=30)
    plain, box, again = SyntheticUnimed(**kw), SyntheticUnimed(boxes={"num_boxes": 3, "size": 64}, **kw), SyntheticUnimed(boxes={"num_boxes": 3, "size": 64}, **kw)
    both = SyntheticUnimed(boxes={"num_boxes": 3, "size": 64}, masks={"num_classes": 2, "size": 32}, **kw)
    absent = 0
    for i in range(8):
        a, b, c, d = plain[i], box[i], again[i], both[i]
        assert len(a) == 3 and len(b) == 4 and len(d) == 5
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]          # image, caption, class: bit-identical
        assert sorted(b[3]) == ["box", "span"] and all(torch.equal(b[3][k], c[3][k]) and torch.equal(b[3][k], d[4][k]) for k in b[3])
        bx, sp = b[3]["box"], b[3]["span"]
        assert bx.dtype == torch.int32 and tuple(bx.shape) == (3, 4) and sp.dtype == torch.int64 and tuple(sp.shape) == (2,)
        assert bx[0, 2] > bx[0, 0] and bx[0, 3] > bx[0, 1] and int(bx.min()) >= 0 and int(bx.max()) <= 64
        n_tok = int((a[1] != 0).sum())
        assert 0 <= int(sp[0]) < int(sp[1]) <= n_tok - 2
        absent += int((bx[1:, 2] <= bx[1:, 0]).sum())
    assert 0 < absent < 16 and not torch.equal(box[0][3]["box"], box[1][3]["box"])
    cb, cs, cd = collate_fn([plain[i] for i in range(4)]), collate_fn([box[i] for i in range(4)]), collate_fn([both[i] for i in range(4)])
    assert sorted(cb) == ["caption", "image", "label"] and sorted(cs) == ["box", "caption", "image", "label", "span"]
    assert sorted(cd) == ["box", "caption", "image", "label", "mask", "span"] and tuple(cd["mask"].shape) == (4, 2, 32, 32)
    assert tuple(cs["box"].shape) == (4, 3, 4) and tuple(cs["span"].shape) == (4, 2) and torch.equal(cb["label"], cs["label"])
    dkw = dict(batch_size=4, synthetic_size=8, max_len=16, synthetic_vocab=97)
    b0 = next(iter(UnimedDataModule(**dkw).train_dataloader()))
    b1 = next(iter(UnimedDataModule(boxes={"num_boxes": 1, "size": 24}, **dkw).train_dataloader()))
    assert sorted(b0) == ["caption", "image", "label"] and sorted(b1) == ["box", "caption", "image", "label", "span"]
    assert all(torch.equal(x, y) for x, y in zip(b0["image"], b1["image"])) and all(torch.equal(x, y) for x, y in zip(b0["caption"], b1["caption"]))
    dev = UnimedDataModule._with_captions(torch.zeros(4, 3, 8, 8), b1, "cpu")
    assert torch.equal(dev["box"], b1["box"]) and torch.equal(dev["span"], b1["span"])
    assert "box" not in UnimedDataModule._with_captions(torch.zeros(4, 3, 8, 8), b0, "cpu")
    with pytest.raises(KeyError, match="sizes"):
        SyntheticUnimed(boxes={"sizes": 3})
    with pytest.raises(ValueError, match="num_boxes"):
        SyntheticUnimed(boxes={"num_boxes": 9})
    with pytest.raises(NotImplementedError, match="data.boxes with data.transformations"):
        UnimedDataModule(boxes={"num_boxes": 1}, transformations={"imsize": 256}, **dkw)


def test_the_experiment_composes_and_the_block_is_validated(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from src.models.medmoe_module import MedMoEPretrainingLightningModule as M
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_grounding", "data=unimed_boxes", "model.grounding.mode=cosine",
                                          "model.grounding.thetas=[0.3,0.5]"])
    assert cfg.model.fused_step is True and cfg.model.model.vision.arch == "vit_b16" and dict(cfg.data.boxes) == {"num_boxes": 2, "size": 224}
    blk = dict(cfg.model.grounding)
    assert blk["mode"] == "cosine" and list(blk["thetas"]) == [0.3, 0.5] and blk["size"] is None and blk["span_key"] == "span" and blk["box_key"] == "box"
    loss = {"local_loss": None, "global_loss": None}
    with pytest.raises(KeyError, match=r"model.grounding: unknown keys \['theta'\] \(mode, thetas, size, span_key, box_key\)"):
        M(torch.nn.Identity(), loss, grounding={"theta": 0.5})
    with pytest.raises(NotImplementedError, match="model.grounding needs fused_step=true"):
        M(torch.nn.Identity(), loss, grounding={"mode": "attention"})

    # the block's own checks, on stand-ins for a module in fused mode: the Swin model, a width mismatch, the values
    from types import SimpleNamespace as NS
    block = lambda model, blk: M._grounding_block(NS(model=model, fused_step=True), blk)
    with pytest.raises(NotImplementedError, match="swin_t"):
        block(NS(swin=object()), {"mode": "attention"})
    with pytest.raises(NotImplementedError, match="d_t = 128 against regions of d_out = 64"):
        block(NS(engine=NS(cfg=NS(d_t=128, d_out=64))), {"mode": "attention"})
    plain = NS(engine=NS(cfg=NS(d_t=64, d_out=64)))
    with pytest.raises(ValueError, match="mode must be one of"):
        block(plain, {"mode": "softmax"})
    with pytest.raises(ValueError, match="thetas must hold 1 .. 4"):
        block(plain, {"thetas": [0.1, 0.2, 0.3, 0.4, 0.5]})
    with pytest.raises(ValueError, match="size must be a side"):
        block(plain, {"size": [1, 2, 3]})
    assert block(plain, None) is None
    assert block(plain, {"size": 96, "thetas": 0.25}) == {"mode": "attention", "thetas": (0.25,), "size": (96, 96), "span_key": "span", "box_key": "box"}
    # the pretraining experiment without the block is what it was
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert "grounding" not in dict(base.model) and "boxes" not in dict(base.data)
