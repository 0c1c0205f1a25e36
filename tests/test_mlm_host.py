"""Host side of the masked-language-model objective: configuration and its refusals, the Hydra keys, the head arena's layout and
parameter groups, the `src.losses` surface, and the mask rule restated on the Philox of tests/test_text_dropout_host.py (mlm_reference)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import mlm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
ENTRIES = ("medmoe_mlm_mask", "medmoe_rows_gather", "medmoe_rows_scatter_add", "medmoe_rows_mul", "medmoe_vocab_ce_fwd", "medmoe_vocab_ce_scratch",
           "medmoe_vocab_ce_bwd_dx", "medmoe_vocab_ce_bwd_dw")


def _mlm_cfg(**kw):
    from medmoe_amd.config import config_by_name
    c = config_by_name("tiny")
    c.freeze_text, c.text_mlm, c.mlm_mask_id = False, True, 4
    for k, v in kw.items():
        setattr(c, k, v)
    return c


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
    src = open(os.path.join(ROOT, "medmoe_amd", "csrc", "mlm.hip")).read()
    assert "atomic" not in src.replace("no atomics", "")                                        # scan and single owners: none at all
    phil = open(os.path.join(ROOT, "medmoe_amd", "csrc", "philox.h")).read()
    assert "#define DROPOUT_SITE_MLM 0x60000000u" in phil and ops.DROPOUT_SITE_MLM == R.SITE_MLM == 0x60000000
    lib.medmoe_vocab_ce_scratch.restype = ctypes.c_longlong
    assert lib.medmoe_vocab_ce_scratch(81920, 28996, 768) == (2 * 114 + 2) * 81920
    assert lib.medmoe_vocab_ce_scratch(8, 97, 96) == 0 and lib.medmoe_vocab_ce_scratch(8, 1, 64) == 0 and lib.medmoe_vocab_ce_scratch(8, 97, 1088) == 0


def test_wrappers_refuse_bad_arguments_before_any_launch():
    """CPU tensors: a call that got through the checks would raise the "GPU" RuntimeError instead"""
    from medmoe_amd import ops
    ids, attn = torch.zeros(2, 4, dtype=torch.int32), torch.ones(2, 4, dtype=torch.uint8)
    kw = dict(cls_id=1, sep_id=2, pad_id=0, mask_id=4, vocab=97, seed=0, step=0, p=0.15)
    with pytest.raises(TypeError):
        ops.mlm_mask(ids.long(), attn, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.mlm_mask(ids, attn, **kw)
    z, E, b = torch.zeros(4, 96, dtype=torch.bfloat16), torch.zeros(8, 96, dtype=torch.bfloat16), torch.zeros(8)
    with pytest.raises(TypeError):
        ops.vocab_ce_fwd(z.float(), E, b, ids.view(-1), ids.view(-1)[:1])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vocab_ce_fwd(z, E, b, ids.view(-1), ids.view(-1)[:1])


# ------------------------------------------------------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_off_and_validate_names_what_it_refuses():
    from medmoe_amd.config import MedMoEConfig
    c = MedMoEConfig()
    assert (c.text_mlm, c.mlm_prob, c.mlm_weight, c.mlm_mask_id) == (False, 0.15, 1.0, 103)
    c.mlm_prob, c.mlm_mask_id = 7.0, -1                               # not looked at while the objective is off
    c.validate()
    _mlm_cfg().validate()
    with pytest.raises(ValueError, match="text_mlm.*freeze_text"):
        _mlm_cfg(freeze_text=True).validate()
    with pytest.raises(ValueError, match="text_mlm.*text_lora"):
        _mlm_cfg(freeze_text=True, text_lora=True).validate()
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="mlm_prob"):
            _mlm_cfg(mlm_prob=bad).validate()
    for bad in (-1, 97, 103):
        with pytest.raises(ValueError, match="mlm_mask_id"):
            _mlm_cfg(mlm_mask_id=bad).validate()
    with pytest.raises(ValueError, match="mlm_weight"):
        _mlm_cfg(mlm_weight=0.0).validate()
    with pytest.raises(NotImplementedError, match="deterministic"):
        _mlm_cfg(deterministic=True).validate()


def test_refused_with_the_captured_graph_step_and_the_swin_engine(monkeypatch):
    from medmoe_amd.engine import Engine
    from medmoe_amd.swin_engine import SwinEngine
    monkeypatch.setenv("MEDMOE_GRAPH", "1")
    with pytest.raises(NotImplementedError, match="text_mlm.*MEDMOE_GRAPH"):
        Engine(_mlm_cfg(), "cpu")
    monkeypatch.delenv("MEDMOE_GRAPH")
    eng = types.SimpleNamespace(cfg=_mlm_cfg(), dist=False, deterministic=False)
    with pytest.raises(NotImplementedError, match="text_mlm.*swin_t"):
        SwinEngine(eng, None)


def test_hydra_keys_reach_the_module():
    from medmoe_amd.hydra_lite import compose, locate
    from src.models.medmoe_module import MedMoEPretrainingLightningModule as Mod
    os.environ.setdefault("PROJECT_ROOT", ROOT)
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_mlm"])
    m = cfg.model
    assert dict(m.mlm) == {"weight": 1.0, "prob": 0.15, "mask_token_id": 103, "validate": True}
    assert m.fused_step is True and m.model.text.freeze_bert is False and m.model.vision.arch == "vit_b16" and cfg.data.batch_size == 1024
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2", "model.model.text.freeze_bert=false", "+model.mlm.weight=0.5",
                                          "+model.mlm.prob=0.2", "+model.mlm.mask_token_id=4"])
    assert dict(cfg.model.mlm) == {"weight": 0.5, "prob": 0.2, "mask_token_id": 4}
    assert "mlm" not in dict(compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"]).model)       # off: the key does not exist
    assert locate(cfg.model._target_) is Mod
    with pytest.raises(KeyError, match="model.mlm: unknown keys"):
        Mod(model=types.SimpleNamespace(), loss={}, mlm={"probability": 0.15})
    with pytest.raises(NotImplementedError, match="model.mlm needs fused_step"):
        Mod(model=types.SimpleNamespace(), loss={}, mlm={"prob": 0.15})
    with pytest.raises(NotImplementedError, match="model.mlm with vision.arch = swin_t"):
        Mod(model=types.SimpleNamespace(swin=object()), loss={}, mlm={"prob": 0.15}, fused_step=True)


def test_losses_classes_resolve_by_target_with_the_reference_surface():
    from medmoe_amd.hydra_lite import instantiate, locate
    import src.losses as L
    assert locate("src.losses.MaskedPredictionLoss") is L.MaskedPredictionLoss and locate("src.losses.MaskedPredictionHead") is L.MaskedPredictionHead
    m = instantiate({"_target_": "src.losses.MaskedPredictionLoss", "hidden_size": 64, "vocab_size": 97, "ignore_index": -1, "ignore_nan": True})
    assert sorted(n for n, _ in m.named_parameters()) == ["cls.bias", "cls.decoder.weight", "cls.dense.bias", "cls.dense.weight",
                                                          "cls.layer_norm.bias", "cls.layer_norm.weight"]
    assert tuple(m.cls.decoder.weight.shape) == (97, 64) and m.cls.decoder.bias is None and m.cls.layer_norm.eps == 1e-5
    assert (m.ignore_index, m.vocab_size, m.ignore_nan) == (-1, 97, True)
    with pytest.raises(RuntimeError, match="GPU"):                    # no CPU fallback
        m(torch.zeros(1, 2, 64), torch.tensor([[3, -1]]))
    with pytest.raises(ValueError, match="masked labels"):
        m(torch.zeros(1, 2, 64))
    with pytest.raises(NotImplementedError, match="GELU"):
        L.MaskedPredictionHead(64, 97, transform_act_fn=torch.relu)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the head's arena
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_head_arena_layout_and_parameter_groups():
    from medmoe_amd.flat import FlatArena
    from medmoe_amd.mlm import HEAD_NAMES, head_entries, init_head
    from medmoe_amd.optim_groups import GroupRules, build_assign
    D, V = 128, 97
    ent = head_entries(D, V)
    assert tuple(n for n, _ in ent) == HEAD_NAMES and "cls.decoder.weight" not in HEAD_NAMES           # the tied table is the tower's
    a = FlatArena("cpu", ent, gemm=[("cls.dense.weight", False)])
    assert a.offsets == {"cls.dense.weight": 0, "cls.dense.bias": D * D, "cls.layer_norm.weight": D * D + D, "cls.layer_norm.bias": D * D + 2 * D,
                         "cls.bias": D * D + 3 * D}
    assert a.numel == D * D + 3 * D + 104 and a.numel % 8 == 0 and a.train_from == 0                       # 97 -> 104: padded to 8
    assert tuple(a.w16t("cls.dense.weight").shape) == (D, D) and a.tr_table.shape[0] == 1
    init = init_head(D, V, seed=3)
    assert {k: tuple(v.shape) for k, v in init.items()} == {n: s for n, s in ent}
    assert float(init["cls.layer_norm.weight"].min()) == 1.0 and not init["cls.bias"].any() and 0.015 < float(init["cls.dense.weight"].std()) < 0.025
    assert torch.equal(init["cls.dense.weight"], init_head(D, V, seed=3)["cls.dense.weight"])
    # no_decay_1d: everything but the dense matrix is a bias or a LayerNorm; the head sits behind the tower (layer_decay multiplier 1)
    assign = build_assign({"mlm": a}, GroupRules(no_decay_1d=True, layer_decay=0.5))["mlm"]
    assert assign == {n: (1.0, 0.0) for n in HEAD_NAMES if n != "cls.dense.weight"}
    assert build_assign({"mlm": a}, GroupRules(no_decay=("cls.bias",)))["mlm"] == {"cls.bias": (1.0, 0.0)}


# ------------------------------------------------------------------------------------------------------------------------------------------
# the mask rule
# ------------------------------------------------------------------------------------------------------------------------------------------
IDS = dict(cls_id=1, sep_id=2, pad_id=0, mask_id=4)


def _batch(B, T, V, seed):
    g = np.random.default_rng(seed)
    ids = g.integers(5, V, size=(B, T))
    attn = np.ones((B, T), np.uint8)
    for b in range(B):
        n = int(g.integers(3, T + 1))
        ids[b, 0], ids[b, n - 1] = IDS["cls_id"], IDS["sep_id"]
        ids[b, n:], attn[b, n:] = IDS["pad_id"], 0
    return ids, attn


def test_philox_of_the_restatement_gives_the_known_answers():
    assert [int(v) for v in R.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert [int(v) for v in R.philox4x32_10(f, f, f, f, f, f)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert (R.T80, R.T90) == (3435973836, 3865470566)


def test_mask_rule_selects_candidates_only_and_is_a_function_of_the_global_token():
    B, T, V = 16, 20, 97
    ids, attn = _batch(B, T, V, 0)
    kw = dict(vocab=V, seed=(7 << 32) + 5, step=3, p=0.3, **IDS)
    m = R.mlm_mask_ref(ids, attn, **kw)
    sel = m["labels"] >= 0
    special = (attn == 0) | np.isin(ids, (IDS["cls_id"], IDS["sep_id"], IDS["pad_id"]))
    assert sel.any() and not (sel & special).any() and m["count"] == int(sel.sum())
    assert np.array_equal(m["labels"][sel], ids[sel]) and np.array_equal(m["ids_masked"][~sel], ids[~sel])
    assert (np.diff(m["rows"]) > 0).all() and np.array_equal(m["row_labels"], ids.reshape(-1)[m["rows"]])
    assert (m["ids_masked"][m["action"] == 0] == IDS["mask_id"]).all() and np.array_equal(m["ids_masked"][m["action"] == 2], ids[m["action"] == 2])
    # rank 1 of two ranks (its first global sample is 8) draws what the one-process batch draws for samples 8..15
    half = R.mlm_mask_ref(ids[8:], attn[8:], sample_offset=8, **kw)
    assert np.array_equal(half["labels"], m["labels"][8:]) and np.array_equal(half["ids_masked"], m["ids_masked"][8:])
    # every input moves the draw
    for other in (dict(kw, seed=kw["seed"] + 1), dict(kw, seed=kw["seed"] + (1 << 32)), dict(kw, step=4)):
        assert not np.array_equal(R.mlm_mask_ref(ids, attn, **other)["labels"], m["labels"])
    # packed rows: the same tokens under the packed numbering
    tok_row = np.where(attn.reshape(-1) != 0, np.cumsum(attn.reshape(-1) != 0) - 1, -1)
    pk = R.mlm_mask_ref(ids, attn, tok_row=tok_row, **kw)
    assert np.array_equal(pk["rows"], tok_row[m["rows"]]) and (np.diff(pk["rows"]) > 0).all() and np.array_equal(pk["row_labels"], m["row_labels"])


@pytest.mark.parametrize("p", [0.15, 0.5])
def test_mask_rule_rates_lie_within_four_sigma(p):
    n, V = 5120, 28996
    ids = np.random.default_rng(1).integers(5, V, size=(64, 80))
    m = R.mlm_mask_ref(ids, np.ones_like(ids), vocab=V, seed=77, step=1, p=p, **IDS)
    k = m["count"]
    assert abs(k / n - p) <= 4 * (p * (1 - p) / n) ** 0.5
    for action, q in ((0, 0.8), (1, 0.1), (2, 0.1)):
        assert abs(float((m["action"] == action).sum()) / k - q) <= 4 * (q * (1 - q) / k) ** 0.5
    rand = m["ids_masked"][m["action"] == 1]
    assert rand.min() >= 0 and rand.max() < V
