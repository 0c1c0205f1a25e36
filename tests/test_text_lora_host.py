"""LoRA adapters of the text tower, host side (no GPU): configuration rules, the Hydra keys, the experiment file, the header."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")


def _cfg(**kw):
    from medmoe_amd.config import config_by_name
    c = config_by_name("tiny2")
    c.text_lora = True
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_defaults_are_off_and_a_plain_lora_config_validates():
    from medmoe_amd.config import MedMoEConfig
    c = MedMoEConfig()
    assert (c.text_lora, c.text_lora_r, c.text_lora_alpha, c.text_lora_dropout, tuple(c.text_lora_targets)) == (False, 8, 16.0, 0.0, ("query", "value"))
    c.validate()
    _cfg().validate()
    _cfg(text_lora_r=1, text_lora_targets=("value",)).validate()
    _cfg(text_lora_r=16, text_lora_targets=("query", "key", "value"), text_lora_dropout=0.5).validate()


def test_validate_rejects_what_the_adapters_are_not_built_for():
    with pytest.raises(ValueError, match="(?i)frozen"):
        _cfg(freeze_text=False).validate()
    for r in (0, 17, -1):
        with pytest.raises(ValueError, match="text_lora_r"):
            _cfg(text_lora_r=r).validate()
    for tg in ((), ("query", "query"), ("query", "output"), ("dense",)):
        with pytest.raises(ValueError, match="text_lora_targets"):
            _cfg(text_lora_targets=tg).validate()
    for p in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="text_lora_dropout"):
            _cfg(text_lora_dropout=p).validate()
    with pytest.raises(NotImplementedError, match="deterministic with text_lora.*named follow-up \\(DESIGN 3e\\)"):
        _cfg(deterministic=True).validate()


def test_hydra_keys_reach_the_config_and_absent_keys_change_nothing():
    from src.models.components.med_moe import config_from_hydra
    vision = {"config_name": "tiny2"}
    c = config_from_hydra(vision, {"freeze_bert": True})
    assert not c.text_lora and c.text_lora_dropout == 0.0 and tuple(c.text_lora_targets) == ("query", "value")
    c = config_from_hydra(vision, {"freeze_bert": True, "lora": True, "lora_r": 4, "lora_alpha": 32, "lora_dropout": 0.1,
                                   "lora_targets": ["query", "key", "value"]})
    assert c.text_lora and c.text_lora_r == 4 and c.text_lora_alpha == 32.0 and c.text_lora_dropout == 0.1
    assert tuple(c.text_lora_targets) == ("query", "key", "value")
    c.validate()
    c = config_from_hydra({"arch": "vit_b16"}, {"lora": True, "lora_targets": "value"})
    assert c.text_lora and tuple(c.text_lora_targets) == ("value",) and c.freeze_text
    with pytest.raises(ValueError, match="(?i)frozen"):
        config_from_hydra(vision, {"freeze_bert": False, "lora": True}).validate()


def test_vision_lora_is_still_rejected():
    from src.models.components.med_moe import config_from_hydra
    with pytest.raises(NotImplementedError, match="vision.lora"):
        config_from_hydra({"config_name": "tiny2", "lora": True}, {})


def test_the_lora_experiment_composes(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from src.models.components.med_moe import config_from_hydra
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_lora"])
    text = cfg.model.model.text
    assert text.freeze_bert is True and text.lora is True and text.lora_r == 8 and text.lora_alpha == 16 and text.lora_dropout == 0.1
    c = config_from_hydra(cfg.model.model.vision, text)
    c.validate()
    assert c.text_lora and c.freeze_text and c.n_expert == 8 and c.top_k == 2 and c.max_len == 77
    assert tuple(c.text_lora_targets) == ("query", "value")
    # cfg2 itself is unchanged by the new keys
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    cb = config_from_hydra(base.model.model.vision, base.model.model.text)
    assert not cb.text_lora and cb.text_lora_dropout == 0.0


def test_header_declares_the_lora_entry_points():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    for name in ("medmoe_lora_fwd", "medmoe_lora_bwd_dx", "medmoe_lora_bwd_wgrad", "medmoe_lora_merge"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
    assert re.search(r"^long long medmoe_lora_wgrad_scratch\(", hdr, re.M)
    from medmoe_amd import ops
    for name in ("lora_fwd", "lora_bwd_dx", "lora_bwd_wgrad", "lora_merge"):
        decl = re.search(r"^int medmoe_%s\((.*)\);" % name, hdr, re.M).group(1)
        assert len(decl.split(",")) == len(ops._SIGS[name]) + 1, name          # + the stream


def test_column_offsets_follow_the_fused_row():
    from medmoe_amd import ops
    assert ops.lora_cols(("query", "value"), 768) == (0, 1536, 0)
    assert ops.lora_cols(("value",), 128) == (256, 0, 0)
    assert ops.lora_cols(("query", "key", "value"), 128) == (0, 128, 256)
    assert ops.DROPOUT_SITE_LORA == 3


# ------------------------------------------------------------------------------------------------------------------------------------------
# the engine's launch sequence in LoRA mode against a stub library that computes nothing (as tests/test_host_logic.py runs the other modes)
# ------------------------------------------------------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("medmoe_"):
            raise AttributeError(name)

        def f(*a):
            self.calls.append(name)
            if name == "medmoe_local_geometry":
                HW, T = a[0].value, a[1].value
                a[2]._obj.value = (HW + 15) // 16 * 16; a[3]._obj.value = (T + 15) // 16 * 16
                a[4]._obj.value = (((HW + 15) // 16) + 1) // 2 * 32
            if name == "medmoe_local_fast_path":
                nht, ntt = (a[0].value + 15) // 16, (a[1].value + 15) // 16
                return int((nht == 4 and ntt == 1) or (nht in (13, 16) and 1 <= ntt <= 5))
            if name == "medmoe_local_pair3_supported":
                HW, ntt = a[0].value, (a[1].value + 15) // 16
                return int((HW == 64 and ntt == 1) or (HW == 196 and 1 <= ntt <= 5))
            return 0
        return f


@pytest.fixture
def stub(monkeypatch):
    import ctypes
    import torch
    from medmoe_amd import _lib, ops
    lib = _StubLib()
    monkeypatch.setattr(_lib, "_LIB", lib)
    monkeypatch.setattr(ops, "load_library", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(ops, "_stream_handle", lambda: 0)
    for cache in ("_FN", "_NT_FN", "_TN_FN"):
        monkeypatch.setattr(ops, cache, {})
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    return lib


@pytest.mark.parametrize("targets", [("query", "value"), ("value", "key", "query")])
def test_engine_launch_sequence_in_lora_mode(stub, targets):
    """One train_step and one eval_step: per text layer one adapter forward launch, in the backward one d x and one weight-gradient launch;
    no weight-gradient GEMM, LayerNorm parameter sum or embedding backward of the base; the optimiser steps two arenas."""
    import medmoe_oracle as O
    from medmoe_amd.engine import Engine
    from medmoe_amd.text_lora import LoraStore
    cfg = _cfg(text_lora_targets=targets, text_lora_r=4, text_lora_dropout=0.1, text_hidden_dropout=0.1)
    eng = Engine(cfg, "cpu")
    Lv, Lt = cfg.n_layer_v, cfg.n_layer_t
    assert eng.train_text and eng.tstore is None and isinstance(eng.lora, LoraStore) and eng.text_arena() is eng.lora
    assert eng.lora.targets == tuple(t for t in ("query", "key", "value") if t in targets)
    assert set(eng.optimizer_stores()) == {"vit", "text"} and eng.optimizer_stores()["text"] is eng.lora
    assert len(eng._base_t) == 4 * Lt
    batch = O.synthetic_batch(O.config_by_name("tiny2"), 8, min_len=4)
    del stub.calls[:]
    out = eng.train_step(batch)
    n = [x for x in stub.calls if x != "medmoe_lora_wgrad_scratch"]                # the scratch size is a host query, not a launch
    assert set(out) >= {"loss", "l_loss", "g_loss"}
    assert n.count("medmoe_lora_fwd") == Lt and n.count("medmoe_lora_bwd_dx") == Lt and n.count("medmoe_lora_bwd_wgrad") == Lt
    assert n.count("medmoe_gemm_tn") == 4 * Lv + 1 + 8 + 1                         # the image side's only
    assert n.count("medmoe_text_embed_ln_bwd") == 0 and n.count("medmoe_text_aggregate_bwd") == 1
    assert n.count("medmoe_layernorm_bwd") == 2 * Lv + 1 + 2 * Lt
    assert n.count("medmoe_adam_step") == 2 and n.count("medmoe_sumsq_det") == 2
    assert n.count("medmoe_attn_bwd") == Lv + Lt
    # every adapter forward follows its layer's input_proj GEMM directly
    f = [i for i, x in enumerate(n) if x == "medmoe_lora_fwd"]
    assert all(n[i - 1] == "medmoe_gemm_nt" for i in f)
    # the backward's pair comes behind the layer's attention backward; at layer 0 no base dgrad GEMM sits between them
    dx = [i for i, x in enumerate(n) if x == "medmoe_lora_bwd_dx"]
    assert all(n[i + 1] == "medmoe_lora_bwd_wgrad" for i in dx)
    assert all(n[i - 1] == "medmoe_gemm_nt" and n[i - 2] == "medmoe_attn_bwd" for i in dx[:-1]) and n[dx[-1] - 1] == "medmoe_attn_bwd"
    assert eng.dropout_step == 1
    del stub.calls[:]
    eng.eval_step(batch)
    n = stub.calls
    assert n.count("medmoe_lora_fwd") == Lt and n.count("medmoe_lora_bwd_dx") == 0 and n.count("medmoe_dropout_apply") == 0
    assert eng.dropout_step == 1


def test_lora_store_layout_and_names():
    """The arena's layout needs no GPU to be checked: padded entries, per-layer concatenations, true shapes on export."""
    import torch
    from medmoe_amd import ops
    from medmoe_amd.flat import FlatArena
    cfg = _cfg(text_lora_r=4, text_lora_targets=("value", "query"))
    D, L = cfg.d_t, cfg.n_layer_t
    ar = FlatArena("cpu", [("layer.0.attention.query.lora_A", (16, D)), ("layer.0.attention.value.lora_A", (16, D))],
                   [("layer.0.lora_A", ["layer.0.attention.query.lora_A", "layer.0.attention.value.lora_A"])], [("layer.0.lora_A", False)])
    assert ar.shapes["layer.0.lora_A"] == (32, D) and ar.offsets["layer.0.attention.value.lora_A"] == 16 * D
    assert tuple(ar.w16t("layer.0.lora_A").shape) == (D, 32)
    assert ops.LORA_RANK_PAD == 16
