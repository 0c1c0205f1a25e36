"""Variable-length pass of the trainable text tower, host side (no GPU): the switch (config key, Hydra key, environment), the
refusal with attention dropout, the header, and the engine's launch sequence in packed mode against a stub library that computes nothing."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")

NEW_SYMBOLS = ("medmoe_attn_bwd_varlen", "medmoe_layernorm_bwd_rows", "medmoe_text_aggregate_bwd_packed", "medmoe_text_embed_ln_bwd_packed",
               "medmoe_lora_fwd_rows", "medmoe_lora_bwd_dx_rows", "medmoe_lora_bwd_wgrad_rows")


def _cfg(**kw):
    from medmoe_amd.config import config_by_name
    c = config_by_name("tiny2")
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_default_is_off_and_the_key_validates():
    from medmoe_amd.config import MedMoEConfig
    assert MedMoEConfig().text_train_varlen is False
    _cfg(freeze_text=False, text_train_varlen=True).validate()
    _cfg(text_lora=True, text_train_varlen=True, text_lora_dropout=0.1, text_hidden_dropout=0.1).validate()
    _cfg(text_train_varlen=True).validate()                          # a frozen tower ignores the key


def test_validate_refuses_attention_dropout_and_names_both_keys():
    with pytest.raises(NotImplementedError, match="text_train_varlen.*text_attn_dropout"):
        _cfg(freeze_text=False, text_train_varlen=True, text_attn_dropout=0.1).validate()
    _cfg(freeze_text=False, text_train_varlen=False, text_attn_dropout=0.1).validate()


def test_hydra_key_reaches_the_config():
    from src.models.components.med_moe import config_from_hydra
    vision = {"config_name": "tiny2"}
    assert config_from_hydra(vision, {"freeze_bert": False}).text_train_varlen is False
    c = config_from_hydra(vision, {"freeze_bert": False, "train_varlen": True})
    assert c.text_train_varlen is True and not c.freeze_text
    c.validate()
    with pytest.raises(NotImplementedError, match="text_train_varlen.*text_attn_dropout"):
        config_from_hydra(vision, {"freeze_bert": False, "train_varlen": True, "attention_probs_dropout_prob": 0.1}).validate()


def test_the_model_yaml_carries_the_key_switched_off(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from src.models.components.med_moe import config_from_hydra
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert cfg.model.model.text.train_varlen is False
    assert config_from_hydra(cfg.model.model.vision, cfg.model.model.text).text_train_varlen is False
    on = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_lora", "model.model.text.train_varlen=true"])
    assert config_from_hydra(on.model.model.vision, on.model.model.text).text_train_varlen is True


def test_header_declares_every_new_symbol():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    from medmoe_amd import ops
    for name in NEW_SYMBOLS:
        m = re.search(r"^int %s\((.*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(ops._SIGS[name[len("medmoe_"):]]) + 1, name          # + the stream


# ------------------------------------------------------------------------------------------------------------------------------------------
# the engine's launch sequence against a stub library (as tests/test_host_logic.py runs the other modes)
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


def _batch():
    import medmoe_oracle as O
    return O.synthetic_batch(O.config_by_name("tiny2"), 8, min_len=4)


def _launches(stub):
    return [x for x in stub.calls if not x.endswith("_scratch")]     # scratch sizes are host queries, not launches


def test_env_switch_and_engine_refusal(stub, monkeypatch):
    from medmoe_amd.engine import Engine
    assert not Engine(_cfg(freeze_text=False), "cpu").text_train_varlen
    assert Engine(_cfg(freeze_text=False, text_train_varlen=True), "cpu").text_train_varlen
    monkeypatch.setenv("MEDMOE_TEXT_TRAIN_VARLEN", "1")
    eng = Engine(_cfg(freeze_text=False), "cpu")
    assert eng.text_train_varlen and not eng.text_train_varlen_active
    assert not Engine(_cfg(), "cpu").text_train_varlen               # nothing trains: the frozen tower's own switch (text_varlen) is the one that acts
    with pytest.raises(NotImplementedError, match="text_train_varlen.*text_attn_dropout"):
        Engine(_cfg(freeze_text=False, text_attn_dropout=0.1), "cpu")


def test_full_tower_launch_sequence_packed_and_padded(stub):
    """Packed: one text_pack, every text GEMM / LayerNorm / attention / weight-gradient launch in its device-row-count form, none in the padded
    one.  Switch off: none of the new symbols, and the text launches of a step are the padded ones."""
    from medmoe_amd.engine import Engine
    batch = _batch()
    for packed in (True, False):
        cfg = _cfg(freeze_text=False, text_train_varlen=packed, text_hidden_dropout=0.1)
        eng = Engine(cfg, "cpu")
        Lv, Lt = cfg.n_layer_v, cfg.n_layer_t
        del stub.calls[:]
        out = eng.train_step(batch)
        n = _launches(stub)
        assert set(out) >= {"loss", "l_loss", "g_loss"} and eng.text_train_varlen_active == packed and eng.dropout_step == 1
        if not packed:
            assert not set(n) & set(NEW_SYMBOLS) and not {"medmoe_text_pack", "medmoe_gemm_nt_rows", "medmoe_attn_fwd_varlen"} & set(n)
            assert n.count("medmoe_attn_bwd") == Lv + Lt and n.count("medmoe_text_embed_ln_bwd") == 1
            continue
        assert n.count("medmoe_text_pack") == 1 and n.count("medmoe_text_embed_ln_packed") == 1 and n.count("medmoe_text_embed_ln") == 0
        assert n.count("medmoe_gemm_nt_rows") == 4 * Lt + 4 * Lt                    # forward + the dgrad GEMMs
        assert n.count("medmoe_attn_fwd_varlen") == Lt and n.count("medmoe_attn_bwd_varlen") == Lt and n.count("medmoe_attn_bwd") == Lv
        assert n.count("medmoe_layernorm_bwd_rows") == 2 * Lt and n.count("medmoe_layernorm_bwd") == 2 * Lv + 1
        assert n.count("medmoe_text_aggregate_packed") == 1 and n.count("medmoe_text_aggregate") == 0
        assert n.count("medmoe_text_aggregate_bwd_packed") == 1 and n.count("medmoe_text_aggregate_bwd") == 0
        assert n.count("medmoe_text_embed_ln_bwd_packed") == 1 and n.count("medmoe_text_embed_ln_bwd") == 0
        assert n.count("medmoe_gemm_tn") == 4 * Lv + 1 + 8 + 1 + 4 * Lt             # the image side's and one per text Linear
        assert n.count("medmoe_dropout_add_layernorm_fwd") == 2 * Lt                # hidden dropout keeps its launches
        del stub.calls[:]
        eng.eval_step(batch)                                                        # evaluation of a trainable tower takes the packed pass too
        n = _launches(stub)
        assert n.count("medmoe_text_pack") == 1 and n.count("medmoe_attn_fwd_varlen") == Lt and n.count("medmoe_dropout_apply") == 0
        assert eng.dropout_step == 1


def test_lora_launch_sequence_packed(stub):
    from medmoe_amd.engine import Engine
    cfg = _cfg(text_lora=True, text_lora_r=8, text_lora_dropout=0.1, text_hidden_dropout=0.1, text_train_varlen=True)
    eng = Engine(cfg, "cpu")
    Lv, Lt = cfg.n_layer_v, cfg.n_layer_t
    del stub.calls[:]
    eng.train_step(_batch())
    n = _launches(stub)
    assert eng.text_train_varlen_active
    for name in ("medmoe_lora_fwd", "medmoe_lora_bwd_dx", "medmoe_lora_bwd_wgrad"):
        assert n.count(name) == 0 and n.count(name + "_rows") == Lt, name
    assert n.count("medmoe_gemm_tn") == 4 * Lv + 1 + 8 + 1                          # no base weight gradient
    assert n.count("medmoe_layernorm_bwd_rows") == 2 * Lt and n.count("medmoe_attn_bwd_varlen") == Lt
    assert n.count("medmoe_text_embed_ln_bwd_packed") == 0 and n.count("medmoe_text_aggregate_bwd_packed") == 1
