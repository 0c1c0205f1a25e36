"""Stochastic depth of the ViT tower, host side (no GPU): the config field and its rates, the Hydra key for both towers, the
refusals, the header, and the engine's launch sequence against a stub library that computes nothing (the pattern of
tests/test_text_varlen_train_host.py)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("medmoe_drop_path_scales", "medmoe_scale_add_layernorm_fwd")


def _cfg(**kw):
    from medmoe_amd.config import config_by_name
    c = config_by_name("tiny2")
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ------------------------------------------------------------------------------------------------------------------------------------------
# config, Hydra
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_default_is_off_and_the_rates_are_the_reference_linspace():
    from medmoe_amd.config import MedMoEConfig, config_by_name
    assert MedMoEConfig().vit_drop_path == 0.0
    assert MedMoEConfig().vit_drop_path_rates() == [0.0] * 12
    for name, r in (("tiny2", 0.5), ("cfg2", 0.1), ("cfg4_bf16", 0.3)):
        c = config_by_name(name)
        c.vit_drop_path = r
        c.validate()
        want = [x.item() for x in torch.linspace(0, r, c.n_layer_v)]              # transformer.py:192
        assert c.vit_drop_path_rates() == want and want[0] == 0.0 and abs(want[-1] - r) < 1e-7
    one = _cfg(n_layer_v=1, vit_drop_path=0.4)
    assert one.vit_drop_path_rates() == [0.0]                                     # a single layer never drops


@pytest.mark.parametrize("bad", [-0.1, 1.0])
def test_validate_rejects_rates_outside_the_unit_interval(bad):
    with pytest.raises(ValueError, match="vit_drop_path"):
        _cfg(vit_drop_path=bad).validate()


def test_hydra_key_reaches_the_config_and_an_absent_key_changes_nothing():
    import dataclasses
    from src.models.components.med_moe import config_from_hydra
    for vision in ({"config_name": "tiny2"}, {"arch": "vit_b16", "num_experts": 8, "top_k": 2}):
        base = config_from_hydra(dict(vision), {})
        assert base.vit_drop_path == 0.0
        on = config_from_hydra(dict(vision, drop_path_rate=0.1), {})
        assert on.vit_drop_path == 0.1
        on.validate()
        on.vit_drop_path = 0.0
        assert dataclasses.asdict(on) == dataclasses.asdict(base)
    with pytest.raises(ValueError, match="vit_drop_path"):
        config_from_hydra({"config_name": "tiny2", "drop_path_rate": 1.5}, {}).validate()
    # the Swin tower's key is the module's, not the placeholder ViT's
    assert config_from_hydra({"arch": "swin_t", "drop_path_rate": 0.2}, {}).vit_drop_path == 0.0


def test_the_model_yaml_composes_to_rate_zero_and_the_override_arrives(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from src.models.components.med_moe import config_from_hydra
    cfg = compose(os.path.join(ROOT, "configs"), "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert config_from_hydra(cfg.model.model.vision, cfg.model.model.text).vit_drop_path == 0.0
    on = compose(os.path.join(ROOT, "configs"), "train.yaml", ["experiment=pretraining_medmoe_cfg2", "+model.model.vision.drop_path_rate=0.1"])
    assert config_from_hydra(on.model.model.vision, on.model.model.text).vit_drop_path == 0.1


def test_header_declares_the_new_symbols_and_the_site_constant():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    from medmoe_amd import ops
    for name in NEW_SYMBOLS:
        m = re.search(r"^int %s\((.*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(ops._SIGS[name[len("medmoe_"):]]) + 1, name          # + the stream
    assert ops.DROPOUT_SITE_VIT_DROP_PATH == 0x40000000
    phil = open(os.path.join(ROOT, "medmoe_amd", "csrc", "philox.h")).read()
    assert re.search(r"#define DROPOUT_SITE_VIT_DROP_PATH 0x40000000u", phil)
    # disjoint from the text sites 4 l + {0..3} of any tower this build runs and from the embedding site
    assert ops.DROPOUT_SITE_VIT_DROP_PATH > 4 * 4096 and ops.DROPOUT_SITE_VIT_DROP_PATH + 2 * 4096 < ops.DROPOUT_SITE_EMBED


# ------------------------------------------------------------------------------------------------------------------------------------------
# the stub library
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
    return [x for x in stub.calls if not x.endswith("_scratch")]


def test_graph_mode_is_refused_and_names_both_keys(stub, monkeypatch):
    from medmoe_amd.engine import Engine
    monkeypatch.setenv("MEDMOE_GRAPH", "1")
    Engine(_cfg(), "cpu")                                                         # rate 0: graphs as before
    with pytest.raises(NotImplementedError, match=r"vit_drop_path.*model\.model\.vision\.drop_path_rate.*MEDMOE_GRAPH=1"):
        Engine(_cfg(vit_drop_path=0.1), "cpu")


def test_non_fused_training_is_refused_and_evaluation_is_not(stub):
    """MedMoE.encode_image with grad enabled in train mode and a positive rate: NotImplementedError naming the config field, the Hydra key and
    the fused step; in eval mode (or under no_grad) the check lets the call through."""
    from src.models.components import med_moe as M

    class Reached(Exception):
        pass

    m = M.MedMoE.__new__(M.MedMoE)
    torch.nn.Module.__init__(m)
    m.swin, m.cfg = None, _cfg(vit_drop_path=0.1)

    def reached():
        raise Reached()
    m.refresh_working_copies = reached                                            # the first thing encode_image does after the check
    x = torch.zeros(2, 3, 64, 64)
    m.train()
    with pytest.raises(NotImplementedError, match=r"vit_drop_path.*model\.model\.vision\.drop_path_rate.*model\.fused_step=true"):
        m.encode_image(x)
    with torch.no_grad(), pytest.raises(Reached):
        m.encode_image(x)
    m.eval()
    with pytest.raises(Reached):
        m.encode_image(x)
    m.train()
    m.cfg = _cfg()
    with pytest.raises(Reached):                                                  # rate 0 trains through the mirror as before
        m.encode_image(x)


def test_swin_arch_takes_the_key_for_its_own_tower(stub, monkeypatch):
    """vision.arch = swin_t: the key sets MedMoE.swin.drop_path_rate; absent leaves the module's 0.1."""
    from src.models.components import med_moe as M
    from src.models.components import swin as S

    class FakeSwin(torch.nn.Module):
        def __init__(self, num_experts, state_dict=None):
            super().__init__()
            self.drop_path_rate = 0.1
    monkeypatch.setattr(S, "SWIN", FakeSwin)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)

    class FakeEngine:
        def __init__(self, cfg, device):
            self.cfg = cfg
            self.params = type("P", (), {"p32": torch.zeros(8)})()
    monkeypatch.setattr(M, "Engine", FakeEngine)
    monkeypatch.setattr(FakeSwin, "to", lambda self, dev: self)
    base = M.MedMoE({"arch": "swin_t", "num_experts": 4}, {})
    assert base.swin.drop_path_rate == 0.1 and base.cfg.vit_drop_path == 0.0
    on = M.MedMoE({"arch": "swin_t", "num_experts": 4, "drop_path_rate": 0.25}, {})
    assert on.swin.drop_path_rate == 0.25 and on.cfg.vit_drop_path == 0.0
    off = M.MedMoE({"arch": "swin_t", "num_experts": 4, "drop_path_rate": 0.0}, {})
    assert off.swin.drop_path_rate == 0.0
    with pytest.raises(ValueError, match="drop_path_rate"):
        M.MedMoE({"arch": "swin_t", "num_experts": 4, "drop_path_rate": 1.0}, {})


def test_wrappers_refuse_bad_shapes(stub):
    from medmoe_amd import ops
    BF, F32 = torch.bfloat16, torch.float32

    def args(rows, D, n_scale, rps):
        t = lambda: torch.zeros(rows, D, dtype=BF)
        return (t(), t(), torch.ones(n_scale), rps, torch.ones(D), torch.zeros(D), t(), t(), torch.zeros(rows), torch.zeros(rows), 1e-6)
    ops.scale_add_layernorm_fwd(*args(34, 128, 2, 17))
    assert stub.calls.count("medmoe_scale_add_layernorm_fwd") == 1
    for a in (args(34, 132, 2, 17), args(34, 2056, 2, 17), args(34, 128, 3, 17), args(34, 128, 2, 16)):
        with pytest.raises(ValueError, match="scale_add_layernorm_fwd"):
            ops.scale_add_layernorm_fwd(*a)
    assert stub.calls.count("medmoe_scale_add_layernorm_fwd") == 1
    out = torch.zeros(3, 5)
    ops.drop_path_scales(out, [0.0, 0.1, 0.2], 5, 0, 0, 0)
    for bad in (lambda: ops.drop_path_scales(out, [0.0, 0.1], 5, 0, 0, 0), lambda: ops.drop_path_scales(out, [0.0, 0.1, 1.0], 5, 0, 0, 0),
                lambda: ops.drop_path_scales(out, [0.0, 0.1, 0.2], 5, -1, 0, 0),
                lambda: ops.drop_path_scales(torch.zeros(129, 1), [0.1] * 129, 1, 0, 0, 0)):
        with pytest.raises(ValueError):
            bad()
    assert stub.calls.count("medmoe_drop_path_scales") == 1


def test_launch_sequence_with_and_without_stochastic_depth(stub):
    """Rate > 0: one medmoe_drop_path_scales, 2 (L - 1) fused scale + add + LayerNorm launches, as many backward medmoe_drop_path, and 2 (L - 1)
    stand-alone LayerNorm launches fewer; every other count unchanged.  eval_step: none of the new launches, no counter moved.  Rate 0: the
    sequence of an engine that has never heard of the key."""
    from medmoe_amd.engine import Engine
    batch = _batch()
    seq = {}
    for rate in (0.0, 0.5):
        eng = Engine(_cfg(vit_drop_path=rate), "cpu")
        del stub.calls[:]
        out = eng.train_step(batch)
        seq[rate] = _launches(stub)
        assert set(out) >= {"loss", "l_loss", "g_loss"} and eng.dropout_step == 1 and eng.vit_drop_scales is None
        del stub.calls[:]
        eng.eval_step(batch)
        n = _launches(stub)
        assert not {"medmoe_drop_path_scales", "medmoe_scale_add_layernorm_fwd", "medmoe_drop_path"} & set(n)
        assert eng.dropout_step == 1 and eng.vit_drop_scales is None
        if rate == 0.0:
            assert "vit_dp" not in eng.ws and "dp_a" not in eng.ws
    L = _cfg().n_layer_v
    off, on = seq[0.0], seq[0.5]
    plain = Engine(_cfg(), "cpu")
    del stub.calls[:]
    plain.train_step(batch)
    assert off == _launches(stub) and not {"medmoe_drop_path_scales", "medmoe_scale_add_layernorm_fwd", "medmoe_drop_path"} & set(off)
    assert on.count("medmoe_drop_path_scales") == 1
    assert on.index("medmoe_drop_path_scales") < on.index("medmoe_patchify_ld")   # ahead of the image tower
    assert on.count("medmoe_scale_add_layernorm_fwd") == 2 * (L - 1)
    assert on.count("medmoe_drop_path") == 2 * (L - 1)
    assert on.count("medmoe_layernorm_fwd") == off.count("medmoe_layernorm_fwd") - 2 * (L - 1)
    new = {"medmoe_drop_path_scales", "medmoe_scale_add_layernorm_fwd", "medmoe_drop_path", "medmoe_layernorm_fwd"}
    for name in set(off) | set(on):
        if name not in new:
            assert on.count(name) == off.count(name), name


def test_injected_scales_are_validated(stub):
    from medmoe_amd.engine import Engine
    eng = Engine(_cfg(vit_drop_path=0.5), "cpu")
    eng._alloc(8)
    eng.vit_drop_scales = torch.ones(4, 2, 7)
    with pytest.raises(ValueError, match="vit_drop_scales"):
        eng._vit_blocks(8)
    eng.vit_drop_scales = torch.ones(4, 2, 8)
    del stub.calls[:]
    eng._vit_blocks(8)
    assert stub.calls.count("medmoe_scale_add_layernorm_fwd") == 6
    off = Engine(_cfg(), "cpu")
    off._alloc(8)
    off.vit_drop_scales = torch.ones(4, 2, 8)
    with pytest.raises(RuntimeError, match="vit_drop_path = 0"):
        off._vit_blocks(8)
