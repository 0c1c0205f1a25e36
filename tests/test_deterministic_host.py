"""Host side of deterministic mode (MedMoEConfig.deterministic / MEDMOE_DETERMINISTIC=1 / trainer.deterministic): the refusals, the way
from the Hydra key to the engine, and the entry points a step launches - recorded against a stub library that computes nothing (every
launch returns 0), as tests/test_host_logic.py does for the default mode."""
import ctypes
import json
import os

import pytest
import torch

import medmoe_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
GOLDEN = os.path.join(ROOT, "tests", "golden")


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
    from medmoe_amd import _lib, ops
    lib = _StubLib()
    monkeypatch.setattr(_lib, "_LIB", lib)
    monkeypatch.setattr(ops, "load_library", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(ops, "_stream_handle", lambda: 0)
    for cache in ("_FN", "_NT_FN", "_TN_FN"):                       # entry points cached per process: fresh ones for the stub library
        monkeypatch.setattr(ops, cache, {})
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    for k in ("MEDMOE_LOCAL_PAIR3", "MEDMOE_LOCAL_GRAM", "MEDMOE_PAIR_PITCH", "MEDMOE_TEXT_VARLEN", "MEDMOE_GRAPH", "MEDMOE_WGRAD_STAGED",
              "MEDMOE_DETERMINISTIC"):
        monkeypatch.delenv(k, raising=False)
    return lib


# host queries: the three geometry questions of the default mode and the scratch sizes deterministic mode asks the library for
_HOST_QUERIES = {"medmoe_local_geometry", "medmoe_local_fast_path", "medmoe_local_pair3_supported", "medmoe_gemm_tn_det_scratch",
                 "medmoe_gemm_tn_cols_det_scratch", "medmoe_layernorm_bwd_det_scratch", "medmoe_scale_attn_bwd_det_scratch"}
# entry points that take (or may take) an order-dependent form: none of them may appear in a deterministic step
_ATOMIC_FORMS = {"medmoe_gemm_tn", "medmoe_gemm_tn_staged", "medmoe_gemm_tn_cols", "medmoe_gemm_tn_gram", "medmoe_layernorm_bwd",
                 "medmoe_scale_attn_bwd", "medmoe_router_bwd", "medmoe_ce_strided", "medmoe_soft_xent_strided", "medmoe_hardneg_strided",
                 "medmoe_cos_scale_bwd", "medmoe_sumsq", "medmoe_text_embed_ln_bwd"}
# one case of each local-loss formulation, keyed as in tests/golden/engine_launch_sequences.json
_CASES = {"tiny-transposed": ("tiny", 8), "tinyL-ragged": ("tinyL", 8), "tinyL336-generic": ("tinyL336", 8)}
_IDS = [f"{k}:{step}" for k in _CASES for step in ("train_step", "eval_step")]


def _launches(stub, case, deterministic, how="config"):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    key, step = case.split(":")
    name, B = _CASES[key]
    cfg = config_by_name(name)
    if how == "config":
        cfg.deterministic = deterministic
    eng = Engine(cfg, "cpu")
    if how == "setter":
        eng.set_deterministic(deterministic)
    assert eng.deterministic is deterministic
    batch = O.synthetic_batch(O.config_by_name(name), B, min_len=4)
    del stub.calls[:]
    getattr(eng, step)(batch)
    return [n for n in stub.calls if n not in _HOST_QUERIES]


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_deterministic_is_a_config_field_and_defaults_to_off(stub):
    from medmoe_amd.config import MedMoEConfig, config_by_name
    from medmoe_amd.engine import Engine
    assert MedMoEConfig().deterministic is False
    eng = Engine(config_by_name("tiny"), "cpu")
    assert eng.deterministic is False and eng._det is None


def test_trainable_text_tower_is_refused(stub):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny")
    cfg.deterministic, cfg.freeze_text = True, False
    with pytest.raises(NotImplementedError) as e:
        Engine(cfg, "cpu")
    assert "deterministic" in str(e.value) and "freeze_text" in str(e.value)
    # the same refusal when the flag arrives later (Trainer -> module -> engine)
    cfg = config_by_name("tiny")
    cfg.freeze_text = False
    eng = Engine(cfg, "cpu")
    with pytest.raises(NotImplementedError) as e:
        eng.set_deterministic(True)
    assert "deterministic" in str(e.value) and "freeze_text" in str(e.value)
    assert eng.deterministic is False


def test_graph_replay_is_refused(stub, monkeypatch):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    monkeypatch.setenv("MEDMOE_GRAPH", "1")
    cfg = config_by_name("tiny")
    cfg.deterministic = True
    with pytest.raises(NotImplementedError) as e:
        Engine(cfg, "cpu")
    assert "deterministic" in str(e.value) and "MEDMOE_GRAPH" in str(e.value)


def test_swin_engine_is_refused(stub):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    from medmoe_amd.swin_engine import SwinEngine
    cfg = config_by_name("tiny")
    cfg.deterministic = True
    eng = Engine(cfg, "cpu")
    with pytest.raises(NotImplementedError) as e:
        SwinEngine(eng, encoder=None)
    assert "deterministic" in str(e.value) and "SwinEngine" in str(e.value)


def test_environment_switch(stub, monkeypatch):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    monkeypatch.setenv("MEDMOE_DETERMINISTIC", "1")
    assert Engine(config_by_name("tiny"), "cpu").deterministic is True
    monkeypatch.setenv("MEDMOE_DETERMINISTIC", "0")
    assert Engine(config_by_name("tiny"), "cpu").deterministic is False


# ---------------------------------------------------------------------------------------------------------------------------------
# Hydra key -> Trainer -> module -> engine
# ---------------------------------------------------------------------------------------------------------------------------------
class _NoData:
    def val_dataloader(self):
        return []


def test_trainer_deterministic_reaches_the_engine(stub, monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    from medmoe_amd.hydra_lite import compose, instantiate
    from src.models.medmoe_module import MedMoEPretrainingLightningModule
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg1", "trainer.deterministic=true"])
    assert cfg.trainer.deterministic is True
    tr = instantiate(cfg.trainer, callbacks=[], logger=[])
    assert tr.deterministic is True
    off = instantiate(compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg1"]).trainer, callbacks=[], logger=[])
    assert off.deterministic is False

    class Model(torch.nn.Module):                                   # what the module needs of src.models.components.med_moe.MedMoE here
        def __init__(self):
            super().__init__()
            self.engine = Engine(config_by_name("tiny"), "cpu")

    lit = MedMoEPretrainingLightningModule(model=Model(), loss=instantiate(cfg.model.loss), optimizer=instantiate(cfg.model.optimizer))
    eng = lit.model.engine
    assert eng.deterministic is False
    tr.validate(lit, _NoData())                                      # the start of fit / validate / test hands the flag over
    assert eng.deterministic is True and eng._det is not None
    # the trainer only raises the flag: its default False leaves an engine alone that is deterministic through its config or the
    # environment switch (`MEDMOE_DETERMINISTIC=1 python src/train.py ...` must repeat)
    off.test(lit, _NoData())
    assert eng.deterministic is True and eng._det is not None
    eng.set_deterministic(False)
    off.validate(lit, _NoData())
    assert eng.deterministic is False and eng._det is None
    # a module whose engine cannot honour the flag fails loudly instead of running a step that does not repeat
    eng.cfg.freeze_text = False
    with pytest.raises(NotImplementedError):
        tr.validate(lit, _NoData())


# ---------------------------------------------------------------------------------------------------------------------------------
# launch lists
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _IDS)
def test_deterministic_launch_lists_are_the_recorded_ones_and_hold_no_atomic_form(stub, case):
    got = _launches(stub, case, True)
    assert not (set(got) & _ATOMIC_FORMS), sorted(set(got) & _ATOMIC_FORMS)
    with open(os.path.join(GOLDEN, "engine_launch_sequences_det.json")) as f:
        want = json.load(f)[case]
    assert got == want, next((i, a, b) for i, (a, b) in enumerate(zip(got + [None], want + [None])) if a != b)
    if case.endswith("train_step"):                                  # every weight gradient, LayerNorm and loss head took its deterministic entry
        assert "medmoe_gemm_tn_det" in got and "medmoe_layernorm_bwd_det" in got and "medmoe_scale_attn_bwd_det" in got
        assert "medmoe_router_bwd_det" in got and "medmoe_ce_strided_det" in got and "medmoe_sumsq_det" in got
    assert _launches(stub, case, True, how="setter") == got          # the flag set after construction selects the same launches


@pytest.mark.parametrize("case", _IDS)
def test_launch_lists_with_the_flag_off_are_the_default_ones(stub, case):
    with open(os.path.join(GOLDEN, "engine_launch_sequences.json")) as f:
        want = json.load(f)[case]
    assert _launches(stub, case, False) == want
    # switched on and off again: the default launches, nothing left behind
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    key, step = case.split(":")
    name, B = _CASES[key]
    eng = Engine(config_by_name(name), "cpu")
    batch = O.synthetic_batch(O.config_by_name(name), B, min_len=4)
    eng.set_deterministic(True)
    getattr(eng, step)(batch)
    eng.set_deterministic(False)
    del stub.calls[:]
    getattr(eng, step)(batch)
    assert [n for n in stub.calls if n not in _HOST_QUERIES] == want


def test_header_declares_the_deterministic_entry_points():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    for n in ("medmoe_gemm_tn_det", "medmoe_gemm_tn_cols_det", "medmoe_gemm_tn_gram_det", "medmoe_layernorm_bwd_det", "medmoe_scale_attn_bwd_det",
              "medmoe_router_bwd_det", "medmoe_ce_strided_det", "medmoe_soft_xent_strided_det", "medmoe_hardneg_strided_det",
              "medmoe_cos_scale_bwd_det", "medmoe_nondet_launches"):
        assert n + "(" in hdr, n
    from medmoe_amd import lib_path
    if os.path.exists(lib_path()):
        lib = ctypes.CDLL(lib_path())
        lib.medmoe_nondet_launches.restype = ctypes.c_longlong
        assert lib.medmoe_nondet_launches() >= 0
        lib.medmoe_gemm_tn_det_scratch.restype = ctypes.c_longlong
        # 2 tiles x 4 ranges of (65536 + 512) floats for the plain (8192, 256, 512) wgrad; nothing for an odd shape
        assert lib.medmoe_gemm_tn_det_scratch(8192, 256, 512, 0, 0, 0, 1) == 8 * (65536 + 512)
        assert lib.medmoe_gemm_tn_det_scratch(96, 136, 72, 0, 0, 0, 1) == 0


def test_staged_plans_under_the_host_sanitizers():
    """`make check-plan`: tools/det_plan_check.cpp, a stand-alone host program over csrc/det_plan.h - the range enumeration the wgrad kernel
    and its summing kernel call, the slot counts and the scratch sizes - built with the address and undefined-behaviour sanitizers."""
    import subprocess
    r = subprocess.run(["make", "-C", ROOT, "check-plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "staged plans checked" in r.stdout
