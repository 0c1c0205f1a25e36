"""Weight EMA of the fused step, host side (no GPU): the config keys, the decay schedule, the Hydra experiment, the refusals, the
header and signature table, and which launches `FlatArena` makes against a stub library that computes nothing (the pattern of
tests/test_vit_drop_path_host.py)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")

NEW_SYMBOLS = ("medmoe_adam_step_ema", "medmoe_adam_groups_step_ema", "medmoe_adam_step_ema_g16", "medmoe_adam_groups_step_ema_g16")


def f32(x: float) -> float:
    return ctypes.c_float(x).value


# ------------------------------------------------------------------------------------------------------------------------------------------
# config, schedule
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_default_is_off_and_validate_wants_a_decay_in_the_half_open_unit_interval():
    from medmoe_amd.config import MedMoEConfig, config_by_name
    assert MedMoEConfig().ema_decay == 0.0 and MedMoEConfig().ema_warmup is False
    for ok in (0.0, 0.5, 0.9999):
        c = config_by_name("tiny")
        c.ema_decay = ok
        c.validate()
    for bad in (-0.1, 1.0, 1.5):
        c = config_by_name("tiny")
        c.ema_decay = bad
        with pytest.raises(ValueError, match="ema_decay"):
            c.validate()


def test_schedule_against_hand_computed_values():
    from medmoe_amd.ema import ema_decay_at, one_minus_decay
    # constant: every update takes 1 - decay of the new parameter
    assert [ema_decay_at(t, 0.9999) for t in (0, 1, 1000)] == [0.9999] * 3
    # warm-up: (1 + t) / (10 + t) until it reaches the constant
    assert ema_decay_at(0, 0.9999, True) == 0.1
    assert ema_decay_at(1, 0.9999, True) == 2.0 / 11.0
    assert ema_decay_at(8, 0.9999, True) == 0.5
    assert ema_decay_at(90, 0.9999, True) == 0.91
    # decay 0.9: (1 + t) / (10 + t) < 0.9 <=> t < 80; at t = 80 the two meet, from there on the constant
    assert ema_decay_at(79, 0.9, True) == 80.0 / 89.0 < 0.9
    assert ema_decay_at(80, 0.9, True) == 0.9 and ema_decay_at(81, 0.9, True) == 0.9 and ema_decay_at(10 ** 6, 0.9, True) == 0.9
    # 0.9999 is reached at (1 + t) >= 0.9999 (10 + t) <=> t >= 89990
    assert ema_decay_at(89989, 0.9999, True) < 0.9999 and ema_decay_at(89990, 0.9999, True) == 0.9999
    # a small decay is never raised by the ramp
    assert ema_decay_at(0, 0.05, True) == 0.05
    # what the kernel is handed: 1 - d_t formed in double, rounded once to float
    assert one_minus_decay(0, 0.9999, True) == f32(0.9)
    assert one_minus_decay(5, 0.9999) == f32(1.0 - 0.9999) != 1.0 - 0.9999
    assert one_minus_decay(8, 0.9999, True) == 0.5
    for bad in (-0.5, 1.0):
        with pytest.raises(ValueError, match="ema_decay"):
            ema_decay_at(0, bad)
    with pytest.raises(ValueError, match="update index"):
        ema_decay_at(-1, 0.9)


def test_step_kwargs_are_empty_while_off():
    from medmoe_amd.config import config_by_name
    from medmoe_amd.ema import step_kwargs
    c = config_by_name("tiny")
    assert step_kwargs(c) == {}
    c.ema_decay, c.ema_warmup = 0.999, True
    assert step_kwargs(c) == {"ema_decay": 0.999, "ema_warmup": True}


# ------------------------------------------------------------------------------------------------------------------------------------------
# Hydra, module
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_experiment_resolves_and_carries_the_three_keys(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_ema"])
    assert cfg.model.fused_step is True
    assert (cfg.model.ema.decay, cfg.model.ema.warmup, cfg.model.ema.validate) == (0.9999, True, True)
    assert sorted(dict(cfg.model.ema)) == ["decay", "validate", "warmup"]
    # the rest is cfg2
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert cfg.model.model.vision.num_experts == base.model.model.vision.num_experts == 8 and cfg.data.batch_size == base.data.batch_size
    assert "ema" not in dict(base.model)
    # the same keys from the command line
    on = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2", "+model.ema.decay=0.999", "+model.ema.warmup=true",
                                         "+model.ema.validate=true"])
    assert (on.model.ema.decay, on.model.ema.warmup, on.model.ema.validate) == (0.999, True, True)


def test_module_refuses_ema_without_the_fused_step_and_bad_keys():
    from src.models.medmoe_module import MedMoEPretrainingLightningModule as M
    net = torch.nn.Identity()
    with pytest.raises(NotImplementedError, match="fused_step"):
        M(net, {}, ema={"decay": 0.9999})
    with pytest.raises(ValueError, match="model.ema.decay"):
        M(net, {}, ema={"decay": 1.0})
    with pytest.raises(KeyError, match="decy"):
        M(net, {}, ema={"decy": 0.5})
    with pytest.raises(ValueError, match="validate"):
        M(net, {}, ema={"validate": True})
    off = M(net, {}, ema={"decay": 0.0})                             # off: the module as it was, fused or not
    assert off._ema_decay == 0.0 and not off._ema_validate
    assert M(net, {})._ema_decay == 0.0


def test_header_declares_the_four_symbols_and_the_signature_table_lists_them():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    from medmoe_amd import ops
    for name in NEW_SYMBOLS:
        m = re.search(r"^int %s\((.*)\);" % name, hdr, re.M)
        assert m, name
        short = name[len("medmoe_"):]
        sibling = short.replace("_ema", "")
        assert len(m.group(1).split(",")) == len(ops._SIGS[short]) + 1, name                      # + the stream
        assert ops._SIGS[short] == ops._SIGS[sibling] + "pf", name                               # the sibling's arguments + (ema, one_minus_decay)
        assert m.group(1).endswith("float* ema, float one_minus_decay, hipStream_t stream"), name


# ------------------------------------------------------------------------------------------------------------------------------------------
# FlatArena against a stub library
# ------------------------------------------------------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls, self.args = [], []

    def __getattr__(self, name):
        if not name.startswith("medmoe_"):
            raise AttributeError(name)

        def f(*a):
            self.calls.append(name)
            self.args.append(a)
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
    for cache in ("_FN", "_NT_FN", "_TN_FN"):
        monkeypatch.setattr(ops, cache, {})
    return lib


def _arena():
    from medmoe_amd.flat import FlatArena
    return FlatArena("cpu", [("w", (8, 8)), ("b", (5,))], gemm=[("w", False)])


def test_an_arena_that_never_enables_it_allocates_nothing_and_calls_the_old_entry_points(stub):
    a = _arena()
    nsq = torch.zeros(1)
    a.adam_step(nsq, 1e-3, 0.0, 0.25)
    a.adam_step(nsq, 1e-3, 0.0, 0.25, decoupled=True)
    a.g16_reduced = True
    a.adam_step(nsq, 1e-3, 0.0, 0.25)
    assert a.e32 is None and a.ema_updates == 0
    steps = [c for c in stub.calls if "adam" in c]
    assert steps == ["medmoe_adam_step", "medmoe_adam_groups_step", "medmoe_adam_step_g16"]
    with pytest.raises(RuntimeError, match="enable_ema"):
        a.adam_step(nsq, 1e-3, 0.0, 0.25, ema_decay=0.9)
    with pytest.raises(RuntimeError, match="enable_ema"):
        a.load_ema()
    with pytest.raises(RuntimeError, match="enable_ema"):
        a.ema("w")


def test_ema_steps_call_the_sibling_with_the_scheduled_float_and_count_updates(stub):
    from medmoe_amd.ema import one_minus_decay
    a = _arena()
    a.p32.copy_(torch.arange(a.numel, dtype=torch.float32))
    a.enable_ema()
    assert a.e32.dtype == torch.float32 and torch.equal(a.e32, a.p32) and a.e32.data_ptr() != a.p32.data_ptr() and a.ema_updates == 0
    assert a.ema("b").data_ptr() == a.e32.data_ptr() + 4 * a.offsets["b"] and a.ema("b") is a.ema("b")
    nsq = torch.zeros(1)
    a.adam_step(nsq, 1e-3, 0.0, 0.25, ema_decay=0.9999, ema_warmup=True)
    a.adam_step(nsq, 1e-3, 0.0, 0.25, decoupled=True, ema_decay=0.9999, ema_warmup=True)
    a.g16_reduced = True
    a.adam_step(nsq, 1e-3, 0.0, 0.25, ema_decay=0.9999)
    a.set_param_groups({"b": (0.5, 0.0)})
    a.g16_reduced = True
    a.adam_step(nsq, 1e-3, 0.0, 0.25, ema_decay=0.9999, ema_warmup=True)
    a.adam_step(nsq, 1e-3, 0.0, 0.25)                                # decay 0 on an enabled arena: the old launch, the average stands still
    got = [(c, x) for c, x in zip(stub.calls, stub.args) if "adam" in c]
    assert [c for c, _ in got] == ["medmoe_adam_step_ema", "medmoe_adam_groups_step_ema", "medmoe_adam_step_ema_g16",
                                   "medmoe_adam_groups_step_ema_g16", "medmoe_adam_groups_step"]
    assert a.ema_updates == 4 and a.step_count == 5
    want = [one_minus_decay(0, 0.9999, True), one_minus_decay(1, 0.9999, True), one_minus_decay(2, 0.9999), one_minus_decay(3, 0.9999, True)]
    assert want[0] == f32(0.9) and want[1] == f32(1.0 - 2.0 / 11.0) and want[2] == f32(1.0 - 0.9999)
    for (name, args), omd in zip(got[:4], want):
        assert args[-3] == a.e32.data_ptr() and args[-2] == omd and args[-1] == 0, name         # (..., ema, one_minus_decay, stream)
    # enable_ema() again: back to the master as it is now, no update counted
    a.p32.add_(1.0)
    a.enable_ema()
    assert torch.equal(a.e32, a.p32) and a.ema_updates == 0


def test_load_ema_casts_from_the_average_and_hands_the_hook_its_source(stub):
    from medmoe_amd.flat import FlatArena
    seen = []

    class Store(FlatArena):
        def after_update(self, src=None):
            seen.append(src)
    a = Store("cpu", [("w", (8, 8)), ("b", (5,))], gemm=[("w", False)])
    a.enable_ema()
    master_view = a.f32("b")
    del stub.calls[:], stub.args[:], seen[:]
    a.load_ema()
    assert stub.calls == ["medmoe_cast_bf16", "medmoe_transpose_many"] and stub.args[0][0] == a.e32.data_ptr() and stub.args[0][1] == a.p16.data_ptr()
    assert len(seen) == 1 and seen[0] is a.e32 and a.ema_loaded
    assert a.f32("b").data_ptr() == a.e32.data_ptr() + 4 * a.offsets["b"]             # fp32 reads follow the average
    with pytest.raises(RuntimeError, match="restore_master"):
        a.adam_step(torch.zeros(1), 1e-3, 0.0, 0.25, ema_decay=0.9)
    with pytest.raises(RuntimeError, match="restore_master"):
        a.enable_ema()
    del stub.calls[:], stub.args[:], seen[:]
    a.restore_master()
    assert stub.calls == ["medmoe_cast_bf16", "medmoe_transpose_many"] and stub.args[0][0] == a.p32.data_ptr()
    assert seen == [None] and not a.ema_loaded                                        # existing hooks are called as they always were
    assert a.f32("b") is master_view
