"""Host side of the bf16 gradient exchange (MedMoEConfig.grad_comm_dtype / MEDMOE_GRAD_COMM=bf16 / model.grad_comm_dtype): config
validation, the environment switch, the Hydra key's way into the engine's config, the refusal without the fused step, the engine's launch
list with the exchange on (against a stub library that computes nothing), and medmoe_amd.dist's reducers with a `comm` object on two CPU
gloo ranks - the bf16 buffer holds bf16(g0 / 2) + bf16(g1 / 2) exactly, the fp32 gradient is left alone, and without `comm` the reducers
do what they did."""
import ctypes
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

import medmoe_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")


class _StubLib:
    def __init__(self):
        self.calls = []
        self.args = []

    def __getattr__(self, name):
        if not name.startswith("medmoe_"):
            raise AttributeError(name)

        def f(*a):
            self.calls.append(name)
            self.args.append(a)
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
    for cache in ("_FN", "_NT_FN", "_TN_FN"):
        monkeypatch.setattr(ops, cache, {})
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    for k in ("MEDMOE_GRAD_COMM", "MEDMOE_DETERMINISTIC", "MEDMOE_GRAPH", "MEDMOE_DIST_WORLD1"):
        monkeypatch.delenv(k, raising=False)
    return lib


_NEW = {"medmoe_grad_pack_bf16", "medmoe_sumsq_det_bf16", "medmoe_adam_step_g16", "medmoe_adam_groups_step_g16"}


# ---------------------------------------------------------------------------------------------------------------------------------
# config, environment switch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_config_field_defaults_to_fp32_and_rejects_anything_else():
    from medmoe_amd.config import MedMoEConfig, config_by_name
    assert MedMoEConfig().grad_comm_dtype == "fp32"
    cfg = config_by_name("tiny")
    for ok in ("fp32", "bf16"):
        cfg.grad_comm_dtype = ok
        cfg.validate()
    for bad in ("fp16", "BF16", "", None, 16):
        cfg.grad_comm_dtype = bad
        with pytest.raises(ValueError, match="grad_comm_dtype"):
            cfg.validate()


def test_a_single_process_ignores_the_key_and_a_data_parallel_engine_takes_it(stub, monkeypatch):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny")
    cfg.grad_comm_dtype = "bf16"
    eng = Engine(cfg, "cpu")
    assert not eng.dist and eng.grad_comm(eng.params) is None        # no all-reduce happens: nothing to pack
    batch = O.synthetic_batch(O.config_by_name("tiny"), 8, min_len=4)
    del stub.calls[:]
    eng.train_step(batch)
    with_key = list(stub.calls)
    ref = Engine(config_by_name("tiny"), "cpu")
    del stub.calls[:]
    ref.train_step(batch)
    assert with_key == stub.calls and not set(with_key) & _NEW
    eng.dist = True
    assert eng.grad_comm(eng.params) is eng.params
    eng.cfg.grad_comm_dtype = "fp32"                                 # read per step: the Lightning module writes the key after construction
    assert eng.grad_comm(eng.params) is None
    eng.cfg.grad_comm_dtype = "fp8"
    with pytest.raises(ValueError, match="grad_comm_dtype"):
        eng.grad_comm(eng.params)


def test_environment_switch(stub, monkeypatch):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    monkeypatch.setenv("MEDMOE_GRAD_COMM", "bf16")
    eng = Engine(config_by_name("tiny"), "cpu")
    assert eng.cfg.grad_comm_dtype == "fp32" and eng.grad_comm(eng.params) is None     # a single process ignores it
    eng.dist = True
    assert eng.grad_comm(eng.params) is eng.params
    monkeypatch.setenv("MEDMOE_GRAD_COMM", "fp32")
    eng = Engine(config_by_name("tiny"), "cpu")
    eng.dist = True
    assert eng.grad_comm(eng.params) is None
    monkeypatch.setenv("MEDMOE_GRAD_COMM", "int8")
    with pytest.raises(ValueError, match="MEDMOE_GRAD_COMM"):
        Engine(config_by_name("tiny"), "cpu")


# ---------------------------------------------------------------------------------------------------------------------------------
# Hydra key -> module -> engine config
# ---------------------------------------------------------------------------------------------------------------------------------
def _module(cfg, **kw):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    from medmoe_amd.hydra_lite import instantiate
    from src.models.medmoe_module import MedMoEPretrainingLightningModule

    class Model(torch.nn.Module):                                   # what the module needs of src.models.components.med_moe.MedMoE here
        def __init__(self):
            super().__init__()
            self.engine = Engine(config_by_name("tiny"), "cpu")

    loss = dict(cfg.model.loss)
    loss["local_loss"], loss["global_loss"] = instantiate(cfg.model.loss.local_loss), instantiate(cfg.model.loss.global_loss)
    return MedMoEPretrainingLightningModule(model=Model(), loss=loss, optimizer=instantiate(cfg.model.optimizer), **kw)


def test_hydra_key_reaches_the_engine_config(stub, monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert base.model.grad_comm_dtype == "fp32" and base.model.fused_step is True
    assert compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe"]).model.grad_comm_dtype == "fp32"
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2", "model.grad_comm_dtype=bf16"])
    assert cfg.model.grad_comm_dtype == "bf16"
    lit = _module(cfg, fused_step=True, grad_comm_dtype=cfg.model.grad_comm_dtype)
    assert lit.model.engine.cfg.grad_comm_dtype == "bf16"
    lit = _module(base, fused_step=True, grad_comm_dtype=base.model.grad_comm_dtype)
    assert lit.model.engine.cfg.grad_comm_dtype == "fp32"
    assert _module(base, fused_step=True).model.engine.cfg.grad_comm_dtype == "fp32"


def test_refused_without_the_fused_step_and_with_an_unknown_value(stub, monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe"])
    with pytest.raises(NotImplementedError, match="grad_comm_dtype"):
        _module(cfg, fused_step=False, grad_comm_dtype="bf16")
    _module(cfg, fused_step=False, grad_comm_dtype="fp32")           # the default value with the autograd path: what the yaml composes to
    for fused in (False, True):
        with pytest.raises(ValueError, match="grad_comm_dtype"):
            _module(cfg, fused_step=fused, grad_comm_dtype="fp16")


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine's launches with the exchange on (collectives replaced by local fakes)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_engine_launches_with_the_bf16_exchange(stub, monkeypatch):
    """One pack per bucket (in the order the backward completes them) and one for the text arena, the clip norm and Adam in their bf16-gradient
    forms, nothing else changed; an accumulating micro-batch packs nothing; the fp32 exchange launches none of the new entry points."""
    import medmoe_amd.dist as D
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    reduced = []
    monkeypatch.setattr(D, "_all_reduce_bf16", lambda t, async_op=False: reduced.append(t.numel()))
    monkeypatch.setattr(D.dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(D, "gather_embeddings", lambda a, b: (torch.cat([a, a]), torch.cat([b, b])))
    monkeypatch.setattr(D, "gather_rows", lambda t: torch.cat([t, t]))
    monkeypatch.setattr(D, "scatter_key_grads", lambda d: d[: d.shape[0] // 2].clone())
    monkeypatch.setattr(D, "label_offset", lambda B: B * 1)
    monkeypatch.setattr(D, "allreduce_mean_", (lambda real: lambda g, comm=None: real(g, comm=comm) if comm is not None else g)(D.allreduce_mean_))

    class Fp32Reducer:                                               # the fp32 exchange without a process group
        def __init__(self, flat, bounds):
            pass
        def ready(self, i):
            pass
        def finish(self):
            pass

    batch = O.synthetic_batch(O.config_by_name("tiny"), 8, min_len=4)
    runs = {}
    Real = D.BucketedAllReduce
    for mode in ("fp32", "bf16"):
        cfg = config_by_name("tiny")
        cfg.freeze_text, cfg.grad_comm_dtype = False, mode
        eng = Engine(cfg, "cpu")
        eng.world, eng.rank, eng.dist = 2, 1, True
        monkeypatch.setattr(D, "BucketedAllReduce", Fp32Reducer if mode == "fp32" else Real)
        del stub.calls[:], stub.args[:]
        eng.train_step(batch, optimizer=False)                      # accumulates locally: no pack, no collective
        assert not set(stub.calls) & _NEW and not reduced, mode
        del stub.calls[:], stub.args[:]
        eng.train_step(batch, zero_grad=False)
        runs[mode] = (list(stub.calls), list(stub.args), eng)
    calls, args, eng = runs["bf16"]
    b = eng.bucket_bounds
    L = eng.cfg.n_layer_v
    packs = [a for n, a in zip(calls, args) if n == "medmoe_grad_pack_bf16"]
    order = [L + 1] + list(range(L, 0, -1)) + [0]
    assert len(packs) == L + 3                                       # L + 2 buckets of the image arena, then the text arena whole
    for i, a in zip(order, packs):
        assert a[0] == eng.params.g32.data_ptr() + 4 * b[i] and a[1] == eng.params.g16.data_ptr() + 2 * b[i] and a[2] == b[i + 1] - b[i]
        assert a[3] == 0.5 and b[i] % 8 == 0
    assert packs[-1][:3] == (eng.tstore.g32.data_ptr(), eng.tstore.g16.data_ptr(), eng.tstore.numel) and packs[-1][3] == 0.5
    assert reduced == [b[i + 1] - b[i] for i in order] + [eng.tstore.numel]
    assert calls.count("medmoe_sumsq_det_bf16") == 2 and calls.count("medmoe_adam_step_g16") == 2
    assert "medmoe_sumsq_det" not in calls and "medmoe_adam_step" not in calls
    adam = [a for n, a in zip(calls, args) if n == "medmoe_adam_step_g16"]
    assert [a[1] for a in adam] == [eng.params.g16.data_ptr(), eng.tstore.g16.data_ptr()]
    assert not eng.params.g16_reduced and not eng.tstore.g16_reduced   # cleared with the step
    rename = {"medmoe_sumsq_det_bf16": "medmoe_sumsq_det", "medmoe_adam_step_g16": "medmoe_adam_step"}
    assert [rename.get(n, n) for n in calls if n != "medmoe_grad_pack_bf16"] == runs["fp32"][0]
    assert not set(runs["fp32"][0]) & _NEW


def test_engine_refuses_bucket_offsets_that_are_no_multiple_of_8(stub, monkeypatch):
    """The pack moves 16 bytes per lane from a bucket's first element on: a layout whose bucket offsets are not multiples of 8 elements is
    refused when the engine is built, not at the first distributed step."""
    import medmoe_amd.engine as E
    from medmoe_amd.config import config_by_name

    class Shifted(E.ParamStore):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.offsets = dict(self.offsets)
            self.offsets["vit.layer.1.attention_layernorm.weight"] += 4
    assert all(b % 8 == 0 for b in E.Engine(config_by_name("tiny"), "cpu").bucket_bounds)
    monkeypatch.setattr(E, "ParamStore", Shifted)
    with pytest.raises(ValueError, match="multiples of 8"):
        E.Engine(config_by_name("tiny"), "cpu")


def test_arena_flag_selects_the_grouped_bf16_form_too(stub):
    from medmoe_amd.flat import FlatStore
    st = FlatStore({"a": torch.zeros(5, 3), "b": torch.zeros(7)}, "cpu")
    assert st._g16 is None and not st.g16_reduced                   # allocated on first need
    st.pack(0, st.numel, 0.5)
    assert st.g16.dtype == torch.bfloat16 and st.g16.numel() == st.numel == st.g32.numel()
    st.g16_reduced = True
    assert st.reduced_grad().dtype == torch.float32 and st.reduced_grad() is not st.g32
    del stub.calls[:]
    st.adam_step(st.sumsq(), 1e-4, 0.05, 0.25, decoupled=True)
    assert stub.calls[:2] == ["medmoe_sumsq_det_bf16", "medmoe_adam_groups_step_g16"] and not st.g16_reduced
    assert st.reduced_grad() is st.g32
    del stub.calls[:]
    st.adam_step(st.sumsq(), 1e-4, 0.05, 0.25, decoupled=True)
    assert stub.calls[:2] == ["medmoe_sumsq_det", "medmoe_adam_groups_step"]
    for clear in (st.zero_grad, st.new_grad_arena):
        st.g16_reduced = True
        clear()
        assert not st.g16_reduced


# ---------------------------------------------------------------------------------------------------------------------------------
# the reducers on two CPU gloo ranks, with a torch pack
# ---------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


class _TorchComm:
    """What the reducers need of an arena, in torch on CPU tensors."""
    def __init__(self, flat):
        self.flat, self.g16, self.g16_reduced = flat, torch.zeros(flat.numel(), dtype=torch.bfloat16), False

    def pack(self, lo, hi, scale):
        self.g16[lo:hi] = (self.flat[lo:hi] * scale).to(torch.bfloat16)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from medmoe_amd import dist as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, bounds = 40, [0, 8, 24, 40]
    g = [torch.randn(n, generator=torch.Generator().manual_seed(7 + r)) * 3.0 for r in range(world)]
    g[0][3], g[1][3] = 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8             # a round-to-even tie after the halving on both ranks
    want = (g[0] * 0.5).to(torch.bfloat16) + (g[1] * 0.5).to(torch.bfloat16)      # evaluated in bf16: one rounding of the exact sum
    ok = {}
    flat = g[rank].clone()
    comm = _TorchComm(flat)
    red = D.BucketedAllReduce(flat, bounds, comm=comm)
    for i in (2, 0, 1):
        red.ready(i)
    try:
        red.ready(0); ok["twice"] = False
    except RuntimeError as e:
        ok["twice"] = "reduced twice" in str(e)
    assert not comm.g16_reduced
    red.finish()
    ok["buckets"] = all(torch.equal(comm.g16[bounds[i]: bounds[i + 1]], want[bounds[i]: bounds[i + 1]]) for i in range(3))
    ok["flag"] = comm.g16_reduced is True
    ok["flat_untouched"] = torch.equal(flat, g[rank])
    comm2 = _TorchComm(flat)
    red2 = D.BucketedAllReduce(flat, [0, 16, 40], comm=comm2); red2.ready(0)
    try:
        red2.finish(); ok["never"] = False
    except RuntimeError as e:
        ok["never"] = "never reduced" in str(e) and not comm2.g16_reduced
        red2.ready(1); red2.finish()
    ok["second"] = torch.equal(comm2.g16, want) and comm2.g16_reduced
    comm3 = _TorchComm(flat)
    out = D.allreduce_mean_(flat, comm=comm3)
    ok["unbucketed"] = torch.equal(comm3.g16, want) and comm3.g16_reduced and out is comm3.g16 and torch.equal(flat, g[rank])
    comm6 = _TorchComm(flat)                                        # the two halves of the un-bucketed pair: launched, then joined
    started = D.allreduce_mean_start(flat, comm=comm6)
    ok["start_not_flagged"] = not comm6.g16_reduced
    started.finish()
    ok["start_finish"] = torch.equal(comm6.g16, want) and comm6.g16_reduced and torch.equal(flat, g[rank])
    flat7 = g[rank].clone()
    D.allreduce_mean_start(flat7).finish()
    ok["start_fp32"] = torch.equal(flat7, (g[0] + g[1]) / world)
    # without comm: today's results (sum in fp32, then the division)
    red4 = D.BucketedAllReduce(flat, bounds)
    for i in (1, 2, 0):
        red4.ready(i)
    red4.finish()
    ok["fp32_bucketed"] = torch.equal(flat, (g[0] + g[1]) / world)
    flat5 = g[rank].clone()
    ok["fp32_unbucketed"] = D.allreduce_mean_(flat5) is flat5 and torch.equal(flat5, (g[0] + g[1]) / world)
    q.put((rank, ok))
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_reducers_with_comm_on_two_gloo_ranks():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=100) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    for rank, ok in res:
        assert all(ok.values()) and len(ok) == 12, (rank, ok)
