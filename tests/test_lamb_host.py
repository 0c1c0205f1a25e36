"""CPU tests of LAMB's host side: src.optim.Lamb against the float64 restatement of tests/lamb_reference.py, the configuration
keys and the experiment, the segment tables of the real stores, which launches a `lamb` engine's step issues (the stub library of
tests/test_optim_groups_host.py: no launch computes anything), the record enumeration under the sanitizers, and the refusals."""
import functools
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")

import lamb_reference as R                                           # noqa: E402
from test_optim_groups_host import stub                              # noqa: E402,F401  (the stub-library fixture)


# ---- 1. src.optim.Lamb == the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("always_adapt", [False, True])
@pytest.mark.parametrize("trust_clip", [False, True])
@pytest.mark.parametrize("wd", [0.01, 0.0])
def test_torch_lamb_equals_the_reference_in_float64(always_adapt, trust_clip, wd):
    from src.optim import Lamb
    g = torch.Generator().manual_seed(7)
    shapes = [(5, 3), (17,), (4, 4), (9,), (1,)]
    init = [torch.randn(s, generator=g, dtype=torch.float64) * 0.1 for s in shapes]
    init[2].zero_()                                                  # an all-zero tensor: wn = 0 -> r = 1
    init[0] *= 30.0                                                  # a large tensor: r > 1 without trust_clip
    params = [torch.nn.Parameter(t.clone()) for t in init]
    kw = dict(lr=1e-2, weight_decay=wd, betas=(0.9, 0.99), eps=1e-6)
    opt = Lamb(params, always_adapt=always_adapt, trust_clip=trust_clip, **kw)
    ref = [{"p": t.clone(), "m": torch.zeros_like(t), "v": torch.zeros_like(t)} for t in init]
    seen_big, seen_one = False, False
    for t in range(1, 4):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
        grads[3].zero_()                                             # a tensor whose gradient is zero in every step
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt.step()
        for k, (st, gr) in enumerate(zip(ref, grads)):
            one = R.lamb_tensor(st["p"], gr, st["m"], st["v"], t, lr=kw["lr"], wd=wd, betas=kw["betas"], eps=kw["eps"],
                                always_adapt=always_adapt, trust_clip=trust_clip)
            st.update(p=one["p"], m=one["m"], v=one["v"])
            seen_big |= one["r"] > 1.0
            seen_one |= one["r"] == 1.0
            if trust_clip:
                assert one["r"] <= 1.0
            if k == 2 and t == 1:
                assert one["r"] == 1.0                               # zero weights
            if not always_adapt and wd == 0.0:
                assert one["r"] == 1.0
            err = float((params[k].detach() - one["p"]).abs().max())
            assert err <= 1e-12, (t, k, err)
            assert float((opt.state[params[k]]["exp_avg"] - one["m"]).abs().max()) <= 1e-12
            assert float((opt.state[params[k]]["exp_avg_sq"] - one["v"]).abs().max()) <= 1e-12
    assert seen_one
    if not trust_clip and (always_adapt or wd != 0.0):
        assert seen_big


def test_torch_lamb_refuses_bad_arguments():
    from src.optim import Lamb
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(lr=-1.0), dict(eps=0.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            Lamb(p, **kw)
    d = Lamb(p).defaults
    assert (d["lr"], d["weight_decay"], d["betas"], d["eps"], d["always_adapt"], d["trust_clip"]) == (1e-3, 0.01, (0.9, 0.999), 1e-6, False, False)


# ---- 2. configuration -------------------------------------------------------------------------------------------------------------------------
def test_validate_accepts_lamb_and_rejects_non_bool_flags():
    from medmoe_amd.config import config_by_name
    cfg = config_by_name("cfg2")
    assert (cfg.optimizer, cfg.lamb_always_adapt, cfg.lamb_trust_clip) == ("adam", False, False)
    cfg.optimizer, cfg.weight_decay, cfg.adam_eps, cfg.no_decay_1d = "lamb", 0.01, 1e-6, True
    cfg.validate()
    cfg.lamb_always_adapt, cfg.lamb_trust_clip = True, True
    cfg.validate()
    for key in ("lamb_always_adapt", "lamb_trust_clip"):
        for bad in (1, "true", None, 0.0):
            c = config_by_name("tiny")
            setattr(c, key, bad)
            with pytest.raises(ValueError, match=key):
                c.validate()
    c = config_by_name("tiny")
    c.optimizer = "lars"
    with pytest.raises(ValueError, match="optimizer"):
        c.validate()


def test_the_experiment_composes_and_cfg2_is_unchanged(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose, instantiate
    c = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_lamb"])
    o = c.model.optimizer
    assert (o._target_, o.lr, list(o.betas), o.eps, o.weight_decay, o.always_adapt, o.trust_clip) == \
        ("src.optim.Lamb", 1e-3, [0.9, 0.999], 1e-6, 0.01, False, False)
    assert c.model.optimizer_groups.no_decay_1d is True and c.model.fused_step is True and c.trainer.gradient_clip_val == 1.0
    assert c.data.batch_size == 1024
    part = instantiate(o)
    from src.optim import Lamb
    assert isinstance(part, functools.partial) and part.func is Lamb
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert "optimizer_groups" not in base.model and base.model.optimizer._target_ == "torch.optim.Adam"
    assert dict(base.model.optimizer) == {"_target_": "torch.optim.Adam", "_partial_": True, "weight_decay": 0.0, "lr": 5e-5}
    assert base.trainer.gradient_clip_val != 1.0


# ---- 3. segment tables ------------------------------------------------------------------------------------------------------------------------
def _check_table(store, tensors, label):
    """tensors: name -> view of store.p32 (one per parameter tensor of the model).  The table is ascending, ends at n_train, has one segment
    per tensor, under its name, starting at the tensor's storage offset, and covers at least the tensor's extent."""
    segs = store.segments()
    ends = [e for _, e in segs]
    assert ends == sorted(ends) and ends[-1] == store.n_train and all(e > 0 for e in ends), label
    assert len(set(ends)) == len(ends), label                        # no empty segment in a real store
    assert [n for n, _ in segs] == list(tensors) or sorted(n for n, _ in segs) == sorted(tensors), label
    start = 0
    for name, end in segs:
        v = tensors[name]
        assert v.storage_offset() == start + store.train_from, (label, name)
        flat_extent = 1 + sum((s - 1) * st for s, st in zip(v.shape, v.stride()))
        assert flat_extent <= end - start < flat_extent + 8 + (store.shapes.get(name, (0, 0))[-1] if name == "vit.patch_embed.weight" else 0), (label, name)
        start = end
    dev = store._seg_table
    assert dev[0].dtype == torch.int64 and dev[0].tolist() == ends and dev[1].dtype == dev[2].dtype == torch.float32
    assert dev[3].dtype == torch.int64 and all(t.numel() == len(segs) for t in dev)


def _stores(**over):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny")
    for k, v in over.items():
        setattr(cfg, k, v)
    return Engine(cfg, "cpu")


def test_segment_tables_of_the_real_stores(stub):
    from medmoe_amd.optim_groups import GroupRules, apply_rules
    eng = _stores(freeze_text=False)
    ps, ts = eng.params, eng.tstore
    E = eng.cfg.n_expert
    _check_table(ps, ps.named_views(), "ParamStore")
    names = [n for n, _ in ps.segments()]
    assert names == list(ps.named_views())                           # the same order: storage order
    assert sum(n.startswith("moe.experts.") for n in names) == E * 12 and "moe.proj.0.weight" not in names
    # the one-element per-expert tensors: boundaries on single elements, the last one carries the entry's padding
    k = names.index("moe.experts.0.attn_proj.2.bias")
    ends = [e for _, e in ps.segments()]
    assert [ends[k + j] - ends[k + j - 1] for j in range(E - 1)] == [1] * (E - 1)
    _check_table(ts, {n: ts.view(ts.p32, n) for n in ts.shapes}, "TextStore")
    eng.enable_mlm(0.15, 1.0, 3)
    ms = eng.mlm.store
    _check_table(ms, {n: ms.view(ms.p32, n) for n in ms.names}, "MLMStore")
    lo = _stores(text_lora=True).lora
    _check_table(lo, {n: lo.view(lo.p32, n) for n in sorted(lo.true_names(), key=lambda n: lo.offsets[n])}, "LoraStore")
    assert not any(a in [n for n, _ in lo.segments()] for a in lo.groups)        # members individually, never the alias
    # a frozen backbone: only the trainable tail has segments, offsets relative to the tail
    fz = _stores(freeze_vit=True).params
    assert fz.train_from > 0
    _check_table(fz, {n: v for n, v in fz.named_views().items() if n.startswith("moe.")}, "ParamStore:freeze_vit")
    assert list(fz.named_views(fz.g32)) == [n for n, _ in fz.segments()]
    # no segment straddles a run; the table is rebuilt with the groups and carries the runs' multipliers
    stores = {"vit": ps, "text": ts}
    before = ps._seg_table
    apply_rules(stores, GroupRules(no_decay_1d=True, layer_decay=0.75))
    for label, st in stores.items():
        assert st._segments is None
        segs, runs = st.segments(), st.runs
        assert len(runs) > 4
        ends, lrm, wdm, _ = st._seg_table
        start = 0
        for (name, end), lm, wm in zip(segs, lrm.tolist(), wdm.tolist()):
            run = next(r for r in runs if r[0] > start)
            assert end <= run[0], (label, name)                      # one run per segment
            assert (lm, wm) == (pytest.approx(run[1]), run[2]), (label, name)
            start = end
        assert any(w == 0.0 for w in wdm.tolist()) and any(w == 1.0 for w in wdm.tolist())
    assert ps._seg_table is not before
    apply_rules(stores, GroupRules())
    assert ps._segments is None and set(ps.segments() and ps._seg_table[2].tolist()) == {1.0}


def test_a_straddling_segment_is_refused(stub):
    from medmoe_amd.flat import FlatArena
    ar = FlatArena("cpu", [("a", (16,)), ("b", (8,))])
    ar._segment_parts = lambda name: [(name, 16)] if name == "a" else [("b", 8)]
    ar.runs = [(8, 1.0, 1.0), (24, 0.5, 0.0)]                        # a run boundary inside `a`: cannot come from set_param_groups
    with pytest.raises(AssertionError, match="straddles"):
        ar.segments()
    ar._segment_parts = lambda name: [(name, 3)]
    ar.runs = None
    with pytest.raises(AssertionError, match="add up"):
        ar.segments()


# ---- 4. launches ------------------------------------------------------------------------------------------------------------------------------
def test_a_lamb_step_issues_three_launches_per_arena_and_no_adam(stub):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import medmoe_oracle as O
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    batch = O.synthetic_batch(O.config_by_name("tiny"), 8, min_len=4)

    def run(**over):
        cfg = config_by_name("tiny")
        cfg.freeze_text = False
        for k, v in over.items():
            setattr(cfg, k, v)
        eng = Engine(cfg, "cpu")
        del stub.calls[:], stub.args[:]
        eng.train_step(batch)
        return eng, list(stub.calls), list(stub.args)

    _, adam, _ = run()
    assert adam.count("medmoe_adam_step") == 2 and not any(n.startswith("medmoe_lamb") for n in adam)      # what it was
    eng, lamb, args = run(optimizer="lamb", weight_decay=0.01, no_decay_1d=True, layer_decay=0.75, adam_eps=1e-6, lamb_trust_clip=True)
    assert not any(n.startswith("medmoe_adam") for n in lamb)
    trio = ["medmoe_lamb_moments", "medmoe_lamb_ratios", "medmoe_lamb_apply"]
    # the step is the adam one with each medmoe_adam_step replaced by the three LAMB launches; the clip-norm launches stay
    want = []
    for n in adam:
        want += trio if n == "medmoe_adam_step" else [n]
    host = ("medmoe_lamb_plan", "medmoe_lamb_scratch_floats", "medmoe_lamb_coef_slot")        # host queries of the first step, when the segment tables are built
    assert [n for n in lamb if n not in host] == want
    assert sorted(n for n in lamb if n in host) == sorted(host * 2)
    assert lamb.count("medmoe_sumsq_det") == adam.count("medmoe_sumsq_det") == 2
    del stub.calls[:]
    eng.optimizer_step()                                             # a later step reads nothing from the host
    assert [n for n in stub.calls if "lamb" in n] == trio * 2
    mom = [a for n, a in zip(lamb, args) if n == "medmoe_lamb_moments"]
    rat = [a for n, a in zip(lamb, args) if n == "medmoe_lamb_ratios"]
    app = [a for n, a in zip(lamb, args) if n == "medmoe_lamb_apply"]
    for st, m_, r_, a_ in zip((eng.params, eng.tstore), mom, rat, app):
        S = len(st.segments())
        ends, lrm, wdm, base = st._seg_table
        assert m_[0] == st.p32.data_ptr() and m_[1] == st.g32.data_ptr() and m_[4] == st.n_train and m_[8] == S
        assert (m_[5], m_[6], m_[7]) == (ends.data_ptr(), wdm.data_ptr(), base.data_ptr()) and m_[9] == st._lamb_scratch.data_ptr()
        assert (m_[11], m_[12], m_[13], m_[14], m_[15]) == (0.9, 0.999, 1e-6, 0.01, 1) and m_[16] == eng.params.normsq.data_ptr()
        assert r_[0] == m_[9] and r_[5] == S and (r_[8], r_[9]) == (0, 1) and r_[10] == st._lamb_ratios.data_ptr()
        assert a_[0] == st.p32.data_ptr() and a_[3] == st.p16.data_ptr() and (a_[5], a_[6], a_[7]) == (ends.data_ptr(), lrm.data_ptr(), wdm.data_ptr())
        assert a_[9] == st._lamb_ratios.data_ptr() and a_[15] == 1 and st.step_count == 2
        names, r = st.trust_ratios()
        assert len(names) == S == r.numel() and st._lamb_ratios.numel() == 3 * S
    # the EMA and bf16-gradient forms
    ar = eng.tstore
    ar.enable_ema()
    ar.g16_reduced = True
    del stub.calls[:]
    ar.lamb_step(ar.sumsq(), 1e-3, 0.01, 1.0, ema_decay=0.99)
    assert [n for n in stub.calls if "lamb" in n] == ["medmoe_lamb_moments_g16", "medmoe_lamb_ratios", "medmoe_lamb_apply_ema"]
    assert ar.g16_reduced is False and ar.ema_updates == 1 and ar.step_count == 3
    ar.ema_loaded = True
    with pytest.raises(RuntimeError, match="restore_master"):
        ar.lamb_step(ar.normsq, 1e-3, 0.01, 1.0)


def test_signatures_match_the_header():
    import re
    from medmoe_amd import ops
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    for name in ("lamb_moments", "lamb_moments_g16", "lamb_ratios", "lamb_apply", "lamb_apply_ema"):
        m = re.search(r"^int medmoe_%s\((.*)\);" % name, hdr, re.M)
        assert m and m.group(1).endswith("hipStream_t stream"), name
        assert len(m.group(1).split(",")) == len(ops._SIGS[name]) + 1, name
        kinds = "".join("p" if "*" in a else "l" if "long long" in a else "d" if "double" in a else "f" if "float" in a else "i"
                        for a in m.group(1).split(",")[:-1])
        assert kinds == ops._SIGS[name], name
    src = open(os.path.join(ROOT, "medmoe_amd", "csrc", "lamb.hip")).read()
    assert "atomic" not in src.replace("No floating-point atomics", "") and "g_mm_nondet" not in src


# ---- 5. the record enumeration ----------------------------------------------------------------------------------------------------------------
def test_make_check_lamb_plan():
    out = subprocess.run(["make", "-C", ROOT, "check-lamb-plan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "segment tables" in out.stdout


def test_plan_through_the_library_matches_a_python_count():
    from medmoe_amd import lib_path, ops
    if not os.path.exists(lib_path()):                              # the project's own library: build it, never skip
        import __graft_entry__ as entry
        entry.build()
    C = ops.lamb_chunk()
    assert C >= 1024 and C % 4 == 0
    ends = torch.tensor([1, 8, C - 1, C, C + 1, 3 * C + 5, 3 * C + 5, 5 * C], dtype=torch.int64)
    base = ops.lamb_plan(ends, 5 * C).tolist()
    want, start, recs = [], 0, 0
    for e in ends.tolist():
        want.append(recs)
        recs += 0 if e == start else (e - 1) // C - start // C + 1
        start = e
    assert base == want and 2 * recs <= ops.lamb_scratch_floats(5 * C, len(want))
    with pytest.raises(ValueError, match="ascending"):
        ops.lamb_plan(torch.tensor([8, 4], dtype=torch.int64), 8)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_the_module_without_the_fused_step_and_classify_step_refuse(stub, monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from test_grad_comm_host import _module
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_lamb"])
    with pytest.raises(NotImplementedError, match="Lamb.*fused_step"):
        _module(cfg, fused_step=False)
    lit = _module(cfg, fused_step=True, optimizer_groups=dict(cfg.model.optimizer_groups))
    c = lit.model.engine.cfg
    assert (c.optimizer, c.lr, c.weight_decay, c.adam_betas, c.adam_eps, c.lamb_always_adapt, c.lamb_trust_clip, c.no_decay_1d) == \
        ("lamb", 1e-3, 0.01, (0.9, 0.999), 1e-6, False, False, True)
    lit.model.register_parameter("flat", torch.nn.Parameter(torch.zeros(4)))        # the stand-in model has no parameter of its own
    opt = lit.configure_optimizers()["optimizer"]
    from src.optim import Lamb
    assert isinstance(opt, Lamb) and lit._fused_opt is opt and opt.param_groups[0]["lr"] == 1e-3
    # an Adam module is what it was, and still refuses Lamb's keywords
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert _module(base, fused_step=True).model.engine.cfg.optimizer == "adam"
    from medmoe_amd.classify import ClassifierHead
    eng = lit.model.engine
    with pytest.raises(NotImplementedError, match="cfg.optimizer.*model.optimizer._target_"):
        eng.classify_step({"image": torch.zeros(1)}, ClassifierHead(eng.cfg.d_out, 5, "cpu"), train_tower=False)
