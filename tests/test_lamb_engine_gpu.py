"""LAMB through the engines and the Lightning module on the GPU (cfg.optimizer = "lamb").  The oracle is src.optim.Lamb stepped
in float64 on the gradients the stores export, from the state the stores held before the step, scaled by the step's own clip coefficient
(the fp32 value the launches formed and kept, FlatArena.last_clip_coef, held against the float64 formula first);
the bar per element is the kernel test's: |err| <= 2^-24 |p_ref| + lr lr_mult r_ref (|a| + |wd p|) (bar_r + 8 2^-24), bar_r from the
library's summation constants (tests/test_lamb_gpu.py).  Measured values are printed as `[bar]` lines."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lamb_reference as R                                           # noqa: E402

U24 = 2.0 ** -24
F64 = torch.float64
LR, WD, CLIP, EPS, BETAS = 1e-3, 0.01, 1.0, 1e-6, (0.9, 0.999)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


@pytest.fixture()
def project_root(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)


def _cfg(**over):
    from medmoe_amd.config import config_by_name
    cfg = config_by_name("tiny2")
    cfg.optimizer, cfg.lr, cfg.weight_decay, cfg.clip, cfg.adam_eps, cfg.adam_betas = "lamb", LR, WD, CLIP, EPS, BETAS
    cfg.no_decay_1d, cfg.layer_decay = True, 0.75
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _named(st, flat):
    """name -> device view of `flat` (a buffer of the store's layout), one per parameter tensor of the model, under the names the store exports."""
    if hasattr(st, "named_views"):
        return st.named_views(flat)
    if hasattr(st, "true_names"):
        return {n: st.true_view(flat, n) for n in st.true_names()}
    return {n: st.view(flat, n) for n in st.shapes if n not in st.groups and not st.is_frozen(n)}


def _mults(st, view):
    """(lr_mult, wd_mult) of the run the tensor lies in, found from the view's storage offset and the store's run list - not from the segment
    table under test."""
    off = view.storage_offset() + (st.train_from if view.untyped_storage().data_ptr() != st.p32.untyped_storage().data_ptr() else 0)
    for end, lm, wm in (st.runs or [(st.numel, 1.0, 1.0)]):
        if off < end:
            return lm, wm
    raise AssertionError(off)


def _bar_r(ops, st):
    C = ops.lamb_chunk()
    T, RT = ops.lamb_sum_shape()
    ends = [0] + [e for _, e in st.segments()]
    recs = max((b - 1) // C - a // C + 1 for a, b in zip(ends, ends[1:]) if b > a)
    K = C // T + -(-recs // RT)
    D = int(math.log2(64)) + int(math.log2(T // 64)) + int(math.log2(RT))
    return R.sum_bar(K, D) + 3 * U24


def _lamb_oracle_step(ops, eng, arenas, step_fn, always_adapt=False, trust_clip=False, label=""):
    """One optimiser step of the engine against src.optim.Lamb in float64.  Returns the worst |err| / bar."""
    from src.optim import Lamb
    c = eng.cfg
    before = []
    for st in arenas:
        m, v = st.adam_state()
        p_named = st.named_views() if hasattr(st, "named_views") else _named(st, st.p32)
        if st.train_from:
            p_named = {n: t for n, t in p_named.items() if n in _named(st, st.g32)}
        g_named, m_named, v_named = _named(st, st.g32), _named(st, m), _named(st, v)
        assert list(p_named) == list(g_named)
        before.append({n: (p_named[n].detach().cpu().to(F64), g_named[n].detach().cpu().to(F64), m_named[n].detach().cpu().to(F64),
                           v_named[n].detach().cpu().to(F64), _mults(st, p_named[n])) for n in p_named})
    t_before = [st.step_count for st in arenas]
    step_fn()
    torch.cuda.synchronize()
    # ONE clip norm over all arenas (the image arena's buffer holds the total): every arena's launch formed the same fp32 coefficient from it
    coefs = [R.device_coef(st, float(eng.params.normsq), c.clip, 1.0, label) for st in arenas]
    coef = coefs[0]
    assert all(x == coef for x in coefs)
    worst = 0.0
    for st, rec, t0 in zip(arenas, before, t_before):
        t = t0 + 1
        assert st.step_count == t
        bar_r = _bar_r(ops, st)
        params, groups = {}, []
        for n, (p, g, m, v, (lm, wm)) in rec.items():
            q = torch.nn.Parameter(p.clone())
            q.grad = g * coef
            params[n] = q
            groups.append({"params": [q], "lr": c.lr * lm, "weight_decay": c.weight_decay * wm})
        opt = Lamb(groups, lr=c.lr, weight_decay=c.weight_decay, betas=tuple(c.adam_betas), eps=c.adam_eps, always_adapt=always_adapt,
                   trust_clip=trust_clip)
        for n, (p, g, m, v, _) in rec.items():
            opt.state[params[n]] = {"step": t - 1, "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        opt.step()
        after = st.named_views() if hasattr(st, "named_views") else _named(st, st.p32)
        names, ratios = st.trust_ratios()
        ratios = dict(zip(names, ratios.cpu().tolist()))
        assert set(rec) <= set(names) or hasattr(st, "true_names")
        for n, (p, g, m, v, (lm, wm)) in rec.items():
            one = R.lamb_tensor(p, g, m, v, t, lr=c.lr * lm, wd=c.weight_decay * wm, betas=tuple(c.adam_betas), eps=c.adam_eps, coef=coef,
                                always_adapt=always_adapt, trust_clip=trust_clip)
            want = params[n].detach()
            tol = U24 * want.abs() + (c.lr * lm * one["r"]) * (one["a"].abs() + (c.weight_decay * wm * p).abs()) * (bar_r + 8 * U24)
            err = (after[n].detach().cpu().to(F64) - want).abs()
            bad = err > tol
            if bool(bad.any()):                                      # the figures of the worst element, before the assertion
                i = int((err / tol.clamp_min(1e-300)).argmax())
                f = lambda x: float(x.reshape(-1)[i])
                m_dev, v_dev = _named(st, st.m)[n].detach().cpu().to(F64), _named(st, st.v)[n].detach().cpu().to(F64)
                print(f"[bar] {label} {n}[{i}] MISSES: |err| {f(err):.6e} > bar {f(tol):.6e}; p {f(p):.9e} g {f(g):.9e} m {f(m):.9e} v {f(v):.9e} "
                      f"-> m_ref {f(one['m']):.9e} m_dev {f(m_dev):.9e} v_ref {f(one['v']):.9e} v_dev {f(v_dev):.9e} a_ref {f(one['a']):.9e} "
                      f"r_ref {one['r']:.9e} r_dev {ratios.get(n)} lr*lr_mult {c.lr * lm:.9e} wd {c.weight_decay * wm} coef {coef:.9e} "
                      f"p_ref {f(want):.9e} p_dev {f(after[n].detach().cpu().to(F64)):.9e}")
            assert not bool(bad.any()), (label, n, t, float((err / tol.clamp_min(1e-300)).max()))
            if bool((tol > 0).any()):
                worst = max(worst, float((err / tol.clamp_min(1e-300))[tol > 0].max()))
            if n in ratios:                                          # the per-tensor ratio, expert by expert
                if one["r"] == 1.0:
                    assert ratios[n] == 1.0, (label, n)
                else:
                    assert abs(ratios[n] - one["r"]) <= bar_r * one["r"], (label, n, ratios[n], one["r"])
        assert torch.equal(st.p16, st.p32.to(torch.bfloat16))
    print(f"[bar] {label} p_new: max |err| / bar {worst:.3f} <= 1 (clip coefficient {coef:.4f})")
    return worst


def _three_steps(ops, eng, arenas, label):
    import bench
    for it in range(3):
        eng.train_step(bench.synthetic_batch(eng.cfg, 8, 30 + it, eng.device), optimizer=False)
        _lamb_oracle_step(ops, eng, arenas, eng.optimizer_step, eng.cfg.lamb_always_adapt, eng.cfg.lamb_trust_clip, label=f"{label} step {it + 1}")
    assert all(st.step_count == 3 for st in arenas)


def test_engine_steps_match_the_float64_oracle_and_experts_have_their_own_ratios(ops):
    from medmoe_amd.engine import Engine
    eng = Engine(_cfg(), "cuda:0", seed=0)
    _three_steps(ops, eng, [eng.params], "frozen text")
    names, r = eng.params.trust_ratios()
    r = dict(zip(names, r.cpu().tolist()))
    E = eng.cfg.n_expert
    per_expert = [r[f"moe.experts.{e}.proj_convs.0.0.weight"] for e in range(E)]
    assert len(set(per_expert)) == E and all(x != 1.0 and x > 0 for x in per_expert)          # one ratio per expert, not one per stack
    assert all(r[n] == 1.0 for n in names if n.endswith(".bias") or "layernorm" in n or "layer_norm" in n)   # no decay: plain Adam


def test_two_arenas_share_one_clip_norm(ops):
    from medmoe_amd.engine import Engine
    eng = Engine(_cfg(freeze_text=False, lamb_always_adapt=True), "cuda:0", seed=0)
    _three_steps(ops, eng, [eng.params, eng.tstore], "trainable text")
    _, r = eng.tstore.trust_ratios()
    assert bool((r != 1.0).any())


def test_text_lora_adapters_step_with_lamb(ops):
    from medmoe_amd.engine import Engine
    eng = Engine(_cfg(text_lora=True, lamb_trust_clip=True), "cuda:0", seed=0)
    _three_steps(ops, eng, [eng.params, eng.lora], "text_lora")
    assert eng.lora.pad_is_zero() and eng.lora.pad_is_zero(eng.lora.m)


def test_deterministic_mode_two_engines_agree_bit_for_bit(ops):
    import bench
    from medmoe_amd.engine import Engine
    batches = [bench.synthetic_batch(_cfg(), 8, 50 + i, "cuda:0") for i in range(3)]

    def run():
        eng = Engine(_cfg(deterministic=True), "cuda:0", seed=3)
        assert eng.deterministic
        eng.train_step(batches[0])
        torch.cuda.synchronize()
        before = ops.nondet_launches()
        for b in batches[1:]:
            eng.train_step(b)
        torch.cuda.synchronize()
        assert ops.nondet_launches() == before and eng.params.step_count == 3
        m, v = eng.params.adam_state()
        return [eng.params.p32.clone(), m.clone(), v.clone(), eng.params.p16.clone(), eng.params.trust_ratios()[1].clone()]
    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(bool(torch.isfinite(x.float()).all()) for x in a)


def test_the_weight_average_follows(ops):
    import bench
    from medmoe_amd.ema import one_minus_decay
    from medmoe_amd.engine import Engine
    eng = Engine(_cfg(ema_decay=0.9), "cuda:0", seed=0)
    st = eng.params
    for it in range(2):
        eng.train_step(bench.synthetic_batch(eng.cfg, 8, 60 + it, eng.device), optimizer=False)
        e0 = st.e32.clone() if st.e32 is not None else st.p32.clone()
        eng.optimizer_step()
        omd = one_minus_decay(it, 0.9, False)
        assert st.ema_updates == it + 1 and torch.equal(st.e32, e0 + omd * (st.p32 - e0))
    assert not torch.equal(st.e32, st.p32)


def test_one_rank_rccl_group_lamb_reads_the_bf16_sum():
    """grad_comm_dtype = "bf16" with optimizer = "lamb" over a one-rank RCCL group (tools/rccl_world1_lamb.py, MEDMOE_DIST_WORLD1=1: how
    tests/test_grad_comm_engine_gpu.py reaches the _g16 path), in a child process of its own - the group has to exist before anything
    touches the GPU: in front of every arena's lamb_step the exchange has set the flag and g16 == bf16(g32), the step issues the _g16
    moments launch, and p, m, v, p16 and the ratios equal the fp32-gradient launches on g16.float() bit for bit."""
    import subprocess
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561")
    env.pop("MEDMOE_GRAD_COMM", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_world1_lamb.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "rccl world-1 lamb bf16 path OK" in r.stdout and "lamb behind the bf16 exchange:" in r.stdout, r.stdout[-2000:]


# ---- through Hydra ----------------------------------------------------------------------------------------------------------------------------
LAMB = ["experiment=pretraining_medmoe_cfg2_lamb", "model.model.vision.config_name=tiny2"]


def _lit(overrides):
    from medmoe_amd.hydra_lite import compose, instantiate
    cfg = compose(CONFIGS, "train.yaml", overrides)
    return cfg, instantiate(cfg.model)


def _mb(b):
    return {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"]}}


def test_one_fit_step_runs_through_the_entry_point(ops, project_root, tmp_path):
    import src.train as T
    from medmoe_amd.hydra_lite import compose
    cfg = compose(CONFIGS, "train.yaml", LAMB + ["data.synthetic_size=16", "data.synthetic_vocab=97", "data.batch_size=8", "data.max_len=16",
                                                "data.num_workers=0", "extras.print_config=false", "trainer.max_epochs=1",
                                                "+trainer.limit_train_batches=1", "+trainer.limit_val_batches=1",
                                                f"callbacks.model_checkpoint.dirpath={tmp_path}/ckpt"], output_dir=str(tmp_path))
    metrics, objects = T.train(cfg)
    lit = objects["model"]
    eng = lit.model.engine
    assert eng.cfg.optimizer == "lamb" and eng.cfg.clip == 1.0 and eng.params.step_count == 1 and objects["trainer"].global_step == 1
    assert math.isfinite(float(metrics["train/loss"]))
    names, r = eng.params.trust_ratios()
    assert bool(torch.isfinite(r).all()) and bool((r != 1.0).any())


def test_the_schedulers_lr_reaches_the_engine_and_the_state_travels_with_the_checkpoint(ops, project_root, tmp_path):
    import bench
    from src.optim import Lamb

    def build():
        cfg, lit = _lit(LAMB)
        lit.train()
        opt = lit.configure_optimizers()["optimizer"]
        lit.configure_fused(cfg.trainer.accumulate_grad_batches, cfg.trainer.gradient_clip_val)
        return lit, opt
    a, opt = build()
    eng = a.model.engine
    c = eng.cfg
    assert isinstance(opt, Lamb) and (c.optimizer, c.lr, c.weight_decay, c.adam_betas, c.adam_eps, c.clip, c.no_decay_1d) == \
        ("lamb", 1e-3, 0.01, (0.9, 0.999), 1e-6, 1.0, True)
    losses = [float(a.training_step(_mb(bench.synthetic_batch(c, 8, 90 + it, eng.device)), it)) for it in range(2)]
    assert all(math.isfinite(x) for x in losses) and eng.params.step_count == 2
    opt.param_groups[0]["lr"] = 2.5e-4                               # what a scheduler does to the never-stepped carrier
    ck = {"state_dict": a.state_dict()}
    a.on_save_checkpoint(ck)
    path = os.path.join(str(tmp_path), "c.ckpt")
    torch.save(ck, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["fused_adam"]["image"]["step"] == 2 and set(ck["fused_adam"]["image"]) == {"step", "numel", "exp_avg", "exp_avg_sq"}
    r, ropt = build()
    r.load_state_dict(ck["state_dict"]); r.on_load_checkpoint(ck)
    ropt.param_groups[0]["lr"] = 2.5e-4
    er = r._fused_engine()
    assert a._fused_engine().cfg.lr == 2.5e-4 and er.cfg.lr == 2.5e-4
    assert er.params.step_count == 2 and torch.equal(er.params.p32, eng.params.p32) and torch.equal(er.params.m, eng.params.m)
    g = (torch.randn(eng.params.g32.numel(), generator=torch.Generator().manual_seed(1)) * 0.01).to("cuda")
    g[torch.as_tensor(_pad_of(eng.params), device="cuda")] = 0.0
    for e in (a._fused_engine(), er):
        e.params.g32.copy_(g)
        e.optimizer_step()
    torch.cuda.synchronize()
    for k in ("p32", "p16", "m", "v"):
        assert torch.equal(getattr(er.params, k), getattr(eng.params, k)), k
    assert torch.equal(er.params.trust_ratios()[1], eng.params.trust_ratios()[1]) and er.params.step_count == 3


def _pad_of(st):
    mask = torch.ones(st.n_train, dtype=torch.bool)
    for n, o in st.offsets.items():
        if n not in st.groups and o >= st.train_from:
            k = 1
            for d in st.shapes[n]:
                k *= int(d)
            mask[o - st.train_from: o - st.train_from + k] = False
    return mask
