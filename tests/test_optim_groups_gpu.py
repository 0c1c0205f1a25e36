"""The grouped optimiser step on the GPU (medmoe_adam_groups_step, FlatArena.set_param_groups, medmoe_amd/optim_groups.py, the engines and
the Lightning module): bit-identity with medmoe_adam_step where the two compute the same thing, bit-identity per run under power-of-two
multipliers, torch.optim.Adam / AdamW with param_groups at the bars of tests/test_parity2_gpu.py::test_fused_clip_adam_matches_torch_adam
(p, m, v 1e-6 relative L2, the update p - p_prev 1e-4, the bf16 copy exactly the rounded master), every store kind under the rule set of
configs/experiment/pretraining_medmoe_cfg2_adamw.yaml, both engines, deterministic mode, and the module with its checkpoint."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
DEV = "cuda"
BF = torch.bfloat16
# the new experiment's optimiser and rule set
BETAS, EPS, WD, LAYER_DECAY = (0.9, 0.98), 1e-6, 0.05, 0.75


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


@pytest.fixture()
def project_root(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def table(runs):
    """[(end, lr_mult, wd_mult)] -> the device run table."""
    return (torch.tensor([r[0] for r in runs], device=DEV, dtype=torch.int64), torch.tensor([r[1] for r in runs], device=DEV, dtype=torch.float32),
            torch.tensor([r[2] for r in runs], device=DEV, dtype=torch.float32))


class State:
    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.n = n
        self.p = (torch.randn(n, generator=g) * 0.05).to(DEV)
        self.m = torch.zeros(n, device=DEV); self.v = torch.zeros(n, device=DEV)
        self.p16 = torch.zeros(n, device=DEV, dtype=BF)
        self.gen = g

    def clone(self):
        o = State.__new__(State)
        o.n, o.p, o.m, o.v, o.p16 = self.n, self.p.clone(), self.m.clone(), self.v.clone(), self.p16.clone()
        return o

    def same(self, o):
        return all(torch.equal(a, b) for a, b in ((self.p, o.p), (self.m, o.m), (self.v, o.v), (self.p16, o.p16)))


def plain(ops, s, g, lo, hi, lr, wd, step, nsq, clip):
    ops.call("adam_step", s.p[lo:hi], g[lo:hi], s.m[lo:hi], s.v[lo:hi], s.p16[lo:hi], hi - lo, lr, 0.9, 0.999, 1e-8, wd, step, nsq, clip, 1.0)


def grouped(ops, s, g, lo, hi, tab, lr, betas, eps, wd, decoupled, step, nsq, clip):
    ops.call("adam_groups_step", s.p[lo:hi], g[lo:hi], s.m[lo:hi], s.v[lo:hi], s.p16[lo:hi], hi - lo, tab[0], tab[1], tab[2], tab[0].numel(),
             lr, betas[0], betas[1], eps, wd, decoupled, step, nsq, clip, 1.0)


def short_runs(n, count, lo, hi, seed):
    """`count` run lengths in [lo, hi] at the END of [0, n), one long first run in front of them (so the short runs lie in the last sweep of
    a launch that loops), the first boundary at an index that is odd modulo 4; fewer short runs where n is too small for `count`."""
    rs = np.random.RandomState(seed)
    lens = []
    while len(lens) < count and sum(lens) + hi + 3 <= n:
        lens.append(int(rs.randint(lo, hi + 1)))
    first = n - sum(lens)
    if lens and first % 4 != 3 and first % 4 != 1:
        lens[0] += 1; first -= 1                                    # first is now odd
    ends = np.cumsum([first] + lens).tolist()
    assert ends[-1] == n and all(b > a for a, b in zip(ends, ends[1:]))
    return [(e, 1.0, 1.0) for e in ends]


SWEEP = 2048 * 256 * 4                                              # elements one grid-stride sweep of the launch covers


# ---- 1. bit-identity with the plain kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [0.25, 0.0], ids=["clip", "noclip"])
@pytest.mark.parametrize("n", [8, 4096 + 8, SWEEP + (1 << 20) + 40])
@pytest.mark.parametrize("case", ["one", "many", "searched"])
def test_grouped_step_with_unit_multipliers_is_the_plain_step(ops, n, case, clip):
    """decoupled = 0, default betas / eps, all multipliers (1, 1): p, m, v and the bf16 copy equal medmoe_adam_step's bit for bit over three
    steps.  one: one run; many: ~700 runs of 3..64 elements (3..8 at the small size) with boundaries off the multiples of 4 - more runs
    than a workgroup has threads, staged in LDS; searched: ~1500 runs of 1..4 elements, more than the LDS table holds (1024), so the table
    is searched in global memory.  n: one float4 pair; more than one block; more than one grid-stride sweep (the loop and a partial last sweep)."""
    if case == "one":
        runs = [(n, 1.0, 1.0)]
    elif n == 8:                                                    # both float4s straddle a boundary; runs of one element
        runs = [(e, 1.0, 1.0) for e in ((3, 8) if case == "many" else (1, 2, 3, 7, 8))]
    elif case == "many":
        runs = short_runs(n, 700, 3, 64 if n > SWEEP else 8, 1)
        assert n < 100 or len(runs) > 600
        assert any(r[0] % 4 for r in runs[:-1]) or n < 100
    else:
        runs = short_runs(n, 1500, 1, 4, 2)
        assert n < 100 or len(runs) > 1024
    tab = table(runs)
    a = State(n, 0); b = a.clone()
    nsq = torch.zeros(1, device=DEV)
    for step in range(1, 4):
        g = (torch.randn(n, generator=a.gen) * (1.0 + step)).to(DEV)
        nsq.copy_((g.double() ** 2).sum().float())
        plain(ops, a, g, 0, n, 5e-5, 0.01, step, nsq, clip)
        grouped(ops, b, g, 0, n, tab, 5e-5, (0.9, 0.999), 1e-8, 0.01, 0, step, nsq, clip)
        assert a.same(b), (case, n, step)
    assert float((a.p16.float() - a.p).abs().max()) > 0 and torch.equal(b.p16, b.p.to(BF))


def test_argument_checks(ops):
    s = State(8, 0)
    tab = table([(8, 1.0, 1.0)])
    g = torch.zeros(8, device=DEV)
    ok = dict(p=s.p, g=g, m=s.m, v=s.v, n=8, ends=tab[0], lr=tab[1], wd=tab[2], n_runs=1, step=1)

    def rc(**kw):
        a = dict(ok, **kw)
        ptr = lambda t: None if t is None else t.data_ptr()
        f = ops._fn("adam_groups_step")
        return f(ptr(a["p"]), ptr(a["g"]), ptr(a["m"]), ptr(a["v"]), s.p16.data_ptr(), a["n"], ptr(a["ends"]), ptr(a["lr"]), ptr(a["wd"]), a["n_runs"],
                 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, a["step"], None, 0.0, 1.0, ops.current_stream_handle())
    assert rc() == 0
    bad = {rc(p=None), rc(g=None), rc(m=None), rc(v=None), rc(ends=None), rc(lr=None), rc(wd=None), rc(n_runs=0), rc(step=0), rc(n=6)}
    assert 0 not in bad
    assert rc(n=6) != rc(step=0)                                     # MM_ERR_SHAPE against MM_ERR_ARG
    torch.cuda.synchronize()


# ---- 2. bit-identity per run with power-of-two multipliers --------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [0, 1])
def test_grouped_step_equals_one_launch_per_run(ops, decoupled):
    """8-aligned runs, lr_mult in {1, 1/2, 1/4}, wd_mult in {0, 1}, weight_decay > 0: the grouped launch equals one launch per run with
    lr * lr_mult and weight_decay * wd_mult (scaling by a power of two commutes with every rounding).  decoupled = 0: against
    medmoe_adam_step per run; decoupled = 1: against one-run launches of the new entry point."""
    rs = np.random.RandomState(5)
    runs, end = [], 0
    for i in range(40):
        end += 8 * int(rs.randint(1, 40))
        runs.append((end, (1.0, 0.5, 0.25)[i % 3], float((i // 3) % 2)))
    n = end
    assert n > 2048 and {r[1:] for r in runs} == {(l, w) for l in (1.0, 0.5, 0.25) for w in (0.0, 1.0)}
    tab = table(runs)
    lr, wd, clip = 1e-3, 0.05, 0.25
    a = State(n, 1); b = a.clone()
    nsq = torch.zeros(1, device=DEV)
    for step in range(1, 4):
        g = (torch.randn(n, generator=a.gen) * step).to(DEV)
        nsq.copy_((g.double() ** 2).sum().float())
        grouped(ops, a, g, 0, n, tab, lr, (0.9, 0.999), 1e-8, wd, decoupled, step, nsq, clip)
        lo = 0
        for hi, lm, wm in runs:
            if decoupled:
                grouped(ops, b, g, lo, hi, table([(hi - lo, 1.0, 1.0)]), lr * lm, (0.9, 0.999), 1e-8, wd * wm, 1, step, nsq, clip)
            else:
                plain(ops, b, g, lo, hi, lr * lm, wd * wm, step, nsq, clip)
            lo = hi
        assert a.same(b), (decoupled, step)


# ---- 3. against torch ---------------------------------------------------------------------------------------------------------------------
def torch_optimizer(params, mults, decoupled, lr, wd, betas, eps):
    """torch.optim.Adam / AdamW over `params` (name -> Parameter) with one param_group per distinct (lr_mult, wd_mult) of `mults`."""
    by = {}
    for n, p in params.items():
        by.setdefault(tuple(mults.get(n, (1.0, 1.0))), []).append(p)
    groups = [{"params": ps, "lr": lr * lm, "weight_decay": wd * wm} for (lm, wm), ps in by.items()]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    return cls(groups, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)


def check_against_torch(stores, mults, decoupled, lr, wd, betas, eps, clip, steps, seed, step_fn=None, plant=True):
    """stores: [arena]; mults: per arena name -> (lr_mult, wd_mult) as the TEST states them.  Plants seeded gradients (or takes the ones the
    arenas hold), steps every arena with one clip norm over all of them, and compares every named entry with torch at the bars above."""
    from medmoe_amd.optim_groups import entry_names
    gen = torch.Generator().manual_seed(seed)
    ref = [{n: torch.nn.Parameter(st.f32(n).detach().clone()) for n in entry_names(st)} for st in stores]
    opt = torch_optimizer({(i, n): p for i, r in enumerate(ref) for n, p in r.items()}, {(i, n): v for i, ms in enumerate(mults) for n, v in ms.items()},
                          decoupled, lr, wd, betas, eps)
    allp = [p for r in ref for p in r.values()]
    for step in range(steps):
        prev = [st.p32.clone() for st in stores]
        for st, r in zip(stores, ref):
            if plant:
                st.zero_grad()                                      # the padding carries no gradient
                for n, p in r.items():
                    st.grad(n).copy_((torch.randn(p.shape, generator=gen) * (0.02 * (1 + step))).to(DEV))
            for n, p in r.items():
                p.grad = st.grad(n).detach().clone()
        if clip > 0:
            torch.nn.utils.clip_grad_norm_(allp, clip)
        opt.step()
        if step_fn is not None:
            step_fn()
        else:
            total = stores[0].sumsq()
            for st in stores[1:]:
                total.add_(st.sumsq())
            for st in stores:
                st.adam_step(total, lr, wd, clip, betas=betas, eps=eps, decoupled=bool(decoupled))
        for st, r, pv in zip(stores, ref, prev):
            m, v = st.adam_state()
            for n, p in r.items():
                got, was = st.f32(n), st.view(pv, n)
                assert rel(got, p.detach()) < 1e-6, (n, step, rel(got, p.detach()))
                assert rel(got - was, p.detach() - was) < 1e-4, (n, step, rel(got - was, p.detach() - was))
                assert rel(st.view(m, n), opt.state[p]["exp_avg"]) < 1e-6, (n, step)
                assert rel(st.view(v, n), opt.state[p]["exp_avg_sq"]) < 1e-6, (n, step)
            assert torch.equal(st.p16, st.p32.to(BF))


@pytest.mark.parametrize("clip", [0.25, 0.0], ids=["clip", "noclip"])
@pytest.mark.parametrize("decoupled", [0, 1], ids=["adam", "adamw"])
def test_three_param_groups_match_torch(ops, decoupled, clip):
    """torch.optim.Adam / AdamW with three param_groups (decay, no decay, lr x 0.1), betas (0.9, 0.98), eps 1e-6, three steps.  The arena
    group `ab` stores a (3 elements) and b (5 elements) back to back: the boundary between the no-decay run and the decayed one is element 3."""
    from medmoe_amd.flat import FlatArena
    g = torch.Generator().manual_seed(7)
    ar = FlatArena(DEV, [("c", (37,)), ("a", (3,)), ("d", (66, 7)), ("b", (5,)), ("e", (129,)), ("f", (300, 5))], groups=[("ab", ["a", "b"])])
    for n in ("a", "b", "c", "d", "e", "f"):
        ar.f32(n).copy_((torch.randn(ar.shapes[n], generator=g) * 0.05).to(DEV))
    ar.refresh()
    mults = {"a": (1.0, 0.0), "c": (1.0, 0.0), "e": (0.1, 1.0), "f": (0.1, 1.0)}
    ar.set_param_groups(mults)
    assert ar.runs[0][0] == 3 and len(ar.runs) == 5
    check_against_torch([ar], [mults], decoupled, 1e-3, WD, BETAS, EPS, clip, 3, 11)
    d0 = ar.f32("d").clone()
    ar.zero_grad()
    ar.adam_step(ar.sumsq(), 1e-3, WD, clip, betas=BETAS, eps=EPS, decoupled=bool(decoupled))
    assert not torch.equal(ar.f32("d"), d0)                         # zero gradient: the decayed group still moves (decay, momentum)


# ---- 4. stores ----------------------------------------------------------------------------------------------------------------------------
def expected_mults(kind, names, shapes):
    """The rule set of the new experiment (no_decay_1d, layer_decay 0.75) restated: name -> (lr_mult, wd_mult)."""
    out = {}
    if kind == "vit":
        L = 1 + max(int(n.split(".")[2]) for n in names if n.startswith("vit.layer."))
    elif kind == "text":
        L = 1 + max(int(n.split(".")[1]) for n in names if n.startswith("layer."))
    elif kind == "swin_tower":
        blocks = sorted({tuple(int(x) for x in re.findall(r"\d+", n)[:2]) for n in names if ".blocks." in n})
        L = len(blocks)
    for n in names:
        if kind == "vit":
            depth = int(n.split(".")[2]) + 1 if n.startswith("vit.layer.") else (0 if n.startswith(("vit.patch_embed", "vit.cls", "vit.pos")) else L + 1)
        elif kind == "text":
            depth = int(n.split(".")[1]) + 1 if n.startswith("layer.") else 0
        elif kind == "swin_tower":
            if ".blocks." in n:
                depth = blocks.index(tuple(int(x) for x in re.findall(r"\d+", n)[:2])) + 1
            elif ".downsample." in n:
                stage = int(re.findall(r"\d+", n)[0])
                depth = max(i + 1 for i, b in enumerate(blocks) if b[0] == stage)
            else:
                depth = 0 if n.startswith("embeddings.") else L + 1
        else:
            L, depth = 0, 1
        one_d = len(shapes[n]) == 1 or n.endswith(".bias") or n in ("vit.cls_token", "vit.pos_embed", "position_embeddings", "token_type_embeddings") \
            or n.endswith("relative_position_bias_table")
        out[n] = (LAYER_DECAY ** (L + 1 - depth), 0.0 if one_d else 1.0)
    return out


def _layout_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("record_store_layouts", os.path.join(ROOT, "tools", "record_store_layouts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _build_store(label):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.flat import FlatStore
    from medmoe_amd.params import ParamStore
    from medmoe_amd.pyramid import GroupedPyramidExperts
    from medmoe_amd.swin import SwinTower
    from medmoe_amd.text_params import TextStore
    tool = _layout_tool()
    g = torch.Generator().manual_seed(3)
    if label.startswith("ParamStore:"):
        return "vit", ParamStore(config_by_name(label.split(":")[1]), DEV)
    if label == "TextStore":
        cfg = config_by_name("tiny")
        return "text", TextStore(cfg, DEV, ParamStore(cfg, DEV).text)
    if label == "swin_tower":
        w = {k: torch.randn(v.shape, generator=g) * 0.05 for k, v in tool.swin_tiny_weights().items()}
        return "swin_tower", SwinTower(w, DEV, **tool.SWIN_TINY).store
    z = np.load(os.path.join(ROOT, "tests", "golden", "expert_pyramid_mfma.npz"))
    E = 3
    allw = {f"moe.experts.{e}.{k}": torch.from_numpy(z[k]) + 0.01 * e for e in range(E) for k in z.files if k.startswith(("proj_convs", "attn_proj"))}
    gemm = [f"moe.experts.{e}.proj_convs.{s}.0.weight" for e in range(E) for s in range(4)] + [f"moe.experts.{e}.attn_proj.0.weight" for e in range(E)]
    return "swin_moe", FlatStore(allw, DEV, groups=GroupedPyramidExperts.groups(E), gemm=gemm)


@pytest.mark.parametrize("label", ["ParamStore:tiny", "ParamStore:tinyL8mx", "TextStore", "swin_tower", "swin_moe"])
def test_stores_under_the_experiment_rules_match_torch_adamw(ops, label):
    from medmoe_amd.optim_groups import GroupRules, apply_rules, entry_names
    kind, st = _build_store(label)
    g = torch.Generator().manual_seed(5)
    for n in entry_names(st):                                      # biases start at zero: give every entry a value of its own
        if float(st.f32(n).abs().max()) == 0.0:
            st.f32(n).copy_((torch.randn(st.shapes[n], generator=g) * 0.05).to(DEV))
    st.refresh()
    apply_rules({kind: st}, GroupRules(no_decay_1d=True, layer_decay=LAYER_DECAY))
    names = entry_names(st)
    mults = expected_mults(kind, names, st.shapes)
    assert len(st.runs) > 1 and st.runs[-1][0] == st.numel
    check_against_torch([st], [mults], 1, 1e-3, WD, BETAS, EPS, 0.25, 2, 13)
    # the working copies follow the grouped step as they follow the plain one
    assert torch.equal(st.p16, st.p32.to(BF))
    assert st.tr_table is not None
    for n in st._mat:
        assert torch.equal(st.w16t(n), st.w16(n).transpose(-1, -2)), n
    if label == "ParamStore:tinyL8mx":
        assert len(st.fp8) == 5
        for n, copies in st.fp8.items():
            fresh = [torch.zeros_like(c) for c in copies]
            E, N, K = st.shapes[n]
            ops.call("quant_weights_mx", st.f32(n), *fresh, E, N, K)
            assert all(torch.equal(a, b) for a, b in zip(copies, fresh)), n
            assert int(copies[0].count_nonzero()) > 0


# ---- 5. engines ---------------------------------------------------------------------------------------------------------------------------
def _experiment_cfg(name, freeze_text):
    from medmoe_amd.config import config_by_name
    cfg = config_by_name(name)
    cfg.freeze_text = freeze_text
    cfg.optimizer, cfg.adam_betas, cfg.adam_eps, cfg.weight_decay, cfg.lr = "adamw", BETAS, EPS, WD, 1e-3
    cfg.no_decay_1d, cfg.layer_decay = True, LAYER_DECAY
    return cfg


def test_engine_optimizer_step_matches_torch_adamw(ops):
    """Engine (tiny, trainable text tower): the gradients of a real backward, ONE clip norm over both stores, the grouped AdamW step of each."""
    import bench
    from medmoe_amd.engine import Engine
    from medmoe_amd.optim_groups import entry_names
    cfg = _experiment_cfg("tiny", False)
    eng = Engine(cfg, "cuda:0", seed=0)
    assert eng.params.runs is not None and eng.tstore.runs is not None
    eng.train_step(bench.synthetic_batch(cfg, 8, 21, eng.device), optimizer=False)
    stores = [eng.params, eng.tstore]
    mults = [expected_mults("vit", entry_names(eng.params), eng.params.shapes), expected_mults("text", entry_names(eng.tstore), eng.tstore.shapes)]
    check_against_torch(stores, mults, 1, cfg.lr, WD, BETAS, EPS, cfg.clip, 1, 0, step_fn=eng.optimizer_step, plant=False)
    assert eng.params.step_count == 1 and eng.tstore.step_count == 1


def test_swin_engine_optimizer_step_matches_torch_adamw(ops, project_root):
    from medmoe_amd.hydra_lite import compose, instantiate
    from medmoe_amd.optim_groups import entry_names
    import bench
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe", "model.model.vision.arch=swin_t", "model.optimizer.lr=0.001",
                                          "model.fused_step=true", "model.optimizer._target_=torch.optim.AdamW", "model.optimizer.weight_decay=0.05",
                                          "+model.optimizer.betas=[0.9,0.98]", "+model.optimizer.eps=0.000001",
                                          "+model.optimizer_groups.no_decay_1d=true", "+model.optimizer_groups.layer_decay=0.75"])
    lit = instantiate(cfg.model)
    lit.model.swin.drop_path_rate = 0.0
    lit.train(); lit.configure_optimizers(); lit.configure_fused(1, 0.25)
    sw = lit._fused_engine()
    c = sw.cfg
    assert (c.optimizer, c.adam_betas, c.adam_eps, c.weight_decay, c.no_decay_1d, c.layer_decay) == ("adamw", BETAS, EPS, WD, True, LAYER_DECAY)
    st_t, st_m = sw.enc.tower.store, sw.enc.store
    assert len(st_t.runs) > 24 and len(st_m.runs) > 1
    b = bench.synthetic_batch(lit.model.cfg, 8, 40, lit.model.device)
    b["label"] = b["label"] % lit.model.cfg.n_expert
    sw.train_step(b, optimizer=False)
    mults = [expected_mults("swin_tower", entry_names(st_t), st_t.shapes), expected_mults("swin_moe", entry_names(st_m), st_m.shapes)]
    assert min(v[0] for v in mults[0].values()) == LAYER_DECAY ** 13
    check_against_torch([st_t, st_m], mults, 1, c.lr, WD, BETAS, EPS, 0.25, 1, 0, step_fn=sw.optimizer_step, plant=False)


def test_deterministic_mode_keeps_its_promise_over_the_grouped_step(ops, monkeypatch):
    import bench
    from medmoe_amd.engine import Engine
    monkeypatch.setenv("MEDMOE_DETERMINISTIC", "1")
    cfg = _experiment_cfg("tiny2", True)
    batches = [bench.synthetic_batch(cfg, 8, 50 + i, "cuda:0") for i in range(2)]

    def run():
        eng = Engine(_experiment_cfg("tiny2", True), "cuda:0", seed=3)
        assert eng.deterministic and eng.params.runs is not None
        eng.train_step(batches[0], optimizer=False)
        torch.cuda.synchronize()
        before = ops.nondet_launches()
        eng.optimizer_step()
        torch.cuda.synchronize()
        assert ops.nondet_launches() == before
        eng.train_step(batches[1])
        torch.cuda.synchronize()
        assert ops.nondet_launches() == before
        m, v = eng.params.adam_state()
        return [eng.params.p32.clone(), m.clone(), v.clone(), eng.params.p16.clone()]
    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 6. module ----------------------------------------------------------------------------------------------------------------------------
def _lit(overrides):
    from medmoe_amd.hydra_lite import compose, instantiate
    cfg = compose(CONFIGS, "train.yaml", overrides)
    return cfg, instantiate(cfg.model)


def _mb(b):
    return {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"]}}


ADAMW = ["experiment=pretraining_medmoe_cfg2_adamw", "model.model.vision.config_name=tiny2", "model.optimizer.lr=0.001"]


def test_new_experiment_builds_the_fused_module_and_trains(ops, project_root):
    import bench
    cfg, lit = _lit(ADAMW)
    assert lit.fused_step
    lit.configure_optimizers(); lit.configure_fused(cfg.trainer.accumulate_grad_batches, cfg.trainer.gradient_clip_val)
    eng = lit.model.engine
    c = eng.cfg
    assert (c.optimizer, c.adam_betas, c.adam_eps, c.weight_decay, c.lr, c.clip) == ("adamw", BETAS, EPS, WD, 1e-3, 0.25)
    assert (c.no_decay, c.no_decay_1d, c.text_lr_mult, c.layer_decay) == ((), True, 1.0, LAYER_DECAY)
    assert eng.params.runs is not None and min(r[1] for r in eng.params.runs) == LAYER_DECAY ** (c.n_layer_v + 1)
    b = bench.synthetic_batch(c, 8, 21, eng.device)
    l0 = float(lit.training_step(_mb(b), 0))
    l1 = float(lit.training_step(_mb(b), 1))
    assert np.isfinite(l0) and np.isfinite(l1) and l1 < l0, (l0, l1)
    assert eng.params.step_count == 2


def test_optimizer_overrides_reach_the_engine_and_groups_need_the_fused_step(ops, project_root):
    base = ["experiment=pretraining_medmoe_cfg2", "model.model.vision.config_name=tiny2"]
    _, lit = _lit(base + ["model.optimizer._target_=torch.optim.AdamW", "+model.optimizer.betas=[0.85,0.95]", "+model.optimizer.eps=0.00001"])
    c = lit.model.engine.cfg
    assert (c.optimizer, c.adam_betas, c.adam_eps, c.weight_decay) == ("adamw", (0.85, 0.95), 1e-5, 0.0) and lit.model.engine.params.runs is None
    _, lit = _lit(base + ["+model.optimizer.betas=[0.9,0.98]"])
    assert (lit.model.engine.cfg.optimizer, lit.model.engine.cfg.adam_betas) == ("adam", (0.9, 0.98))
    _, lit = _lit(base)
    c = lit.model.engine.cfg
    assert (c.optimizer, c.adam_betas, c.adam_eps) == ("adam", (0.9, 0.999), 1e-8) and lit.model.engine.params.runs is None
    with pytest.raises(NotImplementedError, match="optimizer_groups"):
        _lit(["experiment=pretraining_medmoe", "model.model.vision.config_name=tiny2", "+model.optimizer_groups.no_decay_1d=true"])
    with pytest.raises(ValueError, match="vit.layr"):
        _lit(base + ["+model.optimizer_groups.no_decay=[vit.layr.*]"])


def test_checkpoint_round_trip_continues_the_grouped_optimisation_bit_for_bit(ops, project_root, tmp_path):
    """Save after step 2, reload into a fresh module (the groups come from its config, m / v / the step count from the checkpoint): a third
    optimiser step on identical planted gradients equals the uninterrupted module's bit for bit."""
    import bench

    def build():
        _, lit = _lit(ADAMW)
        lit.train(); lit.configure_optimizers(); lit.configure_fused(1, 0.25)
        return lit
    a = build()
    eng = a.model.engine
    for it in range(2):
        a.training_step(_mb(bench.synthetic_batch(eng.cfg, 8, 90 + it, eng.device)), it)
    ck = {"state_dict": a.state_dict()}
    a.on_save_checkpoint(ck)
    path = os.path.join(str(tmp_path), "c.ckpt")
    torch.save(ck, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["fused_adam"]["image"]["step"] == 2 and "runs" not in ck["fused_adam"]["image"]
    r = build()
    r.load_state_dict(ck["state_dict"]); r.on_load_checkpoint(ck)
    er = r._fused_engine()
    assert er.params.runs == eng.params.runs and er.params.step_count == 2
    assert torch.equal(er.params.p32, eng.params.p32) and torch.equal(er.params.m, eng.params.m) and torch.equal(er.params.v, eng.params.v)
    g = (torch.randn(eng.params.numel, generator=torch.Generator().manual_seed(1)) * 0.01).to(DEV)
    for e in (a._fused_engine(), er):
        e.params.g32.copy_(g)
        e.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(er.params.p32, eng.params.p32) and torch.equal(er.params.p16, eng.params.p16)
    assert torch.equal(er.params.m, eng.params.m) and torch.equal(er.params.v, eng.params.v) and er.params.step_count == 3
