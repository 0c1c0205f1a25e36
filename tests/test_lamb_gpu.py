"""The three LAMB launches on the GPU (csrc/lamb.hip through FlatArena.lamb_step) on hand-built arenas, against the float64
restatement of tests/lamb_reference.py on the same fp32 inputs.  The bars are derived, not tuned, and printed with the measured value as
`[bar]` lines:
  segment sums of squares   relative (K + D + 4) 2^-24 - all terms are non-negative; K = the longest chain of sequential additions (a
                            moments thread adds chunk / threads squares, a ratios lane ceil(records / lanes) records), D = the depth of the
                            trees behind them (wave xor tree + the four waves, then the ratios wave's xor tree); from the library's queries
  r_s                       that bar + 3 2^-24 (two square roots and a division)
  m, v                      1e-6 relative L2, the bar of the Adam kernel tests (tests/test_optim_groups_gpu.py)
  p_new, per element        |err| <= 2^-24 |p_ref| + lr lr_mult r_ref (|a| + |wd p|) (bar_r + 8 2^-24)
The clip coefficient is, by the update's definition, formed in fp32 as the Adam launches form it: the restatement takes the value the launch
used (FlatArena.last_clip_coef) as the fp32 input it is, after holding it against the float64 formula (lamb_reference.device_coef).
Exact properties are checked with torch.equal."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lamb_reference as R                                           # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
U24 = 2.0 ** -24
LR, WD, BETAS, EPS = 1e-2, 0.01, (0.9, 0.999), 1e-6


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


def _weights(ops, long_entry: bool):
    """name -> fp32 CPU tensor.  Sizes 1, 7, 8, 9, 255, 256, 257, 4096, 4097 around the float4 / block / chunk edges, a group alias of three
    members stored back to back (7 + 9 + 255: boundaries off every multiple of 4), an all-zero tensor, a tensor whose gradient stays zero,
    and one entry of three chunks and a bit - or, long_entry, longer than one pass of either launch's grid (2048 workgroups)."""
    C = ops.lamb_chunk()
    big = 2048 * C + 3 * C + 17 if long_entry else 3 * C + 17
    g = torch.Generator().manual_seed(11)
    sizes = {"s1": 1, "g7": 7, "g9": 9, "g255": 255, "s8": 8, "s256": 256, "s257": 257, "s4096": 4096, "s4097": 4097, "zero": 40, "nograd": 33,
             "big": big, "tail": 5}
    w = {n: torch.randn(k, generator=g) * 0.05 for n, k in sizes.items()}
    w["zero"].zero_()
    w["s4096"] *= 40.0                                               # a large-norm tensor: r > 1
    return w


GROUPS = [("g", ["g7", "g9", "g255"])]
# two runs and more with different (lr_mult, wd_mult); `nograd` has no decay and no gradient: u = 0, r = 1, p stays
ASSIGN = {"g9": (0.5, 0.0), "s256": (0.25, 1.0), "s257": (0.25, 1.0), "nograd": (1.0, 0.0), "s1": (2.0, 1.0), "tail": (1.0, 0.0)}


def _store(ops, w, seed=0, state=False):
    """A fresh FlatStore of `w` with the groups and the assignment above, gradients drawn from `seed` (norm >> 1: a clip of 1 is active), and,
    state: random moments as after many steps."""
    from medmoe_amd.flat import FlatStore
    st = FlatStore(w, DEV, groups=GROUPS)
    st.set_param_groups(ASSIGN)
    g = torch.Generator().manual_seed(100 + seed)
    for n in st.names:
        if n != "nograd":
            st.grad(n).copy_((torch.randn(w[n].numel(), generator=g) * 0.3).to(DEV))
    m, v = st.adam_state()
    if state:
        for n in st.names:
            if n != "nograd":
                st.view(m, n).copy_((torch.randn(w[n].numel(), generator=g) * 0.1).to(DEV))
                st.view(v, n).copy_((torch.rand(w[n].numel(), generator=g) * 0.02).to(DEV))
    return st


def _snapshot(st):
    return {k: getattr(st, k).detach().cpu().clone() for k in ("p32", "g32", "m", "v")}


def _pad_mask(st):
    """True on the alignment padding of the trainable tail: what lies between a tensor's last element and the next entry."""
    mask = torch.ones(st.n_train, dtype=torch.bool)
    for n, o in st.offsets.items():
        if n not in st.groups and o >= st.train_from:
            k = 1
            for d in st.shapes[n]:
                k *= int(d)
            mask[o - st.train_from: o - st.train_from + k] = False
    return mask


def _expected_table(st):
    """Segment ends and multipliers of a store without stacked entries, from st.offsets and st.runs alone: a segment runs from its entry's
    offset to the next entry's (the last to numel), relative to the trainable tail; its multipliers are those of the run its first element lies in."""
    tf = st.train_from
    offs = sorted(o for n, o in st.offsets.items() if n not in st.groups and o >= tf)
    ends = [o - tf for o in offs[1:]] + [st.numel - tf]
    runs = st.runs if st.runs is not None else [(st.numel, 1.0, 1.0)]
    mult = [next((lm, wm) for end, lm, wm in runs if o < end) for o in offs]
    return (torch.tensor(ends, dtype=torch.int64), torch.tensor([m[0] for m in mult], dtype=torch.float32),
            torch.tensor([m[1] for m in mult], dtype=torch.float32))


def _sum_bars(ops, st):
    C = ops.lamb_chunk()
    T, RT = ops.lamb_sum_shape()
    ends = [0] + [e for _, e in st.segments()]
    recs = max((b - 1) // C - a // C + 1 for a, b in zip(ends, ends[1:]) if b > a)
    K = C // T + -(-recs // RT)
    D = int(math.log2(64)) + int(math.log2(T // 64)) + int(math.log2(RT))
    return R.sum_bar(K, D), K, D


def _check(ops, st, before, t, *, clip, always_adapt, trust_clip, grad_scale=1.0, label=""):
    """Everything of one step against the restatement; `before`: the snapshot the step started from."""
    tf = st.train_from
    segs = st.segments()
    ends, lrm, wdm = _expected_table(st)                            # from the layout and the run list, not from the table under test
    dev = [x.cpu() for x in st._seg_table]
    assert dev[0].tolist() == ends.tolist() and torch.equal(dev[1], lrm) and torch.equal(dev[2], wdm)
    normsq = float(st.normsq)
    coef = R.device_coef(st, normsq, clip, grad_scale, label)       # the fp32 coefficient the launch used: an input of the restatement
    ref = R.lamb_arena(before["p32"][tf:], before["g32"], before["m"], before["v"], t, ends.tolist(), lrm.tolist(), wdm.tolist(), lr=LR, wd=WD,
                       betas=BETAS, eps=EPS, coef=coef, always_adapt=always_adapt, trust_clip=trust_clip)
    S = len(segs)
    out = st._lamb_ratios.cpu().double()
    names, r_dev = st.trust_ratios()
    assert names == [n for n, _ in segs] and torch.equal(r_dev.cpu().double(), out[:S])
    r, sums = out[:S], out[S:].view(S, 2)
    bar_s, K, D = _sum_bars(ops, st)
    bar_r = bar_s + 3 * U24
    worst_s = worst_r = 0.0
    ones = 0
    for k, (name, _) in enumerate(segs):
        for j, want in enumerate((ref["wn2"][k], ref["un2"][k])):
            got = float(sums[k, j])
            if want == 0.0:
                assert got == 0.0, (label, name, j)
            else:
                worst_s = max(worst_s, abs(got - want) / want)
        want_r = ref["r"][k]
        rule_one = ref["wn2"][k] == 0.0 or ref["un2"][k] == 0.0 or not (always_adapt or float(wdm[k]) * WD != 0.0)
        if rule_one:
            assert float(r[k]) == 1.0, (label, name)                 # exactly 1 where the rule says 1
            ones += 1
        else:
            worst_r = max(worst_r, abs(float(r[k]) - want_r) / want_r)
    print(f"[bar] {label} t={t} segment sums: rel err {worst_s:.3e} <= {bar_s:.3e} (K={K}, D={D})")
    print(f"[bar] {label} t={t} trust ratios: rel err {worst_r:.3e} <= {bar_r:.3e} ({ones} of {S} exactly 1)")
    assert worst_s <= bar_s and worst_r <= bar_r and ones >= 1
    p, m, v = st.p32[tf:].cpu().double(), st.m.cpu().double(), st.v.cpu().double()
    for nm, got, want in (("m", m, ref["m"]), ("v", v, ref["v"])):
        e = float((got - want).norm() / want.norm().clamp_min(1e-300))
        print(f"[bar] {label} t={t} {nm}: rel L2 {e:.3e} <= 1e-6")
        assert e <= 1e-6, (label, nm)
    tol = U24 * ref["p"].abs() + ref["step"] * (ref["a"].abs() + ref["wdp"].abs()) * (bar_r + 8 * U24)
    err = (p - ref["p"]).abs()
    ratio = float((err / tol.clamp_min(1e-300))[tol > 0].max())
    print(f"[bar] {label} t={t} p_new: max |err| / bar {ratio:.3f} <= 1 (max |err| {float(err.max()):.3e})")
    assert bool((err <= tol).all()), (label, float((err - tol).max()))
    _exact(st)
    assert float((p - before["p32"][tf:].double()).abs().max()) > 0.0
    return ref


def _exact(st):
    tf = st.train_from
    assert torch.equal(st.p16, st.p32.to(BF))
    pad = _pad_mask(st).to(DEV)
    assert bool(pad.any())
    for buf in (st.p32[tf:], st.m, st.v, st.g32):
        assert float(buf[pad].abs().max()) == 0.0                    # the padding is still exactly zero
    for buf in (st.p32, st.m, st.v, st._lamb_ratios, st.p16.float()):
        assert bool(torch.isfinite(buf).all())


@pytest.fixture(scope="module")
def weights(ops):
    return _weights(ops, False)


FLAGS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("clip", [1.0, 1e9], ids=["clip", "noclip"])
@pytest.mark.parametrize("always_adapt,trust_clip", FLAGS, ids=["plain", "adapt", "tclip", "adapt+tclip"])
def test_steps_one_two_and_a_thousand(ops, weights, always_adapt, trust_clip, clip):
    kw = dict(betas=BETAS, eps=EPS, always_adapt=always_adapt, trust_clip=trust_clip)
    nondet = ops.nondet_launches()
    st = _store(ops, weights)
    assert len(st.segments()) == len(weights) and st.runs is not None and len(st.runs) >= 5
    for t in (1, 2):
        before = _snapshot(st)
        st.lamb_step(st.sumsq(), LR, WD, clip, **kw)
        assert st.step_count == t
        ref = _check(ops, st, before, t, clip=clip, always_adapt=always_adapt, trust_clip=trust_clip, label="small")
        if clip == 1.0:
            assert R.clip_coef(float(st.normsq), clip) < 0.5         # the clip is active
        if trust_clip:
            assert max(ref["r"]) <= 1.0
        elif t == 1:
            assert max(ref["r"]) > 1.0
        st.g32.mul_(0.5)                                             # another gradient for the next step (the padding stays zero)
    st = _store(ops, weights, seed=1, state=True)
    st.step_count = 999
    before = _snapshot(st)
    st.lamb_step(st.sumsq(), LR, WD, clip, **kw)
    _check(ops, st, before, 1000, clip=clip, always_adapt=always_adapt, trust_clip=trust_clip, label="small")
    assert ops.nondet_launches() == nondet


def test_an_entry_longer_than_one_pass_of_the_grid(ops):
    w = _weights(ops, True)
    st = _store(ops, w, seed=2, state=True)
    assert w["big"].numel() > 2048 * ops.lamb_chunk()
    st.step_count = 4
    before = _snapshot(st)
    st.lamb_step(st.sumsq(), LR, WD, 1.0, 0.5, betas=BETAS, eps=EPS)
    _check(ops, st, before, 5, clip=1.0, always_adapt=False, trust_clip=False, grad_scale=0.5, label="long")


@pytest.mark.parametrize("form", ["fp32", "g16+ema"])
def test_more_segments_than_the_lds_table_holds(ops, form):
    """About 1500 entries of 1 .. 4 elements (padded to 8 each) and a group of 40 one-to-four-element members stored back to back: more than
    the 1024 segments the launches stage in LDS, so the moments and the applying launch search the tables in global memory - in the fp32 /
    plain forms and in the bf16-gradient / EMA forms.  One chunk meets several hundred segments."""
    from medmoe_amd.ema import one_minus_decay
    from medmoe_amd.flat import FlatStore
    g = torch.Generator().manual_seed(21)
    w = {f"e{i}": torch.randn(1 + i % 4, generator=g) * 0.05 for i in range(1500)}
    members = [f"m{i}" for i in range(40)]
    w.update({n: torch.randn(1 + (3 * i) % 4, generator=g) * 0.05 for i, n in enumerate(members)})
    w["e7"].zero_()
    st = FlatStore(w, DEV, groups=[("grp", members)])
    st.set_param_groups({f"e{i}": ((0.5, 0.0) if i % 3 == 0 else (0.25, 1.0)) for i in range(0, 1500, 2)})
    assert len(st.segments()) == 1540 > 1024
    for n in st.names:
        st.grad(n).copy_((torch.randn(w[n].numel(), generator=g) * 0.3).to(DEV))
    m, v = st.adam_state()
    for n in st.names:
        st.view(m, n).copy_((torch.randn(w[n].numel(), generator=g) * 0.1).to(DEV))
        st.view(v, n).copy_((torch.rand(w[n].numel(), generator=g) * 0.02).to(DEV))
    kw = dict(betas=BETAS, eps=EPS, always_adapt=True)
    if form != "fp32":
        st.g16.copy_(st.g32.to(BF)); st.g32.copy_(st.g16.float())
        st.enable_ema(); st.e32.mul_(0.9)
        kw["ema_decay"] = 0.99
    st.step_count = 2
    before = _snapshot(st)
    e0 = st.e32.clone() if form != "fp32" else None
    total = st.sumsq()
    if form != "fp32":
        st.g16_reduced = True
    st.lamb_step(total, LR, WD, 1.0, **kw)
    _check(ops, st, before, 3, clip=1.0, always_adapt=True, trust_clip=False, label=f"searched tables, {form}")
    if form != "fp32":
        assert torch.equal(st.e32, e0 + one_minus_decay(0, 0.99, False) * (st.p32 - e0)) and st.g16_reduced is False


def test_two_runs_agree_and_the_bf16_gradient_form_equals_the_fp32_form(ops, weights):
    nondet = ops.nondet_launches()
    kw = dict(betas=BETAS, eps=EPS, ema_decay=0.99)
    runs = []
    for form in ("fp32", "fp32", "g16"):
        st = _store(ops, weights, seed=3, state=True)
        st.g16.copy_(st.g32.to(BF))
        st.g32.copy_(st.g16.float())                                 # the fp32 form runs on g16.float()
        st.enable_ema()
        st.e32.mul_(0.9)
        st.step_count = 6
        if form == "g16":
            st.g32.zero_()                                           # nothing may read it
            st.g16_reduced = True
        e0 = st.e32.clone()
        st.lamb_step(st.sumsq(), LR, WD, 1.0, **kw)
        assert st.g16_reduced is False and st.ema_updates == 1
        from medmoe_amd.ema import one_minus_decay
        omd = one_minus_decay(0, 0.99, False)
        assert torch.equal(st.e32, e0 + omd * (st.p32 - e0))         # three separately rounded fp32 operations
        _exact(st)
        runs.append({k: getattr(st, k).clone() for k in ("p32", "m", "v", "p16", "e32", "_lamb_ratios", "normsq")})
    for other in runs[1:]:
        for k, a in runs[0].items():
            assert torch.equal(a, other[k]), k
    assert ops.nondet_launches() == nondet
    # and the plain launch gives the same p, m, v as the EMA form
    st = _store(ops, weights, seed=3, state=True)
    st.g32.copy_(st.g32.to(BF).float())
    st.step_count = 6
    st.lamb_step(st.sumsq(), LR, WD, 1.0, betas=BETAS, eps=EPS)
    assert all(torch.equal(getattr(st, k), runs[0][k]) for k in ("p32", "m", "v", "p16"))


def test_a_frozen_head_steps_the_tail_only(ops, weights):
    from medmoe_amd.flat import FlatArena
    names = ["s257", "s4097", "g7", "g9", "g255", "s1", "zero", "big", "tail"]
    ar = FlatArena(DEV, [(n, tuple(weights[n].shape)) for n in names], groups=GROUPS, train_from="s1")
    assert ar.train_from > 0 and ar.n_train < ar.numel
    for n in names:
        ar.f32(n).copy_(weights[n].to(DEV))
    ar.refresh()
    ar.set_param_groups({"s1": (2.0, 1.0), "tail": (1.0, 0.0)})
    assert [n for n, _ in ar.segments()] == ["s1", "zero", "big", "tail"] and ar.segments()[-1][1] == ar.n_train
    g = torch.Generator().manual_seed(5)
    for n in ("s1", "zero", "big", "tail"):
        ar.grad(n).copy_((torch.randn(weights[n].numel(), generator=g) * 0.3).to(DEV))
    ar.names = names
    head, head16 = ar.p32[:ar.train_from].clone(), ar.p16[:ar.train_from].clone()
    ar.adam_state()
    before = _snapshot(ar)
    ar.lamb_step(ar.sumsq(), LR, WD, 1.0, betas=BETAS, eps=EPS, always_adapt=True)
    _check(ops, ar, before, 1, clip=1.0, always_adapt=True, trust_clip=False, label="frozen head")
    assert torch.equal(ar.p32[:ar.train_from], head) and torch.equal(ar.p16[:ar.train_from], head16)


def test_argument_checks(ops):
    n, S = 16, 2
    z = lambda k: torch.zeros(k, device=DEV)
    p, g, m, v = z(n), z(n), z(n), z(n)
    ends = torch.tensor([5, 16], device=DEV, dtype=torch.int64)
    base = ops.lamb_plan(ends.cpu(), n).to(DEV)
    one = torch.ones(S, device=DEV)
    floats = ops.lamb_scratch_floats(n, S)
    assert floats >= 2 * 2
    scratch, ratios = z(floats), z(3 * S)
    ptr = lambda t: None if t is None else t.data_ptr()
    h = ops.current_stream_handle()

    def mom(p_=p, n_=n, S_=S, floats_=floats, step=1, ends_=ends):
        return ops._fn("lamb_moments")(ptr(p_), ptr(g), ptr(m), ptr(v), n_, ptr(ends_), ptr(one), ptr(base), S_, ptr(scratch), floats_, 0.9, 0.999, 1e-6,
                                       0.01, step, None, 0.0, 1.0, h)
    assert mom() == 0
    assert 0 not in {mom(p_=None), mom(n_=6), mom(S_=0), mom(floats_=floats - 1), mom(step=0), mom(ends_=None)}
    rat = ops._fn("lamb_ratios")
    assert rat(ptr(scratch), floats, ptr(ends), ptr(one), ptr(base), S, n, 0.01, 0, 0, ptr(ratios), h) == 0
    assert rat(ptr(scratch), floats - 1, ptr(ends), ptr(one), ptr(base), S, n, 0.01, 0, 0, ptr(ratios), h) != 0
    app = ops._fn("lamb_apply")
    assert app(ptr(p), ptr(m), ptr(v), None, n, ptr(ends), ptr(one), ptr(one), S, ptr(ratios), 1e-3, 0.9, 0.999, 1e-6, 0.01, 1, h) == 0
    assert app(ptr(p), ptr(m), ptr(v), None, n, ptr(ends), ptr(one), ptr(one), S, None, 1e-3, 0.9, 0.999, 1e-6, 0.01, 1, h) != 0
    assert ops._fn("lamb_apply_ema")(ptr(p), ptr(m), ptr(v), None, n, ptr(ends), ptr(one), ptr(one), S, ptr(ratios), 1e-3, 0.9, 0.999, 1e-6, 0.01, 1,
                                     ptr(z(n)), 1.5, h) != 0
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and float(ratios[:S].min()) == 1.0
