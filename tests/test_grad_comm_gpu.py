"""The kernels of the bf16 gradient exchange on the GPU (csrc/optim.hip), alone: medmoe_grad_pack_bf16 against torch's own
scale-and-round on the bit patterns, medmoe_sumsq_det_bf16 against medmoe_sumsq_det on the up-cast buffer (bit-identical), the _g16 Adam
kernels against the fp32-gradient kernels fed float(g16) (bit-identical over three steps, plain and grouped), and FlatArena's flag life
cycle around a real reduce."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
THIRD = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))        # the fp32 value both sides multiply by


@pytest.fixture(scope="module")
def ops():
    from medmoe_amd import ops as o
    return o


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


# fp32 patterns planted among the random normals
SPECIALS = [
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,                 # exact ties: low half 0x8000 under an even / an odd upper half, both signs
    0x40490FDB, 0x3F7F8000, 0x3F7FFFFF, 0x3FFF8000, 0x3FFFFFFF,     # pi; roundings that carry into the exponent (0x3F7F -> 0x3F80, 0x3FFF -> 0x4000)
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,                             # the largest finite values round to +-Inf
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000,     # +-0, +-Inf, NaN
    0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x00400000, 0x807F8000,     # fp32 subnormals (ties among them)
    0x00800000, 0x00FF8000,                                         # the smallest normals: subnormal after a scale below 1
]


def specials():
    return torch.tensor(np.array(SPECIALS, dtype=np.uint32).view(np.int32)).view(torch.float32)


def planted(n, seed):
    """Random normals with the special patterns at the start, in the middle (not a multiple of 8) and at the very end of the buffer."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 2.0
    sp = specials()
    if n < 3 * sp.numel():
        return g
    for at in (0, n // 2 + 3, n - sp.numel()):
        g[at: at + sp.numel()] = sp
    return g


def check_pack(ops, g, scale, off):
    """g (host fp32) packed from offset `off` of a larger device buffer into offset `off` of a larger bf16 buffer, sentinels around it."""
    n = g.numel()
    src = torch.full((n + 2 * off + 8,), 123.0, device=DEV)
    src[off: off + n] = g.to(DEV)
    assert torch.equal(bits(src[off: off + n]).cpu(), bits(g))      # the copy kept every pattern (NaN payload, subnormals)
    dst = torch.full((n + 2 * off + 8,), -7.0, device=DEV, dtype=BF)
    keep = src.clone()
    ops.call("grad_pack_bf16", src[off: off + n], dst[off: off + n], n, scale)
    want = (src[off: off + n] * scale).to(BF)
    got = dst[off: off + n]
    bad = (bits(got) != bits(want)).nonzero().flatten()
    print(f"pack n={n} scale={scale} off={off}: {bad.numel()} mismatches",
          [(int(i), hex(int(bits(src[off + i: off + i + 1]).item()) & 0xFFFFFFFF), hex(int(bits(got[i: i + 1]).item()) & 0xFFFF),
            hex(int(bits(want[i: i + 1]).item()) & 0xFFFF)) for i in bad[:8]])
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(dst[:off]), bits(torch.full((off,), -7.0, device=DEV, dtype=BF)))
    assert torch.equal(bits(dst[off + n:]), bits(torch.full((off + 8,), -7.0, device=DEV, dtype=BF)))
    assert torch.equal(bits(src), bits(keep))                       # the fp32 gradient is only read
    return got


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("scale", [1.0, 0.5, THIRD], ids=["1", "half", "third"])
@pytest.mark.parametrize("n", [8, 1032, 4104, 3 * (1 << 20) + 8, 5 * (1 << 20) + 8])
def test_pack_equals_torch_scale_and_round_bit_for_bit(ops, n, scale, off):
    """out = bf16_rne(g * scale), the product in fp32: the bit patterns of torch's (g * scale).to(bfloat16).  n: one lane's 8 elements; more
    than one block; not a multiple of the block's 2048 elements; 1538 blocks of the 2048 the grid is capped at (one sweep); more than one
    sweep of the capped grid (2048 blocks x 2048 elements = 4 194 304) with a partial second one, so lanes step by gridDim.x * 256.
    off = 8: a range inside a larger buffer, the elements on both sides left as they were."""
    if n == 8:
        sp = torch.cat([specials(), torch.randn(6)])
        assert sp.numel() % 8 == 0
        for k in range(0, sp.numel(), 8):
            check_pack(ops, sp[k: k + 8].clone(), scale, off)
        return
    got = check_pack(ops, planted(n, n), scale, off)
    sp = specials().to(DEV)
    out = got[: sp.numel()]                                         # the planted values, by property
    assert bool(out[sp != sp].isnan().all()) and int((out != out).sum()) == int((sp != sp).sum())
    assert torch.equal(out[sp.isinf()], sp[sp.isinf()].to(BF))
    zero = bits(sp) << 1 == 0
    assert torch.equal(bits(out[zero]), bits(sp[zero].to(BF))) and int((bits(out[zero]) < 0).sum()) == 1      # -0 stays -0
    if scale == 1.0:
        v = lambda x: int(bits(out[SPECIALS.index(x)].reshape(1)).item()) & 0xFFFF
        assert (v(0x3F808000), v(0x3F818000), v(0xBF808000), v(0xBF818000)) == (0x3F80, 0x3F82, 0xBF80, 0xBF82)      # ties to even
        assert (v(0x3F7F8000), v(0x3F7FFFFF), v(0x3FFF8000), v(0x3FFFFFFF)) == (0x3F80, 0x3F80, 0x4000, 0x4000)      # carries
        assert (v(0x7F7FFFFF), v(0xFF7FFFFF)) == (0x7F80, 0xFF80)


@pytest.mark.parametrize("n", [5, 13, 1037])
def test_pack_scalar_tail(ops, n):
    """n % 8 != 0: the last n % 8 elements go through the scalar tail, nothing behind them is written."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 2.0
    g[-3:] = specials()[[1, 13, 5]]
    check_pack(ops, g, 0.5, 8)


def test_pack_refuses_misaligned_pointers(ops):
    src = torch.zeros(64, device=DEV)
    dst = torch.zeros(64, device=DEV, dtype=BF)
    for s, d in ((src[1:33], dst[:32]), (src[2:34], dst[:32]), (src[:32], dst[4:36]), (src[:32], dst[1:33])):
        with pytest.raises(RuntimeError, match="code -1"):
            ops.call("grad_pack_bf16", s, d, 32, 1.0)
    ops.call("grad_pack_bf16", src[4:36], dst[8:40], 32, 1.0)       # 16-byte aligned on both sides
    torch.cuda.synchronize()


# ---- the clip norm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 1032, 4104, 3 * (1 << 20) + 8])
def test_sumsq_det_bf16_is_sumsq_det_on_the_upcast_buffer(ops, n):
    g16 = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.7).to(BF).to(DEV)
    up = g16.float()
    scratch = torch.zeros(2049, device=DEV)
    a, a2, b = (torch.full((1,), -1.0, device=DEV) for _ in range(3))
    ops.call("sumsq_det_bf16", g16, n, a, scratch)
    ops.call("sumsq_det", up, n, b, scratch)
    ops.call("sumsq_det_bf16", g16, n, a2, scratch)
    exact = float((up.double() ** 2).sum())
    print(f"sumsq n={n}: bf16 {float(a)!r} fp32 {float(b)!r} float64 {exact!r} bound {n * 2.0 ** -24 * exact!r}")
    assert torch.equal(a, b)                                        # the same sum in the same order
    assert torch.equal(a, a2)                                       # and repeatable
    assert int(scratch[2048:].view(torch.int32)) == 0              # the arrival counter is back at zero
    assert abs(float(a) - exact) <= n * 2.0 ** -24 * exact


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------
class State:
    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.p = (torch.randn(n, generator=g) * 0.05).to(DEV)
        self.m = torch.zeros(n, device=DEV); self.v = torch.zeros(n, device=DEV)
        self.p16 = torch.zeros(n, device=DEV, dtype=BF)
        self.gen = g

    def clone(self):
        o = State.__new__(State)
        o.p, o.m, o.v, o.p16 = self.p.clone(), self.m.clone(), self.v.clone(), self.p16.clone()
        return o

    def same(self, o):
        return all(torch.equal(bits(a), bits(b)) for a, b in ((self.p, o.p), (self.m, o.m), (self.v, o.v), (self.p16, o.p16)))


def run_table(n, searched):
    """Runs with boundaries on odd elements and a one-element run; searched: more than 1024 runs (1..4 elements each) where n allows it,
    so the table is searched in global memory instead of LDS."""
    if n == 8:
        ends = [1, 2, 3, 7, 8] if searched else [3, 4, 8]
    elif searched:
        rs = np.random.RandomState(3)
        lens = rs.randint(1, 5, size=1500)
        ends = np.cumsum(lens)
        ends = [int(e) for e in ends if e < n - 8] + [n]
        assert len(ends) > 1024
    else:
        ends = [5, 6, 1001, 2047, n - 7, n]                         # run 2 is one element long
    assert all(b > a for a, b in zip(ends, ends[1:])) and ends[-1] == n and any(e % 2 for e in ends[:-1])
    rs = np.random.RandomState(len(ends))
    lrm = rs.choice([1.0, 0.5, 0.75, 0.1], size=len(ends)); wdm = rs.choice([1.0, 0.0], size=len(ends))
    t = lambda a, dt: torch.tensor(np.asarray(a), device=DEV, dtype=dt)
    return t(ends, torch.int64), t(lrm, torch.float32), t(wdm, torch.float32)


@pytest.mark.parametrize("clip", [0.25, 1e9], ids=["clip", "noclip"])
@pytest.mark.parametrize("n", [8, 4100, (1 << 20) + 4, 3 * (1 << 20) + 4])
@pytest.mark.parametrize("form", ["plain", "lds-adam", "lds-adamw", "searched-adam", "searched-adamw"])
def test_adam_on_bf16_gradients_is_adam_on_their_upcast(ops, form, n, clip):
    """Three steps from the same p, m, v: the _g16 kernel on g16, the existing kernel on g16.float(); p, m, v and the bf16 copy agree bit for
    bit after every step.  clip: 0.25 against a norm of several units scales every gradient; 1e9 never does (coefficient 1).  n: two
    float4s; more than one block, not a multiple of 8; 1025 blocks of the 2048 the grid is capped at (one sweep); more than one sweep of
    the capped grid (2048 blocks x 1024 elements = 2 097 152) with a partial second one, so lanes step by gridDim.x * 256."""
    a = State(n, n); b = a.clone()
    nsq = torch.zeros(1, device=DEV)
    tab = run_table(n, form.startswith("searched")) if form != "plain" else None
    dec = 1 if form.endswith("adamw") else 0
    for step in range(1, 4):
        g16 = (torch.randn(n, generator=a.gen) * (0.5 * step)).to(BF).to(DEV)
        up = g16.float()
        nsq.copy_((up.double() ** 2).sum().float())
        assert float(nsq) ** 0.5 > 0.25
        if tab is None:
            rest = (n, 5e-5, 0.9, 0.999, 1e-8, 0.01, step, nsq, clip, 1.0)
            ops.call("adam_step_g16", a.p, g16, a.m, a.v, a.p16, *rest)
            ops.call("adam_step", b.p, up, b.m, b.v, b.p16, *rest)
        else:
            rest = (n, tab[0], tab[1], tab[2], tab[0].numel(), 5e-5, 0.9, 0.98, 1e-6, 0.05, dec, step, nsq, clip, 1.0)
            ops.call("adam_groups_step_g16", a.p, g16, a.m, a.v, a.p16, *rest)
            ops.call("adam_groups_step", b.p, up, b.m, b.v, b.p16, *rest)
        assert a.same(b), (form, n, clip, step)
    assert bool(torch.isfinite(a.p).all()) and float(a.m.abs().max()) > 0 and torch.equal(a.p16, a.p.to(BF))


# ---- FlatArena ----------------------------------------------------------------------------------------------------------------------------
def test_arena_flag_life_cycle_and_the_step_on_the_reduced_gradient(ops, tmp_path):
    """pack -> g16 = bf16(g32 * scale); the reduce (a one-rank gloo group: a sum over one rank) sets the flag, reduced_grad() follows it,
    sumsq / adam_step read g16 while it is set and clear it; zero_grad clears it; the stepped parameters equal those of a second arena
    stepped through the fp32-gradient path on g16.float()."""
    import torch.distributed as dist
    from medmoe_amd import dist as D
    from medmoe_amd.flat import FlatStore
    gen = torch.Generator().manual_seed(5)
    w = {"q": torch.randn(24, 16, generator=gen), "k": torch.randn(24, 16, generator=gen), "b": torch.randn(13, generator=gen),
         "w2": torch.randn(40, 24, generator=gen)}
    mk = lambda: FlatStore(w, DEV, groups=[("qk", ["q", "k"])], gemm=["qk", "w2"])
    st, ref = mk(), mk()
    assert st._g16 is None and not st.g16_reduced
    st.g32.copy_(torch.randn(st.numel, generator=gen).to(DEV))
    g32 = st.g32.clone()
    assert st.reduced_grad() is st.g32
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        mid = st.offsets["w2"]
        assert 0 < mid < st.numel and mid % 8 == 0
        red = D.BucketedAllReduce(st.g32, [0, mid, st.numel], comm=st)
        red.ready(1)
        assert not st.g16_reduced and torch.equal(bits(st.g16[mid:]), bits(g32[mid:].to(BF))) and int(st.g16[:mid].abs().sum()) == 0
        red.ready(0)
        red.finish()
        assert st.g16_reduced and torch.equal(bits(st.g16), bits(g32.to(BF))) and torch.equal(st.g32, g32)
        assert torch.equal(st.reduced_grad(), st.g16.float())
        st.zero_grad()
        assert not st.g16_reduced and st.reduced_grad() is st.g32 and int(st.g32.abs().sum()) == 0
        st.g32.copy_(g32)
        D.allreduce_mean_(st.g32, comm=st)                          # the un-bucketed pair
        assert st.g16_reduced and torch.equal(bits(st.g16), bits(g32.to(BF))) and torch.equal(st.g32, g32)
    finally:
        dist.destroy_process_group()
    ref.g32.copy_(st.g16.float())
    for kw in (dict(), dict(decoupled=True, betas=(0.9, 0.98), eps=1e-6)):
        st.g16_reduced = True
        na, nb = st.sumsq().clone(), ref.sumsq().clone()
        assert torch.equal(na, nb) and float(na) > 0.25 ** 2
        st.adam_step(na, 1e-3, 0.05, 0.25, **kw)
        ref.adam_step(nb, 1e-3, 0.05, 0.25, **kw)
        assert not st.g16_reduced and st.reduced_grad() is st.g32
        for x, y in ((st.p32, ref.p32), (st.m, ref.m), (st.v, ref.v), (st.p16, ref.p16), (st.p16t, ref.p16t)):
            assert torch.equal(bits(x), bits(y))
    assert not torch.equal(st.p32, mk().p32)
