"""Per-element float64 tests of every LayerNorm kernel instance (csrc/norm.hip and the two fused residual + LayerNorm launches of
csrc/dropout.hip), each called through medmoe_amd.ops as the engine calls it.  References, launch geometry and bars: tests/layernorm_reference.py
(every chain length is counted from the kernel source there; tests/test_layernorm_bars_host.py shows the bars hold for an fp32 emulation and
catch eight mutants).  An element passes when |got - ref| <= c_r |ref| + c_a terms (`check` of test_glue_kernels_gpu.py); every test prints
the worst |err| / bar per output as "[bar] ..." (run with -s).

Every output buffer carries a sentinel tail that must stay untouched, no element that should be written may still hold the sentinel, and
rows at or past a device row count must hold nothing else.

Data: rows of five kinds in turn (randn * 2 + 0.5; 4 + 0.25 randn - what a one-pass variance gets wrong; 1e3 randn; one constant; zero),
gamma of both signs, beta non-zero, eps in {1e-6, 1e-5, 1e-12}.  On constant rows mean == c and y == beta exactly.

Row counts per instance, R rows per wave and W rows per workgroup (forward 4 R, backward 16 R): 1, W - 1, W, W + 1, 3 W + 1 and, for R > 1,
2 W + R - 1 (a partly filled wave); above the grid caps (2048 forward / 512 backward workgroups = 8192 R rows) 8192 R + W + 1 rows at
D = 96, 192, 384, 520, so the row loop runs a ragged second trip at every lane width and with two chunk slots.

Which test reaches which template instance (layernorm_fwd_kernel<bf16 | float, NCH, LPR> and layernorm_bwd_kernel<NCH, LPR>; names without
their test_ prefix, above_cap = forward_ / backward_above_the_grid_cap, det = backward_ordered_reduce, fwd_rows / bwd_rows = the device row
counts, independence = rows_are_independent, apply = apply_repeats_the_forward):

  instance (widths)                         elementwise float64                              bit / exact tests
  LPR 16         (8, 96, 128)               forward[l16] backward[l16] above_cap[96]         fwd_rows bwd_rows det independence option16
  LPR 32         (136, 192, 256)            forward[l32] backward[l32] above_cap[192]        fwd_rows bwd_rows det independence option16
  LPR 64 NCH 1   (264, 384, 512)            forward[n1] backward[n1] above_cap[384]          fwd_rows bwd_rows det independence apply
  NCH 2          (520, 768, 1024)           forward[n2] backward[n2] above_cap[520]          fwd_rows bwd_rows det independence apply
  NCH 3          (1032, 1280, 1536)         forward[n3] backward[n3]                         fwd_rows bwd_rows det independence apply
  NCH 4          (1544, 2048)               forward[n4] backward[n4]                         fwd_rows bwd_rows det independence apply
  option 16 = 3  (8, 96, 128, 136, 256)     forward[opt16] backward[opt16]                   option16 (bits of the default form) fwd_rows bwd_rows
  fused launches (8, 264, 520, 1032,        fused[scale | dropout] (x1 per element; y, mean, rstd: the bits of layernorm_fwd on the stored x1,
                  1544, 2048; above the     itself judged per element above), fused_above_cap[96, 192, 384, 520].  The fused kernels have one
                  cap 96, 192, 384, 520)    instance each (64 lanes, four slots looped at run time): NCH 3 and 4 exist only in norm.hip.
  layernorm_apply                           bits of the forward's y at 264, 520, 1032, 1544 and past 1024 x 256 chunks with a ragged last
                                            workgroup
  refusals                                  D % 8 != 0, D = 2056, rows = 0, dgamma without dbeta, ordered-reduce scratch one float short"""
import contextlib
import io
from types import SimpleNamespace

import pytest
import torch

import layernorm_reference as R
from test_glue_kernels_gpu import _BITS, BF, DEV, F32, F64, I32, SENT, UBF, check, guarded, sentinel_ok, tail_ok

pytestmark = pytest.mark.gpu

INSTANCES = {"l16": ((8, 96, 128), False), "l32": ((136, 192, 256), False), "n1": ((264, 384, 512), False), "n2": ((520, 768, 1024), False),
             "n3": ((1032, 1280, 1536), False), "n4": ((1544, 2048), False), "opt16": ((8, 96, 128, 136, 256), True)}
EPS = (1e-6, 1e-5, 1e-12)
CAP_WIDTHS = (96, 192, 384, 520)
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def one_row(ops, on):
    """option 16 = 3: one row per wave whatever the width, forward (bit 0) and backward (bit 1); the default restored"""
    try:
        if on:
            ops.set_option(16, 3)
        yield
    finally:
        ops.set_option(16, 0)


class Worst:
    """the worst |err| / bar per output over the cases of one test; `check` raises at the first element over its bar"""

    def __init__(self, label):
        self.label, self.worst = label, {}

    def check(self, name, where, got, ref, terms, c_r, c_a):
        with contextlib.redirect_stdout(io.StringIO()):
            w = check(f"{self.label} {name} {where}", got, ref, terms, c_r, c_a)
        self.worst[name] = max(self.worst.get(name, 0.0), w)

    def report(self):
        for name, w in self.worst.items():
            print(f"[bar] {self.label} {name}: worst |err|/bar = {w:.3g}")


def bits(t):
    return t.reshape(-1).view(_BITS[t.dtype])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def written(t):
    return not bool((bits(t) == SENT[t.dtype]).any().item())


def counts(rpw, per):
    c = {1, per - 1, per, per + 1, 3 * per + 1}
    if rpw > 1:
        c.add(2 * per + rpw - 1)
    return sorted(n for n in c if n > 0)


def data(seed, rows, D):
    gen = torch.Generator().manual_seed(seed)
    x = R.make_x(gen, rows, D)
    gamma, beta = R.make_params(gen, D)
    dy, add = R.make_dy(gen, rows, D)
    mu, rs = R.make_stats(gen, rows)
    const = R.kinds(rows)[1]
    return SimpleNamespace(rows=rows, D=D, **{k: v.to(DEV) for k, v in dict(x=x, gamma=gamma, beta=beta, dy=dy, add=add, mu=mu, rs=rs,
                                                                           const=const).items()})


def run_fwd(ops, d, eps, dtype, x=None, want_mean=True, want_rstd=True):
    x = d.x if x is None else x
    rows = x.shape[0]
    by, y = guarded((rows, d.D), dtype)
    bm, mean = guarded((rows,), F32)
    br, rstd = guarded((rows,), F32)
    ops.layernorm_fwd(x, d.gamma, d.beta, y, mean if want_mean else None, rstd if want_rstd else None, eps)
    torch.cuda.synchronize()
    assert tail_ok(by, y.numel()) and tail_ok(bm, rows) and tail_ok(br, rows), "wrote past an output"
    assert written(y) and (written(mean) if want_mean else sentinel_ok(mean)) and (written(rstd) if want_rstd else sentinel_ok(rstd))
    return y, mean, rstd


def judge_fwd(w, where, d, eps, geo, y, mean, rstd):
    (m64, tm, cm), (r64, tr, cr) = R.stats_bars(d.x, eps, geo, exact_mean=d.const)
    w.check("mean", where, mean, m64, tm, 0.0, cm)
    w.check("rstd", where, rstd, r64, tr, 0.0, cr)
    y64, ty, cy = R.y_from_stats(d.x, mean, rstd, d.gamma, d.beta)
    tag = "y bf16" if y.dtype == BF else "y fp32"
    w.check(tag, where, y, y64, ty, *((UBF, R.c_bf16(cy)) if y.dtype == BF else (0.0, cy)))
    if bool(d.const.any()):                                             # constant rows: c * D is exact in fp32, so mean == c and y == beta
        assert torch.equal(mean[d.const], d.x[d.const][:, 0].float()), f"{where}: mean of a constant row"
        yc = y[d.const]
        assert torch.equal(yc, d.beta.to(y.dtype).expand_as(yc)), f"{where}: y of a constant row"


def run_bwd(ops, d, mean, rstd, add, cols, det=None, rows_dev=None, x=None, dy=None):
    """-> dx, dgamma, dbeta, prior_g, prior_b (the last four None without cols); the column sums start from a non-zero prior"""
    x, dy = (d.x if x is None else x), (d.dy if dy is None else dy)
    rows = x.shape[0]
    bdx, dx = guarded((rows, d.D), BF)
    pg = pb = dg = db = None
    if cols:
        gen = torch.Generator().manual_seed(rows * 7 + d.D)
        pg, pb = (torch.randn(d.D, generator=gen) * 3).to(DEV), (torch.randn(d.D, generator=gen) * 3).to(DEV)
        (bg, dg), (bb, db) = guarded((d.D,), F32, pg), guarded((d.D,), F32, pb)
    ops.layernorm_bwd(dy, x, mean, rstd, d.gamma, dx, dg, db, add=add, det=det, rows_dev=rows_dev)
    torch.cuda.synchronize()
    assert tail_ok(bdx, dx.numel()), "wrote past dx"
    if cols:
        assert tail_ok(bg, d.D) and tail_ok(bb, d.D), "wrote past dgamma / dbeta"
    return dx, dg, db, pg, pb


def judge_bwd(w, where, d, mean, rstd, add, geo, dx, dg, db, pg, pb, det=False, dx_too=True):
    dx64, tdx, tg, tb = R.bwd_from_stats(d.dy, d.x, mean, rstd, d.gamma, add)
    if dx_too:
        assert written(dx), f"{where}: dx not written everywhere"
        w.check("dx", where, dx, dx64, tdx, UBF, R.c_bf16(R.c_dx(geo)))
    if dg is not None:
        form = " (ordered)" if det else ""
        for nm, got, t, prior, which in (("dgamma", dg, tg, pg, 0), ("dbeta", db, tb, pb, 1)):
            ref, terms = R.col_reference(t, prior)
            w.check(nm + form, where, got, ref, terms, 0.0, R.c_col(geo, which, det))


# ------------------------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_forward(ops, inst):
    """mean, rstd per row against float64, y per element (bf16 and fp32 output), exact on constant rows; mean / rstd passed as None leave
    the other outputs unchanged"""
    widths, opt = INSTANCES[inst]
    w = Worst(f"forward[{inst}]")
    with one_row(ops, opt):
        for wi, D in enumerate(widths):
            g0 = R.geometry(D, 1, one_row=opt)
            for ci, rows in enumerate(counts(g0["rpw"], g0["per"])):
                d, eps = data(11 * D + rows, rows, D), EPS[(wi + ci) % 3]
                geo = R.geometry(D, rows, one_row=opt)
                outs = {}
                for dt in (BF, F32):
                    outs[dt] = run_fwd(ops, d, eps, dt)
                    judge_fwd(w, f"D={D} rows={rows} eps={eps}", d, eps, geo, *outs[dt])
                assert same_bits(outs[BF][1], outs[F32][1]) and same_bits(outs[BF][2], outs[F32][2]), "statistics depend on the output type"
                if rows == 3 * g0["per"] + 1:
                    y, mean, rstd = outs[BF]
                    for wm, wr in ((False, True), (True, False), (False, False)):
                        y2, m2, r2 = run_fwd(ops, d, eps, BF, want_mean=wm, want_rstd=wr)
                        assert same_bits(y2, y) and (not wm or same_bits(m2, mean)) and (not wr or same_bits(r2, rstd)), (D, wm, wr)
    w.report()


@pytest.mark.parametrize("D", CAP_WIDTHS)
def test_forward_above_the_grid_cap(ops, D):
    """8192 R + W + 1 rows: 2048 workgroups, a ragged second trip through the row loop"""
    g0 = R.geometry(D, 1)
    rows = 8192 * g0["rpw"] + g0["per"] + 1
    geo = R.geometry(D, rows)
    assert (geo["grid"], geo["iters"]) == (R.FWD_GRID_CAP, 2)
    d, w = data(5 * D, rows, D), Worst(f"forward_above_cap[{D}]")
    for dt, eps in ((BF, 1e-5), (F32, 1e-12)):
        judge_fwd(w, f"rows={rows}", d, eps, geo, *run_fwd(ops, d, eps, dt))
    w.report()


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_forward_rows_device_count(ops, inst):
    """medmoe_layernorm_fwd_rows as the text engine calls it: rows below the device count carry the bits of layernorm_fwd on the slice; rows
    at or past it are NaN on input and keep the sentinel in y, mean and rstd; a count past `rows` behaves as `rows`"""
    widths, opt = INSTANCES[inst]
    with one_row(ops, opt):
        for wi, D in enumerate(widths):
            g0 = R.geometry(D, 1, one_row=opt)
            rows, eps = 3 * g0["per"] + 1, EPS[wi % 3]
            d = data(13 * D, rows, D)
            for count in (0, 1, g0["per"] + max(g0["rpw"] - 1, 1), rows, rows + 5):
                n = min(count, rows)
                x = d.x.clone()
                x[n:] = NAN
                for dt in ((BF, F32) if count == rows else (BF,)):
                    (by, y), (bm, mean), (br, rstd) = guarded((rows, D), dt), guarded((rows,), F32), guarded((rows,), F32)
                    ops.call("layernorm_fwd_rows", x, d.gamma, d.beta, y, mean, rstd, rows, D, eps, int(dt == F32),
                             torch.tensor([count], dtype=I32, device=DEV))
                    torch.cuda.synchronize()
                    assert tail_ok(by, y.numel()) and tail_ok(bm, rows) and tail_ok(br, rows)
                    assert sentinel_ok(y[n:]) and sentinel_ok(mean[n:]) and sentinel_ok(rstd[n:]), (D, count, "rows past the count written")
                    if n:
                        ref = run_fwd(ops, d, eps, dt, x=x[:n])
                        for got, want, nm in zip((y, mean, rstd), ref, ("y", "mean", "rstd")):
                            assert same_bits(got[:n], want), (D, count, nm)


@pytest.mark.parametrize("rows,D", [(37, 264), (37, 520), (37, 1032), (37, 1544), (8001, 264)])
def test_apply_repeats_the_forward(ops, rows, D):
    """layernorm_apply from the saved statistics: the bits of the forward's y at the widths with one lane in the last chunk slot, and at
    8001 x 33 = 264033 chunks > 1024 x 256: 258 workgroups of 1024 chunks, the last one ragged, rows found by the 64-bit division"""
    d = data(17 * D + rows, rows, D)
    y, mean, rstd = run_fwd(ops, d, 1e-5, BF)
    by, y2 = guarded((rows, D), BF)
    ops.layernorm_apply(d.x, mean, rstd, d.gamma, d.beta, y2)
    torch.cuda.synchronize()
    assert tail_ok(by, y2.numel()) and same_bits(y2, y)


# ------------------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_backward(ops, inst):
    """dx per element with and without `add`, with and without dgamma / dbeta; the column sums against float64 onto a non-zero prior; the
    statistics once from the forward and once arbitrary per row (a statistic read at the wrong row shows)"""
    widths, opt = INSTANCES[inst]
    w = Worst(f"backward[{inst}]")
    with one_row(ops, opt):
        for wi, D in enumerate(widths):
            g0 = R.geometry(D, 1, backward=True, one_row=opt)
            for ci, rows in enumerate(counts(g0["rpw"], g0["per"])):
                d, k = data(19 * D + rows, rows, D), (wi + ci) % 2
                geo = R.geometry(D, rows, backward=True, one_row=opt)
                _, mean, rstd = run_fwd(ops, d, EPS[(wi + ci) % 3], BF)
                for (mu, rs), add, cols, tag in (((mean, rstd), d.add if k else None, True, "forward stats"),
                                                 ((d.mu, d.rs), None if k else d.add, (wi + ci) % 3 != 0, "arbitrary stats")):
                    out = run_bwd(ops, d, mu, rs, add, cols)
                    judge_bwd(w, f"D={D} rows={rows} {tag} add={add is not None}", d, mu, rs, add, geo, *out)
    w.report()


@pytest.mark.parametrize("D", CAP_WIDTHS)
def test_backward_above_the_grid_cap(ops, D):
    """8192 R + W + 1 rows: 512 workgroups, a ragged second trip; atomic and ordered column sums; dx of both forms bit-equal"""
    g0 = R.geometry(D, 1, backward=True)
    rows = 8192 * g0["rpw"] + g0["per"] + 1
    geo = R.geometry(D, rows, backward=True)
    assert (geo["grid"], geo["iters"]) == (R.BWD_GRID_CAP, 2)
    d, w = data(7 * D, rows, D), Worst(f"backward_above_cap[{D}]")
    a = run_bwd(ops, d, d.mu, d.rs, d.add, True)
    judge_bwd(w, f"rows={rows}", d, d.mu, d.rs, d.add, geo, *a)
    o = run_bwd(ops, d, d.mu, d.rs, d.add, True, det=ops.DetScratch(DEV))
    assert same_bits(o[0], a[0])
    judge_bwd(w, f"rows={rows}", d, d.mu, d.rs, d.add, geo, *o, det=True, dx_too=False)
    w.report()


class ShortScratch:
    """a DetScratch that hands out one float less than the launch needs"""

    def __init__(self, floats):
        self.buf = torch.zeros(floats, device=DEV)

    def get(self, floats):
        return self.buf


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_backward_ordered_reduce(ops, inst):
    """the deterministic backward: two runs give the same bits, dx is bit-equal to the atomic form, the column sums keep their bars onto the
    prior, and a scratch one float short is refused with the argument code before anything is written"""
    widths, opt = INSTANCES[inst]
    w = Worst(f"ordered[{inst}]")
    with one_row(ops, opt):
        for D in widths:
            g0 = R.geometry(D, 1, backward=True, one_row=opt)
            for rows in (g0["per"] + 1, 3 * g0["per"] + 1):
                d = data(23 * D + rows, rows, D)
                geo = R.geometry(D, rows, backward=True, one_row=opt)
                det = ops.DetScratch(DEV)
                a = run_bwd(ops, d, d.mu, d.rs, d.add, True, det=det)
                b = run_bwd(ops, d, d.mu, d.rs, d.add, True, det=det)
                for i in range(3):
                    assert same_bits(a[i], b[i]), (D, rows, i)
                assert same_bits(a[0], run_bwd(ops, d, d.mu, d.rs, d.add, False)[0]), (D, rows, "dx against the atomic form")
                judge_bwd(w, f"D={D} rows={rows}", d, d.mu, d.rs, d.add, geo, *a, det=True, dx_too=False)
            (bdx, dx), (bg, dg), (bb, db) = guarded((rows, D), BF), guarded((D,), F32), guarded((D,), F32)
            with pytest.raises(RuntimeError, match="code -1"):
                ops.layernorm_bwd(d.dy, d.x, d.mu, d.rs, d.gamma, dx, dg, db, det=ShortScratch(geo["grid"] * 2 * D - 1))
            torch.cuda.synchronize()
            assert sentinel_ok(bdx) and sentinel_ok(bg) and sentinel_ok(bb), (D, "a refused launch wrote")
    w.report()


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_backward_rows_device_count(ops, inst):
    """medmoe_layernorm_bwd_rows at the device counts 0 (nothing read, dx untouched, the column sums keep the prior's bits) and rows + 5
    (behaves as rows: dx bit-equal to layernorm_bwd, the column sums within their bars)"""
    widths, opt = INSTANCES[inst]
    w = Worst(f"bwd_rows[{inst}]")
    with one_row(ops, opt):
        for D in widths:
            g0 = R.geometry(D, 1, backward=True, one_row=opt)
            rows = 3 * g0["per"] + 1
            d = data(29 * D, rows, D)
            geo = R.geometry(D, rows, backward=True, one_row=opt)
            nan = torch.full_like(d.x, NAN)
            dx, dg, db, pg, pb = run_bwd(ops, d, d.mu, d.rs, nan, True, rows_dev=torch.zeros(1, dtype=I32, device=DEV), x=nan, dy=nan)
            assert sentinel_ok(dx) and same_bits(dg, pg) and same_bits(db, pb), (D, "count 0")
            out = run_bwd(ops, d, d.mu, d.rs, d.add, True, rows_dev=torch.tensor([rows + 5], dtype=I32, device=DEV))
            assert same_bits(out[0], run_bwd(ops, d, d.mu, d.rs, d.add, False)[0]), (D, "count rows + 5")
            judge_bwd(w, f"D={D} count={rows + 5}", d, d.mu, d.rs, d.add, geo, *out, dx_too=False)
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------------------
# invariances
# ------------------------------------------------------------------------------------------------------------------------------------------
def fwd_bwd_bits(ops, d, sel):
    """y, mean, rstd, dx of the rows `sel` (an index tensor or a slice) launched on their own"""
    x, dy, add = d.x[sel].contiguous(), d.dy[sel].contiguous(), d.add[sel].contiguous()
    y, mean, rstd = run_fwd(ops, d, 1e-5, BF, x=x)
    dx = run_bwd(ops, d, mean, rstd, add, False, x=x, dy=dy)[0]
    return y, mean, rstd, dx


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_rows_are_independent(ops, inst):
    """launching rows[a:b] alone gives the bits of the full launch, and permuting the rows permutes y, mean, rstd and dx bit for bit: nothing
    leaks between the rows of a wave"""
    widths, opt = INSTANCES[inst]
    with one_row(ops, opt):
        for D in widths:
            g0 = R.geometry(D, 1, backward=True, one_row=opt)
            rows = 3 * g0["per"] + 1
            d = data(31 * D, rows, D)
            full = fwd_bwd_bits(ops, d, slice(0, rows))
            a, b = g0["rpw"] + 1, rows - 2
            for got, want in zip(fwd_bwd_bits(ops, d, slice(a, b)), full):
                assert same_bits(got, want[a:b]), (D, "slice")
            perm = torch.randperm(rows, generator=torch.Generator().manual_seed(D)).to(DEV)
            for got, want in zip(fwd_bwd_bits(ops, d, perm), full):
                assert same_bits(got, want[perm]), (D, "permutation")


@pytest.mark.parametrize("D", [8, 96, 128, 136, 256])
def test_option_16_gives_the_bits_of_the_default_form(ops, D):
    """one row per wave against several: the same bits in y (both types), mean, rstd and dx - the claim of lpr_sum's comment; dgamma / dbeta
    sum in another order and are held to their bars"""
    w = Worst(f"option16[{D}]")
    for rows in (1, 2 * 64 + 3, 8 * 64 + 5):
        d = data(37 * D + rows, rows, D)
        res = []
        for opt in (False, True):
            with one_row(ops, opt):
                y, mean, rstd = run_fwd(ops, d, 1e-6, BF)
                y32 = run_fwd(ops, d, 1e-6, F32)[0]
                out = run_bwd(ops, d, mean, rstd, d.add, True)
                judge_bwd(w, f"rows={rows} option={int(opt)}", d, mean, rstd, d.add, R.geometry(D, rows, backward=True, one_row=opt), *out,
                          dx_too=False)
                res.append((y, y32, mean, rstd, out[0]))
        for nm, p, q in zip(("y", "y fp32", "mean", "rstd", "dx"), *res):
            assert same_bits(p, q), (rows, nm)
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------------------
# the fused residual + LayerNorm launches
# ------------------------------------------------------------------------------------------------------------------------------------------
def run_fused(ops, kind, w, where, rows, D, rps, eps, seed):
    gen = torch.Generator().manual_seed(seed)
    z, res = R.make_x(gen, rows, D).to(DEV), (torch.randn(rows, D, generator=gen) * 1.5).to(BF).to(DEV)
    gamma, beta = (t.to(DEV) for t in R.make_params(gen, D))
    (b1, x1), (b2, y), (b3, mean), (b4, rstd) = guarded((rows, D), BF), guarded((rows, D), BF), guarded((rows,), F32), guarded((rows,), F32)
    if kind == "scale":
        scale = torch.tensor([1.25, 0.0, 1.0, 0.3], dtype=F32)[torch.arange(rows // rps) % 4].to(DEV)
        per_row = scale.repeat_interleave(rps)
        z[per_row == 0] = NAN                                            # a dropped sample copies residual: z is not read there
        ops.scale_add_layernorm_fwd(z, res, scale, rps, gamma, beta, x1, y, mean, rstd, eps)
        factor = per_row.to(F64)[:, None]
        zz = torch.where(per_row[:, None] == 0, torch.zeros_like(z), z)
    else:
        args, p = (seed, 3, 4 * 2 + 1), 0.1
        rng = ops.dropout_rng(*args, p)
        ops.dropout_add_layernorm_fwd(z, res, gamma, beta, x1, y, mean, rstd, eps, rng)
        keep = torch.full((rows, D), 0xA5, dtype=torch.uint8, device=DEV)
        ops.dropout_mask(keep, rows, D, D, rng)
        assert bool((keep <= 1).all())
        factor, zz = keep.to(F64) * R.f32_scalar(rng[4]), z
    torch.cuda.synchronize()
    for b, t in ((b1, x1), (b2, y), (b3, mean), (b4, rstd)):
        assert tail_ok(b, t.numel()) and written(t), where
    ref, terms, c = R.x1_reference(res, zz, factor)
    w.check("x1", where, x1, ref, terms, UBF, R.c_bf16(c))
    if kind == "scale":
        assert same_bits(x1[per_row == 0], res[per_row == 0]), f"{where}: a dropped row is not the residual"
    d = SimpleNamespace(D=D, gamma=gamma, beta=beta)
    for got, want, nm in zip((y, mean, rstd), run_fwd(ops, d, eps, BF, x=x1), ("y", "mean", "rstd")):
        assert same_bits(got, want), f"{where}: {nm} differs from layernorm_fwd on the stored x1"


@pytest.mark.parametrize("kind", ["scale", "dropout"])
def test_fused(ops, kind):
    """x1 per element against float64 (one fp32 product, one sum, the bf16 rounding; the dropout mask is the one medmoe_dropout_mask
    exports); y, mean, rstd bit-equal to layernorm_fwd on the stored x1"""
    w = Worst(f"fused[{kind}]")
    for wi, D in enumerate((8, 264, 520, 1032, 1544, 2048)):
        for ci, (rows, rps) in enumerate(((1, 1), (3, 1), (4, 2), (5, 1), (13, 1), (24, 3))):
            run_fused(ops, kind, w, f"D={D} rows={rows}", rows, D, rps, EPS[(wi + ci) % 3], 41 * D + rows)
    w.report()


@pytest.mark.parametrize("D", CAP_WIDTHS)
@pytest.mark.parametrize("kind", ["scale", "dropout"])
def test_fused_above_the_grid_cap(ops, kind, D):
    """8192 + 4 + 1 rows (one row per wave, four waves): 2048 workgroups, a ragged second trip"""
    w = Worst(f"fused_above_cap[{kind}-{D}]")
    run_fused(ops, kind, w, "rows=8197", 8197, D, 1, 1e-5, 43 * D)
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ops):
    """D % 8 != 0, D = 2056 and rows = 0 return the shape code (-2) from every entry that takes them as arguments, dgamma without dbeta the
    library's argument code (-1: a pointer is missing, no shape is wrong); the wrappers of the two base launches refuse a bad width and an
    unpaired dgamma on the host, and an empty x reaches the library as a null pointer.  Whoever refuses, the sentinel-filled outputs stay
    untouched.  Every buffer is at least as large as its shape asks for."""
    one = torch.ones(1, dtype=I32, device=DEV)
    rng = ops.dropout_rng(1, 2, 3, 0.1)

    def bufs(rows, D):
        s = SimpleNamespace(x=torch.zeros(rows, D, dtype=BF, device=DEV), gamma=torch.ones(D, device=DEV), beta=torch.zeros(D, device=DEV),
                            st=torch.ones(2, rows, device=DEV), scale=torch.ones(rows, device=DEV))
        s.out = [guarded((rows, D), BF), guarded((rows, D), F32), guarded((rows,), F32), guarded((rows,), F32), guarded((D,), F32),
                 guarded((D,), F32), guarded((rows, D), BF)]
        s.y, s.y32, s.mean, s.rstd, s.dg, s.db, s.x1 = (v for _, v in s.out)
        return s

    def untouched(s):
        torch.cuda.synchronize()
        return all(sentinel_ok(b) for b, _ in s.out)

    for rows, D in ((4, 132), (4, 2056), (0, 128)):                      # rows = 0: the row count passed, over buffers of four rows
        s = bufs(4, D)
        launches = [lambda: ops.call("layernorm_fwd_rows", s.x, s.gamma, s.beta, s.y, s.mean, s.rstd, rows, D, 1e-5, 0, one),
                    lambda: ops.call("layernorm_fwd_rows", s.x, s.gamma, s.beta, s.y32, s.mean, s.rstd, rows, D, 1e-5, 1, one),
                    lambda: ops.call("layernorm_bwd_rows", s.x, s.x, s.st[0], s.st[1], s.gamma, None, s.y, s.dg, s.db, rows, D, one),
                    lambda: ops.call("layernorm_apply", s.x, s.st[0], s.st[1], s.gamma, s.beta, s.y, rows, D),
                    lambda: ops.call("scale_add_layernorm_fwd", s.x, s.x, s.scale, 1, s.gamma, s.beta, s.x1, s.y, s.mean, s.rstd, rows, D, 1e-5),
                    lambda: ops.call("dropout_add_layernorm_fwd", s.x, s.x, s.gamma, s.beta, s.x1, s.y, s.mean, s.rstd, rows, D, 1e-5, *rng)]
        for i, f in enumerate(launches):
            with pytest.raises(RuntimeError, match="code -2"):
                f()
            assert untouched(s), (rows, D, i)
        if rows:
            for f in (lambda: ops.layernorm_fwd(s.x, s.gamma, s.beta, s.y, s.mean, s.rstd, 1e-5),
                      lambda: ops.layernorm_bwd(s.x, s.x, s.st[0], s.st[1], s.gamma, s.y, s.dg, s.db)):
                with pytest.raises(ValueError, match="multiple of 8"):
                    f()
                assert untouched(s), (rows, D)
    s, empty = bufs(4, 128), torch.zeros(0, 128, dtype=BF, device=DEV)   # the base launches take their row count from x: an empty x
    for f in (lambda: ops.layernorm_fwd(empty, s.gamma, s.beta, torch.zeros_like(empty), s.mean, s.rstd, 1e-5),
              lambda: ops.layernorm_bwd(empty, empty, s.st[0], s.st[1], s.gamma, torch.zeros_like(empty), s.dg, s.db),
              lambda: ops.layernorm_bwd(empty, empty, s.st[0], s.st[1], s.gamma, torch.zeros_like(empty), s.dg, s.db, det=ops.DetScratch(DEV))):
        with pytest.raises(RuntimeError, match="failed with code"):
            f()
        assert untouched(s)
    s = bufs(4, 128)
    for dg, db in ((s.dg, None), (None, s.db)):
        with pytest.raises(RuntimeError, match="code -1"):
            ops.call("layernorm_bwd_rows", s.x, s.x, s.st[0], s.st[1], s.gamma, None, s.y, dg, db, 4, 128, one)
        with pytest.raises(ValueError, match="come together"):
            ops.layernorm_bwd(s.x, s.x, s.st[0], s.st[1], s.gamma, s.y, dg, db)
        assert untouched(s)
