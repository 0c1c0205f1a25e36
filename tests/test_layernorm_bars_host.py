"""The bars of tests/layernorm_reference.py before any GPU sees them (no GPU), and the argument checks of ops.layernorm_fwd / ops.layernorm_bwd.

Not too tight: an fp32 emulation of the kernels in torch CPU ops - the same two passes, the same per-lane then xor-tree summation order at 16,
32 and 64 lanes per row, the same order of the column sums (trips of a wave, rows of a wave, 16 waves, workgroups; atomic and ordered form) -
passes `check` with a ratio <= 1 on the data of the GPU test, at one width per template instance.
Not vacuous: eight mutants of that emulation each fail `check` on at least one output, at every width they are defined for.

The emulation rounds after every operation; the compiler may fuse a multiply and an add, which only removes roundings (layernorm_reference)."""
import math

import pytest
import torch
import torch.nn.functional as F

import layernorm_reference as R
from test_glue_kernels_gpu import UBF, check
from test_vit_drop_path_host import stub  # noqa: F401  (the fixture)

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
# one width per instance (the ones that leave a single lane in the last chunk slot where there is one): (D, one row per wave, eps)
CASES = {"l16": (96, False, 1e-6), "l32": (136, False, 1e-5), "n1": (264, False, 1e-12), "n2": (520, False, 1e-6), "n3": (1032, False, 1e-5),
         "n4": (1544, False, 1e-12), "opt16": (96, True, 1e-5)}
MUTANTS = ("one_pass_variance", "unbiased_variance", "eps_dropped", "stats_of_previous_row", "gamma_beta_shifted_a_chunk", "last_slot_dropped",
           "dx_without_xhat_m2", "dgamma_missing_last_row")


# ------------------------------------------------------------------------------------------------------------------------------------------
# the emulation
# ------------------------------------------------------------------------------------------------------------------------------------------
def lanes(t, geo):
    """[rows, D] -> [rows, NCH, LPR, 8] as the lanes hold it (chunk c = lane + slot * LPR; zeros past D), and the mask of loaded chunks"""
    n = geo["nch"] * geo["lpr"]
    v = F.pad(t, (0, n * 8 - geo["D"])).reshape(t.shape[0], geo["nch"], geo["lpr"], 8)
    return v, (torch.arange(n) < geo["D"] // 8).reshape(geo["nch"], geo["lpr"])


def tree(s):
    """lpr_sum / wave_sum: v += shfl_xor(v, m) for m = LPR / 2 .. 1; every lane ends with the same bits"""
    lane = torch.arange(s.shape[1])
    m = s.shape[1] // 2
    while m:
        s = s + s[:, lane ^ m]
        m //= 2
    return s[:, 0]


def pair_sum(v, slots):
    """`s += a + b` over the four pairs of every chunk slot of a lane"""
    s = torch.zeros(v.shape[0], v.shape[2])
    for i in range(slots):
        for e in range(4):
            s = s + (v[:, i, :, 2 * e] + v[:, i, :, 2 * e + 1])
    return s


def emu_fwd(x, gamma, beta, eps, geo, out_dtype, mutant=None):
    D = torch.tensor(float(geo["D"]), dtype=F32)
    x32 = x.float()
    v, valid = lanes(x32, geo)
    slots = geo["nch"] - (1 if mutant == "last_slot_dropped" else 0)
    mean = tree(pair_sum(v, slots)) / D
    sq = torch.zeros(v.shape[0], v.shape[2])
    if mutant == "one_pass_variance":
        for i in range(slots):
            for e in range(8):
                sq = sq + v[:, i, :, e] * v[:, i, :, e]
        var = tree(sq) / D - mean * mean
    else:
        for i in range(slots):
            d = torch.where(valid[i][None, :, None], v[:, i] - mean[:, None, None], torch.zeros(()))
            for e in range(8):
                sq = sq + d[:, :, e] * d[:, :, e]
        var = tree(sq) / (D - 1 if mutant == "unbiased_variance" else D)
    rstd = torch.rsqrt(var if mutant == "eps_dropped" else var + torch.tensor(eps, dtype=F32))
    if mutant == "stats_of_previous_row":
        mean, rstd = mean.roll(1), rstd.roll(1)
    if mutant == "gamma_beta_shifted_a_chunk":
        gamma, beta = gamma.roll(8), beta.roll(8)
    y = (x32 - mean[:, None]) * rstd[:, None] * gamma + beta
    return y.to(out_dtype), mean, rstd


def col_sums(t, geo, prior, det):
    """dgamma / dbeta of the per-row terms t [rows, D]: a lane's trips through the row loop, the rows of a wave, the 16 waves in LDS, the
    workgroups (atomics: taken in workgroup order; ordered form: det_sum_records)"""
    rows, grid, waves, rpw, iters = t.shape[0], geo["grid"], geo["waves"], geo["rpw"], geo["iters"]
    b, w, s, k = torch.meshgrid(torch.arange(grid), torch.arange(waves), torch.arange(rpw), torch.arange(iters), indexing="ij")
    idx = (b * waves + w) * rpw + s + k * grid * waves * rpw
    idx = torch.where(idx < rows, idx, torch.full_like(idx, rows))
    tz = torch.cat([t, torch.zeros(1, t.shape[1])])
    acc = torch.zeros(grid, waves, rpw, t.shape[1])
    for i in range(iters):
        acc = acc + tz[idx[..., i]]
    m = 1
    while m < rpw:
        acc = acc + acc[:, :, torch.arange(rpw) ^ m]
        m *= 2
    acc = acc[:, :, 0]
    wg = torch.zeros(grid, t.shape[1])
    for i in range(waves):
        wg = wg + acc[:, i]
    out = prior.clone()
    if not det:
        for i in range(grid):
            out = out + wg[i]
        return out
    part = [torch.zeros(t.shape[1]) for _ in range(16)]
    for i in range(grid):
        part[i % 16] = part[i % 16] + wg[i]
    tot = torch.zeros(t.shape[1])
    for p in part:
        tot = tot + p
    return out + tot


def emu_bwd(dy, x, mean, rstd, gamma, add, geo, prior_g, prior_b, det=False, mutant=None):
    D = torch.tensor(float(geo["D"]), dtype=F32)
    x32, d32 = x.float(), dy.float()
    xh = (x32 - mean[:, None]) * rstd[:, None]
    dg = d32 * gamma
    m1 = tree(pair_sum(lanes(dg, geo)[0], geo["nch"])) / D
    m2 = tree(pair_sum(lanes(dg * xh, geo)[0], geo["nch"])) / D
    o = dg - m1[:, None]
    if mutant != "dx_without_xhat_m2":
        o = o - xh * m2[:, None]
    o = rstd[:, None] * o
    if add is not None:
        o = o + add.float()
    tg = d32 * xh
    if mutant == "dgamma_missing_last_row":
        tg = torch.cat([tg[:-1], torch.zeros(1, tg.shape[1])])
    return o.to(BF), col_sums(tg, geo, prior_g, det), col_sums(d32, geo, prior_b, det)


# ------------------------------------------------------------------------------------------------------------------------------------------
# emulation and mutants against the bars
# ------------------------------------------------------------------------------------------------------------------------------------------
def ratio(name, got, ref, terms, c_r, c_a):
    try:
        return check(name, got, ref, terms, c_r, c_a)
    except AssertionError:
        return math.inf


def run_case(inst, mutant=None):
    """worst |err| / bar of every output of the (mutated) emulation, forward with both output types and backward in both column forms"""
    D, one_row, eps = CASES[inst]
    gen = torch.Generator().manual_seed(1000 + D + one_row)
    gf = R.geometry(D, 1, one_row=one_row)
    rows = 3 * 16 * gf["rpw"] + 1                                       # 3 W + 1 of the backward; more than one forward workgroup too
    gf, gb = R.geometry(D, rows, one_row=one_row), R.geometry(D, rows, backward=True, one_row=one_row)
    x, (gamma, beta) = R.make_x(gen, rows, D), R.make_params(gen, D)
    dy, add = R.make_dy(gen, rows, D)
    out = {}
    for dt in (BF, F32):
        y, mean, rstd = emu_fwd(x, gamma, beta, eps, gf, dt, mutant)
        (m64, tm, cm), (r64, tr, cr) = R.stats_bars(x, eps, gf, exact_mean=R.kinds(rows)[1])
        y64, ty, cy = R.y_from_stats(x, mean, rstd, gamma, beta)
        tag = "bf16" if dt == BF else "fp32"
        out["mean"] = ratio(f"{inst} mean", mean, m64, tm, 0.0, cm)
        out["rstd"] = ratio(f"{inst} rstd", rstd, r64, tr, 0.0, cr)
        out["y " + tag] = ratio(f"{inst} y {tag}", y, y64, ty, *((UBF, R.c_bf16(cy)) if dt == BF else (0.0, cy)))
    fwd_mutant = mutant in MUTANTS[:6]
    for label, (mu, rs), ad in (("fwd stats", (mean, rstd) if not fwd_mutant else emu_fwd(x, gamma, beta, eps, gf, BF)[1:], add),
                                ("any stats", R.make_stats(gen, rows), None)):
        for det in (False, True):
            pg, pb = torch.randn(D, generator=gen), torch.randn(D, generator=gen)
            dx, dgm, dbt = emu_bwd(dy, x, mu, rs, gamma, ad, gb, pg, pb, det, mutant)
            dx64, tdx, tg, tb = R.bwd_from_stats(dy, x, mu, rs, gamma, ad)
            key = f"{label} {'det' if det else 'atomic'}"
            out["dx " + key] = ratio(f"{inst} dx {key}", dx, dx64, tdx, UBF, R.c_bf16(R.c_dx(gb)))
            for nm, got, t, prior, which in (("dgamma", dgm, tg, pg, 0), ("dbeta", dbt, tb, pb, 1)):
                ref, terms = R.col_reference(t, prior)
                out[f"{nm} {key}"] = ratio(f"{inst} {nm} {key}", got, ref, terms, 0.0, R.c_col(gb, which, det))
    return out


@pytest.mark.parametrize("inst", list(CASES))
def test_faithful_emulation_passes_every_bar(inst):
    out = run_case(inst)
    assert all(r <= 1.0 for r in out.values()), out


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_fails_a_bar(mutant):
    for inst in CASES:
        if mutant == "last_slot_dropped" and R.geometry(CASES[inst][0], 1, one_row=CASES[inst][1])["nch"] < 2:
            continue                                                    # one chunk slot: nothing to drop but the whole row
        out = run_case(inst, mutant)
        assert any(r > 1.0 for r in out.values()), (mutant, inst, out)


def test_geometry_restates_the_host_dispatch():
    """the widths of the GPU test land on the instance its table names; the trip counts around and above the grid caps"""
    for D, lpr, nch in ((8, 16, 1), (128, 16, 1), (136, 32, 1), (256, 32, 1), (264, 64, 1), (512, 64, 1), (520, 64, 2), (1024, 64, 2),
                        (1032, 64, 3), (1536, 64, 3), (1544, 64, 4), (2048, 64, 4)):
        geo = R.geometry(D, 100)
        assert (geo["lpr"], geo["nch"]) == (lpr, nch), D
        assert (R.geometry(D, 100, one_row=True)["lpr"], R.geometry(D, 100, fused=True)["nch"]) == (64, 4)
    for D, rpw in ((96, 4), (192, 2), (384, 1), (520, 1)):
        f = R.geometry(D, 8192 * rpw)
        assert (f["grid"], f["iters"]) == (2048, 1)
        f = R.geometry(D, 8192 * rpw + 4 * rpw + 1)
        b = R.geometry(D, 8192 * rpw + 16 * rpw + 1, backward=True)
        assert (f["grid"], f["iters"], b["grid"], b["iters"]) == (2048, 2, 512, 2)


# ------------------------------------------------------------------------------------------------------------------------------------------
# argument checks of the two base wrappers (stub library: a launch is a recorded name)
# ------------------------------------------------------------------------------------------------------------------------------------------
def _fwd_args(rows=5, D=128, **kw):
    a = dict(x=torch.zeros(rows, D, dtype=BF), gamma=torch.ones(D), beta=torch.zeros(D), y=torch.zeros(rows, D, dtype=BF),
             mean=torch.zeros(rows), rstd=torch.zeros(rows), eps=1e-6)
    a.update(kw)
    return a


def _bwd_args(rows=5, D=128, **kw):
    a = dict(dy=torch.zeros(rows, D, dtype=BF), x=torch.zeros(rows, D, dtype=BF), mean=torch.zeros(rows), rstd=torch.ones(rows),
             gamma=torch.ones(D), dx=torch.zeros(rows, D, dtype=BF), dgamma=torch.zeros(D), dbeta=torch.zeros(D),
             add=torch.zeros(rows, D, dtype=BF))
    a.update(kw)
    return a


def test_layernorm_fwd_checks_its_arguments(stub):
    from medmoe_amd import ops
    name = "medmoe_layernorm_fwd"
    good = [_fwd_args(), _fwd_args(D=2048), _fwd_args(D=8), _fwd_args(mean=None), _fwd_args(rstd=None), _fwd_args(mean=None, rstd=None),
            _fwd_args(mean=torch.zeros(9), rstd=torch.zeros(2, 5)[0]), _fwd_args(y=torch.zeros(5, 128))]
    for a in good:
        ops.layernorm_fwd(**a)
    assert stub.calls.count(name) == len(good)
    bad = [_fwd_args(gamma=torch.ones(120)), _fwd_args(beta=torch.ones(136)), _fwd_args(gamma=torch.ones(256)[::2]),
           _fwd_args(beta=torch.ones(128, dtype=F64)), _fwd_args(gamma=torch.ones(128, dtype=BF)), _fwd_args(mean=torch.zeros(4)),
           _fwd_args(rstd=torch.zeros(4)), _fwd_args(mean=torch.zeros(5, dtype=F64)), _fwd_args(rstd=torch.zeros(10)[::2]),
           _fwd_args(D=132), _fwd_args(D=2056), _fwd_args(gamma=None), _fwd_args(y=torch.zeros(5, 128, dtype=torch.float16))]
    for a in bad:
        with pytest.raises((ValueError, TypeError)):
            ops.layernorm_fwd(**a)
    assert stub.calls.count(name) == len(good)


def test_layernorm_bwd_checks_its_arguments(stub):
    from medmoe_amd import ops
    rows_dev = torch.zeros(1, dtype=torch.int32)
    good = [(_bwd_args(), "medmoe_layernorm_bwd"), (_bwd_args(D=2048), "medmoe_layernorm_bwd"), (_bwd_args(add=None), "medmoe_layernorm_bwd"),
            (_bwd_args(dgamma=None, dbeta=None), "medmoe_layernorm_bwd"), (_bwd_args(mean=torch.zeros(2, 9)[1]), "medmoe_layernorm_bwd"),
            (_bwd_args(rows_dev=rows_dev), "medmoe_layernorm_bwd_rows"), (_bwd_args(det=ops.DetScratch("cpu")), "medmoe_layernorm_bwd_det")]
    for a, _ in good:
        ops.layernorm_bwd(**a)
    launches = [c for c in stub.calls if not c.endswith("_scratch")]
    assert launches == [n for _, n in good]
    bad = [_bwd_args(gamma=torch.ones(120)), _bwd_args(gamma=torch.ones(128, dtype=BF)), _bwd_args(dgamma=torch.zeros(120)),
           _bwd_args(dbeta=torch.zeros(256)[::2]), _bwd_args(dbeta=torch.zeros(128, dtype=F64)), _bwd_args(dbeta=None), _bwd_args(dgamma=None),
           _bwd_args(mean=torch.zeros(4)), _bwd_args(rstd=torch.zeros(4)), _bwd_args(mean=None), _bwd_args(rstd=torch.zeros(5, dtype=F64)),
           _bwd_args(add=torch.zeros(4, 128, dtype=BF)), _bwd_args(add=torch.zeros(5, 128)), _bwd_args(add=torch.zeros(5, 256, dtype=BF)[:, ::2]),
           _bwd_args(D=132), _bwd_args(D=2056), _bwd_args(mean=torch.zeros(4), rows_dev=rows_dev),
           _bwd_args(gamma=torch.ones(120), det=ops.DetScratch("cpu"))]
    for a in bad:
        with pytest.raises((ValueError, TypeError)):
            ops.layernorm_bwd(**a)
    assert [c for c in stub.calls if not c.endswith("_scratch")] == [n for _, n in good]
