"""Float64 restatement of the LayerNorm kernels (csrc/norm.hip, the two fused launches of csrc/dropout.hip) on the bf16-rounded inputs, the
launch geometry the host code picks, and the per-element bars of tests/test_layernorm_gpu.py and tests/test_layernorm_bars_host.py.
Device-agnostic: every function computes where its inputs live.

An element passes when |got - ref| <= c_r |ref| + c_a * terms (`check` of test_glue_kernels_gpu.py): c_r = UBF for a bf16 output, 0 for an
fp32 one; `terms` is the float64 magnitude the roundings act on; c_a = g(n) = n U / (1 - n U) (Higham's gamma_n, U = 2^-24) for the longest
chain of n fp32 roundings behind the element.  Every n below is COUNTED FROM THE KERNEL SOURCE as a function of the geometry - none is
fitted to an observed error.  A compiler that contracts a multiply and an add into one FMA only removes roundings from a chain.

Geometry (layernorm_fwd_impl / layernorm_bwd_impl):
    LPR   lanes per row: 16 for D <= 128, 32 for D <= 256, else 64; 64 always under option 16 (bit 0 forward, bit 1 backward) and in the
          two fused kernels
    NCH   chunk slots of 8 columns per lane: ceil(D / 8 / 64); 1 whenever LPR < 64.  The fused kernels always loop over 4 slots, the empty
          ones add nothing
    RPW   rows per wave = 64 / LPR; waves per workgroup: 4 forward, 16 backward; grid = min(ceil(rows / (waves RPW)), 2048 forward | 512
          backward); a wave makes `iters` = ceil(rows / (grid waves RPW)) trips through the row loop

Chains (L = log2(LPR)):
  row sum of k-times-rounded elements, divided by D        S(k) = k + 1 + 4 NCH + L + 1
      a lane adds pairs (`s += a + b`: 1 rounding for the pair, then at most 4 NCH accumulations), the xor tree adds L levels, `/ D` one more
  mean                                                     S(0), on sum |x| / D
  rstd                                                     relative: (2 + 1 + 8 NCH + L + 2) / 2 + 2 RSQRT_ULP, plus the fp32 mean's share
      d = x - mean (1 rounding: 2 on d^2), d * d (1), `sq += d * d` one value at a time (8 NCH), the tree (L), `/ D` and `+ eps` (2): every
      term is non-negative, so the count is a relative error of var + eps and half of it reaches its inverse square root.  rsqrtf itself:
      see RSQRT_ULP; one ulp is at most 2 U relative.  The kernel's squares are taken around ITS mean m' = mean + e: sum (x - m')^2 =
      sum (x - mean)^2 + D e^2 exactly, so var grows by e^2 <= (mean's bar)^2 and rstd moves by at most rstd e^2 / (2 (var + eps)).
  y given the kernel's own fp32 mean, rstd                 4: (x - mean), * rstd, * gamma, + beta; on |(x - mean) rstd gamma| + |beta|
  dx given mean, rstd                                      S(3) + 7, on rstd (|dy g| + mean|dy g| + |xhat| mean|dy g xhat|) + |add|
      xhat = (x - mean) * rstd (2), dg = dy * g (1).  m1 = rowsum(dg) / D is S(1) on A1 = mean|dg|; m2 = rowsum(dg * xhat) / D is S(4) on
      A2 = mean|dg xhat| (elements carry 1 + 2, their product one more).  o = rs * (dg - m1 - xhat * m2): xhat * m2 carries 2 + S(4) + 1;
      `dg - m1`, `- xhat * m2` and `rs *` round once each on at most Q = |dg| + A1 + |xhat| A2.  Per unit of rs U that is 4 on |dg|,
      S(1) + 3 on A1 and S(4) + 5 on |xhat| A2, at most S(4) + 5 on Q; `+ add` rounds rs Q + |add| once more: S(4) + 6 = S(3) + 7.
  dgamma / dbeta column sums                               k + iters + log2(RPW) + 16 + W, on sum_rows |term| + |prior|
      k = 3 for dgamma (xhat 2, dy * xhat 1), 0 for dbeta; a lane accumulates one term per trip (iters); the rows of a wave meet by
      log2(RPW) shuffle adds; 16 waves are added in LDS; W = grid for the atomic form (one atomicAdd per workgroup onto the running value,
      the prior included), ceil(grid / 16) + 16 + 1 for the ordered reduce (det_sum_records: 16 strided partial sums, their sum, `+=`)
  x1 of the fused launches                                 2: one fp32 product, one sum; then the bf16 rounding (c_r)"""
import math

import numpy as np
import torch

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
UBF = 2.0 ** -8
# rsqrtf: the one term that cannot be counted from the source.  The ROCm 7.0 headers state no accuracy for it (clang's __clang_hip_math.h only
# forwards to __ocml_rsqrt_f32, and no document shipped with the toolchain mentions the function), so 2 ulp is allowed; the public HIP math
# documentation lists 1 ulp.
RSQRT_ULP = 2
FWD_WAVES, BWD_WAVES, FWD_GRID_CAP, BWD_GRID_CAP = 4, 16, 2048, 512
KINDS = ("normal", "offset", "large", "const", "zero", "normal", "offset", "normal")      # row r is of kind KINDS[r % 8]


def g(n):
    return n * U / (1.0 - n * U)


def c_bf16(c_a):
    """c_a of an output that is then rounded to bf16: |bf16(o) - ref| <= UBF |o| + |o - ref| <= UBF |ref| + (1 + UBF) |o - ref|"""
    return c_a * (1.0 + UBF)


def geometry(D, rows, backward=False, one_row=False, fused=False):
    lpr = 64 if (one_row or fused) else 16 if D <= 128 else 32 if D <= 256 else 64
    nch = 4 if fused else (D // 8 + 63) // 64 if lpr == 64 else 1
    rpw = 64 // lpr
    waves, cap = (BWD_WAVES, BWD_GRID_CAP) if backward else (FWD_WAVES, FWD_GRID_CAP)
    per = waves * rpw
    grid = max(1, min((rows + per - 1) // per, cap))
    return dict(D=D, rows=rows, lpr=lpr, nch=nch, rpw=rpw, waves=waves, per=per, grid=grid, iters=(rows + grid * per - 1) // (grid * per),
                L=int(math.log2(lpr)))


def row_sum_chain(geo, k):
    return k + 1 + 4 * geo["nch"] + geo["L"] + 1


def f32_scalar(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------------------------------------------------
def make_x(gen, rows, D):
    """bf16 [rows, D] on the CPU, row r of kind KINDS[r % 8]: normal randn * 2 + 0.5; offset 4 + 0.25 randn (variance far below the squared
    mean); large 1e3 randn; const one bf16 value; zero."""
    x = torch.randn(rows, D, generator=gen) * 2 + 0.5
    kind = torch.arange(rows) % len(KINDS)
    for k, name in enumerate(KINDS):
        sel = kind == k
        n = int(sel.sum())
        if not n:
            continue
        if name == "offset":
            x[sel] = 4 + 0.25 * torch.randn(n, D, generator=gen)
        elif name == "large":
            x[sel] = 1e3 * torch.randn(n, D, generator=gen)
        elif name == "const":
            x[sel] = (torch.randn(n, 1, generator=gen) * 3 + 0.37).to(BF).float().expand(n, D)
        elif name == "zero":
            x[sel] = 0.0
    return x.to(BF)


def kinds(rows):
    """names of the rows' kinds, and the mask of constant rows (const and zero)"""
    k = [KINDS[r % len(KINDS)] for r in range(rows)]
    return k, torch.tensor([n in ("const", "zero") for n in k])


def make_params(gen, D):
    """gamma of both signs away from zero, beta non-zero (fp32)"""
    sign = torch.where(torch.rand(D, generator=gen) < 0.5, -1.0, 1.0)
    gamma = (0.5 + torch.rand(D, generator=gen)) * sign
    beta = torch.randn(D, generator=gen) * 0.3
    beta = torch.where(beta == 0, torch.full_like(beta, 0.125), beta)
    return gamma.to(F32), beta.to(F32)


def make_dy(gen, rows, D):
    """bf16 upstream gradient, rows scaled by 1, 1e-2 and 30 in turn; bf16 residual gradient `add`"""
    scale = torch.tensor([1.0, 1e-2, 30.0])[torch.arange(rows) % 3].reshape(rows, 1)
    return (torch.randn(rows, D, generator=gen) * scale).to(BF), torch.randn(rows, D, generator=gen).to(BF)


def make_stats(gen, rows):
    """arbitrary per-row statistics for the backward: a statistic read at the wrong row shows"""
    return torch.randn(rows, generator=gen).to(F32), (0.2 + 2 * torch.rand(rows, generator=gen)).to(F32)


# ------------------------------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------------------------------
def stats(x, eps):
    """float64 mean and 1 / sqrt(var + eps): biased variance, two passes; eps as the fp32 value the kernel receives"""
    x = x.to(F64)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + f32_scalar(eps)), var


def stats_bars(x, eps, geo, exact_mean=None):
    """(mean64, terms, c_a), (rstd64, terms, c_a) for the fp32 statistics a kernel of geometry `geo` writes.  exact_mean: mask of the rows
    whose fp32 mean is exact (constant rows: c * D is exact in fp32 for a bf16 c and D <= 2048) - their rstd gets no share for the mean."""
    mean, rstd, var = stats(x, eps)
    t_mean = x.to(F64).abs().mean(-1)
    c_mean = g(row_sum_chain(geo, 0))
    e = c_mean * t_mean                                                # the fp32 mean's own bar
    n_var = 2 + 1 + 8 * geo["nch"] + geo["L"] + 2
    rel = g(n_var)
    c_rstd = rel / (2.0 * (1.0 - rel)) + g(2 * RSQRT_ULP)              # |(1 + r)^-1/2 - 1| <= r / (2 (1 - r)) for |r| < 1
    shift = e * e / (2.0 * (var + f32_scalar(eps)))
    if exact_mean is not None:
        shift = torch.where(exact_mean.to(shift.device), torch.zeros_like(shift), shift)
    t_rstd = rstd * (1.0 + shift / c_rstd)
    return (mean, t_mean, c_mean), (rstd, t_rstd, c_rstd)


def y_from_stats(x, mean, rstd, gamma, beta):
    """y64 = (x - mean) * rstd * gamma + beta from the fp32 statistics the kernel wrote, its terms, c_a"""
    p = (x.to(F64) - mean.to(F64)[:, None]) * rstd.to(F64)[:, None] * gamma.to(F64)
    b = beta.to(F64)
    return p + b, p.abs() + b.abs(), g(4)


def x1_reference(res, z, scale_rows):
    """x1 = res + scale_rows * z (scale_rows float64 [rows, 1] or [rows, D], fp32 values), terms, c_a: one product, one sum"""
    p = z.to(F64) * scale_rows
    r = res.to(F64)
    return r + p, r.abs() + p.abs(), g(2)


# ------------------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------------------
def bwd_from_stats(dy, x, mean, rstd, gamma, add=None):
    """dx64 [+ add], its terms, and the per-row terms of dgamma (dy * xhat) and dbeta (dy); mean / rstd are inputs of the backward, so this
    is the true reference whatever they hold"""
    rs = rstd.to(F64)[:, None]
    xh = (x.to(F64) - mean.to(F64)[:, None]) * rs
    d = dy.to(F64)
    dg = d * gamma.to(F64)
    m1, m2 = dg.mean(-1, keepdim=True), (dg * xh).mean(-1, keepdim=True)
    a1, a2 = dg.abs().mean(-1, keepdim=True), (dg * xh).abs().mean(-1, keepdim=True)
    dx = rs * (dg - m1 - xh * m2)
    terms = rs.abs() * (dg.abs() + a1 + xh.abs() * a2)
    if add is not None:
        dx = dx + add.to(F64)
        terms = terms + add.to(F64).abs()
    return dx, terms, d * xh, d


def c_dx(geo):
    return g(row_sum_chain(geo, 3) + 7)


def c_col(geo, which, det=False):
    """chain of a dgamma (which = 0) or dbeta (1) column sum"""
    across = (geo["grid"] + 15) // 16 + 16 + 1 if det else geo["grid"]
    return g((0 if which else 3) + geo["iters"] + int(math.log2(geo["rpw"])) + 16 + across)


def col_reference(terms, prior):
    """float64 column sum onto the prior, and the magnitude behind it"""
    p = prior.to(F64)
    return p + terms.sum(0), p.abs() + terms.abs().sum(0)
