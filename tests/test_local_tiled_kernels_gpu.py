"""The tiled local-loss kernels that run at 64, 196 and 256 regions, each one alone against the float64 restatement of its contract in
tests/local_tiled_reference.py, called through medmoe_amd.ops as the engine calls them, EVERY element of every output judged:
the three score kernels (loss.hip local_scores_kernel, gemm_scores.hip scores512_kernel<NTT, false / true>), all fourteen
local_pair2_kernel instances, the forward launch of local_pair3_kernel, local_pair_kernel on precomputed tiles, scale_blocks(_ragged)
and words_prep(_ragged).

The kernel is forced, never guessed: option 6 selects scores512 for the untransposed output (`scores512()` sets it and restores the
default 1 in a `finally`), and the kernel also switches on M = B*HW >= 1024; `local_pair3_chunks` is restored to 0 likewise.
Every output buffer is allocated by `guarded` (sentinel body + sentinel tail): after the launch every element the contract says is
written no longer holds the sentinel, every other element and the tail are bit-identical.  Pair-kernel inputs are SYNTHESISED (fp16
log-probabilities of a float64 softmax, arbitrary lse, a bf16 Gram matrix in the kernel's own layout), with NaN bit patterns on the
region rows >= HW that the score kernels never write: a read of one shows.

Which test reaches what (n = captions of the launch, CAPB = 16 / 8 / 4 / 4 / 2 captions per scores512 workgroup; every launch has an odd
n, a non-zero col_base / row_base, a permuted cap_list, lengths at both ends 16 (ntt - 1) + 1 and min(16 ntt, T) of its class, one between,
one beyond T, a caption shorter than its class (1 word; 5 words in class 3: whole 16-word tiles masked) and, at 196 regions, an EMPTY one):

  kernel instance                         reached through                                  shapes (B x HW, T; D = 128 unless noted)         tests
  local_scores_kernel<1..5>               local_scores_ragged, option 6 = 0               6 x 196 (M = 1176: 9 tiles + 24 rows), D 192 / 768  scores_128row
  local_scores_kernel<1..5>               local_scores_ragged, M < 1024                   3 x 196 (M = 588), 3 x 256                          scores_128row
  local_scores_kernel<1, 3, 5>            local_scores_ragged, option 6 = 0               4 x 256 (M = 1024), 17 x 64 and 3 x 64 (<1>)       scores_128row
  local_scores_kernel<1, 2, 5>            local_scores (uniform layout)                   3 x 64 T 16, 3 x 196 T 25, 3 x 196 T 77            scores_uniform
  scores512_kernel<1..5, false>           local_scores_ragged, M >= 1024                  6 x 196 (4 tiles + 152 rows), 4 x 256 (M = 1024,    scores_512
                                                                                          n = CAPB + 1), 17 x 64 (<1>), D 192 / 768,
                                                                                          265 tiles > 256 workgroups (class 5, n = 105)
  scores512_kernel<1..5, true>            local_scores_t, image-major (ld = 224,          6 x 196, 3 x 196, 17 x 64 (<1>, pw 64), D 160 /    scores_transposed
                                          bs = rows * 224)                                768, 265 tiles (class 5, n = 105)
  scores512_kernel<1..5, true>            local_scores_t, word-row (ld = B * 208,         the same                                           scores_transposed
                                          bs = 208)
  all five forms, <2>                     a live word 65536 below the row maximum         6 x 196                                            scores_clamp_to_logp_min
  local_pair2_kernel<4,1> <13,1..5>       local_pair2_ragged, gsim given and None         2 x 64 T 16, 2 x 196 T 77, 2 x 256 T 77            pair2_ragged
    <16,1..5>
  local_pair2_kernel<4,1> <13,2> <13,5>   local_pair2 (uniform: att, cap_list null)       2 x 64 T 16, 2 x 196 T 25, 2 x 196 T 77            pair2_uniform
  local_pair_kernel<4,1> <13,2> <13,5>    local_pair with precomputed tiles, forward and  2 x 64 T 16, 2 x 196 T 25, 2 x 196 T 77            local_pair_precomputed
    PRECOMP                               backward launch, gsim given and None
  local_pair3_kernel<64,1,false>          local_pair3 forward, image-major and word-row,  2 x 64 T 16, 41 captions                           pair3_forward_64
  local_pair3_kernel<196,1..5,false>      one chunk and the automatic spread              2 x 196 T 77, 114 captions (four epochs per class) pair3_forward_196
  Gram layout [B*HWp][GW], lpos columns   gemm_nt(col_perm = True) as the engine calls it 64 / 196 / 256 regions                             gram_layout_is_the_producers
  scale_blocks_kernel                     scale_blocks, scale_blocks_ragged               8 x 208 rows x 5120 columns (> one grid pass)      scale_blocks
  words_prep_kernel, words_norm_kernel    words_prep, words_prep_ragged (wT / None)       D 128, 768; ragged None also D 100                 words_prep_uniform, words_prep_ragged

Bars.  An element passes when |got - ref| <= c_r |ref| + (absolute part); `check` of test_glue_kernels_gpu.py is used with the absolute
part as `terms` and c_a = 1, through the `Worst` reporter of test_attention_gpu.py.  c_r is the output format's half ulp: UBF = 2^-8 for
bf16, UH = 2^-11 for fp16, 0 for fp32.  The absolute parts are first-order error propagations COUNTED FROM THE KERNEL SOURCE in units of
U = 2^-24, with every magnitude (sum |term|) taken from the float64 reference; none is set from an observed error:
  MFMA chain over K         (32 + K / 32) U sum|a b|: K / 32 accumulator roundings and the 32 exact bf16 products summed inside one
                            v_mfma_f32_16x16x32_bf16, bounded as 32 sequential fp32 additions
  fp32 sum of n terms       n U sum|term|
  v_exp_f32 / v_log_f32     1 ulp = 2 U relative; __expf(x) = exp2(x log2 e) adds 2 |x| U (the constant and the product);
                            log: 4 U (|log| + 1) absolute
  division, sqrt, product   U each
`score_bars` and `pair_bars` hold the propagation; their docstrings name the source lines behind every count.

The staged references: A (bf16) is judged against the float64 A on its own; sim, dS, U, num and n2 are then judged against the reference
evaluated on the kernel's OWN bf16 A, as the kernels themselves use it.

Ratios.  The worst |err| / bar seen on an MI355X is in the docstring of every test.  Two kinds stand out and are meant to:
  0.9 .. 0.99 on every fp16 / bf16 output (lp, A, dS, U).  The bar's relative part IS the format's half ulp, which round-to-nearest
      reaches at the bottom of a binade and some element among 10^5 .. 10^7 all but does; a correct kernel cannot pass it, because what
      fp32 arithmetic adds in front of the rounding is the absolute part, on top.  A wider relative part would hide a wrong last bit.
  0.002 .. 0.05 on the fp32 outputs behind long sums (lse, sim, num, n2).  Their bars are worst-case sums n U sum|term| (every rounding
      with one sign); the errors of 200 .. 800 roundings add like a random walk, sqrt(n) of them.  The bars still resolve a wrong
      operand: num taken from the bf16 A instead of the unrounded one lands at 30 .. 280 times the bar, a dropped row sum in dS at 2000
      times, the last region tile's row mask on every tile at 2000 times.
The file was run against single-line arithmetic / mask changes of local_pair2_kernel (row mask, t <= cap, dS without rd), of both
scores512 epilogues (no clamp to LOGP_MIN) and of the pair3 forward launch (num from the bf16 A): each one fails tests here."""
import contextlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from local_tiled_reference import LN2, LOGP_MIN, LOGP_MIN_BITS, clamp_caps, live_words, ref_pair_bwd, ref_pair_fwd, ref_scores
from test_attention_gpu import Worst
from test_glue_kernels_gpu import BF, DEV, F32, F64, I32, SENT, U, UBF, _BITS, guarded, tail_ok
from test_pair3_onepass_gpu import caps_all_classes

pytestmark = pytest.mark.gpu

F16 = torch.float16
UH = 2.0 ** -11                     # one fp16 rounding (RNE, 11 significant bits)
LOG2E = 1.4426950408889634
T1, T2, EPS = 4.0, 5.0, 1e-8
CAPB = {1: 16, 2: 8, 3: 4, 4: 4, 5: 2}
NAN16 = 0x7E00                      # an fp16 NaN: what the never-written region rows of a pair tile hold


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


@contextlib.contextmanager
def scores512(ops, on):
    """force the untransposed score kernel: option 6 = 1 scores512 (for M >= 1024), 0 the 128-row kernel; the default 1 restored"""
    try:
        ops.set_option(6, 1 if on else 0)
        yield
    finally:
        ops.set_option(6, 1)


def ibits(t):
    return t.contiguous().view(_BITS.get(t.dtype, torch.int16))


def assert_written(t, mask, what):
    """the elements under `mask` no longer hold the sentinel, all the others still do (t and mask in the same logical frame)"""
    b, s = ibits(t), SENT[t.dtype]
    assert bool((b[mask] != s).all()), what + ": an element the contract writes still holds the sentinel"
    assert bool((b[~mask] == s).all()), what + ": an element outside the contract was written"


def lpos(r):
    """loss.hip lpos(): position of region r in the k-order the Gm.A product of local_pair2 reads"""
    o = r & 31
    return (r & ~31) + (((o & 15) >> 2) << 3) + ((o >> 4) << 2) + (o & 3)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the score kernels
# ------------------------------------------------------------------------------------------------------------------------------
def class_lens(ntt, T, n, empty):
    """n caption lengths for a launch of class ntt: both ends, one between, one beyond T where the class reaches T, a caption shorter than
    the class, an empty one (if asked and n >= 5), then lengths spread over the class"""
    lo, hi = 16 * (ntt - 1) + 1, min(16 * ntt, T)
    lens = [lo, hi if hi < T else T + 9, (lo + hi) // 2]
    if n >= 5:
        lens += [5 if ntt == 3 else 1, 0 if empty else lo + 1]
    k = 0
    while len(lens) < n:
        lens.append(lo + (5 * k + 3) % (hi - lo + 1))
        k += 1
    return lens[:n]


class ScoreCase:
    """bf16 ctx [B*HW, D] and words [Bc, T, D], the launch's caption list (a permuted subset of the Bc captions; None: uniform layout, all
    captions in order) and the float64 reference of the launch, on the GPU"""

    def __init__(self, B, HW, T, D, ntt, lens, seed, uniform=False, log2=False, extra=3):
        g = torch.Generator().manual_seed(seed)
        self.B, self.HW, self.T, self.D, self.ntt, self.TP, self.n = B, HW, T, D, ntt, 16 * ntt, len(lens)
        self.HWP = (HW + 15) // 16 * 16
        self.Bc = Bc = self.n + (0 if uniform else extra)
        scale = 0.5 if D <= 192 else 0.3
        self.ctx = (torch.randn(B * HW, D, generator=g) * scale).to(BF).to(DEV)
        self.words = (torch.randn(Bc, T, D, generator=g) * scale).to(BF).to(DEV)
        self.members = torch.arange(Bc) if uniform else torch.randperm(Bc, generator=g)[:self.n]
        all_lens = torch.randint(1, T + 1, (Bc,), generator=g)
        all_lens[self.members] = torch.tensor(lens)
        self.cap = all_lens.to(I32).to(DEV)
        self.caps = clamp_caps(lens, T, self.TP)
        self.mem_dev = self.members.to(I32).to(DEV)
        self.log2 = log2

    def reference(self):
        return ref_scores(self.ctx.view(self.B, self.HW, self.D).to(F64), self.words[self.members.to(DEV)].to(F64),
                          torch.tensor(self.caps, device=DEV), self.TP, log2=self.log2)


def score_bars(r, D, TP, log2):
    """(absolute bar of lse, absolute part of the bar of lp); lp adds c_r = UH.  Untransposed kernels (loss.hip:954-988, gemm_scores.hip
    epilogue): S from D / 32 MFMAs; mx exact; sm = sum_t __expf(S - mx) - each term (3 |x| + 2) U relative (the difference, the constant,
    the product, v_exp_f32), the sum of <= 20 in-lane terms and two shuffle adds (TP / 4 + 2) U; lse = mx + __logf(sm): 4 U (|log sm| + 1)
    and U |lse|; a shift of every S by E_S moves lse by at most max_t E_S.  lp = S - lse: E_S + E_lse + U |lp|, then fmaxf and the fp16
    rounding (2^-25 absolute below the normal range).  Transposed kernel (epilogue_t): the same in the log2 domain - mx log2 e (2 U |mx|),
    exp2(fma(S, log2 e, -mx)) (2 |x| + 3) U, lse2 = mx + v_log_f32(sm), output fma(S, log2 e, -lse2): log2 e (E_S + U |S|) + E_lse2 + U |lp2|,
    and the stored lse = lse2 ln 2 adds 2 U |lse|."""
    live = r["live"]
    z = torch.zeros_like(r["S"])
    E_S = torch.where(live, (32 + D / 32) * U * r["sabs"], z)
    E_max = E_S.amax(-1)
    px = (r["p"] * (3 * r["x"].abs() + 3)).sum(-1)
    logsm = (r["lse"] - r["mx"]).abs()
    k = LOG2E if log2 else 1.0
    E_dom = k * (E_max + (2 * U * r["mx"].abs() if log2 else 0.0)) + (px + TP / 4 + 2) * U + 4 * U * (k * logsm + 1) + U * k * r["lse"].abs()
    E_lse = E_dom / k + (2 * U * r["lse"].abs() if log2 else 0.0)
    E_lp = k * (E_S + (U * r["S"].abs() if log2 else 0.0)) + E_dom[..., None] + U * r["lp"].abs() + 2.0 ** -25
    return E_lse, torch.where(live, E_lp, z)


def judge_scores(w, c, r, lp_bits, lse_got):
    """lp_bits int16 [B, HW, n, TP] (the fp16 output), lse_got fp32 [B, HW, n]: every element"""
    live = r["live"]
    assert bool((lp_bits[~live] == LOGP_MIN_BITS).all()), "a word at or beyond cap does not hold LOGP_MIN exactly"
    lp_got = lp_bits.view(F16).to(F64)
    assert bool(torch.isfinite(lp_got).all()) and bool(torch.isfinite(lse_got).all()), "lp / lse not finite"
    E_lse, E_lp = score_bars(r, c.D, c.TP, c.log2)
    z = torch.zeros_like(r["S"])
    w("lse", lse_got, r["lse"], 0.0, E_lse)
    w("lp", torch.where(live, lp_got, z), torch.where(live, r["lp"], z), UH, E_lp)


def run_untransposed(ops, c, uniform=False):
    """local_scores_ragged (or local_scores): returns (lp bits [B, HW, n, TP], lse [B, HW, n]) after the written / untouched checks"""
    B, HW, HWP, n, TP, Bc = c.B, c.HW, c.HWP, c.n, c.TP, c.Bc
    cb = 0 if uniform else 32
    ldp = Bc * TP if uniform else cb + n * TP + 16
    abuf, a = guarded((B, HWP, ldp), BF)
    lbuf, lse = guarded((B, Bc, HWP), F32)
    if uniform:
        ops.call("local_scores", c.ctx, c.words, c.cap, a, lse, B, Bc, HW, c.T, c.D)
    else:
        ops.call("local_scores_ragged", c.ctx, c.words, c.cap, a, lse, B, Bc, HW, c.T, c.D, c.mem_dev, n, c.ntt, cb, ldp)
    torch.cuda.synchronize()
    wa = torch.zeros(B, HWP, ldp, dtype=torch.bool, device=DEV)
    wa[:, :HW, cb:cb + n * TP] = True
    wl = torch.zeros(B, Bc, HWP, dtype=torch.bool, device=DEV)
    wl[:, c.members.to(DEV), :HW] = True
    assert_written(a, wa, "lp")
    assert_written(lse, wl, "lse")
    assert tail_ok(abuf, a.numel()) and tail_ok(lbuf, lse.numel())
    return (ibits(a)[:, :HW, cb:cb + n * TP].reshape(B, HW, n, TP), lse[:, c.members.to(DEV), :HW].permute(0, 2, 1))


def run_transposed(ops, c, form):
    """local_scores_t in one of its two layouts: element (row, image, region) at row * ld + image * bs + region"""
    B, HW, HWP, n, TP, Bc = c.B, c.HW, c.HWP, c.n, c.TP, c.Bc
    rb = 16
    rows = rb + n * TP + 16
    pw = 64 if HW == 64 else (224 if form == "image" else 208)
    ld, bs = (pw, rows * pw) if form == "image" else (B * pw, pw)
    abuf, a = guarded((B * rows * pw,), BF)
    lbuf, lse = guarded((B, Bc, HWP), F32)
    ops.call("local_scores_t", c.ctx, c.words, c.cap, a, lse, B, Bc, HW, c.T, c.D, c.mem_dev, n, c.ntt, rb, ld, bs)
    torch.cuda.synchronize()
    logical = a.view(B, rows, pw) if form == "image" else a.view(rows, B, pw).permute(1, 0, 2)          # [image][row][region]
    wa = torch.zeros(B, rows, pw, dtype=torch.bool, device=DEV)
    wa[:, rb:rb + n * TP, :HW] = True
    wl = torch.zeros(B, Bc, HWP, dtype=torch.bool, device=DEV)
    wl[:, c.members.to(DEV), :HW] = True
    assert_written(logical.contiguous(), wa, "lpT")
    assert_written(lse, wl, "lse")
    assert tail_ok(abuf, a.numel()) and tail_ok(lbuf, lse.numel())
    lp = ibits(logical.contiguous())[:, rb:rb + n * TP, :HW].reshape(B, n, TP, HW).permute(0, 3, 1, 2)
    return lp, lse[:, c.members.to(DEV), :HW].permute(0, 2, 1)


def n_caps(HW, ntt):
    """CAPB + 1 captions (one workgroup column of scores512 plus one caption; odd); at 196 regions at least five, so that the short and the
    empty caption fit (class 5: 2 CAPB + 1)"""
    return max(CAPB[ntt] + 1, 5) if HW == 196 else CAPB[ntt] + 1


R128 = ([(6, 196, 77, 128, ntt, True) for ntt in range(1, 6)] + [(3, 196, 77, 128, ntt, False) for ntt in range(1, 6)]
        + [(4, 256, 77, 128, ntt, True) for ntt in (1, 3, 5)] + [(3, 256, 77, 128, ntt, False) for ntt in range(1, 6)]
        + [(17, 64, 16, 128, 1, True), (3, 64, 16, 128, 1, False), (6, 196, 77, 192, 3, True), (6, 196, 77, 768, 5, True)])


@pytest.mark.parametrize("B,HW,T,D,ntt,force", R128)
def test_scores_128row(ops, B, HW, T, D, ntt, force):
    """local_scores_kernel<NTT> through local_scores_ragged: forced by option 6 = 0 where M >= 1024, reached by M < 1024 with the option at
    its default.  M = 1176 is nine full 128-row tiles plus 24 rows with every image boundary inside a tile; D = 192 is three K-steps.
    Seen: lse 0.026 .. 0.048, lp 0.94 .. 0.98 (see "Ratios" in the module docstring)."""
    assert force == (B * HW >= 1024)
    c = ScoreCase(B, HW, T, D, ntt, class_lens(ntt, T, n_caps(HW, ntt), HW == 196), seed=1000 * HW + 10 * B + ntt)
    w = Worst(f"local_scores_kernel<{ntt}> {B}x{HW} D={D}")
    with scores512(ops, not force):
        lp, lse = run_untransposed(ops, c)
    judge_scores(w, c, c.reference(), lp, lse)
    w.report()


@pytest.mark.parametrize("B,HW,T", [(3, 64, 16), (3, 196, 25), (3, 196, 77)])
def test_scores_uniform(ops, B, HW, T):
    """local_scores_kernel<1 / 2 / 5> through local_scores: cap_list null, five captions (odd: the last tile's second caption slot is
    clamped and its stores predicated), every caption Tp columns wide.  Seen: lse 0.021 .. 0.028, lp 0.97."""
    ntt = (T + 15) // 16
    c = ScoreCase(B, HW, T, 128, ntt, [T + 9, 1, T // 2, min(5, T), 0], seed=HW + T, uniform=True)
    w = Worst(f"local_scores_kernel<{ntt}> uniform {B}x{HW}")
    lp, lse = run_untransposed(ops, c, uniform=True)
    judge_scores(w, c, c.reference(), lp, lse)
    w.report()


R512 = ([(6, 196, 77, 128, ntt, 0) for ntt in range(1, 6)] + [(4, 256, 77, 128, ntt, 0) for ntt in range(1, 6)]
        + [(17, 64, 16, 128, 1, 0), (6, 196, 77, 192, 2, 0), (6, 196, 77, 768, 4, 0), (6, 196, 77, 128, 5, 105)])


@pytest.mark.parametrize("B,HW,T,D,ntt,n", R512)
def test_scores_512(ops, B, HW, T, D, ntt, n):
    """scores512_kernel<NTT, false> through local_scores_ragged with M >= 1024 (M = 1024 exactly at 4 x 256): M = 1176 is four full 256-row
    tiles plus 152 rows; n = CAPB + 1 captions leave all but one caption slot of the last workgroup column empty; D = 192 is six sub-steps;
    n = 105 in class 5 is 5 x 53 = 265 tiles for 256 workgroups, so nine workgroups run the persistent loop twice.
    Seen: lse 0.016 .. 0.046, lp 0.955 .. 0.985."""
    assert B * HW >= 1024
    c = ScoreCase(B, HW, T, D, ntt, class_lens(ntt, T, n or n_caps(HW, ntt), HW == 196), seed=2000 * HW + 10 * B + ntt + n)
    w = Worst(f"scores512_kernel<{ntt},false> {B}x{HW} D={D} n={c.n}")
    with scores512(ops, True):
        lp, lse = run_untransposed(ops, c)
    judge_scores(w, c, c.reference(), lp, lse)
    w.report()


RT = ([(6, 196, 77, 128, ntt, 0) for ntt in range(1, 6)] + [(3, 196, 77, 128, ntt, 0) for ntt in (2, 5)]
      + [(17, 64, 16, 128, 1, 0), (6, 196, 77, 160, 3, 0), (6, 196, 77, 768, 1, 0), (6, 196, 77, 128, 5, 105)])


@pytest.mark.parametrize("form", ["image", "word"])
@pytest.mark.parametrize("B,HW,T,D,ntt,n", RT)
def test_scores_transposed(ops, B, HW, T, D, ntt, n, form):
    """scores512_kernel<NTT, true> through local_scores_t, image-major (ld = 224, bs = rows * 224) and word-row (ld = B * 208, bs = 208):
    fp16 log2-probabilities; 196 regions are 24 whole 8-region stores and one that ends an image after four (the split store); D = 160
    is five sub-steps of 32 (D % 64 != 0).  Seen: lse 0.030 .. 0.051, lp 0.92 .. 0.98."""
    c = ScoreCase(B, HW, T, D, ntt, class_lens(ntt, T, n or n_caps(HW, ntt), HW == 196), seed=3000 * HW + 10 * B + ntt + n, log2=True)
    w = Worst(f"scores512_kernel<{ntt},true> {form} {B}x{HW} D={D} n={c.n}")
    lp, lse = run_transposed(ops, c, form)
    judge_scores(w, c, c.reference(), lp, lse)
    w.report()


@pytest.mark.parametrize("kind", ["128row", "512", "image", "word"])
def test_scores_clamp_to_logp_min(ops, kind):
    """A LIVE word whose log-probability lies below the fp16 range: eight ctx dimensions of 16 against +-256 in two words of one caption put
    word 1 65536 below word 0 in every region row, so S - lse converts to -inf unless it is clamped to LOGP_MIN (fmaxf before the
    conversion in the untransposed kernels, a packed max behind it in the transposed one).  The reference clamps; the bits must be LOGP_MIN.
    Seen: lse 0.17, lp 0.99 (the scores reach 3e4 here: fp32 spacing 2^-9, and S of word 0 is a sum of like-signed products)."""
    B, HW, T, D, ntt = 6, 196, 77, 128, 2
    c = ScoreCase(B, HW, T, D, ntt, class_lens(ntt, T, n_caps(HW, ntt), False), seed=77, log2=kind in ("image", "word"))
    c.ctx[:, :8] = 16.0
    victim = int(c.members[1])                                # the class's longest caption
    c.words[victim, 0, :8], c.words[victim, 1, :8] = 256.0, -256.0
    r = c.reference()
    assert bool((r["lp"][:, :, 1, 1] == LOGP_MIN).all()) and bool(r["live"][:, :, 1, 1].all())
    w = Worst(f"clamp {kind}")
    if kind in ("128row", "512"):
        with scores512(ops, kind == "512"):
            lp, lse = run_untransposed(ops, c)
    else:
        lp, lse = run_transposed(ops, c, kind)
    assert bool((lp[:, :, 1, 1] == LOGP_MIN_BITS).all()), "a live word below the fp16 range is not clamped to LOGP_MIN"
    judge_scores(w, c, r, lp, lse)
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. the pair kernels on synthesised tiles
# ------------------------------------------------------------------------------------------------------------------------------
def pair_lens(ntt, T):
    """the class reaching beyond T (or its upper end), its lower end, one between, a caption shorter than the class, an empty one"""
    lo, hi = 16 * (ntt - 1) + 1, min(16 * ntt, T)
    return [hi if hi < T else T + 9, lo, (lo + hi) // 2, 5 if ntt == 3 else (1 if ntt > 1 else 5), 0]


class PairCase:
    """Synthesised inputs of one pair launch, float64 on the CPU in the logical shapes of local_tiled_reference.py: lp = fp16 of a float64
    log-softmax (log2: in the log2 domain) with LOGP_MIN on the masked words - caption 0 with a score spread of 12 (most probabilities
    below exp(-20)), caption 1 near-uniform (spread 0.01), the others spread 2, a one-word caption holding lp = 0; lse arbitrary fp32 of a
    few units; Gm = bf16 of c c^T for random bf16 region vectors with a common offset (so n2 stays well away from 0: den < eps is out of
    scope); wn positive fp32; gsim fp32."""

    def __init__(self, B, HW, T, ntt, lens, seed, uniform=False, log2=False, extra=2, Gm=None):
        g = torch.Generator().manual_seed(seed)
        self.B, self.HW, self.T, self.ntt, self.TP, self.n, self.uniform, self.log2 = B, HW, T, ntt, 16 * ntt, len(lens), uniform, log2
        n, TP = self.n, self.TP
        self.HWP = (HW + 15) // 16 * 16
        self.Bc = Bc = n + (0 if uniform else extra)
        self.members = torch.arange(Bc) if uniform else torch.randperm(Bc, generator=g)[:n]
        all_lens = torch.randint(1, T + 1, (Bc,), generator=g)
        all_lens[self.members] = torch.tensor(lens)
        self.all_lens = all_lens
        self.caps = clamp_caps(lens, T, TP)
        live = live_words(self.caps, TP)
        spread = torch.tensor(([12.0, 0.01] + [2.0] * n)[:n], dtype=F64)
        s = spread[None, None, :, None] * torch.randn(B, HW, n, TP, generator=g, dtype=F64)
        lpn = torch.log_softmax(s.masked_fill(~live[None, None], -math.inf), dim=-1)
        if log2:
            lpn = lpn / LN2
        self.lp16 = torch.where(live[None, None], lpn, torch.full_like(lpn, LOGP_MIN)).to(F16)
        self.lp_nat = self.lp16.to(F64) * (LN2 if log2 else 1.0)
        self.lse = (2.0 * torch.randn(B, HW, n, generator=g)).float().to(F64)
        if Gm is None:
            Gm = make_gram(B, HW, g)
        self.Gm = Gm
        self.wn_all = (0.5 + torch.rand(Bc, T, generator=g)).float()
        w = self.wn_all[self.members]
        self.wn = (F.pad(w, (0, TP - T), value=1.0) if TP > T else w[:, :TP]).to(F64)
        self.gs_all = (0.3 * torch.randn(B, Bc, generator=g)).float()
        self.live = live[None, None].expand(B, HW, n, TP)


def make_gram(B, HW, g):
    c = (0.3 * torch.randn(B, HW, 32, generator=g) + 1.5).to(BF).float()
    return torch.bmm(c, c.transpose(1, 2)).to(BF).to(F64)


def pair_bars(f, bw, lp_nat, HW, K, NTT, ea1, caps, log2_S, summed=False):
    """First-order error bars of a pair kernel's outputs, f / bw = the reference evaluated on the kernel's own bf16 A.  Counted from
    local_pair2_kernel (loss.hip phases 1-3) and the forward launch of local_pair3_kernel (pair3.hip), which compute the same chain:
      a1 = exp2(log2 e * lp): ea1 = (2 |lp| + 2) U relative (pair3: lp is in the log2 domain already, 2 U)
      x = exp2(c1 a1): ex = temp1 a1 (ea1 + 2 U) + 2 U;  column sum of HW terms, 1 / sum and two products: eA = ex + max_hw ex + (HW + 6) U
      A (bf16): UBF |A| + eA |A|
      num = sum_hw a (lp + lse): (max_hw eA + (HW + 4) U) sum|A S|  (pair3: S = fma(lp, ln 2, lse) adds U sum A |lp ln 2|)
      y = Gm . A over K = the padded region count: (32 + K / 32) U sum|Gm A|;  n2 = sum_hw a y: (32 + K / 32 + HW + 2) U sum|A Gm A|
      cos = num / (|w| sqrt n2): E_num / den + |cos| (E_n2 / (2 n2) + 3 U);  e = __expf(temp2 cos): e (4 U + 3 U |temp2 cos| + temp2 E_cos)
      s = sum_t e in word order: sum E_e + cap U s;  sim = __logf(s): 4 U (|sim| + 1) + E_s / s
      dcos = gsim temp2 e / s: relative E_e / e + E_s / s + 3 U;  dn = dcos / den: + E_n2 / (2 n2) + 4 U;  d2 = -dcos cos / n2
      cA = dn num + d2 n2, dA = dn S + d2 y, da1 = temp1 a (dA - cA), rd = sum_t a1 da1 (NTT in-lane terms, four shuffle adds),
      dS = dn a + a1 (da1 - rd), U = d2 a: the product rule on each, one U per operation on the magnitudes of its operands.
    summed (local_pair_kernel): num is summed with the rounded a (no eA), and cA is not the closed form but the fp32 sum over the regions of
    a (dn S + d2 y): (HW + 4) U (|dn| sum|A S| + |d2| sum|A Gm A|) more.
    The differences dA - cA and da1 - rd cancel, so these bars are absolute in the summed magnitudes; dS and U add UBF |ref| for the store."""
    live = f["live"]                                                                             # [1, n, TP]
    a1, A, Ab, S, y = f["a1"], f["A"], f["Ab"], f["S"], f["y"]
    ex = T1 * a1 * (ea1 + 2 * U) + 2 * U
    eA = ex + ex.amax(1, keepdim=True) + (HW + 6) * U
    E_num = ((0.0 if summed else eA.amax(1)) + (HW + 4) * U) * f["numabs"] + (U * (A * lp_nat.abs()).sum(1) if log2_S else 0.0)
    E_y = (32 + K / 32) * U * f["yabs"]
    E_n2 = (32 + K / 32 + HW + 2) * U * f["n2abs"]
    one = torch.ones_like(f["n2"])
    n2 = torch.where(live, f["n2"], one).expand_as(f["n2"])
    den = torch.where(live, f["den"], one)
    cos, e, s = f["cos"], f["e"], f["sume"]
    E_cos = torch.where(live, E_num / den + cos.abs() * (E_n2 / (2 * n2) + 3 * U), 0 * one)
    E_e = e * (4 * U + 3 * U * (T2 * cos).abs() + T2 * E_cos) + 2.0 ** -126            # + one flush of a denormal result
    capn = torch.tensor(caps, dtype=F64)[None]
    E_s = E_e.sum(-1) + capn * U * s
    E_sim = 4 * U * (f["sim"].abs() + 1) + E_s / s
    r_dcos = torch.where(live, E_e / torch.where(live, e, one), 0 * one) + (E_s / s)[..., None] + 3 * U
    dn, d2, dcos, ca, dA, da1, rd = bw["dn"], bw["d2"], bw["dcos"], bw["ca"], bw["dA"], bw["da1"], bw["rd"]
    E_dn = dn.abs() * (r_dcos + E_n2 / (2 * n2) + 4 * U)
    E_d2 = d2.abs() * (r_dcos + E_n2 / n2 + 3 * U) + dcos.abs() / n2 * E_cos
    E_ca = (E_dn * f["num"].abs() + dn.abs() * E_num + E_d2 * f["n2"].abs() + d2.abs() * E_n2
            + 2 * U * ((dn * f["num"]).abs() + (d2 * f["n2"]).abs()))
    if summed:
        E_ca = E_ca + (HW + 4) * U * (dn.abs() * f["numabs"] + d2.abs() * f["n2abs"])
    b4 = lambda v: v[:, None]
    E_dA = (b4(E_dn) * S.abs() + b4(E_d2) * y.abs() + b4(d2.abs()) * E_y + 2 * U * ((b4(dn) * S).abs() + (b4(d2) * y).abs()) + U * dA.abs())
    E_da1 = T1 * Ab * (E_dA + b4(E_ca) + U * (dA.abs() + b4(ca.abs()))) + 2 * U * da1.abs()
    m = a1 * da1.abs()
    E_rd = (a1 * (E_da1 + ea1 * da1.abs()) + U * m).sum(-1, keepdim=True) + (NTT + 5) * U * m.sum(-1, keepdim=True)
    E_dS = (b4(E_dn) * Ab + U * (b4(dn) * Ab).abs() + a1 * (E_da1 + E_rd + U * (da1.abs() + rd.abs()))
            + (ea1 + U) * (a1 * (da1 - rd)).abs() + U * bw["dS"].abs())
    return dict(A=eA * A, num=E_num, n2=E_n2, sim=E_sim, dS=E_dS, U=b4(E_d2) * Ab + U * bw["U"].abs())


def run_pair2(ops, c, gs_given, w):
    """sim-only launch (the input tile stays bit-identical), then the full launch; A, sim, dS, U (and att) judged per element"""
    B, HW, HWP, n, TP, Bc, T = c.B, c.HW, c.HWP, c.n, c.TP, c.Bc, c.T
    cb = 0 if c.uniform else 32
    ldp = Bc * TP if c.uniform else cb + n * TP + 16
    GW = (HWP // 16 + 1) // 2 * 32
    cols = slice(cb, cb + n * TP)
    tbuf, tile = guarded((B, HWP, ldp), BF)
    blk = torch.full((B, HWP, n, TP), NAN16, dtype=torch.int16)
    blk[:, :HW] = c.lp16.view(torch.int16)
    ibits(tile)[:, :, cols] = blk.reshape(B, HWP, n * TP).to(DEV)
    lse = torch.full((B, Bc, HWP), math.nan, device=DEV)
    lse[:, c.members.to(DEV), :HW] = c.lse.permute(0, 2, 1).float().to(DEV)
    gm = gram_device(c.Gm, HWP, GW)
    wn, cap, mem = c.wn_all.to(DEV), c.all_lens.to(I32).to(DEV), c.members.to(I32).to(DEV)
    gs = c.gs_all.to(DEV) if gs_given else None

    def launch(sim, dS, Uo, att):
        if c.uniform:
            ops.call("local_pair2", tile, lse, gm, wn, cap, gs, sim, dS, Uo, att, B, Bc, HW, T, T1, T2, EPS)
        else:
            ops.call("local_pair2_ragged", tile, lse, gm, wn, cap, gs, sim, dS, Uo, B, Bc, HW, T, T1, T2, EPS, mem, n, c.ntt, cb, ldp)
        torch.cuda.synchronize()

    before = ibits(tile).clone()
    s0buf, sim0 = guarded((B, Bc), F32)
    a0buf, att0 = guarded((Bc, T, HW), F32) if c.uniform else (None, None)
    launch(sim0, None, None, att0)
    assert torch.equal(ibits(tile), before), "the sim-only launch wrote into its input tile"
    sbuf, sim = guarded((B, Bc), F32)
    dbuf, dS = guarded((B, HWP, ldp), BF)
    ubuf, Uo = guarded((B, HWP, ldp), BF)
    abuf, att = guarded((Bc, T, HW), F32) if c.uniform else (None, None)
    launch(sim, dS, Uo, att)
    assert torch.equal(ibits(sim0), ibits(sim)) and tail_ok(s0buf, sim.numel()), "sim of the sim-only launch differs"
    wcol = torch.zeros(B, HWP, ldp, dtype=torch.bool, device=DEV)
    wcol[:, :, cols] = True
    wsim = torch.zeros(B, Bc, dtype=torch.bool, device=DEV)
    wsim[:, c.members.to(DEV)] = True
    for name, buf, t in (("A", tbuf, tile), ("dS", dbuf, dS), ("U", ubuf, Uo)):
        assert_written(t, wcol, name)
        assert tail_ok(buf, t.numel()), name
    assert_written(sim, wsim, "sim")
    assert tail_ok(sbuf, sim.numel())
    logical = lambda t: t[:, :, cols].reshape(B, HWP, n, TP).cpu().to(F64)
    Agot, dSgot, Ugot = logical(tile), logical(dS), logical(Uo)
    dead = torch.ones(B, HWP, n, TP, dtype=torch.bool)
    dead[:, :HW] = ~c.live
    for name, v in (("A", Agot), ("dS", dSgot), ("U", Ugot)):
        assert bool((v[dead] == 0).all()), name + ": not an exact zero on a masked word, a padded region row or a tile beyond the caption"
    f0 = ref_pair_fwd(c.lp_nat, c.lse, c.Gm, c.wn, c.caps, T1, T2, EPS)
    f = ref_pair_fwd(c.lp_nat, c.lse, c.Gm, c.wn, c.caps, T1, T2, EPS, A_stored=Agot[:, :HW])
    assert float(f["den"][f["live"].expand_as(f["den"])].min()) > 1e-3
    gsel = c.gs_all[:, c.members].to(F64) if gs_given else None
    bw = ref_pair_bwd(f, c.wn, gsel, T1, T2, EPS)
    ea1 = (2 * c.lp_nat.abs() + 2) * U * c.live
    bars = pair_bars(f, bw, c.lp_nat, HW, GW, c.ntt, ea1, c.caps, False)
    w("A", Agot[:, :HW], f0["A"], UBF, pair_bars(f0, ref_pair_bwd(f0, c.wn, gsel, T1, T2, EPS), c.lp_nat, HW, GW, c.ntt, ea1, c.caps, False)["A"])
    w("sim", sim.cpu()[:, c.members], f["sim"], 0.0, bars["sim"])
    w("dS", dSgot[:, :HW], bw["dS"], UBF, bars["dS"])
    w("U", Ugot[:, :HW], bw["U"], UBF, bars["U"])
    if c.uniform:
        k = min(B, Bc)
        watt = torch.zeros(Bc, T, HW, dtype=torch.bool, device=DEV)
        watt[:k] = True
        assert_written(att, watt, "att")
        assert tail_ok(abuf, att.numel()) and torch.equal(ibits(att0), ibits(att))
        for i in range(k):                                    # the attention map of the matching pair IS the kernel's bf16 A (judged above)
            assert torch.equal(att[i].cpu().to(F64), Agot[i, :HW, i, :T].t().contiguous()), "att"


PAIR2_RAGGED = [(64, 16, 1)] + [(196, 77, ntt) for ntt in range(1, 6)] + [(256, 77, ntt) for ntt in range(1, 6)]


@pytest.mark.parametrize("gs_given", [True, False])
@pytest.mark.parametrize("HW,T,ntt", PAIR2_RAGGED)
def test_pair2_ragged(ops, HW, T, ntt, gs_given):
    """local_pair2_kernel<4,1>, <13,1..5>, <16,1..5> through local_pair2_ragged, B = 2 images against five captions of the class (out of
    seven, permuted list, col_base 32), with gsim and with gsim = None (the kernel uses 1).  The empty caption counts as its first word.
    Seen: A 0.97 .. 0.99, sim 0.0019 .. 0.0087, dS 0.92 .. 0.97, U 0.91 .. 0.96."""
    c = PairCase(2, HW, T, ntt, pair_lens(ntt, T), seed=100 * HW + ntt)
    w = Worst(f"local_pair2_kernel<{c.HWP // 16},{ntt}> gsim={'given' if gs_given else 'None'}")
    run_pair2(ops, c, gs_given, w)
    w.report()


@pytest.mark.parametrize("gs_given", [True, False])
@pytest.mark.parametrize("HW,T", [(64, 16), (196, 25), (196, 77)])
def test_pair2_uniform(ops, HW, T, gs_given):
    """local_pair2_kernel<4,1>, <13,2>, <13,5> through local_pair2: cap_list null, every caption Tp columns wide, att of the matching pairs
    (b == i, i < 2) written and equal to the kernel's A, att of the other captions untouched.  Seen: A 0.98 .. 0.99, sim 0.0025 .. 0.014, dS 0.93 .. 0.96, U 0.93 .. 0.95."""
    ntt = (T + 15) // 16
    c = PairCase(2, HW, T, ntt, [T + 9, 1, T // 2, min(5, T), 0], seed=200 * HW + T, uniform=True)
    w = Worst(f"local_pair2_kernel<{c.HWP // 16},{ntt}> uniform gsim={'given' if gs_given else 'None'}")
    run_pair2(ops, c, gs_given, w)
    w.report()


@pytest.mark.parametrize("gs_given", [True, False])
@pytest.mark.parametrize("HW,T", [(64, 16), (196, 25), (196, 77)])
def test_local_pair_precomputed(ops, HW, T, gs_given):
    """local_pair_kernel<4,1 / 13,2 / 13,5, ., PRECOMP> as src/losses.py runs it on the tiles of local_scores: the forward launch (sim, att of
    the matching pairs; the input tile stays bit-identical) and the backward launch (dS, A in place over the tile, U).  The kernel differs
    from local_pair2 in three counted ways: a1 = __expf((lp + lse) - lse), so ea1 = (|S| + 3 |lp| + 2) U; num is summed with the ROUNDED
    a; cA is the fp32 sum over the regions (pair_bars(summed=True)).  Both launches run the same arithmetic up to sim: their sim and the
    att / A of the matching pairs are bit-identical, so the forward launch is judged through the backward launch's A.
    An empty caption counts as its first word here too (the kernel took cap = 0 before: A = 0 everywhere and sim = log 0).
    Seen: A 0.98 .. 0.99, sim 0.004 .. 0.012, dS 0.93 .. 0.98, U 0.94 .. 0.98."""
    ntt = (T + 15) // 16
    c = PairCase(2, HW, T, ntt, [T + 9, 1, T // 2, min(5, T), 0], seed=300 * HW + T, uniform=True)
    B, HWP, n, TP, Bc = c.B, c.HWP, c.n, c.TP, c.Bc
    ldp = Bc * TP
    GW = (HWP // 16 + 1) // 2 * 32
    tbuf, tile = guarded((B, HWP, ldp), BF)
    blk = torch.full((B, HWP, n, TP), NAN16, dtype=torch.int16)
    blk[:, :HW] = c.lp16.view(torch.int16)
    ibits(tile)[:] = blk.reshape(B, HWP, ldp).to(DEV)
    lse = torch.full((B, Bc, HWP), math.nan, device=DEV)
    lse[:, :, :HW] = c.lse.permute(0, 2, 1).float().to(DEV)
    gm, wn, cap = gram_device(c.Gm, HWP, GW), c.wn_all.to(DEV), c.all_lens.to(I32).to(DEV)
    gs = c.gs_all.to(DEV) if gs_given else None
    before = ibits(tile).clone()
    s0buf, sim0 = guarded((B, Bc), F32)
    abuf, att = guarded((Bc, T, HW), F32)
    ops.call("local_pair", None, None, gm, wn, cap, None, sim0, None, None, None, att, tile, lse, B, Bc, HW, T, 128, T1, T2, EPS, 0)
    torch.cuda.synchronize()
    assert torch.equal(ibits(tile), before), "the forward launch wrote into its input tile"
    sbuf, sim = guarded((B, Bc), F32)
    dbuf, dS = guarded((B, HWP, ldp), BF)
    ubuf, Uo = guarded((B, HWP, ldp), BF)
    ops.call("local_pair", None, None, gm, wn, cap, gs, sim, dS, tile, Uo, None, tile, lse, B, Bc, HW, T, 128, T1, T2, EPS, 1)
    torch.cuda.synchronize()
    full = torch.ones(B, HWP, ldp, dtype=torch.bool, device=DEV)
    for name, buf, t in (("A", tbuf, tile), ("dS", dbuf, dS), ("U", ubuf, Uo)):
        assert_written(t, full, name)
        assert tail_ok(buf, t.numel()), name
    for name, buf, t in (("sim forward", s0buf, sim0), ("sim backward", sbuf, sim)):
        assert_written(t, torch.ones(B, Bc, dtype=torch.bool, device=DEV), name)
        assert tail_ok(buf, t.numel()), name
    assert torch.equal(ibits(sim0), ibits(sim)), "sim of the forward and of the backward launch differ"
    logical = lambda t: t.reshape(B, HWP, n, TP).cpu().to(F64)
    Agot, dSgot, Ugot = logical(tile), logical(dS), logical(Uo)
    dead = torch.ones(B, HWP, n, TP, dtype=torch.bool)
    dead[:, :HW] = ~c.live
    for name, v in (("A", Agot), ("dS", dSgot), ("U", Ugot)):
        assert bool((v[dead] == 0).all()), name + ": not an exact zero on a masked word or a padded region row"
    watt = torch.zeros(Bc, T, HW, dtype=torch.bool, device=DEV)
    watt[:B] = True
    assert_written(att, watt, "att")
    assert tail_ok(abuf, att.numel())
    for i in range(B):
        assert torch.equal(att[i].cpu().to(F64), Agot[i, :HW, i, :T].t().contiguous()), "att"
    kw = dict(num_stored=True)
    f0 = ref_pair_fwd(c.lp_nat, c.lse, c.Gm, c.wn, c.caps, T1, T2, EPS, **kw)
    f = ref_pair_fwd(c.lp_nat, c.lse, c.Gm, c.wn, c.caps, T1, T2, EPS, A_stored=Agot[:, :HW], **kw)
    assert float(f["den"][f["live"].expand_as(f["den"])].min()) > 1e-3
    gsel = c.gs_all.to(F64) if gs_given else None
    bw = ref_pair_bwd(f, c.wn, gsel, T1, T2, EPS)
    ea1 = (f["S"].abs() + 3 * c.lp_nat.abs() + 2) * U * c.live
    bars = pair_bars(f, bw, c.lp_nat, HW, GW, ntt, ea1, c.caps, False, summed=True)
    w = Worst(f"local_pair_kernel<{HWP // 16},{ntt},PRECOMP> gsim={'given' if gs_given else 'None'}")
    w("A", Agot[:, :HW], f0["A"], UBF, pair_bars(f0, ref_pair_bwd(f0, c.wn, gsel, T1, T2, EPS), c.lp_nat, HW, GW, ntt, ea1, c.caps, False, summed=True)["A"])
    w("sim", sim.cpu(), f["sim"], 0.0, bars["sim"])
    w("dS", dSgot[:, :HW], bw["dS"], UBF, bars["dS"])
    w("U", Ugot[:, :HW], bw["U"], UBF, bars["U"])
    w.report()


def run_pair3(ops, B, HW, T, caps, form, seed):
    """the forward launch of every class of `caps`, with one caption chunk per image and with the automatic spread (bit-identical); returns
    the judged ratios"""
    from medmoe_amd.engine import ragged_layout
    Bc = len(caps)
    HWP, GR = (HW + 15) // 16 * 16, (HW + 31) // 32 * 32
    pw = 64 if HW == 64 else (224 if form == "image" else 208)
    perm, _, _, _, classes, Kc, Kp = ragged_layout(np.array(caps), T, (T + 15) // 16 * 16)
    ld, bs = (pw, Kp * pw) if form == "image" else (B * pw, pw)
    g = torch.Generator().manual_seed(seed)
    Gm = make_gram(B, HW, g)
    cases = [(ntt, start, n_c, cbase, PairCase(B, HW, T, ntt, [caps[i] for i in perm[start:start + n_c]], seed + ntt, uniform=True, log2=True, Gm=Gm))
             for ntt, start, n_c, cbase in classes]
    lbuf, lp = guarded((B * Kp * pw,), BF)                     # the sentinel is a NaN as fp16 too: regions >= HW and the rows Kc.. stay poisoned
    view = (lambda t: t.view(B, Kp, pw)) if form == "image" else (lambda t: t.view(Kp, B, pw).permute(1, 0, 2))
    lse = torch.full((B, Bc, HWP), math.nan, device=DEV)
    wn = torch.empty(Bc, T, device=DEV)
    for ntt, start, n_c, cbase, c in cases:
        mem = torch.from_numpy(perm[start:start + n_c]).to(DEV)
        tgt = view(ibits(lp))                                  # shares lp's memory
        tgt[:, cbase:cbase + n_c * c.TP, :HW] = c.lp16.view(torch.int16).permute(0, 2, 3, 1).reshape(B, n_c * c.TP, HW).to(DEV)
        lse[:, mem, :HW] = c.lse.permute(0, 2, 1).float().to(DEV)
        wn[mem] = c.wn_all.to(DEV)
    gm = torch.zeros(B, GR, GR, dtype=BF, device=DEV)
    gm[:, :HW, :HW] = Gm.to(BF).to(DEV)
    capd = torch.tensor(caps, dtype=I32, device=DEV)
    d_perm = torch.from_numpy(perm.astype(np.int32)).to(DEV)
    lp_before = ibits(lp).clone()
    runs = []
    try:
        for chunks in (1, 0):
            ops.local_pair3_chunks(chunks)
            out = dict(A=guarded((B * Kp * pw,), BF), stats=guarded((B, Kp, 2), F32), sim=guarded((B, Bc), F32), att=guarded((Bc, T, HW), F32))
            for ntt, start, n_c, cbase, c in cases:
                ops.call("local_pair3", lp, None, out["A"][1], None, lse, gm, wn, capd, None, out["sim"][1], out["att"][1], out["stats"][1], Kp,
                         B, Bc, HW, T, T1, T2, EPS, d_perm[start:start + n_c], n_c, ntt, cbase, ld, bs, pw, None)
            torch.cuda.synchronize()
            runs.append(out)
    finally:
        ops.local_pair3_chunks(0)
    assert torch.equal(ibits(lp), lp_before), "the forward launch wrote into its input"
    for k in runs[0]:
        assert torch.equal(ibits(runs[0][k][0]), ibits(runs[1][k][0])), k + ": one chunk and the automatic spread differ"
    out = runs[0]
    A, stats, sim, att = view(out["A"][1]), out["stats"][1], out["sim"][1], out["att"][1]
    wa = torch.zeros(B, Kp, pw, dtype=torch.bool, device=DEV)
    wa[:, :Kc] = True
    ws = torch.zeros(B, Kp, 2, dtype=torch.bool, device=DEV)
    ws[:, :Kc] = True
    watt = torch.zeros(Bc, T, HW, dtype=torch.bool, device=DEV)
    for ntt, start, n_c, cbase, c in cases:
        for i in perm[start:start + n_c]:
            if i < B:
                watt[i, :min(T, c.TP)] = True                  # a class writes the word rows of its own 16 * ntt columns
    assert_written(A.contiguous(), wa, "A")
    assert_written(stats, ws, "stats")
    assert_written(sim, torch.ones(B, Bc, dtype=torch.bool, device=DEV), "sim")
    assert_written(att, watt, "att")
    for k, (buf, t) in out.items():
        assert tail_ok(buf, t.numel()), k
    assert bool((A[:, :Kc, HW:].float() == 0).all()), "the region columns HW .. pw of A are not zeros"
    for ntt, start, n_c, cbase, c in cases:
        w = Worst(f"local_pair3_kernel<{HW},{ntt},false> {form}")
        mem = torch.from_numpy(perm[start:start + n_c])
        rows = slice(cbase, cbase + n_c * c.TP)
        Agot = A[:, rows, :HW].reshape(B, n_c, c.TP, HW).permute(0, 3, 1, 2).cpu().to(F64)
        st = stats[:, rows].reshape(B, n_c, c.TP, 2).cpu().to(F64)
        deadw = ~live_words(c.caps, c.TP)
        assert bool((Agot[~c.live] == 0).all()) and bool((st[:, deadw] == 0).all()), "words beyond cap: A and stats must be exact zeros"
        f0 = ref_pair_fwd(c.lp_nat, c.lse, c.Gm, c.wn, c.caps, T1, T2, EPS)
        f = ref_pair_fwd(c.lp_nat, c.lse, c.Gm, c.wn, c.caps, T1, T2, EPS, A_stored=Agot)
        assert float(f["den"][f["live"].expand_as(f["den"])].min()) > 1e-3
        ea1 = 2 * U * c.live
        bars0 = pair_bars(f0, ref_pair_bwd(f0, c.wn, None, T1, T2, EPS), c.lp_nat, HW, GR, ntt, ea1, c.caps, True)
        bars = pair_bars(f, ref_pair_bwd(f, c.wn, None, T1, T2, EPS), c.lp_nat, HW, GR, ntt, ea1, c.caps, True)
        w("A", Agot, f0["A"], UBF, bars0["A"])
        w("num", st[..., 0], f["num"], 0.0, bars["num"])
        w("n2", st[..., 1], f["n2"], 0.0, bars["n2"])
        w("sim", sim.cpu()[:, mem], f["sim"], 0.0, bars["sim"])
        for j, i in enumerate(mem.tolist()):
            if i < B:
                tw = min(T, c.TP)
                assert torch.equal(att[i, :tw].cpu().to(F64), Agot[i, :, j, :tw].t().contiguous()), "att"
        w.report()


@pytest.mark.parametrize("form", ["image", "word"])
def test_pair3_forward_196(ops, form):
    """local_pair3_kernel<196, 1..5, false>: the caption list of test_pair3_onepass_gpu.py (49 / 25 / 16 / 13 / 10 captions: four epochs per
    class at one chunk, both mailbox parities twice) plus an empty caption, image-major (pw 224) and word-row (pw 208).
    Seen: A 0.99, num 0.009 .. 0.017, n2 0.015 .. 0.018, sim 0.0024 .. 0.0061."""
    run_pair3(ops, 2, 196, 77, caps_all_classes(77) + [0], form, seed=31)


@pytest.mark.parametrize("form", ["image", "word"])
def test_pair3_forward_64(ops, form):
    """local_pair3_kernel<64, 1, false>: forty captions of the onepass test plus an empty one.  Seen: A 0.99, num 0.023, n2 0.030, sim 0.014."""
    run_pair3(ops, 2, 64, 16, [16, 3, 9, 1, 12, 16, 7, 5] * 5 + [0], form, seed=32)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the Gram layout's producer and the glue kernels
# ------------------------------------------------------------------------------------------------------------------------------
def gram_device(Gm, HWP, GW):
    """bf16 Gm [B, HW, HW] -> what local_pair2 reads: [B, HWP, GW], region k of a row at column lpos(k), zero outside [HW][HW]"""
    B, HW = Gm.shape[:2]
    out = torch.zeros(B, HWP, GW, dtype=BF, device=DEV)
    out[:, :HW, torch.tensor([lpos(k) for k in range(HW)], device=DEV)] = Gm.to(BF).to(DEV)
    return out


@pytest.mark.parametrize("P,T", [(64, 16), (196, 77), (256, 77)])
def test_gram_layout_is_the_producers(ops, P, T):
    """The layout run_pair2 synthesises is the one the engine's producer writes: gemm_nt(col_perm = True) with RaggedLocalLoss's own
    tables, on integer-valued vectors (every Gram entry is an integer of at most 128: exact in bf16, so the comparison is torch.equal)."""
    B, D = 2, 128
    HWp, _, GW = ops.local_geometry(P, T)
    assert GW == (HWp // 16 + 1) // 2 * 32
    g = torch.Generator().manual_seed(P)
    ctx = torch.randint(-1, 2, (B * P, D), generator=g).to(BF).to(DEV)
    tl = [[b, m, (b + 1) * P, 0] for b in range(B) for m in range(b * P, (b + 1) * P, 128)]
    tiles, count = torch.tensor(tl, device=DEV, dtype=I32).reshape(-1, 4), torch.tensor([len(tl)], device=DEV, dtype=I32)
    ar = torch.arange(B * P, device=DEV)
    gmp = torch.zeros(B * HWp, GW, device=DEV, dtype=BF)
    ops.gemm_nt(ctx, ctx, gmp, c_rowmap=(ar // P * HWp + ar % P).to(I32), tiles=tiles, tile_count=count, max_tiles=len(tl), stride_b=P * D,
                M=B * P, N=P, col_perm=True)
    torch.cuda.synchronize()
    c = ctx.view(B, P, D).float()
    assert torch.equal(gmp.view(B, HWp, GW), gram_device(torch.bmm(c, c.transpose(1, 2)), HWp, GW))


def test_scale_blocks(ops):
    """scale_blocks and scale_blocks_ragged: X[(b, hw)][(i, t)] *= g[b][i] on two matrices, one fp32 product and one bf16 rounding per
    element - bit-equal to torch.  1664 rows x 640 chunks of 8 columns = 1 064 960 chunks for a grid of 4096 x 256 threads: the grid-stride
    loop runs twice.  Ragged: the chunks whose cap_of_chunk is -1 (gaps between captions, the padding at the end) keep their bits."""
    B, Bc, HWp, Tp = 8, 64, 208, 80
    ld = Bc * Tp
    g = torch.Generator().manual_seed(5)
    X = [(torch.randn(B * HWp, ld, generator=g)).to(BF).to(DEV) for _ in range(2)]
    gs = torch.randn(B, Bc, generator=g).to(DEV)
    bufs = [guarded((B * HWp, ld), BF, init=x) for x in X]
    ops.call("scale_blocks", bufs[0][1], bufs[1][1], gs, B, Bc, HWp, Tp)
    torch.cuda.synchronize()
    for x, (buf, got) in zip(X, bufs):
        want = (x.float().view(B, HWp, Bc, Tp) * gs[:, None, :, None]).to(BF).view(B * HWp, ld)
        assert torch.equal(ibits(got), ibits(want)) and tail_ok(buf, got.numel())
    chunk, col, i = torch.full((ld // 8,), -1, dtype=torch.int64), 0, 0
    while col + 80 + 16 <= ld - 64:                            # captions of 16 .. 80 columns, a gap of 16 columns after every third
        wd = 16 * (1 + i % 5)
        chunk[col // 8:(col + wd) // 8] = i
        col += wd + (16 if i % 3 == 2 else 0)
        i += 1
    nc = i
    gs = torch.randn(B, nc, generator=g).to(DEV)
    bufs = [guarded((B * HWp, ld), BF, init=x) for x in X]
    ops.call("scale_blocks_ragged", bufs[0][1], bufs[1][1], gs, B, nc, HWp, chunk.to(I32).to(DEV), ld)
    torch.cuda.synchronize()
    capcol = chunk.repeat_interleave(8).to(DEV)                                                    # caption of every column
    f = torch.where(capcol >= 0, gs[:, capcol.clamp_min(0)], torch.ones((), device=DEV))          # [B, ld]
    for x, (buf, got) in zip(X, bufs):
        want = torch.where((capcol >= 0)[None, None], (x.float().view(B, HWp, ld) * f[:, None]).to(BF), x.view(B, HWp, ld)).view(B * HWp, ld)
        assert torch.equal(ibits(got), ibits(want)) and tail_ok(buf, got.numel())
        assert int((capcol < 0).sum()) >= 64


def wn_bar(D):
    """|w| = sqrtf(s), s an fp32 sum of D squares (each exact: a bf16 squared has 16 bits): words_prep_kernel adds ceil(D / 64) terms per
    lane, words_norm_kernel 4 ceil(D / 512) pairs (a product, a fused add, the add into s: 3 roundings), both six shuffle adds; the
    root halves the relative error of s and adds its own rounding.  One bar for both kernels: the two counts added."""
    return ((12 * math.ceil(D / 512) + math.ceil(D / 64) + 6) / 2 + 1) * U


@pytest.mark.parametrize("D", [128, 768])
def test_words_prep_uniform(ops, D):
    """words_prep: wn = |w| (fp32 bar of wn_bar) and wT[d][i * Tp + t] = words[i, t, d], exact zeros for T <= t < Tp - torch.equal.
    Seen: wn 0.06 .. 0.13."""
    Bc, T, Tp = 5, 77, 80
    g = torch.Generator().manual_seed(D)
    words = (0.5 * torch.randn(Bc, T, D, generator=g)).to(BF).to(DEV)
    nbuf, wn = guarded((Bc, T), F32)
    tbuf, wT = guarded((D, Bc, Tp), BF)
    ops.call("words_prep", words, wn, wT, Bc, T, Tp, D)
    torch.cuda.synchronize()
    want = torch.zeros(D, Bc, Tp, dtype=BF, device=DEV)
    want[:, :, :T] = words.permute(2, 0, 1)
    assert torch.equal(ibits(wT), ibits(want)) and tail_ok(tbuf, wT.numel()) and tail_ok(nbuf, wn.numel())
    w = Worst(f"words_prep D={D}")
    ref = torch.linalg.vector_norm(words.to(F64), dim=-1)
    w("wn", wn, ref, 0.0, wn_bar(D) * ref)
    w.report()


@pytest.mark.parametrize("D,with_wT", [(128, True), (768, True), (128, False), (768, False), (100, False)])
def test_words_prep_ragged(ops, D, with_wT):
    """words_prep_ragged: caption i at columns col_of_cap[i] .. + tp_of_cap[i] of rows ldw wide (words for t < T, zeros up to tp_of_cap[i]),
    every other column untouched; wT = None runs words_norm_kernel where D % 8 == 0 and the general kernel at D = 100.  Seen: wn 0.05 .. 0.14."""
    Bc, T, Tp = 7, 77, 80
    g = torch.Generator().manual_seed(D + 1)
    words = (0.5 * torch.randn(Bc, T, D, generator=g)).to(BF).to(DEV)
    tp = [16, 80, 32, 48, 80, 64, 16]
    col, c0 = [], 16
    for i in range(Bc):
        col.append(c0)
        c0 += tp[i] + (16 if i % 2 else 0)
    ldw = c0 + 24
    nbuf, wn = guarded((Bc, T), F32)
    tbuf, wT = guarded((D, ldw), BF) if with_wT else (None, None)
    ops.call("words_prep_ragged", words, wn, wT, Bc, T, Tp, D, torch.tensor(col, dtype=I32, device=DEV), torch.tensor(tp, dtype=I32, device=DEV), ldw)
    torch.cuda.synchronize()
    if with_wT:
        want = torch.full((D, ldw), SENT[BF], dtype=torch.int16, device=DEV).view(BF)
        for i in range(Bc):
            want[:, col[i]:col[i] + tp[i]] = 0
            k = min(tp[i], T)
            want[:, col[i]:col[i] + k] = words[i, :k].t()
        assert torch.equal(ibits(wT), ibits(want)) and tail_ok(tbuf, wT.numel())
    assert tail_ok(nbuf, wn.numel())
    w = Worst(f"words_prep_ragged D={D} wT={'yes' if with_wT else 'None'}")
    ref = torch.linalg.vector_norm(words.to(F64), dim=-1)
    w("wn", wn, ref, 0.0, wn_bar(D) * ref)
    w.report()
