"""Elementwise, exact and invariance tests of the attention kernels (attention.hip: resident and streaming forward, dQ and dK/dV
passes, the packed variable-length forward; swin.hip: window attention), each called through medmoe_amd.ops as the engine calls it.

Kernel build is forced, never guessed: option 11 (1 resident / 0 streaming) and option 15 (448 / 512 threads at 13 key tiles) are set by
`family()` and restored to their defaults (1, 0) in a `finally`.  Every output buffer (out, lse, dqkv, delta, window slabs) is
allocated by `guarded` with a sentinel tail and a sentinel-filled body: after each launch the tail must be untouched and no body
element may still hold the sentinel.

Which test reaches what (R5/R13/R17/R37 = resident build of 5/13/17/37 key tiles, R13 in its 448- and 512-thread forms; S = streaming;
u / m = the unmasked / masked template instance):

  build   shape class (N)                         mask kind                       tests
  R5  u/m 1 15 16 17 63 64 65 80                  none, prefix, holes             elementwise, onehot (80), uniform, masked_contents,
                                                                                  batch_head_independence (16 65)
  R5  u   packed lengths 1 16 17 79 80            -                               varlen_equals_resident
  R13 u/m 81 128 129 197 208 (448 and 512)        none, prefix, holes             elementwise, onehot (208), uniform, masked_contents,
                                                                                  batch_head_independence (197)
  R17 u/m 209 257 272                             none, prefix, holes, head-128   elementwise, onehot (272), uniform, masked_contents,
                                                                                  batch_head_independence (257)
  R37 u/m 273 577 592                             none, prefix, holes, head-128   elementwise, onehot (592), uniform, masked_contents,
                                                                                  batch_head_independence (577)
  S   u/m all of the above and 593 1025           none, prefix, holes, head-64    elementwise, onehot (80 .. 1025), uniform,
                                                                                  masked_contents, batch_head_independence
  window  (B, H, C, heads, shift) of test_swin_gpu + B = 1, shift mask on / off   window_elementwise, window_onehot, window_independence

Bars.  An element passes when |got - ref| <= c_r |ref| + (absolute part), as in test_glue_kernels_gpu.py (its `check` is used with the
absolute part as `terms` and c_a = 1).  The bf16 parts are one UBF = 2^-8 per bf16 rounding point of the kernels (output rounding:
c_r = UBF; probabilities rounded before P.V and P^T.dO; dS rounded before dS.K and dS^T.Q).  The fp32 parts are counted from the kernel
source, in units of U = 2^-24, in `fwd_bars` / `bwd_bars` / the window functions below; none was set from an observed error.
"""
import contextlib
import io
import math

import pytest
import torch

from test_glue_kernels_gpu import BF, DEV, F32, F64, SENT, U, UBF, _BITS, check, guarded, sentinel_ok, tail_ok

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
NS = [1, 15, 16, 17, 63, 64, 65, 80, 81, 128, 129, 197, 208, 209, 257, 272, 273, 577, 592, 593, 1025]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# kernel builds
# ------------------------------------------------------------------------------------------------------------------------------
def pick_nkt(N):
    """key tiles of the resident build that serves N keys (attention.hip pick_nkt)"""
    return 5 if N <= 80 else 13 if N <= 208 else 17 if N <= 272 else 37 if N <= 592 else 0


def families(N):
    """kernel families that serve N: streaming always, resident up to 592 keys, and the 448-thread build where 13 key tiles are used"""
    f = ["stream"]
    if N <= 592:
        f.append("res")
    if pick_nkt(N) == 13:
        f.append("res448")
    return f


@contextlib.contextmanager
def family(ops, fam):
    """force the kernel build: option 11 = resident / streaming, option 15 = threads of the 13-tile resident build; defaults restored"""
    try:
        ops.set_option(11, 0 if fam == "stream" else 1)
        ops.set_option(15, 448 if fam == "res448" else 512)
        yield
    finally:
        ops.set_option(11, 1)
        ops.set_option(15, 0)


def chain(fam, N):
    """(roundings behind the fp32 row sum l, roundings behind an fp32 P.V accumulator, keys an MFMA accumulation runs over)
    forward: keys come in blocks (streaming: 64 keys = 4 tiles; resident: chunks of 8 tiles).  Per block the lane's partial sum takes one
    add per tile (l2 += e0 + e1 on pairs) and lp = lp * alpha + l2[0] + l2[1] (3 roundings); two shuffle adds at the end.  An output
    accumulator takes one rounding per accumulated product at worst (16 keys per tile) and one for `o *= alpha` per block."""
    if fam == "stream":
        nb, tb = (N + 63) // 64, 4
    else:
        nb, tb = (pick_nkt(N) + 7) // 8, 8
    return nb * (tb + 3) + 2, nb * (tb * 16 + 1), nb * tb * 16


class Worst:
    """runs `check` quietly and keeps the worst ratio per output; report() prints one "[bar]" line per output"""

    def __init__(self, tag):
        self.tag, self.w = tag, {}

    def __call__(self, name, got, ref, c_r, abs_bar):
        with contextlib.redirect_stdout(io.StringIO()):
            r = check(f"{self.tag} {name}", got, ref, abs_bar, c_r, 1.0)
        self.w[name] = max(self.w.get(name, 0.0), r)

    def report(self):
        for k, v in self.w.items():
            print(f"[bar] {self.tag} {k}: worst |err|/bar = {v:.3g}")


def bits(t):
    return t.contiguous().view(_BITS[t.dtype])


def same_bits(a, b):
    return bool(torch.equal(bits(a), bits(b)))


def written(t):
    """no element still holds the sentinel the buffer was filled with"""
    return bool((bits(t) != SENT[t.dtype]).all().item())


def nonzero(t):
    """randn can return an exact zero, which the 2^-40 weights of the other keys would turn into a tiny non-zero: one-hot data avoids it"""
    return torch.where(t == 0, torch.ones_like(t), t)


def heads(t, B, N, H):
    """[B, N, H*64] -> float64 [B, H, N, 64]"""
    return t.to(F64).view(B, N, H, 64).permute(0, 2, 1, 3)


def split(qkv, B, N, H):
    q, k, v = qkv.to(F64).view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    return q, k, v


def run_fwd(ops, qkv, mask, B, N, H):
    D = H * 64
    ob, out = guarded((B, N, D), BF)
    lb, lse = guarded((B, H, N), F32)
    ops.attn_fwd(qkv, out, lse, mask, B, N, H)
    torch.cuda.synchronize()
    assert tail_ok(ob, out.numel()) and tail_ok(lb, lse.numel()), "forward wrote past the end of out / lse"
    assert written(out) and written(lse), "forward left part of out / lse unwritten"
    return out, lse


def run_bwd(ops, qkv, out, dout, lse, mask, B, N, H):
    gb, dqkv = guarded((B, N, 3 * H * 64), BF)
    db, delta = guarded((B, H, N), F32)
    ops.attn_bwd(qkv, out, dout, lse, mask, dqkv, delta, B, N, H)
    torch.cuda.synchronize()
    assert tail_ok(gb, dqkv.numel()) and tail_ok(db, delta.numel()), "backward wrote past the end of dqkv / delta"
    assert written(dqkv) and written(delta), "backward left part of dqkv / delta unwritten"
    return dqkv, delta


# ------------------------------------------------------------------------------------------------------------------------------
# float64 references and bars
# ------------------------------------------------------------------------------------------------------------------------------
def scores(qkv, mask, B, N, H):
    """float64 S = q k^T / 8 with masked keys at -inf, and A = sum_d |q_d k_d| / 8 (0 at masked keys): the magnitude of the terms behind
    a score, which bounds |S| and scales every fp32 error of the exponent's argument"""
    q, k, v = split(qkv, B, N, H)
    S = q @ k.transpose(-1, -2) * 0.125
    A = q.abs() @ k.abs().transpose(-1, -2) * 0.125
    if mask is not None:
        dead = ~mask.bool()[:, None, None, :]
        S = S.masked_fill(dead, -math.inf)
        A = A.masked_fill(dead, 0.0)
    return q, k, v, S, A


def e_p(A, N):
    """fp32 roundings behind one probability, relative, in U, per query row (A: [.., N, N]):
      64 A  the score: 64 products accumulated in fp32 by two MFMAs, each rounding relative to sum |q_d k_d|
       6 A  the exponent's argument in the exp2 domain: c2 = scale * log2(e) is a rounded product of a rounded constant (2 roundings on
            |S|), the fma / (multiply, add mask, subtract maximum) round 1 to 2 times on |S - m| <= 2 max|S|, and the backward's
            -lse * log2(e) rounds twice on |lse| <= max|S| + ln N (the ln N part is the next line); 6 covers the longest of the kernels
       3 ln N  the lse part above
       2    v_exp_f32 (one ulp)"""
    return 70.0 * A.amax(-1) + 3.0 * math.log(max(N, 2)) + 2.0


def fwd_ref(qkv, mask, B, N, H):
    q, k, v, S, A = scores(qkv, mask, B, N, H)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    return dict(out=P @ v, T=P @ v.abs(), lse=lse, E=e_p(A, N))


def fwd_bars(w, fam, r, out, lse, B, N, H):
    """out: c_r = UBF (output rounding); absolute part (UBF + c U) sum_k p_k |v_k| with UBF for the probabilities' bf16 rounding and
         c = 2 E_p (the probability and the row sum it is divided by) + n_l (row sum chain) + n_o (P.V accumulation) + 3 (1 / l, o * inv
         and the last rescale), see `chain` and `e_p`.
       lse (fp32, c_r = 0): U (E_p + n_l + 2 log2 N + 4 |lse|): the exponent arguments and the row sum chain move ln l by their relative
         error; v_log_f32 is one ulp of log2 l <= log2 N; m + log2 l and the product with the rounded constant ln 2 are three roundings
         on |lse| log2 e, counted as 4 |lse|."""
    n_l, n_o, _ = chain(fam, N)
    c = 2.0 * r["E"] + n_l + n_o + 3.0
    w("out", heads(out, B, N, H), r["out"], UBF, (UBF + U * c)[..., None] * r["T"])
    w("lse", lse, r["lse"], 0.0, U * (r["E"] + n_l + 2.0 * math.log2(max(N, 2)) + 4.0 * r["lse"].abs()))


def bwd_ref(qkv, out_in, lse_in, dout, mask, B, N, H):
    """float64 restatement on the kernel's own inputs (the bf16 out and fp32 lse handed to medmoe_attn_bwd)"""
    q, k, v, S, A = scores(qkv, mask, B, N, H)
    P = torch.exp(S - lse_in.to(F64)[..., None])
    o, do = heads(out_in, B, N, H), heads(dout, B, N, H)
    delta, Dabs = (do * o).sum(-1), (do * o).abs().sum(-1)
    dP = do @ v.transpose(-1, -2)
    G = do.abs() @ v.abs().transpose(-1, -2)
    dS = P * (dP - delta[..., None])
    return dict(q=q, k=k, do=do, P=P, dS=dS, dP=dP, G=G, delta=delta, Dabs=Dabs, E=e_p(A, N),
                dV=P.transpose(-1, -2) @ do, dQ=0.125 * dS @ k, dK=0.125 * dS.transpose(-1, -2) @ q)


def bwd_bars(w, fam, r, dqkv, delta, B, N, H):
    """delta (fp32, c_r = 0): 18 U sum |dO O|: 16 products per lane (exact: bf16 x bf16) added one by one, two shuffle adds.
       dV: c_r = UBF; (UBF + U (E_p(q) + n_k)) sum_q p_qk |dO_q|: probabilities rounded to bf16, their fp32 error, n_k = accumulation depth.
       dQ: c_r = UBF; scale (UBF sum_k |dS_qk| |K_k| + U sum_k (p_qk w_qk + n_k |dS_qk|) |K_k|), dK likewise over q with |Q_q|, where
         p w bounds the fp32 error of dS = p (dP - delta) before its bf16 rounding:
         w_qk = (E_p + 2) |dP - delta| (p's error; the subtraction and the product round once each) + 64 sum_d |dO_qd V_kd| (dP: 64
         products accumulated by two MFMAs) + 18 sum_d |dO_qd O_qd| (delta, above).  The scale 1/8 is a power of two: no rounding."""
    _, _, n_k = chain(fam, N)
    D = H * 64
    g = dqkv.view(B, N, 3, D)
    P, dS, E = r["P"], r["dS"], r["E"]
    w("delta", delta, r["delta"], 0.0, 18.0 * U * r["Dabs"])
    Pt = P.transpose(-1, -2)
    w("dV", heads(g[:, :, 2], B, N, H), r["dV"], UBF, UBF * (Pt @ r["do"].abs()) + U * ((P * (E + n_k)[..., None]).transpose(-1, -2) @ r["do"].abs()))
    W = (E + 2.0)[..., None] * (r["dP"] - r["delta"][..., None]).abs() + 64.0 * r["G"] + 18.0 * r["Dabs"][..., None]
    f32 = P * W + n_k * dS.abs()
    ka, qa = r["k"].abs(), r["q"].abs()
    w("dQ", heads(g[:, :, 0], B, N, H), r["dQ"], UBF, 0.125 * (UBF * (dS.abs() @ ka) + U * (f32 @ ka)))
    w("dK", heads(g[:, :, 1], B, N, H), r["dK"], UBF, 0.125 * (UBF * (dS.abs().transpose(-1, -2) @ qa) + U * (f32.transpose(-1, -2) @ qa)))


def masked_rows_zero(dqkv, mask, B, N, H):
    """dK and dV rows of masked keys: bit pattern zero"""
    pad = ~mask.bool()
    return not bool(bits(dqkv.view(B, N, 3, H * 64)[:, :, 1:][pad]).any().item())


# ------------------------------------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------------------------------------
def prefix(N, lens):
    lens = torch.tensor([min(max(1, l), N) for l in lens])
    return (torch.arange(N)[None] < lens[:, None]).to(torch.uint8).to(DEV)


def holes(N, kind, gen):
    """one mask row with holes; at least one valid key.  head64 / head128: the first 64 / 128 keys masked (a whole streaming block / a
    whole resident chunk: "nothing but masked keys so far"); lastblock: the last 64-key block masked; even: every second key masked;
    random / sparse: each key valid with probability 0.5 / 0.1"""
    m = torch.ones(N, dtype=torch.bool)
    if kind in ("head64", "head128"):
        m[:min(64 if kind == "head64" else 128, N - 1)] = False
    elif kind == "lastblock":
        lo = 64 * ((N - 1) // 64)
        m[(lo if lo > 0 else N - 1 if N > 1 else N):] = False
    elif kind == "even":
        m[0::2] = False
    else:
        m = torch.rand(N, generator=gen) < (0.5 if kind == "random" else 0.1)
    if not m.any():
        m[N // 2] = True
    return m


def mask_sets(N, gen):
    """name -> uint8 [3, N] (None: no mask).  Prefix lengths 1, 16, 17, N - 1, N and a random one; hole masks as in `holes`."""
    hs = lambda *kinds: torch.stack([holes(N, kd, gen) for kd in kinds]).to(torch.uint8).to(DEV)
    return {"none": None,
            "prefixA": prefix(N, [1, 16, 17]),
            "prefixB": prefix(N, [N - 1, N, int(torch.randint(1, N + 1, (1,), generator=gen))]),
            "holesA": hs("head64", "lastblock", "random"),
            "holesB": hs("head128", "even", "sparse")}


def make_inputs(gen, B, N, H, peak):
    D = H * 64
    x = torch.randn(B, N, 3, D, generator=gen)
    x[:, :, :2] *= peak
    qkv = x.view(B, N, 3 * D).to(DEV).to(BF)
    dout = torch.randn(B, N, D, generator=gen).to(DEV).to(BF)
    return qkv, dout


# ------------------------------------------------------------------------------------------------------------------------------
# 1. elementwise bars on random data
# ------------------------------------------------------------------------------------------------------------------------------
CASES = [(N, f) for N in NS for f in families(N)]


@pytest.mark.parametrize("N,fam", CASES)
def test_elementwise(ops, N, fam):
    """Forward against float64 softmax attention on the bf16-rounded qkv; backward against the float64 restatement on the kernel's own
    inputs, twice: on the forward kernel's out / lse ("bwd") and on the float64 reference's out / lse rounded to bf16 / fp32 ("bwd@ref").
    randn inputs and a peaked variant (q, k times 3).  All of `mask_sets`; with a mask, dK / dV rows of masked keys are zero bit for bit.
    fp32 counts: `chain`, `e_p`, `fwd_bars`, `bwd_bars`."""
    gen = torch.Generator().manual_seed(7000 + N)
    w = Worst(f"N={N} {fam}")
    masks = mask_sets(N, gen)
    with family(ops, fam):
        for peak in (1.0, 3.0):
            for mname, mask in masks.items():
                shapes = [(3, 3)] if N <= 272 else [(3, 1), (1, 3)] if mask is None else [(3, 1)]
                for B, H in shapes:
                    qkv, dout = make_inputs(gen, B, N, H, peak)
                    out, lse = run_fwd(ops, qkv, mask, B, N, H)
                    r = fwd_ref(qkv, mask, B, N, H)
                    fwd_bars(w, fam, r, out, lse, B, N, H)
                    ref_out = r["out"].permute(0, 2, 1, 3).reshape(B, N, H * 64).to(BF)
                    for tag, o_in, l_in in (("", out, lse), ("@ref", ref_out, r["lse"].to(F32))):
                        dqkv, delta = run_bwd(ops, qkv, o_in, dout, l_in, mask, B, N, H)
                        rb = bwd_ref(qkv, o_in, l_in, dout, mask, B, N, H)
                        bwd_bars(lambda n, *a, _t=tag: w(n + _t, *a), fam, rb, dqkv, delta, B, N, H)
                        if mask is not None:
                            assert masked_rows_zero(dqkv, mask, B, N, H), (mname, "dK / dV rows of masked keys are not zero")
    w.report()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. exact data
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("N,fam", [(N, f) for N in (17, 80, 197, 208, 272, 577, 592, 1025) for f in families(N)])
def test_onehot(ops, N, fam, masked):
    """k_j = 4 * (seeded random +-1 vector), q_i = k_perm(i): the matching score is 128 and, asserted on the float64 scores before the
    launch, every other score is at least 40 lower in the log2 domain, so all other keys together weigh less than N * 2^-40.  out[i] must
    equal V[perm(i)] and dV must equal dout permuted back, bit for bit; lse must be 128 within the forward's fp32 bar (with A = 128).
    perm(i) = i + off (mod the valid keys) for off over the multiples of 16, 1 and n - 1: every (query tile, key tile) pair is on the
    diagonal at least once; one (batch, head) per offset.  With a mask: the permutation runs inside the valid keys; queries at masked
    positions look at a valid key and carry dout = 0."""
    gen = torch.Generator().manual_seed(1000 + N)
    Kmat = 4.0 * (torch.randint(0, 2, (N, 64), generator=gen) * 2 - 1).to(F64)
    S2 = (Kmat @ Kmat.t()) * 0.125 * LOG2E
    other = S2 - torch.diag(torch.full((N,), math.inf, dtype=F64))
    assert float(S2.diagonal().min()) == 128 * LOG2E and (N == 1 or float(other.max()) <= 128 * LOG2E - 40), "one-hot gap too small"
    valid = torch.ones(N, dtype=torch.bool)
    if masked:
        valid = torch.rand(N, generator=gen) < 0.7
        valid[:min(16, N - 1)] = False
        valid[N - 1] = True
    vi = valid.nonzero().flatten()
    nv = len(vi)
    offs = sorted(set(range(0, nv, 16)) | {1 % nv, nv - 1})
    H = 3 if N <= 272 else 1
    B = (len(offs) + H - 1) // H
    rank = torch.cumsum(valid.long(), 0) - 1
    target = torch.empty(B, H, N, dtype=torch.long)
    for u in range(B * H):
        off = offs[u % len(offs)]
        t = vi[torch.arange(N) % nv]                             # queries at masked positions
        t[vi] = vi[(rank[vi] + off) % nv]
        target[u // H, u % H] = t
    q = Kmat[target]                                             # [B, H, N, 64]
    k = Kmat[None, None].expand(B, H, N, 64)
    v = nonzero(torch.randn(B, H, N, 64, generator=gen).to(BF))
    qkv = torch.stack([q.to(BF), k.to(BF), v], 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * 64).contiguous().to(DEV)
    dout = nonzero(torch.randn(B, H, N, 64, generator=gen).to(BF)) * valid.to(BF)[None, None, :, None]
    mask = valid.to(torch.uint8)[None].expand(B, N).contiguous().to(DEV) if masked else None
    target = target.to(DEV)
    with family(ops, fam):
        out, lse = run_fwd(ops, qkv, mask, B, N, H)
        dqkv, _ = run_bwd(ops, qkv, out, dout.permute(0, 2, 1, 3).reshape(B, N, H * 64).contiguous().to(DEV), lse, mask, B, N, H)
    idx = target[..., None].expand(B, H, N, 64)
    want = torch.gather(v.to(DEV), 2, idx)
    got = out.view(B, N, H, 64).permute(0, 2, 1, 3)
    assert same_bits(got, want), f"out != V[perm]: {int((bits(got) != bits(want)).any(-1).sum())} rows differ"
    want_dv = torch.zeros(B, H, N, 64, dtype=BF, device=DEV)
    src = target[:, :, vi.to(DEV)]                               # valid query vi[r] -> its key
    want_dv.scatter_(2, src[..., None].expand(B, H, nv, 64), dout.to(DEV)[:, :, vi.to(DEV)])
    got_dv = dqkv.view(B, N, 3, H, 64)[:, :, 2].permute(0, 2, 1, 3)
    assert same_bits(got_dv, want_dv), f"dV != dout permuted back: {int((bits(got_dv) != bits(want_dv)).any(-1).sum())} rows differ"
    n_l, _, _ = chain(fam, N)
    E = 70.0 * 128.0 + 3.0 * math.log(max(N, 2)) + 2.0
    ref = torch.full((B, H, N), 128.0, dtype=F64, device=DEV)
    check(f"onehot N={N} {fam} masked={masked} lse", lse, ref, torch.ones_like(ref), 0.0, U * (E + n_l + 2.0 * math.log2(max(N, 2)) + 4.0 * 128.0))


@pytest.mark.parametrize("N,fam", [(N, f) for N in (1, 16, 17, 64, 65, 128, 129, 197, 257, 577, 1025) for f in families(N)])
def test_uniform(ops, N, fam):
    """q = 0: every score is exactly 0, every probability exactly 1, the row sum the exact integer n_valid.  lse must be ln(n_valid) within
    U (n_l + 2 log2 N + 4 ln n_valid) (row sum chain, which is exact here but counted as in `fwd_bars`; v_log_f32 one ulp; the product with
    the rounded ln 2: `fwd_bars` with A = 0 and its exp2 terms dropped) - one leaked or dropped key moves it by 1 / n.  Where n_valid is
    a power of two, V holding integers in [-8, 8] makes P.V, 1 / l and their product exact: out must equal the bf16 rounding of the mean."""
    gen = torch.Generator().manual_seed(300 + N)
    B, H = 3, (3 if N <= 272 else 1)
    D = H * 64
    x = torch.randn(B, N, 3, D, generator=gen)
    x[:, :, 0] = 0.0
    x[:, :, 2] = torch.randint(-8, 9, (B, N, D), generator=gen).float()
    qkv = x.view(B, N, 3 * D).to(DEV).to(BF)
    p2 = 1 << (N.bit_length() - 1)
    scattered = torch.zeros(3, N, dtype=torch.bool)
    for b, n in enumerate((p2, max(1, p2 // 2), 1)):
        scattered[b, torch.randperm(N, generator=gen)[:n]] = True
    masks = {"none": None, "prefix": prefix(N, [p2, min(16, p2), 1]), "scattered": scattered.to(torch.uint8).to(DEV)}
    n_l, _, _ = chain(fam, N)
    _, _, v = split(qkv, B, N, H)
    with family(ops, fam):
        for mname, mask in masks.items():
            out, lse = run_fwd(ops, qkv, mask, B, N, H)
            valid = torch.ones(B, N, dtype=torch.bool, device=DEV) if mask is None else mask.bool()
            nv = valid.sum(1).to(F64)                                                    # [B]
            ref = torch.log(nv)[:, None, None].expand(B, H, N)
            check(f"uniform N={N} {fam} {mname} lse", lse, ref, n_l + 2.0 * math.log2(max(N, 2)) + 4.0 * ref.abs(), 0.0, U)
            mean = (v * valid.to(F64)[:, None, :, None]).sum(2) / nv[:, None, None]      # [B, H, 64]
            got = out.view(B, N, H, 64).permute(0, 2, 1, 3)
            for b in range(B):
                n = int(nv[b].item())
                if n & (n - 1) == 0:
                    want = mean[b].to(F32).to(BF)[:, None, :].expand(H, N, 64)
                    assert same_bits(got[b], want), (mname, b, n, "out != bf16(mean of the valid V rows)")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. invariances, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
def fwd_bwd(ops, qkv, dout, mask, B, N, H):
    out, lse = run_fwd(ops, qkv, mask, B, N, H)
    dqkv, delta = run_bwd(ops, qkv, out, dout, lse, mask, B, N, H)
    return out, lse, dqkv, delta


@pytest.mark.parametrize("N,fam", [(N, f) for N in (17, 80, 129, 197, 272, 577, 1025) for f in families(N)])
def test_masked_contents(ops, N, fam):
    """The K and V rows of masked keys hold +-2^60 in one run and zeros in the other: out, lse, dQ, delta and the valid rows of dK, dV
    must be bit-identical (finite values: 0 * 2^60 = 0 in the kernel as in any float reference), the masked rows zero in both."""
    gen = torch.Generator().manual_seed(500 + N)
    B, H = 3, 2
    D = H * 64
    w = mask_sets(N, gen)
    for mname in ("prefixA", "prefixB", "holesA", "holesB"):
        mask = w[mname]
        qkv, dout = make_inputs(gen, B, N, H, 1.0)
        dead = ~mask.bool()
        big = (torch.randint(0, 2, (B, N, 2 * D), generator=gen) * 2 - 1).to(DEV).to(BF) * 2.0 ** 60
        a, b = qkv.clone().view(B, N, 3, D), qkv.clone().view(B, N, 3, D)
        a[:, :, 1:][dead] = 0
        b[:, :, 1:][dead] = big.view(B, N, 2, D)[dead]
        with family(ops, fam):
            ra = fwd_bwd(ops, a.view(B, N, 3 * D), dout, mask, B, N, H)
            rb = fwd_bwd(ops, b.view(B, N, 3 * D), dout, mask, B, N, H)
        for nm, x, y in zip(("out", "lse", "dqkv", "delta"), ra, rb):
            assert same_bits(x, y), (mname, nm, "depends on the contents of masked keys")
        assert masked_rows_zero(ra[2], mask, B, N, H) and masked_rows_zero(rb[2], mask, B, N, H), mname


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("N,fam", [(N, f) for N in (16, 65, 197, 257, 577, 1025) for f in families(N)])
def test_batch_head_independence(ops, N, fam, masked):
    """Sequence b, head h of a (3, 3) call equals the (1, 1) call on that slice, and two runs of the same call are bit-identical (no
    atomics).  Option 15 is pinned by `family`, so both sides run the same build."""
    gen = torch.Generator().manual_seed(900 + N)
    B, H = 3, 3
    qkv, dout = make_inputs(gen, B, N, H, 1.0)
    mask = mask_sets(N, gen)["holesA" if N > 64 else "prefixB"] if masked else None
    with family(ops, fam):
        full = fwd_bwd(ops, qkv, dout, mask, B, N, H)
        again = fwd_bwd(ops, qkv, dout, mask, B, N, H)
        for nm, x, y in zip(("out", "lse", "dqkv", "delta"), full, again):
            assert same_bits(x, y), (nm, "two runs differ")
        out, lse, dqkv, delta = full
        for b in range(B):
            for h in range(H):
                q1 = qkv.view(B, N, 3, H, 64)[b:b + 1, :, :, h].reshape(1, N, 192).contiguous()
                d1 = dout.view(B, N, H, 64)[b:b + 1, :, h].contiguous()
                o1, l1, g1, dl1 = fwd_bwd(ops, q1, d1, None if mask is None else mask[b:b + 1].contiguous(), 1, N, 1)
                assert same_bits(out.view(B, N, H, 64)[b, :, h], o1[0]), ("out", b, h)
                assert same_bits(lse[b, h], l1[0, 0]), ("lse", b, h)
                assert same_bits(dqkv.view(B, N, 3, H, 64)[b, :, :, h], g1.view(N, 3, 64)), ("dqkv", b, h)
                assert same_bits(delta[b, h], dl1[0, 0]), ("delta", b, h)


@pytest.mark.parametrize("H", [1, 3])
def test_varlen_equals_resident(ops, H):
    """Sequence b of medmoe_attn_fwd_varlen equals the resident unmasked forward on that sequence alone at N = len(b) (both the 5-tile
    256-thread build), for lengths 1, 16, 17, 79, 80 mixed in one batch.  The packed out carries sentinel rows after the packed end; lse
    rows are [Nmax] long and entries at positions >= len(b) are unspecified (only the tail of the buffer is checked for them)."""
    gen = torch.Generator().manual_seed(42 + H)
    lens = [17, 1, 80, 16, 79, 1, 80]
    B, Nmax, D = len(lens), 80, H * 64
    tot = sum(lens)
    off = torch.tensor([0] + lens).cumsum(0).to(torch.int32).to(DEV)
    qkv = torch.randn(tot, 3 * D, generator=gen).to(DEV).to(BF)
    ob, out = guarded((tot, D), BF)
    lb, lse = guarded((B, H, Nmax), F32)
    with family(ops, "res"):
        ops.call("attn_fwd_varlen", qkv, out, lse, off, B, Nmax, H, 64)
        torch.cuda.synchronize()
        assert tail_ok(ob, out.numel()) and tail_ok(lb, lse.numel()) and written(out)
        r0 = 0
        for b, n in enumerate(lens):
            o1, l1 = run_fwd(ops, qkv[r0:r0 + n].contiguous().view(1, n, 3 * D), None, 1, n, H)
            assert same_bits(out[r0:r0 + n], o1[0]), ("out", b, n)
            assert same_bits(lse[b, :, :n], l1[0]), ("lse", b, n)
            r0 += n


# ------------------------------------------------------------------------------------------------------------------------------
# 4. window attention
# ------------------------------------------------------------------------------------------------------------------------------
WIN_GEOM = [(2, 14, 96, 3, 0), (2, 14, 96, 3, 3), (3, 7, 768, 24, 0), (1, 28, 192, 6, 3), (2, 56, 96, 3, 3), (1, 14, 96, 3, 0), (1, 14, 96, 3, 3)]
WSCALE = 32 ** -0.5


def win_rows(B, H, W, shift):
    """rows [B * nW, 49] of the token-major activation behind every window (cyclic shift + window partition of SwinLayer.forward) and
    the shift-mask region ids [nW, 49] (get_attn_mask: slices (0, -7), (-7, -shift), (-shift, None) of the shifted image)"""
    Y, X = torch.arange(H), torch.arange(W)
    rows = (torch.arange(B)[:, None, None] * H + ((Y + shift) % H)[None, :, None]) * W + ((X + shift) % W)[None, None, :]
    part = lambda t, n: t.view(n, H // 7, 7, W // 7, 7).permute(0, 1, 3, 2, 4).reshape(-1, 49)
    reg = lambda c, n: (c >= n - 7).long() + (c >= n - shift).long()
    ids = reg(Y, H)[:, None] * 3 + reg(X, W)[None, :] if shift else torch.zeros(H, W, dtype=torch.long)
    return part(rows, B).to(DEV), part(ids[None], 1).to(DEV)


def win_bias(gen, nheads, table_std=0.5):
    """relative position bias of the 49 x 49 token pairs from a random [169, heads] table, padded as the kernel wants it: [heads][64][64],
    key columns >= 49 at -30000, everything else 0"""
    c = torch.stack(torch.meshgrid(torch.arange(7), torch.arange(7), indexing="ij")).flatten(1)
    d = c[:, :, None] - c[:, None, :] + 6
    index = d[0] * 13 + d[1]
    table = torch.randn(169, nheads, generator=gen) * table_std
    b = torch.zeros(nheads, 64, 64)
    b[:, :, 49:] = -30000.0
    b[:, :49, :49] = table[index.view(-1)].view(49, 49, nheads).permute(2, 0, 1)
    return b.contiguous().to(DEV)


def win_split(t, rows, nheads):
    """[B*H*W, n*C] -> float64 [n][B*nW, heads, 49, 32]"""
    C = nheads * 32
    g = t.to(F64)[rows]                                          # [B*nW, 49, n*C]
    return g.view(g.shape[0], 49, -1, nheads, 32).permute(2, 0, 3, 1, 4)


def win_scores64(qkv, bias, rows, ids, nheads, shift):
    q, k, v = win_split(qkv, rows, nheads)
    nW = ids.shape[0]
    S = q @ k.transpose(-1, -2) * WSCALE + bias.to(F64)[None, :, :49, :49]
    M = (q.abs() @ k.abs().transpose(-1, -2)) * WSCALE + bias.to(F64).abs()[None, :, :49, :49]
    if shift:
        cross = (ids[:, :, None] != ids[:, None, :]).to(F64) * 100.0        # [nW, 49, 49]
        cross = cross.repeat(S.shape[0] // nW, 1, 1)[:, None]
        S, M = S - cross, M + cross
    return q, k, v, S, M


def win_e(M):
    """fp32 roundings behind one window probability, relative, in U, per query row; M = scale sum |q_d k_d| + |bias| + 100 (shift mask)
    bounds |s|:  32 M the score (32 products in one MFMA); 9 M: acc * scale + bias with the rounded constant scale (2), - 100 (1),
    - m or - lse (1 on <= 2 M), __expf = exp2(x log2 e) (2 on <= 2 M); 3 ln 64 for |lse| <= max|s| + ln 64; 2 for v_exp_f32."""
    return 41.0 * M.amax(-1) + 3.0 * math.log(64.0) + 2.0


def win_run(ops, qkv, bias, dout, B, H, W, C, nheads, shift):
    n_units = B * (H // 7) * (W // 7) * nheads
    ob, out = guarded((B * H * W, C), BF)
    lb, lse = guarded((n_units, 64), F32)
    ops.call("win_attn_fwd", qkv, bias, out, lse, B, H, W, C, nheads, shift)
    gb, dqkv = guarded((B * H * W, 3 * C), BF)
    sb, slabs = guarded((n_units, 64, 64), F32)
    ops.call("win_attn_bwd", qkv, bias, dout, lse, dqkv, slabs, B, H, W, C, nheads, shift)
    torch.cuda.synchronize()
    for nm, buf, body in (("out", ob, out), ("lse", lb, lse), ("dqkv", gb, dqkv), ("dbias", sb, slabs)):
        assert tail_ok(buf, body.numel()), f"{nm}: written past the end"
        assert written(body), f"{nm}: not fully written"
    return out, lse, dqkv, slabs


@pytest.mark.parametrize("B,H,C,nheads,shift", WIN_GEOM)
def test_window_elementwise(ops, B, H, C, nheads, shift):
    """out, lse, dqkv and the dbias slabs against the float64 restatement (backward on the kernel's own lse; the kernel's delta is
    sum_k p dP, it does not read out).  Bars, with E = `win_e`:
      out   c_r = UBF; (UBF + U (2 E + 4 + 21 + 64)) sum_k p |v|: the NORMALISED probabilities are rounded to bf16; each carries its own
            and the row sum's exponent error (2 (E + 2)), the row sum's 16 + 2 adds, 1 / s and p * inv (21), 64 accumulated products.
      lse   c_r = 0; U (E + 18 + 2 ln 64 + 2 |lse|): exponent error, row sum chain, __logf = log2 * ln 2 (one ulp + a rounding), m + log s.
      dbias c_r = 0; U p w, w = (E + 2) |dP - delta| + 32 sum_d |dO V| (dP: 32 products) + sum_k p ((E + 19) |dP| + 32 sum_d |dO V|)
            (delta: every p dP term's own error, 16 + 2 adds and the product), + 2^-126: below the smallest normal fp32 number a
            probability is flushed to zero (pairs behind the shift mask: e^-100).
      dV    c_r = UBF; (UBF + U (E + 64)) sum_q p |dO|.
      dQ    c_r = UBF; scale (UBF sum_k |dS| |K| + U sum_k (p w + 66 |dS|) |K|): 64 accumulated products, the rounded scale and its product;
            dK likewise over q.
    Rows and columns 49 .. 63 of a slab: a padded query has dO = 0, so dP = 0 and delta = 0 and dS = p * 0; a padded key has the bias
    -30000, so p = 0: the kernel writes zeros there, asserted by value."""
    gen = torch.Generator().manual_seed(11 * H + shift + B)
    W = H
    qkv = torch.randn(B * H * W, 3 * C, generator=gen).to(DEV).to(BF)
    dout = (torch.randn(B * H * W, C, generator=gen) * 0.5).to(DEV).to(BF)
    bias = win_bias(gen, nheads)
    rows, ids = win_rows(B, H, W, shift)
    out, lse, dqkv, slabs = win_run(ops, qkv, bias, dout, B, H, W, C, nheads, shift)
    q, k, v, S, M = win_scores64(qkv, bias, rows, ids, nheads, shift)
    E = win_e(M)
    w = Worst(f"window B={B} H={H} C={C} shift={shift}")
    lse_ref = torch.logsumexp(S, -1)
    P = torch.exp(S - lse_ref[..., None])
    got_out = win_split(out, rows, nheads)[0]
    w("out", got_out, P @ v, UBF, (UBF + U * (2.0 * E + 89.0))[..., None] * (P @ v.abs()))
    lse_k = lse.view(-1, nheads, 64)[:, :, :49]
    w("lse", lse_k, lse_ref, 0.0, U * (E + 18.0 + 2.0 * math.log(64.0) + 2.0 * lse_ref.abs()))
    # backward on the kernel's own lse
    P = torch.exp(S - lse_k.to(F64)[..., None])
    do = win_split(dout, rows, nheads)[0]
    dP = do @ v.transpose(-1, -2)
    G = do.abs() @ v.abs().transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    Wt = (E + 2.0)[..., None] * (dP - delta).abs() + 32.0 * G + (P * ((E + 19.0)[..., None] * dP.abs() + 32.0 * G)).sum(-1, keepdim=True)
    sl = slabs.view(-1, nheads, 64, 64)
    w("dbias", sl[:, :, :49, :49], dS, 0.0, U * P * Wt + 2.0 ** -126)
    assert bool((sl[:, :, 49:, :] == 0).all()) and bool((sl[:, :, :, 49:] == 0).all()), "dbias slab rows / columns 49..63 are not zero"
    gq, gk, gv = win_split(dqkv, rows, nheads)
    w("dV", gv, P.transpose(-1, -2) @ do, UBF, UBF * (P.transpose(-1, -2) @ do.abs()) + U * ((P * (E + 64.0)[..., None]).transpose(-1, -2) @ do.abs()))
    f32 = P * Wt + 66.0 * dS.abs()
    w("dQ", gq, WSCALE * dS @ k, UBF, WSCALE * (UBF * (dS.abs() @ k.abs()) + U * (f32 @ k.abs())))
    w("dK", gk, WSCALE * dS.transpose(-1, -2) @ q, UBF, WSCALE * (UBF * (dS.abs().transpose(-1, -2) @ q.abs()) + U * (f32.transpose(-1, -2) @ q.abs())))
    w.report()


@pytest.mark.parametrize("by_bias", [False, True])
@pytest.mark.parametrize("B,H,C,nheads,shift", WIN_GEOM)
def test_window_onehot(ops, B, H, C, nheads, shift, by_bias):
    """Every query of a window looks at exactly one key of its own shift-mask region: target(i) = the next token (cyclically, a stride per
    head) among those with i's region id.  by_bias = False: bias zero, k_j = 8 * (seeded +-1 vector of 32), q_i = k_target(i): the matching
    score is 2048 / sqrt(32) = 362 and, asserted before the launch, every other one is at least 40 lower in the log2 domain.
    by_bias = True: q = 0 and the bias alone decides: 60 at (i, target(i)), 0 elsewhere (gap 60 log2(e) = 86).  Tokens of other regions sit
    another 100 lower through the shift mask.  out[i] must equal V[target(i)] and dV must equal dout permuted back, bit for bit."""
    gen = torch.Generator().manual_seed(77 + H + shift)
    W = H
    rows, ids = win_rows(B, H, W, shift)
    nW, U0 = ids.shape[0], rows.shape[0]
    target = torch.empty(nW, nheads, 49, dtype=torch.long)
    for wdx in range(nW):
        for r in ids[wdx].unique().tolist():
            mem = (ids[wdx] == r).nonzero().flatten().cpu()
            for h in range(nheads):
                target[wdx, h, mem] = mem[(torch.arange(len(mem)) + 1 + h) % len(mem)]
    Kmat = 8.0 * (torch.randint(0, 2, (49, 32), generator=gen) * 2 - 1).to(F64)
    S2 = Kmat @ Kmat.t() * WSCALE * LOG2E
    assert float((S2 - torch.diag(torch.full((49,), math.inf, dtype=F64))).max()) <= float(S2.diagonal().min()) - 40, "one-hot gap too small"
    tgt = target.repeat(B, 1, 1)                                                  # [B*nW, heads, 49]
    qw = torch.zeros(U0, nheads, 49, 32, dtype=F64) if by_bias else Kmat[tgt]
    kw = Kmat[None, None].expand(U0, nheads, 49, 32)
    vw = nonzero(torch.randn(U0, nheads, 49, 32, generator=gen).to(BF))
    gw = nonzero(torch.randn(U0, nheads, 49, 32, generator=gen).to(BF))
    pack = lambda *ts: torch.cat([t.to(BF).permute(0, 2, 1, 3).reshape(U0, 49, C) for t in ts], -1)
    qkv = torch.zeros(B * H * W, 3 * C, dtype=BF, device=DEV)
    qkv[rows] = pack(qw, kw, vw).to(DEV)
    dout = torch.zeros(B * H * W, C, dtype=BF, device=DEV)
    dout[rows] = pack(gw).to(DEV)
    idx = tgt.to(DEV)[..., None].expand(U0, nheads, 49, 32)
    want = torch.gather(vw.to(DEV), 2, idx)
    want_dv = torch.empty_like(want).scatter_(2, idx, gw.to(DEV))
    # the bias is shared by all windows, their region layouts (hence target) are not: with by_bias, one launch per layout of interest (the
    # first window: one region; the last: every region of the shifted image), comparing the windows that have that layout
    for layout in ([target[0], target[nW - 1]] if by_bias else [None]):
        bias = torch.zeros(nheads, 64, 64)
        bias[:, :, 49:] = -30000.0
        sel = torch.ones(U0, dtype=torch.bool)
        if by_bias:
            bias[:, :49, :49].scatter_(2, layout[..., None], 60.0)
            sel = torch.tensor([bool((target[wdx] == layout).all()) for wdx in range(nW)]).repeat(B)
        sel = sel.to(DEV)
        out, lse, dqkv, slabs = win_run(ops, qkv, bias.to(DEV), dout, B, H, W, C, nheads, shift)
        got = out[rows].view(U0, 49, nheads, 32).permute(0, 2, 1, 3)
        assert same_bits(got[sel], want[sel]), "out != V[target]"
        got_dv = dqkv[rows][:, :, 2 * C:].reshape(U0, 49, nheads, 32).permute(0, 2, 1, 3)
        assert same_bits(got_dv[sel], want_dv[sel]), "dV != dout permuted back"


@pytest.mark.parametrize("B,H,C,nheads,shift", WIN_GEOM)
def test_window_independence(ops, B, H, C, nheads, shift):
    """Bit for bit: two runs agree; image b of the batch equals the B = 1 call on that image; replacing the tokens of one window (the
    first of image 0, in shifted coordinates) changes nothing outside that window's rows and slabs."""
    gen = torch.Generator().manual_seed(5 + H + shift)
    W = H
    T = H * W
    qkv = torch.randn(B * T, 3 * C, generator=gen).to(DEV).to(BF)
    dout = torch.randn(B * T, C, generator=gen).to(DEV).to(BF)
    bias = win_bias(gen, nheads)
    full = win_run(ops, qkv, bias, dout, B, H, W, C, nheads, shift)
    for nm, x, y in zip(("out", "lse", "dqkv", "dbias"), full, win_run(ops, qkv, bias, dout, B, H, W, C, nheads, shift)):
        assert same_bits(x, y), (nm, "two runs differ")
    upi = (H // 7) * (W // 7) * nheads                           # units per image
    for b in range(B):
        one = win_run(ops, qkv[b * T:(b + 1) * T].contiguous(), bias, dout[b * T:(b + 1) * T].contiguous(), 1, H, W, C, nheads, shift)
        for nm, x, y, per in zip(("out", "lse", "dqkv", "dbias"), full, one, (T, upi, T, upi)):
            assert same_bits(x[b * per:(b + 1) * per], y), (nm, b, "depends on the other images")
    rows, _ = win_rows(B, H, W, shift)
    q2, d2 = qkv.clone(), dout.clone()
    q2[rows[0]] = torch.randn(49, 3 * C, generator=gen).to(DEV).to(BF)
    d2[rows[0]] = torch.randn(49, C, generator=gen).to(DEV).to(BF)
    other = win_run(ops, q2, bias, d2, B, H, W, C, nheads, shift)
    keep = torch.ones(B * T, dtype=torch.bool, device=DEV)
    keep[rows[0]] = False
    for nm, x, y in zip(("out", "lse", "dqkv", "dbias"), full, other):
        if nm in ("out", "dqkv"):
            assert same_bits(x[keep], y[keep]), (nm, "depends on another window")
        else:
            assert same_bits(x[nheads:], y[nheads:]), (nm, "depends on another window")
