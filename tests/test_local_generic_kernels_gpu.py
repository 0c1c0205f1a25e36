"""The generic-geometry local-loss kernels (loss.hip "GENERIC-GEOMETRY": local_gen_fwd_a / cos / dwctx / dwords / bwd_s, unpad_cast / unpad_cast2),
each one alone against a float64 restatement of its contract, at every template instance and index path; then `GenericLocalLoss` at every Tp
class, judged per block.  Order: (1) the float64 references, (2) a CPU test that proves them against the oracle (their chain reproduces
`medmoe_oracle.gloria_local` and its autograd to 1e-9), (3) per-kernel GPU tests with DERIVED error bars, (4) the whole object.

Error-bar vocabulary (u = 2^-24, one fp32 rounding):
  bf16 output           2^-8 |ref|: one round-to-nearest of an 8-bit significand is at most half an ulp = 2^-8 of the binade's lower end (2^-9
                        relative at its upper end); what fp32 arithmetic before the rounding adds is bounded separately by the terms below
  fp32 sum of n terms   n u sum|term|, sum|term| from the float64 reference (absolute: the sums of bwd_s cancel)
  __expf / __logf       2^-20 relative / absolute (v_exp_f32, v_log_f32: 1 ulp; the argument's rounding adds |x| u with |x| <= temp2 = 5)
  exp(lp), lp a half    (2 |lp| + 2) u: lp * log2(e) rounds twice (the constant and the product, |lp| u each after the exponential), v_exp_f32 1 ulp
  zeros, untouched      torch.equal
Every input is exactly representable in its storage type, so the float64 reference starts from the kernel's own numbers."""
import math

import pytest
import torch
import torch.nn.functional as F

import medmoe_oracle as O

F64, F32, F16, BF, I32 = torch.float64, torch.float32, torch.float16, torch.bfloat16, torch.int32
U = 2.0 ** -24
T1, T2, EPS = 4.0, 5.0, 1e-8
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------
# 1. float64 references: one kernel's contract each, read from the kernel and its header comment.
#    Pair tensors are logical [B, HWp, Bc, Tp] (region row, caption, word); WC / DWC / stats are [B, Bc, Tp, ...].
# ---------------------------------------------------------------------------------------------
def clamp_caps(cap_lens, T, Tp):
    return [max(1, min(int(c), T, Tp)) for c in cap_lens]


def word_mask(caps, Tp):
    return torch.arange(Tp)[None, :] < torch.tensor(caps)[:, None]                                # [Bc, Tp]


def ref_fwd_a(lp, caps, HW, temp1):
    """A = softmax over hw < HW of temp1 * exp(lp) for t < cap; exact zeros elsewhere."""
    live = word_mask(caps, lp.shape[3])[None, None] & (torch.arange(lp.shape[1]) < HW)[None, :, None, None]
    x = torch.where(live, temp1 * torch.exp(lp), torch.full_like(lp, -math.inf))
    return torch.where(live, torch.softmax(x, dim=1), torch.zeros_like(lp))


def ref_cos(wc, words, wnorm, caps, temp2, eps):
    """stats = {cos, n2, e, 0} (zero for t >= cap), sume = sum_{t<cap} e, sim = log sume.  Differentiable in wc, words and wnorm."""
    B, Bc, Tp, D = wc.shape
    T = words.shape[1]
    live = word_mask(caps, Tp)[None]                                                             # [1, Bc, Tp]
    w = F.pad(words, (0, 0, 0, Tp - T))[None]
    wn = F.pad(wnorm, (0, Tp - T))[None]
    v = torch.where(live[..., None], wc, torch.zeros_like(wc))
    n2 = (v * v).sum(-1)
    cos = (w * v).sum(-1) / torch.clamp(wn * torch.linalg.vector_norm(v, dim=-1), min=eps)
    e = torch.where(live, torch.exp(temp2 * cos), torch.zeros_like(cos))
    z = torch.zeros_like(cos)
    stats = torch.stack([torch.where(live, cos, z), n2, e, z], dim=-1)
    sume = e.sum(-1)
    return stats, sume, torch.log(sume)


def ref_dwctx(wc, words, wnorm, caps, gsim, temp2, eps):
    """d (sum gsim * sim) / d wc: float64 autograd of ref_cos (the clamp keeps den < eps consistent with the forward); zero rows for t >= cap."""
    x = wc.clone().requires_grad_(True)
    sim = ref_cos(x, words, wnorm, caps, temp2, eps)[2]
    return torch.autograd.grad((gsim * sim).sum(), x)[0]


def ref_dwords(wc, words, caps, gsim, dws, temp2, eps):
    """dws[col] + d (sum_b gsim[b,i] sim[b,i]) / d word through the cosine only; |w| is a function of the word; zero rows for t >= cap."""
    T = words.shape[1]
    x = words.clone().requires_grad_(True)
    sim = ref_cos(wc, x, torch.linalg.vector_norm(x, dim=-1), caps, temp2, eps)[2]
    g = torch.autograd.grad((gsim * sim).sum(), x)[0]
    if dws is not None:
        g = g + dws[:, :T]
    return torch.where(word_mask(caps, T)[..., None], g, torch.zeros_like(g))


def ref_bwd_s(lp, A, dA, caps, HW, temp1):
    """ca_t = sum_hw A dA; da1 = temp1 A (dA - ca_t); dS = a1 (da1 - sum_t a1 da1), a1 = exp(lp) for t < cap; zeros outside [HW][cap]."""
    live = word_mask(caps, lp.shape[3])[None, None] & (torch.arange(lp.shape[1]) < HW)[None, :, None, None]
    z = torch.zeros_like(lp)
    a1 = torch.where(live, torch.exp(lp), z)
    Al, dAl = torch.where(live, A, z), torch.where(live, dA, z)
    ca = (Al * dAl).sum(1, keepdim=True)
    da1 = temp1 * Al * (dAl - ca)
    rd = (a1 * da1).sum(3, keepdim=True)
    return a1 * (da1 - rd)


def ref_unpad_cast(src, HW, src2=None):
    """rows < HW of fp32 [B, HWp, D] (plus src2, the sum formed in fp32), rounded once to bf16."""
    x = src[:, :HW] if src2 is None else src[:, :HW] + src2[:, :HW]
    return x.to(BF)


def ident(x):
    return x


def q16(x):
    return x.to(F16).to(F64)


def qbf(x):
    return x.to(BF).to(F64)


def ce_gsim(sim, scale=10.0):
    """d (CE rows + CE columns of scale * sim) / d sim, as tests/test_generic_word_grad_gpu.py takes it."""
    s = sim.detach().clone().requires_grad_(True)
    lab = torch.arange(s.shape[0], device=s.device)
    (F.cross_entropy(scale * s, lab) + F.cross_entropy(scale * s.t(), lab)).backward()
    return s.grad


def chain(ctx, words, cap_lens, temp1=T1, temp2=T2, eps=EPS, stored=False):
    """The references chained with float64 matmuls in place of the GEMMs: ctx [B, HW, D], words [B, T, D] -> sim, d ctx, d words of
    CE rows + CE columns of 10 * sim.  stored=True rounds every intermediate to the type GenericLocalLoss stores it in (lp fp16; A, DWC,
    dA, dS and d ctx bf16): the distance between the two chains is what the storage formats alone cost."""
    h, b = (q16, qbf) if stored else (ident, ident)
    B, HW, D = ctx.shape
    T = words.shape[1]
    caps = clamp_caps(cap_lens, T, T)
    S = torch.einsum("bhd,itd->bhit", ctx, words).masked_fill(~word_mask(caps, T)[None, None], -math.inf)
    lp = h(torch.log_softmax(S, dim=-1))
    A = b(ref_fwd_a(lp, caps, HW, temp1))
    wc = torch.einsum("bhit,bhd->bitd", A, ctx)
    wn = torch.linalg.vector_norm(words, dim=-1)
    sim = ref_cos(wc, words, wn, caps, temp2, eps)[2]
    gsim = ce_gsim(sim)
    dwc = b(ref_dwctx(wc, words, wn, caps, gsim, temp2, eps))
    dA = b(torch.einsum("bhd,bitd->bhit", ctx, dwc))
    dS = b(ref_bwd_s(lp, A, dA, caps, HW, temp1))
    dctx = b(torch.einsum("bhit,bitd->bhd", A, dwc) + torch.einsum("bhit,itd->bhd", dS, words))
    dws = torch.einsum("bhit,bhd->itd", dS, ctx)
    return dict(sim=sim, dctx=dctx, dwords=ref_dwords(wc, words, caps, gsim, dws, temp2, eps), caps=caps)


# ---------------------------------------------------------------------------------------------
# 2. the references against the oracle, on the CPU
# ---------------------------------------------------------------------------------------------
def test_reference_chain_reproduces_the_oracle():
    """sim, d ctx and d words of the float64 chain against medmoe_oracle.gloria_local in float64 and its autograd, 1e-9 relative."""
    B, H, W, T, D, caps = 3, 4, 5, 11, 16, [11, 1, 6]
    g = torch.Generator().manual_seed(0)
    img = torch.randn(B, D, H, W, generator=g, dtype=F64).requires_grad_(True)
    words = torch.randn(B, D, T, generator=g, dtype=F64).requires_grad_(True)
    sim_o = O.gloria_local_sim(img, words, caps, T1, T2)[0]
    l0, l1, _ = O.gloria_local(img, words, caps, T1, T2, 10.0)
    (l0 + l1).backward()
    got = chain(img.detach().reshape(B, D, H * W).transpose(1, 2), words.detach().transpose(1, 2), caps)
    for name, a, b in (("sim", got["sim"], sim_o.detach()), ("d ctx", got["dctx"], img.grad.reshape(B, D, H * W).transpose(1, 2)),
                       ("d words", got["dwords"], words.grad.transpose(1, 2))):
        e = float((a - b).abs().max() / b.abs().max())
        print(f"{name}: {e:.2e}")
        assert e < 1e-9, (name, e)


# ---------------------------------------------------------------------------------------------
# inputs and checks shared by the GPU tests
# ---------------------------------------------------------------------------------------------
def _check(got, ref, bar, what):
    """every element within its bar (bar 0: equal)"""
    got, ref, bar = got.detach().to(F64).cpu(), ref.to(F64), bar.to(F64).expand_as(ref)
    assert bool(torch.isfinite(got).all()), what + ": not finite"
    diff = (got - ref).abs()
    ratio = float((diff / bar.clamp_min(1e-300)).max()) if diff.numel() else 0.0
    print(f"{what}: worst |got - ref| / bar = {ratio:.3f}, max |diff| {float(diff.max()) if diff.numel() else 0.0:.3e}")
    bad = diff > bar
    assert not bool(bad.any()), (what, int(bad.sum()), ratio, [tuple(i) for i in bad.nonzero()[:4].tolist()])


def _sentinel(rows, cols, dtype):
    """a pattern that no kernel output equals by accident, compared by bits afterwards"""
    n = rows * cols
    if dtype in (BF, F16):
        return ((torch.arange(n, dtype=torch.int32) * 37 % 1999) + 0x3A00).to(torch.int16).view(dtype).reshape(rows, cols)
    return ((torch.arange(n, dtype=torch.int64) * 7919 % 65521) + 0x4B000000).to(torch.int32).view(F32).reshape(rows, cols)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _pair_buffer(x, ldp, dtype):
    """logical [B, HWp, Bc, Tp] -> device buffer [B*HWp, ldp] with sentinels in the columns past Bc*Tp; returns (buffer, the sentinels)"""
    B, HWp, Bc, Tp = x.shape
    s = _sentinel(B * HWp, ldp - Bc * Tp, dtype)
    return torch.cat([x.reshape(B * HWp, Bc * Tp).to(dtype), s], dim=1).contiguous().cuda(), s


def _pair_logical(buf, B, HWp, Bc, Tp):
    return buf.cpu()[:, :Bc * Tp].reshape(B, HWp, Bc, Tp)


def _pair_case(T, Tp, HW, HWp, seed, B=3, Bc=5):
    """lp (exact halves; masked words hold -inf or finite non-positive halves, rows HW..HWp NaN), A = bf16 of the reference, dA bf16"""
    g = torch.Generator().manual_seed(seed)
    cap_lens = [T + 9, 0, 1, T, T // 2]
    caps = clamp_caps(cap_lens, T, Tp)
    wm = word_mask(caps, Tp)[None, None].expand(B, HWp, Bc, Tp)
    s = (2.0 * torch.randn(B, HWp, Bc, Tp, generator=g)).masked_fill(~wm, -math.inf)
    junk = -(torch.rand(B, HWp, Bc, Tp, generator=g) * 40.0)
    junk = torch.where(torch.rand(B, HWp, Bc, Tp, generator=g) < 0.5, junk, torch.full_like(junk, -math.inf))
    lp = torch.where(wm, torch.log_softmax(s, dim=-1), junk).to(F16)
    lp[:, HW:] = math.nan                                      # the padded region rows are never read: a read of one shows
    A = ref_fwd_a(lp.to(F64), caps, HW, T1).to(BF)
    dA = (0.5 * torch.randn(B, HWp, Bc, Tp, generator=g)).to(BF)
    return dict(B=B, Bc=Bc, T=T, Tp=Tp, HW=HW, HWp=HWp, ldp=Bc * Tp + 24, caps=caps, lp=lp, A=A, dA=dA,
                cap=torch.tensor(cap_lens, dtype=I32).cuda(), live=wm & (torch.arange(HWp) < HW)[None, :, None, None])


TP_CASES = [(9, 16), (25, 32), (40, 48), (64, 64), (77, 80)]
HW_CASES = [(1, 16), (37, 48), (144, 144), (300, 304)]


# ---------------------------------------------------------------------------------------------
# 3. one kernel at a time
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("HW,HWp", HW_CASES)
@pytest.mark.parametrize("T,Tp", TP_CASES)
def test_fwd_a(T, Tp, HW, HWp):
    """local_gen_fwd_a<LP>, LP 1..4.  Bar per element: 2^-8 A (bf16) + (HW + 2 temp1 (2 L + 2) + 8) u A, L = max live |lp|: the column sum
    of HW terms, exp(temp1 a1) in the numerator and in the sum (argument error temp1 a1 (2|lp| + 2) u, a1 <= 1), 1 / sum and the product.
    Rows HW..HWp and words cap..Tp exact zeros; the columns Bc*Tp..ldp of A keep their bits."""
    from medmoe_amd import ops
    c = _pair_case(T, Tp, HW, HWp, seed=100 * Tp + HW)
    B, Bc, ldp = c["B"], c["Bc"], c["ldp"]
    lp, _ = _pair_buffer(c["lp"], ldp, F16)
    A, sent = _pair_buffer(_sentinel(B * HWp, Bc * Tp, BF).reshape(B, HWp, Bc, Tp), ldp, BF)
    ops.call("local_gen_fwd_a", lp, c["cap"], A, B, Bc, HW, HWp, T, Tp, T1, ldp)
    torch.cuda.synchronize()
    got = _pair_logical(A, B, HWp, Bc, Tp)
    ref = ref_fwd_a(c["lp"].to(F64), c["caps"], HW, T1)
    L = float(c["lp"].to(F64)[c["live"]].abs().max())
    assert torch.equal(_bits(A.cpu()[:, Bc * Tp:]), _bits(sent))
    assert torch.equal(got[~c["live"]].float(), torch.zeros(int((~c["live"]).sum())))
    _check(got, ref, (2.0 ** -8 + (HW + 2 * T1 * (2 * L + 2) + 8) * U) * ref, f"fwd_a Tp={Tp} HW={HW}")


@gpu
@pytest.mark.parametrize("HW,HWp", HW_CASES)
@pytest.mark.parametrize("T,Tp", TP_CASES)
def test_bwd_s(T, Tp, HW, HWp):
    """local_gen_bwd_s<LP>, LP 1..4, in place over dA.  Bar per element, every sum from the float64 reference:
      E_ca  = HW u sum_hw |A dA|                                 (A dA is exact in fp32: two 8-bit significands)
      E_da1 = temp1 A (E_ca + 3 u (|dA| + |ca|))                 (the difference and two products)
      E_rd  = sum_t a1 (E_da1 + eps_e |da1|) + (cap + 1) u sum_t |a1 da1|,   eps_e = (2 |lp| + 2) u for a1 = exp(lp)
      bar   = 2^-8 |dS| + a1 (E_da1 + E_rd + u (|da1| + |rd|)) + (eps_e + u) |dS|
    dA - ca and da1 - rd cancel, so the bar is absolute in the summed magnitudes, not relative to dS.  The buffer's rows HW..HWp and
    words cap..Tp hold garbage before the call and exact zeros after it; the columns Bc*Tp..ldp keep their bits."""
    from medmoe_amd import ops
    c = _pair_case(T, Tp, HW, HWp, seed=100 * Tp + HW + 1)
    B, Bc, ldp, live = c["B"], c["Bc"], c["ldp"], c["live"]
    g = torch.Generator().manual_seed(7)
    junk = (torch.randn(B, HWp, Bc, Tp, generator=g).abs() + 0.5).to(BF)
    lp, _ = _pair_buffer(c["lp"], ldp, F16)
    A, _ = _pair_buffer(c["A"], ldp, BF)
    io, sent = _pair_buffer(torch.where(live, c["dA"], junk), ldp, BF)
    ops.call("local_gen_bwd_s", lp, A, io, c["cap"], B, Bc, HW, HWp, T, Tp, T1, ldp)
    torch.cuda.synchronize()
    got = _pair_logical(io, B, HWp, Bc, Tp)
    assert torch.equal(_bits(io.cpu()[:, Bc * Tp:]), _bits(sent))
    assert torch.equal(got[~live].float(), torch.zeros(int((~live).sum())))
    l64, A64, dA64 = c["lp"].to(F64), c["A"].to(F64), c["dA"].to(F64)
    ref = ref_bwd_s(l64, A64, dA64, c["caps"], HW, T1)
    z = torch.zeros_like(l64)
    a1, Al, dAl = torch.where(live, torch.exp(l64), z), torch.where(live, A64, z), torch.where(live, dA64, z)
    ee = torch.where(live, (2 * l64.abs() + 2) * U, z)
    ca = (Al * dAl).sum(1, keepdim=True)
    e_ca = HW * U * (Al * dAl).abs().sum(1, keepdim=True)
    da1 = T1 * Al * (dAl - ca)
    e_da1 = T1 * Al * (e_ca + 3 * U * (dAl.abs() + ca.abs()))
    rd = (a1 * da1).sum(3, keepdim=True)
    ncap = torch.tensor(c["caps"], dtype=F64)[None, None, :, None]
    e_rd = (a1 * (e_da1 + ee * da1.abs())).sum(3, keepdim=True) + (ncap + 1) * U * (a1 * da1).abs().sum(3, keepdim=True)
    bar = 2.0 ** -8 * ref.abs() + a1 * (e_da1 + e_rd + U * (da1.abs() + rd.abs())) + (ee + U) * ref.abs()
    _check(got, ref, bar, f"bwd_s Tp={Tp} HW={HW}")


def _cos_case(B, Bc, T, Tp, D, Kp, seed):
    """wc fp32 [B, Bc, Tp, D], words bf16 values, wnorm = fp32 of the float64 norm, gsim fp32; all as float64.  den < eps both ways:
    caption 0's word 1 is a row of exact zeros (wnorm 0: den = 0 for every image); its word 2 is short (|w| about 0.03) and image 1's
    wctx row for it has norm 1e-7, so den is about 3e-9 there and ordinary for the other images."""
    g = torch.Generator().manual_seed(seed)
    cap_lens = [T + 9, 0, 1, T, T // 2][:Bc] if Bc > 1 else [T - 2]
    caps = clamp_caps(cap_lens, T, Tp)
    words = (0.2 * torch.randn(Bc, T, D, generator=g)).to(BF).float()
    words[0, 1] = 0.0
    words[0, 2] = (0.03 / math.sqrt(D) * torch.randn(D, generator=g)).to(BF).float()
    wc = 0.2 * torch.randn(B, Bc, Tp, D, generator=g)
    r = torch.randn(D, generator=g)
    wc[1 % B, 0, 2] = 1e-7 * r / r.norm()
    wn = torch.linalg.vector_norm(words.to(F64), dim=-1).float()
    gsim = 0.1 * torch.randn(B, Bc, generator=g)
    return dict(B=B, Bc=Bc, T=T, Tp=Tp, D=D, Kp=Kp, caps=caps, cap=torch.tensor(cap_lens, dtype=I32), wc=wc.to(F64), words=words.to(F64),
                wn=wn.to(F64), gsim=gsim.to(F64), dws=(0.05 * torch.randn(Bc, Tp, D, generator=g)).to(F64))


def _cos_terms(c, for_words=False):
    """closed form of the cosine backward in float64: d wctx = kw w + kc wctx (for_words: d w = sum_b kc_b wctx_b + (sum_b kw_b) w) with
    their magnitudes; the bars take sum|term| from here."""
    T, Tp = c["T"], c["Tp"]
    live = word_mask(c["caps"], Tp)[None]
    w = F.pad(c["words"], (0, 0, 0, Tp - T))[None]
    wn = F.pad(c["wn"], (0, Tp - T))[None]
    v = torch.where(live[..., None], c["wc"], torch.zeros_like(c["wc"]))
    st, sume, _ = ref_cos(c["wc"], c["words"], c["wn"], c["caps"], T2, EPS)
    cos, n2, e = st[..., 0], st[..., 1], st[..., 2]
    den_raw = wn * n2.sqrt()
    dcos = c["gsim"][..., None] * T2 * e / sume[..., None]
    hard = live & (den_raw >= EPS)
    z = torch.zeros_like(cos)
    if for_words:
        kc = torch.where(hard, dcos / den_raw.clamp_min(1e-300), torch.where(live, dcos / EPS, z))
        kw = torch.where(hard, -dcos * cos / (wn * wn).clamp_min(1e-300), z)
    else:
        kw = torch.where(hard, dcos / den_raw.clamp_min(1e-300), torch.where(live, dcos / EPS, z))
        kc = torch.where(hard, -dcos * cos / n2.clamp_min(1e-300), z)
    return dict(kw=kw, kc=kc, w=w.expand_as(v), v=v, den_raw=den_raw, live=live)


def test_closed_forms_of_the_bars_match_autograd():
    """The bars of dwctx / dwords need sum|term| of d wctx = kw w + kc wctx and d w = sum_b kc_b c_b + (sum_b kw_b) w: the closed form those
    come from reproduces the autograd references, den < eps cases included."""
    B, Bc, T, Tp, D = 3, 5, 9, 16, 64
    c = _cos_case(B, Bc, T, Tp, D, Bc * Tp + 40, seed=1)
    t = _cos_terms(c)
    ref = ref_dwctx(c["wc"], c["words"], c["wn"], c["caps"], c["gsim"], T2, EPS)
    assert float((t["kw"][..., None] * t["w"] + t["kc"][..., None] * t["v"] - ref).abs().max()) < 1e-9 * float(ref.abs().max())
    t = _cos_terms(c, for_words=True)
    ref = ref_dwords(c["wc"], c["words"], c["caps"], c["gsim"], None, T2, EPS)
    got = ((t["kc"][..., None] * t["v"]).sum(0) + t["kw"].sum(0)[..., None] * t["w"][0])[:, :T]
    assert float((got - ref).abs().max()) < 1e-7 * float(ref.abs().max())                       # wnorm is an fp32 input here: 2^-24 relative
    assert int((t["den_raw"] < EPS)[:, 0, 1:3].sum()) == B + 1                                   # the zero word in every image, the tiny wctx row in one


def _rows(x, Kp):
    """logical [B, Bc, Tp, C] -> device [B, Kp, C] with sentinels in the rows past Bc*Tp; returns (buffer, the sentinels)"""
    B, Bc, Tp, C = x.shape
    s = _sentinel(B * (Kp - Bc * Tp), C, x.dtype).reshape(B, Kp - Bc * Tp, C)
    return torch.cat([x.reshape(B, Bc * Tp, C), s], dim=1).contiguous().cuda(), s


def _cos_device(c):
    """the device operands of the three cosine kernels; wc's padding rows hold NaN (a read of one shows)"""
    B, Bc, Tp, D, Kp = c["B"], c["Bc"], c["Tp"], c["D"], c["Kp"]
    wc = torch.cat([c["wc"].float().reshape(B, Bc * Tp, D), torch.full((B, Kp - Bc * Tp, D), math.nan)], dim=1).contiguous().cuda()
    return wc, c["words"].to(BF).cuda(), c["wn"].float().cuda(), c["cap"].cuda(), c["gsim"].float().cuda()


COS_CASES = [(T, Tp, D) for T, Tp in ((9, 16), (77, 80)) for D in (64, 100, 768)]


@gpu
@pytest.mark.parametrize("T,Tp,D", COS_CASES)
def test_cos(T, Tp, D):
    """local_gen_cos.  Bars, every sum in float64:
      n2   D u n2;   num  D u sum|wc w|   (fp32 sums of D terms)
      den  max(|w| sqrt(n2), eps) is 1-Lipschitz in the raw product, whose error is raw (D u / 2 + 3 u) (n2 under the root, sqrt, product)
      cos  E_num / den + |cos| E_raw / den + 2 u |cos|
      e    e (2^-20 + temp2 E_cos)          (__expf)
      sume sum_t E_e + cap u sume;   sim  2^-20 + E_sume / sume   (__logf, absolute)
    stats rows t >= cap are exact zeros, lane 3 of every row is zero, the rows Bc*Tp..Kp of stats keep their bits."""
    from medmoe_amd import ops
    B, Bc = 3, 5
    Kp = Bc * Tp + 40
    c = _cos_case(B, Bc, T, Tp, D, Kp, seed=Tp + D)
    wc, words, wn, cap, _ = _cos_device(c)
    stats, sent = _rows(_sentinel(B * Bc * Tp, 4, F32).reshape(B, Bc, Tp, 4), Kp)
    sim, sume = torch.full((B, Bc), math.nan, device="cuda"), torch.full((B, Bc), math.nan, device="cuda")
    ops.call("local_gen_cos", wc, words, wn, cap, sim, stats, sume, B, Bc, T, Tp, D, T2, EPS, Kp)
    torch.cuda.synchronize()
    assert torch.equal(_bits(stats.cpu()[:, Bc * Tp:]), _bits(sent))
    got = stats.cpu()[:, :Bc * Tp].reshape(B, Bc, Tp, 4)
    st, se, sm = ref_cos(c["wc"], c["words"], c["wn"], c["caps"], T2, EPS)
    t = _cos_terms(c)
    dead = ~t["live"].expand(B, Bc, Tp)
    assert torch.equal(got[dead], torch.zeros(int(dead.sum()), 4)) and torch.equal(got[..., 3], torch.zeros(B, Bc, Tp))
    assert int((t["den_raw"] < EPS)[t["live"].expand(B, Bc, Tp)].sum()) == B + 1
    cos, n2, e = st[..., 0], st[..., 1], st[..., 2]
    e_n2 = D * U * n2
    den = t["den_raw"].clamp_min(EPS)
    e_cos = D * U * (t["v"] * t["w"]).abs().sum(-1) / den + cos.abs() * t["den_raw"] * (D * U / 2 + 3 * U) / den + 2 * U * cos.abs()
    e_e = e * (2.0 ** -20 + T2 * e_cos)
    e_sume = e_e.sum(-1) + torch.tensor(c["caps"], dtype=F64)[None] * U * se
    _check(got[..., 0], cos, e_cos, f"cos Tp={Tp} D={D}")
    _check(got[..., 1], n2, e_n2, f"n2 Tp={Tp} D={D}")
    _check(got[..., 2], e, e_e, f"e Tp={Tp} D={D}")
    _check(sume, se, e_sume, f"sume Tp={Tp} D={D}")
    _check(sim, sm, 2.0 ** -20 + e_sume / se, f"sim Tp={Tp} D={D}")


def _stats32(c):
    """the forward's stats / sume as the backward kernels read them: the float64 reference rounded to fp32 (u relative each)"""
    st, se, _ = ref_cos(c["wc"], c["words"], c["wn"], c["caps"], T2, EPS)
    return st.float(), se.float()


@gpu
@pytest.mark.parametrize("T,Tp,D", COS_CASES)
def test_dwctx(T, Tp, D):
    """local_gen_dwctx: d wctx = kw w + kc wctx, bf16.  kw = dcos / den and kc = -dcos cos / n2 take at most 9 fp32 roundings each from
    the fp32 inputs (e, sume, cos, n2, |w|: u each; products, quotients, the root), 12 u allowed; the two products and the sum 4 u more:
      bar = 2^-8 |ref| + 16 u (|kw w| + |kc wctx|)         (absolute in the two terms: they cancel along wctx)
    Rows t >= cap exact zeros; the rows Bc*Tp..Kp of DWC keep their bits; the den < eps rows take kw = dcos / eps, kc = 0."""
    from medmoe_amd import ops
    B, Bc = 3, 5
    Kp = Bc * Tp + 40
    c = _cos_case(B, Bc, T, Tp, D, Kp, seed=Tp + D)
    wc, words, wn, cap, gsim = _cos_device(c)
    st, se = _stats32(c)
    stats, _ = _rows(st.reshape(B, Bc, Tp, 4), Kp)
    dwc, sent = _rows(_sentinel(B * Bc * Tp, D, BF).reshape(B, Bc, Tp, D), Kp)
    ops.call("local_gen_dwctx", wc, words, wn, cap, gsim, stats, se.cuda(), dwc, B, Bc, T, Tp, D, T2, EPS, Kp)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dwc.cpu()[:, Bc * Tp:]), _bits(sent))
    got = dwc.cpu()[:, :Bc * Tp].reshape(B, Bc, Tp, D)
    t = _cos_terms(c)
    dead = ~t["live"].expand(B, Bc, Tp)
    assert torch.equal(got[dead].float(), torch.zeros(int(dead.sum()), D))
    ref = ref_dwctx(c["wc"], c["words"], c["wn"], c["caps"], c["gsim"], T2, EPS)
    bar = 2.0 ** -8 * ref.abs() + 16 * U * ((t["kw"][..., None] * t["w"]).abs() + (t["kc"][..., None] * t["v"]).abs())
    _check(got, ref, bar, f"dwctx Tp={Tp} D={D}")


DW_CASES = [(B, Bc, 9, 16, D) for B, Bc in ((3, 5), (70, 2), (130, 1)) for D in (64, 100, 512, 768, 1024)] + [(3, 5, 77, 80, 64), (3, 5, 77, 80, 1024)]


@gpu
@pytest.mark.parametrize("B,Bc,T,Tp,D", DW_CASES)
def test_dwords(B, Bc, T, Tp, D):
    """local_gen_dwords<NC>, NC 1..4 (D = 100: 25 of 64 lanes), images in one chunk of 64, one full chunk plus six, and three chunks;
    Bc*T = 45 / 18 / 9 / 385 leaves idle waves in the last block; with dWS and with a null dWS.  fp32 output:
      bar = (B + 24) u (|dWS| + sum_b |kc_b wctx_b| + (sum_b |kw_b|) |w|)
    B + 1 additions into the accumulator and one product each (B + 2), kc / kw 12 u as in dwctx, the shuffle sum of kw over 64 lanes and
    up to three chunks (9), the last product.  Words t >= cap exact zeros; a second call gives the same bits (fixed summation order)."""
    from medmoe_amd import ops
    Kp = Bc * Tp + 40
    c = _cos_case(B, Bc, T, Tp, D, Kp, seed=B + D + Tp)
    assert (Bc * T) % 4 != 0
    wc, words, wn, cap, gsim = _cos_device(c)
    st, se = _stats32(c)
    stats, _ = _rows(st.reshape(B, Bc, Tp, 4), Kp)
    se = se.cuda()
    dws = torch.cat([c["dws"].float().reshape(Bc * Tp, D), torch.full((Kp - Bc * Tp, D), math.nan)]).contiguous().cuda()
    t = _cos_terms(c, for_words=True)
    mag = ((t["kc"][..., None] * t["v"]).abs().sum(0) + t["kw"].abs().sum(0)[..., None] * t["w"][0].abs())[:, :T]
    dead = ~word_mask(c["caps"], T)
    assert int((t["den_raw"] < EPS)[:, 0, 1:3].sum()) == B + 1
    for given in (dws, None):
        out = [torch.full((Bc, T, D), math.nan, device="cuda") for _ in range(2)]
        for o in out:
            ops.call("local_gen_dwords", wc, words, wn, cap, gsim, stats, se, given, o, B, Bc, T, Tp, D, T2, EPS, Kp)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[0]), _bits(out[1]))
        got = out[0].cpu()
        assert torch.equal(got[dead], torch.zeros(int(dead.sum()), D))
        d64 = c["dws"] if given is not None else None
        ref = ref_dwords(c["wc"], c["words"], c["caps"], c["gsim"], d64, T2, EPS)
        bar = (B + 24) * U * (mag + (c["dws"][:, :T].abs() if given is not None else 0.0))
        _check(got, ref, bar, f"dwords B={B} Bc={Bc} Tp={Tp} D={D} dWS={'yes' if given is not None else 'null'}")


@gpu
@pytest.mark.parametrize("B,HW,HWp,D", [(2, 37, 48, 64), (3, 49, 64, 100), (1, 576, 576, 768)])
def test_unpad_cast(B, HW, HWp, D):
    """medmoe_unpad_cast / unpad_cast2: the row gather and ONE bf16 rounding of src, of src + src2 (summed in fp32) - bit-equal to the
    reference.  The padded source rows hold NaN: a read of one shows."""
    from medmoe_amd import ops
    g = torch.Generator().manual_seed(HW)
    src, src2 = torch.randn(B, HWp, D, generator=g), torch.randn(B, HWp, D, generator=g) * 0.37
    src[:, HW:], src2[:, HW:] = math.nan, math.nan
    a, b = torch.zeros(B, HW, D, dtype=BF, device="cuda"), torch.zeros(B, HW, D, dtype=BF, device="cuda")
    ops.call("unpad_cast", src.cuda(), a, B, HW, HWp, D)
    ops.call("unpad_cast2", src.cuda(), src2.cuda(), b, B, HW, HWp, D)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.cpu()), _bits(ref_unpad_cast(src, HW)))
    assert torch.equal(_bits(b.cpu()), _bits(ref_unpad_cast(src, HW, src2)))


@gpu
def test_rejections():
    """Shapes outside the contract come back as the argument / shape error of ops.call and leave the output as it was: Tp = 96, Tp = 24,
    ldp % 8, ldp < Bc*Tp, HWp < HW, Kp < Bc*Tp, and for dwords D % 4 and D = 1028.  Each case breaks exactly one condition of its entry point
    (the buffers, ldp and Kp hold Bc * 96 columns, so Tp = 96 fails on Tp > 80 alone - the guard that keeps the kernels' 80-word LDS rows in bounds)."""
    from medmoe_amd import ops
    B, Bc, HW, HWp, T, Tp, D = 2, 2, 20, 32, 9, 16, 64
    ldp = Kp = 256                                             # >= Bc * 96: at Tp = 96 nothing but Tp > 80 is out of contract
    dev = "cuda"
    lp = torch.zeros(B * HWp, ldp, dtype=F16, device=dev)
    A = torch.zeros(B * HWp, ldp, dtype=BF, device=dev)
    cap = torch.tensor([T, 3], dtype=I32, device=dev)
    wc = torch.zeros(B, Kp, 1028, device=dev)
    words, wn = torch.zeros(Bc, 96, 1028, dtype=BF, device=dev), torch.ones(Bc, 96, device=dev)
    gsim, sume, stats = torch.ones(B, Bc, device=dev), torch.ones(B, Bc, device=dev), torch.zeros(B, Kp, 4, device=dev)
    f32 = torch.zeros(B, HWp, D, device=dev)

    def refused(name, out, *args):
        before = _bits(out).clone()
        with pytest.raises(RuntimeError, match=r"failed with code -[12]"):
            ops.call(name, *args)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), before), name

    pair_bad = [dict(Tp=96, T=90), dict(Tp=24, T=20), dict(ldp=ldp - 4), dict(ldp=Bc * Tp - 8), dict(HWp=HW - 4)]
    for bad in pair_bad:
        k = dict(dict(HW=HW, HWp=HWp, T=T, Tp=Tp, ldp=ldp), **bad)
        out = _sentinel(B * HWp, ldp, BF).cuda()
        refused("local_gen_fwd_a", out, lp, cap, out, B, Bc, k["HW"], k["HWp"], k["T"], k["Tp"], T1, k["ldp"])
        refused("local_gen_bwd_s", out, lp, A, out, cap, B, Bc, k["HW"], k["HWp"], k["T"], k["Tp"], T1, k["ldp"])
    for bad in (dict(Tp=96, T=90), dict(Kp=Bc * Tp - 1)):
        k = dict(dict(T=T, Tp=Tp, Kp=Kp, D=D), **bad)
        tail = (B, Bc, k["T"], k["Tp"], k["D"], T2, EPS, k["Kp"])
        out = _sentinel(B * Kp, 4, F32).cuda()
        refused("local_gen_cos", out, wc, words, wn, cap, torch.zeros(B, Bc, device=dev), out, sume, *tail)
        out = _sentinel(B * Kp, 1028, BF).cuda()
        refused("local_gen_dwctx", out, wc, words, wn, cap, gsim, stats, sume, out, *tail)
    for bad in (dict(Tp=96, T=90), dict(Kp=Bc * Tp - 1), dict(D=66), dict(D=1028)):
        k = dict(dict(T=T, Tp=Tp, Kp=Kp, D=D), **bad)
        out = _sentinel(Bc * 96, 1028, F32).cuda()
        refused("local_gen_dwords", out, wc, words, wn, cap, gsim, stats, sume, None, out, B, Bc, k["T"], k["Tp"], k["D"], T2, EPS, k["Kp"])
    out = _sentinel(B * HW, D, BF).cuda()
    refused("unpad_cast", out, f32, out, B, HW, HW - 4, D)
    refused("unpad_cast2", out, f32, f32, out, B, HW, HW - 4, D)


# ---------------------------------------------------------------------------------------------
# 4. the whole object at every Tp class, judged per block
# ---------------------------------------------------------------------------------------------
OBJ_CASES = [(T, HW) for T in (9, 25, 40, 60, 77) for HW in (48, 40)]
OBJ_D = 128
CAP_DWORDS, CAP_DCTX = 2e-2, 6e-2                              # the project's whole-tensor bars: no block bar is looser


def _obj_inputs(T, HW):
    B = 8 if T <= 16 else 4
    g = torch.Generator().manual_seed(1000 * T + HW)
    ctx = (0.2 * torch.randn(B, HW, OBJ_D, generator=g)).to(BF)
    words = (0.2 * torch.randn(B, T, OBJ_D, generator=g)).to(BF)
    caps = [T, 1, max(2, T // 2), max(2, T // 3), T, max(3, (2 * T) // 3), 1, max(2, T // 4)][:B]
    return B, ctx, words, caps


def _blocks(x, ref, caps):
    """sim: |x - ref| per element; d ctx: relative L2 per image; d words: relative L2 per (caption, 8-word piece) over its live words"""
    out = dict(sim=(x["sim"] - ref["sim"]).abs().reshape(-1))
    out["dctx"] = torch.linalg.vector_norm(x["dctx"] - ref["dctx"], dim=(1, 2)) / torch.linalg.vector_norm(ref["dctx"], dim=(1, 2))
    dw = []
    for i, c in enumerate(caps):
        for t0 in range(0, c, 8):
            a, b = x["dwords"][i, t0:min(t0 + 8, c)], ref["dwords"][i, t0:min(t0 + 8, c)]
            dw.append(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))
    out["dwords"] = torch.stack(dw)
    return out


_MODEL = {}


def _model(T, HW):
    """the exact float64 chain, and the worst block distance of the stored-format chain from it, per block kind (computed once per geometry)"""
    if (T, HW) not in _MODEL:
        B, ctx, words, caps = _obj_inputs(T, HW)
        exact = chain(ctx.to(F64), words.to(F64), caps)
        stored = chain(ctx.to(F64), words.to(F64), caps, stored=True)
        _MODEL[(T, HW)] = (exact, {k: float(v.max()) for k, v in _blocks(stored, exact, exact["caps"]).items()})
    return _MODEL[(T, HW)]


def _bars(dist):
    return dict(sim=3 * dist["sim"], dctx=min(3 * dist["dctx"], CAP_DCTX), dwords=min(3 * dist["dwords"], CAP_DWORDS))


@pytest.mark.parametrize("T,HW", OBJ_CASES)
def test_storage_model_distances(T, HW):
    """What lp in fp16 and A, DWC, dA, dS, d ctx in bf16 cost, per block kind: the worst block of the stored-format float64 chain against
    the exact one.  Three times these numbers are the bars of test_whole_object (fp32 summation order and the atomics are the margin).
    Recorded (worst block; sim absolute, d ctx per image and d words per 8-word piece relative L2), HW = 48 / 40:
      T =  9   sim 4.99e-4 / 8.13e-4   d ctx 3.43e-3 / 3.22e-3   d words 2.29e-3 / 2.27e-3
      T = 25   sim 6.48e-4 / 5.62e-4   d ctx 4.96e-3 / 3.21e-3   d words 2.22e-3 / 2.46e-3
      T = 40   sim 6.32e-4 / 3.77e-4   d ctx 2.96e-3 / 3.04e-3   d words 2.34e-3 / 2.02e-3
      T = 60   sim 2.43e-4 / 4.01e-4   d ctx 3.05e-3 / 3.01e-3   d words 2.13e-3 / 1.77e-3
      T = 77   sim 1.74e-4 / 1.96e-4   d ctx 3.27e-3 / 2.91e-3   d words 2.22e-3 / 1.81e-3
    The model must stay a real bar: every distance is positive, and three times it is already inside the whole-tensor bars."""
    _, dist = _model(T, HW)
    print(f"T={T} HW={HW}: modelled distance " + "  ".join(f"{k} {v:.2e}" for k, v in dist.items()))
    assert 0 < dist["sim"] < 1e-2 and 0 < 3 * dist["dctx"] < CAP_DCTX and 0 < 3 * dist["dwords"] < CAP_DWORDS


@gpu
@pytest.mark.parametrize("T,HW", OBJ_CASES)
def test_whole_object(T, HW):
    """GenericLocalLoss(word_grad=True), forward and backward, against the exact float64 chain at the same bf16 inputs, gsim from the row and
    column cross entropy of 10 * sim on either side.  Judged per block - sim per element, d ctx per image, d words per (caption, 8-word
    piece), words t >= cap exactly zero - against three times the modelled storage distance of test_storage_model_distances (its
    docstring records them), never looser than 2e-2 (d words) / 6e-2 (d ctx)."""
    from medmoe_amd.local_generic import GenericLocalLoss
    B, ctx, words, caps = _obj_inputs(T, HW)
    exact, dist = _model(T, HW)
    bars = _bars(dist)
    loss = GenericLocalLoss(B, HW, T, OBJ_D, "cuda", word_grad=True)
    assert loss.dense == (HW == 48) and loss.Tp == (T + 15) // 16 * 16 and (loss.Kp >= 128)
    cap = torch.tensor(caps, dtype=I32, device="cuda")
    sim = loss.forward(ctx.reshape(B * HW, OBJ_D).cuda(), words.cuda(), cap, T1, T2).clone()
    dctx, dwords = loss.backward(ce_gsim(sim).contiguous())
    torch.cuda.synchronize()
    got = dict(sim=sim.cpu().to(F64), dctx=dctx.cpu().to(F64).reshape(B, HW, OBJ_D), dwords=dwords.cpu().to(F64))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    for i, c in enumerate(caps):
        assert torch.equal(dwords[i, c:].cpu(), torch.zeros(T - c, OBJ_D))
    worst = {k: float(v.max()) for k, v in _blocks(got, exact, caps).items()}
    print(f"T={T} HW={HW} dense={loss.dense}: " + "  ".join(f"{k} {worst[k]:.2e} (model {dist[k]:.2e}, bar {bars[k]:.2e})" for k in worst))
    for k in worst:
        assert worst[k] <= bars[k], (k, worst[k], dist[k], bars[k])
