"""Float64 restatements of the tiled local-loss kernels' contracts (the header comments of loss.hip "local_scores" / "local_pair2",
gemm_scores.hip "scores512" and pair3.hip), one function per contract, shared by test_local_tiled_reference_host.py (which proves their
chain against the oracle) and test_local_tiled_kernels_gpu.py (which judges every kernel instance against them).

Logical shapes (the device layouts are the tests' business): pair tensors [B, HW, n, TP] = (image, region, caption of the launch, word of
its 16*ntt columns); per-word vectors [B, n, TP]; lse [B, HW, n]; Gm [B, HW, HW]; wn [n, TP].  Everything follows the device of its inputs.

The references are STAGED: a kernel that rounds an intermediate it also outputs (A, bf16) is judged on that output alone, and the later
stages start from the kernel's own rounded output (`A_stored`), so their bars stay those of the fp32 scalar chain.  A, the word mask and
the caption clamp are the ones of test_local_generic_kernels_gpu.py (one copy).  The word-softmax backward is NOT its ref_bwd_s: the tiled
kernels take cA = sum_hw A dA in closed form, dn num + d2 n2, with num from the unrounded A and n2 from the bf16 A - that equals the sum
ref_bwd_s forms only without the bf16 rounding (the host test asserts exactly that)."""
import math

import torch
import torch.nn.functional as F

from test_local_generic_kernels_gpu import ce_gsim, clamp_caps, ref_bwd_s, ref_fwd_a, word_mask  # noqa: F401  (re-exported)

F64 = torch.float64
LOGP_MIN = -60000.0                                            # common.h: the fp16 value on masked words
LOGP_MIN_BITS = 0xFB53 - 0x10000                               # its bit pattern as an int16
LN2 = math.log(2.0)


def live_words(caps, TP, device=None):
    return (torch.arange(TP, device=device)[None, :] < torch.as_tensor(caps, device=device)[:, None])          # [n, TP]


def ref_scores(ctx, words, caps, TP, log2=False):
    """The score GEMM with the word softmax fused.  ctx [B, HW, D], words [n, T, D] (the launch's captions in list order), caps the CLAMPED
    lengths (1 <= cap <= min(T, TP): an empty caption counts as its first word).  S = ctx . w; lse = log sum_{t < cap} exp S;
    lp = S - lse (log2: divided by ln 2, the transposed form), clamped below at LOGP_MIN, LOGP_MIN on every word t >= cap.
    Also returns what the bars are counted from: sabs = sum_d |ctx w|, p = the softmax, x = S - max."""
    n, T, D = words.shape
    w = F.pad(words, (0, 0, 0, max(0, TP - T)))[:, :TP]
    S = torch.einsum("bhd,ntd->bhnt", ctx, w)
    sabs = torch.einsum("bhd,ntd->bhnt", ctx.abs(), w.abs())
    live = live_words(caps, TP, ctx.device)[None, None]
    Sm = S.masked_fill(~live, -math.inf)
    mx = Sm.amax(-1, keepdim=True)
    lse = torch.logsumexp(Sm, dim=-1)
    lp = Sm - lse[..., None]
    p = torch.exp(lp)
    if log2:
        lp = lp / LN2
    lp = torch.where(live, lp.clamp_min(LOGP_MIN), torch.full_like(lp, LOGP_MIN))
    return dict(S=S, sabs=sabs, live=live.expand_as(S), lse=lse, lp=lp, p=p, x=torch.where(live, Sm - mx, torch.zeros_like(S)), mx=mx[..., 0])


def ref_pair_fwd(lp, lse, Gm, wn, caps, temp1, temp2, eps, A_stored=None, num_stored=False):
    """Everything after the word softmax, forward.  lp [B, HW, n, TP] NATURAL log-probabilities (LOGP_MIN or anything on masked words: they
    are not used), lse [B, HW, n], Gm [B, HW, HW], wn [n, TP] word norms.  a1 = exp(lp); A = softmax over the regions of temp1 a1;
    num_t = sum_hw A (lp + lse) with the UNROUNDED A; n2_t = a_t^T Gm a_t with the STORED A (A_stored: the kernel's bf16 output; None: A);
    cos = num / max(|w| sqrt(max(n2, 0)), eps); e = exp(temp2 cos) for t < cap; sim = log sum_t e.  Words t >= cap: zeros everywhere.
    num_stored: num from the STORED A as well - local_pair_kernel, which keeps only the rounded A."""
    B, HW, n, TP = lp.shape
    live = live_words(caps, TP, lp.device)[None]                                                   # [1, n, TP]
    z = torch.zeros_like(lp)
    A = ref_fwd_a(lp.cpu(), list(caps), HW, temp1).to(lp.device)
    Ab = A if A_stored is None else torch.where(live[:, None], A_stored, z)
    S = torch.where(live[:, None], lp + lse[..., None], z)
    a1 = torch.where(live[:, None], torch.exp(lp), z)
    An = Ab if num_stored else A
    num = (An * S).sum(1)
    y = torch.einsum("bhk,bknt->bhnt", Gm, Ab)
    n2 = (Ab * y).sum(1)
    n2c = n2.clamp_min(0.0)
    den = wn[None] * n2c.sqrt()
    cos = torch.where(live, num / den.clamp_min(eps), torch.zeros_like(num))
    e = torch.where(live, torch.exp(temp2 * cos), torch.zeros_like(cos))
    sume = e.sum(-1)
    return dict(A=A, Ab=Ab, S=S, a1=a1, y=y, num=num, n2=n2, den=den, cos=cos, e=e, sume=sume, sim=torch.log(sume), live=live,
                numabs=(An * S).abs().sum(1), n2abs=torch.einsum("bhnt,bhk,bknt->bnt", Ab.abs(), Gm.abs(), Ab.abs()),
                yabs=torch.einsum("bhk,bknt->bhnt", Gm.abs(), Ab.abs()))


def ref_pair_bwd(f, wn, gsim, temp1, temp2, eps):
    """The gradients of sum gsim * sim with respect to the scores, from ref_pair_fwd's dict f (gsim [B, n]; None: ones).
      dcos = gsim temp2 e / sum e;  den >= eps: dn = dcos / den, d2 = -dcos cos / max(n2, 1e-30);  den < eps: dn = dcos / eps, d2 = 0
      cA = dn num + d2 n2;  dA = dn S + d2 (Gm A);  da1 = temp1 A (dA - cA);  rd = sum_t a1 da1;  dS = dn A + a1 (da1 - rd);  U = d2 A
    with the stored A throughout (d2 = 2 d loss / d n2, so U A^T is the gradient of the Gram matrix's symmetric use).  dwn = -dcos cos / |w|^2
    is the coefficient of w_t that comes from the word's own norm (for the chain's word gradient; the kernels here do not emit it)."""
    live, A = f["live"], f["Ab"]
    gs = torch.ones_like(f["sim"]) if gsim is None else gsim
    zero = torch.zeros_like(f["cos"])
    dcos = torch.where(live, gs[..., None] * temp2 * f["e"] / f["sume"][..., None], zero)
    hard = f["den"] >= eps
    n2c = f["n2"].clamp_min(0.0)
    dn = torch.where(hard, dcos / f["den"].clamp_min(1e-300), dcos / eps)
    d2 = torch.where(hard, -dcos * f["cos"] / n2c.clamp_min(1e-30), zero)
    dwn = torch.where(hard, -dcos * f["cos"] / (wn * wn)[None].clamp_min(1e-300), zero)
    ca = dn * f["num"] + d2 * f["n2"]
    dA = dn[:, None] * f["S"] + d2[:, None] * f["y"]
    da1 = temp1 * A * (dA - ca[:, None])
    rd = (f["a1"] * da1).sum(-1, keepdim=True)
    dS = dn[:, None] * A + f["a1"] * (da1 - rd)
    return dict(dcos=dcos, dn=dn, d2=d2, dwn=dwn, ca=ca, dA=dA, da1=da1, rd=rd, dS=dS, U=d2[:, None] * A)


def qh(x):
    return x.to(torch.float16).to(F64)


def qb(x):
    return x.to(torch.bfloat16).to(F64)


def chain(ctx, words, cap_lens, temp1=4.0, temp2=5.0, eps=1e-8, stored=False, gsim=None):
    """scores -> pair forward -> pair backward, the three follow-up GEMMs as float64 matmuls: ctx [B, HW, D], words [B, T, D] (square: image
    b matches caption b) -> sim, d ctx, d words of CE rows + CE columns of 10 * sim (or of sum gsim * sim).  stored=True rounds lp to
    fp16 and A to bf16 as the kernels store them."""
    B, HW, D = ctx.shape
    n, T, _ = words.shape
    TP = (T + 15) // 16 * 16
    caps = clamp_caps(cap_lens, T, TP)
    sc = ref_scores(ctx, words, torch.tensor(caps), TP)
    lp = qh(sc["lp"]) if stored else sc["lp"]
    wn = F.pad(torch.linalg.vector_norm(words, dim=-1), (0, TP - T), value=1.0)
    Gm = torch.einsum("bhd,bkd->bhk", ctx, ctx)
    f = ref_pair_fwd(lp, sc["lse"], Gm, wn, caps, temp1, temp2, eps)
    if stored:
        f = ref_pair_fwd(lp, sc["lse"], Gm, wn, caps, temp1, temp2, eps, A_stored=qb(f["A"]))
    g = ce_gsim(f["sim"]) if gsim is None else gsim
    bw = ref_pair_bwd(f, wn, g, temp1, temp2, eps)
    wp = F.pad(words, (0, 0, 0, TP - T))
    wctx = torch.einsum("bhnt,bhd->bntd", f["Ab"], ctx)
    dctx = torch.einsum("bhnt,ntd->bhd", bw["dS"], wp) + torch.einsum("bhnt,bntd->bhd", bw["U"], wctx)
    dwords = (torch.einsum("bhnt,bhd->ntd", bw["dS"], ctx) + bw["dwn"].sum(0)[..., None] * wp)[:, :T]
    return dict(sim=f["sim"], dctx=dctx, dwords=dwords, caps=caps, fwd=f, bwd=bw, lp=lp)
