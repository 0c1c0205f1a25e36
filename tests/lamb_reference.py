"""Host restatement of the LAMB step the LAMB tests share, in float64 torch, written from the formulas and independent of
src/optim.py and of the kernels.  Not a test module.

    g'  = g * (grad_scale * c)                       c = min(1, clip / (sqrt(normsq) * grad_scale + 1e-6)), 1 without a clip; grad_scale * c is
                                                     formed in fp32 as the Adam launches form it: an fp32 input of the step (device_coef)
    m   = b1 m + (1 - b1) g'
    v   = b2 v + (1 - b2) g' g'
    a   = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps)    bc1 = 1 - b1^t, bc2 = 1 - b2^t
    u   = a + (wd wd_mult) p
    per segment: wn = |p|, un = |u|;  r = wn / un if wn > 0 and un > 0 and (always_adapt or wd wd_mult != 0) else 1;  min(r, 1) with trust_clip
    p   = p - (lr lr_mult) r u
"""
import math

import torch

F64 = torch.float64
U24 = 2.0 ** -24


def clip_coef(normsq: float, clip: float, grad_scale: float = 1.0) -> float:
    """grad_scale times the clip coefficient in float64 (clip <= 0: no clipping).  The launches form it in fp32 as the Adam launches do (a square
    root, a product, a sum, a division: at most one unit in the last place each, COEF_BAR in all) and keep what they used
    (FlatArena.last_clip_coef): the tests hand THAT value to the restatement as the fp32 input it is, and hold it against this one."""
    if clip is None or clip <= 0.0:
        return float(grad_scale)
    return float(grad_scale) * min(1.0, clip / (math.sqrt(normsq) * grad_scale + 1e-6))


COEF_BAR = 4 * 2 * U24                                               # four fp32 operations, one ulp (2 * 2^-24 relative) each


def device_coef(st, normsq: float, clip: float, grad_scale: float = 1.0, label: str = "") -> float:
    """The coefficient the arena's last lamb_step used, checked against the float64 formula."""
    got, want = float(st.last_clip_coef()), clip_coef(normsq, clip, grad_scale)
    print(f"[bar] {label} clip coefficient: device {got:.9e}, float64 {want:.9e}, rel err {abs(got - want) / want:.3e} <= {COEF_BAR:.3e}")
    assert abs(got - want) <= COEF_BAR * want
    return got


def lamb_tensor(p, g, m, v, t, *, lr, wd, betas=(0.9, 0.999), eps=1e-6, coef=1.0, always_adapt=False, trust_clip=False):
    """One step of ONE parameter tensor (any shape), float64.  Returns a dict: p (new), m, v, a, u, wn2, un2, r."""
    p, g, m, v = (x.to(F64) for x in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    gs = g * coef
    m = b1 * m + (1.0 - b1) * gs
    v = b2 * v + (1.0 - b2) * gs * gs
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    a = (m / bc1) / (v.sqrt() / math.sqrt(bc2) + eps)
    u = a + wd * p
    wn2, un2 = float((p * p).sum()), float((u * u).sum())
    r = 1.0
    if wn2 > 0.0 and un2 > 0.0 and (always_adapt or wd != 0.0):
        r = math.sqrt(wn2) / math.sqrt(un2)
    if trust_clip:
        r = min(r, 1.0)
    return {"p": p - (lr * r) * u, "m": m, "v": v, "a": a, "u": u, "wn2": wn2, "un2": un2, "r": r}


def lamb_arena(p, g, m, v, t, seg_ends, seg_lr, seg_wd, *, lr, wd, betas=(0.9, 0.999), eps=1e-6, coef=1.0, always_adapt=False,
               trust_clip=False):
    """One step of a flat arena cut into segments [seg_ends[k - 1], seg_ends[k]) with multipliers (seg_lr[k], seg_wd[k]); the multipliers are
    taken as the fp32 values the device tables hold.  Returns flat float64 p, m, v, a, u, step (the per-element lr lr_mult r) and the
    per-segment lists wn2, un2, r."""
    n = p.numel()
    out = {k: torch.zeros(n, dtype=F64) for k in ("p", "m", "v", "a", "u", "step", "wdp")}
    wn2, un2, rs = [], [], []
    lo = 0
    for hi, lm, wm in zip(seg_ends, seg_lr, seg_wd):
        wds = float(torch.tensor(wd, dtype=torch.float32) * torch.tensor(wm, dtype=torch.float32))      # the kernel's fp32 product wd * wd_mult
        one = lamb_tensor(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], t, lr=lr * lm, wd=wds, betas=betas, eps=eps, coef=coef,
                          always_adapt=always_adapt, trust_clip=trust_clip)
        for k in ("p", "m", "v", "a", "u"):
            out[k][lo:hi] = one[k]
        out["step"][lo:hi] = lr * lm * one["r"]
        out["wdp"][lo:hi] = wds * p[lo:hi].to(F64)
        wn2.append(one["wn2"]); un2.append(one["un2"]); rs.append(one["r"])
        lo = hi
    out.update(wn2=wn2, un2=un2, r=rs)
    return out


def sum_bar(K: int, D: int) -> float:
    """Relative error bound of a sum of non-negative fp32 terms whose longest chain of additions is K sequential ones followed by D tree /
    record-walk levels: (K + D + 4) 2^-24 - the 4 covers the rounding of the squares and of the final store."""
    return (K + D + 4) * U24
