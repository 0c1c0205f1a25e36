"""Direct parity tests of the MoE and token glue kernels (moe.hip, embed.hip) at full width, each called through
medmoe_amd.ops.call exactly as the engine calls it, against a float64 torch restatement of the same operation on the same
bf16-rounded inputs (backward kernels: float64 autograd of the forward restatement).

Bars are elementwise.  Where the kernel's order of fp32 operations can be restated, the comparison is exact (torch.equal).
Otherwise an element passes when |got - ref| <= c_r |ref| + c_a sum|terms|:
  c_r = 2^-8 (one bf16 rounding) for bf16 outputs, 0 for fp32 outputs;
  sum|terms| = the float64 sum of the absolute values of the products behind that element;
  c_a = u * (the longest chain of fp32 roundings that element goes through), u = 2^-24, counted per test below.
Every test prints the worst observed |got - ref| / bar per output ("[bar] ...", run with -s).

Every output buffer carries a tail of TAIL sentinel elements that must stay untouched; accumulating outputs are pre-filled with
non-zero values and checked as prior + delta.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
U = 2.0 ** -24                  # fp32 unit roundoff
UBF = 2.0 ** -8                 # one bf16 rounding (RNE, 8 significant bits)
TAIL = 256
SENT = {BF: 0x7FC1, F32: 0x7FC00001, I32: 0x7A5A5A5A}
_BITS = {BF: torch.int16, F32: torch.int32, I32: torch.int32}
SA_WAVES = 16                   # waves per workgroup of scale_attn_bwd_kernel (moe.hip)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------------
def guarded(shape, dtype, init=None):
    """(flat buffer with a sentinel tail, view of the first prod(shape) elements).  init: values of the body (else sentinel too)."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), SENT[dtype], dtype=_BITS[dtype], device=DEV).view(dtype)
    body = buf[:n].view(shape)
    if init is not None:
        body.copy_(init)
    return buf, body


def sentinel_ok(t):
    bits = t.reshape(-1).view(_BITS[t.dtype])
    return bool((bits == SENT[t.dtype]).all().item())


def tail_ok(buf, n):
    return sentinel_ok(buf[n:])


def check(name, got, ref, terms, c_r, c_a):
    """|got - ref| <= c_r |ref| + c_a terms elementwise (all float64 on the GPU); prints and returns the worst ratio."""
    got = got.to(F64)
    err = (got - ref).abs()
    bar = c_r * ref.abs() + c_a * terms
    ratio = torch.where(bar > 0, err / torch.where(bar > 0, bar, torch.ones_like(bar)),
                        torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    worst = ratio.max().item()
    print(f"[bar] {name}: worst |err|/bar = {worst:.3g}  (c_r = {c_r:.3g}, c_a = {c_a:.3g})")
    if not worst <= 1.0:
        i = int(torch.argmax(ratio.reshape(-1)).item())
        raise AssertionError(f"{name}: element {i} got {got.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r} "
                             f"bar {bar.reshape(-1)[i].item()!r} (worst ratio {worst:.3g})")
    return worst


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV)


def fma32(a, b, c):
    """fp32 RNE(a * b + c) with one rounding (v_fma_f32), restated in float64: a * b is exact in float64, the sum's rounding error comes
    from TwoSum and settles the one case where rounding the float64 sum to fp32 would round twice (a float64 sum exactly halfway)."""
    p = a.to(F64) * b.to(F64)
    c = c.to(F64)
    r = p + c
    bb = r - p
    e = (p - (r - bb)) + (c - bb)
    r32 = r.to(F32)
    d = r - r32.to(F64)
    other = torch.nextafter(r32, torch.where(d > 0, torch.full_like(r32, math.inf), torch.full_like(r32, -math.inf)))
    mid = (d != 0) & ((other.to(F64) - r) == d)
    return torch.where(mid & (e * d > 0), other, r32)


def f32_div(a, n):
    """fp32 a / n correctly rounded (the float64 quotient of two fp32 values rounds to the correctly rounded fp32 one)."""
    return (a.to(F64) / float(np.float32(n))).to(F32)


# ------------------------------------------------------------------------------------------------------------------------------
# dispatch
# ------------------------------------------------------------------------------------------------------------------------------
def host_dispatch(idx, k, E, P, Nt, max_tiles):
    """Python restatement: stable sort of the items (b, j) by expert, tile tables, rowmap."""
    n = idx.size
    item_of_slot = np.argsort(idx, kind="stable").astype(np.int64)
    slot_of = np.empty(n, np.int64)
    slot_of[item_of_slot] = np.arange(n)
    expert_of_slot = idx[item_of_slot]
    counts = np.bincount(idx, minlength=E)
    off = np.concatenate([[0], np.cumsum(counts)])
    t128, t256 = [], []
    for e in range(E):
        r0, r1 = off[e] * P, off[e + 1] * P
        t128 += [(e, r0 + t * 128, r1, 0) for t in range((r1 - r0 + 127) // 128)]
        t256 += [(e, r0 + t * 256, r1, 0) for t in range((r1 - r0 + 255) // 256)]
    assert len(t128) <= max_tiles and len(t256) <= max_tiles
    rowmap = ((item_of_slot // k)[:, None] * Nt + 1 + np.arange(P)[None, :]).reshape(-1)
    return dict(slot_of=slot_of, item_of_slot=item_of_slot, expert_of_slot=expert_of_slot, row_off=off * P,
                t128=np.array(t128, np.int64).reshape(-1, 4), t256=np.array(t256, np.int64).reshape(-1, 4), rowmap=rowmap)


def make_idx(gen, B, k, E, mode):
    """top-k expert indices [B*k]: distinct experts per sample ("random"), all on one expert ("one"; k = 1), or random over a subset
    that leaves the first, a middle and the last expert empty ("holes")."""
    if mode == "one":
        return np.full(B * k, E - 1, np.int64)
    pool = np.arange(E) if mode == "random" else np.array([e for e in range(E) if e not in (0, E // 2, E - 1)])
    if len(pool) < k:
        pool = np.arange(E)
    keys = torch.rand(B, len(pool), generator=gen)
    return pool[keys.argsort(dim=1)[:, :k].numpy()].reshape(-1).astype(np.int64)


def run_dispatch(ops, idx_np, B, k, E, P, Nt, max_tiles):
    n, R = B * k, B * k * P
    idx = torch.from_numpy(idx_np).to(DEV, I32)
    bufs = {nm: guarded((sz,), I32) for nm, sz in
            (("slot_of", n), ("item_of_slot", n), ("expert_of_slot", n), ("row_off", E + 1), ("tiles", 2 * max_tiles * 4),
             ("tile_count", 2), ("rowmap", R))}
    v = {nm: b[1] for nm, b in bufs.items()}
    ops.call("dispatch", idx, B, k, E, P, Nt, v["slot_of"], v["item_of_slot"], v["expert_of_slot"], v["row_off"], v["tiles"],
             v["tile_count"], max_tiles, v["rowmap"])
    torch.cuda.synchronize()
    return bufs, v


@pytest.mark.parametrize("mode", ["random", "one", "holes"])
@pytest.mark.parametrize("B,k,E,P", [(1, 1, 1, 196), (255, 1, 8, 196), (128, 2, 8, 196), (257, 1, 8, 16), (1024, 2, 8, 196),
                                     (256, 8, 16, 256), (65535, 1, 64, 1)])
def test_dispatch_matches_stable_sort(ops, B, k, E, P, mode):
    """Every integer output exact against a Python stable sort; both tile tables; entries past the counts untouched."""
    if mode == "one" and k > 1:
        k, B = 1, B * k
    gen = torch.Generator().manual_seed(B * 131 + E * 7 + P + k)
    idx_np = make_idx(gen, B, k, E, mode)
    R = B * k * P
    Nt = P + 1 if P != 16 else P + 3            # one case with Nt > P + 1: rowmap must use Nt, not P + 1
    engine_mt = (R + 127) // 128 + E
    for max_tiles in (engine_mt, engine_mt + 37):
        ref = host_dispatch(idx_np, k, E, P, Nt, max_tiles)
        bufs, v = run_dispatch(ops, idx_np, B, k, E, P, Nt, max_tiles)
        for nm in ("slot_of", "item_of_slot", "expert_of_slot", "row_off", "rowmap"):
            assert np.array_equal(v[nm].cpu().numpy(), ref[nm]), (nm, max_tiles)
        n128, n256 = len(ref["t128"]), len(ref["t256"])
        assert v["tile_count"].cpu().tolist() == [n128, n256]
        tiles = v["tiles"].view(2 * max_tiles, 4)
        assert np.array_equal(tiles[:n128].cpu().numpy(), ref["t128"])
        assert np.array_equal(tiles[max_tiles:max_tiles + n256].cpu().numpy(), ref["t256"])
        assert sentinel_ok(tiles[n128:max_tiles]) and sentinel_ok(tiles[max_tiles + n256:]), "tile entries past the counts written"
        for nm, (buf, body) in bufs.items():
            assert tail_ok(buf, body.numel()), nm


# ------------------------------------------------------------------------------------------------------------------------------
# scale_attn_fwd + combine_fwd
# ------------------------------------------------------------------------------------------------------------------------------
def moe_tables(ops, gen, B, k, E, P):
    idx_np = make_idx(gen, B, k, E, "random")
    R = B * k * P
    mt = (R + 127) // 128 + E
    _, v = run_dispatch(ops, idx_np, B, k, E, P, P + 1, mt)
    return idx_np, v


def scale_logits64(H1, w2, b2, e_row):
    """a[s, r] = H1[s, r] . w2[e(r)] + b2[e(r)] in float64, and the float64 sum |H1 . w2| + |b2| behind it."""
    H64, w64 = H1.to(F64), w2.to(F64)[e_row]
    a = torch.einsum("srd,rd->sr", H64, w64) + b2.to(F64)[e_row][None]
    s = torch.einsum("srd,rd->sr", H64.abs(), w64.abs()) + b2.to(F64).abs()[e_row][None]
    return a, s


@pytest.mark.parametrize("Do,Dh", [(768, 384), (1024, 512), (8, 8)])
@pytest.mark.parametrize("k", [1, 2])
def test_scale_attn_fwd_and_combine(ops, k, Do, Dh):
    """wts against the float64 softmax, the expert output and img_l one bf16 rounding off.  B*P = 13*49 is not a multiple of 4;
    slot tables come from the real dispatch on random top-k indices."""
    gen = torch.Generator().manual_seed(1000 * k + Do)
    B, P, E = 13, 49, 8
    _, v = moe_tables(ops, gen, B, k, E, P)
    R = B * k * P
    e_row = v["expert_of_slot"].long().repeat_interleave(P)
    G = rnd(gen, 4, R, Do).clamp_min(0).to(BF)
    H1 = rnd(gen, 4, R, Dh).clamp_min(0).to(BF)
    w2 = rnd(gen, E, Dh, scale=1.0 / math.sqrt(Dh))
    b2 = rnd(gen, E, scale=0.5)
    gates = (torch.rand(B * k, generator=gen) * 0.8 + 0.2).to(DEV)
    ob, out = guarded((R, Do), BF)
    wb, wts = guarded((R, 4), F32)
    ops.call("scale_attn_fwd", G, H1, w2, b2, v["expert_of_slot"], P, out, wts, R, Do, Dh)
    lb, img_l = guarded((B * P, Do), BF)
    ops.call("combine_fwd", out, v["slot_of"], gates, img_l, B, k, P, Do)
    torch.cuda.synchronize()
    assert tail_ok(ob, R * Do) and tail_ok(wb, R * 4) and tail_ok(lb, B * P * Do)

    a, S = scale_logits64(H1, w2, b2, e_row)
    w_ref = torch.softmax(a, dim=0)                                         # [4, R]
    # logits: per-lane chain of 8 * ceil(Dh / 512) products, a 6-level wave tree and the bias -> |da| <= (8*ceil(Dh/512) + 7) u S.
    # softmax: |dw_s| <= w_s (|da_s| + sum_t w_t |da_t|) + (exp, max, 4-term sum, division) <= w_s (2 (c_logit) max_t S_t + (4 + |a_s - m|)) u
    c_logit = 8 * math.ceil(Dh / 512) + 7
    terms_w = w_ref * (2 * c_logit * S.max(dim=0).values[None] + 4 + (a - a.max(dim=0).values[None]).abs())
    check(f"scale_attn_fwd wts k={k} Do={Do} Dh={Dh}", wts.t(), w_ref, terms_w, 0.0, U)
    # out = bf16(sum_s w_s G_s): 4 fp32 products / sums plus the weights' own error (relative, from terms_w)
    G64 = G.to(F64)
    rel_w = (terms_w * U / w_ref).max().item()
    out_ref = torch.einsum("sr,srd->rd", w_ref, G64)
    terms_o = torch.einsum("sr,srd->rd", w_ref, G64.abs())
    check(f"scale_attn_fwd out k={k} Do={Do} Dh={Dh}", out, out_ref, terms_o, UBF, 5 * U + rel_w)
    # combine on the kernel's own expert output: k products / sums (fma) in fp32, then one bf16 rounding
    eo = out.to(F64)
    rows = (v["slot_of"].long().view(B, k, 1) * P + torch.arange(P, device=DEV).view(1, 1, P))       # [B, k, P]
    g64 = gates.to(F64).view(B, k, 1, 1)
    l_ref = (g64 * eo[rows]).sum(1).reshape(B * P, Do)
    l_terms = (g64 * eo[rows].abs()).sum(1).reshape(B * P, Do)
    check(f"combine_fwd img_l k={k} Do={Do}", img_l, l_ref, l_terms, UBF, (k + 1) * U)


# ------------------------------------------------------------------------------------------------------------------------------
# scale_attn_bwd
# ------------------------------------------------------------------------------------------------------------------------------
def wave_kinds(expert_of_slot, P, R, rpw):
    """From the host-side slot table: does some wave change expert inside its rows (mid-wave flush), does some workgroup end all its
    waves on one expert (LDS reduction), does some workgroup end them on several (per-wave fallback)?"""
    e_row = np.repeat(np.asarray(expert_of_slot), P)
    waves = (R + rpw - 1) // rpw
    first = e_row[np.arange(waves) * rpw]
    last = e_row[np.minimum(np.arange(waves) * rpw + rpw, R) - 1]
    kinds = set()
    if (first != last).any():
        kinds.add("mid-wave flush")
    for g in range(0, waves, SA_WAVES):
        kinds.add("LDS reduction" if len(set(last[g:g + SA_WAVES].tolist())) == 1 else "per-wave fallback")
    n_flush = max(int(((first <= e) & (last >= e)).sum()) for e in np.unique(e_row))     # waves touching expert e: one flush each at most
    return kinds, n_flush


def auto_rows_per_wave(R):
    return max(4, min(8, (R + 49999) // 50000))         # the built-in rule of medmoe_scale_attn_bwd


SA_CASES = [(rpw, k, var) for rpw in (0, 1, 3, 8, 200) for k in (1, 2) for var in ("both+dgate", "l", "g+dgate")] + \
           [(1, 2, "both"), (200, 1, "g")]


def run_scale_attn_bwd(ops, B, k, P, E, Do, Dh, rpw, var, seed):
    gen = torch.Generator().manual_seed(seed)
    _, v = moe_tables(ops, gen, B, k, E, P)
    R = B * k * P
    e_row = v["expert_of_slot"].long().repeat_interleave(P)
    G = rnd(gen, 4, R, Do).clamp_min(0).to(BF)
    H1 = rnd(gen, 4, R, Dh).clamp_min(0).to(BF)                              # post-ReLU: about half exact zeros
    w2 = rnd(gen, E, Dh, scale=1.0 / math.sqrt(Dh))
    b2 = rnd(gen, E, scale=0.5)
    gates = (torch.rand(B * k, generator=gen) * 0.8 + 0.2).to(DEV)
    use_l, use_g, use_gate = var.startswith(("both", "l")), var.startswith(("both", "g")), var.endswith("dgate")
    d_img_l = rnd(gen, B * P, Do).to(BF) if use_l else None
    d_img_g = rnd(gen, B, Do, scale=4.0) if use_g else None
    a, _ = scale_logits64(H1, w2, b2, e_row)
    w_ref = torch.softmax(a, dim=0)
    wts = w_ref.t().to(F32).contiguous()
    eout = torch.einsum("sr,srd->rd", w_ref, G.to(F64)).to(BF)
    dGb, dG = guarded((4, R, Do), BF)
    dHb, dH1 = guarded((4, R, Dh), BF)
    p_w2, p_b2, p_g = rnd(gen, E, Dh, scale=0.1), rnd(gen, E, scale=0.1), rnd(gen, B * k, scale=0.1)
    w2b, dw2 = guarded((E, Dh), F32, p_w2)
    b2b, db2 = guarded((E,), F32, p_b2)
    gb, dgate = guarded((B * k,), F32, p_g) if use_gate else (None, None)
    try:
        ops.set_option(13, rpw)
        ops.call("scale_attn_bwd", d_img_l, d_img_g, G, H1, wts, w2, eout, v["expert_of_slot"], v["item_of_slot"], gates, k, P,
                 dG, dH1, dw2, db2, dgate, R, Do, Dh)
        torch.cuda.synchronize()
    finally:
        ops.set_option(13, 0)
    for buf, n in ((dGb, 4 * R * Do), (dHb, 4 * R * Dh), (w2b, E * Dh), (b2b, E)) + (((gb, B * k),) if use_gate else ()):
        assert tail_ok(buf, n)

    # ---- float64 autograd of loss = <img_l, d_img_l> + <mean_p img_l, d_img_g>; G, H1, w2, b2, gates independent leaves ----
    G64 = G.to(F64).requires_grad_()
    H64 = H1.to(F64).requires_grad_()
    w64 = w2.to(F64).requires_grad_()
    b64 = b2.to(F64).requires_grad_()
    g64 = gates.to(F64).requires_grad_()
    aa = torch.einsum("srd,rd->sr", H64, w64[e_row]) + b64[e_row][None]
    ww = torch.softmax(aa, dim=0)
    out = torch.einsum("sr,srd->rd", ww, G64)
    eo = out + (eout.to(F64) - out).detach()          # value = the kernel's expert_out (dgate reads it), gradient flows into w, G
    rows = v["slot_of"].long().view(B, k, 1) * P + torch.arange(P, device=DEV).view(1, 1, P)
    img_l = (g64.view(B, k, 1, 1) * eo[rows]).sum(1)                        # [B, P, Do]
    loss = 0
    if use_l:
        loss = loss + (img_l * d_img_l.to(F64).view(B, P, Do)).sum()
    if use_g:
        loss = loss + (img_l.mean(1) * d_img_g.to(F64)).sum()
    loss.backward()
    del eo, img_l, out, loss

    with torch.no_grad():
        item = v["item_of_slot"].long()
        b_row = (item // k).repeat_interleave(P)
        p_row = torch.arange(R, device=DEV) % P
        gt_row = gates.to(F64)[item].repeat_interleave(P)
        fabs = torch.zeros(R, Do, device=DEV, dtype=F64)                     # |d_img_l| + |d_img_g| / P per slot row
        if use_l:
            fabs += d_img_l.to(F64).view(B, P, Do)[b_row, p_row].abs()
        if use_g:
            fabs += d_img_g.to(F64).abs()[b_row] / P
        # dG = bf16(w_s * (gt * (d_img_l + d_img_g * fl(1/P)))): 1/P, the product, the sum, * gt, * w_s, w_s itself -> 6 roundings
        check(f"scale_attn_bwd dG rpw={rpw} k={k} {var}", dG, G64.grad, ww.detach()[..., None] * (gt_row[:, None] * fabs)[None], UBF, 6 * U)
        # dws_s = <dfin, G_s>: per-lane chain of 8 * ceil(Do / 512) products + 6-level tree (+ dfin's 3 roundings);
        # da_s = w_s (dws_s - sum_t w_t dws_t) -> |err| <= c_da u A_s with A_s = w_s (D_s + sum_t w_t D_t), D_s = sum |dfin G_s|
        chain = 8 * math.ceil(Do / 512) + 6
        c_da = chain + 8
        D = torch.einsum("rd,srd->sr", gt_row[:, None] * fabs, G64.detach().abs())
        A = ww.detach() * (D + (ww.detach() * D).sum(0, keepdim=True))
        mask = (H1 > 0).to(F64)
        check(f"scale_attn_bwd dH1 rpw={rpw} k={k} {var}", dH1, H64.grad * mask, A[..., None] * w2.to(F64).abs()[e_row][None] * mask, UBF,
              (c_da + 2) * U)
        # dw2 / db2: per-wave sequential over 4 * rows_per_wave terms, the 16-wave LDS sum, then one atomic per flush of the expert.
        # This worst case over thousands of summands sits orders of magnitude above the observed error; the dyadic test below pins
        # the same sums bit for bit.
        r_eff = rpw if rpw > 0 else auto_rows_per_wave(R)
        _, n_flush = wave_kinds(v["expert_of_slot"].cpu().numpy(), P, R, r_eff)
        depth = 4 * r_eff + SA_WAVES + n_flush + 1
        tw = torch.zeros(E, Dh, device=DEV, dtype=F64).index_add_(0, e_row, torch.einsum("sr,srd->rd", A, H1.to(F64)))
        check(f"scale_attn_bwd dw2 rpw={rpw} k={k} {var}", dw2, p_w2.to(F64) + w64.grad, p_w2.to(F64).abs() + tw, 0.0, (c_da + depth + 1) * U)
        tb = torch.zeros(E, device=DEV, dtype=F64).index_add_(0, e_row, A.sum(0))
        check(f"scale_attn_bwd db2 rpw={rpw} k={k} {var}", db2, p_b2.to(F64) + b64.grad, p_b2.to(F64).abs() + tb, 0.0, (c_da + depth + 1) * U)
        if use_gate:
            # dgate[item] += sum_p <d_final, expert_out>: the per-row dot (chain) and P atomics per item
            td = torch.zeros(B * k, device=DEV, dtype=F64).index_add_(0, item.repeat_interleave(P), (fabs * eout.to(F64).abs()).sum(1))
            check(f"scale_attn_bwd dgate rpw={rpw} k={k} {var}", dgate, p_g.to(F64) + g64.grad, p_g.to(F64).abs() + td, 0.0,
                  (chain + P + 4) * U)
    return v


@pytest.mark.parametrize("rpw,k,var", SA_CASES)
def test_scale_attn_bwd_full_width(ops, rpw, k, var):
    """cfg2 width (Do 768, Dh 384, P 196, 8 experts); rows per wave forced through option 13 (0 = the built-in rule)."""
    run_scale_attn_bwd(ops, 32, k, 196, 8, 768, 384, rpw, var, seed=7 * rpw + 3 * k + len(var))


def test_scale_attn_bwd_cases_cover_every_workgroup_kind():
    """The slot tables of the cases above produce all three workgroup kinds of the final flush (host-side replay of the tables)."""
    seen = set()
    for rpw, k, var in SA_CASES:
        gen = torch.Generator().manual_seed(7 * rpw + 3 * k + len(var))
        idx = make_idx(gen, 32, k, 8, "random")
        R = 32 * k * 196
        kinds, _ = wave_kinds(idx[np.argsort(idx, kind="stable")], 196, R, rpw if rpw > 0 else auto_rows_per_wave(R))
        seen |= kinds
    print(f"[kinds] {sorted(seen)}")
    assert seen == {"mid-wave flush", "LDS reduction", "per-wave fallback"}, seen


def test_scale_attn_bwd_auto_rule_above_four_rows(ops):
    """R = 200704 > 200 000 at Do 64 / Dh 32: the built-in rule picks more than 4 rows per wave."""
    assert auto_rows_per_wave(512 * 2 * 196) > 4
    run_scale_attn_bwd(ops, 512, 2, 196, 8, 64, 32, 0, "both+dgate", seed=11)


def snap(x, bits=12):
    """A float64 reference that is exact up to float64 noise, put back on its dyadic grid (every value here is a multiple of 2^-11)."""
    return torch.round(x * 2.0 ** bits) / 2.0 ** bits


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("rpw", [0, 1, 3, 8, 200])
def test_scale_attn_bwd_exact_on_dyadic_data(ops, rpw, k):
    """On inputs from small dyadic grids every fp32 product and partial sum inside the kernel is exact, whatever the order: G, H1, expert_out
    integers in [0, 3]; d_img_l in {0, +-1/4}; gates in {1/2, 1}; scale weights a permutation of (1/2, 1/4, 1/8, 1/8); w2 in {j/4}; priors
    multiples of 2^-9.  dG, dH1, dw2, db2 and dgate must then equal the float64 autograd reference bit for bit.  This pins the cross-wave
    reductions of dw2 / db2 (thousands of summands), which the fp32 bars of the random-data cases above can only bound loosely."""
    B, P, E, Do, Dh = 32, 196, 8, 768, 384
    gen = torch.Generator().manual_seed(100 + rpw + k)
    _, v = moe_tables(ops, gen, B, k, E, P)
    R = B * k * P
    e_row = v["expert_of_slot"].long().repeat_interleave(P)
    G = torch.randint(0, 4, (4, R, Do), generator=gen).to(DEV, BF)
    H1 = (torch.rand(4, R, Dh, generator=gen) < 0.25).to(DEV, BF)
    eout = torch.randint(0, 4, (R, Do), generator=gen).to(DEV, BF)
    w2 = (torch.randint(-4, 5, (E, Dh), generator=gen) / 4.0).to(DEV)
    b2 = torch.zeros(E, device=DEV)
    gates = (torch.randint(1, 3, (B * k,), generator=gen) / 2.0).to(DEV)
    d_img_l = (torch.randint(-1, 2, (B * P, Do), generator=gen) * (torch.rand(B * P, Do, generator=gen) < 0.125) / 4.0).to(DEV, BF)
    wts = torch.tensor([0.5, 0.25, 0.125, 0.125])[torch.rand(R, 4, generator=gen).argsort(1)].to(DEV)
    p_w2, p_b2, p_g = (torch.randint(-512, 513, s, generator=gen).to(DEV) / 512.0 for s in ((E, Dh), (E,), (B * k,)))
    dGb, dG = guarded((4, R, Do), BF)
    dHb, dH1 = guarded((4, R, Dh), BF)
    w2b, dw2 = guarded((E, Dh), F32, p_w2)
    b2b, db2 = guarded((E,), F32, p_b2)
    gb, dgate = guarded((B * k,), F32, p_g)
    try:
        ops.set_option(13, rpw)
        ops.call("scale_attn_bwd", d_img_l, None, G, H1, wts, w2, eout, v["expert_of_slot"], v["item_of_slot"], gates, k, P,
                 dG, dH1, dw2, db2, dgate, R, Do, Dh)
        torch.cuda.synchronize()
    finally:
        ops.set_option(13, 0)
    for buf, n in ((dGb, 4 * R * Do), (dHb, 4 * R * Dh), (w2b, E * Dh), (b2b, E), (gb, B * k)):
        assert tail_ok(buf, n)

    G64, H64 = G.to(F64).requires_grad_(), H1.to(F64).requires_grad_()
    w64, b64, g64 = w2.to(F64).requires_grad_(), b2.to(F64).requires_grad_(), gates.to(F64).requires_grad_()
    lin = torch.einsum("srd,rd->sr", H64, w64[e_row]) + b64[e_row][None]
    aa = lin + (wts.t().to(F64).log() - lin).detach()          # the logits' value gives softmax = wts; the gradient is that of H1 . w2 + b2
    aa.retain_grad()
    ww = torch.softmax(aa, dim=0)
    out = torch.einsum("sr,srd->rd", ww, G64)
    eo = out + (eout.to(F64) - out).detach()
    rows = v["slot_of"].long().view(B, k, 1) * P + torch.arange(P, device=DEV).view(1, 1, P)
    img_l = (g64.view(B, k, 1, 1) * eo[rows]).sum(1)
    (img_l * d_img_l.to(F64).view(B, P, Do)).sum().backward()
    with torch.no_grad():
        # precondition: every partial sum stays below 2^24 units of its grid, so that fp32 holds it exactly in any order
        item = v["item_of_slot"].long()
        f_rows = d_img_l.to(F64).view(B, P, Do)[(item // k).repeat_interleave(P), torch.arange(R, device=DEV) % P]
        fin = gates.to(F64)[item].repeat_interleave(P)[:, None] * f_rows
        dws_abs = torch.einsum("rd,srd->sr", fin.abs(), G.to(F64))
        assert (2 * dws_abs * 64).max() < 2 ** 24                                      # dws (grid 2^-3), w . dws and dws - wd (2^-6)
        da = aa.grad                                                                   # grid 2^-9
        tw = torch.zeros(E, Dh, device=DEV, dtype=F64).index_add_(0, e_row, torch.einsum("sr,srd->rd", da.abs(), H1.to(F64)))
        tb = torch.zeros(E, device=DEV, dtype=F64).index_add_(0, e_row, da.abs().sum(0))
        td = torch.zeros(B * k, device=DEV, dtype=F64).index_add_(0, item.repeat_interleave(P), (f_rows.abs() * eout.to(F64)).sum(1))
        for t_, prior in ((tw, p_w2), (tb, p_b2), (td, p_g)):
            assert ((t_ + prior.to(F64).abs()) * 2 ** 9).max() < 2 ** 24
        for name, got, ref in (("dw2", dw2, p_w2.to(F64) + w64.grad), ("db2", db2, p_b2.to(F64) + b64.grad),
                               ("dgate", dgate, p_g.to(F64) + g64.grad)):
            assert torch.equal(got, snap(ref).to(F32)), name
        assert torch.equal(dG, snap(G64.grad).to(F32).to(BF))
        assert torch.equal(dH1, snap(H64.grad * (H1 > 0)).to(F32).to(BF))
        print(f"[exact] scale_attn_bwd dyadic rpw={rpw} k={k}: dG, dH1, dw2, db2, dgate bit-exact")


# ------------------------------------------------------------------------------------------------------------------------------
# stage_grad_add, mean_tokens, broadcast_tokens
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [196, 256, 576])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("D", [768, 1024, 64])
def test_stage_grad_add_exact(ops, D, k, P):
    """dx[b, 1 + p] = bf16((dx + dF[slot(b, 0)]) + dF[slot(b, 1)]) in fp32, in that order: exact.  The CLS rows stay untouched."""
    gen = torch.Generator().manual_seed(D + 10 * k + P)
    B, E = 5, 8
    Nt = P + 1
    _, v = moe_tables(ops, gen, B, k, E, P)
    dF = rnd(gen, B * k * P, D).to(BF)
    prior = rnd(gen, B, Nt, D).to(BF)
    buf, dx = guarded((B, Nt, D), BF, prior)
    dx[:, 0] = torch.full((B, D), SENT[BF], dtype=torch.int16, device=DEV).view(BF)        # CLS rows: sentinel, must stay
    ops.call("stage_grad_add", dF, v["slot_of"], dx, B, k, P, Nt, D)
    torch.cuda.synchronize()
    acc = prior[:, 1:].float()
    slots = v["slot_of"].long().view(B, k)
    for j in range(k):
        acc = acc + dF.view(-1, P, D)[slots[:, j]].float()
    assert torch.equal(dx[:, 1:], acc.to(BF))
    assert sentinel_ok(dx[:, 0]) and tail_ok(buf, B * Nt * D)


MEAN_CASES = [(D, t0, cnt, P) for D in (768, 1024, 64) for (t0, cnt) in ((1, "P"), (0, "P"), (0, 1)) for P in (196, 256, 576)]


@pytest.mark.parametrize("D,t0,cnt,P", MEAN_CASES)
def test_mean_tokens_bit_exact(ops, D, t0, cnt, P):
    """out = (t-ascending fp32 sum) / cnt, contraction off: the bit-exact contract the router's top-k rests on."""
    cnt = P if cnt == "P" else cnt
    gen = torch.Generator().manual_seed(D + 3 * P + t0 + cnt)
    B, Nt = 3, P + 1
    x = rnd(gen, B, Nt, D).to(BF)
    buf, out = guarded((B, D), F32)
    ops.call("mean_tokens", x, out, B, Nt, D, t0, cnt)
    torch.cuda.synchronize()
    acc = torch.zeros(B, D, device=DEV, dtype=F32)
    for t in range(t0, t0 + cnt):
        acc = acc + x[:, t].float()
    assert torch.equal(out, f32_div(acc, cnt))
    assert tail_ok(buf, B * D)


@pytest.mark.parametrize("D,t0,cnt,P", MEAN_CASES)
def test_broadcast_tokens_exact(ops, D, t0, cnt, P):
    """dy[b, t] = bf16(g[b] * scale) for t in [t0, t0 + cnt), exact zeros elsewhere (the buffer starts non-zero)."""
    cnt = P if cnt == "P" else cnt
    gen = torch.Generator().manual_seed(D + 5 * P + t0 + cnt)
    B, Nt = 3, P + 1
    g = rnd(gen, B, D)
    scale = float(np.float32(1.0 / cnt))
    buf, dy = guarded((B, Nt, D), BF, rnd(gen, B, Nt, D).to(BF))
    ops.call("broadcast_tokens", g, dy, B, Nt, D, t0, cnt, scale)
    torch.cuda.synchronize()
    ref = torch.zeros(B, Nt, D, device=DEV, dtype=BF)
    ref[:, t0:t0 + cnt] = (g.to(F64) * scale).to(F32).to(BF)[:, None]
    assert torch.equal(dy, ref)
    assert tail_ok(buf, B * Nt * D)


# ------------------------------------------------------------------------------------------------------------------------------
# router_bwd
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 1024])
@pytest.mark.parametrize("Hd", [128, 300])
@pytest.mark.parametrize("E,k", [(8, 1), (8, 2), (8, 8), (16, 1), (16, 2), (16, 8), (64, 1), (64, 2), (64, 8)])
def test_router_bwd(ops, E, k, Hd, B):
    """dlogits, dh, CE and accuracy against float64 autograd of CE(softmax probabilities as logits) + <dgates, gates(p)> + <dprobs_ext, p>;
    labels / dgates / dprobs_ext each present or NULL; rows with exact probability ties."""
    import medmoe_oracle as O
    gen = torch.Generator().manual_seed(E * 100 + k * 10 + Hd + B)
    logits = torch.randn(B, E, generator=gen, dtype=F64)
    logits[0::3, :3] = logits[0::3].max(dim=1, keepdim=True).values + 0.5          # a three-way tie at the top (experts 0, 1, 2)
    logits[1::3] = 0.25                                                           # every expert tied
    probs32 = torch.softmax(logits, dim=-1).to(F32)
    idx = O.topk_lowest_index(probs32, k)
    labels = torch.randint(0, E, (B,), generator=gen)
    labels[0::6] = 0
    labels[3::6] = 1                                                              # tied rows with the first and the second tied index
    pre = torch.randn(B, Hd, generator=gen)
    w2 = torch.randn(E, Hd, generator=gen) / math.sqrt(Hd)
    dgates = torch.randn(B, k, generator=gen)
    dprobs = torch.randn(B, E, generator=gen) * 0.3
    ce_scale = 0.7 / B
    am = np.argmax(probs32.numpy(), axis=1)                                       # first maximum
    for use_lab, use_dg, use_ext in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        L64 = logits.to(DEV).requires_grad_()
        p = torch.softmax(L64, dim=-1)
        loss = torch.zeros((), device=DEV, dtype=F64)
        if use_lab:
            loss = loss + ce_scale * F.cross_entropy(p, labels.to(DEV), reduction="sum")
        if use_dg and k > 1:
            loss = loss + (O.gates_from_probs(p, idx.to(DEV)) * dgates.to(DEV, F64)).sum()
        if use_ext:
            loss = loss + (p * dprobs.to(DEV, F64)).sum()
        if loss.requires_grad:
            loss.backward()
        dl_ref = L64.grad if L64.grad is not None else torch.zeros_like(L64)
        pre64 = pre.to(DEV, F64).requires_grad_()
        ((torch.relu(pre64) @ w2.to(DEV, F64).t()) * dl_ref).sum().backward()
        h = torch.relu(pre).to(DEV)
        dlb, dl = guarded((B, E), F32)
        dhb, dh = guarded((B, Hd), F32)
        prior = torch.tensor([2.5, 0.25], device=DEV)
        lab, la = guarded((2,), F32, prior)
        ops.call("router_bwd", probs32.to(DEV), h, w2.to(DEV), idx.to(DEV, I32).contiguous(), dgates.to(DEV) if use_dg else None,
                 labels.to(DEV, I32) if use_lab else None, dprobs.to(DEV) if use_ext else None, ce_scale, dl, dh, la, B, Hd, E, k)
        torch.cuda.synchronize()
        assert tail_ok(dlb, B * E) and tail_ok(dhb, B * Hd) and tail_ok(lab, 2)
        tag = f"router_bwd E={E} k={k} Hd={Hd} B={B} lab={use_lab} dg={use_dg} ext={use_ext}"
        with torch.no_grad():
            p64 = probs32.to(DEV, F64)
            # scale of dL/dp per row: CE (q - onehot) <= 2 |ce_scale|, the external gradient, the renormalised gates' gradient
            M = torch.full((B,), 2 * abs(ce_scale) * use_lab, device=DEV, dtype=F64)
            if use_ext:
                M += dprobs.to(DEV, F64).abs().max(dim=1).values
            if use_dg and k > 1:
                sel = p64.gather(1, idx.to(DEV))
                ss = sel.sum(1)
                dgd = dgates.to(DEV, F64)
                M += dgd.abs().sum(1) / ss + (dgd * sel).sum(1).abs() / ss ** 2
            # dp: __expf / __logf-free CE softmax over E terms (<= (E + 4) u relative); pd = sum p dp (E terms); dlogits = p (dp - pd)
            terms_dl = p64 * M[:, None] + dl_ref.abs()
            check(tag + " dlogits", dl, dl_ref, terms_dl, 0.0, (2 * E + 17) * U)
            # dh = (sum_e dlogits_e w2[e]) * (h > 0): E-term chain on top of dlogits' error
            terms_dh = terms_dl @ w2.to(DEV, F64).abs()
            check(tag + " dh", dh, pre64.grad, terms_dh, 0.0, (3 * E + 18) * U)
            assert torch.equal(dh[h <= 0], torch.zeros_like(dh[h <= 0]))
            if use_lab:
                q = torch.softmax(p64, dim=-1).gather(1, labels.to(DEV).view(-1, 1)).view(-1)
                ce = -torch.log(q).sum() / B
                # B atomics of -log(q_b) / B; q from an E-term softmax on the device intrinsics
                check(tag + " loss_acc[0]", la[0:1], 2.5 + ce.view(1), (2.5 + ((-torch.log(q)).abs() + 1).sum() / B).view(1), 0.0,
                      (B + E + 8) * U)
                # 1/B is a power of two for B in {1, 1024}: every partial sum of the accuracy is exact
                acc = float(np.float32(0.25) + np.float32((am == labels.numpy()).sum()) / np.float32(B))
                assert la[1].item() == acc, (la[1].item(), acc)
            else:
                assert torch.equal(la, prior)


# ------------------------------------------------------------------------------------------------------------------------------
# patchify_ld, init_tokens, pos_cls_grad
# ------------------------------------------------------------------------------------------------------------------------------
PATCH_CFGS = [(16, 224, 768), (14, 224, 640), (14, 336, 640)]          # (patch, image size, row pitch ld)


@pytest.mark.parametrize("patch,S,ld,in_f32,B", [c + (f, b) for c in PATCH_CFGS for f in (1, 0) for b in (1, 7, 8, 13)] +
                         [(16, 224, 768, f, 1024) for f in (1, 0)])
def test_patchify_ld_exact(ops, patch, S, ld, in_f32, B):
    """Conv2d weight order (c, py, px), fp32 -> bf16 RNE or a bf16 copy: exact.  Padding columns [C p^2, ld) stay untouched."""
    gen = torch.Generator().manual_seed(B + patch + S + in_f32)
    C, gh = 3, S // patch
    img = rnd(gen, B, C, S, S)
    if not in_f32:
        img = img.to(BF)
    P = gh * gh
    buf, out = guarded((B * P, ld), BF)
    ops.call("patchify_ld", img, out, B, C, S, S, patch, in_f32, ld)
    torch.cuda.synchronize()
    ref = img.reshape(B, C, gh, patch, gh, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * P, C * patch * patch).to(BF)
    assert torch.equal(out[:, :C * patch * patch], ref)
    assert sentinel_ok(out[:, C * patch * patch:]) and tail_ok(buf, B * P * ld)


@pytest.mark.parametrize("patch,S,D,B", [(p, s, d, b) for (p, s, _) in PATCH_CFGS for d in (768, 1024, 516) for b in (1, 7, 8, 13)] +
                         [(16, 224, d, 1024) for d in (768, 1024, 516)])
def test_init_tokens_and_pos_cls_grad_exact(ops, patch, S, D, B):
    """init_tokens: bf16(pos[t] + cls at t = 0), exact.  pos_cls_grad: dpos[t] += b-ascending fp32 sum of dx[b, t], dcls += the t = 0
    sum, exact; B = 13 runs both the 8-wide main loop and the tail, D = 516 a partial second 512-column slab."""
    gen = torch.Generator().manual_seed(B + patch + S + D)
    Nt = (S // patch) ** 2 + 1
    cls, pos = rnd(gen, D), rnd(gen, Nt, D)
    xb, x = guarded((B, Nt, D), BF)
    ops.call("init_tokens", x, cls, pos, B, Nt, D)
    dx = rnd(gen, B, Nt, D).to(BF)
    p_pos, p_cls = rnd(gen, Nt, D), rnd(gen, D)
    pb, dpos = guarded((Nt, D), F32, p_pos)
    cb, dcls = guarded((D,), F32, p_cls)
    ops.call("pos_cls_grad", dx, dpos, dcls, B, Nt, D)
    torch.cuda.synchronize()
    ref = pos.clone()
    ref[0] = ref[0] + cls
    assert torch.equal(x, ref.to(BF).expand(B, Nt, D))
    assert tail_ok(xb, B * Nt * D)
    s = torch.zeros(Nt, D, device=DEV, dtype=F32)
    for b in range(B):
        s = s + dx[b].float()
    assert torch.equal(dpos, p_pos + s)
    assert torch.equal(dcls, p_cls + s[0])
    assert tail_ok(pb, Nt * D) and tail_ok(cb, D)


# ------------------------------------------------------------------------------------------------------------------------------
# text embedding front-end and the aggregation backward
# ------------------------------------------------------------------------------------------------------------------------------
TXT_B, TXT_T, TXT_VOCAB, TXT_EPS = 112, 77, 300, 1e-12          # 8624 rows: the forward's (8192) and the backward's (4096 rows per
                                                                 # pass) grid-stride loops both run more than once; ids repeat


def text_inputs(gen, D, with_tt):
    rows = TXT_B * TXT_T
    ids = torch.randint(0, TXT_VOCAB, (rows,), generator=gen).to(DEV, I32)
    tts = torch.randint(0, 2, (rows,), generator=gen).to(DEV, I32) if with_tt else None
    word, pos, typ = rnd(gen, TXT_VOCAB, D, scale=0.5), rnd(gen, TXT_T, D, scale=0.2), rnd(gen, 2, D, scale=0.1)
    gamma, beta = 1 + rnd(gen, D, scale=0.1), rnd(gen, D, scale=0.1)
    return ids, tts, word, pos, typ, gamma, beta


def text_sum64(ids, tts, word, pos, typ):
    rows = ids.numel()
    t = torch.arange(rows, device=DEV) % TXT_T
    tt = tts.long() if tts is not None else torch.zeros(rows, device=DEV, dtype=torch.long)
    parts = (word.to(F64)[ids.long()], pos.to(F64)[t], typ.to(F64)[tt])
    return parts, t, tt


def ln_depth(D):
    return 4 * math.ceil(D / 256) + 6            # per-lane chain of the row sums (float4 per 64-lane chunk) + 6-level wave tree


@pytest.mark.parametrize("with_tt", [True, False])
@pytest.mark.parametrize("D", [128, 768, 260, 2048])
def test_text_embed_ln_and_packed(ops, D, with_tt):
    """y = LN(word[id] + pos[t] + type[tt]) against float64 F.layer_norm, eps 1e-12; the packed form equals the padded form bit for bit
    on kept rows and leaves the rows past the count untouched."""
    gen = torch.Generator().manual_seed(D + with_tt)
    ids, tts, word, pos, typ, gamma, beta = text_inputs(gen, D, with_tt)
    rows = TXT_B * TXT_T
    ob, out = guarded((rows, D), BF)
    ops.call("text_embed_ln", ids, tts, word, pos, typ, gamma, beta, out, TXT_B, TXT_T, D, TXT_VOCAB, TXT_EPS)
    lens = torch.randint(1, TXT_T + 1, (TXT_B,), generator=gen)
    mask = (torch.arange(TXT_T)[None] < lens[:, None]).to(torch.uint8).to(DEV)
    pk = {nm: guarded((n,), I32) for nm, n in (("tok_row", rows), ("src_of_row", rows), ("seq_off", TXT_B + 1), ("count", 1))}
    ops.call("text_pack", mask, pk["tok_row"][1], pk["src_of_row"][1], pk["seq_off"][1], pk["count"][1], TXT_B, TXT_T)
    pb, packed = guarded((rows, D), BF)
    ops.call("text_embed_ln_packed", ids, tts, word, pos, typ, gamma, beta, packed, TXT_B, TXT_T, D, TXT_VOCAB, TXT_EPS,
             pk["src_of_row"][1], pk["count"][1])
    torch.cuda.synchronize()
    (a, p, y), _, _ = text_sum64(ids, tts, word, pos, typ)
    x = a + p + y
    ref = F.layer_norm(x, (D,), gamma.to(F64), beta.to(F64), TXT_EPS)
    mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    rstd = (var + TXT_EPS).rsqrt()
    xhat = (x - mu) * rstd
    S3 = a.abs() + p.abs() + y.abs()
    terms = gamma.to(F64).abs() * (xhat.abs() + rstd * (S3 + x.abs().mean(-1, keepdim=True))) + beta.to(F64).abs()
    check(f"text_embed_ln y D={D} tt={with_tt}", out, ref, terms, UBF, (ln_depth(D) + 8) * U)
    assert tail_ok(ob, rows * D)
    n = int(pk["count"][1].item())
    assert n == int(lens.sum())
    src = torch.nonzero(mask.view(-1)).view(-1)
    assert torch.equal(pk["src_of_row"][1][:n].long(), src)
    assert torch.equal(packed[:n], out[src])
    assert sentinel_ok(packed[n:]) and tail_ok(pb, rows * D)


@pytest.mark.parametrize("with_tt", [True, False])
@pytest.mark.parametrize("D", [128, 768, 260, 2048])
def test_text_embed_ln_bwd(ops, D, with_tt):
    """dx, the word-table gradient (atomics, repeated ids), dgamma and dbeta (accumulated onto non-zero priors) against float64
    autograd of F.layer_norm(word[id] + pos[t] + type[tt])."""
    gen = torch.Generator().manual_seed(3 * D + with_tt)
    ids, tts, word, pos, typ, gamma, beta = text_inputs(gen, D, with_tt)
    rows = TXT_B * TXT_T
    (a, p, y), _, _ = text_sum64(ids, tts, word, pos, typ)
    x = (a + p + y)
    mu, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    rstd = (var + TXT_EPS).rsqrt()
    xhat = (x - mu) * rstd
    dy = (0.5 * xhat + rnd(gen, rows, D, scale=0.5)).to(BF)                # correlated with xhat: mean(dy g xhat) is not small
    dxb, dx = guarded((rows, D), F32)
    p_g, p_b, p_w = rnd(gen, D, scale=0.3), rnd(gen, D, scale=0.3), rnd(gen, TXT_VOCAB, D, scale=0.3)
    gb, dgamma = guarded((D,), F32, p_g)
    bb, dbeta = guarded((D,), F32, p_b)
    wb, g_word = guarded((TXT_VOCAB, D), F32, p_w)
    ops.call("text_embed_ln_bwd", ids, tts, word, pos, typ, gamma, dy, dx, dgamma, dbeta, g_word, TXT_B, TXT_T, D, TXT_VOCAB, TXT_EPS)
    torch.cuda.synchronize()
    for buf, n in ((dxb, rows * D), (gb, D), (bb, D), (wb, TXT_VOCAB * D)):
        assert tail_ok(buf, n)
    xin = x.clone().requires_grad_()
    g64 = gamma.to(F64).requires_grad_()
    b64 = beta.to(F64).requires_grad_()
    (F.layer_norm(xin, (D,), g64, b64, TXT_EPS) * dy.to(F64)).sum().backward()
    with torch.no_grad():
        depth = ln_depth(D)
        dyg = dy.to(F64) * gamma.to(F64)
        M1, M2 = dyg.abs().mean(-1, keepdim=True), (dyg * xhat).abs().mean(-1, keepdim=True)
        K = rstd * ((a.abs() + p.abs() + y.abs()).max(-1, keepdim=True).values + x.abs().mean(-1, keepdim=True))
        # dx = rstd (dy g - m1 - xhat m2): m1, m2 row sums (depth), xhat and rstd from the recomputed statistics
        terms_dx = rstd * (dyg.abs() + M1 + (xhat.abs() + K) * M2)
        c_dx = 2 * (depth + 8)
        check(f"text_embed_ln_bwd dx D={D} tt={with_tt}", dx, xin.grad, terms_dx, 0.0, c_dx * U)
        occ = torch.bincount(ids.long(), minlength=TXT_VOCAB).max().item()
        ref_w = p_w.to(F64).index_add(0, ids.long(), xin.grad)
        terms_w = p_w.to(F64).abs().index_add(0, ids.long(), terms_dx)
        check(f"text_embed_ln_bwd g_word D={D} tt={with_tt}", g_word, ref_w, terms_w, 0.0, (c_dx + occ + 1) * U)
        grid = min((rows + 3) // 4, 256 * 4)
        chain = math.ceil(rows / (grid * 4)) + 4 + grid + 1          # per-thread rows, the 4-wave LDS sum, one atomic per workgroup, prior
        check(f"text_embed_ln_bwd dgamma D={D} tt={with_tt}", dgamma, p_g.to(F64) + g64.grad,
              p_g.to(F64).abs() + (dy.to(F64).abs() * (xhat.abs() + K)).sum(0), 0.0, (chain + depth + 8) * U)
        check(f"text_embed_ln_bwd dbeta D={D} tt={with_tt}", dbeta, p_b.to(F64) + b64.grad,
              p_b.to(F64).abs() + dy.to(F64).abs().sum(0), 0.0, chain * U)


@pytest.mark.parametrize("which", ["both", "word", "sent"])
@pytest.mark.parametrize("D", [128, 768, 260, 2048])
def test_text_aggregate_bwd_exact(ops, D, which):
    """dH[b, t] = bf16(fma(d_sent[b], fl(1/T), d_word[b, seg])) for kept tokens, exact zeros for seg = -1 (the buffer starts non-zero)."""
    gen = torch.Generator().manual_seed(D + len(which))
    B, T = TXT_B, TXT_T
    lens = torch.randint(1, T + 1, (B,), generator=gen)
    starts = torch.rand(B, T, generator=gen) < 0.6
    starts[:, 0] = True
    seg = starts.long().cumsum(1) - 1
    seg[torch.arange(T)[None] >= lens[:, None]] = -1
    seg = seg.to(DEV, I32).contiguous()
    d_word = rnd(gen, B, T, D) if which in ("both", "word") else None
    d_sent = rnd(gen, B, D) if which in ("both", "sent") else None
    buf, dH = guarded((B * T, D), BF, rnd(gen, B * T, D).to(BF))
    ops.call("text_aggregate_bwd", d_word, d_sent, seg, dH, B, T, D)
    torch.cuda.synchronize()
    segl = seg.long().view(B, T)
    keep = segl >= 0
    b_idx = torch.arange(B, device=DEV)[:, None].expand(B, T)
    w = d_word[b_idx, segl.clamp_min(0)] if d_word is not None else torch.zeros(B, T, D, device=DEV)
    if d_sent is not None:
        invT = torch.tensor(np.float32(1) / np.float32(T), device=DEV)
        v = fma32(d_sent[:, None].expand(B, T, D), invT, w)
    else:
        v = w
    ref = torch.where(keep[..., None], v, torch.zeros_like(v)).to(BF).view(B * T, D)
    assert torch.equal(dH, ref)
    dropped = dH.view(B, T, D)[~keep]
    assert torch.equal(dropped.view(torch.int16), torch.zeros_like(dropped.view(torch.int16)))        # +0.0, not -0.0
    assert tail_ok(buf, B * T * D)


# ------------------------------------------------------------------------------------------------------------------------------
# lerp_tokens_bwd2
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_aux", [True, False])
@pytest.mark.parametrize("Pin,Pout", [(196, 196), (49, 196), (49, 3136), (7, 5)])
def test_lerp_tokens_bwd2(ops, Pin, Pout, with_aux):
    """dx = (gradient of F.interpolate(size = Pout, mode = 'linear', align_corners = False) for dy + dy2) * ReLU'(aux): float64 autograd;
    exact at Pin == Pout (identity: bf16(fl(dy + dy2)) masked)."""
    gen = torch.Generator().manual_seed(Pin * 7 + Pout + with_aux)
    n, D = 4, 768
    dy, dy2 = rnd(gen, n, Pout, D).to(BF), rnd(gen, n, Pout, D).to(BF)
    aux = rnd(gen, n, Pin, D).to(BF) if with_aux else None
    buf, dx = guarded((n, Pin, D), BF)
    ops.call("lerp_tokens_bwd2", dy, dy2, aux, dx, n, Pin, Pout, D)
    torch.cuda.synchronize()
    assert tail_ok(buf, n * Pin * D)
    mask = (aux > 0) if with_aux else torch.ones(n, Pin, D, device=DEV, dtype=torch.bool)
    if Pin == Pout:
        ref = torch.where(mask, dy.float() + dy2.float(), torch.zeros(n, Pin, D, device=DEV)).to(BF)
        assert torch.equal(dx, ref)
        return
    xin = torch.zeros(n, D, Pin, device=DEV, dtype=F64, requires_grad=True)
    yv = F.interpolate(xin, size=Pout, mode="linear", align_corners=False)
    (yv * (dy.to(F64) + dy2.to(F64)).permute(0, 2, 1)).sum().backward()
    ref = xin.grad.permute(0, 2, 1) * mask
    # support: output j reaches input i when its clamped source coordinate lies within one token of i
    src = ((torch.arange(Pout, dtype=F64) + 0.5) * Pin / Pout - 0.5).clamp(0, Pin - 1)
    S = ((src[None, :] - torch.arange(Pin, dtype=F64)[:, None]).abs() < 1 + 1e-3).to(F64).to(DEV)          # [Pin, Pout]
    terms = torch.einsum("ij,njd->nid", S, dy.to(F64).abs() + dy2.to(F64).abs()) * mask
    # fp32 source coordinate and weight (|error| <= 2 (Pin + 2) u), one product + sum per contribution (<= S.sum(1).max() terms)
    c_a = (2 * (Pin + 2) + 2 * int(S.sum(1).max().item()) + 2) * U
    check(f"lerp_tokens_bwd2 Pin={Pin} Pout={Pout} aux={with_aux}", dx, ref, terms, UBF, c_a)
