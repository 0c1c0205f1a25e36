"""Variable-length pass of the trainable text tower (cfg.text_train_varlen).
1. the new entry points, each against the existing entry point on the rows below the device-side count (bit for bit where the arithmetic per
   row is the same) or against float64 (sums whose order differs).  Operand rows at and past the count are NaN, output rows past it carry a
   sentinel that must survive;
2. the engine in packed mode against the CPU oracle (the chain and the bars of tests/test_text_train_gpu.py) with every t_* workspace buffer
   NaN-filled before the step, against the padded engine, for LoRA, under dropout, over optimiser steps, and with the switch off."""
import numpy as np
import pytest
import torch

import medmoe_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
EPS = 2.0 ** -23
NAN = float("nan")
NEW_SYMBOLS = ("attn_bwd_varlen", "layernorm_bwd_rows", "text_aggregate_bwd_packed", "text_embed_ln_bwd_packed", "lora_fwd_rows",
               "lora_bwd_dx_rows", "lora_bwd_wgrad_rows")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def nan_tail(t, count):
    """A copy of t (rows on dim 0) with the rows at and past `count` set to NaN."""
    t = t.clone()
    t[count:] = NAN
    return t


def i32(*v):
    return torch.tensor(v, dtype=I32, device=DEV)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. kernels
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 3])
def test_attn_bwd_varlen_equals_resident(H):
    """dqkv rows and delta[:len] of sequence b are bit-equal to medmoe_attn_bwd (resident 5-tile build, no mask, B = 1, N = len) on that sequence
    alone, for the lengths of tests/test_attention_gpu.py::test_varlen_equals_resident.  16 NaN rows follow the packed operands; the same rows
    of dqkv and every delta entry at positions >= len carry a sentinel."""
    from medmoe_amd import ops
    ops.set_option(11, 1)                                            # the resident kernels (the default)
    gen = torch.Generator().manual_seed(7 + H)
    lens = [17, 1, 80, 16, 79, 1, 80]
    B, Nmax, D, PAD = len(lens), 80, H * 64, 16
    tot = sum(lens)
    off = torch.tensor([0] + lens).cumsum(0).to(I32).to(DEV)
    qkv = nan_tail(torch.randn(tot + PAD, 3 * D, generator=gen).to(DEV).to(BF), tot)
    dout = nan_tail(torch.randn(tot + PAD, D, generator=gen).to(DEV).to(BF), tot)
    out = torch.full((tot + PAD, D), NAN, device=DEV, dtype=BF)
    lse = torch.full((B, H, Nmax), NAN, device=DEV)
    ops.call("attn_fwd_varlen", qkv, out, lse, off, B, Nmax, H, 64)
    dqkv = torch.full((tot + PAD, 3 * D), 7.0, device=DEV, dtype=BF)
    delta = torch.full((B, H, Nmax), 7.0, device=DEV)
    ops.attn_bwd_varlen(qkv, out, dout, lse, off, dqkv, delta, B, Nmax, H)
    torch.cuda.synchronize()
    assert bool((dqkv[tot:] == 7.0).all()) and bool(torch.isfinite(dqkv[:tot].float()).all())
    r0 = 0
    for b, n in enumerate(lens):
        q1, d1 = qkv[r0:r0 + n].contiguous(), dout[r0:r0 + n].contiguous()
        o1, l1 = torch.empty(n, D, device=DEV, dtype=BF), torch.empty(1, H, n, device=DEV)
        ops.attn_fwd(q1, o1, l1, None, 1, n, H)
        g1, dl1 = torch.empty_like(q1), torch.empty(1, H, n, device=DEV)
        ops.attn_bwd(q1, o1, d1, l1, None, g1, dl1, 1, n, H)
        assert same_bits(out[r0:r0 + n], o1), ("out", b, n)
        assert same_bits(dqkv[r0:r0 + n], g1), ("dqkv", b, n)
        assert same_bits(delta[b, :, :n], dl1[0]), ("delta", b, n)
        assert bool((delta[b, :, n:] == 7.0).all()), ("delta tail", b, n)
        r0 += n
    with pytest.raises(RuntimeError, match="code -2"):               # only the 5-tile build exists: Nmax > 80 is a shape error
        ops.call("attn_bwd_varlen", qkv, out, dout, lse, off, dqkv, delta, B, 96, H, 64)


@pytest.mark.parametrize("with_dgamma", [False, True], ids=["dx", "dx+dgamma"])
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("D", [128, 768])
def test_layernorm_bwd_rows(D, with_add, with_dgamma):
    """Buffer of 96 rows, counts 1 / 5 / 95 / 96: dx[:count] bit-equal to medmoe_layernorm_bwd(rows = count); dgamma / dbeta against float64 sums
    of the per-row terms the kernel forms (dy * xhat with xhat = (x - mean) * rstd in fp32, and dy) within count * 2^-23 * sum |terms|."""
    from medmoe_amd import ops
    R = 96
    gen = torch.Generator().manual_seed(D + 2 * with_add + with_dgamma)
    x0 = (torch.randn(R, D, generator=gen) * 1.5 + 0.3).to(DEV).to(BF)
    dy0 = torch.randn(R, D, generator=gen).to(DEV).to(BF)
    add0 = torch.randn(R, D, generator=gen).to(DEV).to(BF)
    gamma = (1 + 0.2 * torch.randn(D, generator=gen)).to(DEV)
    beta = torch.zeros(D, device=DEV)
    for count in (1, 5, 95, 96):
        x, dy, add = nan_tail(x0, count), nan_tail(dy0, count), (nan_tail(add0, count) if with_add else None)
        mean, rstd = torch.full((R,), NAN, device=DEV), torch.full((R,), NAN, device=DEV)
        ops.layernorm_fwd(x[:count], gamma, beta, torch.empty(count, D, device=DEV, dtype=BF), mean, rstd, 1e-5)
        dx = torch.full((R, D), 7.0, device=DEV, dtype=BF)
        dg, db = (torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)) if with_dgamma else (None, None)
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, dx, dg, db, add=add, rows_dev=i32(count))
        ref = torch.empty(count, D, device=DEV, dtype=BF)
        ops.layernorm_bwd(dy[:count], x[:count], mean[:count], rstd[:count], gamma, ref, add=None if add is None else add[:count])
        torch.cuda.synchronize()
        assert same_bits(dx[:count], ref), ("dx", count)
        assert bool((dx[count:] == 7.0).all()), ("dx tail", count)
        if with_dgamma:
            xh = ((x[:count].float() - mean[:count, None]) * rstd[:count, None]).to(F64)          # the kernel's own fp32 xhat
            d64 = dy[:count].to(F64)
            for got, terms, nm in ((dg, d64 * xh, "dgamma"), (db, d64, "dbeta")):
                err = (got.to(F64) - terms.sum(0)).abs()
                tol = count * EPS * terms.abs().sum(0)
                print(f"    D={D} count={count} {nm}: worst error / tolerance {float((err / tol.clamp_min(1e-300)).max()):.3f}")
                assert bool((err <= tol).all()), (nm, count)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.call("layernorm_bwd_rows", dy0, x0, mean, rstd, gamma, None, dx, None, None, R, D, None)


def _pack(mask):
    from medmoe_amd import ops
    B, T = mask.shape
    tok, src, off, cnt = (torch.full((n,), -7, dtype=I32, device=DEV) for n in (B * T, B * T, B + 1, 1))
    ops.call("text_pack", mask.to(torch.uint8).contiguous(), tok, src, off, cnt, B, T)
    return tok, src, off, cnt


def _masks():
    """B = 3, T = 16: holes inside a caption, a caption of a single token, a full caption."""
    m = torch.zeros(3, 16, dtype=torch.bool)
    m[0, :11] = True; m[0, 3] = False; m[0, 7:9] = False
    m[1, 0] = True
    m[2, :] = True
    return m.to(DEV)


def test_aggregate_and_embedding_backward_packed():
    """B = 3, T = 16, D = 128, vocabulary of 11 (ids repeat).  dH[r] bit-equal to the padded kernel's row src[r]; the embedding backward's dx
    bit-equal at the src rows of the zeroed padded buffer and exactly zero elsewhere; g_word / dgamma / dbeta against float64 (g_word: index_add
    of the kernel's own dx) within n_occurrences * 2^-23 * sum |terms| (dgamma / dbeta: every packed row is an occurrence)."""
    from medmoe_amd import ops
    B, T, D, V = 3, 16, 128, 11
    gen = torch.Generator().manual_seed(11)
    mask = _masks()
    tok, src, off, cnt = _pack(mask)
    count = int(cnt.item())
    assert count == int(mask.sum()) == 8 + 1 + 16 and off.tolist() == [0, 8, 9, 25]
    srcl = src[:count].long()
    # ---- aggregation backward ----
    seg = torch.full((B, T), -1, dtype=I32)
    for b in range(B):
        w = 0
        for t in range(T):
            if bool(mask[b, t]) and t % 5 != 4:                     # some kept tokens are dropped ones (seg = -1), words span 1..2 tokens
                seg[b, t] = w
                w += int(t % 3 != 0)
    seg = seg.to(DEV)
    d_word, d_sent = torch.randn(B, T, D, generator=gen).to(DEV), torch.randn(B, D, generator=gen).to(DEV)
    for dw, ds in ((d_word, d_sent), (d_word, None), (None, d_sent)):
        pad = torch.empty(B * T, D, device=DEV, dtype=BF)
        ops.call("text_aggregate_bwd", dw, ds, seg, pad, B, T, D)
        dH = torch.full((B * T, D), 7.0, device=DEV, dtype=BF)
        ops.call("text_aggregate_bwd_packed", dw, ds, seg, src, cnt, dH, B, T, D)
        torch.cuda.synchronize()
        assert same_bits(dH[:count], pad[srcl]) and bool((dH[count:] == 7.0).all())
        assert float(dH[:count].float().abs().max()) > 0
    # ---- embedding backward ----
    ids = torch.randint(0, V, (B, T), generator=gen).to(I32).to(DEV)
    tts = torch.randint(0, 2, (B, T), generator=gen).to(I32).to(DEV)
    word, pos, typ = (torch.randn(n, D, generator=gen).to(DEV) for n in (V, T, 2))
    gamma = (1 + 0.2 * torch.randn(D, generator=gen)).to(DEV)
    dy = nan_tail(torch.randn(B * T, D, generator=gen).to(DEV).to(BF), count)
    dy_pad = torch.zeros(B * T, D, device=DEV, dtype=BF)
    dy_pad[srcl] = dy[:count]
    for tt in (tts, None):
        dx_pad, dgp, dbp, gwp = torch.empty(B * T, D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(V, D, device=DEV)
        ops.call("text_embed_ln_bwd", ids, tt, word, pos, typ, gamma, dy_pad, dx_pad, dgp, dbp, gwp, B, T, D, V, 1e-12)
        dx, dg, db, gw = torch.zeros(B * T, D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(V, D, device=DEV)
        ops.call("text_embed_ln_bwd_packed", ids, tt, word, pos, typ, gamma, dy, dx, dg, db, gw, B, T, D, V, 1e-12, src, cnt)
        torch.cuda.synchronize()
        assert same_bits(dx[srcl], dx_pad[srcl]), "dx at the src rows"
        rest = torch.ones(B * T, dtype=torch.bool, device=DEV); rest[srcl] = False
        assert bool((dx[rest] == 0).all()) and bool(torch.isfinite(dx).all())
        idl = ids.view(-1).long()[srcl]
        terms = dx[srcl].to(F64)
        want = torch.zeros(V, D, device=DEV, dtype=F64).index_add_(0, idl, terms)
        mag = torch.zeros(V, D, device=DEV, dtype=F64).index_add_(0, idl, terms.abs())
        occ = torch.bincount(idl, minlength=V).to(F64)[:, None]
        assert int(occ.max()) > 1 and int(occ.min()) >= 0
        err, tol = (gw.to(F64) - want).abs(), occ * EPS * mag
        print(f"    g_word: worst error / tolerance {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= tol).all())
        assert bool((gw[occ[:, 0] == 0] == 0).all())
        # dgamma / dbeta: xhat of the embedding sum in float64 from the fp32 tables
        tl = (tt.view(-1).long()[srcl] if tt is not None else torch.zeros(count, dtype=torch.long, device=DEV))
        v = ((word[idl] + pos[srcl % T]) + typ[tl]).to(F64)
        xh = (v - v.mean(1, keepdim=True)) / torch.sqrt(v.var(1, unbiased=False, keepdim=True) + 1e-12)
        d64 = dy[:count].to(F64)
        for got, t_, nm in ((dg, d64 * xh, "dgamma"), (db, d64, "dbeta")):
            err, tol = (got.to(F64) - t_.sum(0)).abs(), count * EPS * t_.abs().sum(0)
            print(f"    {nm}: worst error / tolerance {float((err / tol.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= tol).all()), nm


@pytest.mark.parametrize("M,count,N", [(160, 1, 128), (160, 77, 128), (160, 159, 128), (4928, 2500, 256)])
def test_weight_gradient_with_a_device_row_count(M, count, N):
    """medmoe_gemm_tn with n_groups = 1, row_off = [0, count] on the device and M as the host-side bound (the last shape takes the four-wave
    grouped kernel): dW and db against float64 over the first `count` rows within count * 2^-23 * sum |terms|; the rows past the count are NaN."""
    from medmoe_amd import ops
    gen = torch.Generator().manual_seed(M + count)
    g = nan_tail((0.5 * torch.randn(M, N, generator=gen)).to(DEV).to(BF), count)
    x = nan_tail(torch.randn(M, N, generator=gen).to(DEV).to(BF), count)
    dw, db = torch.zeros(N, N, device=DEV), torch.zeros(N, device=DEV)
    ops.gemm_tn(g, x, dw, db=db, row_off=i32(0, count), n_groups=1, M=M)
    torch.cuda.synchronize()
    g64, x64 = g[:count].to(F64), x[:count].to(F64)
    for got, want, mag, nm in ((dw, g64.t() @ x64, g64.abs().t() @ x64.abs(), "dW"), (db, g64.sum(0), g64.abs().sum(0), "db")):
        err, tol = (got.to(F64) - want).abs(), count * EPS * mag
        print(f"    M={M} count={count} {nm}: worst error / tolerance {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        assert bool(torch.isfinite(got).all()) and bool((err <= tol).all()), nm


RP = 16
ALL = ("query", "key", "value")


def _lora_inputs(M, D, r, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g).to(BF)
    qkv = torch.randn(M, 3 * D, generator=g).to(BF)
    dqkv = (0.1 * torch.randn(M, 3 * D, generator=g)).to(BF)
    dy = (0.1 * torch.randn(M, D, generator=g)).to(BF)
    A = torch.zeros(n, RP, D); A[:, :r] = torch.randn(n, r, D, generator=g) * D ** -0.5
    Bw = torch.zeros(n, D, RP); Bw[:, :, :r] = torch.randn(n, D, r, generator=g) * 0.3
    return tuple(t.to(DEV) for t in (x, qkv, dqkv, dy, A.to(BF).reshape(n * RP, D), Bw.to(BF).reshape(n * D, RP)))


@pytest.mark.parametrize("targets", [("query", "value"), ("query", "key", "value"), ("value",)], ids=["qv", "qkv", "v"])
@pytest.mark.parametrize("M,D", [(200, 128), (231, 768), (16, 128), (600, 128)])
def test_lora_rows_equal_the_plain_entry_points(M, D, targets):
    """The shapes of tests/test_text_lora_gpu.py, counts 1 / 17 / M (17 > M: the bound M acts), dropout 0 and 0.5: U, qkv (targeted columns
    changed, the others and the rows past the count untouched), dU, dy, gA and gB bit-equal to the existing entry point with M = count on the
    sliced operands.  (600, 128): three 256-row chunks of the weight-gradient launch, of which the count leaves two or one empty."""
    from medmoe_amd import ops
    n, r, s = len(targets), 8, 2.0
    x0, qkv0, dqkv0, dy0, A, Bw = _lora_inputs(M, D, r, n, seed=M + D + n)
    At, Bt = A.t().contiguous(), Bw.t().contiguous()
    for given in (1, 17, M):
        count = min(given, M)
        for p in (0.0, 0.5):
            rng = ops.dropout_rng(99, 3, 4 + ops.DROPOUT_SITE_LORA, p) if p > 0 else None
            cd = i32(given)
            x, dqkv = nan_tail(x0, count), nan_tail(dqkv0, count)
            # forward
            U, qkv = torch.full((M, n * RP), 7.0, device=DEV, dtype=BF), nan_tail(qkv0, count)
            ops.lora_fwd(x, A, Bw, U, qkv, targets, s, rng, rows_dev=cd)
            Ur, qr = torch.empty(count, n * RP, device=DEV, dtype=BF), qkv0[:count].clone()
            ops.lora_fwd(x0[:count].contiguous(), A, Bw, Ur, qr, targets, s, rng)
            assert same_bits(U[:count], Ur) and same_bits(qkv[:count], qr), ("fwd", given, p)
            assert bool((U[count:] == 7.0).all()) and bool(torch.isnan(qkv[count:].float()).all())
            assert not torch.equal(qr, qkv0[:count])
            # d U and d x
            dU, dy = torch.full((M, n * RP), 7.0, device=DEV, dtype=BF), dy0.clone()
            dy[count:] = 7.0
            ops.lora_bwd_dx(dqkv, Bt, At, dU, dy, targets, s, rng, rows_dev=cd)
            dUr, dyr = torch.empty(count, n * RP, device=DEV, dtype=BF), dy0[:count].clone()
            ops.lora_bwd_dx(dqkv0[:count].contiguous(), Bt, At, dUr, dyr, targets, s, rng)
            assert same_bits(dU[:count], dUr) and same_bits(dy[:count], dyr), ("dx", given, p)
            assert bool((dU[count:] == 7.0).all()) and bool((dy[count:] == 7.0).all())
            dU2 = torch.full_like(dU, 7.0)
            ops.lora_bwd_dx(dqkv, Bt, At, dU2, None, targets, s, rng, rows_dev=cd)
            assert same_bits(dU2, dU)
            # the adapters' gradients: U / dU rows past the count are NaN operands here
            Un, dUn = nan_tail(U, count), nan_tail(dU, count)
            gA, gB = torch.zeros(n * RP, D, device=DEV), torch.zeros(n * D, RP, device=DEV)
            sc = torch.full((ops.lora_wgrad_scratch(M, D, n),), NAN, device=DEV)
            ops.lora_bwd_wgrad(dqkv, x, Un, dUn, gA, gB, sc, targets, s, rng, rows_dev=cd)
            gAr, gBr = torch.zeros_like(gA), torch.zeros_like(gB)
            scr = torch.empty(ops.lora_wgrad_scratch(count, D, n), device=DEV)
            ops.lora_bwd_wgrad(dqkv0[:count].contiguous(), x0[:count].contiguous(), Ur, dUr, gAr, gBr, scr, targets, s, rng)
            torch.cuda.synchronize()
            assert same_bits(gA, gAr) and same_bits(gB, gBr), ("wgrad", given, p)
            assert float(gB.abs().max()) > 0
            gA2, gB2 = torch.zeros_like(gA), torch.zeros_like(gB)
            ops.lora_bwd_wgrad(dqkv, x, Un, dUn, gA2, gB2, torch.empty_like(sc), targets, s, rng, rows_dev=cd)      # reruns stay bit-identical
            assert same_bits(gA2, gA) and same_bits(gB2, gB)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. engine
# ------------------------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def bf_round(t):
    return t.to(BF).float()


def make(cfg_name, B, seed=0, n_continuation=0, varlen=True, lora=False, hidden_dropout=0.0, lora_dropout=0.0):
    """tests/test_text_train_gpu.py::make (the same parameters and batch) with the packed switch; lora: adapters of rank 8 on query and value of
    the frozen base, as tests/test_text_lora_gpu.py::make builds them."""
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine, VocabTables
    ocfg, cfg = O.config_by_name(cfg_name), config_by_name(cfg_name)
    ocfg.freeze_text = False
    cfg.freeze_text = lora
    cfg.text_train_varlen, cfg.text_hidden_dropout = varlen, hidden_dropout
    if lora:
        cfg.text_lora, cfg.text_lora_r, cfg.text_lora_alpha, cfg.text_lora_dropout, cfg.text_lora_targets = True, 8, 16.0, lora_dropout, ("query", "value")
    p = O.init_params(ocfg, seed=seed, std=0.05)
    g = torch.Generator().manual_seed(seed + 7)
    for k in p:
        if k.endswith("layernorm.weight") or k.endswith("layer_norm.weight"):
            p[k] = 1 + 0.2 * torch.randn(p[k].shape, generator=g)
        elif k.endswith(".bias"):
            p[k] = 0.05 * torch.randn(p[k].shape, generator=g)
    p["moe.router.0.weight"] *= 8.0; p["moe.router.2.weight"] *= 8.0
    for k in p:
        if k.endswith(".weight") and p[k].dim() >= 2 and not k.startswith("moe.router") and "embeddings" not in k:
            p[k] = bf_round(p[k])
    batch = O.synthetic_batch(ocfg, B, min_len=4)
    batch["image"] = bf_round(batch["image"])
    if n_continuation:
        gi = torch.Generator().manual_seed(seed + 5)
        ids = batch["ids"]
        cont = torch.randint(ocfg.vocab - n_continuation, ocfg.vocab, ids.shape, generator=gi)
        pick = (torch.rand(ids.shape, generator=gi) < 0.35) & (ids > 2)
        pick[:, :2] = False
        batch["ids"] = torch.where(pick, cont, ids)
    eng = Engine(cfg, "cuda:0", vocab=VocabTables.synthetic(cfg.vocab, "cuda:0", n_continuation))
    if lora:
        eng.params.load_named(p)
        ga, D = torch.Generator().manual_seed(seed + 11), cfg.d_t
        ad = {}
        for l in range(cfg.n_layer_t):
            for t in eng.lora.targets:
                ad[f"text.layer.{l}.attention.{t}.lora_A"] = bf_round(torch.randn(8, D, generator=ga) * D ** -0.5)
                ad[f"text.layer.{l}.attention.{t}.lora_B"] = bf_round(torch.randn(D, 8, generator=ga) * 0.05)
        eng.lora.load_named(ad)
    else:
        eng.params.load_named({k: v for k, v in p.items() if not k.startswith("text.")})
        eng.tstore.load_named(p)
    assert eng.text_train_varlen == varlen
    return ocfg, cfg, p, batch, eng, O.Vocab.synthetic(ocfg.vocab, n_continuation)


def nan_fill_text_workspace(eng, B):
    """Every t_* buffer of the workspace (saved activations, gradients, scratch) NaN after allocation: a packed pass must never let a row at or
    past the count reach a result."""
    eng._alloc(B)
    n = 0
    for k, v in eng.ws.items():
        if k.startswith("t_") and v.is_floating_point():
            v.fill_(NAN)
            n += 1
    assert n > 10
    return n


def to_dev(batch):
    return {k: v.cuda() for k, v in batch.items()}


def test_packed_text_tower_gradients_against_the_oracle():
    """tests/test_text_train_gpu.py::test_text_tower_gradients_against_the_oracle in packed mode (tiny2, B = 8, seed 3, 12 continuation pieces),
    the same comparisons and bars, with the t_* workspace NaN-filled before the step."""
    B = 8
    ocfg, cfg, p, batch, eng, vocab = make("tiny2", B, seed=3, n_continuation=12)
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    ref = O.model_step(batch, pr, ocfg, vocab)
    ref["loss"].backward()
    nan_fill_text_workspace(eng, B)
    out = eng.train_step(to_dev(batch), optimizer=False)
    torch.cuda.synchronize()
    assert eng.text_train_varlen_active
    count = int(batch["attn_mask"].sum())
    assert int(eng._tp.cnt.item()) == count < B * cfg.max_len and eng._tp.row_off.tolist() == [0, count]
    o = eng.outputs()
    assert np.array_equal(o["cap_lens"].cpu().numpy(), np.asarray(ref["cap_lens"]))
    assert torch.equal(o["idx"].cpu().long(), ref["idx"])
    e_g, e_l = rel(o["txt_g"], ref["txt_g"]), rel(o["txt_l"], ref["txt_l"])
    print(f"forward: txt_g {e_g:.5f} txt_l {e_l:.5f}")
    assert e_g < 2e-2 and e_l < 2e-2
    for k in ("g_loss", "l_loss"):
        assert abs(out[k].item() - ref[k].item()) < 1e-2 * abs(ref[k].item()), k
    assert all(np.isfinite(float(v)) for v in out.values())
    P, Do, Hh, T = cfg.n_patch, cfg.d_out, int(cfg.n_patch ** 0.5), cfg.max_len
    x = eng.ws["img_l"].float().cpu().transpose(1, 2).reshape(B, Do, Hh, Hh)
    w = eng.ws["words"].float().cpu().transpose(1, 2).clone().requires_grad_(True)
    tg = eng.ws["txt_g"].float().cpu().clone().requires_grad_(True)
    l0, l1, _ = O.gloria_local(x, w, ref["cap_lens"], ocfg.temp1, ocfg.temp2, ocfg.temp3)
    (ocfg.w_local * (l0 + l1) + ocfg.w_global * O.gloria_global(eng.ws["img_g"].float().cpu(), tg, ocfg.temp3)).backward()
    e_w, e_t = rel(eng._d_words.transpose(1, 2), w.grad), rel(eng.ws["d_txt_g"], tg.grad)
    print(f"caption-side loss gradients: d words {e_w:.4f}  d txt_g {e_t:.5f}")
    assert e_w < 2e-2 and e_t < 1e-3
    got = eng.tstore.export_named(eng.tstore.g32)
    assert bool(torch.isfinite(eng.tstore.g32).all()) and bool(torch.isfinite(eng.params.g32).all())
    for v in pr.values():
        v.grad = None
    word_o, sent_o, _ = O.text_tower(batch["ids"], batch["attn_mask"], batch["token_type"], pr, ocfg, vocab)
    ((word_o * eng._d_words.cpu().transpose(1, 2)).sum() + (sent_o * eng.ws["d_txt_g"].cpu()).sum()).backward()
    errs = {}
    for k, v in pr.items():
        if k.startswith("text.") and v.grad is not None and float(v.grad.norm()) > 1e-9:
            errs[k] = rel(got[k].reshape(v.grad.shape), v.grad)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    print("text backward worst", [(k, round(e, 4)) for k, e in worst], "median", float(np.median(list(errs.values()))), "n", len(errs))
    assert len(errs) == 5 + 12 * ocfg.n_layer_t
    assert max(errs.values()) < 6e-2 and float(np.median(list(errs.values()))) < 2e-2, worst
    used = torch.zeros(ocfg.vocab, dtype=torch.bool); used[batch["ids"].reshape(-1)] = True
    assert float(got["text.word_embeddings"][~used].abs().max()) == 0.0


# Relative error of the packed engine against the padded engine (one state, one batch), measured on an MI355X over 49 repetitions
# (profiles/r14_notes.md has the values); each bar is twice the worst value seen - far inside the quantity's oracle bar of
# tests/test_text_train_gpu.py (2e-2 / 1e-2 / 6e-2).  words and txt_g never differed in a bit (the forward has no order-dependent sum and its
# row-count kernels compute a row as the padded ones do): their bar is 0.  The losses of two PADDED runs differ by the same last-place amounts
# (their sums meet in fp32 atomics); the text gradients' difference is the order of the weight-gradient / LayerNorm / word-table atomics.
PACKED_VS_PADDED = {"words": 0.0, "txt_g": 0.0, "loss": 2 * 1.27e-7, "g_loss": 2 * 1.15e-7, "l_loss": 2 * 8.1e-8, "classifier_loss": 2 * 1.9e-7,
                    "text_grad": 2 * 4.81e-7, "lora_grad": 2 * 7.54e-8}


def _pair(**kw):
    a = make("tiny2", 8, seed=3, n_continuation=12, varlen=True, **kw)
    b = make("tiny2", 8, seed=3, n_continuation=12, varlen=False, **kw)
    return a, b


def test_packed_against_padded_full_tower():
    (_, _, _, batch, pk, _), (_, _, _, _, pd, _) = _pair()
    nan_fill_text_workspace(pk, 8)
    b = to_dev(batch)
    op, od = pk.train_step(b, optimizer=False), pd.train_step(b, optimizer=False)
    torch.cuda.synchronize()
    assert pk.text_train_varlen_active and not pd.text_train_varlen_active
    e = {"words": rel(pk.ws["words"], pd.ws["words"]), "txt_g": rel(pk.ws["txt_g"], pd.ws["txt_g"])}
    for k in ("loss", "g_loss", "l_loss", "classifier_loss"):
        e[k] = abs(float(op[k]) - float(od[k])) / abs(float(od[k]))
    gp, gd = pk.tstore.export_named(pk.tstore.g32), pd.tstore.export_named(pd.tstore.g32)
    ge = {k: rel(gp[k], gd[k]) for k in gd if float(gd[k].norm()) > 1e-9}
    worst = sorted(ge.items(), key=lambda kv: -kv[1])[:4]
    print("packed against padded:", {k: float(f"{v:.3g}") for k, v in e.items()}, "text gradients worst", [(k, float(f"{v:.3g}")) for k, v in worst],
          "median", float(f"{np.median(list(ge.values())):.3g}"), "n", len(ge))
    assert len(ge) == 5 + 12 * pk.cfg.n_layer_t and bool(torch.isfinite(pk.tstore.g32).all())
    assert all(e[k] <= PACKED_VS_PADDED[k] for k in e), e
    assert max(ge.values()) <= PACKED_VS_PADDED["text_grad"], worst


def test_packed_against_padded_lora():
    (_, _, _, batch, pk, _), (_, _, _, _, pd, _) = _pair(lora=True)
    nan_fill_text_workspace(pk, 8)
    b = to_dev(batch)
    pk.train_step(b, optimizer=False); pd.train_step(b, optimizer=False)
    torch.cuda.synchronize()
    assert pk.text_train_varlen_active and pk.lora is not None
    gp, gd = pk.lora.export_named(pk.lora.g32), pd.lora.export_named(pd.lora.g32)
    ge = {k: rel(gp[k], gd[k]) for k in gd}
    worst = sorted(ge.items(), key=lambda kv: -kv[1])[:4]
    print("LoRA packed against padded: words", float(f"{rel(pk.ws['words'], pd.ws['words']):.3g}"), "adapter gradients worst",
          [(k, float(f"{v:.3g}")) for k, v in worst], "median", float(f"{np.median(list(ge.values())):.3g}"), "n", len(ge))
    assert len(ge) == 2 * 2 * pk.cfg.n_layer_t and all(float(v.norm()) > 1e-9 for v in gd.values())
    assert bool(torch.isfinite(pk.lora.g32).all()) and pk.lora.pad_is_zero(pk.lora.g32)
    assert rel(pk.ws["words"], pd.ws["words"]) <= PACKED_VS_PADDED["words"] and rel(pk.ws["txt_g"], pd.ws["txt_g"]) <= PACKED_VS_PADDED["txt_g"]
    assert max(ge.values()) <= PACKED_VS_PADDED["lora_grad"], worst


def test_packed_lora_step_with_dropout_is_bit_identical_when_rerun():
    """Hidden and LoRA dropout 0.1 in packed mode: the same step from the same state twice (dropout_step reset, gradients zeroed by the step)
    gives bit-identical adapter gradients, and other masks at another step."""
    _, _, _, batch, eng, _ = make("tiny2", 8, seed=6, n_continuation=12, lora=True, hidden_dropout=0.1, lora_dropout=0.1)
    b = to_dev(batch)

    def step(n):
        eng.dropout_step = n
        eng.train_step(b, optimizer=False)
        torch.cuda.synchronize()
        return eng.ws["words"].clone(), eng.ws["t_lu1"].clone(), eng.lora.g32.clone()
    a, a2, c = step(5), step(5), step(6)
    count = int(batch["attn_mask"].sum())
    print("rerun: adapter g32 relative difference", rel(a2[2], a[2]))
    assert eng.text_train_varlen_active and eng.dropout_step == 7
    assert torch.equal(a[0], a2[0]) and same_bits(a[1][:count], a2[1][:count])
    assert not torch.equal(a[0], c[0])
    assert float(a[2].abs().max()) > 0 and bool(torch.isfinite(a[2]).all())
    assert same_bits(a[2], a2[2])


@pytest.mark.parametrize("lora", [False, True], ids=["full", "lora"])
def test_three_fused_adam_steps_in_packed_mode(lora):
    _, _, _, batch, eng, _ = make("tiny2", 8, seed=2, lora=lora, hidden_dropout=0.1, lora_dropout=0.1 if lora else 0.0)
    _, _, _, _, pad, _ = make("tiny2", 8, seed=2, lora=lora, hidden_dropout=0.1, lora_dropout=0.1 if lora else 0.0, varlen=False)
    eng.cfg.lr = pad.cfg.lr = 1e-3
    b = to_dev(batch)
    arena = eng.text_arena()
    before = arena.p32.clone()
    losses = [float(eng.train_step(b)["loss"]) for _ in range(3)]
    for _ in range(3):
        pad.train_step(b)
    torch.cuda.synchronize()
    print("losses", losses)
    assert all(np.isfinite(losses)) and eng.text_train_varlen_active
    assert eng.dropout_step == pad.dropout_step == 3
    assert bool(torch.isfinite(arena.p32).all()) and float((arena.p32 - before).abs().max()) > 0


def test_switch_off_launches_none_of_the_new_symbols(monkeypatch):
    """The names of every launch of a step that goes through ops.call, recorded: with the switch off none of the new entry points appears (and
    text_pack does not run); with it on, all that the full tower uses do."""
    from medmoe_amd import ops
    names = []
    real = ops._fn
    monkeypatch.setattr(ops, "_fn", lambda name: (names.append(name), real(name))[1])
    _, _, _, batch, off, _ = make("tiny2", 8, seed=1, varlen=False)
    off.train_step(to_dev(batch))
    torch.cuda.synchronize()
    assert len(names) > 50 and not set(names) & set(NEW_SYMBOLS) and "text_pack" not in names and not off.text_train_varlen_active
    del names[:]
    _, _, _, _, on, _ = make("tiny2", 8, seed=1, varlen=True)
    on.train_step(to_dev(batch))
    torch.cuda.synchronize()
    assert set(names) >= {"text_pack", "attn_bwd_varlen", "layernorm_bwd_rows", "text_aggregate_bwd_packed", "text_embed_ln_bwd_packed"}
