"""Dropout of the trainable text tower on the GPU (csrc/dropout.hip): the mask contract against the numpy restatement, the attention kernels
with probability dropout, the fused dropout + residual + LayerNorm launch, and both engines' training steps.

Every float64 reference multiplies by the mask that medmoe_dropout_mask exports (the mask contract itself is test 1).  Attention bars: the
per-element bars of tests/test_attention_gpu.py (`fwd_bars` / `bwd_bars`, resident 5-tile chain counts, evaluated on this computation's
float64 quantities) times 1 / (1 - p): surviving probabilities are scaled by that factor and so is their rounding error."""
import math
import os

import numpy as np
import pytest
import torch

import medmoe_oracle as O
from test_attention_gpu import Worst, bits, bwd_bars, e_p, fwd_bars, heads, make_inputs, prefix, run_bwd, run_fwd, scores
from test_glue_kernels_gpu import BF, DEV, F32, F64, UBF, guarded, tail_ok
from test_text_dropout_host import SITE_EMBED, keep_mask

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


def export_mask(ops, rows, cols, cols_padded, seed, step, site, p):
    """the keep mask as a bool tensor; the byte buffer carries a sentinel body and tail (test_glue_kernels_gpu.guarded has no uint8 form)"""
    n, tail, sent = rows * cols, 256, 0xA5
    buf = torch.full((n + tail,), sent, dtype=torch.uint8, device=DEV)
    out = buf[:n].view(rows, cols)
    ops.dropout_mask(out, rows, cols, cols_padded, ops.dropout_rng(seed, step, site, p))
    torch.cuda.synchronize()
    assert bool((buf[n:] == sent).all()), "dropout_mask wrote past the end"
    assert bool((out <= 1).all()), "dropout_mask left part of the mask unwritten"
    return out.bool()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. mask contract
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(5, 128), (2 * 2 * 77, 80), (3, 20)])
def test_mask_equals_the_numpy_restatement(ops, rows, cols):
    for seed, step, site, p in ((0, 0, 0, 0.1), (0x123456789ABCDEF, 7, SITE_EMBED, 0.1), ((1 << 64) - 3, 0xFFFFFFFF, 4 * 11 + 2, 0.5)):
        got = export_mask(ops, rows, cols, cols, seed, step, site, p).cpu().numpy()
        assert np.array_equal(got, keep_mask(rows, cols, cols, seed, step, site, p)), (seed, step, site, p)


def test_mask_key_axis_padded_to_a_multiple_of_four(ops):
    """attention rows of 77 keys: groups of 4 along a key axis of 80, the three pad words are never written"""
    got = export_mask(ops, 2 * 2 * 77, 77, 80, 5, 6, 8, 0.1).cpu().numpy()
    assert np.array_equal(got, keep_mask(2 * 2 * 77, 77, 80, 5, 6, 8, 0.1))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_kept_fraction(ops, p):
    n = 2 * 2 * 77 * 80
    kept = float(export_mask(ops, 2 * 2 * 77, 80, 80, 1, 2, 3, p).float().mean())
    assert abs(kept - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), kept                  # binomial: 5 standard deviations


def test_mask_depends_on_seed_step_site_and_nothing_else(ops):
    a = export_mask(ops, 2 * 2 * 77, 80, 80, 11, 22, 33, 0.5)
    assert torch.equal(a, export_mask(ops, 2 * 2 * 77, 80, 80, 11, 22, 33, 0.5))
    assert torch.equal(a[:77], export_mask(ops, 77, 80, 80, 11, 22, 33, 0.5))           # not the launch geometry
    for other in ((12, 22, 33), (11, 23, 33), (11, 22, 34), (11 + (1 << 32), 22, 33)):
        assert not torch.equal(a, export_mask(ops, 2 * 2 * 77, 80, 80, *other, 0.5)), other


# ------------------------------------------------------------------------------------------------------------------------------
# 2. attention with probability dropout
# ------------------------------------------------------------------------------------------------------------------------------
B_, H_ = 2, 2
FAM = "res"              # chain counts of the resident 5-tile kernels, whose geometry the dropout kernels share


def attn_keep(ops, N, rng_args, p):
    seed, step, site = rng_args
    return export_mask(ops, B_ * H_ * N, N, (N + 3) // 4 * 4, seed, step, site, p).view(B_, H_, N, N)


def run_drop_fwd(ops, qkv, mask, N, rng):
    ob, out = guarded((B_, N, H_ * 64), BF)
    lb, lse = guarded((B_, H_, N), F32)
    ops.attn_drop_fwd(qkv, out, lse, mask, B_, N, H_, rng)
    torch.cuda.synchronize()
    assert tail_ok(ob, out.numel()) and tail_ok(lb, lse.numel()), "forward wrote past the end of out / lse"
    return out, lse


def run_drop_bwd(ops, qkv, out, dout, lse, mask, N, rng):
    gb, dqkv = guarded((B_, N, 3 * H_ * 64), BF)
    db, delta = guarded((B_, H_, N), F32)
    ops.attn_drop_bwd(qkv, out, dout, lse, mask, dqkv, delta, B_, N, H_, rng)
    torch.cuda.synchronize()
    assert tail_ok(gb, dqkv.numel()) and tail_ok(db, delta.numel()), "backward wrote past the end of dqkv / delta"
    return dqkv, delta


def drop_fwd_ref(qkv, mask, keep, sc, N):
    q, k, v, S, A = scores(qkv, mask, B_, N, H_)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    return dict(out=(P * keep * sc) @ v, T=P @ v.abs(), lse=lse, E=e_p(A, N), P=P)


def drop_bwd_ref(qkv, out_in, lse_in, dout, mask, keep, sc, N):
    """float64 restatement on the kernel's own inputs, the softmax multiplied by the exported mask"""
    q, k, v, S, A = scores(qkv, mask, B_, N, H_)
    P = torch.exp(S - lse_in.to(F64)[..., None])
    o, do = heads(out_in, B_, N, H_), heads(dout, B_, N, H_)
    delta, Dabs = (do * o).sum(-1), (do * o).abs().sum(-1)
    dP = (do @ v.transpose(-1, -2)) * keep * sc
    G = do.abs() @ v.abs().transpose(-1, -2)
    dS = P * (dP - delta[..., None])
    return dict(q=q, k=k, do=do, P=P, dS=dS, dP=dP, G=G, delta=delta, Dabs=Dabs, E=e_p(A, N),
                dV=(P * keep * sc).transpose(-1, -2) @ do, dQ=0.125 * dS @ k, dK=0.125 * dS.transpose(-1, -2) @ q)


def scaled(w, f):
    """the bars of out / dQ / dK / dV times f = 1 / (1 - p); lse and delta do not see the mask and keep theirs"""
    return lambda name, got, ref, c_r, bar: w(name, got, ref, c_r, bar * (1.0 if name in ("lse", "delta") else f))


def key_masks(N):
    return {"ragged1": prefix(N, [1, N - 3]), "ragged2": prefix(N, [N, (N + 1) // 2])}


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("N", [16, 17, 77, 80])
def test_attention_elementwise(ops, N, p):
    gen = torch.Generator().manual_seed(9100 + N)
    w = Worst(f"drop N={N} p={p}")
    sc = 1.0 / (1.0 - p)
    for i, (mname, mask) in enumerate(key_masks(N).items()):
        args = (40 + i, 3, 4 * i)
        rng = ops.dropout_rng(*args, p)
        keep = attn_keep(ops, N, args, p).to(F64)
        qkv, dout = make_inputs(gen, B_, N, H_, 1.0)
        out, lse = run_drop_fwd(ops, qkv, mask, N, rng)
        fwd_bars(scaled(w, sc), FAM, drop_fwd_ref(qkv, mask, keep, sc, N), out, lse, B_, N, H_)
        dqkv, delta = run_drop_bwd(ops, qkv, out, dout, lse, mask, N, rng)
        bwd_bars(scaled(w, sc), FAM, drop_bwd_ref(qkv, out, lse, dout, mask, keep, sc, N), dqkv, delta, B_, N, H_)
        pad = ~mask.bool()
        assert not bool(bits(dqkv.view(B_, N, 3, H_ * 64)[:, :, 1:][pad]).any()), (mname, "dK / dV rows of masked keys are not zero")
    w.report()


def test_attention_fully_dropped_rows(ops):
    """p = 0.9 at N = 16 with a caption of length 1: query rows whose unmasked keys are all dropped give out = 0 exactly, nothing is NaN"""
    N, p = 16, 0.9
    sc = 1.0 / (1.0 - p)
    gen = torch.Generator().manual_seed(77)
    mask = prefix(N, [1, N - 3])
    args = (5, 1, 8)
    rng = ops.dropout_rng(*args, p)
    keep = attn_keep(ops, N, args, p)
    dead = ~(keep & mask.bool()[:, None, None, :]).any(-1)                       # [B, H, N] rows with no surviving key
    assert bool(dead.any()), "no fully dropped row in this case"
    qkv, dout = make_inputs(gen, B_, N, H_, 1.0)
    out, lse = run_drop_fwd(ops, qkv, mask, N, rng)
    dqkv, delta = run_drop_bwd(ops, qkv, out, dout, lse, mask, N, rng)
    for t in (out, lse, dqkv, delta):
        assert bool(torch.isfinite(t.float()).all())
    oh = out.view(B_, N, H_, 64).permute(0, 2, 1, 3)
    assert bool((oh[dead] == 0).all()) and bool((delta[dead] == 0).all())
    w = Worst("drop N=16 p=0.9")
    keep = keep.to(F64)
    fwd_bars(scaled(w, sc), FAM, drop_fwd_ref(qkv, mask, keep, sc, N), out, lse, B_, N, H_)
    bwd_bars(scaled(w, sc), FAM, drop_bwd_ref(qkv, out, lse, dout, mask, keep, sc, N), dqkv, delta, B_, N, H_)
    w.report()


@pytest.mark.parametrize("N", [16, 17, 77, 80])
def test_attention_p0_equals_the_plain_kernels(ops, N):
    """p = 0 (thresh 0: every word survives, scale 1): the new kernels against ops.attn_fwd / ops.attn_bwd on the same inputs, within the
    unscaled bars"""
    gen = torch.Generator().manual_seed(9300 + N)
    w = Worst(f"drop-vs-plain N={N}")
    rng = ops.dropout_rng(9, 9, 9, 0.0)
    one = torch.ones(B_, H_, N, N, dtype=F64, device=DEV)
    for mname, mask in key_masks(N).items():
        qkv, dout = make_inputs(gen, B_, N, H_, 1.0)
        out, lse = run_drop_fwd(ops, qkv, mask, N, rng)
        out0, lse0 = run_fwd(ops, qkv, mask, B_, N, H_)
        r = drop_fwd_ref(qkv, mask, one, 1.0, N)
        fwd_bars(w, FAM, dict(r, out=heads(out0, B_, N, H_), lse=lse0.to(F64)), out, lse, B_, N, H_)
        dqkv, delta = run_drop_bwd(ops, qkv, out0, dout, lse0, mask, N, rng)
        dqkv0, delta0 = run_bwd(ops, qkv, out0, dout, lse0, mask, B_, N, H_)
        rb = drop_bwd_ref(qkv, out0, lse0, dout, mask, one, 1.0, N)
        g0 = dqkv0.view(B_, N, 3, H_ * 64)
        rb = dict(rb, delta=delta0.to(F64), dQ=heads(g0[:, :, 0], B_, N, H_), dK=heads(g0[:, :, 1], B_, N, H_), dV=heads(g0[:, :, 2], B_, N, H_))
        bwd_bars(w, FAM, rb, dqkv, delta, B_, N, H_)
    w.report()


def test_attention_shapes_outside_the_limits_are_refused(ops):
    rng = ops.dropout_rng(0, 0, 0, 0.1)
    N = 81
    qkv = torch.zeros(1, N, 192, dtype=BF, device=DEV); out = torch.zeros(1, N, 64, dtype=BF, device=DEV)
    lse = torch.zeros(1, 1, N, device=DEV); dq = torch.zeros_like(qkv); dl = torch.zeros_like(lse)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.attn_drop_fwd(qkv, out, lse, None, 1, N, 1, rng)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.attn_drop_bwd(qkv, out, out, lse, None, dq, dl, 1, N, 1, rng)
    N = 16
    qkv, out, lse = qkv[:, :N].contiguous(), out[:, :N].contiguous(), lse[:, :, :N].contiguous()
    with pytest.raises(RuntimeError, match="code -2"):
        ops.attn_drop_fwd(qkv, out, lse, None, 1, N, 1, rng, head_dim=32)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.attn_drop_bwd(qkv, out, out, lse, None, torch.zeros_like(qkv), torch.zeros_like(lse), 1, N, 1, rng, head_dim=32)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. fused dropout + residual + LayerNorm, elementwise apply
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", [(7, 128), (2 * 16, 768)])
def test_dropout_add_layernorm(ops, rows, D):
    """x1, y, mean, rstd against float64 with the exported mask; the bars of test_kernels_gpu.py::test_layernorm (rel-L2 4e-3 for a bf16
    result, 1e-5 for the statistics, which are taken from the stored bf16 x1 as layernorm_fwd would take them)"""
    torch.manual_seed(5)
    p, eps = 0.1, 1e-6
    sc = 1.0 / (1.0 - p)
    args = (21, 4, 4 * 3 + 1)
    z = (torch.randn(rows, D, device=DEV) * 2 + 0.5).to(BF); res = torch.randn(rows, D, device=DEV).to(BF)
    gam = torch.rand(D, device=DEV) + 0.5; bet = torch.randn(D, device=DEV) * 0.1
    b1, x1 = guarded((rows, D), BF); b2, y = guarded((rows, D), BF); b3, mean = guarded((rows,), F32); b4, rstd = guarded((rows,), F32)
    ops.dropout_add_layernorm_fwd(z, res, gam, bet, x1, y, mean, rstd, eps, ops.dropout_rng(*args, p))
    keep = export_mask(ops, rows, D, D, *args, p).to(F64)
    for b, t in ((b1, x1), (b2, y), (b3, mean), (b4, rstd)):
        assert tail_ok(b, t.numel())
    x1_ref = res.to(F64) + keep * z.to(F64) * sc
    assert rel(x1, x1_ref) < 4e-3
    assert bool(((x1.to(F64) - x1_ref).abs() <= UBF * x1_ref.abs() + 2.0 ** -24 * (res.to(F64).abs() + 2 * z.to(F64).abs() * sc)).all())
    y_ref = torch.nn.functional.layer_norm(x1_ref, (D,), gam.to(F64), bet.to(F64), eps)
    assert rel(y, y_ref) < 4e-3
    xs = x1.to(F64)
    assert torch.allclose(mean.to(F64), xs.mean(1), atol=1e-5, rtol=1e-5)
    assert torch.allclose(rstd.to(F64), 1.0 / torch.sqrt(xs.var(1, unbiased=False) + eps), atol=1e-5, rtol=1e-5)
    # the same layout as layernorm_fwd: its backward runs on (x1, mean, rstd) unchanged (test_layernorm's bars: 5e-3 on dx, 1e-4 on dgamma / dbeta)
    xr = x1.float().requires_grad_(True); gr = gam.clone().requires_grad_(True); br = bet.clone().requires_grad_(True)
    dy = torch.randn(rows, D, device=DEV).to(BF)
    torch.nn.functional.layer_norm(xr, (D,), gr, br, eps).backward(dy.float())
    dx = torch.empty_like(x1); dg = torch.zeros(D, device=DEV); db = torch.zeros(D, device=DEV)
    ops.layernorm_bwd(dy, x1, mean, rstd, gam, dx, dg, db)
    assert rel(dx, xr.grad) < 5e-3 and rel(dg, gr.grad) < 1e-4 and rel(db, br.grad) < 1e-4


@pytest.mark.parametrize("dtype", [BF, F32])
def test_dropout_apply_is_exact(ops, dtype):
    rows, D, p = 33, 128, 0.1
    args = (3, 9, SITE_EMBED)
    rng = ops.dropout_rng(*args, p)
    x = torch.randn(rows, D, device=DEV).to(dtype)
    x = torch.where(x == 0, torch.ones_like(x), x)
    buf, y = guarded((rows, D), dtype)
    ops.dropout_apply(x, y, rng)
    keep = export_mask(ops, rows, D, D, *args, p)
    assert tail_ok(buf, y.numel())
    want = (x.float() * torch.tensor(rng[4], dtype=F32, device=DEV)).to(dtype)      # one fp32 product, rounded once to the output type
    assert torch.equal(y[keep], want[keep])
    assert not bool(bits(y[~keep]).any()), "dropped elements are not exactly zero"
    ops.dropout_apply(x, x, rng)                                                     # in place, as the embedding site runs it
    assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. Engine
# ------------------------------------------------------------------------------------------------------------------------------
def bf_round(t):
    return t.to(torch.bfloat16).float()


def make_engine(hidden=None, attn=None, dropout_seed=None, B=8, seed=3):
    """config `tiny`, trainable text tower; None leaves a field unmentioned"""
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine, VocabTables
    ocfg, cfg = O.config_by_name("tiny"), config_by_name("tiny")
    ocfg.freeze_text = cfg.freeze_text = False
    if hidden is not None:
        cfg.text_hidden_dropout = hidden
    if attn is not None:
        cfg.text_attn_dropout = attn
    if dropout_seed is not None:
        cfg.dropout_seed = dropout_seed
    p = O.init_params(ocfg, seed=seed, std=0.05)
    g = torch.Generator().manual_seed(seed + 7)
    for k in p:
        if k.endswith("layernorm.weight") or k.endswith("layer_norm.weight"):
            p[k] = 1 + 0.2 * torch.randn(p[k].shape, generator=g)
        elif k.endswith(".bias"):
            p[k] = 0.05 * torch.randn(p[k].shape, generator=g)
    for k in p:
        if k.endswith(".weight") and p[k].dim() >= 2 and not k.startswith("moe.router") and "embeddings" not in k:
            p[k] = bf_round(p[k])
    batch = O.synthetic_batch(ocfg, B, min_len=4)
    batch["image"] = bf_round(batch["image"])
    eng = Engine(cfg, "cuda:0", vocab=VocabTables.synthetic(cfg.vocab, "cuda:0"))
    eng.params.load_named({k: v for k, v in p.items() if not k.startswith("text.")})
    eng.tstore.load_named(p)
    return ocfg, cfg, p, batch, eng


LOSSES = ("loss", "g_loss", "l_loss", "classifier_loss")


def step(eng, batch, **kw):
    out = eng.train_step({k: v.cuda() for k, v in batch.items()}, optimizer=False, **kw)
    torch.cuda.synchronize()
    return {k: float(out[k]) for k in LOSSES}


def test_engine_same_seed_same_step(ops):
    """(a) two engines from one seed agree (fp32 atomics in the wgrad and the loss parts: rel 1e-6, not bits); (b) another dropout_seed
    changes the loss; (d) two consecutive steps on one batch draw different masks"""
    _, _, _, batch, e1 = make_engine(0.1, 0.1, 5)
    _, _, _, _, e2 = make_engine(0.1, 0.1, 5)
    _, _, _, _, e3 = make_engine(0.1, 0.1, 6)
    l1, l2, l3 = step(e1, batch), step(e2, batch), step(e3, batch)
    for k in LOSSES:
        assert abs(l1[k] - l2[k]) <= 1e-6 * max(1.0, abs(l2[k])), (k, l1[k], l2[k])
    assert rel(e1.tstore.g32, e2.tstore.g32) < 1e-6
    assert l3["loss"] != l1["loss"] and rel(e3.tstore.g32, e1.tstore.g32) > 1e-3
    assert e1.dropout_step == 1
    again = step(e1, batch)
    assert e1.dropout_step == 2 and again["loss"] != l1["loss"]


def test_engine_eval_never_drops(ops):
    """(e) eval_step of an engine with dropout 0.1 = eval_step of its twin with 0.0, and the step counter stays; (f) with both probabilities
    0.0 a training step gives the losses of an engine whose config never mentions the new fields"""
    _, _, _, batch, ed = make_engine(0.1, 0.1, 5)
    _, _, _, _, e0 = make_engine(0.0, 0.0, 5)
    _, _, _, _, en = make_engine()
    b = {k: v.cuda() for k, v in batch.items()}
    ed.dropout_step = 4
    od, o0 = ed.eval_step(b), e0.eval_step(b)
    torch.cuda.synchronize()
    assert ed.dropout_step == 4
    for k in LOSSES:
        assert abs(float(od[k]) - float(o0[k])) <= 1e-6 * max(1.0, abs(float(o0[k]))), k
    l0, ln = step(e0, batch), step(en, batch)
    for k in LOSSES:
        assert abs(l0[k] - ln[k]) <= 1e-6 * max(1.0, abs(ln[k])), k
    assert rel(e0.tstore.g32, en.tstore.g32) < 1e-6
    assert "t_z" not in e0.ws and "t_z" not in en.ws and "t_z" in ed.ws          # the z buffers exist only where hidden dropout is on


def text_tower_drop64(batch, p, ocfg, masks, sc_h, sc_a):
    """float64 restatement of the embedding front-end, the post-norm blocks (transformer.py:116-130) and the aggregation with BertModel's
    four train-mode dropouts, the masks given"""
    F = torch.nn.functional
    ids, tt, km = batch["ids"], batch["token_type"], batch["attn_mask"].bool()
    B, T = ids.shape
    H, eps = ocfg.n_head_t, ocfg.eps_t
    g = lambda n: p["text." + n]
    ln = lambda x, n: F.layer_norm(x, (x.shape[-1],), g(n + ".weight"), g(n + ".bias"), eps)
    x = g("word_embeddings")[ids] + g("position_embeddings")[:T][None] + g("token_type_embeddings")[tt]
    x = ln(x, "emb_layernorm") * masks["emb"] * sc_h
    hs = [x]
    for l in range(ocfg.n_layer_t):
        b = f"layer.{l}."
        D = x.shape[-1]
        q, k, v = F.linear(x, g(b + "attention.input_proj.weight"), g(b + "attention.input_proj.bias")).view(B, T, 3, H, D // H).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2) / math.sqrt(D // H)).masked_fill(~km[:, None, None, :], float("-inf"))
        a = torch.softmax(s, -1) * masks[f"att{l}"] * sc_a
        o = (a @ v).transpose(1, 2).reshape(B, T, D)
        z = F.linear(o, g(b + "attention.output_proj.weight"), g(b + "attention.output_proj.bias"))
        r = ln(x + z * masks[f"out{l}"] * sc_h, b + "attention_layernorm")
        z = F.linear(F.gelu(F.linear(r, g(b + "feedforward.model.0.weight"), g(b + "feedforward.model.0.bias"))),
                     g(b + "feedforward.model.2.weight"), g(b + "feedforward.model.2.bias"))
        x = ln(r + z * masks[f"ffn{l}"] * sc_h, b + "feedforward_layernorm")
        hs.append(x)
    seg, _, _ = O.segment_map(ids.numpy(), O.Vocab.synthetic(ocfg.vocab))
    return O.aggregate_last_layers(hs, seg, ocfg.last_n_layers)


def test_engine_text_gradients_against_autograd(ops):
    """(c) the text backward alone, as tests/test_text_train_gpu.py (3): the engine's own gradients at the tower's outputs pushed through the
    float64 restatement with the exported masks of the step - every text parameter, the same bars (worst 6e-2, median 2e-2 rel-L2)"""
    ph = pa = 0.1
    ocfg, cfg, p, batch, eng = make_engine(ph, pa, 5)
    B, T, Dt, H, L = 8, cfg.max_len, cfg.d_t, cfg.n_head_t, cfg.n_layer_t
    s0 = eng.dropout_step
    step(eng, batch)
    hm = lambda site: export_mask(ops, B * T, Dt, Dt, cfg.dropout_seed, s0, site, ph).view(B, T, Dt).cpu().double()
    masks = {"emb": hm(SITE_EMBED)}
    for l in range(L):
        masks[f"att{l}"] = export_mask(ops, B * H * T, T, (T + 3) // 4 * 4, cfg.dropout_seed, s0, 4 * l, pa).view(B, H, T, T).cpu().double()
        masks[f"out{l}"], masks[f"ffn{l}"] = hm(4 * l + 1), hm(4 * l + 2)
    pr = {k: v.double().clone().requires_grad_(True) for k, v in p.items() if k.startswith("text.")}
    word, sent = text_tower_drop64(batch, pr, ocfg, masks, 1.0 / (1.0 - ph), 1.0 / (1.0 - pa))
    # forward: the engine's words / sentence embeddings are this graph's
    assert rel(eng.ws["words32"].transpose(1, 2), word) < 2e-2 and rel(eng.ws["txt_g"], sent) < 2e-2
    ((word * eng._d_words.cpu().double().transpose(1, 2)).sum() + (sent * eng.ws["d_txt_g"].cpu().double()).sum()).backward()
    got = eng.tstore.export_named(eng.tstore.g32)
    errs = {}
    for k, v in pr.items():
        if v.grad is not None and float(v.grad.norm()) > 1e-9:
            errs[k] = rel(got[k].reshape(v.grad.shape), v.grad)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    print("text backward under dropout, worst", [(k, round(e, 4)) for k, e in worst], "median", float(np.median(list(errs.values()))), "n", len(errs))
    assert len(errs) == 5 + 12 * ocfg.n_layer_t
    assert max(errs.values()) < 6e-2 and float(np.median(list(errs.values()))) < 2e-2, worst


# ------------------------------------------------------------------------------------------------------------------------------
# 5. SwinEngine
# ------------------------------------------------------------------------------------------------------------------------------
def test_swin_engine_step_with_text_dropout(monkeypatch):
    """one SwinEngine.train_step with a trainable text tower at the smallest geometry of tests/test_swin_text_train_gpu.py: finite losses
    that differ from the dropout-0 twin's on the same weights and batch; the step counter advances once"""
    from test_swin_text_train_gpu import SWIN, TEXT, _batch, _lit
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    DROP = ["model.model.text.hidden_dropout_prob=0.1", "model.model.text.attention_probs_dropout_prob=0.1"]
    _, plain = _lit(SWIN + TEXT)
    _, drop = _lit(SWIN + TEXT + DROP)
    assert drop.model.engine.text_dropout and not plain.model.engine.text_dropout
    mb = _batch(plain, 8, 31)
    op = plain.fused_training_step(mb, optimizer_step=False)
    od = drop.fused_training_step(mb, optimizer_step=False)
    torch.cuda.synchronize()
    for k in ("loss", "l_loss", "g_loss", "classifier_loss"):
        assert math.isfinite(float(od[k])), k
    assert float(od["loss"]) != float(op["loss"]) and float(od["g_loss"]) != float(op["g_loss"])
    assert drop.model.engine.dropout_step == 1
    assert bool(torch.isfinite(drop.model.engine.tstore.g32).all()) and float(drop.model.engine.tstore.g32.abs().max()) > 0
