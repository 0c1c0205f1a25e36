"""LoRA adapters of the text tower (cfg.text_lora; medmoe_amd/text_lora.py, csrc/lora.hip).
1. the four kernels against float64 evaluated from the same bf16 inputs (second stages from the chip's own stored bf16 U / dU), elementwise:
   one bf16 ulp of the exact value + K * 2^-23 * sum |terms| of fp32 accumulation over a contraction of length K (fp32 outputs: the slack only);
2. the engine against the CPU oracle, whose fused projection weight is built in the test as W + s [B_q A_q; 0; B_v A_v] from A / B leaves;
3. engine behaviour: B = 0 is the base tower, optimiser steps, accumulation, dropout, merge, checkpoint, SwinEngine, two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import medmoe_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
BF, F64 = torch.bfloat16, torch.float64
RP = 16
ALL = ("query", "key", "value")


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. kernels
# ------------------------------------------------------------------------------------------------------------------------------------------
def ulp_bf16(v):
    """One unit in the last place of bf16 (8 significant bits) at the magnitude of v; 0 at 0 (the slack term covers it)."""
    a = v.abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 7), torch.zeros_like(a))


def close(got, exact, terms, K, ulps=1.0, what=""):
    """|got - exact| <= ulps * ulp_bf16(exact) + K * 2^-23 * sum|terms|, elementwise."""
    err = (got.to(F64) - exact).abs()
    tol = ulps * ulp_bf16(exact) + K * 2.0 ** -23 * terms
    bad = err > tol
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"    {what}: worst error / tolerance {worst:.3f}")
    assert not bool(bad.any()), (what, int(bad.sum()), worst)


def kernel_inputs(M, D, r, targets, seed):
    g = torch.Generator().manual_seed(seed)
    n = len(targets)
    x = torch.randn(M, D, generator=g).to(BF)
    qkv = torch.randn(M, 3 * D, generator=g).to(BF)
    dqkv = (0.1 * torch.randn(M, 3 * D, generator=g)).to(BF)
    dy = (0.1 * torch.randn(M, D, generator=g)).to(BF)
    A = torch.zeros(n, RP, D); A[:, :r] = torch.randn(n, r, D, generator=g) * D ** -0.5
    Bw = torch.zeros(n, D, RP); Bw[:, :, :r] = torch.randn(n, D, r, generator=g) * 0.3
    A, Bw = A.to(BF).reshape(n * RP, D), Bw.to(BF).reshape(n * D, RP)
    return tuple(t.cuda() for t in (x, qkv, dqkv, dy, A, Bw))


def keep_scale(M, D, rng):
    """keep * 1 / (1 - p) of the [M, D] array as the chip draws it, read back through medmoe_dropout_apply on ones."""
    from medmoe_amd import ops
    ones = torch.ones(M, D, device="cuda")
    if rng is None:
        return ones.to(F64)
    return ops.dropout_apply(ones, torch.empty_like(ones), rng).to(F64)


SHAPES = [(200, 128), (231, 768), (16, 128), (600, 128)]      # (600, 128): three 256-row chunks of the weight-gradient launch
TARGETS = [("query", "value"), ("query", "key", "value"), ("value",)]


@pytest.mark.parametrize("targets", TARGETS, ids=["qv", "qkv", "v"])
@pytest.mark.parametrize("M,D", SHAPES)
def test_kernels_against_float64(M, D, targets):
    from medmoe_amd import ops
    n = len(targets)
    cols = [ALL.index(t) * D for t in targets]
    for r in (4, 8, 16):
        for p in (0.0, 0.1):
            s = 16.0 / r
            x, qkv0, dqkv, dy0, A, Bw = kernel_inputs(M, D, r, targets, seed=M + D + r)
            At, Bt = A.t().contiguous(), Bw.t().contiguous()
            rng = ops.dropout_rng(1234, 7, 4 * 2 + ops.DROPOUT_SITE_LORA, p) if p > 0 else None
            m = keep_scale(M, D, rng)
            if p > 0:
                frac = float((m > 0).double().mean())
                assert abs(frac - 0.9) < 0.05 and float(m.max()) == float(torch.tensor(1.0 / 0.9, dtype=torch.float32))
            print(f"  M={M} D={D} r={r} p={p} targets={targets}")
            x64, A64, B64 = x.to(F64), A.to(F64).view(n, RP, D), Bw.to(F64).view(n, D, RP)
            xd = m * x64
            # ---- forward ----
            U, qkv = torch.full((M, n * RP), 7.0, device="cuda", dtype=BF), qkv0.clone()
            ops.lora_fwd(x, A, Bw, U, qkv, targets, s, rng)
            U2, qkv2 = torch.empty_like(U), qkv0.clone()
            ops.lora_fwd(x, A, Bw, U2, qkv2, targets, s, rng)
            assert torch.equal(U, U2) and torch.equal(qkv, qkv2)
            Uv = U.view(M, n, RP)
            assert bool((Uv[:, :, r:] == 0).all())
            close(U, xd @ A.to(F64).t(), xd.abs() @ A.to(F64).abs().t(), D, what="U")
            U64 = U.to(F64).view(M, n, RP)
            touched = torch.zeros(3 * D, dtype=torch.bool)
            for t, c in enumerate(cols):
                q0 = qkv0[:, c:c + D].to(F64)
                close(qkv[:, c:c + D], q0 + s * U64[:, t] @ B64[t].t(), q0.abs() + s * U64[:, t].abs() @ B64[t].abs().t(), RP + 1, what=f"qkv[{targets[t]}]")
                touched[c:c + D] = True
            assert torch.equal(qkv[:, ~touched], qkv0[:, ~touched])
            # ---- backward: d U and d x ----
            dU, dy = torch.full((M, n * RP), 7.0, device="cuda", dtype=BF), dy0.clone()
            ops.lora_bwd_dx(dqkv, Bt, At, dU, dy, targets, s, rng)
            dU2 = torch.empty_like(dU)
            ops.lora_bwd_dx(dqkv, Bt, At, dU2, None, targets, s, rng)              # layer 0: no d x
            assert torch.equal(dU, dU2)
            dU64 = dU.to(F64).view(M, n, RP)
            assert bool((dU64[:, :, r:] == 0).all())
            for t, c in enumerate(cols):
                g64 = dqkv[:, c:c + D].to(F64)
                close(dU.view(M, n, RP)[:, t], s * g64 @ B64[t], s * g64.abs() @ B64[t].abs(), D, what=f"dU[{targets[t]}]")
            flatA = A.to(F64)
            close(dy, dy0.to(F64) + m * (dU.to(F64) @ flatA), dy0.to(F64).abs() + m * (dU.to(F64).abs() @ flatA.abs()), n * RP + 1, what="dx")
            # ---- backward: the adapters' gradients (fp32: the accumulation slack only) ----
            gA, gB = torch.zeros(n * RP, D, device="cuda"), torch.zeros(n * D, RP, device="cuda")
            sc = torch.empty(ops.lora_wgrad_scratch(M, D, n), device="cuda")
            ops.lora_bwd_wgrad(dqkv, x, U, dU, gA, gB, sc, targets, s, rng)
            gA1, gB1 = gA.clone(), gB.clone()
            for t, c in enumerate(cols):
                g64 = dqkv[:, c:c + D].to(F64)
                close(gB.view(n, D, RP)[t], s * g64.t() @ U64[:, t], s * g64.abs().t() @ U64[:, t].abs(), M, ulps=0.0, what=f"gB[{targets[t]}]")
                close(gA.view(n, RP, D)[t], dU64[:, t].t() @ xd, dU64[:, t].abs().t() @ xd.abs(), M, ulps=0.0, what=f"gA[{targets[t]}]")
            assert bool((gA.view(n, RP, D)[:, r:] == 0).all()) and bool((gB.view(n, D, RP)[:, :, r:] == 0).all())
            assert float(gA.abs().max()) > 0 and float(gB.abs().max()) > 0
            ops.lora_bwd_wgrad(dqkv, x, U, dU, gA, gB, sc, targets, s, rng)        # accumulates: a second backward doubles the gradient exactly
            assert torch.equal(gA, 2 * gA1) and torch.equal(gB, 2 * gB1)
            gA3, gB3 = torch.zeros_like(gA), torch.zeros_like(gB)
            ops.lora_bwd_wgrad(dqkv, x, U, dU, gA3, gB3, torch.empty_like(sc), targets, s, rng)
            assert torch.equal(gA3, gA1) and torch.equal(gB3, gB1)
            # ---- merge ----
            W0 = (0.05 * torch.randn(3 * D, D, generator=torch.Generator().manual_seed(r))).to(BF).cuda()
            W = ops.lora_merge(W0.clone(), A, Bw, targets, s)
            rows = torch.zeros(3 * D, dtype=torch.bool)
            for t, c in enumerate(cols):
                w0 = W0[c:c + D].to(F64)
                close(W[c:c + D], w0 + s * B64[t] @ A64[t], w0.abs() + s * B64[t].abs() @ A64[t].abs(), RP + 1, what=f"merge[{targets[t]}]")
                rows[c:c + D] = True
            assert torch.equal(W[~rows], W0[~rows])


def test_wrappers_refuse_bad_shapes():
    from medmoe_amd import ops
    x = torch.zeros(16, 96, device="cuda", dtype=BF)                               # D not a multiple of 64
    with pytest.raises(ValueError):
        ops.lora_fwd(x, torch.zeros(16, 96, device="cuda", dtype=BF), torch.zeros(96, 16, device="cuda", dtype=BF),
                     torch.zeros(16, 16, device="cuda", dtype=BF), torch.zeros(16, 288, device="cuda", dtype=BF), ("value",), 2.0)
    x = torch.zeros(16, 128, device="cuda", dtype=BF)
    with pytest.raises(ValueError):                                                # U of the wrong width
        ops.lora_fwd(x, torch.zeros(16, 128, device="cuda", dtype=BF), torch.zeros(128, 16, device="cuda", dtype=BF),
                     torch.zeros(16, 32, device="cuda", dtype=BF), torch.zeros(16, 384, device="cuda", dtype=BF), ("value",), 2.0)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. engine
# ------------------------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def bf_round(t):
    return t.to(BF).float()


def make(cfg_name, B, seed=0, n_continuation=0, lora=True, r=8, targets=("query", "value"), dropout=0.0, random_b=True, freeze=True):
    """tests/test_text_train_gpu.py::make with adapters: the same parameters and batch, an engine in LoRA mode (or, lora=False, the frozen /
    fully trainable one on the same weights), A and B random (B = 0 would hide A's gradient) and bf16-representable."""
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine, VocabTables
    ocfg, cfg = O.config_by_name(cfg_name), config_by_name(cfg_name)
    ocfg.freeze_text = False                                       # the oracle's text graph carries gradients (to the adapter leaves)
    cfg.freeze_text = freeze
    cfg.text_lora, cfg.text_lora_r, cfg.text_lora_alpha, cfg.text_lora_dropout, cfg.text_lora_targets = lora, r, 16.0, dropout, targets
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
    eng.params.load_named(p)
    if eng.tstore is not None:
        eng.tstore.load_named(p)
    ad = {}
    if lora:
        ga = torch.Generator().manual_seed(seed + 11)
        D = cfg.d_t
        for l in range(cfg.n_layer_t):
            for t in eng.lora.targets:
                ad[f"text.layer.{l}.attention.{t}.lora_A"] = bf_round(torch.randn(r, D, generator=ga) * D ** -0.5)
                ad[f"text.layer.{l}.attention.{t}.lora_B"] = bf_round(torch.randn(D, r, generator=ga) * 0.05) if random_b else torch.zeros(D, r)
        eng.lora.load_named(ad)
    return ocfg, cfg, p, batch, eng, O.Vocab.synthetic(ocfg.vocab, n_continuation), ad


def merged_oracle_params(p, ad, cfg, targets, leaves=None):
    """The oracle's parameter dict with every layer's fused projection weight W + s [B_t A_t in the target's rows; 0 elsewhere] built from
    the adapter tensors `leaves` (default: `ad`) - differentiable in them."""
    leaves = ad if leaves is None else leaves
    s, D = cfg.text_lora_alpha / cfg.text_lora_r, cfg.d_t
    out = dict(p)
    for l in range(cfg.n_layer_t):
        blocks = []
        for t in ALL:
            if t in targets:
                blocks.append(s * leaves[f"text.layer.{l}.attention.{t}.lora_B"] @ leaves[f"text.layer.{l}.attention.{t}.lora_A"])
            else:
                blocks.append(torch.zeros(D, D))
        out[f"text.layer.{l}.attention.input_proj.weight"] = p[f"text.layer.{l}.attention.input_proj.weight"] + torch.cat(blocks, 0)
    return out


def to_dev(batch):
    return {k: v.cuda() for k, v in batch.items()}


def test_engine_against_the_oracle_with_the_merged_weight():
    """tiny2, 8 captions with continuation pieces, adapters on query and value with random A and B, no LoRA dropout.  Forward embeddings and
    losses against the oracle on the merged weight; the adapters' gradients against the oracle's autograd through that weight, with the
    engine's own gradients at the tower's outputs pushed through the oracle's text graph (the chain and the bars of
    tests/test_text_train_gpu.py: embeddings 2e-2, losses 1e-2, gradients worst 6e-2 / median 2e-2).  No base text gradient exists."""
    B = 8
    ocfg, cfg, p, batch, eng, vocab, ad = make("tiny2", B, seed=3, n_continuation=12)
    leaves = {k: v.clone().requires_grad_(True) for k, v in ad.items()}
    pm = merged_oracle_params(p, ad, cfg, eng.lora.targets, leaves)
    ref = O.model_step(batch, pm, ocfg, vocab)
    out = eng.train_step(to_dev(batch), optimizer=False)
    torch.cuda.synchronize()
    o = eng.outputs()
    assert np.array_equal(o["cap_lens"].cpu().numpy(), np.asarray(ref["cap_lens"]))
    e_g, e_l = rel(o["txt_g"], ref["txt_g"]), rel(o["txt_l"], ref["txt_l"])
    print(f"forward: txt_g {e_g:.5f} txt_l {e_l:.5f}")
    assert e_g < 2e-2 and e_l < 2e-2
    for k in ("g_loss", "l_loss"):
        d = abs(out[k].item() - ref[k].item()) / abs(ref[k].item())
        print(f"{k}: engine {out[k].item():.5f} oracle {ref[k].item():.5f} rel {d:.5f}")
        assert d < 1e-2, k
    # the adapters matter at these values: the base tower alone gives other embeddings
    base = O.text_tower(batch["ids"], batch["attn_mask"], batch["token_type"], p, ocfg, vocab)[1]
    assert rel(base, ref["txt_g"]) > 5e-2
    word_o, sent_o, _ = O.text_tower(batch["ids"], batch["attn_mask"], batch["token_type"], pm, ocfg, vocab)
    ((word_o * eng._d_words.cpu().transpose(1, 2)).sum() + (sent_o * eng.ws["d_txt_g"].cpu()).sum()).backward()
    got = eng.lora.export_named(eng.lora.g32)
    assert set(got) == set(ad)
    errs = {k: rel(got[k], leaves[k].grad) for k in ad}
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    med = float(np.median(list(errs.values())))
    print("adapter gradients worst", [(k, round(e, 4)) for k, e in worst], "median", med, "n", len(errs))
    assert len(errs) == 2 * 2 * ocfg.n_layer_t and all(float(leaves[k].grad.norm()) > 1e-9 for k in ad)
    assert max(errs.values()) < 6e-2 and med < 2e-2, worst
    # every base text gradient is absent: no text store, no gradient buffer beyond the adapters' arena, pads exactly zero
    assert eng.tstore is None and eng.text_arena() is eng.lora and eng.lora.pad_is_zero(eng.lora.g32) and eng.lora.pad_is_zero()
    assert "t_dxemb" not in eng.ws


def test_base_tower_keeps_no_master_gradient_or_adam_state():
    """LoRA mode allocates nothing of tower size for the base: params.text stays the frozen dict (bf16 GEMM weights), the only fp32 arena on
    the text side is the adapters' (n_layer * n_t * 2 * 16 * D elements), and the transposed copies are made once (not per step)."""
    ocfg, cfg, p, batch, eng, vocab, ad = make("tiny2", 8, seed=1)
    L, D, ff = cfg.n_layer_t, cfg.d_t, cfg.ff_t
    tower = L * (4 * D * D + 2 * D * ff)
    lo = eng.lora
    assert lo.numel == L * 2 * 2 * RP * D and lo.numel < tower // 8
    for buf in (lo.p32, lo.g32, lo.m, lo.v, lo.p16, lo.p16t):
        assert buf.numel() == lo.numel
    assert all(eng.params.text[f"layer.{l}.attention.input_proj.weight"].dtype == BF for l in range(L))
    fp32_text = sum(v.numel() for k, v in eng.params.text.items() if v.dtype == torch.float32 and k.startswith("layer."))
    assert fp32_text < tower // 8                                   # biases and LayerNorms only
    assert sum(t.numel() for _, t in eng._base_t.values()) == tower and all(t.dtype == BF for _, t in eng._base_t.values())
    b = to_dev(batch)
    eng.train_step(b)                                               # make() loaded the base after construction: the first use re-made the copies
    ptrs = {k: t.data_ptr() for k, (_, t) in eng._base_t.items()}
    eng.train_step(b); eng.train_step(b)
    assert ptrs == {k: t.data_ptr() for k, (_, t) in eng._base_t.items()}
    w = "layer.1.attention.output_proj.weight"
    assert torch.equal(eng._base_wt(w), eng.params.text[w].t())
    # a loaded base (the tensors of params.text are replaced) gets fresh transposes
    eng.params.load_named_text({"text." + w: p["text." + w] * 2})
    assert torch.equal(eng._base_wt(w), eng.params.text[w].t()) and eng._base_wt(w).data_ptr() != ptrs[w]


def test_zero_b_is_the_trainable_tower_bit_for_bit():
    """peft's init (B = 0): the LoRA engine's words / txt_g equal a freeze_text=False engine's on the same weights, bit for bit."""
    _, _, _, batch, lo, _, _ = make("tiny2", 8, seed=4, n_continuation=12, random_b=False)
    _, _, _, _, tr, _, _ = make("tiny2", 8, seed=4, n_continuation=12, lora=False, freeze=False)
    b = to_dev(batch)
    lo.train_step(b, optimizer=False); tr.train_step(b, optimizer=False)
    torch.cuda.synchronize()
    assert tr.tstore is not None and lo.tstore is None
    assert torch.equal(lo.ws["words"], tr.ws["words"]) and torch.equal(lo.ws["txt_g"], tr.ws["txt_g"])
    assert float(lo.lora.gB(0).abs().max()) > 0 and float(lo.lora.gA(0).abs().max()) == 0.0     # d A = B^T ... = 0 while B = 0


def test_optimiser_steps_move_only_adapters_and_image_tower_and_track_torch_adam():
    """Three optimiser steps: the loss falls, the base text weights stay bit-identical, adapters and image tower move; the adapters follow
    torch.optim.Adam + ONE clip_grad_norm_ over image and adapter parameters on the oracle (direction cosine > 0.9)."""
    ocfg, cfg, p, batch, eng, vocab, ad = make("tiny", 8, seed=2)
    eng.cfg.lr = 1e-3
    b = to_dev(batch)
    po = {k: v.clone().requires_grad_(not k.startswith("text.")) for k, v in p.items()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in ad.items()}
    train = [v for v in po.values() if v.requires_grad] + list(leaves.values())
    opt = torch.optim.Adam(train, lr=1e-3)
    for _ in range(3):
        opt.zero_grad()
        O.model_step(batch, merged_oracle_params(po, ad, cfg, eng.lora.targets, leaves), ocfg, vocab)["loss"].backward()
        torch.nn.utils.clip_grad_norm_(train, cfg.clip)
        opt.step()
    base0 = {k: v.clone() for k, v in eng.params.text.items()}
    img0 = eng.params.p32.clone()
    losses = [float(eng.train_step(b)["loss"]) for _ in range(3)]
    torch.cuda.synchronize()
    named = eng.lora.export_named()
    for k in ("text.layer.0.attention.query.lora_A", "text.layer.0.attention.value.lora_B", "text.layer.3.attention.value.lora_A",
              "text.layer.2.attention.query.lora_B"):
        dv, do = named[k] - ad[k], leaves[k].detach() - ad[k]
        cos = float((dv * do).sum() / (dv.norm() * do.norm() + 1e-30))
        print(k, "cosine", round(cos, 4))
        assert float(dv.norm()) > 0 and cos > 0.9, (k, cos)
    for _ in range(12):
        losses.append(float(eng.train_step(b)["loss"]))
    print("losses", [round(v, 4) for v in losses[::3]])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(torch.equal(base0[k], v) for k, v in eng.params.text.items())
    assert float((eng.params.p32 - img0).abs().max()) > 0
    lo = eng.lora
    assert lo.pad_is_zero() and lo.pad_is_zero(lo.m) and lo.pad_is_zero(lo.v)
    assert torch.equal(lo.A16(0), lo.f32("layer.0.lora_A").to(BF)) and torch.equal(lo.B16t(1), lo.B16(1).t())


def test_adamw_with_groups_keeps_the_pads_at_zero():
    ocfg, cfg, p, batch, eng, vocab, ad = make("tiny", 8, seed=2, r=4)
    eng.cfg.optimizer, eng.cfg.weight_decay, eng.cfg.lr = "adamw", 0.05, 1e-3
    eng.set_optimizer_groups(text_lr_mult=2.0, no_decay_1d=True)
    before = eng.lora.p32.clone()
    for _ in range(2):
        eng.train_step(to_dev(batch))
    assert eng.lora.runs is not None and eng.lora.pad_is_zero() and float((eng.lora.p32 - before).abs().max()) > 0


def test_two_half_micro_batches_equal_one_batch():
    ocfg, cfg, p, batch, eng, vocab, ad = make("tiny2", 8, seed=5)
    b = to_dev(batch)
    eng.train_step(b, optimizer=False)
    torch.cuda.synchronize()
    g1 = eng.lora.g32.clone()
    eng.train_step(b, optimizer=False, zero_grad=True, loss_scale=0.5)
    eng.train_step(b, optimizer=False, zero_grad=False, loss_scale=0.5)
    torch.cuda.synchronize()
    e = rel(eng.lora.g32, g1)
    print("accumulated / one step", e)
    assert float(g1.abs().max()) > 0 and e < 2e-3, e


def test_lora_dropout_repeats_per_step_and_evaluation_ignores_it():
    ocfg, cfg, p, batch, eng, vocab, ad = make("tiny2", 8, seed=6, dropout=0.1)
    _, _, _, _, plain, _, _ = make("tiny2", 8, seed=6, dropout=0.0)
    b = to_dev(batch)

    def step(e, n):
        e.dropout_step = n
        e.train_step(b, optimizer=False)
        torch.cuda.synchronize()
        return e.ws["words"].clone(), e.ws["txt_g"].clone(), e.ws["t_lu1"].clone(), e.lora.g32.clone()
    a, a2, c, q = step(eng, 5), step(eng, 5), step(eng, 6), step(plain, 5)
    assert all(torch.equal(u, v) for u, v in zip(a[:3], a2[:3]))              # the same (seed, step): the same masks, the same pass
    assert rel(a2[3], a[3]) < 2e-3                                              # (the image side of the losses sums with atomics)
    assert not torch.equal(a[2], c[2]) and not torch.equal(a[0], c[0])          # another step: other masks
    assert not torch.equal(a[2], q[2]) and rel(a[0], q[0]) < 0.2                # dropout acts, mildly
    assert eng.dropout_step == 7                                                # one per train_step call: the step after the last one run
    eng.eval_step(b); plain.eval_step(b)
    torch.cuda.synchronize()
    assert torch.equal(eng.ws["words"], plain.ws["words"]) and torch.equal(eng.ws["txt_g"], plain.ws["txt_g"]) and eng.dropout_step == 7


def test_merged_tower_reproduces_the_adapted_evaluation():
    """A frozen engine loaded with merged_text_params() reproduces the LoRA engine's eval_step embeddings within 2e-2."""
    ocfg, cfg, p, batch, eng, vocab, ad = make("tiny2", 8, seed=7, r=16, targets=ALL)
    _, _, _, _, fz, _, _ = make("tiny2", 8, seed=7, lora=False)
    b = to_dev(batch)
    base = {k: v.clone() for k, v in eng.params.text.items()}
    merged = eng.merged_text_params()
    assert all(torch.equal(base[k], v) for k, v in eng.params.text.items())     # the merge works on a copy
    assert set(merged) == set(base) and not torch.equal(merged["layer.0.attention.input_proj.weight"], base["layer.0.attention.input_proj.weight"])
    fz.params.load_named_text({"text." + k: v for k, v in merged.items()})
    oe, of = eng.eval_step(b), fz.eval_step(b)
    torch.cuda.synchronize()
    e_w, e_g = rel(fz.ws["words"], eng.ws["words"]), rel(fz.ws["txt_g"], eng.ws["txt_g"])
    print(f"merged against adapted: words {e_w:.5f} txt_g {e_g:.5f}")
    assert e_w < 2e-2 and e_g < 2e-2
    assert abs(float(oe["loss"]) - float(of["loss"])) < 1e-2 * abs(float(of["loss"]))


@pytest.fixture()
def project_root(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)


def _lit(overrides):
    from medmoe_amd.hydra_lite import compose, instantiate
    cfg = compose(CONFIGS, "train.yaml", overrides)
    return cfg, instantiate(cfg.model)


def _mb(lit, B, seed):
    import bench
    b = bench.synthetic_batch(lit.model.cfg, B, seed, lit.model.device)
    b["label"] = b["label"] % lit.model.cfg.n_expert
    return {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"], "token_type": b["token_type"]}}


def _randomise_b(lit, seed=5):
    lo = lit.model.engine.lora
    g = torch.Generator().manual_seed(seed)
    lo.load_named({"text." + n: 0.05 * torch.randn(lo.D, lo.r, generator=g) for n in lo.true_names() if n.endswith("lora_B")})


def test_adapters_and_their_adam_state_travel_with_the_checkpoint(project_root, tmp_path):
    """The Hydra experiment key set builds a LoRA module; state_dict carries `...attention.{query|value}.lora_A.weight` / `lora_B.weight` in
    peft's shapes; save after step 2, load into a fresh module, step 3 equals the uninterrupted run."""
    ov = ["experiment=pretraining_medmoe_cfg2_lora", "model.model.vision.config_name=tiny2", "model.model.text.lora_dropout=0.0",
          "model.optimizer.lr=0.001"]

    def build():
        _, lit = _lit(ov)
        lit.train(); lit.configure_optimizers(); lit.configure_fused(1, 0.25)
        _randomise_b(lit)
        return lit

    def state(lit):
        return torch.cat([q.detach().float().reshape(-1) for q in lit.parameters() if q.requires_grad]), lit.model.engine.lora.p32.detach().clone()

    a = build()
    eng = a.model.engine
    assert eng.cfg.text_lora and eng.cfg.freeze_text and eng.lora is not None and eng.lora.targets == ("query", "value") and eng.lora.r == 8
    for it in range(2):
        a.training_step(_mb(a, 8, 90 + it), it)
    sd = a.state_dict()
    D = eng.cfg.d_t
    assert tuple(sd["model.text_encoder.layer.0.attention.query.lora_A.weight"].shape) == (8, D)
    assert tuple(sd["model.text_encoder.layer.1.attention.value.lora_B.weight"].shape) == (D, 8)
    assert not any(".attention.key.lora_" in k for k in sd)
    ck = {"state_dict": {k: v.detach().cpu().clone() for k, v in sd.items()}}
    a.on_save_checkpoint(ck)
    assert ck["fused_adam"]["text"]["step"] == 2 and ck["fused_adam"]["text"]["numel"] == eng.lora.numel
    path = os.path.join(str(tmp_path), "c.ckpt")
    torch.save(ck, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    r = build()
    r.load_state_dict(ck["state_dict"]); r.on_load_checkpoint(ck)
    (sa, ta), (sr, tr) = state(a), state(r)
    assert rel(sr, sa) < 1e-7 and torch.equal(tr, ta)
    b3 = _mb(a, 8, 93)
    for m in (a, r):
        m.training_step(b3, 2)
    torch.cuda.synchronize()
    (sa3, ta3), (sr3, tr3) = state(a), state(r)
    ua, ur, va, vr = sa3 - sa, sr3 - sr, ta3 - ta, tr3 - tr
    assert float(ua.norm()) > 0 and rel(ur, ua) < 2e-2, rel(ur, ua)
    assert float(va.norm()) > 0 and rel(vr, va) < 2e-2, rel(vr, va)


def test_swin_engine_step_with_adapters_against_the_autograd_mirror(project_root):
    """experiment=pretraining_medmoe_swin with text.lora: one SwinEngine step (through the shared text-arena accessor); its losses equal the
    torch-autograd mirror's on the merged text weights, and the adapters receive a gradient.  The bar is the 1e-2 of the merged-weight loss
    comparison above, not the 2e-3 of tests/test_swin_engine_gpu.py: the mirror's weight is bf16(W + s B A), rounded once more than the side
    path computes it (a bf16 ulp of W is a few per cent of an entry of s B A at these values)."""
    SWIN = ["experiment=pretraining_medmoe_swin", "model.model.text.n_layer=2"]
    _, ref = _lit(SWIN + ["model.fused_step=false"])
    _, fus = _lit(SWIN + ["model.fused_step=true", "model.model.text.lora=true", "model.model.text.lora_r=4"])
    for m in (ref, fus):
        m.model.swin.drop_path_rate = 0.0
        m.train()
    fus.configure_optimizers(); fus.configure_fused(1, 0.25)
    _randomise_b(fus)
    eng = fus.model.engine
    ref.model.engine.params.load_named_text({"text." + k: v for k, v in eng.merged_text_params().items()})
    mb = _mb(ref, 8, 40)
    with torch.no_grad():
        out_r = ref.model_step(mb)
    before = eng.lora.p32.clone()
    out_f = fus.fused_training_step(mb)
    torch.cuda.synchronize()
    for k in ("loss", "l_loss", "g_loss", "classifier_loss"):
        a, b = float(out_f[k]), float(out_r[k])
        print(k, a, b)
        assert abs(a - b) < 1e-2 * max(1.0, abs(b)), (k, a, b)
    from medmoe_amd.swin_engine import SwinEngine
    se = fus._swin_engine
    assert isinstance(se, SwinEngine) and se.optimizer_stores()["text"] is eng.lora and eng.tstore is None
    assert float(eng.lora.g32.abs().max()) > 0 and float((eng.lora.p32 - before).abs().max()) > 0 and eng.lora.pad_is_zero()


@pytest.mark.parametrize("comm,port", [("fp32", 29561), ("bf16", 29563)])
def test_two_ranks_keep_identical_replicas(comm, port):
    """tools/two_rank_lora.py: two gloo ranks on the one GPU, each a fresh child process; after two steps the replicas' adapters and image
    towers are bit-identical, with the fp32 and with the bf16 gradient exchange."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TWO_RANK_LORA_COMM=comm)
    env.pop("MEDMOE_GRAD_COMM", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "two_rank_lora.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "two-rank LoRA OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
