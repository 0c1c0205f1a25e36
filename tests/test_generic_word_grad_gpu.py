"""Word gradient of the generic-geometry GLoRIA local loss (`GenericLocalLoss(word_grad=True)`, loss.hip `medmoe_local_gen_dwords`): the
3136 regions of the Swin-T stage-0 map, the 576 of ViT-L/14 at 336 px, a padded 10 x 10 map - against the fp32 autograd of the oracle's local
loss with respect to the words; and the engine on that path (`freeze_text = False` at 576 and 256 regions) against the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import medmoe_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _inputs(B, side, T, D, seed):
    g = torch.Generator().manual_seed(seed)
    img = (torch.randn(B, D, side, side, generator=g) * 0.2).to(BF).float()
    words = (torch.randn(B, D, T, generator=g) * 0.2).to(BF).float()
    caps = [T, 7, 13, 4, 20, 11, T, 2][:B]
    return img, words, caps


def _run(B, HW, T, D, ctx16, words16, cap, word_grad, gsim=None):
    from medmoe_amd.local_generic import GenericLocalLoss
    loss = GenericLocalLoss(B, HW, T, D, "cuda", word_grad=word_grad)
    sim = loss.forward(ctx16, words16, cap, 4.0, 5.0).clone()
    if gsim is None:                                          # d (CE rows + CE columns of 10 * sim) / d sim
        s = sim.detach().clone().requires_grad_(True)
        lab = torch.arange(B, device="cuda")
        (F.cross_entropy(10.0 * s, lab) + F.cross_entropy(10.0 * s.t(), lab)).backward()
        gsim = s.grad.contiguous()
    return loss, sim, gsim, loss.backward(gsim)


@pytest.mark.parametrize("B,side,D", [(4, 56, 768), (8, 24, 768), (8, 10, 768), (8, 10, 128)])
def test_word_gradient_against_the_oracle(B, side, D):
    """d words against the fp32 autograd of O.gloria_local; exact zeros at t >= cap; d ctx bit-identical to the frozen-text mode (dense
    branch at 3136 / 576 regions, padded branch at 100)."""
    T, HW = 25, side * side
    img, words, caps = _inputs(B, side, T, D, 11 + side)
    w = words.clone().requires_grad_(True)
    l0, l1, _ = O.gloria_local(img, w, caps, 4.0, 5.0, 10.0)
    (l0 + l1).backward()
    ctx16 = img.reshape(B, D, HW).transpose(1, 2).contiguous().view(B * HW, D).to(BF).cuda()
    words16 = words.transpose(1, 2).contiguous().to(BF).cuda()
    cap = torch.tensor(caps, dtype=torch.int32, device="cuda")
    _, sim0, gsim, dctx0 = _run(B, HW, T, D, ctx16, words16, cap, False)
    lw, sim1, _, (dctx1, dw) = _run(B, HW, T, D, ctx16, words16, cap, True, gsim)
    torch.cuda.synchronize()
    assert lw.dense == (HW % 16 == 0)
    assert torch.equal(sim0, sim1)
    assert torch.equal(dctx0, dctx1)
    assert dw.shape == (B, T, D) and dw.dtype == torch.float32 and bool(torch.isfinite(dw).all())
    for i, c in enumerate(caps):
        assert float(dw[i, c:].abs().max()) == 0.0 if c < T else True
    e = rel(dw.transpose(1, 2), w.grad)
    print(f"B={B} HW={HW} D={D}: d words rel-L2 {e:.4f}")
    assert e < 2e-2, e


def test_word_gradient_is_reproducible_on_the_staged_path():
    """576 regions at B = 8 (Kp = 256, D = 768): the dS^T ctx GEMM runs in its staged form and the new kernel sums the images in a fixed
    order - two backward passes of the same forward give the same bits."""
    B, side, T, D = 8, 24, 25, 768
    HW = side * side
    img, words, caps = _inputs(B, side, T, D, 5)
    ctx16 = img.reshape(B, D, HW).transpose(1, 2).contiguous().view(B * HW, D).to(BF).cuda()
    words16 = words.transpose(1, 2).contiguous().to(BF).cuda()
    cap = torch.tensor(caps, dtype=torch.int32, device="cuda")
    lw, _, gsim, (_, dw1) = _run(B, HW, T, D, ctx16, words16, cap, True)
    assert lw.tn_scratch is not None
    lw.forward(ctx16, words16, cap, 4.0, 5.0)
    _, dw2 = lw.backward(gsim)
    torch.cuda.synchronize()
    assert torch.equal(dw1, dw2)


def test_generic_and_transposed_word_gradients_agree():
    """196 regions (B = 8): the two independent formulations of d words - generic (dS^T ctx + cosine term over WC) and transposed pair3
    (row-major pair matrices, one NT GEMM + word-norm term) - agree."""
    from medmoe_amd.local_transposed import TransposedLocalLoss
    B, side, T, D = 8, 14, 25, 768
    HW = side * side
    img, words, caps = _inputs(B, side, T, D, 3)
    ctx16 = img.reshape(B, D, HW).transpose(1, 2).contiguous().view(B * HW, D).to(BF).cuda()
    words16 = words.transpose(1, 2).contiguous().to(BF).cuda()
    cap = torch.tensor(caps, dtype=torch.int32, device="cuda")
    _, sim_g, gsim, (_, dw_g) = _run(B, HW, T, D, ctx16, words16, cap, True)
    tl = TransposedLocalLoss.standalone(B, HW, T, D, "cuda", word_grad=True)
    sim_t = tl.forward(ctx16, words16, cap, np.asarray(caps), 4.0, 5.0).clone()
    d_img = torch.empty(B, HW, D, device="cuda", dtype=BF)
    dw_t = tl.backward(gsim, d_img)
    torch.cuda.synchronize()
    assert rel(sim_g, sim_t) < 1e-2
    e = rel(dw_g, dw_t)
    print(f"generic vs transposed d words: {e:.4f}")
    assert e < 2e-2, e


def bf_round(t):
    return t.to(torch.bfloat16).float()


def _make(cfg_name, B, seed):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine, VocabTables
    ocfg, cfg = O.config_by_name(cfg_name), config_by_name(cfg_name)
    ocfg.freeze_text = cfg.freeze_text = False
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
    eng = Engine(cfg, "cuda:0", vocab=VocabTables.synthetic(cfg.vocab, "cuda:0", 0))
    eng.params.load_named({k: v for k, v in p.items() if not k.startswith("text.")})
    eng.tstore.load_named(p)
    return ocfg, cfg, p, batch, eng, O.Vocab.synthetic(ocfg.vocab, 0)


@pytest.mark.parametrize("cfg_name", ["tinyL336", "tinyL"])
def test_engine_trains_the_text_tower_at_generic_geometries(cfg_name):
    """tinyL336 (576 regions) and tinyL (256 regions) with freeze_text = False run the generic word-gradient path: (1) losses against the
    oracle; (2) d words / d txt_g against the oracle's losses differentiated at the engine's own features; (3) those gradients through the
    oracle's text graph give every text parameter's gradient (the bars of test_text_train_gpu.py)."""
    B = 8
    ocfg, cfg, p, batch, eng, vocab = _make(cfg_name, B, seed=4)
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    ref = O.model_step(batch, pr, ocfg, vocab)
    out = eng.train_step({k: v.cuda() for k, v in batch.items()}, optimizer=False)
    torch.cuda.synchronize()
    from medmoe_amd.local_generic import GenericLocalLoss
    assert type(eng._local) is GenericLocalLoss and eng._local.word_grad and eng._d_words is not None
    for k in ("g_loss", "l_loss"):
        assert abs(out[k].item() - ref[k].item()) < 1e-2 * abs(ref[k].item()), (k, out[k].item(), ref[k].item())
    P, Do, Hh = cfg.n_patch, cfg.d_out, int(cfg.n_patch ** 0.5)
    x = eng.ws["img_l"].float().cpu().transpose(1, 2).reshape(B, Do, Hh, Hh)
    w = eng.ws["words"].float().cpu().transpose(1, 2).clone().requires_grad_(True)
    tg = eng.ws["txt_g"].float().cpu().clone().requires_grad_(True)
    l0, l1, _ = O.gloria_local(x, w, ref["cap_lens"], ocfg.temp1, ocfg.temp2, ocfg.temp3)
    (ocfg.w_local * (l0 + l1) + ocfg.w_global * O.gloria_global(eng.ws["img_g"].float().cpu(), tg, ocfg.temp3)).backward()
    e_w = rel(eng._d_words.transpose(1, 2), w.grad)
    e_g = rel(eng.ws["d_txt_g"], tg.grad)
    print(f"{cfg_name}: d words {e_w:.4f}  d txt_g {e_g:.5f}")
    assert e_w < 2e-2 and e_g < 1e-3
    got = eng.tstore.export_named(eng.tstore.g32)
    for v in pr.values():
        v.grad = None
    word_o, sent_o, _ = O.text_tower(batch["ids"], batch["attn_mask"], batch["token_type"], pr, ocfg, vocab)
    ((word_o * eng._d_words.cpu().transpose(1, 2)).sum() + (sent_o * eng.ws["d_txt_g"].cpu()).sum()).backward()
    errs = {}
    for k, v in pr.items():
        if k.startswith("text.") and v.grad is not None and float(v.grad.norm()) > 1e-9:
            errs[k] = rel(got[k].reshape(v.grad.shape), v.grad)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    print("text backward worst", [(k, round(e, 4)) for k, e in worst], "median", float(np.median(list(errs.values()))))
    assert len(errs) == 5 + 12 * ocfg.n_layer_t
    assert max(errs.values()) < 6e-2 and float(np.median(list(errs.values()))) < 2e-2, worst
