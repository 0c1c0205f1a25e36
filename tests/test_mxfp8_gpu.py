"""MXFP8 expert path (medmoe_amd/csrc/mxfp8.hip): the quantisers bit-exact against the torch twin of tests/test_mxfp8_host.py, the
operand / scale layout of the block-scaled MFMA pinned with exact integer data, the grouped GEMM against the fp32 product of the
dequantised operands, its fused quantised output, the engine at tinyL8mx against the oracle with the twin patched in, the Hydra
key through one fused training step."""
import os

import numpy as np
import pytest
import torch

import medmoe_oracle as O
from test_mxfp8_host import edge_rows, fake_quant_mx, mx_dequant, mx_quant

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8 = torch.uint8


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _tiles(counts, dev):
    tl, start = [], 0
    for g, c in enumerate(counts):
        for m in range(start, start + c, 128):
            tl.append([g, m, start + c, 0])
        start += c
    return torch.tensor(tl, device=dev, dtype=torch.int32).reshape(-1, 4), torch.tensor([len(tl)], device=dev, dtype=torch.int32)


def _grouped_ref(a, b, counts, bias=None, epi=0, res=None, aux=None):
    ref = torch.zeros(a.shape[0], b.shape[1], device=a.device); start = 0
    for g, cc in enumerate(counts):
        z = a[start:start + cc] @ b[g].t()
        if bias is not None:
            z = z + bias[g]
        if epi == 1:
            z = torch.relu(z)
        if epi == 2:
            z = (z + res[start:start + cc].float()) * (aux[start:start + cc].float() > 0)
        ref[start:start + cc] = z; start += cc
    return ref


@pytest.mark.parametrize("K", [64, 192, 1024])
def test_row_quantiser_bit_exact(K):
    """Plain and gathered rows; an all-zero row, one huge element in an otherwise small block, amax / 448 exactly a power of two and one
    bf16 step above it (edge_rows); K = 64: most lanes of the wave idle, K = 1024: two passes per row."""
    from medmoe_amd import ops
    torch.manual_seed(0)
    M = 300
    x = (torch.randn(M + 50, K, device="cuda") * torch.rand(M + 50, 1, device="cuda") * 4).to(torch.bfloat16)
    x[:5] = edge_rows(K).cuda().to(torch.bfloat16)
    rowmap = torch.randperm(M + 50, device="cuda")[:M].int()
    rowmap[:5] = torch.tensor([4, 3, 2, 1, 0], dtype=torch.int32)
    for use_map in (False, True):
        q = torch.full((M, K), 0xAB, device="cuda", dtype=U8); s = torch.full((M, K // 32), 0xCD, device="cuda", dtype=U8)
        ops.call("quant_rows_mx", x, K, rowmap if use_map else None, q, s, M, K)
        q_ref, s_ref = mx_quant(x[rowmap.long()] if use_map else x[:M])
        assert torch.equal(s, s_ref), int((s != s_ref).sum())
        assert torch.equal(q, q_ref), int((q != q_ref).sum())


def test_weight_quantiser_bit_exact_both_copies():
    """The forward copy (blocks along K) and the dgrad copy (the transposed matrix quantised AGAIN with blocks along N - not a byte
    transpose) with both scale arrays."""
    from medmoe_amd import ops
    torch.manual_seed(1)
    G, N, K = 3, 64, 96
    w = torch.randn(G, N, K, device="cuda") * 0.05 * (1 + 10 * torch.rand(G, N, 1, device="cuda"))
    w[1, :, 32:64] = 0                      # all-zero blocks in both directions
    w[2, 7, 3] = 0.0625 * 448; w[2, 7, :3] = 0.01; w[2, 7, 4:32] = -0.02          # exact power of two along K
    q = torch.empty(G, N, K, device="cuda", dtype=U8); sq = torch.empty(G, N, K // 32, device="cuda", dtype=U8)
    qT = torch.empty(G, K, N, device="cuda", dtype=U8); sT = torch.empty(G, K, N // 32, device="cuda", dtype=U8)
    ops.call("quant_weights_mx", w, q, sq, qT, sT, G, N, K)
    q_ref, s_ref = mx_quant(w)
    qT_ref, sT_ref = mx_quant(w.transpose(1, 2).contiguous())
    assert torch.equal(sq, s_ref) and torch.equal(q, q_ref) and int(s_ref[2, 7, 0]) == 123
    assert torch.equal(sT, sT_ref) and torch.equal(qT, qT_ref)
    assert not torch.equal(qT, q.transpose(1, 2))


def test_gemm_mx_layout_pin():
    """The probe of the block-scaled MFMA's operand layout, kept as a test: small integers, an asymmetric B, and a power-of-two scale
    2^j that differs for every (row, 32-block) of A and of B.  Every partial sum is an integer multiple of 2^-3 below 2^15, exact in
    fp32, so the bf16 output must equal the bf16 rounding of the exact product: any mix-up of fragment order, of the k order inside a
    lane (one run of 32 bytes or two of 16), or of which lane's scale byte belongs to which (row, block) gives a different number."""
    from medmoe_amd import ops
    dev = "cuda"
    counts = [300, 0, 129, 77]
    M, N, K, G = sum(counts), 200, 256, len(counts)
    tiles, cnt = _tiles(counts, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    a = torch.randint(-4, 5, (M, K), device=dev, generator=gen).float(); b = torch.randint(-3, 4, (G, N, K), device=dev, generator=gen).float()
    m_i = torch.arange(M, device=dev)[:, None]; n_i = torch.arange(N, device=dev)[None, :, None]
    kb = torch.arange(K // 32, device=dev); g_i = torch.arange(G, device=dev)[:, None, None]
    ja = (m_i * 3 + kb[None, :] * 2) % 5 - 2                              # -2..2, varies over rows and blocks
    jb = (n_i * 2 + kb[None, None, :] + g_i) % 3 - 1                  # -1..1
    sa = (127 + ja).to(U8); sb = (127 + jb).to(U8)
    c = torch.full((M, N), 7.0, device=dev, dtype=torch.bfloat16)
    ops.call("gemm_mx_grouped", a.to(F8).view(U8), sa, b.to(F8).view(U8), sb.contiguous(), None, c, N, None, None, None, None,
             tiles, cnt, tiles.shape[0], N, K, N * K, N * (K // 32), 0, 0)
    ad = mx_dequant(a.to(F8).view(U8), sa); bd = mx_dequant(b.to(F8).view(U8), sb.contiguous())
    ref = torch.zeros(M, N, device=dev, dtype=torch.float64); start = 0
    for g, cc in enumerate(counts):
        ref[start:start + cc] = ad[start:start + cc].double() @ bd[g].double().t(); start += cc
    assert float(ref.abs().max()) < 2 ** 15
    want = ref.float().to(torch.bfloat16).float()
    assert torch.equal(c.float(), want), (int((c.float() != want).sum()), c[:2, :8], want[:2, :8])


@pytest.mark.parametrize("K", [64, 128, 192, 1024])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_mx_grouped(epi, K):
    """Random e4m3 data and random scale bytes against the fp32 product of the dequantised operands: ragged groups (one empty), N not
    a multiple of the tile, K below / equal to / not a multiple of / many times the k-step of 128, every epilogue.  Bar 4e-3: one bf16
    rounding of the output plus fp32 summation order (the bar of tests/test_fp8_gpu.py for the same comparison)."""
    from medmoe_amd import ops
    dev = "cuda"
    counts = [300, 0, 129, 77]
    M, N, G = sum(counts), 200, len(counts)
    tiles, cnt = _tiles(counts, dev)
    gen = torch.Generator(device=dev).manual_seed(3 + K)
    aq = (torch.randn(M, K, device=dev, generator=gen) * 100).clamp(-448, 448).to(F8).view(U8)
    bq = (torch.randn(G, N, K, device=dev, generator=gen) * 100).clamp(-448, 448).to(F8).view(U8)
    sa = torch.randint(113, 123, (M, K // 32), device=dev, generator=gen).to(U8); sb = torch.randint(114, 124, (G, N, K // 32), device=dev, generator=gen).to(U8)
    bias = torch.randn(G, N, device=dev, generator=gen) * 0.1
    res = torch.randn(M, N, device=dev, generator=gen).to(torch.bfloat16); aux = torch.randn(M, N, device=dev, generator=gen).to(torch.bfloat16)
    c = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
    ops.call("gemm_mx_grouped", aq, sa, bq, sb, bias if epi < 2 else None, c, N, res if epi == 2 else None, aux if epi == 2 else None, None, None,
             tiles, cnt, tiles.shape[0], N, K, N * K, N * (K // 32), N if epi < 2 else 0, epi)
    ref = _grouped_ref(mx_dequant(aq, sa), mx_dequant(bq, sb), counts, bias if epi < 2 else None, epi, res, aux)
    err = rel(c, ref)
    print(f"gemm_mx_grouped epi {epi} K {K}: relative L2 {err:.3e}")
    assert err < 4e-3


def test_gemm_mx_fused_quantised_output():
    """The ReLU epilogue's second output equals medmoe_quant_rows_mx (and the twin) of the bf16 output, bit for bit; N = 192: one full
    and one half column tile."""
    from medmoe_amd import ops
    dev = "cuda"
    counts = [300, 0, 129, 77]
    M, N, K, G = sum(counts), 192, 128, len(counts)
    tiles, cnt = _tiles(counts, dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    aq, sa = mx_quant(torch.randn(M, K, device=dev, generator=gen) * torch.rand(M, 1, device=dev, generator=gen) * 3)
    bq, sb = mx_quant(torch.randn(G, N, K, device=dev, generator=gen) * 0.05)
    bias = torch.randn(G, N, device=dev, generator=gen) * 0.1
    bias[:, 64:96] = -1e3                                                 # a 32-block that ReLU turns into zeros: scale byte 127
    c = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
    cq = torch.full((M, N), 0xAB, device=dev, dtype=U8); cs = torch.full((M, N // 32), 0xCD, device=dev, dtype=U8)
    ops.call("gemm_mx_grouped", aq, sa, bq, sb, bias, c, N, None, None, cq, cs, tiles, cnt, tiles.shape[0], N, K, N * K, N * (K // 32), N, 1)
    ref = _grouped_ref(mx_dequant(aq, sa), mx_dequant(bq, sb), counts, bias, 1)
    assert rel(c, ref) < 4e-3
    q2 = torch.empty(M, N, device=dev, dtype=U8); s2 = torch.empty(M, N // 32, device=dev, dtype=U8)
    ops.call("quant_rows_mx", c, N, None, q2, s2, M, N)
    assert torch.equal(cs, s2) and torch.equal(cq, q2) and (cs[:, 2] == 127).all()
    qt, st = mx_quant(c)
    assert torch.equal(cs, st) and torch.equal(cq, qt)


MX_PROJ = [f"moe.proj.{s}.weight" for s in range(4)] + ["moe.attn0.weight"]


def _assert_mx_copies_are_the_twin(params):
    for name in MX_PROJ:
        w = params.f32(name)
        q, sq = params.qmx(name); qT, sT = params.qmxt(name)
        q_ref, s_ref = mx_quant(w)
        qT_ref, sT_ref = mx_quant(w.transpose(1, 2).contiguous())
        assert torch.equal(q, q_ref) and torch.equal(sq, s_ref) and torch.equal(qT, qT_ref) and torch.equal(sT, sT_ref), name


def test_engine_with_mx_expert_weights_vs_oracle_twin(monkeypatch):
    """tinyL8mx = BASELINE configs[4]'s token geometry with MXFP8 expert weights at unit-test width, against the oracle's tinyL8 with
    its fake_quant_rows swapped for the MX twin (blocks of 32 along the last dimension, straight-through gradients): the oracle looks
    the function up when expert_forward runs.  As in tests/test_fp8_gpu.py the engine quantises bf16 activations (the fp32 oracle has
    no such rounding), and its backward also quantises the gradient rows entering the two dgrad products, which the oracle's
    straight-through backward does not.
    Measured on the MI355X (engine against twin, relative): img_l 1.113e-2, img_g 8.26e-4, g_loss 4.35e-6, l_loss 2.32e-4; gradients:
    median 1.12e-2, worst tensor 0.116, worst scale-attention MLP tensor 0.266; the bf16-expert oracle differs from the twin by
    2.148e-2 in img_l.  Every bar below is at most twice the measured value and none is looser than the e4m3 test's (outputs 3e-2,
    losses 1.5e-2, gradient median 3e-2, per tensor 0.12, scale-attention MLP 0.35)."""
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    monkeypatch.setattr(O, "fake_quant_rows", fake_quant_mx)
    B = 8
    ocfg, cfg = O.config_by_name("tinyL8"), config_by_name("tinyL8mx")
    assert ocfg.expert_fp8 and cfg.expert_mx and not cfg.expert_fp8
    p = O.init_params(ocfg, seed=3, std=0.05)
    g = torch.Generator().manual_seed(10)
    for k in p:
        if k.endswith("layernorm.weight") or k.endswith("layer_norm.weight"):
            p[k] = 1 + 0.2 * torch.randn(p[k].shape, generator=g)
        elif k.endswith(".bias"):
            p[k] = 0.05 * torch.randn(p[k].shape, generator=g)
    p["moe.router.0.weight"] *= 8.0; p["moe.router.2.weight"] *= 8.0
    for k in p:      # GEMM weights the engine keeps in bf16 are rounded for the oracle too; the EXPERT projections stay fp32 masters
        if k.endswith(".weight") and p[k].dim() >= 2 and not k.startswith("moe.") and "embeddings" not in k:
            p[k] = p[k].to(torch.bfloat16).float()
    batch = O.synthetic_batch(ocfg, B, min_len=4)
    batch["image"] = batch["image"].to(torch.bfloat16).float()
    eng = Engine(cfg, "cuda:0")
    eng.params.load_named(p)
    _assert_mx_copies_are_the_twin(eng.params)
    vocab = O.Vocab.synthetic(ocfg.vocab)
    pr = {k: v.clone().requires_grad_(not k.startswith("text.")) for k, v in p.items()}
    ref = O.model_step(batch, pr, ocfg, vocab)
    out_l = eng.train_step({k: v.cuda() for k, v in batch.items()}, optimizer=False)
    torch.cuda.synchronize()
    out = eng.outputs()
    assert torch.equal(out["idx"].cpu().long(), ref["idx"])
    e_l, e_g = rel(out["img_l"], ref["img_l"]), rel(out["img_g"], ref["img_g"])
    e_loss = {k_: abs(out_l[k_].item() - ref[k_].item()) / abs(ref[k_].item()) for k_ in ("g_loss", "l_loss")}
    ocfg16 = O.config_by_name("tinyL")
    with torch.no_grad():
        ref16 = O.model_step(batch, p, ocfg16, vocab)
    d16 = rel(ref16["img_l"], ref["img_l"])
    print(f"mx engine vs twin: img_l {e_l:.3e} img_g {e_g:.3e} losses {e_loss}; bf16-expert oracle vs twin img_l {d16:.3e}")
    # measured: img_l 1.113e-2, img_g 8.26e-4, g_loss 4.35e-6, l_loss 2.32e-4 (relative)
    BAR_L, BAR_G, BAR_LOSS = 2e-2, 1.6e-3, {"g_loss": 8.5e-6, "l_loss": 4.5e-4}
    assert e_l < BAR_L and e_g < BAR_G
    for k_, e_ in e_loss.items():
        assert e_ < BAR_LOSS[k_], (k_, e_)
    # the bf16-expert oracle must differ from the twin by more than the bar (2.148e-2: the test would otherwise not see the quantisation at all)
    assert d16 > BAR_L
    # backward: engine's loss gradients and router-input gradient through the twin's graph (tests/test_engine_gpu.py stage 3)
    P, Do = cfg.n_patch, cfg.d_out
    last, hs = O.vit_forward(batch["image"], pr, ocfg)
    router_in = last[:, 1:, :].mean(dim=1)
    feats = [hs[l][:, 1:, :] for l in ocfg.stage_layers()]
    img_g2, img_l2, _, _ = O.moe_forward(feats, router_in.detach(), pr, ocfg.n_expert, ocfg.top_k, True)
    obj = (img_g2 * eng.ws["d_img_g"].cpu()).sum() + (img_l2.reshape(B, Do, P) * eng.ws["d_img_l"].float().cpu().transpose(1, 2)).sum() \
        + (router_in * eng.ws["drouter_in"].cpu()).sum()
    obj.backward()
    got = eng.params.export_named(eng.params.g32)
    errs = {}
    for k, v in pr.items():
        if k.startswith("text.") or k.startswith("moe.router") or v.grad is None or v.grad.norm() < 1e-7:
            continue
        errs[k] = rel(got[k].reshape(v.grad.shape), v.grad)
    med = float(np.median(list(errs.values())))
    worst_attn = max((e for k, e in errs.items() if "attn_proj" in k), default=0.0)
    worst_rest = max((e for k, e in errs.items() if "attn_proj" not in k), default=0.0)
    print("mx worst grads:", sorted(errs.items(), key=lambda kv: -kv[1])[:8], "median", med, "worst attn_proj", worst_attn, "worst other", worst_rest)
    # measured: median 1.12e-2; worst tensor outside the scale-attention MLP 0.116 (moe.experts.2.proj_convs.0.0.weight); worst inside it
    # 0.266 (moe.experts.0.attn_proj.0.bias: a sum of ReLU-masked terms whose mask flips where an e4m3 neighbour was picked).  The last two
    # bars are the e4m3 test's caps, both below twice the measured value.
    BAR_MED, BAR_TENSOR, BAR_ATTN = 2.2e-2, 0.12, 0.35
    assert med < BAR_MED
    bad = {k: e for k, e in errs.items() if e > (BAR_ATTN if "attn_proj" in k else BAR_TENSOR)}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:10]
    # one optimiser step re-derives every MX copy and scale array from the updated master, and changes them
    before = [t.clone() for name in MX_PROJ for t in eng.params.qmx(name) + eng.params.qmxt(name)]
    eng.cfg.lr = 1e-2
    eng.train_step({k: v.cuda() for k, v in batch.items()})
    torch.cuda.synchronize()
    _assert_mx_copies_are_the_twin(eng.params)
    after = [t for name in MX_PROJ for t in eng.params.qmx(name) + eng.params.qmxt(name)]
    assert all(not torch.equal(a_, b_) for a_, b_ in zip(after[0::2], before[0::2]))      # every element array moved


def test_mxfp8_experiment_runs_a_fused_training_step(monkeypatch):
    """`experiment=pretraining_medmoe_cfg4_mx` (vision.expert_dtype: mxfp8) through the Hydra chain: the key reaches the engine
    configuration, and the module built from the experiment at a unit-test geometry takes fused training steps on the MX path."""
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    import bench
    from medmoe_amd.hydra_lite import compose, instantiate
    from src.models.components.med_moe import config_from_hydra
    configs = os.path.join(ROOT, "configs")
    full = compose(configs, "train.yaml", ["experiment=pretraining_medmoe_cfg4_mx"]).model.model
    assert full.vision.expert_dtype == "mxfp8" and config_from_hydra(full.vision, full.text).expert_mx
    cfg = compose(configs, "train.yaml", ["experiment=pretraining_medmoe_cfg4_mx", "model.model.vision.config_name=tinyL8mx", "model.optimizer.lr=0.001"])
    lit = instantiate(cfg.model)
    assert lit.fused_step and lit.model.cfg.expert_mx and lit.model.engine.cfg.expert_mx
    lit.configure_optimizers()
    lit.configure_fused(cfg.trainer.accumulate_grad_batches, cfg.trainer.gradient_clip_val)
    eng = lit.model.engine
    p0 = lit.model.weights.detach().clone()
    q0 = eng.params.qmx("moe.attn0.weight")[0].clone()
    b = bench.synthetic_batch(eng.cfg, 8, 21, eng.device)
    mb = {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"]}}
    losses = [float(lit.training_step(mb, it)) for it in range(2)]
    torch.cuda.synchronize()
    assert all(np.isfinite(l) and l > 0 for l in losses), losses
    assert float((lit.model.weights.detach() - p0).abs().max()) > 0
    assert torch.isfinite(lit.model.weights.detach()).all()
    assert not torch.equal(eng.params.qmx("moe.attn0.weight")[0], q0)
    _assert_mx_copies_are_the_twin(eng.params)
