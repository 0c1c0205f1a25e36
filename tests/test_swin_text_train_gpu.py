"""The reference's own model (Swin-T + pyramid experts, 3136 local regions) with the text tower trained (`text.freeze_bert: false`,
text_encoder.py:27-30) through the fused step: `SwinEngine` with the word-gradient local loss, the text backward on the second stream, one clip
norm over the three arenas, Adam on the text store, gradient accumulation, checkpoints, data parallelism and the Hydra entry point."""
import os

import pytest
import torch

import medmoe_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
SWIN = ["experiment=pretraining_medmoe_swin", "model.model.text.n_layer=2"]
TEXT = ["model.model.text.freeze_bert=false"]


@pytest.fixture()
def project_root(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)


def _lit(overrides, clip=0.25):
    from medmoe_amd.hydra_lite import compose, instantiate
    cfg = compose(CONFIGS, "train.yaml", overrides)
    lit = instantiate(cfg.model)
    lit.model.swin.drop_path_rate = 0.0
    lit.train(); lit.configure_optimizers(); lit.configure_fused(1, clip)
    return cfg, lit


def _batch(lit, B, seed):
    import bench
    b = bench.synthetic_batch(lit.model.cfg, B, seed, lit.model.device)
    b["label"] = b["label"] % lit.model.cfg.n_expert
    return {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"], "token_type": b["token_type"]}}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-20))


def test_trained_text_losses_and_caption_gradients(project_root):
    """(a) the four losses equal the frozen-text run's on the same weights and batch; (b) d words / d txt_g equal the oracle losses
    differentiated at the engine's own local / global features."""
    _, fz = _lit(SWIN)
    _, tr = _lit(SWIN + TEXT)
    assert fz.model.engine.tstore is None and tr.model.engine.tstore is not None
    mb = _batch(fz, 8, 31)
    of = fz.fused_training_step(mb, optimizer_step=False)
    ot = tr.fused_training_step(mb, optimizer_step=False)
    torch.cuda.synchronize()
    for k in ("loss", "l_loss", "g_loss", "classifier_loss"):
        a, b = float(ot[k]), float(of[k])
        assert abs(a - b) < 3e-3 * max(1.0, abs(b)), (k, a, b)
    se, eng = tr._swin_engine, tr.model.engine
    c, loc = eng.cfg, se._loc
    B, HW, D = loc.B, loc.HW, loc.D
    assert loc.word_grad and se._d_words is not None
    x = loc.ctx.float().cpu().view(B, HW, D).transpose(1, 2).reshape(B, D, 56, 56)
    w = eng.ws["words"].float().cpu().transpose(1, 2).clone().requires_grad_(True)
    tg = eng.ws["txt_g"].float().cpu().clone().requires_grad_(True)
    caps = eng.cap_lens.cpu().tolist()
    l0, l1, _ = O.gloria_local(x, w, caps, c.temp1, c.temp2, c.temp3)
    (c.w_local * (l0 + l1) + c.w_global * O.gloria_global(eng.ws["img_g"].float().cpu(), tg, c.temp3)).backward()
    e_w, e_g = rel(se._d_words.transpose(1, 2), w.grad), rel(eng.ws["d_txt_g"], tg.grad)
    print(f"Swin-T trained text: d words {e_w:.4f}  d txt_g {e_g:.5f}")
    assert e_w < 2e-2 and e_g < 1e-3
    assert float(eng.tstore.g32.abs().max()) > 0


def test_trained_text_adam_step_and_accumulation(project_root):
    """(c) one optimiser step with clip 0.25: the text master moves as torch.optim.Adam on the engine's text gradient scaled by the clip
    coefficient of ALL THREE arenas; (d) two accumulated micro-batches leave the sum of the two separate text gradients."""
    hc, lit = _lit(SWIN + TEXT)
    se_batch = _batch(lit, 8, 41)
    eng = lit.model.engine
    ts = eng.tstore
    p0 = ts.p32.detach().clone()
    lit.fused_training_step(se_batch)
    torch.cuda.synchronize()
    enc = lit._swin_engine.enc
    g = ts.g32.detach().clone()
    norm = torch.sqrt(sum(st.g32.double().pow(2).sum() for st in (enc.tower.store, enc.store, ts)))
    coef = float(torch.clamp(0.25 / (norm + 1e-6), max=1.0))
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=eng.cfg.lr, weight_decay=eng.cfg.weight_decay)
    q.grad = g * coef
    opt.step()
    du, dw = ts.p32.detach() - p0, q.detach() - p0
    assert float(du.norm()) > 0 and rel(du, dw) < 1e-3, rel(du, dw)
    # (d) accumulation
    m1, m2 = _batch(lit, 8, 42), _batch(lit, 8, 43)
    lit.fused_training_step(m1, optimizer_step=False, zero_grad=True)
    g1 = ts.g32.detach().clone()
    lit.fused_training_step(m2, optimizer_step=False, zero_grad=True)
    g2 = ts.g32.detach().clone()
    lit.fused_training_step(m1, optimizer_step=False, zero_grad=True)
    lit.fused_training_step(m2, optimizer_step=False, zero_grad=False)
    torch.cuda.synchronize()
    e = rel(ts.g32, g1 + g2)
    assert float(g2.norm()) > 0 and e < 1e-4, e


def test_trained_text_adam_state_travels_with_the_checkpoint(project_root, tmp_path):
    """(e) a save after step 2, a fresh module loading it, and step 3 match the uninterrupted run - the text store included."""
    ov = SWIN + TEXT + ["model.optimizer.lr=0.001"]

    def state(lit):
        return torch.cat([p.detach().float().reshape(-1) for p in lit.parameters() if p.requires_grad]), lit.model.engine.tstore.p32.detach().clone()

    _, a = _lit(ov)
    for it in range(2):
        a.training_step(_batch(a, 8, 90 + it), it)
    ck = {"state_dict": a.state_dict()}
    a.on_save_checkpoint(ck)
    assert "text" in ck["fused_adam"] and ck["fused_adam"]["text"]["step"] == 2
    path = os.path.join(str(tmp_path), "c.ckpt")
    torch.save(ck, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    _, r = _lit(ov)
    r.load_state_dict(ck["state_dict"]); r.on_load_checkpoint(ck)
    sa, ta = state(a)
    sr, tr = state(r)
    assert rel(sr, sa) < 1e-7 and rel(tr, ta) < 1e-2          # the text checkpoint holds the bf16 working copies of the GEMM weights
    b3 = _batch(a, 8, 93)
    for m in (a, r):
        m.training_step(b3, 2)
    torch.cuda.synchronize()
    sa3, ta3 = state(a)
    sr3, tr3 = state(r)
    ua, ur = sa3 - sa, sr3 - sr
    assert float(ua.norm()) > 0 and rel(ur, ua) < 2e-2, rel(ur, ua)
    va, vr = ta3 - ta, tr3 - tr
    assert float(va.norm()) > 0 and rel(vr, va) < 2e-2, rel(vr, va)


def test_two_ranks_step_the_reference_model_with_the_text_tower():
    """(f) tools/two_rank_swin_text.py: two gloo ranks on one GPU - bit-identical replicas in all three arenas, the text gradient = the mean
    of the two ranks'."""
    import subprocess
    import sys
    env = dict(os.environ, PROJECT_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "two_rank_swin_text.py")], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TWO_RANK_SWIN_TEXT_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_train_py_trains_the_text_tower_of_the_reference_model(tmp_path):
    """`src/train.py experiment=pretraining_medmoe_swin model.model.text.freeze_bert=false`: one epoch on synthetic shards; the checkpoint's
    text_encoder.* weights differ from a fresh module's."""
    import subprocess
    import sys
    env = dict(os.environ)
    env.pop("PROJECT_ROOT", None)
    cmd = [sys.executable, os.path.join(ROOT, "src", "train.py"), "experiment=pretraining_medmoe_swin", "model.model.text.freeze_bert=false",
           "model.model.vision.num_experts=3", "model.model.text.n_layer=2", "data.synthetic_size=32", "data.synthetic_classes=3",
           "data.batch_size=8", "data.num_workers=0", "trainer.max_epochs=1", "extras.print_config=false",
           f"callbacks.model_checkpoint.dirpath={tmp_path}/ckpt", "+optimized_metric=train/loss"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    sd = torch.load(os.path.join(str(tmp_path), "ckpt", "last.ckpt"), map_location="cpu", weights_only=True)["state_dict"]
    os.environ["PROJECT_ROOT"] = ROOT
    try:
        from medmoe_amd.hydra_lite import compose, instantiate
        fresh = instantiate(compose(CONFIGS, "train.yaml", SWIN + TEXT + ["model.model.vision.num_experts=3"]).model)
    finally:
        os.environ.pop("PROJECT_ROOT", None)
    f = fresh.state_dict()
    keys = [k for k in sd if k.startswith("model.text_encoder.")]
    assert keys and all(k in f for k in keys)
    moved = [k for k in keys if float((sd[k].float() - f[k].float().cpu()).abs().max()) > 0]
    assert "model.text_encoder.layer.0.attention.input_proj.weight" in moved and len(moved) > len(keys) // 2, (len(moved), len(keys))
