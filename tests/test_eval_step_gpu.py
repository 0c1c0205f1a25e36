"""The fused evaluation step: `medmoe_local_sim_fwd` (csrc/local_eval.hip - the local similarity forward only, a pair's scores and attention
never leave the chip), `Engine.eval_step`, and the module / trainer hooks on top of it (reference medmoe_module.py:114-134)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
TEMP1, TEMP2, TEMP3 = 4.0, 5.0, 10.0

# Maximum absolute error of the EXISTING path's similarity matrix (`TransposedLocalLoss.forward`: fp16 log-probabilities and bf16 attention
# through HBM) against oracle.medmoe_oracle.gloria_local_sim in fp32 on the same bf16-rounded inputs, measured once on an MI355X
# (`python tools/bench_eval.py --part sim-error`; profiles/r05_notes.md) ...
OLD_SIM_ERR = {"fixture64": 1.558e-3, "seeded196": 1.422e-3}      # |sim| up to 4.3 / 4.9; the new kernel measured 9.98e-4 / 7.50e-4
# ... and the new kernel's bar: twice that (a bar does not sit on the noise floor of the number formats).  The kernel
# keeps the scores in fp32, so it is expected under the old error, not over it.
SIM_BAR = {k: 2.0 * v for k, v in OLD_SIM_ERR.items()}                  # 3.116e-3 / 2.844e-3


def fixture_case(golden_dir):
    """The reference's own local-loss fixture: 64 regions, width 128, captions of at most 16 words (B == Bc)."""
    d = np.load(os.path.join(golden_dir, "gloria_local_mfma.npz"))
    img = torch.from_numpy(np.asarray(d["img_l"])).float()                   # [B, D, 8, 8]
    words = torch.from_numpy(np.asarray(d["words"])).float()                 # [B, D, T]
    caps = [int(v) for v in d["cap_lens"]]
    return img, words, caps, float(d["loss0"]), float(d["loss1"])


def seeded_case():
    """196 regions, 4 images against 84 captions (Bc != B) of up to T = 77 words: the lengths hold both edges of every length class 1..5
    (1, 16 | 17, 32 | 33, 48 | 49, 64 | 65, 77), every class has more members than one workgroup takes per iteration at one chunk, and
    twenty short captions make class 1 longer than its 16 per iteration.  bf16-representable values."""
    g = torch.Generator().manual_seed(1234)
    B, P, D, T = 4, 196, 128, 77
    lens = [1, 16, 17, 32, 33, 64, 65, T, 8, 48, 49, 70]
    lens += [int(v) for v in torch.randint(1, T + 1, (52,), generator=g)] + [int(v) for v in torch.randint(1, 17, (20,), generator=g)]
    img = (0.3 * torch.randn(B, D, 14, 14, generator=g)).to(BF).float()
    words = (0.3 * torch.randn(len(lens), D, T, generator=g)).to(BF).float()
    assert img.shape[2] * img.shape[3] == P
    return img, words, lens


def oracle_sim(img, words, caps):
    from oracle.medmoe_oracle import gloria_local_sim
    return gloria_local_sim(img, words, caps, TEMP1, TEMP2)[0]


def device_inputs(img, words, caps):
    B, D = img.shape[:2]
    ctx = img.reshape(B, D, -1).transpose(1, 2).contiguous().view(-1, D).to("cuda", BF)         # [B*P, D]
    w = words.transpose(1, 2).contiguous().to("cuda", BF)                                        # [Bc, T, D]
    return ctx, w, torch.tensor(caps, device="cuda", dtype=I32)


def old_sim(img, words, caps):
    """The training path's forward launches (score GEMM + pair3 forward) on the same inputs."""
    from medmoe_amd.local_transposed import TransposedLocalLoss
    ctx, w, cl = device_inputs(img, words, caps)
    B, P, (Bc, T, D) = img.shape[0], img.shape[2] * img.shape[3], w.shape
    tl = TransposedLocalLoss.standalone(B, P, T, D, "cuda", Bc=Bc)
    return tl.forward(ctx, w, cl, np.asarray(caps), TEMP1, TEMP2).clone()


def new_sim(img, words, caps, chunks=0):
    from medmoe_amd import ops
    from medmoe_amd.local_transposed import local_sim_forward
    ctx, w, cl = device_inputs(img, words, caps)
    B, P, (Bc, T, D) = img.shape[0], img.shape[2] * img.shape[3], w.shape
    GR = (P + 31) // 32 * 32
    arg = torch.arange(B * P, device="cuda")
    tl = [[b, m, (b + 1) * P, 0] for b in range(B) for m in range(b * P, (b + 1) * P, 128)]
    bufs = dict(P=P, gm3=torch.zeros(B * GR, GR, device="cuda", dtype=BF), gm3_crowmap=(arg // P * GR + arg % P).to(I32),
                img_tiles=torch.tensor(tl, device="cuda", dtype=I32), img_tile_count=torch.tensor([len(tl)], device="cuda", dtype=I32),
                wn=torch.empty(Bc, T, device="cuda", dtype=F32), sim=torch.full((B, Bc), float("nan"), device="cuda", dtype=F32))
    ops.local_sim_chunks(chunks)
    try:
        return local_sim_forward(ctx, w, cl, np.asarray(caps), TEMP1, TEMP2, **bufs)
    finally:
        ops.local_sim_chunks(0)


# --------------------------------------------------------------------------------------------------------------------------------------
# kernel
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [0, 1])
@pytest.mark.parametrize("case", ["fixture64", "seeded196"])
def test_local_sim_fwd_against_the_reference(golden_dir, case, chunks):
    """sim of the new kernel against the oracle in fp32 on the CPU; the bar is twice the existing path's own error on the same inputs.
    chunks = 1: one workgroup per image walks the whole caption list (many iterations over the ring and the mailboxes)."""
    img, words, caps = fixture_case(golden_dir)[:3] if case == "fixture64" else seeded_case()
    ref = oracle_sim(img, words, caps)
    err = float((new_sim(img, words, caps, chunks).cpu() - ref).abs().max())
    print(f"local_sim_fwd {case} chunks={chunks}: max abs error {err:.3e} (existing path {OLD_SIM_ERR[case]}, bar {SIM_BAR[case]})")
    assert err <= SIM_BAR[case]


def test_local_sim_fwd_fixture_losses(golden_dir):
    """loss0 / loss1 of the reference's fixture through sim kernel -> cross-entropy heads, within the 5e-3 of
    test_gloria_local_reference_fixture."""
    from medmoe_amd import ops
    img, words, caps, loss0, loss1 = fixture_case(golden_dir)
    sim = new_sim(img, words, caps)
    B = sim.shape[0]
    g, out = torch.empty_like(sim), torch.zeros(2, device="cuda")
    ops.call("ce_strided", sim, g, B, B, B, 1, 0, TEMP3, 1.0 / B, 0, out[0:])
    ops.call("ce_strided", sim, g, B, B, 1, B, 0, TEMP3, 1.0 / B, 1, out[1:])
    e0, e1 = abs(float(out[0]) - loss0) / abs(loss0), abs(float(out[1]) - loss1) / abs(loss1)
    print(f"local_sim_fwd fixture: loss0 {e0:.5f} loss1 {e1:.5f}")
    assert e0 < 5e-3 and e1 < 5e-3


def test_local_sim_fwd_is_deterministic():
    img, words, caps = seeded_case()
    a, b = new_sim(img, words, caps).clone(), new_sim(img, words, caps)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_local_sim_fwd_refuses_other_geometries():
    """100 regions, a sixth length class, 64 regions with more than 16 words: -2 from the argument check, nothing launched (sim untouched)."""
    from medmoe_amd import ops
    D, T = 128, 96
    z = lambda *s, dt=BF: torch.zeros(*s, device="cuda", dtype=dt)
    sim = torch.full((2, 2), 7.0, device="cuda")
    members = torch.arange(2, device="cuda", dtype=I32)
    for HW, ntt in ((100, 1), (196, 6), (64, 2)):
        GR = (HW + 31) // 32 * 32
        with pytest.raises(RuntimeError, match="code -2"):
            ops.call("local_sim_fwd", z(2 * HW, D), z(2, T, D), torch.full((2,), 16 * ntt, device="cuda", dtype=I32), z(2 * GR, GR), z(2, T, dt=F32),
                     sim, 2, 2, HW, T, D, TEMP1, TEMP2, 1e-8, members, 2, ntt)
    torch.cuda.synchronize()
    assert bool((sim == 7.0).all())


# --------------------------------------------------------------------------------------------------------------------------------------
# engine
# --------------------------------------------------------------------------------------------------------------------------------------
def _engine(name, **over):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name(name)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg, Engine(cfg, "cuda:0", seed=0)


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("name,B", [("tiny", 8), ("tiny2", 8), ("cfg0", 8), ("tinyL", 8)])
def test_eval_step_reports_the_training_losses(name, B, soft):
    """eval_step against train_step(optimizer=False) on the same batch and parameters: g_loss / classifier_loss 1e-5 relative (the bar of
    test_gloria_global_reference_fixture for a loss value), classifier_acc equal, l_loss 5e-3 relative (the fixture test's local-loss bar).
    soft: the Soft-GLoRIA heads, with the two thresholds placed in gaps of the batch's own caption scores as test_soft_gloria_gpu.py does -
    at the default 0.98 / 0.97 the synthetic captions have no negatives and both losses are zero up to rounding."""
    import bench
    cfg, eng = _engine(name, soft_label=soft)
    b = bench.synthetic_batch(cfg, B, 31, eng.device)
    if soft:
        from test_soft_gloria_gpu import _thresholds
        eng._alloc(B)
        eng.prefetch_cap_lens(b["ids"])
        eng._forward_both(b)
        cfg.threshold0, cfg.threshold1, margin = _thresholds(eng.text_soft_target().cpu())
        assert margin > 0
    tr = {k: float(v) for k, v in eng.train_step(b, optimizer=False).items()}
    ev = {k: float(v) for k, v in eng.eval_step(b).items()}
    print(name, soft, "train", tr, "eval", ev)
    assert set(ev) == {"loss", "l_loss", "g_loss", "classifier_loss", "classifier_acc"}
    assert tr["g_loss"] > 1e-2 and tr["l_loss"] > 1e-2              # values a relative bar means something for
    for k in ("g_loss", "classifier_loss"):
        assert abs(ev[k] - tr[k]) <= 1e-5 * abs(tr[k]), (k, ev[k], tr[k])
    assert ev["classifier_acc"] == tr["classifier_acc"]
    assert abs(ev["l_loss"] - tr["l_loss"]) <= 5e-3 * abs(tr["l_loss"]), (ev["l_loss"], tr["l_loss"])
    want = cfg.w_cls * ev["classifier_loss"] + cfg.w_global * ev["g_loss"] + cfg.w_local * ev["l_loss"]
    assert abs(ev["loss"] - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize("freeze_text", [True, False])
def test_eval_step_leaves_parameters_gradients_and_adam_state_alone(freeze_text):
    import bench
    cfg, eng = _engine("tiny", freeze_text=freeze_text)
    b = bench.synthetic_batch(cfg, 8, 5, eng.device)
    eng.train_step(b)                                                # one optimiser step: m / v exist
    stores = [eng.params] + ([eng.tstore] if not freeze_text else [])
    for st in stores:
        st.g32.copy_(torch.arange(st.g32.numel(), device=st.g32.device, dtype=F32) % 7 - 3.0)
    torch.cuda.synchronize()
    snap = [{k: getattr(st, k).clone() for k in ("p32", "p16", "p16t", "g32", "m", "v")} for st in stores]
    steps = [int(st.step_count) for st in stores]
    out = eng.eval_step(bench.synthetic_batch(cfg, 8, 6, eng.device))
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"]))
    for st, sn, n in zip(stores, snap, steps):
        for k, v in sn.items():
            assert torch.equal(getattr(st, k), v), k
        assert int(st.step_count) == n


def test_an_engine_that_only_evaluates_allocates_no_pair_matrices():
    import bench
    cfg, eng = _engine("cfg0")
    out = eng.eval_step(bench.synthetic_batch(cfg, 4, 9, eng.device))
    assert 0 < float(out["loss"]) < 100
    from medmoe_amd.local_transposed import TransposedLocalLoss
    loc = eng._local                                                  # the engine's one local-loss object; no second formulation exists
    assert eng.local_t and type(loc) is TransposedLocalLoss and eng._gle is None
    assert loc.cap == 0 and not loc.pair and not {"l_A", "l_dS", "l_U"} & set(eng.ws)
    eng.train_step(bench.synthetic_batch(cfg, 4, 9, eng.device), optimizer=False)      # training on the same engine still sizes them
    assert eng._local is loc and loc.cap > 0 and "l_A" in loc.pair and "l_dS" in loc.pair
    assert not {"l_A", "l_dS", "l_U"} & set(eng.ws)


# --------------------------------------------------------------------------------------------------------------------------------------
# module, trainer, data parallel
# --------------------------------------------------------------------------------------------------------------------------------------
def _mb(b):
    return {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"]}}


def test_module_validation_step_and_trainer_validate(monkeypatch):
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.hydra_lite import compose, instantiate
    from medmoe_amd.trainer import Trainer
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    cfg = compose(os.path.join(ROOT, "configs"), "train.yaml", ["experiment=pretraining_medmoe_cfg2", "model.model.vision.config_name=tiny2"])
    lit = instantiate(cfg.model)
    c2 = config_by_name("tiny2")
    dev = lit.model.engine.device
    b1, b2 = _mb(bench.synthetic_batch(c2, 8, 41, dev)), _mb(bench.synthetic_batch(c2, 8, 42, dev))
    p0 = lit.model.weights.detach().clone()
    v1, f1, t1 = lit.validation_step(b1, 0), lit.fused_eval_step(b1), lit.test_step(b1, 0)
    assert set(v1) == {"loss", "l_loss", "g_loss", "classifier_loss", "classifier_acc"}
    # three separate eval_steps of one batch: the heads add their rows' terms with fp32 atomics in arrival order, so the values agree to
    # a few ulp, not bit for bit - held to the 1e-5 relative of a loss value elsewhere in this file
    close = lambda a, b: abs(float(a) - float(b)) <= 1e-5 * abs(float(b))
    assert close(f1["loss"], v1["loss"]) and close(t1["loss"], v1["loss"])
    want = (float(v1["loss"]) + float(lit.validation_step(b2, 1)["loss"])) / 2

    class DM:
        def val_dataloader(self):
            return [b1, b2]

    got = Trainer().validate(lit, DM())["val/loss"]
    assert abs(got - want) <= 1e-5 * abs(want) and 0 < got < 100      # the same batches evaluated again: the same few ulp
    assert torch.equal(lit.model.weights.detach(), p0)


def test_two_ranks_eval_step_reports_the_training_losses():
    """tools/two_rank_eval.py: two gloo ranks on the one GPU; every rank's eval_step reports the g_loss (gathered embeddings) of its
    train_step(optimizer=False) on the same batch and, with cfg.local_loss_global, the l_loss (gathered captions) too."""
    for extra in ({}, {"TWO_RANK_GLOBAL_LOCAL": "1"}):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", **extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "two_rank_eval.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "two-rank eval path OK" in r.stdout
