"""Engine.segment_step / segment_eval on the GPU, on tiny (8 x 8 regions) and tinyL (16 x 16): the probe leaves the engine's
stores alone, fine-tuning is the hand-run sequence bit for bit, the zero head's first step, accumulation for w_dice = 0, the frozen and
adapter engines, overfitting a fixed batch, and the refusals."""
import math

import pytest
import torch
import torch.nn.functional as F

import segment_reference as R
from test_engine_gpu import make, rel, to_dev
from test_vit_lora_gpu import make_v

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 2
# two runs of the same backward differ by the order of their fp32 atomics: the bar of test_engine_gpu.test_gradient_accumulation_equals_one_step
REPEAT_BAR = 2e-3
SIZES = {"tiny": (4, (64, 64)), "tiny2": (4, (40, 52)), "tinyL": (2, (100, 90))}          # batch, mask size (a multiple of the grid, and not)


def _head(eng, init="normal", **kw):
    from medmoe_amd.segment import SegmenterHead
    return SegmenterHead(eng.cfg.d_out, C, eng.device, init=init, std=0.05, seed=5, **kw)


def _seg_batch(batch, size, seed=0):
    """The images with seeded blob masks int8 [B, C, H, W]; a band of ignored pixels in the first image."""
    g = torch.Generator().manual_seed(seed)
    B = batch["image"].shape[0]
    m = (F.interpolate(torch.randn(B, C, 4, 4, generator=g), size=size, mode="bilinear") > 0.0).to(torch.int8)
    m[0, :, :3] = -1
    return {"image": batch["image"].cuda(), "mask": m.cuda()}


def _arena_snapshot(a):
    names = ("p32", "g32", "p16", "p16t", "m", "v", "e32")
    return {n: getattr(a, n).clone() for n in names if getattr(a, n, None) is not None}


@pytest.mark.parametrize("cfg_name", ["tiny", "tinyL"])
def test_probe_leaves_the_engine_alone_and_moves_the_head(cfg_name):
    B, size = SIZES[cfg_name]
    _, _, _, batch, eng = make(cfg_name, B)
    head = _head(eng, init="zero")
    b = _seg_batch(batch, size)
    eng.train_step(to_dev(batch))                                    # the stores hold a gradient and Adam moments to be left alone
    torch.cuda.synchronize()
    before, step0 = _arena_snapshot(eng.params), eng.dropout_step
    w0 = head.weight.clone()
    out = None
    for _ in range(3):
        out = eng.segment_step(b, head, train_tower=False, head_lr=0.05)
    torch.cuda.synchronize()
    after = _arena_snapshot(eng.params)
    assert sorted(after) == sorted(before) and "m" in before
    for n in before:
        assert torch.equal(before[n], after[n]), n
    assert eng.dropout_step == step0 and eng.params.step_count == 1
    assert not torch.equal(head.weight, w0) and head.store.step_count == 3
    assert int(out["n_valid"]) == int((b["mask"] >= 0).sum()) and math.isfinite(float(out["loss"]))
    # forward only: segment_eval writes nothing of the head either
    hs = _arena_snapshot(head.store)
    z, ev = eng.segment_eval(b, head)
    torch.cuda.synchronize()
    for n, v in _arena_snapshot(head.store).items():
        assert torch.equal(v, hs[n]), n
    g = int(round(eng.cfg.n_patch ** 0.5))
    assert z.shape == (B, g * g, C) and math.isfinite(float(ev["loss"])) and torch.equal(z, head.logits(eng.ws["img_l"]))
    assert head.predict(eng.ws["img_l"], size).shape == (B, C) + size


@pytest.mark.parametrize("cfg_name", ["tiny2", "tinyL"])
def test_finetune_is_the_hand_run_sequence_bit_for_bit(cfg_name):
    B, size = SIZES[cfg_name]
    runs = []
    for hand in (False, True):
        _, _, _, batch, eng = make(cfg_name, B, seed=3)
        eng.set_deterministic(True)
        head = _head(eng, pos_weight=torch.tensor([0.5, 2.0]))
        b = _seg_batch(batch, size)
        eng._alloc(B)
        eng.ws["d_img_l"].fill_(float("nan")); eng.ws["d_img_g"].fill_(float("nan"))
        if not hand:
            out = eng.segment_step(b, head, train_tower=True, head_lr=0.01)
            loss = out["loss"].clone()
        else:
            c = eng.cfg
            eng.params.zero_grad(); head.store.zero_grad()
            eng._forward_image_train(b["image"])
            loss, _ = head.step(eng.ws["img_l"], b["mask"], 1.0, dfeat=eng.ws["d_img_l"])
            loss = loss.clone()
            eng.ws["d_img_g"].zero_()
            eng.backward(None, 1.0)
            eng.dropout_step += 1
            total = eng.params.sumsq()
            total.add_(head.store.sumsq())
            kw = dict(betas=tuple(c.adam_betas), eps=c.adam_eps, decoupled=c.optimizer == "adamw")
            eng.params.adam_step(total, c.lr, c.weight_decay, c.clip, **kw)
            head.adam_step(0.01, c.weight_decay, c.clip, normsq_total=total, **kw)
        torch.cuda.synchronize()
        # the head wrote ALL of d_img_l (it was NaN) and d_img_g is zero
        assert bool(torch.isfinite(eng.ws["d_img_l"].float()).all()) and float(eng.ws["d_img_l"].float().abs().max()) > 0
        assert bool((eng.ws["d_img_g"] == 0).all())
        assert float(eng.params.g32.abs().max()) > 0 and eng.dropout_step == 1
        runs.append((eng.params.p32.clone(), eng.params.g32.clone(), eng.params.m.clone(), head.store.p32.clone(), head.store.g32.clone(), loss))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


@pytest.mark.parametrize("cfg_name", ["tiny", "tinyL"])
def test_zero_head_first_step_moves_the_head_only(cfg_name):
    B, size = SIZES[cfg_name]
    _, _, _, batch, eng = make(cfg_name, B)
    head = _head(eng, init="zero")
    b = _seg_batch(batch, size)
    out = eng.segment_step(b, head, train_tower=True, optimizer=False)
    torch.cuda.synchronize()
    assert bool((eng.params.g32 == 0).all()) and bool((eng.ws["d_img_l"] == 0).all())      # dfeat = dz W with W = 0
    assert float(head.store.g32.abs().max()) > 0
    m = b["mask"].cpu().long()
    zf64, zf32 = torch.zeros(m.shape, dtype=torch.float64), torch.zeros(m.shape, dtype=torch.float32)
    ref, twin = R.loss_of_zf(zf64, m), R.loss_of_zf(zf32, m)
    tol = R.tolerance(ref.reshape(()), twin.reshape(()))
    print(f"{cfg_name}: first loss {float(out['loss']):.8f}, reference {float(ref):.8f}, tolerance {tol:.3e}")
    assert abs(float(out["loss"]) - float(ref)) <= tol
    # BCE alone: exactly ln 2 in fp32 terms
    bce = _head(eng, init="zero", w_dice=0.0)
    o2 = eng.segment_step(b, bce, train_tower=False, optimizer=False)
    r2, t2 = R.loss_of_zf(zf64, m, w_dice=0.0), R.loss_of_zf(zf32, m, w_dice=0.0)
    assert abs(float(r2) - math.log(2.0)) < 1e-15
    assert abs(float(o2["loss"]) - math.log(2.0)) <= R.tolerance(r2.reshape(()), t2.reshape(()))


@pytest.mark.parametrize("cfg_name", ["tiny2", "tinyL"])
def test_accumulation_of_two_half_scaled_micro_batches_for_bce(cfg_name):
    B, size = SIZES[cfg_name]
    _, _, _, batch, eng = make(cfg_name, B)
    head = _head(eng, w_dice=0.0)
    b = _seg_batch(batch, size)
    eng.segment_step(b, head, train_tower=True, optimizer=False)
    torch.cuda.synchronize()
    g1, h1 = eng.params.g32.clone(), head.store.g32.clone()
    eng.segment_step(b, head, train_tower=True, optimizer=False, zero_grad=True, loss_scale=0.5)
    eng.segment_step(b, head, train_tower=True, optimizer=False, zero_grad=False, loss_scale=0.5)
    torch.cuda.synchronize()
    assert float(g1.abs().max()) > 0
    assert rel(eng.params.g32, g1) < REPEAT_BAR and rel(head.store.g32, h1) < REPEAT_BAR


@pytest.mark.parametrize("cfg_name,lora", [("tiny", True), ("tiny", False), ("tinyL", True), ("tinyL", False)])
def test_frozen_and_adapter_engines_finetune_their_trainable_part_only(cfg_name, lora):
    B, size = SIZES[cfg_name]
    _, _, _, batch, eng, _ = make_v(cfg_name, B, lora=lora, freeze=not lora)
    head = _head(eng)
    b = _seg_batch(batch, size)
    p, tf = eng.params, eng.params.train_from
    assert tf > 0 and p.g32.numel() == p.numel - tf
    backbone, tail, w0 = p.p32[:tf].clone(), p.p32[tf:].clone(), head.weight.clone()
    a0 = eng.vlora.p32.clone() if lora else None
    eng.segment_step(b, head, train_tower=True, optimizer=False)
    torch.cuda.synchronize()
    assert p.g32.abs().max() > 0 and head.store.g32.abs().max() > 0 and (not lora or eng.vlora.g32.abs().max() > 0)
    eng.segment_step(b, head, train_tower=True, head_lr=0.01)
    torch.cuda.synchronize()
    assert torch.equal(p.p32[:tf], backbone)                         # the backbone's arena is untouched
    assert not torch.equal(p.p32[tf:], tail) and not torch.equal(head.weight, w0)
    assert not lora or not torch.equal(eng.vlora.p32, a0)


@pytest.mark.parametrize("cfg_name", ["tiny", "tinyL"])
def test_overfitting_a_fixed_batch_lowers_the_loss_and_raises_dice(cfg_name):
    from medmoe_amd.segment import SegBank, segmentation_metrics
    B, size = SIZES[cfg_name]
    _, _, _, batch, eng = make(cfg_name, B)
    head = _head(eng, init="zero")
    b = _seg_batch(batch, size)

    def val():
        bank = SegBank(C, DEV)
        _, ev = eng.segment_eval(b, head)
        bank.add(ev["counts"])
        return float(ev["loss"]), segmentation_metrics(bank, ["a", "b"])

    l0, m0 = val()
    losses = [float(eng.segment_step(b, head, train_tower=True, head_lr=0.02)["loss"]) for _ in range(30)]
    l1, m1 = val()
    print(f"{cfg_name}: loss {losses[0]:.4f} -> {losses[-1]:.4f}; eval {l0:.4f} -> {l1:.4f}; dice {m0['dice_mean']} -> {m1['dice_mean']}")
    assert losses[-1] < losses[0] and l1 < l0
    d0 = 0.0 if m0["dice_mean"] != m0["dice_mean"] else m0["dice_mean"]           # the zero head predicts nothing: Dice 0 (or no class: NaN)
    assert m1["dice_mean"] > d0
    assert sorted(m1) == ["dice/a", "dice/b", "dice_mean", "iou/a", "iou/b", "iou_mean"]


def test_refusals_name_their_keys():
    B, size = SIZES["tiny"]
    _, _, _, batch, eng = make("tiny", B)
    head, b = _head(eng), _seg_batch(batch, size)
    eng.dist = True
    with pytest.raises(NotImplementedError, match="self.dist"):
        eng.segment_step(b, head, train_tower=False)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        eng.segment_eval(b, head)
    eng.dist = False
    eng.cfg.ema_decay = 0.999
    with pytest.raises(NotImplementedError, match="ema_decay.*model.ema.decay"):
        eng.segment_step(b, head, train_tower=True)
    eng.cfg.ema_decay = 0.0
    eng.cfg.optimizer = "lamb"
    with pytest.raises(NotImplementedError, match="lamb"):
        eng.segment_step(b, head, train_tower=False)
    eng.cfg.optimizer = "adam"
    from medmoe_amd.swin_engine import SwinEngine
    sw = SwinEngine.__new__(SwinEngine)
    for call in (lambda: sw.segment_step({}, None, True), lambda: sw.segment_eval({}, None)):
        with pytest.raises(NotImplementedError, match="swin_t"):
            call()
    eng.segment_step(b, head, train_tower=False)                      # and the engine still steps afterwards
