"""Semantic segmentation, host side (no GPU): the header and the built library, the wrappers' refusals, the hand-derived gradient
of the loss against autograd, the Dice / IoU reducers against brute force, prepare_masks, the synthetic masks, the experiments and the
module's `model.segmenter` block, and the sanitizer run of the shared support arithmetic (make check-seg-plan)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import segment_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
ENTRIES = ("medmoe_seg_head_fwd", "medmoe_seg_loss", "medmoe_seg_head_bwd", "medmoe_seg_predict", "medmoe_seg_scratch",
           "medmoe_seg_head_bwd_scratch")


def test_header_declares_the_entries_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    from medmoe_amd import lib_path, ops
    lib = ctypes.CDLL(lib_path())
    for name in ENTRIES:
        m = re.search(r"^(int|long long) %s\((.*)\);" % name, hdr, re.M)
        assert m, name
        assert hasattr(lib, name), name
        short = name[len("medmoe_"):]
        if not short.endswith("_scratch"):
            assert len(m.group(2).split(",")) == len(ops._SIGS[short]) + 1, name                  # + the stream
            assert m.group(2).endswith("hipStream_t stream"), name
    src = open(os.path.join(ROOT, "medmoe_amd", "csrc", "segment.hip")).read()
    assert "atomic" not in src.lower().replace("no fp32 atomic", "") and "g_mm_nondet" not in src           # no atomics at all, nothing counted
    assert '#include "seg_plan.h"' in src and "seg_support(" in src
    # the scratch query is a host function: a refused shape is 0, the cfg2 geometry a few MB
    q = lib.medmoe_seg_scratch
    q.restype = ctypes.c_longlong
    assert q(128, 14, 224, 224, 768, 1) > 0 and q(128, 14, 224, 224, 768, 9) == 0 and q(1, 14, 13, 224, 768, 1) == 0
    assert q(1, 14, 224, 224, 96, 1) == 0 and q(1, 65, 224, 224, 64, 1) == 0
    # a grid of more than 2^31 - 1 workgroups is a refused shape too: nothing is launched before a refusal
    assert q(1 << 25, 64, 64, 64, 64, 8) == 0
    qb = lib.medmoe_seg_head_bwd_scratch
    qb.restype = ctypes.c_longlong
    assert 0 < qb(128 * 196, 768, 1) <= q(128, 14, 224, 224, 768, 1) and qb(128 * 196, 96, 1) == 0 and qb(0, 64, 1) == 0
    assert ops.seg_head_bwd_scratch(64, 64, 2) == qb(64, 64, 2) == 64 * 2 + 64                 # one record of [C][D] + its pad


def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


def test_wrappers_refuse_bad_shapes_and_dtypes():
    from medmoe_amd import ops
    x, W, b = _bf(64, 64), torch.zeros(2, 64), torch.zeros(2)
    with pytest.raises(ValueError, match="feat must be a torch.bfloat16"):
        ops.seg_head_fwd(x.float(), W, b)
    with pytest.raises(ValueError, match="W must be a torch.float32"):
        ops.seg_head_fwd(x, W.double(), b)
    with pytest.raises(ValueError, match="feat has D = 96"):
        ops.seg_head_fwd(_bf(4, 96), torch.zeros(2, 96), b)
    with pytest.raises(ValueError, match="W has C = 9"):
        ops.seg_head_fwd(x, torch.zeros(9, 64), torch.zeros(9))
    with pytest.raises(ValueError, match="W has C = 0"):
        ops.seg_head_fwd(x, torch.zeros(0, 64), torch.zeros(0))
    with pytest.raises(ValueError, match="feat must be contiguous"):
        ops.seg_head_fwd(_bf(64, 128)[:, ::2], W, b)
    with pytest.raises(ValueError, match="b holds 3"):
        ops.seg_head_fwd(x, W, torch.zeros(3))
    with pytest.raises(RuntimeError, match="GPU"):                   # everything in order: the launch itself has no CPU form
        ops.seg_head_fwd(x, W, b)
    z, m = torch.zeros(1, 64, 2), torch.zeros(1, 2, 32, 40, dtype=torch.int8)
    with pytest.raises(ValueError, match="masks must be a torch.int8"):
        ops.seg_loss(z, m.to(torch.uint8))
    with pytest.raises(ValueError, match=r"masks must be \[B, C, H, W\]"):
        ops.seg_loss(z, m[0])
    with pytest.raises(ValueError, match="masks must have shape"):
        ops.seg_loss(z, torch.zeros(1, 3, 32, 40, dtype=torch.int8))
    with pytest.raises(ValueError, match="z must be a torch.float32"):
        ops.seg_loss(z.double(), m)
    with pytest.raises(ValueError, match="P must be a square"):
        ops.seg_loss(torch.zeros(1, 63, 2), m)
    with pytest.raises(ValueError, match="z has C = 9"):
        ops.seg_loss(torch.zeros(1, 64, 9), torch.zeros(1, 9, 32, 40, dtype=torch.int8))
    with pytest.raises(ValueError, match="H = 7 is smaller than the patch grid g = 8"):
        ops.seg_loss(z, torch.zeros(1, 2, 7, 40, dtype=torch.int8))
    with pytest.raises(ValueError, match="W = 5 is smaller"):
        ops.seg_loss(z, torch.zeros(1, 2, 32, 5, dtype=torch.int8))
    with pytest.raises(ValueError, match="pos_weight must have shape"):
        ops.seg_loss(z, m, pos_weight=torch.ones(3))
    with pytest.raises(ValueError, match="dz must have shape"):
        ops.seg_loss(z, m, dz=torch.zeros(1, 64, 3))
    with pytest.raises(ValueError, match="dice_eps"):
        ops.seg_loss(z, m, dice_eps=-1.0)
    with pytest.raises(ValueError, match="scratch holds 4 floats"):
        ops.seg_loss(z, m, scratch=torch.zeros(4))
    with pytest.raises(ValueError, match="counts must be a torch.int64"):
        ops.seg_loss(z, m, counts=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.seg_loss(z, m)
    dz, dW, db = torch.zeros(64, 2), torch.zeros(2, 64), torch.zeros(2)
    with pytest.raises(ValueError, match="dW must have shape"):
        ops.seg_head_bwd(dz, x, W, torch.zeros(2, 128), db)
    with pytest.raises(ValueError, match="dz must hold"):
        ops.seg_head_bwd(torch.zeros(63, 2), x, W, dW, db)
    with pytest.raises(ValueError, match="dfeat must be a torch.bfloat16"):
        ops.seg_head_bwd(dz, x, W, dW, db, dfeat=torch.zeros(64, 64))
    with pytest.raises(ValueError, match="dfeat must hold"):
        ops.seg_head_bwd(dz, x, W, dW, db, dfeat=_bf(64, 128))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.seg_head_bwd(dz, x, W, dW, db, dfeat=_bf(64, 64))
    with pytest.raises(ValueError, match="H = 4 is smaller"):
        ops.seg_predict(z, (4, 40))
    with pytest.raises(ValueError, match="masks must be a torch.uint8"):
        ops.seg_predict(z, (32, 40), masks=m)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.seg_predict(z, (32, 40))
    from medmoe_amd.segment import SegmenterHead
    for kw in (dict(d=96, num_classes=1), dict(d=64, num_classes=0), dict(d=64, num_classes=9), dict(d=64, num_classes=1, init="ones"),
               dict(d=64, num_classes=2, pos_weight=torch.ones(3)), dict(d=64, num_classes=1, w_bce=0.0, w_dice=0.0),
               dict(d=64, num_classes=1, dice_eps=-1.0)):
        with pytest.raises(ValueError):
            SegmenterHead(device="cpu", **kw)


@pytest.mark.parametrize("opts", [dict(), dict(w_dice=0.0, loss_scale=0.25), dict(w_bce=0.0, eps=0.5), dict(pos_weight=torch.tensor([0.5, 3.0, 1.0]))])
def test_the_hand_derived_gradient_equals_autograd_in_float64(opts):
    g = torch.Generator().manual_seed(11)
    zf = (3.0 * torch.randn(2, 3, 9, 7, generator=g, dtype=torch.float64)).requires_grad_(True)
    m = (torch.rand(2, 3, 9, 7, generator=g) < 0.4).long()
    m[torch.rand(2, 3, 9, 7, generator=g) < 0.2] = -1
    m[:, 1] = -1                                                     # a class without a valid pixel: left out of the Dice mean
    R.loss_of_zf(zf, m, **opts).backward()
    hand = R.dzf_formula(zf.detach(), m, **opts)
    assert float(zf.grad.abs().max()) > 0 and float((hand - zf.grad).abs().max()) < 1e-15
    assert not hand[:, 1].any() and not hand[m < 0].any()
    # nothing valid: loss 0, gradient 0, no NaN
    none = torch.full_like(m, -1)
    z0 = zf.detach().clone().requires_grad_(True)
    l0 = R.loss_of_zf(z0, none, **opts)
    l0.backward()
    assert float(l0.detach()) == 0.0 and not z0.grad.any() and not R.dzf_formula(z0.detach(), none, **opts).any()


def test_dice_iou_reducers_match_brute_force_with_an_empty_class():
    from medmoe_amd.segment import SegBank, dice_iou_from_counts, segmentation_metrics
    g = torch.Generator().manual_seed(3)
    C = 4
    bank, tot = SegBank(C, "cpu"), np.zeros((C, 4), dtype=np.int64)
    inter, npred, npos = np.zeros(C), np.zeros(C), np.zeros(C)
    for _ in range(3):
        zf = torch.randn(2, C, 12, 10, generator=g)
        m = (torch.rand(2, C, 12, 10, generator=g) < 0.3).long()
        m[torch.rand(2, C, 12, 10, generator=g) < 0.1] = -1
        m[:, 2][m[:, 2] == 1] = 0
        zf[:, 2] = -zf[:, 2].abs() - 0.1                              # class 2: no positive and no predicted pixel
        counts = R.counts_where(zf, m, torch.ones_like(m, dtype=torch.bool))
        bank.add(counts)
        for c in range(C):                                           # brute force: pixel loops over the valid pixels
            for t, p in zip(m[:, c].reshape(-1).tolist(), (zf[:, c] > 0).reshape(-1).tolist()):
                if t >= 0:
                    inter[c] += t == 1 and p
                    npred[c] += p
                    npos[c] += t == 1
    dice, iou, dmean, imean = dice_iou_from_counts(bank.counts)
    assert dice.dtype == torch.float64 and len(bank) == 3
    want_d = [2 * inter[c] / (npred[c] + npos[c]) if npred[c] + npos[c] else float("nan") for c in range(C)]
    want_i = [inter[c] / (npred[c] + npos[c] - inter[c]) if npred[c] + npos[c] else float("nan") for c in range(C)]
    assert dice[2] != dice[2] and iou[2] != iou[2] and want_d[2] != want_d[2]
    for c in (0, 1, 3):
        assert abs(float(dice[c]) - want_d[c]) < 1e-15 and abs(float(iou[c]) - want_i[c]) < 1e-15
    assert abs(dmean - np.mean([want_d[c] for c in (0, 1, 3)])) < 1e-15 and abs(imean - np.mean([want_i[c] for c in (0, 1, 3)])) < 1e-15
    met = segmentation_metrics(bank, ["a", "b", "c", "d"])
    assert sorted(met) == sorted(["dice_mean", "iou_mean"] + [f"{k}/{n}" for k in ("dice", "iou") for n in "abcd"])
    assert met["dice/a"] == float(dice[0]) and met["dice/c"] != met["dice/c"] and met["dice_mean"] == dmean
    none = dice_iou_from_counts(torch.zeros(2, 4, dtype=torch.int64))
    assert bool(torch.isnan(none[0]).all()) and none[2] != none[2]
    assert segmentation_metrics(SegBank(2, "cpu")) == {}
    with pytest.raises(ValueError):
        bank.add(torch.zeros(3, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        segmentation_metrics(bank, ["a"])
    bank.reset()
    assert len(bank) == 0 and not bank.counts.any()


def test_prepare_masks_accepts_its_documented_forms():
    from medmoe_amd.segment import prepare_masks
    base = torch.tensor([[[0, 1, -1], [1, 0, 0]]], dtype=torch.int8)            # [B = 1, H = 2, W = 3]
    want = base.reshape(1, 1, 2, 3)
    assert torch.equal(prepare_masks(base, 1), want)                            # [B, H, W] for one class
    assert prepare_masks(want, 1).data_ptr() == want.data_ptr()                 # int8 [B, C, H, W]: as it is
    u8 = torch.tensor([[[0, 1, 255], [1, 0, 0]]], dtype=torch.uint8)
    assert torch.equal(prepare_masks(u8, 1), want)                              # uint8 with 255 = ignored
    assert torch.equal(prepare_masks(base.long(), 1), want) and torch.equal(prepare_masks(base.float(), 1), want)
    assert torch.equal(prepare_masks(u8.long(), 1), want)
    assert torch.equal(prepare_masks(torch.tensor([[[False, True], [True, False]]]), 1), torch.tensor([[[[0, 1], [1, 0]]]], dtype=torch.int8))
    two = torch.zeros(2, 2, 4, 4, dtype=torch.int8)
    assert prepare_masks(two.permute(0, 1, 3, 2), 2).is_contiguous()
    off = torch.zeros(2 * 2 * 4 * 4 + 1, dtype=torch.int8)[1:].reshape(2, 2, 4, 4)      # a slice that starts off the 16-byte grid: copied
    assert prepare_masks(off, 2).data_ptr() % 16 == 0
    with pytest.raises(ValueError, match="one class only"):
        prepare_masks(base, 2)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        prepare_masks(two, 3)
    with pytest.raises(ValueError):
        prepare_masks([[0, 1]], 1)


def test_synthetic_masks_are_seeded_and_leave_the_other_entries_alone():
    from src.data.components.unimed import SyntheticUnimed, collate_fn
    from src.data.unimed_datamodule import UnimedDataModule
    kw = dict(n=8, max_len=16, vocab=97, n_classes=5, seed=7, min_side=20, max_side=30)
    plain, seg = SyntheticUnimed(**kw), SyntheticUnimed(masks={"num_classes": 3, "size": 32, "ignore_frac": 0.05}, **kw)
    again = SyntheticUnimed(masks={"num_classes": 3, "size": 32, "ignore_frac": 0.05}, **kw)
    for i in range(8):
        a, b, c = plain[i], seg[i], again[i]
        assert len(a) == 3 and len(b) == 4
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]          # image, caption, class: bit-identical
        assert torch.equal(b[3], c[3]) and b[3].dtype == torch.int8 and tuple(b[3].shape) == (3, 32, 32)
        assert set(b[3].unique().tolist()) <= {-1, 0, 1} and bool((b[3] == 1).any()) and bool((b[3] == -1).any())
    assert not torch.equal(seg[0][3], seg[1][3])
    cb, cs = collate_fn([plain[i] for i in range(4)]), collate_fn([seg[i] for i in range(4)])
    assert sorted(cb) == ["caption", "image", "label"] and sorted(cs) == ["caption", "image", "label", "mask"]
    assert tuple(cs["mask"].shape) == (4, 3, 32, 32) and torch.equal(cb["label"], cs["label"])
    # the datamodule: without the block the same tensors as before, with it one more key
    dkw = dict(batch_size=4, synthetic_size=8, max_len=16, synthetic_vocab=97)
    b0 = next(iter(UnimedDataModule(**dkw).train_dataloader()))
    b1 = next(iter(UnimedDataModule(masks={"num_classes": 1, "size": 24}, **dkw).train_dataloader()))
    assert sorted(b0) == ["caption", "image", "label"] and sorted(b1) == ["caption", "image", "label", "mask"]
    assert all(torch.equal(x, y) for x, y in zip(b0["image"], b1["image"])) and all(torch.equal(x, y) for x, y in zip(b0["caption"], b1["caption"]))
    assert torch.equal(b0["label"], b1["label"]) and tuple(b1["mask"].shape) == (4, 1, 24, 24) and not bool((b1["mask"] == -1).any())
    dev = UnimedDataModule._with_captions(torch.zeros(4, 3, 8, 8), b1, "cpu")
    assert torch.equal(dev["mask"], b1["mask"]) and "mask" not in UnimedDataModule._with_captions(torch.zeros(4, 3, 8, 8), b0, "cpu")
    with pytest.raises(KeyError, match="sizes"):
        SyntheticUnimed(masks={"sizes": 3})
    with pytest.raises(NotImplementedError, match="data.transformations"):
        UnimedDataModule(masks={"num_classes": 1}, transformations={"imsize": 256}, **dkw)


def test_both_experiments_compose_and_their_keys_reach_the_module(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from src.models.segmenter_module import MedMoESegmenterLightningModule as M, segmenter_block
    for exp, mode in (("segment_probe_medmoe_cfg2", "probe"), ("segment_finetune_medmoe_cfg2", "finetune")):
        cfg = compose(CONFIGS, "train.yaml", [f"experiment={exp}", "model.segmenter.num_classes=3", "data.masks.num_classes=3",
                                              "model.segmenter.w_dice=0.5"])
        assert cfg.model._target_ == "src.models.segmenter_module.MedMoESegmenterLightningModule" and cfg.model.fused_step is True
        assert cfg.data._target_.endswith("UnimedDataModule") and cfg.model.model.vision.arch == "vit_b16"
        assert dict(cfg.data.masks) == {"num_classes": 3, "size": 224, "ignore_frac": 0.02}
        blk = segmenter_block(cfg.model.segmenter)
        assert (blk["mode"], blk["num_classes"], blk["mask_key"], blk["w_bce"], blk["w_dice"], blk["dice_eps"]) == (mode, 3, "mask", 1.0, 0.5, 1.0)
        assert blk["pos_weight"] is None and blk["class_names"] is None
    with pytest.raises(KeyError, match="n_classes"):
        M(torch.nn.Identity(), segmenter={"num_classes": 1, "n_classes": 1})
    with pytest.raises(KeyError, match="num_classes"):
        M(torch.nn.Identity(), segmenter={"mode": "probe"})
    with pytest.raises(KeyError, match="model.segmenter is missing"):
        M(torch.nn.Identity())
    with pytest.raises(ValueError, match="mode"):
        M(torch.nn.Identity(), segmenter={"num_classes": 1, "mode": "linear_probe"})
    with pytest.raises(ValueError, match="class_names"):
        M(torch.nn.Identity(), segmenter={"num_classes": 2, "class_names": ["a"]})
    with pytest.raises(NotImplementedError, match="fused_step"):
        M(torch.nn.Identity(), segmenter={"num_classes": 1}, fused_step=False)
    with pytest.raises(NotImplementedError, match="HIP engine"):
        M(torch.nn.Identity(), segmenter={"num_classes": 1})
    # the data group without the block, and the pretraining experiments, are what they were
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert "segmenter" not in dict(base.model) and "masks" not in dict(base.data)


def test_make_check_seg_plan_builds_and_passes():
    """`make check-seg-plan`: tools/seg_plan_check.cpp, a stand-alone host program over csrc/seg_plan.h - the support ranges the gradient pass
    walks - built with the address and undefined-behaviour sanitizers and run."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^check-seg-plan:.*seg_plan_check\.cpp.*seg_plan\.h", mk, re.M)
    r = subprocess.run(["make", "-C", ROOT, "check-seg-plan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "-fsanitize=address,undefined" in r.stdout
    assert re.search(r"seg_plan_check: \d+ axes, \d+ \(pixel, corner\) pairs ok", r.stdout), r.stdout
