"""Semantic segmentation on the region features: a linear decoder on ws["img_l"] (the Segmenter / SETR "linear" baseline) with
independent sigmoids per class, its bilinear upsample to the mask size, BCE + batch-Dice loss and the pixel counts of Dice / IoU - four
launches of csrc/segment.hip (medmoe_amd.ops.seg_head_fwd / seg_loss / seg_head_bwd / seg_predict).  Nothing of the shape [B, C, H, W] is
stored in fp32 and no fp32 atomic is used: two steps on the same inputs give the same bits.

The head's parameters are a `FlatStore` like every other trained arena (head.LinearHead, shared with the classification head), so the clip
norm, the fused Adam launch, zero_grad and the Adam-state export are the arena code that already exists.  The head is fp32 throughout: the
kernels read the fp32 master.

Initialisation.  The head starts at ZERO (init="zero"): every full-resolution logit is 0, so the first BCE is exactly ln 2 whatever the
features are, and because dfeat = dz W the tower's first gradient under fine-tuning is exactly zero - the first step moves the head only.
init="normal" (std=) draws N(0, std^2) weights from a seeded generator instead; the bias stays zero.

Batch Dice.  I, P and T are sums over the (micro-)batch a step sees, so the Dice term is not additive over micro-batches: gradient
accumulation reproduces the one-batch step only for w_dice = 0."""
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .head import LinearHead

WEIGHT, BIAS = "seg_head.weight", "seg_head.bias"


def prepare_masks(masks: torch.Tensor, num_classes: int) -> torch.Tensor:
    """The masks as the loss launch takes them: contiguous int8 [B, C, H, W] in {0, 1, -1} (-1 = ignored).  Accepted: [B, C, H, W], or
    [B, H, W] for a one-class head; int8 (as it is), uint8 with 255 = ignored, bool, or any other integer / floating dtype holding 0, 1 and
    -1 (or 255) - values are not checked beyond that mapping."""
    if not isinstance(masks, torch.Tensor):
        raise ValueError(f"prepare_masks: masks must be a tensor, got {type(masks)}")
    if masks.dim() == 3:
        if int(num_classes) != 1:
            raise ValueError(f"prepare_masks: masks [B, H, W] are accepted for one class only, the head has {num_classes}")
        masks = masks.unsqueeze(1)
    if masks.dim() != 4 or masks.shape[1] != int(num_classes):
        raise ValueError(f"prepare_masks: masks must be [B, {num_classes}, H, W], got {tuple(masks.shape)}")
    if masks.dtype == torch.int8:
        out = masks.contiguous()
    elif masks.dtype == torch.uint8:
        out = masks.contiguous().view(torch.int8).clamp(min=-1)             # 255 reads -1; 128 .. 254 are ignored too
    elif masks.dtype == torch.bool:
        out = masks.to(torch.int8).contiguous()
    else:
        out = masks.to(torch.float32 if masks.dtype.is_floating_point else torch.int16)
        out = torch.where((out == 255) | (out < 0), torch.full_like(out, -1), out).to(torch.int8).contiguous()
    return out.clone() if out.data_ptr() % 16 else out                       # the launch reads 16 bytes at a time: a slice may start anywhere


class SegmenterHead(LinearHead):
    WEIGHT, BIAS, MAX_D, MAX_CLASSES = WEIGHT, BIAS, ops.SEG_MAX_D, ops.SEG_MAX_CLASSES

    def __init__(self, d: int, num_classes: int, device, pos_weight: Optional[torch.Tensor] = None, w_bce: float = 1.0, w_dice: float = 1.0,
                 dice_eps: float = 1.0, init: str = "zero", std: float = 0.01, seed: int = 0):
        if float(w_bce) < 0.0 or float(w_dice) < 0.0 or float(w_bce) + float(w_dice) <= 0.0:
            raise ValueError(f"SegmenterHead: w_bce and w_dice must be >= 0 and not both 0, got {w_bce}, {w_dice}")
        if not float(dice_eps) >= 0.0:
            raise ValueError(f"SegmenterHead: dice_eps must be >= 0, got {dice_eps}")
        super().__init__(d, num_classes, device, pos_weight, init, std, seed)
        self.w_bce, self.w_dice, self.dice_eps = float(w_bce), float(w_dice), float(dice_eps)

    # -- launches --------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _grid(P: int) -> int:
        g = int(round(P ** 0.5))
        if g * g != P or not 1 <= g <= ops.SEG_MAX_GRID:
            raise ValueError(f"SegmenterHead: feat has P = {P} regions; P must be a square g * g with 1 <= g <= {ops.SEG_MAX_GRID}")
        return g

    def _feat(self, feat: torch.Tensor) -> Tuple[int, int]:
        if not isinstance(feat, torch.Tensor) or feat.dim() != 3 or feat.shape[2] != self.d:
            raise ValueError(f"SegmenterHead: feat must be bf16 [B, P, {self.d}], got {tuple(getattr(feat, 'shape', ()))}")
        return feat.shape[0], self._grid(feat.shape[1])

    def _buffers(self, B: int, g: int, H: int, W: int) -> Dict[str, torch.Tensor]:
        key = (B, g, H, W)
        if key != self._key:
            dev, f32 = self.device, torch.float32
            self._ws = {"z": torch.empty((B, g * g, self.C), device=dev, dtype=f32), "dz": torch.empty((B, g * g, self.C), device=dev, dtype=f32),
                        "loss": torch.zeros(1, device=dev, dtype=f32), "counts": torch.zeros((self.C, 4), device=dev, dtype=torch.int64),
                        "scratch": torch.empty(ops.seg_scratch(B, g, H, W, self.d, self.C), device=dev, dtype=f32)}
            self._key = key
        return self._ws

    def logits(self, feat: torch.Tensor) -> torch.Tensor:
        """The patch logits z fp32 [B, P, C] of bf16 features [B, P, d]: a new tensor (medmoe_seg_head_fwd)."""
        B, g = self._feat(feat)
        return ops.seg_head_fwd(feat.reshape(B * g * g, self.d), self.weight, self.bias).reshape(B, g * g, self.C)

    def predict(self, feat: torch.Tensor, size: Sequence[int], want_logits: bool = False):
        """uint8 masks [B, C, H, W] = (zf > 0) at size = (H, W); with want_logits also the fp32 zf (sigmoid gives the probability maps)."""
        return ops.seg_predict(self.logits(feat), size, want_logits=want_logits)

    def step(self, feat: torch.Tensor, masks: torch.Tensor, loss_scale: float = 1.0, dfeat: Optional[torch.Tensor] = None):
        """Forward, loss and backward of the head on bf16 features [B, P, d] against masks (see prepare_masks): the head's gradient is
        ACCUMULATED into the store's gradient buffer, dfeat bf16 [B, P, d] (when given) is WRITTEN with d loss / d feat.  Returns the
        device tensors (loss fp32 scalar, counts int64 [C, 4] = (n_valid, TP, FP, FN)) - views of the head's workspace, valid until its next
        launch; the patch logits stay in `self.last_logits`."""
        return self._launch(feat, masks, loss_scale, dfeat, self.store.grad(WEIGHT), self.store.grad(BIAS))

    def evaluate(self, feat: torch.Tensor, masks: torch.Tensor):
        """(loss, counts) and `last_logits` as `step` leaves them at loss_scale 1, forward only: no gradient pass, nothing of the store is
        written."""
        return self._launch(feat, masks, 1.0, None, None, None)

    def _launch(self, feat, masks, loss_scale, dfeat, dW, db):
        B, g = self._feat(feat)
        m = prepare_masks(masks, self.C)
        if m.shape[0] != B:
            raise ValueError(f"SegmenterHead: masks hold {m.shape[0]} images, feat {B}")
        ws = self._buffers(B, g, m.shape[2], m.shape[3])
        x = feat.reshape(B * g * g, self.d)
        ops.seg_head_fwd(x, self.weight, self.bias, ws["z"])
        grad = dW is not None
        ops.seg_loss(ws["z"], m, pos_weight=self.pos_weight, w_bce=self.w_bce, w_dice=self.w_dice, dice_eps=self.dice_eps, loss_scale=loss_scale,
                     dz=ws["dz"] if grad else None, loss=ws["loss"], counts=ws["counts"], scratch=ws["scratch"])
        if grad:
            ops.seg_head_bwd(ws["dz"], x, self.weight, dW, db, dfeat=dfeat, scratch=ws["scratch"])
        return ws["loss"][0], ws["counts"]


class SegBank:
    """int64 [C, 4] = (n_valid, TP, FP, FN) accumulated over an evaluation epoch, on the device: nothing is read back per batch."""

    def __init__(self, num_classes: int, device):
        self.C, self.device = int(num_classes), torch.device(device)
        self.counts = torch.zeros((self.C, 4), device=self.device, dtype=torch.int64)
        self.batches = 0

    def reset(self):
        self.counts.zero_()
        self.batches = 0

    def __len__(self):
        return self.batches

    def add(self, counts: torch.Tensor):
        if tuple(counts.shape) != (self.C, 4) or counts.dtype != torch.int64:
            raise ValueError(f"SegBank.add: expected int64 [{self.C}, 4] counts, got {counts.dtype} {tuple(counts.shape)}")
        self.counts += counts.to(self.device)
        self.batches += 1


def dice_iou_from_counts(counts: torch.Tensor):
    """(dice float64 [C], iou float64 [C], dice_mean, iou_mean) from int64 [C, 4] = (n_valid, TP, FP, FN): Dice = 2 TP / (2 TP + FP + FN),
    IoU = TP / (TP + FP + FN).  A class with no positive and no predicted pixel (TP + FP + FN = 0) is NaN and left out of the means (NaN when
    no class is left)."""
    c = counts.detach().cpu().to(torch.float64)
    tp, den = c[:, 1], c[:, 1] + c[:, 2] + c[:, 3]
    ok = den > 0
    nan = torch.full_like(den, float("nan"))
    dice = torch.where(ok, 2.0 * tp / (den + tp).clamp(min=1.0), nan)
    iou = torch.where(ok, tp / den.clamp(min=1.0), nan)
    mean = lambda v: float(v[ok].mean()) if bool(ok.any()) else float("nan")
    return dice, iou, mean(dice), mean(iou)


def segmentation_metrics(bank: SegBank, class_names=None) -> Dict[str, float]:
    """{"dice_mean", "iou_mean", "dice/<class>", "iou/<class>"} over a bank; classes are named by `class_names` or their index."""
    if len(bank) == 0:
        return {}
    names = list(class_names) if class_names is not None else [str(c) for c in range(bank.C)]
    if len(names) != bank.C:
        raise ValueError(f"segmentation_metrics: {len(names)} class names for {bank.C} classes")
    dice, iou, dmean, imean = dice_iou_from_counts(bank.counts)
    out: Dict[str, float] = {"dice_mean": dmean, "iou_mean": imean}
    out.update({f"dice/{names[c]}": float(v) for c, v in enumerate(dice.tolist())})
    out.update({f"iou/{names[c]}": float(v) for c, v in enumerate(iou.tolist())})
    return out
