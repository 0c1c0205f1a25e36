"""Semantic segmentation on the MedMoE image tower: a linear decoder on the region features with independent sigmoids per class,
trained as a probe on the frozen tower (`mode: probe`) or together with it (`mode: finetune`) on BCE + batch Dice, reporting per-class and
mean Dice / IoU over each evaluation epoch from integer pixel counts.

The same `MedMoE` net sits under `self.model`, so a checkpoint written by the pretraining module loads with strict=False and leaves the head
at its initial value (zero).  Every step runs on the HIP engine: Engine.segment_step / segment_eval and the head's launches
(medmoe_amd/segment.py, csrc/segment.hip); there is no autograd path."""
from typing import Any, Dict

import torch
from torch import nn

from .head_module import HeadOnEngineModule, _Base

_KEYS = ("num_classes", "mode", "mask_key", "pos_weight", "w_bce", "w_dice", "dice_eps", "head_lr", "pretrained_ckpt", "class_names")
_MODES = ("probe", "finetune")


def segmenter_block(segmenter: Any) -> Dict[str, Any]:
    """The validated `model.segmenter` block with its defaults filled in."""
    if segmenter is None:
        raise KeyError("model.segmenter is missing: the segmenter module needs at least model.segmenter.num_classes")
    c = dict(segmenter)
    unknown = set(c) - set(_KEYS)
    if unknown:
        raise KeyError(f"model.segmenter: unknown keys {sorted(unknown)} ({', '.join(_KEYS)})")
    if c.get("num_classes") is None:
        raise KeyError("model.segmenter.num_classes is required")
    num = lambda k, d: d if c.get(k) is None else float(c[k])
    out = {"num_classes": int(c["num_classes"]), "mode": str(c.get("mode") or "probe"), "mask_key": str(c.get("mask_key") or "mask"),
           "pos_weight": None if c.get("pos_weight") is None else [float(v) for v in c["pos_weight"]],
           "w_bce": num("w_bce", 1.0), "w_dice": num("w_dice", 1.0), "dice_eps": num("dice_eps", 1.0),
           "head_lr": None if c.get("head_lr") is None else float(c["head_lr"]),
           "pretrained_ckpt": c.get("pretrained_ckpt") or None,
           "class_names": None if c.get("class_names") is None else [str(v) for v in c["class_names"]]}
    if out["mode"] not in _MODES:
        raise ValueError(f"model.segmenter.mode must be one of {_MODES}, got {out['mode']!r}")
    if out["class_names"] is not None and len(out["class_names"]) != out["num_classes"]:
        raise ValueError(f"model.segmenter.class_names holds {len(out['class_names'])} names for num_classes = {out['num_classes']}")
    if out["pos_weight"] is not None and len(out["pos_weight"]) != out["num_classes"]:
        raise ValueError(f"model.segmenter.pos_weight holds {len(out['pos_weight'])} values for num_classes = {out['num_classes']}")
    return out


class MedMoESegmenterLightningModule(HeadOnEngineModule):
    """Keys under `model.segmenter`: num_classes (1 .. 8); mode (probe | finetune); mask_key (default "mask": batch[mask_key] holds int8
    [B, C, H, W] in {0, 1, -1}, -1 = ignored; the other forms of medmoe_amd.segment.prepare_masks are accepted); pos_weight ([C]); w_bce,
    w_dice, dice_eps; head_lr (default: the optimizer's lr; the scheduler scales both alike); pretrained_ckpt (a checkpoint of the
    pretraining module, loaded with strict=False); class_names (for the dice/<class> and iou/<class> metric names).
    The checkpoint hooks, configure_fused, set_deterministic and configure_optimizers are the pretraining module's; the head's weights
    travel in the state dict as seg_head.weight / seg_head.bias and its Adam moments under fused_adam["seg_head"]."""

    _KIND, _STEP, _LAUNCH, _FEATURE, _DESIGN = "segmenter", "Engine.segment_step", "loss / backward launches", "region features", "3t"

    def __init__(self, model: nn.Module, segmenter: Any = None, optimizer: Any = None, scheduler: Any = None, compile: bool = False,
                 fused_step: bool = True):
        _Base.__init__(self)
        self._seg = segmenter_block(segmenter)
        eng = self._init_on_engine(model, optimizer, scheduler, fused_step)
        from medmoe_amd.segment import SegBank, SegmenterHead
        c = self._seg
        pw = None if c["pos_weight"] is None else torch.tensor(c["pos_weight"], dtype=torch.float32)
        self.head = SegmenterHead(eng.cfg.d_out, c["num_classes"], eng.device, pos_weight=pw, w_bce=c["w_bce"], w_dice=c["w_dice"],
                                  dice_eps=c["dice_eps"])
        # the head's fp32 master as parameters (views of the store's flat buffer: load_state_dict writes the master in place)
        self.seg_head = nn.Module()
        self.seg_head.weight = nn.Parameter(self.head.weight)
        self.seg_head.bias = nn.Parameter(self.head.bias)
        self._counts = SegBank(c["num_classes"], eng.device)
        self._finish_init(c["head_lr"], c["pretrained_ckpt"])

    @property
    def train_tower(self) -> bool:
        return self._seg["mode"] == "finetune"

    def _batch(self, batch: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        key = self._seg["mask_key"]
        if key not in batch:
            raise KeyError(f"model.segmenter.mask_key = {key!r}: the batch holds {sorted(batch)} (data=unimed_seg yields `mask`)")
        return {"image": batch["image"].contiguous(), "mask": batch[key]}

    def forward(self, batch):
        """The patch logits [B, P, C] of a batch (evaluation form of the image pass)."""
        eng = self._fused_engine()
        eng.embed_image(batch["image"].contiguous())
        return self.head.logits(eng.ws["img_l"])

    def predict(self, batch, size):
        """uint8 masks [B, C, H, W] of a batch at size = (H, W)."""
        from medmoe_amd import ops
        return ops.seg_predict(self.forward(batch), size)

    def fused_training_step(self, batch: Dict[str, Any], optimizer_step: bool = True, zero_grad: bool = True, loss_scale: float = 1.0):
        """One micro-batch through Engine.segment_step: {"loss"} as a device scalar."""
        eng = self._fused_engine()
        out = eng.segment_step(self._batch(batch), self.head, self.train_tower, optimizer=optimizer_step, zero_grad=zero_grad,
                               loss_scale=loss_scale, head_lr=self._head_lr())
        return {"loss": out["loss"]}

    def fused_eval_step(self, batch: Dict[str, Any]):
        """One batch through Engine.segment_eval; the pixel counts go into the epoch's SegBank."""
        eng = self._fused_engine()
        _, out = eng.segment_eval(self._batch(batch), self.head)
        self._counts.add(out["counts"])
        return {"loss": out["loss"]}

    def on_validation_epoch_start(self):
        self._counts.reset()

    def on_validation_epoch_end(self):
        """{"dice_mean", "iou_mean", "dice/<class>", "iou/<class>"} over the epoch's counts; the trainer files them under val/... or test/...."""
        from medmoe_amd.segment import segmentation_metrics
        return segmentation_metrics(self._counts, self._seg["class_names"])

    def _fused_stores(self) -> Dict[str, Any]:
        out = super()._fused_stores()
        out["seg_head"] = self.head.store
        return out
