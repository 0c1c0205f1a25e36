"""Supervised image classification on the MedMoE image tower: the reference's `PretrainedImageClassifier(image_encoder, num_cls,
feature_dim, freeze_encoder)` (vision_encoder.py:140-175) as a module the trainer drives - a linear head on the global image embedding,
trained as a linear probe on the frozen tower (`mode: linear_probe` = freeze_encoder=True) or together with it (`mode: finetune`), reporting
accuracy and per-class / mean AUROC over each evaluation epoch.

The same `MedMoE` net sits under `self.model`, so a checkpoint written by the pretraining module loads with strict=False and leaves the head
at its initial value (zero).  Every step runs on the HIP engine: Engine.classify_step / classify_eval and the head's fused launch
(medmoe_amd/classify.py, csrc/classify.hip); there is no autograd path."""
from typing import Any, Dict

import torch
from torch import nn

from .head_module import HeadOnEngineModule, _Base

_KEYS = ("num_classes", "task", "mode", "label_key", "label_smoothing", "pos_weight", "head_lr", "pretrained_ckpt", "class_names")
_MODES = ("linear_probe", "finetune")


def classifier_block(classifier: Any) -> Dict[str, Any]:
    """The validated `model.classifier` block with its defaults filled in."""
    if classifier is None:
        raise KeyError("model.classifier is missing: the classifier module needs at least model.classifier.num_classes")
    c = dict(classifier)
    unknown = set(c) - set(_KEYS)
    if unknown:
        raise KeyError(f"model.classifier: unknown keys {sorted(unknown)} ({', '.join(_KEYS)})")
    if c.get("num_classes") is None:
        raise KeyError("model.classifier.num_classes is required")
    out = {"num_classes": int(c["num_classes"]), "task": str(c.get("task") or "multiclass"), "mode": str(c.get("mode") or "linear_probe"),
           "label_key": str(c.get("label_key") or "label"), "label_smoothing": float(c.get("label_smoothing") or 0.0),
           "pos_weight": None if c.get("pos_weight") is None else [float(v) for v in c["pos_weight"]],
           "head_lr": None if c.get("head_lr") is None else float(c["head_lr"]),
           "pretrained_ckpt": c.get("pretrained_ckpt") or None,
           "class_names": None if c.get("class_names") is None else [str(v) for v in c["class_names"]]}
    if out["task"] not in ("multiclass", "multilabel"):
        raise ValueError(f"model.classifier.task must be 'multiclass' or 'multilabel', got {out['task']!r}")
    if out["mode"] not in _MODES:
        raise ValueError(f"model.classifier.mode must be one of {_MODES}, got {out['mode']!r}")
    if out["class_names"] is not None and len(out["class_names"]) != out["num_classes"]:
        raise ValueError(f"model.classifier.class_names holds {len(out['class_names'])} names for num_classes = {out['num_classes']}")
    if out["pos_weight"] is not None and len(out["pos_weight"]) != out["num_classes"]:
        raise ValueError(f"model.classifier.pos_weight holds {len(out['pos_weight'])} values for num_classes = {out['num_classes']}")
    return out


class MedMoEClassifierLightningModule(HeadOnEngineModule):
    """Keys under `model.classifier`: num_classes; task (multiclass | multilabel); mode (linear_probe | finetune); label_key (default
    "label": batch[label_key] holds int [B] class indices or, multilabel, int [B, C] in {0, 1, -1}; -1 = not counted); label_smoothing
    (multiclass); pos_weight ([C], multilabel); head_lr (default: the optimizer's lr; the scheduler scales both alike); pretrained_ckpt (a
    checkpoint of the pretraining module, loaded with strict=False); class_names (for the auroc/<class> metric names).
    The checkpoint hooks, configure_fused, set_deterministic and configure_optimizers are the pretraining module's; the head's weights
    travel in the state dict as classifier.weight / classifier.bias and its Adam moments under fused_adam["head"]."""

    _KIND, _STEP, _LAUNCH, _FEATURE, _DESIGN = "classifier", "Engine.classify_step", "fused loss / backward launch", "global embedding", "3p"

    def __init__(self, model: nn.Module, classifier: Any = None, optimizer: Any = None, scheduler: Any = None, compile: bool = False,
                 fused_step: bool = True):
        _Base.__init__(self)
        self._cls = classifier_block(classifier)
        eng = self._init_on_engine(model, optimizer, scheduler, fused_step)
        from medmoe_amd.classify import ClassifierHead, ScoreBank
        c = self._cls
        pw = None if c["pos_weight"] is None else torch.tensor(c["pos_weight"], dtype=torch.float32)
        self.head = ClassifierHead(eng.cfg.d_out, c["num_classes"], eng.device, task=c["task"], label_smoothing=c["label_smoothing"], pos_weight=pw)
        # the head's fp32 master as parameters (views of the store's flat buffer: load_state_dict writes the master in place), under the
        # reference's names - PretrainedImageClassifier.classifier is an nn.Linear
        self.classifier = nn.Module()
        self.classifier.weight = nn.Parameter(self.head.weight)
        self.classifier.bias = nn.Parameter(self.head.bias)
        self._scores = ScoreBank(c["num_classes"], eng.device, task=c["task"])
        self._finish_init(c["head_lr"], c["pretrained_ckpt"])

    @property
    def train_tower(self) -> bool:
        return self._cls["mode"] == "finetune"

    def _batch(self, batch: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        key = self._cls["label_key"]
        if key not in batch:
            raise KeyError(f"model.classifier.label_key = {key!r}: the batch holds {sorted(batch)}")
        return {"image": batch["image"].contiguous(), "label": batch[key]}

    def forward(self, batch):
        """The logits [B, C] of a batch (evaluation form of the image pass)."""
        eng = self._fused_engine()
        return self.head.logits(eng.embed_image(batch["image"].contiguous())).clone()

    def fused_training_step(self, batch: Dict[str, Any], optimizer_step: bool = True, zero_grad: bool = True, loss_scale: float = 1.0):
        """One micro-batch through Engine.classify_step: {"loss", "acc"} as device scalars."""
        eng = self._fused_engine()
        out = eng.classify_step(self._batch(batch), self.head, self.train_tower, optimizer=optimizer_step, zero_grad=zero_grad,
                                loss_scale=loss_scale, head_lr=self._head_lr())
        return {"loss": out["loss"], "acc": out["acc"]}

    def fused_eval_step(self, batch: Dict[str, Any]):
        """One batch through Engine.classify_eval; the logits go into the epoch's ScoreBank."""
        eng, eb = self._fused_engine(), self._batch(batch)
        logits, out = eng.classify_eval(eb, self.head)
        self._scores.add(logits, eb["label"])
        return {"loss": out["loss"], "acc": out["acc"]}

    def on_validation_epoch_start(self):
        self._scores.reset()

    def on_validation_epoch_end(self):
        """{"acc" (multiclass), "auroc_mean", "auroc/<class>"} over the epoch's bank; the trainer files them under val/... or test/...."""
        from medmoe_amd.classify import classification_metrics
        return classification_metrics(self._scores, self._cls["class_names"])

    def _fused_stores(self) -> Dict[str, Any]:
        out = super()._fused_stores()
        out["head"] = self.head.store
        return out
