"""Supervised image classification on the global image embedding: a linear head with its fused loss / backward launch
(medmoe_amd.ops.cls_head_step, csrc/classify.hip), the linear probe on a bank of frozen features, and accuracy / AUROC over a growing
bank of logits.

The head's parameters are a `FlatStore` like every other trained arena (head.LinearHead, shared with the segmentation head), so the clip
norm, the fused Adam launch, zero_grad and the Adam-state export are the arena code that already exists.  The head itself is fp32
throughout: the kernels read the fp32 master, the bf16 working copy the arena keeps is not used.

Initialisation.  The head starts at ZERO (init="zeros"): the first loss is then exactly ln C (multiclass) or ln 2 (multilabel) whatever
the features are, and because dx = dz W the tower's first gradient under fine-tuning is exactly zero - the first step moves the head
only.  init="normal" (std=) draws N(0, std^2) weights from a seeded generator instead; the bias stays zero."""
from typing import Dict, Optional, Tuple

import torch

from . import ops
from .head import LinearHead

TASKS = ("multiclass", "multilabel")
WEIGHT, BIAS = "classifier.weight", "classifier.bias"


def prepare_targets(targets: torch.Tensor, task: str, num_classes: int) -> torch.Tensor:
    """The targets as the head launch takes them: contiguous int32 [N] (multiclass) or int8 [N, C] (multilabel); -1 = not counted."""
    if task == "multiclass":
        if targets.dim() != 1:
            raise ValueError(f"multiclass targets must be [N] class indices, got {tuple(targets.shape)}")
        return targets.to(torch.int32).contiguous()
    if targets.dim() != 2 or targets.shape[1] != num_classes:
        raise ValueError(f"multilabel targets must be [N, {num_classes}] in {{0, 1, -1}}, got {tuple(targets.shape)}")
    return targets.to(torch.int8).contiguous()


def targets_as_int8(targets: torch.Tensor, task: str, num_classes: int) -> torch.Tensor:
    """int8 [N, C] in {0, 1, -1} for the AUROC launch: multilabel targets as they are, multiclass labels one-hot (a row with label -1: all -1)."""
    if task == "multilabel":
        return targets.to(torch.int8).contiguous()
    y = targets.reshape(-1).long()
    out = (y.reshape(-1, 1) == torch.arange(num_classes, device=y.device).reshape(1, -1)).to(torch.int8)
    out[y < 0] = -1
    return out.contiguous()


class ClassifierHead(LinearHead):
    WEIGHT, BIAS, MAX_D, MAX_CLASSES = WEIGHT, BIAS, ops.CLS_MAX_D, ops.CLS_MAX_CLASSES

    def __init__(self, d: int, num_classes: int, device, task: str = "multiclass", label_smoothing: float = 0.0,
                 pos_weight: Optional[torch.Tensor] = None, init: str = "zeros", std: float = 0.01, seed: int = 0):
        if task not in TASKS:
            raise ValueError(f"ClassifierHead: task must be one of {TASKS}, got {task!r}")
        if not 0.0 <= float(label_smoothing) < 1.0 or (task == "multilabel" and float(label_smoothing) != 0.0):
            raise ValueError("ClassifierHead: label_smoothing must be in [0, 1) and is defined for the multiclass task only")
        if pos_weight is not None and task != "multilabel":
            raise ValueError("ClassifierHead: pos_weight is defined for the multilabel task only")
        super().__init__(d, num_classes, device, pos_weight, init, std, seed)
        self.task, self.label_smoothing = task, float(label_smoothing)

    # -- launches --------------------------------------------------------------------------------------------------------------------------
    def _buffers(self, N: int) -> Dict[str, torch.Tensor]:
        if N != self._key:
            dev, f32 = self.device, torch.float32
            self._ws = {"z": torch.empty((N, self.C), device=dev, dtype=f32), "loss": torch.zeros(1, device=dev, dtype=f32),
                        "counts": torch.zeros(2, device=dev, dtype=torch.int32),
                        "scratch": torch.empty(ops.cls_head_scratch(N, self.d, self.C), device=dev, dtype=f32)}
            self._key = N
        return self._ws

    def logits(self, feat: torch.Tensor) -> torch.Tensor:
        """z [N, C] of fp32 features [N, d]: a new tensor (medmoe_cls_head_logits)."""
        return ops.cls_head_logits(feat, self.weight, self.bias)

    def step(self, feat: torch.Tensor, targets: torch.Tensor, loss_scale: float = 1.0, dfeat: Optional[torch.Tensor] = None):
        """Forward, loss and backward of the head on fp32 features [N, d] (medmoe_cls_head_step): the head's gradient is ACCUMULATED into
        the store's gradient buffer, dfeat [N, d] (when given) is WRITTEN with d loss / d feat.  Returns the device scalars
        (loss, n_valid, n_correct) - views of the head's workspace, valid until its next step; the logits stay in `self.last_logits`."""
        return self._launch(feat, targets, loss_scale, dfeat, self.store.grad(WEIGHT), self.store.grad(BIAS))

    def evaluate(self, feat: torch.Tensor, targets: torch.Tensor):
        """(loss, n_valid, n_correct) and `last_logits` as `step` leaves them at loss_scale 1, with the gradient of the launch going to
        two buffers of the head's workspace that nobody reads: the store's gradient is not touched."""
        ws = self._buffers(feat.shape[0])
        if "eval_dW" not in ws:
            ws["eval_dW"], ws["eval_db"] = torch.zeros_like(self.weight), torch.zeros_like(self.bias)
        return self._launch(feat, targets, 1.0, None, ws["eval_dW"], ws["eval_db"])

    def _launch(self, feat, targets, loss_scale, dfeat, dW, db):
        ws = self._buffers(feat.shape[0])
        tg = prepare_targets(targets, self.task, self.C)
        ops.cls_head_step(feat, self.weight, self.bias, tg, dW, db, task=self.task, label_smoothing=self.label_smoothing,
                          pos_weight=self.pos_weight, loss_scale=loss_scale, z=ws["z"], dx=dfeat, loss=ws["loss"], counts=ws["counts"],
                          scratch=ws["scratch"])
        return ws["loss"][0], ws["counts"][0], ws["counts"][1]


class ScoreBank:
    """Growing fp32 logits [n, C] and int8 targets [n, C] in {0, 1, -1} (multiclass labels are stored one-hot, and as int64 [n] for the
    accuracy), filled batch by batch as EmbeddingBank is."""

    def __init__(self, num_classes: int, device, task: str = "multiclass", capacity: int = 1024):
        if task not in TASKS:
            raise ValueError(f"ScoreBank: task must be one of {TASKS}, got {task!r}")
        self.C, self.device, self.task, self.n = int(num_classes), torch.device(device), task, 0
        self._z = torch.empty((capacity, self.C), device=self.device, dtype=torch.float32)
        self._t = torch.empty((capacity, self.C), device=self.device, dtype=torch.int8)
        self._y = torch.empty((capacity,), device=self.device, dtype=torch.int64)

    def reset(self):
        self.n = 0

    def __len__(self):
        return self.n

    @property
    def scores(self) -> torch.Tensor:
        return self._z[:self.n]

    @property
    def targets(self) -> torch.Tensor:
        return self._t[:self.n]

    @property
    def labels(self) -> torch.Tensor:
        """Multiclass: the class index per row (-1 = not counted)."""
        return self._y[:self.n]

    def _reserve(self, n: int):
        cap = self._z.shape[0]
        if n <= cap:
            return
        cap = max(n, 2 * cap)
        for name in ("_z", "_t", "_y"):
            old = getattr(self, name)
            new = torch.empty((cap,) + tuple(old.shape[1:]), device=self.device, dtype=old.dtype)
            new[:self.n] = old[:self.n]
            setattr(self, name, new)

    def add(self, logits: torch.Tensor, targets: torch.Tensor):
        """Append a batch (copied: views of a head's workspace may be handed in)."""
        b = logits.shape[0]
        if tuple(logits.shape) != (b, self.C):
            raise ValueError(f"ScoreBank.add: expected [B, {self.C}] logits, got {tuple(logits.shape)}")
        targets = targets.to(self.device)
        if (self.task == "multiclass" and targets.numel() != b) or (self.task == "multilabel" and tuple(targets.shape) != (b, self.C)):
            raise ValueError(f"ScoreBank.add: targets of shape {tuple(targets.shape)} do not fit {b} rows of a {self.task} bank")
        self._reserve(self.n + b)
        self._z[self.n:self.n + b] = logits
        self._t[self.n:self.n + b] = targets_as_int8(targets, self.task, self.C)
        self._y[self.n:self.n + b] = targets.reshape(-1).long() if self.task == "multiclass" else -1
        self.n += b


# ---------------------------------------------------------------------------------------------------------------------------------------------
# reducers: plain torch over the integer counts, any device, no kernel call
# ---------------------------------------------------------------------------------------------------------------------------------------------
def auroc_from_counts(counts: torch.Tensor) -> Tuple[torch.Tensor, float]:
    """(per_class float64 [C], mean) from int64 [C, 4] = (n_pos, n_neg, n_less, n_equal): the midrank (Mann-Whitney) AUROC
    (n_less + n_equal / 2) / (n_pos n_neg); NaN for a class without a positive or without a negative, which the mean leaves out (NaN when
    no class is left)."""
    c = counts.to(torch.float64)
    pairs = c[:, 0] * c[:, 1]
    per = torch.where(pairs > 0, (c[:, 2] + 0.5 * c[:, 3]) / pairs.clamp(min=1.0), torch.full_like(pairs, float("nan")))
    ok = pairs > 0
    return per, (float(per[ok].mean()) if bool(ok.any()) else float("nan"))


def auroc(scores: torch.Tensor, targets: torch.Tensor) -> Tuple[torch.Tensor, float]:
    """(per_class float64 [C], mean) AUROC of fp32 scores [N, C] against int8 targets [N, C] in {0, 1, -1}: one medmoe_auroc_counts launch,
    then auroc_from_counts."""
    return auroc_from_counts(ops.auroc_counts(scores.to(torch.float32).contiguous(), targets.to(torch.int8).contiguous()))


def accuracy(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """Share of the rows with a label >= 0 whose argmax (ties: the lowest class) is the label; NaN without such a row."""
    ok = labels >= 0
    n = int(ok.sum())
    if n == 0:
        return float("nan")
    top = (scores == scores.max(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)          # the first maximum
    return float(((top == labels) & ok).sum()) / n


def classification_metrics(bank: ScoreBank, class_names=None) -> Dict[str, float]:
    """{"acc" (multiclass only), "auroc_mean", "auroc/<class>"} over a bank; classes are named by `class_names` or their index."""
    if len(bank) == 0:
        return {}
    per, mean = auroc(bank.scores, bank.targets)
    names = list(class_names) if class_names is not None else [str(c) for c in range(bank.C)]
    if len(names) != bank.C:
        raise ValueError(f"classification_metrics: {len(names)} class names for {bank.C} classes")
    out: Dict[str, float] = {}
    if bank.task == "multiclass":
        out["acc"] = accuracy(bank.scores, bank.labels)
    out["auroc_mean"] = mean
    out.update({f"auroc/{names[c]}": float(v) for c, v in enumerate(per.tolist())})
    return out


def fit_linear_probe(features: torch.Tensor, targets: torch.Tensor, head: ClassifierHead, iters: int, lr: float,
                     weight_decay: float = 0.0) -> torch.Tensor:
    """Full-batch Adam on the head over a bank of frozen features [N, d]: one head step (medmoe_cls_head_step) and one fused Adam launch
    per iteration, no clipping, nothing read back.  Returns the loss history as one device tensor fp32 [iters]."""
    if int(iters) < 1:
        raise ValueError(f"fit_linear_probe: iters must be >= 1, got {iters}")
    features = features.to(torch.float32).contiguous()
    history = torch.empty(int(iters), device=features.device, dtype=torch.float32)
    for it in range(int(iters)):
        head.store.zero_grad()
        loss, _, _ = head.step(features, targets)
        history[it] = loss
        head.adam_step(lr, weight_decay)
    return history

