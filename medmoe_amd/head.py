"""What the supervised linear heads share (classify.ClassifierHead; segment.SegmenterHead): an fp32 weight [C, d] and
bias [C] in a `FlatStore` like every other trained arena - so the clip norm, the fused Adam launch, zero_grad and the Adam-state export are
the arena code that already exists - with their range checks, initialisation, per-class pos_weight and state dict.

A subclass names its parameters (WEIGHT, BIAS) and its limits (MAX_D, MAX_CLASSES), checks its own arguments, and supplies the launches:
`_buffers`, `_launch`, `step`, `evaluate`, `logits`.  Engine._head_step drives any such head through a HeadSpec (engine.py)."""
from typing import Dict, Optional

import torch

from .flat import FlatStore


class LinearHead:
    WEIGHT = BIAS = None                                             # the subclass's parameter names
    MAX_D = MAX_CLASSES = 0

    def __init__(self, d: int, num_classes: int, device, pos_weight: Optional[torch.Tensor], init: str, std: float, seed: int):
        name = type(self).__name__
        if d % 64 or not 64 <= d <= self.MAX_D:
            raise ValueError(f"{name}: d must be a multiple of 64 in 64 .. {self.MAX_D}, got {d}")
        if not 1 <= int(num_classes) <= self.MAX_CLASSES:
            raise ValueError(f"{name}: 1 <= num_classes <= {self.MAX_CLASSES}, got {num_classes}")
        if init not in ("zeros", "zero", "normal"):
            raise ValueError(f"{name}: init must be 'zeros' (or 'zero') or 'normal', got {init!r}")
        self.d, self.C, self.device = int(d), int(num_classes), torch.device(device)
        w = torch.zeros(self.C, self.d)
        if init == "normal":
            w = torch.randn(self.C, self.d, generator=torch.Generator().manual_seed(int(seed))) * float(std)
        pw = None
        if pos_weight is not None:
            pw = torch.as_tensor(pos_weight, dtype=torch.float32).reshape(-1)
            if pw.numel() != self.C:
                raise ValueError(f"{name}: pos_weight must hold {self.C} values, got {pw.numel()}")
        self.store = FlatStore({self.WEIGHT: w, self.BIAS: torch.zeros(self.C)}, self.device)
        self.pos_weight = None if pw is None else pw.to(self.device).contiguous()
        self._ws: Dict[str, torch.Tensor] = {}                       # the launches' buffers of the last batch geometry, allocated on first use
        self._key = None                                             # that geometry

    @property
    def weight(self) -> torch.Tensor:
        return self.store.f32(self.WEIGHT)

    @property
    def bias(self) -> torch.Tensor:
        return self.store.f32(self.BIAS)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {self.WEIGHT: self.weight.detach().clone(), self.BIAS: self.bias.detach().clone()}

    def load_state_dict(self, state: Dict[str, torch.Tensor]):
        where = f"{type(self).__name__}.load_state_dict"
        for name, view in ((self.WEIGHT, self.weight), (self.BIAS, self.bias)):
            if name not in state:
                raise KeyError(f"{where}: {name} is missing")
            if tuple(state[name].shape) != tuple(view.shape):
                raise ValueError(f"{where}: {name} has shape {tuple(state[name].shape)}, this head {tuple(view.shape)}")
            view.copy_(state[name].to(self.device, torch.float32))
        self.store.refresh()

    @property
    def last_logits(self) -> torch.Tensor:
        return self._ws["z"]

    def adam_step(self, lr: float, weight_decay: float = 0.0, clip: float = 0.0, normsq_total: Optional[torch.Tensor] = None, **kw):
        """The arena's fused clip + Adam launch on the head; normsq_total None: the head's own gradient norm."""
        total = self.store.sumsq() if normsq_total is None else normsq_total
        self.store.adam_step(total, lr, weight_decay, clip, **kw)
