"""What the supervised "head on the fused engine" modules share (classification; segmentation): a head whose weights
live in a FlatStore trains on an output of the MedMoE image tower, as a probe on the frozen tower or together with it.  The same `MedMoE`
net sits under `self.model`; every step runs on the HIP engine, there is no autograd path.  A subclass sets the four names below, builds its
head in its own __init__ between `_init_on_engine` and `_finish_init`, and supplies `fused_training_step` / `fused_eval_step` and the two
epoch hooks of its metric bank."""
from typing import Any, Dict, Optional

import torch
from torch import nn

from .medmoe_module import MedMoEPretrainingLightningModule, _Base


class HeadOnEngineModule(MedMoEPretrainingLightningModule):
    """The checkpoint hooks, configure_fused, set_deterministic and configure_optimizers are the pretraining module's."""

    _KIND = "head"                  # "classifier" / "segmenter": the module's name in messages and its block model.<_KIND>
    _STEP = "Engine.step"           # the engine method that carries the head's launches
    _LAUNCH = "launch"              # what that method has, for the fused_step refusal
    _FEATURE = "output"             # what of the ViT Engine the head trains on, for the Swin refusal
    _DESIGN = "3"

    def _init_on_engine(self, model: nn.Module, optimizer: Any, scheduler: Any, fused_step: bool):
        """The plumbing of __init__ after the subclass has validated its block (and after _Base.__init__): returns the engine."""
        if not fused_step:
            raise NotImplementedError(f"the {self._KIND} module runs on the HIP engine only (model.fused_step=true): {self._STEP} has the "
                                      f"head's {self._LAUNCH}, there is no autograd path")
        self.model = model
        self._optimizer, self._scheduler = optimizer, scheduler
        self.fused_step = True
        self._fused_acc, self._fused_clip, self._fused_opt = 1, None, None
        self._ema_decay, self._ema_warmup, self._ema_validate = 0.0, False, False      # EMA of the head: a named follow-up
        self._retrieval, self._bank = None, None
        self._swin_engine = None
        self.automatic_optimization = False
        eng = getattr(model, "engine", None)
        if eng is None:
            raise NotImplementedError(f"the {self._KIND} module needs the HIP engine behind self.model (src.models.components.med_moe.MedMoE)")
        if getattr(model, "swin", None) is not None:
            raise NotImplementedError(f"model.{self._KIND} with vision.arch = swin_t: the head trains on the ViT Engine's {self._FEATURE} and "
                                      f"backward; the Swin tower is a named follow-up (DESIGN {self._DESIGN})")
        return eng

    def _finish_init(self, head_lr: Optional[float], pretrained_ckpt: Optional[str]):
        """After the head and its parameters exist: the optimiser's keys into the engine's config, then the pretraining checkpoint."""
        self._configure_engine(head_lr)
        if pretrained_ckpt:
            state = torch.load(str(pretrained_ckpt), map_location="cpu", weights_only=True)
            self.load_state_dict(state.get("state_dict", state), strict=False)

    def _configure_engine(self, head_lr: Optional[float] = None):
        """The optimiser's keys into the engine's config (Adam or AdamW: lr, weight_decay, betas, eps)."""
        import functools
        opt, c = self._optimizer, self.model.engine.cfg
        self._head_lr_mult = 1.0
        if opt is None:
            return
        if not isinstance(opt, functools.partial) or opt.func not in (torch.optim.Adam, torch.optim.AdamW) or opt.args \
                or set(opt.keywords) - {"lr", "weight_decay", "betas", "eps"}:
            raise NotImplementedError(f"the {self._KIND} module fuses torch.optim.Adam or torch.optim.AdamW (lr, weight_decay, betas, eps); no "
                                      "other optimizer and no other keyword")
        adamw = opt.func is torch.optim.AdamW
        c.lr = float(opt.keywords.get("lr", 1e-3))
        c.weight_decay = float(opt.keywords.get("weight_decay", 1e-2 if adamw else 0.0))
        c.optimizer = "adamw" if adamw else "adam"
        c.adam_betas = tuple(float(b) for b in opt.keywords.get("betas", (0.9, 0.999)))
        c.adam_eps = float(opt.keywords.get("eps", 1e-8))
        c.validate()
        if head_lr is not None:
            self._head_lr_mult = head_lr / c.lr

    def _head_lr(self) -> float:
        return self.model.engine.cfg.lr * self._head_lr_mult

    def model_step(self, batch: Dict[str, Any]):
        return self.fused_eval_step(batch)

    def training_step(self, batch, batch_idx: int = 0):
        acc = self._fused_acc
        return self.fused_training_step(batch, optimizer_step=(batch_idx + 1) % acc == 0, zero_grad=batch_idx % acc == 0, loss_scale=1.0 / acc)["loss"]

    def validation_step(self, batch, batch_idx: int = 0):
        return self.fused_eval_step(batch)

    def test_step(self, batch, batch_idx: int = 0):
        return self.fused_eval_step(batch)

    def on_test_epoch_start(self):
        return self.on_validation_epoch_start()

    def on_test_epoch_end(self):
        return self.on_validation_epoch_end()

