"""LAMB (You et al., "Large Batch Optimization for Deep Learning", ICLR 2020) as a plain per-tensor torch optimiser.

It states in torch what the fused step computes on the engine's flat stores (medmoe_amd.flat.FlatArena.lamb_step) and has three
uses: the `_target_` of `model.optimizer`; the never-stepped carrier of `lr` for the scheduler and the checkpoints in the fused step; and,
run on float64 tensors, the oracle of the GPU tests.  Conventions: apex FusedLAMB with use_nvlamb = False / timm Lamb with
always_adapt = False - bias-corrected moments, the weight decay inside the update, a trust ratio only for tensors that decay.  Gradient
clipping is the trainer's (clip_grad_norm_ over all parameters before the step), not the optimiser's."""
from typing import Tuple

import torch


class Lamb(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, weight_decay: float = 0.01, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-6,
                 always_adapt: bool = False, trust_clip: bool = False):
        if not lr >= 0.0:
            raise ValueError(f"Lamb: lr must be >= 0, got {lr}")
        if not eps > 0.0:
            raise ValueError(f"Lamb: eps must be > 0, got {eps}")
        if len(tuple(betas)) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
            raise ValueError(f"Lamb: betas must be two values in [0, 1), got {betas}")
        if not weight_decay >= 0.0:
            raise ValueError(f"Lamb: weight_decay must be >= 0, got {weight_decay}")
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay, betas=tuple(betas), eps=eps, always_adapt=bool(always_adapt),
                                      trust_clip=bool(trust_clip)))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            lr, wd, eps = group["lr"], group["weight_decay"], group["eps"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                st["step"] += 1
                t = st["step"]
                m, v = st["exp_avg"], st["exp_avg_sq"]
                m.lerp_(g, 1.0 - b1)
                v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
                bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
                u = (m / bc1) / (v.sqrt() / (bc2 ** 0.5) + eps)
                if wd != 0.0:
                    u = u + wd * p
                r = 1.0
                if group["always_adapt"] or wd != 0.0:
                    wn, un = float(torch.linalg.vector_norm(p)), float(torch.linalg.vector_norm(u))
                    if wn > 0.0 and un > 0.0:
                        r = wn / un
                if group["trust_clip"]:
                    r = min(r, 1.0)
                p.add_(u, alpha=-lr * r)
        return loss
