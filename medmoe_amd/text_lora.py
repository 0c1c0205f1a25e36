"""LoRA adapters of a tower's attention projections: the text tower's (cfg.text_lora; reference configs/model/med-moe.yaml:27-30 names the keys, vision_encoder.py:30-36 sketches
peft's LoraConfig(target_modules=["query", "value"])).  The base tower stays the frozen bf16 dict of `ParamStore.text`; what trains
is this arena: per layer and target t in (query, key, value) peft's `lora_A` [r, D] and `lora_B` [D, r], the update of the target's slice of
the fused q / k / v projection being s * B A with s = lora_alpha / r.

Storage is padded to rank 16 INSIDE the arena (`layer.{l}.attention.{t}.lora_A` is [16, D], `.lora_B` [D, 16]): the side path runs on the 16-wide
MFMA and the bf16 working copies are its operands as they are.  The pad rows of A and the pad columns of B start at zero and receive exactly
zero gradient (d U's pad columns are dqkv times B's zero columns, U's pad columns are x times A's zero rows), so Adam and AdamW leave them at
zero.  A layer's A matrices lie back to back (`layer.{l}.lora_A` = A_cat [n_t * 16, D], one MFMA operand for all targets), so do its B matrices
(`layer.{l}.lora_B` = [n_t * D, 16]); both are GEMM weights of the arena, so `w16t` holds them transposed - the backward's operands.
Checkpoints and `export_named` carry the true [r, D] / [D, r] shapes.

The image tower's adapters (cfg.vit_lora) are the SAME class: `LoraStore.for_vit` builds it from the vit_lora_* keys with D = d_v,
L = n_layer_v, the export prefix `vit.` and an init stream of its own.  What differs between the towers is data: the prefix, r, alpha, D, L,
the targets and the stream."""
import math
from typing import Dict, List, Tuple

import torch

from . import ops
from .config import MedMoEConfig
from .flat import FlatArena

RP = ops.LORA_RANK_PAD


class LoraStore(FlatArena):
    def __init__(self, device, prefix: str, r: int, alpha: float, D: int, L: int, targets, init_seed: int):
        """prefix: what the adapters' names carry outside the arena (`text.` / `vit.`: load_named, export_named); init_seed: the stream A is
        drawn from."""
        self.prefix = prefix
        self.r, self.D, self.L = int(r), int(D), int(L)
        self.scale = float(alpha) / self.r
        targets = (targets,) if isinstance(targets, str) else tuple(targets)
        self.targets: Tuple[str, ...] = tuple(t for t in ops.LORA_TARGETS if t in targets)     # column order of the fused row
        D = self.D
        entries: List[Tuple[str, Tuple[int, ...]]] = []
        groups, gemm = [], []
        for l in range(self.L):
            a_names = [self.name(l, t, "A") for t in self.targets]
            b_names = [self.name(l, t, "B") for t in self.targets]
            entries += [(n, (RP, D)) for n in a_names] + [(n, (D, RP)) for n in b_names]
            groups += [(f"layer.{l}.lora_A", a_names), (f"layer.{l}.lora_B", b_names)]
            gemm += [(f"layer.{l}.lora_A", False), (f"layer.{l}.lora_B", False)]
        super().__init__(device, entries, groups, gemm)
        self.adam_state()
        # peft's init: A Kaiming-uniform with a = sqrt(5) (bound 1 / sqrt(fan_in)), B zero - the adapted tower starts as the base tower
        g = torch.Generator(device="cpu").manual_seed(int(init_seed))
        bound = 1.0 / math.sqrt(D)
        for l in range(self.L):
            for t in self.targets:
                a = (torch.rand(self.r, D, generator=g) * 2.0 - 1.0) * bound
                self.f32(self.name(l, t, "A"))[:self.r].copy_(a.to(self.device))
        self.refresh()

    @classmethod
    def for_text(cls, cfg: MedMoEConfig, device, seed: int = 0) -> "LoraStore":
        """cfg.text_lora: the text tower's adapters (stream seed + 2: ParamStore draws the towers from seed and seed + 1)."""
        return cls(device, "text.", cfg.text_lora_r, cfg.text_lora_alpha, cfg.d_t, cfg.n_layer_t, cfg.text_lora_targets, int(seed) + 2)

    @classmethod
    def for_vit(cls, cfg: MedMoEConfig, device, seed: int = 0) -> "LoraStore":
        """cfg.vit_lora: the image tower's adapters (stream seed + 3)."""
        return cls(device, "vit.", cfg.vit_lora_r, cfg.vit_lora_alpha, cfg.d_v, cfg.n_layer_v, cfg.vit_lora_targets, int(seed) + 3)

    @staticmethod
    def name(l: int, t: str, which: str) -> str:
        return f"layer.{l}.attention.{t}.lora_{which}"

    def true_names(self) -> List[str]:
        return [self.name(l, t, w) for l in range(self.L) for t in self.targets for w in ("A", "B")]

    def true_view(self, flat, name: str) -> torch.Tensor:
        """The [r, D] / [D, r] part of a stored adapter matrix (a view of `flat`)."""
        v = self.view(flat, name)
        return v[:self.r] if name.endswith("lora_A") else v[:, :self.r]

    # the operands of a layer's launches
    def A16(self, l): return self.w16(f"layer.{l}.lora_A")          # [n_t * 16, D]
    def B16(self, l): return self.w16(f"layer.{l}.lora_B")          # [n_t * D, 16]
    def A16t(self, l): return self.w16t(f"layer.{l}.lora_A")        # [D, n_t * 16]
    def B16t(self, l): return self.w16t(f"layer.{l}.lora_B")        # [16, n_t * D]
    def gA(self, l): return self.grad(f"layer.{l}.lora_A")
    def gB(self, l): return self.grad(f"layer.{l}.lora_B")

    def load_named(self, named: Dict[str, torch.Tensor]):
        """`<prefix>layer.{l}.attention.{t}.lora_A[.weight]` / `.lora_B[.weight]` entries (true shapes) into the master buffer; entries that
        are not adapters are left to the caller.  The pad rows / columns stay zero."""
        for k, v in named.items():
            if not k.startswith(self.prefix) or ".lora_" not in k:
                continue
            kk = k[len(self.prefix):]
            kk = kk[:-len(".weight")] if kk.endswith(".weight") else kk
            if kk not in self.shapes or kk in self.groups:
                raise KeyError(f"unknown adapter parameter {k} (targets {self.targets}, {self.L} layers)")
            dst = self.true_view(self.p32, kk)
            if tuple(v.shape) != tuple(dst.shape):
                raise ValueError(f"{k}: shape {tuple(v.shape)} != {tuple(dst.shape)}")
            dst.copy_(v.to(self.device).float())
        self.refresh()

    def export_named(self, flat=None) -> Dict[str, torch.Tensor]:
        flat = self.p32 if flat is None else flat
        return {self.prefix + n: self.true_view(flat, n).detach().float().cpu().contiguous() for n in self.true_names()}

    def pad_is_zero(self, flat=None) -> bool:
        flat = self.p32 if flat is None else flat
        for n in self.true_names():
            v = self.view(flat, n)
            pad = v[self.r:] if n.endswith("lora_A") else v[:, self.r:]
            if pad.numel() and bool((pad != 0).any()):
                return False
        return True
