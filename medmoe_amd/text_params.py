"""Trainable text tower (reference `freeze_bert: false`, text_encoder.py:27-30 leaves the BERT parameters trainable; configs/model/med-moe.yaml:35
freezes them for the pretraining experiment): the tower's parameters as ONE flat fp32 master with flat gradient / Adam-m / Adam-v buffers, a bf16
working copy in the nn.Linear [out, in] layout and a second one with every GEMM weight transposed (dgrad = the same NT kernel as forward) - the
layout of `ParamStore` for the image tower, so the fused clip + Adam kernels and one more all-reduce bucket serve it.

Names are the text tower's own (`layer.{i}.attention.input_proj.weight`, ..., `word_embeddings`, `position_embeddings`,
`token_type_embeddings`, `emb_layernorm.*`: transformer.py:116-130 post-norm blocks under a BERT-style embedding front-end).  `as_dict()` hands
the engine's forward pass the same name -> tensor mapping the frozen tower uses (bf16 GEMM weights, fp32 everything else), as VIEWS of the flat
buffers: an optimiser step updates them in place."""
from typing import Dict, List, Tuple

import torch

from .config import MedMoEConfig
from .flat import FlatArena


class TextStore(FlatArena):
    def __init__(self, cfg: MedMoEConfig, device, init: Dict[str, torch.Tensor]):
        self.cfg = cfg
        c = cfg
        D, ff = c.d_t, c.ff_t
        specs: List[Tuple[str, Tuple[int, ...], str]] = [("word_embeddings", (c.vocab, D), "v"), ("position_embeddings", (c.max_len, D), "v"),
                                                        ("token_type_embeddings", (2, D), "v"), ("emb_layernorm.weight", (D,), "v"),
                                                        ("emb_layernorm.bias", (D,), "v")]
        for i in range(c.n_layer_t):
            b = f"layer.{i}."
            specs += [(b + "attention.input_proj.weight", (3 * D, D), "wt"), (b + "attention.input_proj.bias", (3 * D,), "v"),
                      (b + "attention.output_proj.weight", (D, D), "wt"), (b + "attention.output_proj.bias", (D,), "v"),
                      (b + "attention_layernorm.weight", (D,), "v"), (b + "attention_layernorm.bias", (D,), "v"),
                      (b + "feedforward.model.0.weight", (ff, D), "wt"), (b + "feedforward.model.0.bias", (ff,), "v"),
                      (b + "feedforward.model.2.weight", (D, ff), "wt"), (b + "feedforward.model.2.bias", (D,), "v"),
                      (b + "feedforward_layernorm.weight", (D,), "v"), (b + "feedforward_layernorm.bias", (D,), "v")]
        self.specs = specs
        self.kinds = {n: k for n, _, k in specs}
        super().__init__(device, [(n, s) for n, s, _ in specs], gemm=[(n, False) for n, _, k in specs if k == "wt"])
        self.adam_state()
        dev = self.device
        missing = [n for n in self.shapes if n not in init]
        if missing:
            raise KeyError(f"TextStore: no initial value for {missing[:3]} ...")
        for name in self.shapes:
            self.f32(name).copy_(init[name].to(dev).float().reshape(self.shapes[name]))
        self.refresh()

    def as_dict(self) -> Dict[str, torch.Tensor]:
        """name -> the tensor the forward pass reads: bf16 [out, in] views for the GEMM weights, fp32 views for embeddings, biases, LayerNorms."""
        return {n: (self.w16(n) if self.kinds[n] == "wt" else self.f32(n)) for n in self.shapes}

    def load_named(self, named: Dict[str, torch.Tensor]):
        """`text.<name>` entries of a reference-style dict into the master buffer (then refresh the working copies)."""
        for k, v in named.items():
            if not k.startswith("text."):
                continue
            kk = k[len("text."):]
            if kk not in self.shapes:
                raise KeyError(f"unknown text parameter {k}")
            if tuple(v.shape) != tuple(self.shapes[kk]):
                raise ValueError(f"{k}: shape {tuple(v.shape)} != {tuple(self.shapes[kk])}")
            self.f32(kk).copy_(v.to(self.device).float())
        self.refresh()

    def export_named(self, flat=None) -> Dict[str, torch.Tensor]:
        flat = self.p32 if flat is None else flat
        return {"text." + n: self.view(flat, n).detach().float().cpu().contiguous() for n in self.shapes}
