"""Masked-language-model head of the text tower (reference losses.py:150-245 MaskedPredictionHead / MaskedPredictionLoss).

    hidden --gather the selected rows--> g --dense + GELU--> t --LayerNorm--> z --tied decoder + bias, cross-entropy--> loss

The decoder's weight is the tower's word-embedding table (`cls.decoder.weight` is not stored twice); the head's own parameters -
`cls.dense.weight`, `cls.dense.bias`, `cls.layer_norm.weight`, `cls.layer_norm.bias`, `cls.bias` [V], the reference's names - live in one
small flat arena (`MLMStore`, a FlatStore: fp32 master, gradient, Adam state, average, bf16 working copies) that the engine steps next to
the towers'.  The number of selected rows is a DEVICE integer: every launch takes it as such, buffers are sized for the bound, nothing is
read back.  `head_forward` / `head_backward` are the launch sequences; the engine (MLMHead) and the `src.losses` classes both run them."""
from typing import Dict, Optional, Tuple

import torch

from . import ops
from .flat import FlatStore

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
HEAD_NAMES = ("cls.dense.weight", "cls.dense.bias", "cls.layer_norm.weight", "cls.layer_norm.bias", "cls.bias")
HEAD_PREFIX = "mlm."                   # the head's entries in reference-style name -> tensor exports
DEFAULT_EPS = 1e-5                     # MaskedPredictionHead(layer_norm_eps=1e-5)


def head_entries(D: int, V: int):
    """(name, shape) of the head's parameters in storage order."""
    return [("cls.dense.weight", (D, D)), ("cls.dense.bias", (D,)), ("cls.layer_norm.weight", (D,)), ("cls.layer_norm.bias", (D,)),
            ("cls.bias", (V,))]


def init_head(D: int, V: int, seed: int = 0, std: float = 0.02) -> Dict[str, torch.Tensor]:
    """Seeded initial values (CPU, fp32): dense ~ N(0, std^2), LayerNorm (1, 0), both biases 0 (BERT's initialisation)."""
    g = torch.Generator().manual_seed(1000003 + seed)
    return {"cls.dense.weight": torch.randn(D, D, generator=g) * std, "cls.dense.bias": torch.zeros(D), "cls.layer_norm.weight": torch.ones(D),
            "cls.layer_norm.bias": torch.zeros(D), "cls.bias": torch.zeros(V)}


class MLMStore(FlatStore):
    """The head's arena.  export_named / load_named speak `mlm.<reference name>`, as the towers' stores speak `text.` / `vit.`."""

    def __init__(self, D: int, V: int, device, seed: int = 0):
        self.D, self.V = D, V
        super().__init__(init_head(D, V, seed), device, gemm=["cls.dense.weight"])
        self.adam_state()

    def export_named(self, flat=None) -> Dict[str, torch.Tensor]:
        flat = self.p32 if flat is None else flat
        return {HEAD_PREFIX + n: self.view(flat, n).detach().float().cpu().contiguous() for n in self.names}

    def load_named(self, named: Dict[str, torch.Tensor]):
        for k, v in named.items():
            if not k.startswith(HEAD_PREFIX):
                continue
            kk = k[len(HEAD_PREFIX):]
            if kk not in self.shapes:
                raise KeyError(f"unknown MLM head parameter {k}")
            if tuple(v.shape) != tuple(self.shapes[kk]):
                raise ValueError(f"{k}: shape {tuple(v.shape)} != {tuple(self.shapes[kk])}")
            self.f32(kk).copy_(v.to(self.device).float())
        self.refresh()


class HeadBuffers:
    """Activations and scratch of one head pass, sized for M_bound rows.  `g` starts as zeros and only ever receives gathered rows, so a row
    past the count is finite: the dense weight gradient runs over all M_bound rows against zeros there."""

    def __init__(self, M_bound: int, D: int, V: int, device):
        self.M_bound, self.D, self.V = M_bound, D, V
        bf = lambda: torch.zeros(M_bound, D, device=device, dtype=BF)
        self.g, self.t, self.aux, self.z, self.dz, self.dt, self.dpre, self.dg = (bf() for _ in range(8))
        self.stat = torch.zeros(2, M_bound, device=device, dtype=F32)
        self.lse = torch.zeros(M_bound, device=device, dtype=F32)
        self.terms = torch.zeros(M_bound, device=device, dtype=F32)
        self.loss = torch.zeros(1, device=device, dtype=F32)
        self.counts = torch.zeros(2, device=device, dtype=I32)
        self.count1 = torch.ones(1, device=device, dtype=I32)      # max(count, 1): the row count of the launches that need one row
        self.scratch = torch.empty(ops.vocab_ce_scratch(M_bound, V, D), device=device, dtype=F32)


def head_forward(buf: HeadBuffers, hidden, rows, row_labels, count, W16, b1, gamma, beta, E16, vbias, loss_scale: float, eps: float):
    """hidden bf16 [R, D] (the tower's row space), rows / row_labels int32 [>= M_bound], count int32 [1] on the device.  Leaves the loss in
    buf.loss (loss_scale * mean over the selected rows), (count, hits) in buf.counts, and what head_backward reads."""
    M, D = buf.M_bound, buf.D
    torch.clamp(count, min=1, out=buf.count1)
    ops.rows_gather(hidden, rows, count, buf.g)
    ops.gemm_nt_rows(buf.g, W16, buf.t, buf.count1, bias=b1, aux=buf.aux, epi=ops.EPI_GELU_DAUX)
    ops.call("layernorm_fwd_rows", buf.t, gamma, beta, buf.z, buf.stat[0], buf.stat[1], M, D, eps, 0, buf.count1)
    ops.vocab_ce_fwd(buf.z, E16, vbias, row_labels, count, loss_scale, lse=buf.lse, terms=buf.terms, loss=buf.loss, counts=buf.counts,
                     scratch=buf.scratch)
    return buf.loss, buf.counts


def head_backward(buf: HeadBuffers, rows, row_labels, count, W16t, gamma, E16, vbias, loss_scale: float, dW, db1, dgamma, dbeta, dE, dvbias,
                  d_hidden=None):
    """The gradients of head_forward's loss: ACCUMULATED into dW [D, D], db1, dgamma, dbeta [D], dE [V, D], dvbias [V] (fp32), and the head's
    d hidden added to the listed rows of d_hidden (bf16 [R, D]) when given."""
    buf.dz[0].zero_()                                                # count = 0: row 0 still passes through the LayerNorm backward, as zeros
    ops.vocab_ce_bwd(buf.z, E16, vbias, row_labels, buf.lse, count, loss_scale, dz=buf.dz, dE=dE, dbias=dvbias)
    ops.layernorm_bwd(buf.dz, buf.t, buf.stat[0], buf.stat[1], gamma, buf.dt, dgamma, dbeta, rows_dev=buf.count1)
    ops.rows_mul(buf.dt, buf.aux, count, buf.dpre)                   # x GELU'; zeros past the count
    ops.gemm_tn(buf.dpre, buf.g, dW, db=db1)
    if d_hidden is not None:
        ops.gemm_nt_rows(buf.dpre, W16t, buf.dg, buf.count1)
        ops.rows_scatter_add(buf.dg, rows, count, d_hidden)


class MLMHead:
    """The engine's head: parameters in `store`, buffers per row bound."""

    def __init__(self, D: int, V: int, device, seed: int = 0, eps: float = DEFAULT_EPS):
        self.D, self.V, self.eps, self.device = D, V, eps, torch.device(device)
        self.store = MLMStore(D, V, device, seed)
        self._bufs: Dict[int, HeadBuffers] = {}
        self.buf: Optional[HeadBuffers] = None                       # the buffers of the last forward

    def buffers(self, M_bound: int) -> HeadBuffers:
        b = self._bufs.get(M_bound)
        if b is None:
            b = self._bufs[M_bound] = HeadBuffers(M_bound, self.D, self.V, self.device)
        return b

    def forward(self, hidden, rows, row_labels, count, E16, loss_scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
        s = self.store
        self.buf = self.buffers(rows.numel())
        self._last = (rows, row_labels, count, E16, loss_scale)
        return head_forward(self.buf, hidden, rows, row_labels, count, s.w16("cls.dense.weight"), s.f32("cls.dense.bias"),
                            s.f32("cls.layer_norm.weight"), s.f32("cls.layer_norm.bias"), E16, s.f32("cls.bias"), loss_scale, self.eps)

    def backward(self, dE, d_hidden=None):
        """Backward of the last forward: the head's gradients into its store, the tied table's into dE (fp32 [V, D], accumulated), d hidden
        added into d_hidden at the selected rows."""
        s = self.store
        rows, row_labels, count, E16, loss_scale = self._last
        head_backward(self.buf, rows, row_labels, count, s.w16t("cls.dense.weight"), s.f32("cls.layer_norm.weight"), E16, s.f32("cls.bias"),
                      loss_scale, s.grad2d("cls.dense.weight"), s.grad("cls.dense.bias"), s.grad("cls.layer_norm.weight"),
                      s.grad("cls.layer_norm.bias"), dE, s.grad("cls.bias"), d_hidden)
