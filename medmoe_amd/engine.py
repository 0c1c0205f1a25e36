"""Hand-scheduled forward / backward / optimiser step of the MedMoE contrastive hot path.

One process drives one MI355X.  Every arithmetic step is a C-ABI HIP kernel launch
(`medmoe_amd.ops`) on torch's current stream into buffers allocated once per batch size;
torch is used for device memory, streams and (multi-GPU) `torch.distributed` only.

Reference call stack being replaced: MedMoE.forward (med_moe.py:102-108) ->
encode_text / encode_image -> SWIN.forward (swin.py:130-149) -> MoE.forward (swin.py:94-117);
model_step (medmoe_module.py:284-316) -> GLORIA local/global losses (losses.py:757-794,
954-1026) + CE on router probabilities (medmoe_module.py:235-237).
"""
import collections
import contextlib
import os
from typing import Callable, Dict, NamedTuple, Optional

import numpy as np
import torch

from . import ema as ema_
from . import ops
from .local_generic import GenericLocalLoss
from .local_ragged import RaggedLocalLoss
from .local_transposed import TransposedLocalLoss, local_sim_forward, ragged_layout  # noqa: F401  (ragged_layout: the tests and tools use it from here)
from .config import MedMoEConfig
from .flat import fused_step_of
from .params import ParamStore

BF = torch.bfloat16
F32 = torch.float32
I32 = torch.int32


class VocabTables:
    """What word-piece aggregation needs from the tokenizer vocabulary (text_encoder.py:23,47-74)."""

    def __init__(self, is_continuation: torch.Tensor, starts_bracket: torch.Tensor, sep_id=2, cls_id=1, pad_id=0):
        self.is_cont = is_continuation.bool()
        self.starts_bracket = starts_bracket.bool()
        self.sep_id, self.cls_id, self.pad_id = sep_id, cls_id, pad_id

    @staticmethod
    def synthetic(vocab: int, device, n_continuation: int = 0):
        cont = torch.zeros(vocab, dtype=torch.bool, device=device)
        if n_continuation:
            cont[vocab - n_continuation:] = True
        br = torch.zeros(vocab, dtype=torch.bool, device=device)
        br[:3] = True
        return VocabTables(cont, br)

    def segment_map(self, ids: torch.Tensor, out=None):
        """(out: optional (seg, cap) int32 device buffers to write into - the engine keeps one pair per batch size.)  The token loop of text_encoder.py:45-76 on the device (no host sync): seg[b,t] = word index of token t (-1 = dropped), cap_lens
        per medmoe_module.py:221-223.  One kernel launch (medmoe_segment_map); `segment_map_torch` is the same rule in torch ops (the
        tests compare the two and the oracle)."""
        B, T = ids.shape
        if not ids.is_cuda:
            return self.segment_map_torch(ids)
        if ids.dtype not in (torch.int64, torch.int32) or not ids.is_contiguous():
            ids = ids.to(torch.int64).contiguous()
        if out is not None:
            seg, cap = out
        else:
            seg = torch.empty(B, T, device=ids.device, dtype=I32); cap = torch.empty(B, device=ids.device, dtype=I32)
        ops.call("segment_map", ids, 1 if ids.dtype == torch.int64 else 0, self.is_cont.view(torch.uint8), self.starts_bracket.view(torch.uint8),
                 seg, cap, B, T, self.is_cont.numel(), self.sep_id)
        return seg, cap

    def segment_map_torch(self, ids: torch.Tensor):
        B, T = ids.shape
        pos = torch.arange(T, device=ids.device)[None]
        is_sep = ids == self.sep_id
        has_sep = is_sep.any(dim=1, keepdim=True)
        sep_pos = torch.where(has_sep, is_sep.float().argmax(dim=1, keepdim=True), torch.full_like(ids[:, :1], T))
        valid = pos <= sep_pos
        start = (~self.is_cont[ids]) & valid
        start[:, 0] = True
        seg = torch.cumsum(start.int(), dim=1) - 1
        n_words = torch.where(has_sep[:, 0], seg.gather(1, sep_pos.clamp(max=T - 1))[:, 0] + 1, seg[:, -1])
        # without a [SEP] the loop never flushes the last bank: that word is dropped
        seg = torch.where(valid & (seg < n_words[:, None]), seg, torch.full_like(seg, -1))
        first_br = self.starts_bracket[ids] & start & (seg >= 0)
        n_real = (start & (seg >= 0)).sum(dim=1) - first_br.sum(dim=1)
        return seg.to(I32).contiguous(), (n_real + 1).to(I32).contiguous()


class _TextRows:
    """One text pass: the launches that depend on its row layout, and what the pass leaves for whoever runs after it.  Every pass builds one -
    the frozen tower's, a trainable tower's, the frozen-style pass of forward_text(embedded=...) - and the block loops (`Engine._text_blocks`,
    `Engine.backward_text`) are written once against it.
    padded: all B x T rows, key-masked attention.  packed (only up to B <= 1024 and T <= 80, else the pass is padded): `text_pack`
    runs here; every launch then takes the device-side row count `cnt` (the first `cnt` rows of the same buffers hold the non-padding tokens
    in (caption, position) order), attention the sequence offsets, the weight gradients one row range [0, cnt] - nothing is copied to the host.
    Left by the pass: `last` (the last hidden state; with `seq_off` what text_soft_target reads), and for `backward_text`, which takes the same
    launches under the same masks: `ids32` / `tt32` / `km`, `seg` (the segment map the aggregation consumed), `first_sel` (the first summed
    hidden state), `drop_step` / `lora_drop_step` (the step whose hidden + attention / LoRA dropout masks the pass applied; None: none)."""

    def __init__(self, eng, km: torch.Tensor, packed: bool, trainable: bool):
        c = eng.cfg
        self.cfg, self.km = c, km
        self.packed = packed = packed and eng.B <= 1024 and c.max_len <= 80
        self.B, self.T, self.H, self.Dt, self.eps = eng.B, c.max_len, c.n_head_t, c.d_t, c.eps_t
        self.tok_row = self.src_row = self.seq_off = self.row_off = self.cnt = None
        self.ids32 = self.tt32 = self.seg = self.first_sel = self.last = self.drop_step = self.lora_drop_step = None
        if packed:
            # ws["tpack"]: tok_row | src_of_row | seq_off | the frozen pass' count | 0 | a trainable pass' count
            pk, Mt, B = eng.ws["tpack"], eng.B * c.max_len, eng.B
            self.tok_row, self.src_row, self.seq_off = pk[:Mt], pk[Mt:2 * Mt], pk[2 * Mt:2 * Mt + B + 1]
            if trainable:
                self.row_off, self.cnt = pk[2 * Mt + B + 2:2 * Mt + B + 4], pk[2 * Mt + B + 3:2 * Mt + B + 4]  # [0, count] and its second element
            else:
                self.cnt = pk[2 * Mt + B + 1:2 * Mt + B + 2]
            ops.call("text_pack", km, self.tok_row, self.src_row, self.seq_off, self.cnt, B, self.T)

    def rng(self, site: int, p: float):
        """The generator of a hidden / attention dropout site under this pass' masks; None: the site drops nothing."""
        return ops.dropout_rng(self.cfg.dropout_seed, self.drop_step, site, p) if self.drop_step is not None and p > 0.0 else None

    def lora_rng(self, l: int):
        if self.lora_drop_step is None:
            return None
        return ops.dropout_rng(self.cfg.dropout_seed, self.lora_drop_step, 4 * l + ops.DROPOUT_SITE_LORA, self.cfg.text_lora_dropout)

    def gemm(self, a, w, out, **kw):
        return ops.gemm_nt_rows(a, w, out, self.cnt, **kw) if self.packed else ops.gemm_nt(a, w, out, **kw)

    def wgrad(self, g, x, dw, db=None):
        if dw is None:             # no gradient target (a frozen base under LoRA adapters): no launch
            return None
        if self.packed:            # the grouped form with ONE group: the row ranges are enumerated from row_off on the device, M bounds them
            return ops.gemm_tn(g, x, dw, db=db, row_off=self.row_off, n_groups=1, M=self.B * self.T)
        return ops.gemm_tn(g, x, dw, db=db)

    def ln(self, x, gamma, beta, y, st):
        if self.packed:
            return ops.call("layernorm_fwd_rows", x, gamma, beta, y, st[0], st[1], self.B * self.T, self.Dt, self.eps, 0, self.cnt)
        return ops.layernorm_fwd(x, gamma, beta, y, st[0], st[1], self.eps)

    def ln_bwd(self, dy, x, mean, rstd, gamma, dx, dgamma=None, dbeta=None):
        return ops.layernorm_bwd(dy, x, mean, rstd, gamma, dx, dgamma, dbeta, rows_dev=self.cnt)

    def attn(self, qkv, out, lse, rng=None):
        """rng: the attention-probability dropout's generator (padded passes only: Engine.__init__ refuses it with the packed one)."""
        if rng is not None:
            return ops.attn_drop_fwd(qkv, out, lse, self.km, self.B, self.T, self.H, rng)
        if self.packed:
            return ops.call("attn_fwd_varlen", qkv, out, lse, self.seq_off, self.B, self.T, self.H, 64)
        return ops.attn_fwd(qkv, out, lse, self.km, self.B, self.T, self.H)

    def attn_bwd(self, qkv, out, dout, lse, dqkv, delta, rng=None):
        if rng is not None:
            return ops.attn_drop_bwd(qkv, out, dout, lse, self.km, dqkv, delta, self.B, self.T, self.H, rng)
        if self.packed:
            return ops.attn_bwd_varlen(qkv, out, dout, lse, self.seq_off, dqkv, delta, self.B, self.T, self.H)
        return ops.attn_bwd(qkv, out, dout, lse, self.km, dqkv, delta, self.B, self.T, self.H)


# The buffers of one block of a forward pass (`Engine._text_blocks`): x -> qkv -> att (+ lse) -> x1 = x + out_proj -> r = LN1(x1) (st1) ->
# h = GELU(FC1 r) (aux: the GELU derivative, kept for the backward, or None) -> x2 = r + FC2 h -> out = LN2(x2) (st2); lu: the adapters' U
# (None: the pass takes no adapter launch)
_TextBufs = collections.namedtuple("_TextBufs", "qkv att lse x1 st1 r h aux x2 st2 out lu")


# Activation recomputation of the image tower (cfg.vit_checkpoint).  A layer's eight bf16 activations and where a mode keeps them:
# per layer under the names below, or (the names listed for the mode) in one of TWO shared sets "ck{l % 2}_<name>", filled again before the
# layer's backward.  The LayerNorm statistics st1_{l} / st2_{l} and lse{l} are kept per layer in every mode.
_VIT_ACT = {"x": "x{}", "ln1": "ln1_{}", "qkv": "qkv{}", "att": "att{}", "xmid": "xmid{}", "ln2": "ln2_{}", "z": "z{}", "h": "h{}"}
_VIT_SHARED = {"none": (), "selective": ("ln1", "ln2", "z", "h"), "full": ("ln1", "qkv", "att", "xmid", "ln2", "z", "h")}


def vit_activation_plan(cfg: MedMoEConfig, B: int, mode: str) -> Dict[str, tuple]:
    """Buffer name -> (shape, dtype) of everything `Engine._alloc` allocates for the image tower's activations at batch B under
    cfg.vit_checkpoint = mode: the layer inputs x0 .. x{L}, per layer what the mode keeps, the statistics and lse, and the two shared sets
    of what it recomputes.  Pure host arithmetic (no GPU, no library): the memory a mode needs can be read off before anything is built."""
    if mode not in _VIT_SHARED:
        raise ValueError(f"vit_checkpoint must be one of {tuple(_VIT_SHARED)}, got {mode!r}")
    Nt, Dv, L, H = cfg.n_tok_v, cfg.d_v, cfg.n_layer_v, cfg.n_head_v
    M = B * Nt
    width = {"x": Dv, "ln1": Dv, "qkv": 3 * Dv, "att": Dv, "xmid": Dv, "ln2": Dv, "z": cfg.ff_v, "h": cfg.ff_v}
    shared = _VIT_SHARED[mode]
    plan = {}
    for l in range(L + 1):
        plan[f"x{l}"] = ((M, Dv), BF)
    for l in range(L):
        for n in ("ln1", "st1", "qkv", "att", "lse", "xmid", "ln2", "st2", "z", "h"):      # the order of the workspace before the modes existed
            if n in ("st1", "st2"):
                plan[f"{n}_{l}"] = ((2, M), F32)
            elif n == "lse":
                plan[f"lse{l}"] = ((B * H * Nt,), F32)
            elif n not in shared:
                plan[_VIT_ACT[n].format(l)] = ((M, width[n]), BF)
    for s in range(2 if shared else 0):
        for n in shared:
            plan[f"ck{s}_{n}"] = ((M, width[n]), BF)
    return plan


def plan_bytes(plan: Dict[str, tuple]) -> int:
    """Total bytes of a buffer plan (vit_activation_plan)."""
    return sum(int(np.prod(shape)) * {BF: 2, F32: 4}[dt] for shape, dt in plan.values())


class HeadSpec(NamedTuple):
    """What Engine._head_step / _head_eval need to know of a supervised task (one constant per task below): where the head reads its
    features, which workspace gradient it writes and which stays zero, the batch key of its targets, how its output tuple becomes the
    result dict, and the words of the refusals."""
    feat: str                       # ws key of the features the head reads
    d_written: str                  # ws key of the gradient the head writes under fine-tuning ...
    d_zeroed: str                   # ... and of the one that is zeroed: backward(None) reads both
    target: str                     # batch key of the targets
    result: Callable                # the head's output tuple -> the dict a step returns (device tensors)
    step: str                       # the public methods' names, the task's, its DESIGN section and what an all-reduce would have to carry
    eval: str
    task: str
    design: str
    unreduced: str


def _classify_result(out):
    loss, n_valid, n_correct = out
    return {"loss": loss, "n_valid": n_valid, "n_correct": n_correct, "acc": n_correct.float() / n_valid.clamp(min=1).float()}


def _segment_result(out):
    loss, counts = out
    return {"loss": loss, "counts": counts, "n_valid": counts[:, 0].sum()}


CLASSIFY = HeadSpec("img_g", "d_img_g", "d_img_l", "label", _classify_result, "classify_step", "classify_eval", "classification", "3p",
                    "the head's gradient has")
SEGMENT = HeadSpec("img_l", "d_img_l", "d_img_g", "mask", _segment_result, "segment_step", "segment_eval", "segmentation", "3t",
                   "the head's gradient and the batch-Dice sums have")


class Engine:
    def __init__(self, cfg: MedMoEConfig, device="cuda:0", seed: int = 0, vocab: Optional[VocabTables] = None):
        cfg.validate()
        # train-mode dropout of the trainable text tower (cfg.text_hidden_dropout / cfg.text_attn_dropout): acts in the padded text pass of
        # train_step and in backward_text only; the mask is a function of (cfg.dropout_seed, self.dropout_step, site, element)
        self.text_dropout = cfg.text_hidden_dropout > 0.0 or cfg.text_attn_dropout > 0.0
        self.dropout_step = 0                                        # one per train_step call, counted on the host; travels with the checkpoint
        if self.text_dropout and cfg.freeze_text and not cfg.text_lora:
            raise NotImplementedError("text_hidden_dropout / text_attn_dropout > 0 (model.model.text.hidden_dropout_prob / "
                                      "attention_probs_dropout_prob) with freeze_text=True (text.freeze_bert: true): dropout is built for the "
                                      "trainable tower's padded pass, not for the packed frozen one")
        if self.text_dropout:
            self._refuse_with_graph("text_hidden_dropout / text_attn_dropout", "model.model.text.hidden_dropout_prob / attention_probs_dropout_prob")
        if cfg.text_mlm:
            self._refuse_mlm_with_graph()
        # stochastic depth of the image tower (cfg.vit_drop_path).  train_step draws the per-sample scales of every site of the step
        # (ws["vit_dp"], [n_layer_v, 2, B] fp32: 0 | 1 / (1 - p_l); [:, 0] the attention branch, [:, 1] the feed-forward branch) and points
        # vit_drop_scales at them for its own forward and backward; None everywhere else: eval_step, forward_image outside a training step and the
        # exports never drop.  Tests (and callers that drive _vit_blocks / _vit_backward themselves) may assign a tensor of that shape: the layers
        # with p_l > 0 then take the scaled launches with exactly these values, until it is set back to None.
        self.vit_drop_scales: Optional[torch.Tensor] = None
        if cfg.vit_drop_path > 0.0:
            self._refuse_with_graph("vit_drop_path", "model.model.vision.drop_path_rate")
        # activation recomputation of the image tower (cfg.vit_checkpoint or MEDMOE_VIT_CHECKPOINT): fixed for the engine's life,
        # the workspace is laid out for it (_alloc) and every _vit_backward recomputes what the mode did not keep
        self.vit_checkpoint = cfg.vit_checkpoint_mode()
        self._ck_shared = _VIT_SHARED[self.vit_checkpoint]
        if self.vit_checkpoint != "none" and os.environ.get("MEDMOE_GRAPH", "0") == "1":
            raise NotImplementedError(f"vit_checkpoint={self.vit_checkpoint!r} (model.model.vision.grad_checkpointing, MEDMOE_VIT_CHECKPOINT) with "
                                      "MEDMOE_GRAPH=1: the recomputation's waits on the second stream have not been verified under hipGraph "
                                      "capture")
        if not torch.cuda.is_available():
            raise RuntimeError("medmoe_amd.Engine needs a GPU: the HIP path is the only path")
        self.cfg = cfg
        self.device = torch.device(device)
        # deterministic mode (cfg.deterministic, MEDMOE_DETERMINISTIC=1, Trainer(deterministic=True) -> set_deterministic): every launch of a
        # step that sums in arrival order is replaced by its staged / single-writer form; self._det owns the scratch buffers, one per stream
        self.deterministic, self._det = False, None
        self.set_deterministic(cfg.deterministic or os.environ.get("MEDMOE_DETERMINISTIC", "0") == "1")
        torch.cuda.set_device(self.device)
        self.params = ParamStore(cfg, self.device, seed)
        # frozen image backbone (cfg.freeze_vit, or implied by cfg.vit_lora): ParamStore keeps gradient / Adam / average buffers
        # for the router and the experts only, _vit_backward runs no tower weight gradient.  vit_lora: rank-r adapters on slices of every
        # block's fused q / k / v projection train in an arena of their own - the text adapters' class and launches.  Their dropout
        # (cfg.vit_lora_dropout) acts in the passes of train_step only: _vit_lora_drop_step is the step whose masks a pass applies, None
        # everywhere else (eval_step, a bare forward_image and the exports apply the adapters without dropout)
        self.vit_frozen = cfg.vit_frozen
        self.vlora = None
        self._vit_lora_drop_step: Optional[int] = None
        if cfg.vit_lora:
            if cfg.vit_lora_dropout > 0.0:
                self._refuse_with_graph("vit_lora_dropout", "model.model.vision.lora_dropout")
            from .text_lora import LoraStore
            self.vlora = LoraStore.for_vit(cfg, self.device, seed)
        self.vocab = vocab or VocabTables.synthetic(cfg.vocab, self.device)
        self.B = 0
        self.ws: Dict[str, torch.Tensor] = {}
        self.rank, self.world = 0, 1
        self._seg = None; self._cap_host = None; self._cap_event = None; self.cap_lens = None
        self._local = None                                           # THE local-loss object of the current (batch size, world, mode): _local_loss_object
        self._gle = None                                             # GenericLocalLoss of eval_step at 256 regions (its forward launches only)
        self.dist = False        # take the data-parallel exchange steps (all-gather / reduce-scatter / bucketed all-reduce)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.rank, self.world = torch.distributed.get_rank(), torch.distributed.get_world_size()
            # MEDMOE_DIST_WORLD1=1: run the collectives even in a one-rank group, so that the RCCL path (backend "nccl",
            # async buckets, stream ordering) can be exercised on a single GPU (tests/test_rccl_world1_gpu.py)
            self.dist = self.world > 1 or os.environ.get("MEDMOE_DIST_WORLD1") == "1"
        # bf16 gradient exchange (cfg.grad_comm_dtype = "bf16" or MEDMOE_GRAD_COMM=bf16): read per step through grad_comm(),
        # because the Lightning module writes its keys into cfg after the engine exists
        env_comm = os.environ.get("MEDMOE_GRAD_COMM", "")
        if env_comm not in ("", "fp32", "bf16"):
            raise ValueError(f"MEDMOE_GRAD_COMM must be 'fp32' or 'bf16', got {env_comm!r}")
        self._grad_comm_env = env_comm == "bf16"
        # trainable text tower (cfg.freeze_text = False; reference freeze_bert: false): flat master / gradient / Adam buffers of its own, the padded
        # text pass with saved activations, a text backward, and the local loss in its word-gradient mode
        # LoRA (cfg.text_lora): the base tower stays the frozen bf16 dict, rank-r adapters on slices of the fused q / k / v projection
        # train in a small arena of their own (medmoe_amd/text_lora.py).  Everything keyed on train_text follows: the padded pass, the word
        # gradients, backward_text (which then skips every base weight gradient), the text dropouts
        self.text_lora = bool(cfg.text_lora)
        self.train_text = (not cfg.freeze_text) or self.text_lora
        self.tstore = None
        self.lora = None
        self._base_t: Dict[str, tuple] = {}                          # LoRA: transposed bf16 copies of the frozen base's GEMM weights (dgrad operands)
        if self.train_text and cfg.soft_label:
            raise NotImplementedError("soft_label with a trainable text tower: the reference scores captions with a SEPARATE frozen BERT "
                                      "(medmoe_module.py:207-210); this build takes them from the tower itself, which must then stay frozen")
        if self.text_lora:
            if cfg.text_lora_dropout > 0.0:
                self._refuse_with_graph("text_lora_dropout", "model.model.text.lora_dropout")
            from .text_lora import LoraStore
            self.lora = LoraStore.for_text(cfg, self.device, seed)
            self.refresh_text_base()
        elif self.train_text:
            from .text_params import TextStore
            self.tstore = TextStore(cfg, self.device, self.params.text)
            self.params.text = self.tstore.as_dict()             # views of the flat buffers: an optimiser step updates them in place
        # masked-language-model objective (cfg.text_mlm): the head's arena is stepped next to the towers'.  _mlm_pass = (step, loss
        # scale) while the text pass that runs is to mask its ids and run the head (train_step, mlm_eval); None everywhere else: eval_step,
        # embed* and classify_* never mask
        self.mlm = None
        self._mlm_pass = None
        self._mlm_bufs: Dict[tuple, tuple] = {}                      # the mask launch's outputs per batch shape
        self._seed = seed
        if cfg.text_mlm:
            self._make_mlm_head()
        self.apply_optimizer_groups()
        # weight EMA (cfg.ema_decay > 0): every arena this engine steps keeps an fp32 average, updated by its Adam launch;
        # ema_weights() points the working copies at it.  The Lightning module writes the key after the engine exists: optimizer_step looks
        self._ema_active = False
        if cfg.ema_decay > 0.0:
            ema_.prepare(self.optimizer_stores().values())
        self.HWp, self.Tp, self.GW = ops.local_geometry(cfg.n_patch, cfg.max_len)
        # LDS-tiled pair kernels exist for 64 / 208 / 256 regions; any other geometry (576 regions of ViT-L/14 at 336 px) runs
        # the generic GEMM formulation (medmoe_amd/local_generic.py)
        self.text_varlen = os.environ.get("MEDMOE_TEXT_VARLEN", "1") != "0" and not self.train_text
        # the TRAINABLE tower's packed pass (cfg.text_train_varlen or MEDMOE_TEXT_TRAIN_VARLEN=1): forward, backward and eval_step on the
        # non-padding tokens, under the rule of every packed pass (_TextRows: else the padded pass); text_train_varlen_active: which one ran
        self.text_train_varlen = self.train_text and (bool(cfg.text_train_varlen) or os.environ.get("MEDMOE_TEXT_TRAIN_VARLEN", "0") == "1")
        self.text_train_varlen_active = False
        # every text pass builds a _TextRows (its row layout, and what it leaves behind): _tp is the last TRAINABLE pass' - backward_text takes
        # the same launches under the same masks, and a frozen-style pass in between (forward_text(embedded=...)) leaves it alone; _rows is
        # the most recent pass' of either kind (text_soft_target)
        self._tp = self._rows = None
        if self.text_train_varlen and cfg.text_attn_dropout > 0.0:
            raise NotImplementedError("text_train_varlen (MEDMOE_TEXT_TRAIN_VARLEN=1) with text_attn_dropout > 0: the attention-probability "
                                      "dropout kernels have no packed form yet (DESIGN 3i)")
        self.local_fast = ops.local_fast_path(cfg.n_patch, cfg.max_len)
        # transposed pair matrices + one wave per (image, caption, word tile): geometries pair3.hip is instantiated for (196 / 64
        # regions); MEDMOE_LOCAL_PAIR3=0 keeps the [region][word] kernels (local_pair2) for A/B runs
        self.local_t = (self.local_fast and ops.local_pair3_supported(cfg.n_patch, cfg.max_len) and cfg.d_out % 32 == 0 and cfg.d_out >= 128
                        and os.environ.get("MEDMOE_LOCAL_PAIR3", "1") != "0")
        # the per-image Gram gradient from ONE operand: the backward pair launch stores a row weight per word instead of the U matrix
        # (MEDMOE_LOCAL_GRAM=0: the two-operand form, for A/B runs)
        self.local_gram = self.local_t and os.environ.get("MEDMOE_LOCAL_GRAM", "1") != "0"
        # region columns stored per (word, image) in the transposed pair matrices (MEDMOE_PAIR_PITCH, for A/B runs; default HWp)
        self.HWq = int(os.environ.get("MEDMOE_PAIR_PITCH", self.HWp))
        # gradient buckets in flat-buffer order: [embeddings | layer 0 | ... | layer L-1 | final LN + router + experts]
        # (a frozen backbone: ONE bucket, the router and the experts - indices of the gradient buffer, which then holds that tail only)
        off = self.params.offsets
        self.bucket_bounds = [0] + [off[f"vit.layer.{l}.attention_layernorm.weight"] for l in range(cfg.n_layer_v)] \
            + [off["vit.final_layer_norm.weight"], self.params.numel]
        self.bucket_bounds = self.params.grad_bounds(self.bucket_bounds)
        if any(b % 8 for b in self.bucket_bounds):                  # FlatArena.pack moves 16 bytes per lane from a bucket's first element on
            raise ValueError(f"gradient bucket offsets {self.bucket_bounds} must be multiples of 8 elements (a bucket starts inside an arena "
                             "group, whose members are stored without padding?)")
        self._reducer = None
        self._side = None
        self.overlap_wgrad = os.environ.get("MEDMOE_OVERLAP_WGRAD", "1") == "1"    # weight-gradient GEMMs on a second stream (backward)
        # MEDMOE_WGRAD_STAGED=1: plain wgrads without atomics on dW (medmoe_gemm_tn_staged: partial tiles + a summing kernel, deterministic).
        # Measured no faster than the atomic form (batch 128: 25.20-25.34 against 25.13-25.19 ms; batch 1024: 217.4 against 216.4): default off
        self.wgrad_staged = os.environ.get("MEDMOE_WGRAD_STAGED", "0") == "1"
        # MEDMOE_GRAPH=1: the two fixed launch sequences of a step - [zero the gradient, both towers' forward, MoE forward] and [the whole
        # backward] - are captured into hipGraphs (torch.cuda.CUDAGraph around the C-ABI launches, the second stream forked and joined inside
        # the capture) and replayed; the losses in between stay eager (the local loss builds its class tables on the host) and so does the
        # optimiser (its bias-correction scalars are host values).  Single rank, frozen text tower.
        self.use_graph = os.environ.get("MEDMOE_GRAPH", "0") == "1"
        self._graph = None

    @staticmethod
    def _refuse_with_graph(keys: str, hydra_keys: str):
        if os.environ.get("MEDMOE_GRAPH", "0") == "1":
            raise NotImplementedError(f"{keys} > 0 ({hydra_keys}) with MEDMOE_GRAPH=1: the dropout step counter is a by-value launch "
                                      "argument, a replayed graph would repeat one step's masks")

    @staticmethod
    def _refuse_mlm_with_graph():
        if os.environ.get("MEDMOE_GRAPH", "0") == "1":
            raise NotImplementedError("text_mlm (model.mlm) with MEDMOE_GRAPH=1: the mask's step counter is a by-value launch argument, a "
                                      "replayed graph would repeat one step's mask")

    def _make_mlm_head(self):
        self._refuse_mlm_with_graph()
        from .mlm import MLMHead
        self.mlm = MLMHead(self.cfg.d_t, self.cfg.vocab, self.device, self._seed)

    def enable_mlm(self, prob: float = 0.15, weight: float = 1.0, mask_id: int = 103):
        """Switch the masked-language-model objective on after construction (the Lightning module reads `model.mlm` when the engine already
        exists): the config keys, their refusals, the head and its arena, the parameter groups and - with cfg.ema_decay > 0 - its average."""
        c = self.cfg
        old = (c.text_mlm, c.mlm_prob, c.mlm_weight, c.mlm_mask_id)
        c.text_mlm, c.mlm_prob, c.mlm_weight, c.mlm_mask_id = True, float(prob), float(weight), int(mask_id)
        try:
            c.validate()
            if self.mlm is None:
                self._make_mlm_head()
        except Exception:
            c.text_mlm, c.mlm_prob, c.mlm_weight, c.mlm_mask_id = old
            raise
        self.apply_optimizer_groups()
        if c.ema_decay > 0.0:
            ema_.prepare(self.optimizer_stores().values())

    def optimizer_stores(self) -> Dict[str, object]:
        """kind (medmoe_amd.optim_groups) -> the arenas this engine steps."""
        out = {"vit": self.params}
        if self.text_arena() is not None:
            out["text"] = self.text_arena()
        if self.vlora is not None:
            out["vit_lora"] = self.vlora
        if self.mlm is not None:
            out["mlm"] = self.mlm.store
        return out

    def merged_image_params(self) -> Dict[str, torch.Tensor]:
        """The image tower + MoE under their reference-style names (ParamStore.export_named: fp32 CPU tensors) with the adapters merged
        into the fused projections: W_t <- bf16(W_t + s B_t A_t) (medmoe_lora_merge on a copy of the bf16 working weight).  For export, and
        for evaluation on a plain engine (`params.load_named`)."""
        if self.vlora is None:
            raise RuntimeError("merged_image_params: this engine has no adapters on the image tower (cfg.vit_lora)")
        lo, out = self.vlora, self.params.export_named()
        for l in range(self.cfg.n_layer_v):
            name = f"vit.layer.{l}.attention.input_proj.weight"
            w = ops.lora_merge(self.params.w16(name).clone(), lo.A16(l), lo.B16(l), lo.targets, lo.scale)
            out[name] = w.float().cpu()
        return out

    def _vit_lora_rng(self, l: int):
        """The generator of layer l's adapter dropout under the masks of the current training pass; None: the pass drops nothing."""
        if self._vit_lora_drop_step is None:
            return None
        return ops.dropout_rng(self.cfg.dropout_seed, self._vit_lora_drop_step, ops.DROPOUT_SITE_VIT_LORA + l, self.cfg.vit_lora_dropout)

    # The adapter weight-gradient launch keeps accumulating over `run` 256-row chunks per workgroup (medmoe_lora_bwd_wgrad_runs).  Measured
    # on one MI355X at D = 768, two targets (tools/bench_vit_lora.py --sweep, profiles/r19_notes.md): M = 201 728 (cfg2, batch 1024) run 1 /
    # 2 / 4 / 8 / 16 = 542 / 380 / 258 / 327 / 558 us, M = 25 216 (batch 128) 62 / 73 / 117 / 217 / 424 us - a workgroup's time grows with
    # its run, so a longer run pays only while the grid still holds about four workgroups per CU: the largest such run, else 1
    @staticmethod
    def vit_lora_wgrad_run(M: int, D: int) -> int:
        groups = ((M + 255) // 256, (D + 127) // 128)
        for run in (16, 8, 4, 2):
            if ((groups[0] + run - 1) // run) * groups[1] >= 4 * 256:
                return run
        return 1

    def text_arena(self):
        """The arena the text side trains: the whole tower's (freeze_text = False), the LoRA adapters' (text_lora), or None (frozen)."""
        return self.lora if self.lora is not None else self.tstore

    # -- LoRA: the frozen base's dgrad operands, the adapters' launches, the merged tower ----------------------------------------------------
    _BASE_GEMMS = ("attention.input_proj.weight", "attention.output_proj.weight", "feedforward.model.0.weight", "feedforward.model.2.weight")

    def refresh_text_base(self):
        """LoRA: the transposed bf16 copy ([in, out]) of the four GEMM weights of every layer of the frozen base - what the text backward's
        dgrad GEMMs read.  Made at construction and again after the base changed (a loaded checkpoint replaces the tensors of params.text:
        `_base_wt` notices); never per step, and the base has no fp32 master, gradient or Adam state."""
        for l in range(self.cfg.n_layer_t):
            for n in self._BASE_GEMMS:
                self._base_wt(f"layer.{l}.{n}")

    def _base_wt(self, name: str) -> torch.Tensor:
        w = self.params.text[name]
        hit = self._base_t.get(name)
        if hit is None or hit[0] is not w:
            hit = self._base_t[name] = (w, w.t().contiguous())
        return hit[1]

    def merged_text_params(self) -> Dict[str, torch.Tensor]:
        """The frozen-tower parameter dict (names and dtypes of params.text) with the adapters merged into the fused projections:
        W_t <- bf16(W_t + s B_t A_t) (medmoe_lora_merge on a copy).  For export, and for evaluation on a plain frozen engine."""
        if self.lora is None:
            raise RuntimeError("merged_text_params: this engine has no LoRA adapters (cfg.text_lora)")
        lo, out = self.lora, {k: v.clone() for k, v in self.params.text.items()}
        for l in range(self.cfg.n_layer_t):
            ops.lora_merge(out[f"layer.{l}.attention.input_proj.weight"], lo.A16(l), lo.B16(l), lo.targets, lo.scale)
        return out

    # -- weight EMA --------------------------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def ema_weights(self):
        """Context: the forward passes run on the AVERAGED weights (eval_step, forward_image, forward_text, merged_text_params).  On entry
        every arena this engine steps loads its average into the working copies (FlatArena.load_ema), on exit - also when the body raises -
        the master's come back.  No master, gradient or optimiser state is written; train_step / optimizer_step inside raise."""
        if not self.cfg.ema_decay > 0.0:
            raise RuntimeError("ema_weights: this engine keeps no average - cfg.ema_decay is 0 (model.ema.decay)")
        if self._ema_active:
            raise RuntimeError("ema_weights: already inside the context")
        arenas = list(self.optimizer_stores().values())
        ema_.prepare(arenas)
        self._ema_active = True
        try:
            for a in arenas:
                a.load_ema()
            self._repoint_text()
            yield self
        finally:
            for a in arenas:
                if a.ema_loaded:
                    a.restore_master()
            self._ema_active = False
            self._repoint_text()

    def _repoint_text(self):
        """The trainable text tower's name -> tensor dict holds fp32 VIEWS for embeddings, biases and LayerNorms: taken again whenever the
        store switches between the master and the average."""
        if self.tstore is not None:
            self.params.text = self.tstore.as_dict()

    def ema_params(self) -> Dict[str, torch.Tensor]:
        """Reference-style names -> the fp32 averages (CPU tensors), for export: the image tower and MoE under their own names, the trainable
        text tower's or the adapters' under `text.`.  A frozen base holds no average."""
        if not self.cfg.ema_decay > 0.0:
            raise RuntimeError("ema_params: this engine keeps no average - cfg.ema_decay is 0 (model.ema.decay)")
        arenas = list(self.optimizer_stores().values())
        ema_.prepare(arenas)
        out = {}
        for a in arenas:
            out.update(a.export_named(a.e32))
        return out

    def apply_optimizer_groups(self):
        """cfg.no_decay / no_decay_1d / text_lr_mult / layer_decay -> the run tables of the stores (uploaded here, once; the default rule
        set clears them and the step stays medmoe_adam_step)."""
        from .optim_groups import GroupRules, apply_rules
        apply_rules(self.optimizer_stores(), GroupRules.from_config(self.cfg))

    def set_optimizer_groups(self, **rules):
        """Change the rule set (any of no_decay, no_decay_1d, text_lr_mult, layer_decay) and regroup the stores."""
        from .optim_groups import set_rules
        set_rules(self.cfg, rules)
        self.apply_optimizer_groups()

    def grad_comm(self, arena):
        """The `comm` argument of the gradient all-reduces (medmoe_amd.dist) for `arena`: the arena itself when its gradient travels as bf16
        (cfg.grad_comm_dtype = "bf16" or MEDMOE_GRAD_COMM=bf16, and this engine takes the data-parallel steps), None for the fp32 exchange."""
        if self.cfg.grad_comm_dtype not in ("fp32", "bf16"):
            raise ValueError(f"grad_comm_dtype must be 'fp32' or 'bf16', got {self.cfg.grad_comm_dtype!r}")
        return arena if self.dist and (self._grad_comm_env or self.cfg.grad_comm_dtype == "bf16") else None

    def set_deterministic(self, flag: bool):
        """Switch deterministic mode on or off; refuses the combinations it is not built for.  The scratch buffers are allocated on first
        use, in deterministic mode only."""
        flag = bool(flag)
        if flag:
            if self.cfg.text_lora:
                raise NotImplementedError("deterministic with text_lora (text.lora: true): the trainable text path (the local loss' word "
                                          "gradients, the text backward) has no deterministic form yet - a named follow-up (DESIGN 3e)")
            if not self.cfg.freeze_text:
                raise NotImplementedError("deterministic with freeze_text=False (text.freeze_bert: false): the trainable text tower's embedding "
                                          "gradients meet in fp32 atomics and index_add_ - a named follow-up (DESIGN 3e)")
            if os.environ.get("MEDMOE_GRAPH", "0") == "1":
                raise NotImplementedError("deterministic with MEDMOE_GRAPH=1: the captured launch sequences are the default mode's - a named "
                                          "follow-up (DESIGN 3e)")
        self.deterministic = flag
        self._det = (self._det or ops.DetScratch(self.device)) if flag else None
        if getattr(self, "_local", None) is not None:
            self._local.det = self._det
        if getattr(self, "_gle", None) is not None:
            self._gle.det = self._det

    def _parts(self, n: int) -> torch.Tensor:
        """Deterministic mode: the loss heads' per-row terms (summed in row order by a second launch) - one fp32 buffer of the engine's.
        One buffer serves every head and router_bwd_det only because all of them launch on the main stream, where stream order keeps
        a head's summing launch ahead of the next head's stores; a launch on the second stream would need its own (as ops.DetScratch has)."""
        buf = self.ws.get("det_parts")
        if buf is None or buf.numel() < n:
            buf = self.ws["det_parts"] = torch.empty(max(n, 2 * self.B * self.world), device=self.device, dtype=F32)
        return buf

    # ------------------------------------------------------------------------------------------
    # workspace
    # ------------------------------------------------------------------------------------------
    def _alloc(self, B: int):
        if B == self.B:
            return
        c, dev = self.cfg, self.device
        self.B = B
        ws = self.ws = {}
        self._local = self._gle = None                       # sized for the old batch: released with the old workspace
        Nt, Dv, P, L = c.n_tok_v, c.d_v, c.n_patch, c.n_layer_v
        M = B * Nt
        H = c.n_head_v

        def buf(name, shape, dtype=BF):
            ws[name] = torch.empty(shape, device=dev, dtype=dtype)
        ws["im2col"] = torch.zeros((B * P, c.patch_dim_pad), device=dev, dtype=BF)    # pad columns (patch 14: 588..639) stay zero
        # the tower's activations: x{l}, per layer ln1 / st1 / qkv / att / lse / xmid / ln2 / st2 / z / h - or, under cfg.vit_checkpoint, the
        # kept ones and the two shared sets (vit_activation_plan; _act finds a layer's buffer)
        for name, (shape, dtype) in vit_activation_plan(c, B, self.vit_checkpoint).items():
            buf(name, shape, dtype)
        buf("lnf", (M, Dv)); buf("stf", (2, M), F32)
        # backward scratch
        buf("dxa", (M, Dv)); buf("dxb", (M, Dv)); buf("dln", (M, Dv)); buf("dqkv", (M, 3 * Dv)); buf("datt", (M, Dv))
        buf("dz", (M, c.ff_v)); buf("delta", (B * H * Nt,), F32)
        if self.vlora is not None:    # the adapters' U = dropout(ln1) A^T per layer (bf16, 16 per target: the backward reads it), one d U, the wgrad partials
            nt = len(self.vlora.targets)
            for l in range(L):
                buf(f"v_lu{l}", (M, nt * ops.LORA_RANK_PAD))
            self._vlora_run = self.vit_lora_wgrad_run(M, Dv)
            buf("v_ldu", (M, nt * ops.LORA_RANK_PAD)); buf("v_lsc", (ops.lora_wgrad_runs_scratch(M, Dv, nt, self._vlora_run),), F32)
        if c.vit_drop_path > 0.0:
            # the scales of a step; dp_a: a branch's GEMM output before its scale + residual + LayerNorm launch (forward), the scaled out-proj
            # gradient (backward); dp_b: the scaled FC2 gradient.  Two gradient copies: the side stream's FC2 wgrad may still read one while
            # the main stream writes the other
            buf("vit_dp", (L, 2, B), F32); buf("dp_a", (M, Dv)); buf("dp_b", (M, Dv))
        ws["rowmap_patch"] = (torch.arange(B * P, device=dev) // P * Nt + 1 + torch.arange(B * P, device=dev) % P).to(I32)
        # MoE
        E, k, Do, Dh = c.n_expert, c.top_k, c.d_out, c.d_out // 2
        R = B * k * P
        self.R = R
        self.max_tiles = (R + 127) // 128 + E
        buf("router_in", (B, Dv), F32); buf("router_h", (B, c.router_hidden), F32)
        buf("probs", (B, E), F32); buf("idx", (B, k), I32); buf("gates", (B, k), F32)
        buf("slot_of", (B * k,), I32); buf("item_of_slot", (B * k,), I32); buf("expert_of_slot", (B * k,), I32)
        buf("row_off", (E + 1,), I32); buf("tiles", (2 * self.max_tiles, 4), I32); buf("tile_count", (2,), I32)   # 128-row table, then 256-row table
        buf("rowmap", (R,), I32)
        buf("G", (4, R, Do)); buf("H1", (4, R, Dh)); buf("eout", (R, Do)); buf("wts", (R, 4), F32)
        buf("dG", (4, R, Do)); buf("dH1", (4, R, Dh)); buf("dF", (4, R, Dv))
        if c.expert_fp8:           # e4m3 activation rows + their scales (one set, reused by every fp8 GEMM of the step)
            buf("q8", (R, max(Dv, Do)), torch.uint8); buf("q8s", (R,), F32)
        if c.expert_mx:            # MXFP8 rows + their scale bytes: one set for the separately quantised operands (x{l} gathered, dH1, dG)
            buf("qmx", (R, max(Dv, Do)), torch.uint8); buf("qmxs", (R, max(Dv, Do) // 32), torch.uint8)    # and one the first projection's
            buf("qG", (R, Do), torch.uint8); buf("qGs", (R, Do // 32), torch.uint8)                        # epilogue writes for the second
        buf("img_l", (B, P, Do)); buf("img_g", (B, Do), F32)
        buf("d_img_g", (B, Do), F32); buf("d_img_l", (B, P, Do)); buf("dgate", (B * k,), F32)
        buf("dlogits", (B, E), F32); buf("drouter_h", (B, c.router_hidden), F32); buf("drouter_in", (B, Dv), F32)
        buf("ones", (B,), F32); ws["ones"].fill_(1.0)
        buf("loss_parts", (8,), F32)    # [0]=cls loss [1]=cls acc [2]=global loss [3]=local loss
        # text tower
        T, Dt = c.max_len, c.d_t
        Mt = B * T
        buf("tx0", (Mt, Dt)); buf("tx1", (Mt, Dt)); buf("tx2", (Mt, Dt)); buf("tr", (Mt, Dt)); buf("tqkv", (Mt, 3 * Dt)); buf("tatt", (Mt, Dt))
        buf("th", (Mt, c.ff_t)); buf("tlse", (B * c.n_head_t * T,), F32); buf("tstat", (2, Mt), F32)
        # text_pack: tok_row | src_of_row | seq_off | count, then (a trainable tower's packed pass) 0 | count - its count sits behind a zero that is
        # never written, so the pair is the row_off = [0, count] of the one-group weight-gradient GEMMs
        ws["tpack"] = torch.zeros(2 * Mt + B + 4, device=dev, dtype=I32)
        for j in range(min(c.last_n_layers, c.n_layer_t + 1)):
            buf(f"ths{j}", (Mt, Dt))
        buf("words", (B, T, Dt)); buf("words32", (B, T, Dt), F32); buf("txt_g", (B, Dt), F32)
        buf("seg", (B, T), I32); buf("cap", (B,), I32)
        if self.train_text:        # every layer's activations stay for the text backward (padded pass: B x T rows)
            Lt, Ht = c.n_layer_t, c.n_head_t
            for l in range(Lt + 1):
                buf(f"t_x{l}", (Mt, Dt))
            for l in range(Lt):
                buf(f"t_qkv{l}", (Mt, 3 * Dt)); buf(f"t_att{l}", (Mt, Dt)); buf(f"t_lse{l}", (B * Ht * T,), F32)
                buf(f"t_x1{l}", (Mt, Dt)); buf(f"t_st1{l}", (2, Mt), F32); buf(f"t_r{l}", (Mt, Dt))
                buf(f"t_h{l}", (Mt, c.ff_t)); buf(f"t_dg{l}", (Mt, c.ff_t)); buf(f"t_x2{l}", (Mt, Dt)); buf(f"t_st2{l}", (2, Mt), F32)
            buf("t_dH", (Mt, Dt)); buf("t_da", (Mt, Dt)); buf("t_db", (Mt, Dt)); buf("t_dc", (Mt, Dt)); buf("t_datt", (Mt, Dt))
            buf("t_dz", (Mt, c.ff_t)); buf("t_dqkv", (Mt, 3 * Dt)); buf("t_delta", (B * Ht * T,), F32)
            if self.lora is None:
                buf("t_dxemb", (Mt, Dt), F32)
            else:                  # the adapters' U = dropout(x) A^T per layer (bf16, 16 per target: the backward reads it), one d U, the wgrad partials
                nt = len(self.lora.targets)
                for l in range(Lt):
                    buf(f"t_lu{l}", (Mt, nt * ops.LORA_RANK_PAD))
                buf("t_ldu", (Mt, nt * ops.LORA_RANK_PAD)); buf("t_lsc", (ops.lora_wgrad_scratch(Mt, Dt, nt),), F32)
            buf("d_txt_g", (B, Dt), F32); buf("cb", (B * self.world,), F32)
            if c.text_hidden_dropout > 0.0:      # a GEMM output before its dropout + residual + LayerNorm launch; d z = keep * d x1 / (1 - p) in the backward
                buf("t_z", (Mt, Dt)); buf("t_dzd", (Mt, Dt))
            if self.dist:
                buf("d_txt_all", (B * self.world, Dt), F32); buf("cb1", (B * self.world,), F32)
        # global loss
        Bg = B * self.world
        buf("na", (B,), F32); buf("nb", (Bg,), F32); buf("S", (B, Bg), F32); buf("dS", (B, Bg), F32)
        buf("ca", (B,), F32)
        if self.dist:
            buf("nb2", (Bg,), F32); buf("na2", (B,), F32); buf("S2", (B, Bg), F32); buf("dS2", (B, Bg), F32)
            buf("cb2", (Bg,), F32); buf("ca2", (B,), F32); buf("d_img_all", (Bg, Do), F32)
        # local loss: the similarity matrix and the heads' d loss / d sim; every other buffer belongs to the local-loss object
        buf("sim", (B, B), F32); buf("gsim", (B, B), F32)

    # ------------------------------------------------------------------------------------------
    # image tower forward (ViT blocks = transformer.py:98-114 pre-norm; embeddings build-defined)
    # ------------------------------------------------------------------------------------------
    def _expert_tiles(self, K: int) -> dict:
        """Tile-table arguments of a grouped expert GEMM with reduction length K: the 256x256 kernel and the 256-row
        table medmoe_dispatch writes behind the 128-row one, or (K < 128) the 128x128 kernel."""
        ws, R, E = self.ws, self.R, self.cfg.n_expert
        if K >= 128:
            return dict(tiles=ws["tiles"][self.max_tiles:], tile_count=ws["tile_count"][1:], max_tiles=(R + 255) // 256 + E, M=R, tile_rows=256)
        return dict(tiles=ws["tiles"], tile_count=ws["tile_count"], max_tiles=self.max_tiles, M=R)

    def _fp8_gemm(self, x, K, rowmap, colscale, wq, wscale, bias, out, N, K_, epi, residual=None, aux=None):
        """out[r, :N] = epi(fp8 product of the rows of x (gathered through rowmap; times the per-expert column scale when the
        weight scales were folded into the rows, i.e. dgrad) with the expert's e4m3 weight [N, K]) over the dispatch's 128-row tiles."""
        ws, P = self.ws, self.cfg.n_patch
        q, qs = ws["q8"].view(-1)[:self.R * K].view(self.R, K), ws["q8s"]
        ops.call("quant_rows_e4m3", x, x.stride(-2), rowmap, colscale, ws["expert_of_slot"] if colscale is not None else None, P, q, qs, self.R, K)
        ops.call("gemm_fp8_grouped", q, qs, wq, wscale, bias, out, out.stride(-2), residual, aux, ws["tiles"], ws["tile_count"], self.max_tiles,
                 N, K_, N * K_, N if wscale is not None else 0, N if bias is not None else 0, epi)

    def _mx_gemm(self, x, K, rowmap, w, bias, out, N, epi, residual=None, aux=None, qout=None):
        """out[r, :N] = epi(MXFP8 product of the rows of x with the expert's weight copy w = (e4m3 [E, N, K], scale bytes [E, N, K/32]))
        over the dispatch's 128-row tiles on the block-scaled MFMA.  x: bf16 rows (gathered through rowmap), quantised here in blocks of
        32 along K, or an already quantised (e4m3 [R, K], scale bytes [R, K/32]) pair.  qout = (e4m3 [R, N], scale bytes [R, N/32]): the
        ReLU epilogue also writes its result MX-quantised along N (the next product's A operand, no separate pass over it)."""
        ws, R = self.ws, self.R
        if isinstance(x, tuple):
            q, qs = x
        else:
            q, qs = ws["qmx"].view(-1)[:R * K].view(R, K), ws["qmxs"].view(-1)[:R * (K // 32)].view(R, K // 32)
            ops.call("quant_rows_mx", x, x.stride(-2), rowmap, q, qs, R, K)
        wq, wsc = w
        ops.call("gemm_mx_grouped", q, qs, wq, wsc, bias, out, out.stride(-2), residual, aux, qout[0] if qout else None, qout[1] if qout else None,
                 ws["tiles"], ws["tile_count"], self.max_tiles, N, K, N * K, N * (K // 32), N if bias is not None else 0, epi)

    def forward_image(self, images: torch.Tensor):
        B = images.shape[0]
        self._alloc(B)
        c, p, ws = self.cfg, self.params, self.ws
        Nt, Dv, P, H = c.n_tok_v, c.d_v, c.n_patch, c.n_head_v
        M = B * Nt
        if images.dtype not in (F32, BF) or tuple(images.shape[1:]) != (3, c.img_size, c.img_size) or not images.is_contiguous():
            raise ValueError("images must be contiguous [B,3,H,W] fp32/bf16")
        ops.call("patchify_ld", images, ws["im2col"], B, 3, c.img_size, c.img_size, c.patch, 1 if images.dtype == F32 else 0,
                 c.patch_dim_pad)        # pad columns were zeroed at allocation and are never written
        x = ws["x0"]
        ops.call("init_tokens", x, p.f32("vit.cls_token"), p.f32("vit.pos_embed"), B, Nt, Dv)
        ops.gemm_nt(ws["im2col"], p.w16("vit.patch_embed.weight"), x, bias=p.f32("vit.patch_embed.bias"), residual=x,
                    c_rowmap=ws["rowmap_patch"], M=B * P)
        self._vit_blocks(B)
        ops.call("mean_tokens", ws["lnf"], ws["router_in"], B, Nt, Dv, 1, P)          # swin.py:137
        self._moe_forward(B)

    def _act(self, l: int, name: str) -> torch.Tensor:
        """Layer l's activation `name` (x | ln1 | qkv | att | xmid | ln2 | z | h): the layer's own buffer, or - when cfg.vit_checkpoint does
        not keep it - the one of the shared set the layer's parity selects.  "none" keeps everything: ws["ln1_{l}"] and so on."""
        if name in self._ck_shared:
            return self.ws[f"ck{l & 1}_{name}"]
        return self.ws[_VIT_ACT[name].format(l)]

    def _vit_blocks(self, B):
        """The pre-norm blocks (transformer.py:98-114) from ws["x0"] to ws["x{L}"] and the final LayerNorm (-> ws["lnf"]); every
        intermediate the backward needs stays in the workspace (cfg.vit_checkpoint: the kept ones; the rest passes through the shared sets
        and is recomputed by _vit_backward).  tests/test_ref_fixtures_gpu.py feeds the reference's own TransformerEncoder fixture in here."""
        c, p, ws = self.cfg, self.params, self.ws
        L = c.n_layer_v
        dp = self._vit_drop_layers()
        ln_done = False                                      # the previous layer's feed-forward site already wrote this LayerNorm
        for l in range(L):
            ln_done = self._vit_layer_forward(l, dp[l], ln_done)
        if not ln_done:
            xl = ws[f"x{L}"]
            ops.layernorm_fwd(xl, p.f32("vit.final_layer_norm.weight"), p.f32("vit.final_layer_norm.bias"), ws["lnf"],
                              ws["stf"][0], ws["stf"][1], c.eps_v)

    def _vit_layer_forward(self, l: int, dp_l, ln_done: bool = False, recompute: bool = False) -> bool:
        """Layer l's forward launches from ws["x{l}"]; dp_l: the layer's stochastic-depth scales or None (_vit_drop_layers).
        The forward pass (recompute=False) runs them all, to ws["x{l + 1}"]; ln_done: the previous layer's feed-forward site already wrote
        this layer's first LayerNorm.  Returns whether this layer's feed-forward site wrote the NEXT LayerNorm.
        recompute (cfg.vit_checkpoint, ahead of the layer's backward): the launches up to FC1 again, into the layer's shared set.  Both
        LayerNorm outputs come from the kept input and the kept statistics (layernorm_apply: the bits of the forward's); "selective" kept
        qkv / att / xmid and skips the attention half, "full" runs it again from x{l} - the same launches on the same inputs, so the same
        bits (the stochastic-depth site under the step's scales; it rewrites st2 and attn_fwd rewrites lse with the values they hold).
        FC2 and the next layer's LayerNorm are not run again: x{l + 1} is kept and the backward reads nothing else of theirs."""
        c, p, ws = self.cfg, self.params, self.ws
        B, Nt, H, L = self.B, c.n_tok_v, c.n_head_v, c.n_layer_v
        pre = f"vit.layer.{l}."
        act = lambda name: self._act(l, name)
        x, xo = ws[f"x{l}"], ws[f"x{l + 1}"]
        st1, st2 = ws[f"st1_{l}"], ws[f"st2_{l}"]
        ln2_w, ln2_b = p.f32(pre + "feedforward_layernorm.weight"), p.f32(pre + "feedforward_layernorm.bias")
        if recompute:
            ops.layernorm_apply(x, st1[0], st1[1], p.f32(pre + "attention_layernorm.weight"), p.f32(pre + "attention_layernorm.bias"), act("ln1"))
        elif not ln_done:
            ops.layernorm_fwd(x, p.f32(pre + "attention_layernorm.weight"), p.f32(pre + "attention_layernorm.bias"),
                              act("ln1"), st1[0], st1[1], c.eps_v)
        ln2_done = False
        if not recompute or self.vit_checkpoint == "full":
            ops.gemm_nt(act("ln1"), p.w16(pre + "attention.input_proj.weight"), act("qkv"),
                        bias=p.f32(pre + "attention.input_proj.bias"))
            if self.vlora is not None:   # qkv[:, target columns] += s (dropout(ln1) A^T) B^T, U kept for the backward: one launch.  A "full"
                lo = self.vlora          # recomputation runs it again under the same mask: the same bits
                ops.lora_fwd(act("ln1"), lo.A16(l), lo.B16(l), ws[f"v_lu{l}"], act("qkv"), lo.targets, lo.scale, self._vit_lora_rng(l))
            ops.attn_fwd(act("qkv"), act("att"), ws[f"lse{l}"], None, B, Nt, H)
            if dp_l is None:
                ops.gemm_nt(act("att"), p.w16(pre + "attention.output_proj.weight"), act("xmid"),
                            bias=p.f32(pre + "attention.output_proj.bias"), residual=x)
            else:
                # stochastic depth: the GEMM leaves the branch in dp_a; the per-sample scale, the residual add and the LayerNorm
                # that follows it are one launch
                ops.gemm_nt(act("att"), p.w16(pre + "attention.output_proj.weight"), ws["dp_a"], bias=p.f32(pre + "attention.output_proj.bias"))
                ops.scale_add_layernorm_fwd(ws["dp_a"], x, dp_l[0], Nt, ln2_w, ln2_b, act("xmid"), act("ln2"), st2[0], st2[1], c.eps_v)
                ln2_done = True
        if not ln2_done:
            if recompute:
                ops.layernorm_apply(act("xmid"), st2[0], st2[1], ln2_w, ln2_b, act("ln2"))
            else:
                ops.layernorm_fwd(act("xmid"), ln2_w, ln2_b, act("ln2"), st2[0], st2[1], c.eps_v)
        ops.gemm_nt(act("ln2"), p.w16(pre + "feedforward.model.0.weight"), act("h"),
                    bias=p.f32(pre + "feedforward.model.0.bias"), aux=act("z"), epi=ops.EPI_GELU_DAUX)    # aux <- GELU'(z): the backward epilogue is one multiply
        if recompute:
            return False
        if dp_l is None:
            ops.gemm_nt(act("h"), p.w16(pre + "feedforward.model.2.weight"), xo,
                        bias=p.f32(pre + "feedforward.model.2.bias"), residual=act("xmid"))
            return False
        # the feed-forward site writes the NEXT LayerNorm with it: ln1 of layer l + 1, or the final one
        ops.gemm_nt(act("h"), p.w16(pre + "feedforward.model.2.weight"), ws["dp_a"], bias=p.f32(pre + "feedforward.model.2.bias"))
        nxt = f"vit.layer.{l + 1}.attention_layernorm." if l + 1 < L else "vit.final_layer_norm."
        y, st = (self._act(l + 1, "ln1"), ws[f"st1_{l + 1}"]) if l + 1 < L else (ws["lnf"], ws["stf"])
        ops.scale_add_layernorm_fwd(ws["dp_a"], act("xmid"), dp_l[1], Nt, p.f32(nxt + "weight"), p.f32(nxt + "bias"), xo, y,
                                    st[0], st[1], c.eps_v)
        return True

    def _vit_drop_layers(self):
        """Per layer: None (today's launches) or the layer's [2, B] scales - the layers with p_l > 0 while self.vit_drop_scales is set."""
        L = self.cfg.n_layer_v
        sc = self.vit_drop_scales
        if sc is None:
            return [None] * L
        if "dp_a" not in self.ws:
            raise RuntimeError("vit_drop_scales is set on an engine built with vit_drop_path = 0: it has no buffers for the scaled launches")
        if sc.dtype != F32 or tuple(sc.shape) != (L, 2, self.B) or not sc.is_contiguous():
            raise ValueError(f"vit_drop_scales must be a contiguous fp32 [{L}, 2, {self.B}] tensor, got {sc.dtype} {tuple(sc.shape)}")
        return [sc[l] if pl > 0.0 else None for l, pl in enumerate(self.cfg.vit_drop_path_rates())]

    def _moe_forward(self, B):
        c, p, ws = self.cfg, self.params, self.ws
        E, k, Do, Dh, Dv, P, Nt = c.n_expert, c.top_k, c.d_out, c.d_out // 2, c.d_v, c.n_patch, c.n_tok_v
        R = self.R
        ops.call("router_fwd", ws["router_in"], p.f32("moe.router.0.weight"), p.f32("moe.router.0.bias"),
                 p.f32("moe.router.2.weight"), p.f32("moe.router.2.bias"), ws["router_h"], ws["probs"], ws["idx"],
                 ws["gates"], B, Dv, c.router_hidden, E, k)
        ops.call("dispatch", ws["idx"], B, k, E, P, Nt, ws["slot_of"], ws["item_of_slot"], ws["expert_of_slot"],
                 ws["row_off"], ws["tiles"], ws["tile_count"], self.max_tiles, ws["rowmap"])
        grp = self._expert_tiles
        for s, l in enumerate(c.stage_layers()):
            if c.expert_fp8:
                # e4m3 weights (per-output-channel scales) x e4m3 activation rows (one dynamic scale per row) on the fp8 MFMA
                self._fp8_gemm(ws[f"x{l}"], Dv, ws["rowmap"], None, p.q8(f"moe.proj.{s}.weight"), p.s8(f"moe.proj.{s}.weight"),
                               p.f32(f"moe.proj.{s}.bias"), ws["G"][s], Do, Dv, 1)
                self._fp8_gemm(ws["G"][s], Do, None, None, p.q8("moe.attn0.weight"), p.s8("moe.attn0.weight"), p.f32("moe.attn0.bias"),
                               ws["H1"][s], Dh, Do, 1)
                continue
            if c.expert_mx:
                # MXFP8 weights x MXFP8 activation rows (one power-of-two scale per 32 along the contraction) on the block-scaled MFMA;
                # the first product's epilogue hands G to the second already quantised
                qG = (ws["qG"], ws["qGs"])
                self._mx_gemm(ws[f"x{l}"], Dv, ws["rowmap"], p.qmx(f"moe.proj.{s}.weight"), p.f32(f"moe.proj.{s}.bias"), ws["G"][s], Do, 1, qout=qG)
                self._mx_gemm(qG, Do, None, p.qmx("moe.attn0.weight"), p.f32("moe.attn0.bias"), ws["H1"][s], Dh, 1)
                continue
            ops.gemm_nt(ws[f"x{l}"], p.w16(f"moe.proj.{s}.weight"), ws["G"][s], bias=p.f32(f"moe.proj.{s}.bias"),
                        a_rowmap=ws["rowmap"], stride_b=Do * Dv, stride_bias=Do, epi=ops.EPI_RELU, **grp(Dv))   # swin.py:40-41
            ops.gemm_nt(ws["G"][s], p.w16("moe.attn0.weight"), ws["H1"][s], bias=p.f32("moe.attn0.bias"),
                        stride_b=Dh * Do, stride_bias=Dh, epi=ops.EPI_RELU, **grp(Do))                      # swin.py:25-27
        ops.call("scale_attn_fwd", ws["G"], ws["H1"], p.f32("moe.attn2.weight"), p.f32("moe.attn2.bias"),
                 ws["expert_of_slot"], P, ws["eout"], ws["wts"], R, Do, Dh)
        ops.call("combine_fwd", ws["eout"], ws["slot_of"], ws["gates"], ws["img_l"], B, k, P, Do)
        ops.call("mean_tokens", ws["img_l"], ws["img_g"], B, P, Do, 0, P)              # swin.py:112

    # ------------------------------------------------------------------------------------------
    # text tower (transformer.py:116-130 post-norm; text_encoder.py:92-144): ONE block loop per direction for every mode - frozen or trainable,
    # padded or packed, with or without the dropouts and the LoRA adapters.  What a mode changes is data: the buffers (_TextBufs), the row
    # layout and the dropout generators (_TextRows), the gradient targets and the adapters
    # ------------------------------------------------------------------------------------------
    def forward_text(self, ids: torch.Tensor, attn_mask: torch.Tensor, token_type: Optional[torch.Tensor] = None,
                     embedded: Optional[torch.Tensor] = None, training: bool = False):
        """The frozen tower's pass: activations in the rotating scratch, nothing kept for a backward.  A trainable tower takes
        `_forward_text_train` instead, unless `embedded` is given.
        `training`: the pass of a training step - a trainable tower then applies its dropout (cfg.text_hidden_dropout / text_attn_dropout) with
        the masks of self.dropout_step; evaluation passes never do.
        `embedded` [B, T, d_t] bf16: use these rows as the encoder's input instead of the embedding front-end's output (the
        reference's TransformerEncoder fixture is fed to the post-norm blocks this way, tests/test_ref_fixtures_gpu.py)."""
        c, ws = self.cfg, self.ws
        B, T = ids.shape
        if B != self.B or T != c.max_len:
            raise ValueError("forward_text: call forward_image first with the same batch; T must equal cfg.max_len")
        if c.last_n_layers < 1 or c.last_n_layers > 4:
            raise ValueError("last_n_layers must be in 1..4")
        ids32 = ids.to(I32).contiguous()
        tt32 = token_type.to(I32).contiguous() if token_type is not None else None
        km = attn_mask.to(torch.uint8).contiguous()
        if self.train_text and embedded is None:
            return self._forward_text_train(ids, ids32, tt32, km, training)
        # VARIABLE LENGTH: the tower runs on the tokens with attention mask 1 only (55 % of the B x T positions for captions of 8..77 words),
        # packed in (caption, position) order by a device-side scan - GEMM / LayerNorm row counts and the attention's sequence offsets stay
        # on the device, nothing is copied to the host.  Padding tokens never reach a result: they are masked keys and carry no word
        # (text_encoder.py:32-90).  MEDMOE_TEXT_VARLEN=0 computes all B x T positions as the reference does.
        rows = _TextRows(self, km, self.text_varlen, trainable=False)
        # hidden_states = [embedding output, layer 1 .. layer L]; the reference sums hidden_states[-last:]
        # (text_encoder.py:97-103), which includes the embedding output when last > L
        first_sel = max(0, c.n_layer_t + 1 - c.last_n_layers)
        x = ws["ths0"] if first_sel == 0 else ws["tx0"]
        self._text_embed(rows, ids32, tt32, x)
        if embedded is not None:           # packed: the rows of the given input in packed order (rows past the count are never read)
            e = embedded.reshape(B * T, c.d_t).to(BF)
            x[:B * T].copy_(e.index_select(0, rows.src_row.long()) if rows.packed else e)

        def bufs(l, x):            # a summed state goes to its own buffer, any other layer's output ping-pongs between tx0 and tx2
            j = l + 1 - first_sel
            out = ws[f"ths{j}"] if j >= 0 else (ws["tx2"] if x is ws["tx0"] else ws["tx0"])
            return _TextBufs(ws["tqkv"], ws["tatt"], ws["tlse"], ws["tx1"], ws["tstat"], ws["tr"], ws["th"], None, ws["tx1"], ws["tstat"], out, None)
        self._text_tail(rows, ids, self._text_blocks(rows, x, bufs))

    def _forward_text_train(self, ids, ids32, tt32, km, training: bool = False):
        """The text pass of a TRAINABLE tower (cfg.freeze_text = False, or LoRA adapters on a frozen base): all B x T positions (key-masked
        attention, as the reference computes them, text_encoder.py:92-117) or, with text_train_varlen, the packed non-padding tokens (the
        first `count` rows of the same buffers); every layer's activations are kept in the workspace, and the pass' _TextRows in self._tp,
        for `backward_text`.
        `training` with a dropout probability > 0: BertModel's four train-mode dropouts - after the embedding LayerNorm, on the attention
        probabilities (medmoe_attn_drop_fwd), after the output projection and after FC2 (each fused with the residual add and the LayerNorm
        that follow: medmoe_dropout_add_layernorm_fwd on the GEMM's output without residual).  No mask is stored: `backward_text`
        regenerates them from (cfg.dropout_seed, the step, the site)."""
        c, ws, lo = self.cfg, self.ws, self.lora
        rows = _TextRows(self, km, self.text_train_varlen, trainable=True)
        rows.mlm = None
        if self._mlm_pass is not None:
            # the tower runs on the MASKED ids (the embedding forward and _text_embed_backward both read rows.ids32); the segment map was
            # built from the original ids (prefetch_cap_lens): a [MASK] or random id does not change which pieces form a word
            rows.mlm = ops.mlm_mask(ids32, km, cls_id=self.vocab.cls_id, sep_id=self.vocab.sep_id, pad_id=self.vocab.pad_id, mask_id=c.mlm_mask_id,
                                    vocab=c.vocab, seed=c.dropout_seed, step=self._mlm_pass[0], p=c.mlm_prob, sample_offset=self.rank * self.B,
                                    tok_row=rows.tok_row, out=self._mlm_out(ids32))
            ids32 = rows.mlm[0]
        rows.ids32, rows.tt32 = ids32, tt32
        rows.drop_step = self.dropout_step if training and self.text_dropout else None
        rows.lora_drop_step = self.dropout_step if training and lo is not None and c.text_lora_dropout > 0.0 else None
        self.text_train_varlen_active = rows.packed
        x = ws["t_x0"]
        self._text_embed(rows, ids32, tt32, x)
        rng = rows.rng(ops.DROPOUT_SITE_EMBED, c.text_hidden_dropout)
        if rng is not None:
            ops.dropout_apply(x, x, rng)

        def bufs(l, x):
            return _TextBufs(ws[f"t_qkv{l}"], ws[f"t_att{l}"], ws[f"t_lse{l}"], ws[f"t_x1{l}"], ws[f"t_st1{l}"], ws[f"t_r{l}"], ws[f"t_h{l}"],
                             ws[f"t_dg{l}"], ws[f"t_x2{l}"], ws[f"t_st2{l}"], ws[f"t_x{l + 1}"], ws[f"t_lu{l}"] if lo is not None else None)
        self._tp = rows
        self._text_tail(rows, ids, self._text_blocks(rows, x, bufs))
        if rows.mlm is not None:
            _, _, sel_rows, sel_labels, count = rows.mlm
            self.mlm.forward(rows.last.view(-1, c.d_t), sel_rows, sel_labels, count, self.tstore.w16("word_embeddings"), self._mlm_pass[1])

    def _mlm_out(self, ids32):
        """The mask launch's five outputs (ids_masked, labels, rows, row_labels, count), kept per batch shape."""
        key = tuple(ids32.shape)
        hit = self._mlm_bufs.get(key)
        if hit is None:
            n, dev = ids32.numel(), self.device
            hit = self._mlm_bufs[key] = (torch.empty_like(ids32), torch.empty_like(ids32), torch.empty(n, device=dev, dtype=I32),
                                         torch.empty(n, device=dev, dtype=I32), torch.zeros(1, device=dev, dtype=I32))
        return hit

    def _text_embed(self, rows, ids32, tt32, x):
        """x = LayerNorm(word + position + token-type embeddings), on all B x T rows or packed."""
        c, t = self.cfg, self.params.text
        a = (ids32, tt32, t["word_embeddings"], t["position_embeddings"], t["token_type_embeddings"], t["emb_layernorm.weight"],
             t["emb_layernorm.bias"], x, rows.B, rows.T, c.d_t, c.vocab, c.eps_t)
        if rows.packed:
            ops.call("text_embed_ln_packed", *a, rows.src_row, rows.cnt)
        else:
            ops.call("text_embed_ln", *a)

    def _text_blocks(self, rows, x, bufs):
        """THE forward loop over the L post-norm blocks, for every pass.  `rows`: the pass' layout and dropout steps; `bufs(l, x)`: the
        _TextBufs of layer l, whose input is x.  Returns hidden_states = [x, layer 1's output, ..., layer L's]."""
        c, t, lo = self.cfg, self.params.text, self.lora
        ph, pa = c.text_hidden_dropout, c.text_attn_dropout
        hidden = [x]
        for l in range(c.n_layer_t):
            b, k = f"layer.{l}.", bufs(l, x)
            rows.gemm(x, t[b + "attention.input_proj.weight"], k.qkv, bias=t[b + "attention.input_proj.bias"])
            if k.lu is not None:   # qkv[:, target columns] += s (dropout(x) A^T) B^T, U kept for the backward: one launch
                ops.lora_fwd(x, lo.A16(l), lo.B16(l), k.lu, k.qkv, lo.targets, lo.scale, rows.lora_rng(l), rows_dev=rows.cnt)
            rows.attn(k.qkv, k.att, k.lse, rows.rng(4 * l, pa))
            self._text_res_ln(rows, k.att, b + "attention.output_proj", x, b + "attention_layernorm", k.x1, k.st1, k.r, rows.rng(4 * l + 1, ph))
            rows.gemm(k.r, t[b + "feedforward.model.0.weight"], k.h, bias=t[b + "feedforward.model.0.bias"], aux=k.aux,
                      epi=ops.EPI_GELU if k.aux is None else ops.EPI_GELU_DAUX)
            self._text_res_ln(rows, k.h, b + "feedforward.model.2", k.r, b + "feedforward_layernorm", k.x2, k.st2, k.out, rows.rng(4 * l + 2, ph))
            x = k.out
            hidden.append(x)
        return hidden

    def _text_res_ln(self, rows, a, linear, res, norm, x1, st, y, rng):
        """A residual + LayerNorm site (two per block): x1 = res + a W^T + b of Linear `linear`, y = LayerNorm `norm`(x1).  With a hidden
        dropout generator: the GEMM's output without residual goes to t_z, and ONE launch drops, adds and normalises."""
        t = self.params.text
        w, bias, gamma, beta = t[linear + ".weight"], t[linear + ".bias"], t[norm + ".weight"], t[norm + ".bias"]
        if rng is None:
            rows.gemm(a, w, x1, bias=bias, residual=res)
            rows.ln(x1, gamma, beta, y, st)
        else:
            rows.gemm(a, w, self.ws["t_z"], bias=bias)
            ops.dropout_add_layernorm_fwd(self.ws["t_z"], res, gamma, beta, x1, y, st[0], st[1], self.cfg.eps_t, rng)

    def _text_tail(self, rows, ids, hidden):
        """The end of every text pass: hidden_states[-last_n_layers:] summed and aggregated to words (text_encoder.py:97-144) under the
        prefetched segment map, which the pass consumes; `rows` keeps what text_soft_target and backward_text read."""
        c, ws = self.cfg, self.ws
        rows.first_sel = max(0, c.n_layer_t + 1 - c.last_n_layers)
        hs = hidden[rows.first_sel:]
        rows.last = hs[-1]
        self._rows = rows
        if self._seg is None:
            self.prefetch_cap_lens(ids)
        rows.seg, self._seg = self._seg, None
        h = hs + [None] * (4 - len(hs))
        out = (ws["words"], ws["words32"], ws["txt_g"], rows.B, rows.T, c.d_t)
        if rows.packed:
            ops.call("text_aggregate_packed", h[0], h[1], h[2], h[3], len(hs), rows.seg, rows.tok_row, *out)
        else:
            ops.call("text_aggregate", h[0], h[1], h[2], h[3], len(hs), rows.seg, *out)

    def backward_text(self, d_words: Optional[torch.Tensor], d_txt_g: Optional[torch.Tensor]):
        """Back-propagate d loss / d word embeddings (fp32 [B, T, D]) and d loss / d sentence embeddings (fp32 [B, D]) through the aggregation,
        the post-norm blocks (transformer.py:116-130) and the embedding front-end, under the layout and the masks of the last trainable pass
        (self._tp).  THE backward loop over the blocks, for both trainable modes:
        full tower: every parameter's gradient into the text store's flat gradient buffer - each weight-gradient GEMM ahead of the dgrad GEMM
        of the same operand, the dgrad GEMMs on the store's transposed copies, the embedding backward at the end.
        LoRA adapters on a frozen base: the same chain of dgrad GEMMs (on the base's transposed copies, `_base_wt`), LayerNorm and attention
        backwards WITHOUT any base parameter gradient - the gradient targets are None, which skips the weight-gradient GEMMs and the
        LayerNorm gamma / beta sums - and no embedding backward.  Per layer, after the attention backward has written d qkv:
        medmoe_lora_bwd_dx (d U, and the adapters' term of d x added into the base dgrad GEMM's output) and medmoe_lora_bwd_wgrad (the
        adapters' gradients, += into the arena).  At layer 0 nothing below trains: the dgrad GEMM and the d x term are both skipped.
        LayerNorm gammas come from params.text in both modes: a trainable tower's entries ARE the store's fp32 views (TextStore.as_dict)."""
        c, ws, ts, lo, t, tp = self.cfg, self.ws, self.tstore, self.lora, self.params.text, self._tp
        B, T, Dt = self.B, c.max_len, c.d_t
        grad = ts.grad if lo is None else (lambda name: None)
        wt = ts.w16t if lo is None else self._base_wt
        dH = ws["t_dH"]
        # the masks of the forward pass just run (tp.rng gives None where it applied none): d z = keep * d x1 / (1 - p) feeds the two GEMMs of
        # a hidden site, the residual branch takes d x1 unchanged
        ph, pa = c.text_hidden_dropout, c.text_attn_dropout
        if tp.packed:
            ops.call("text_aggregate_bwd_packed", d_words, d_txt_g, tp.seg, tp.src_row, tp.cnt, dH, B, T, Dt)
        else:
            ops.call("text_aggregate_bwd", d_words, d_txt_g, tp.seg, dH, B, T, Dt)
        dy, d1, d2 = ws["t_da"], ws["t_db"], ws["t_dc"]
        dy.copy_(dH)                                                 # the last layer's output is always among the summed states
        if getattr(tp, "mlm", None) is not None:                     # + the MLM head's d hidden at the selected rows; the tied table's and the head's gradients
            self.mlm.backward(ts.grad("word_embeddings"), dy)
        for l in range(c.n_layer_t - 1, -1, -1):
            b = f"layer.{l}."
            st1, st2 = ws[f"t_st1{l}"], ws[f"t_st2{l}"]
            below = lo is None or l > 0                              # something that trains reads this layer's input
            # y = LN2(x2), x2 = r + FC2(GELU(FC1(r)))
            tp.ln_bwd(dy, ws[f"t_x2{l}"], st2[0], st2[1], t[b + "feedforward_layernorm.weight"], d1,
                      grad(b + "feedforward_layernorm.weight"), grad(b + "feedforward_layernorm.bias"))
            rng = tp.rng(4 * l + 2, ph)
            dz = ops.dropout_apply(d1, ws["t_dzd"], rng) if rng is not None else d1
            tp.wgrad(dz, ws[f"t_h{l}"], grad(b + "feedforward.model.2.weight"), db=grad(b + "feedforward.model.2.bias"))
            tp.gemm(dz, wt(b + "feedforward.model.2.weight"), ws["t_dz"], aux=ws[f"t_dg{l}"], epi=ops.EPI_MUL_AUX)
            tp.wgrad(ws["t_dz"], ws[f"t_r{l}"], grad(b + "feedforward.model.0.weight"), db=grad(b + "feedforward.model.0.bias"))
            tp.gemm(ws["t_dz"], wt(b + "feedforward.model.0.weight"), d2, residual=d1)                    # d r = d x2 + dz W1
            # r = LN1(x1), x1 = x + out_proj(attention(qkv(x)))
            tp.ln_bwd(d2, ws[f"t_x1{l}"], st1[0], st1[1], t[b + "attention_layernorm.weight"], d1,
                      grad(b + "attention_layernorm.weight"), grad(b + "attention_layernorm.bias"))
            rng = tp.rng(4 * l + 1, ph)
            dz = ops.dropout_apply(d1, ws["t_dzd"], rng) if rng is not None else d1
            tp.wgrad(dz, ws[f"t_att{l}"], grad(b + "attention.output_proj.weight"), db=grad(b + "attention.output_proj.bias"))
            tp.gemm(dz, wt(b + "attention.output_proj.weight"), ws["t_datt"])
            tp.attn_bwd(ws[f"t_qkv{l}"], ws[f"t_att{l}"], ws["t_datt"], ws[f"t_lse{l}"], ws["t_dqkv"], ws["t_delta"], tp.rng(4 * l, pa))
            tp.wgrad(ws["t_dqkv"], ws[f"t_x{l}"], grad(b + "attention.input_proj.weight"), db=grad(b + "attention.input_proj.bias"))
            if below:
                tp.gemm(ws["t_dqkv"], wt(b + "attention.input_proj.weight"), dy, residual=d1)             # d x = d x1 + dqkv Wqkv
            if lo is not None:
                rng = tp.lora_rng(l)
                ops.lora_bwd_dx(ws["t_dqkv"], lo.B16t(l), lo.A16t(l), ws["t_ldu"], dy if below else None, lo.targets, lo.scale, rng, rows_dev=tp.cnt)
                ops.lora_bwd_wgrad(ws["t_dqkv"], ws[f"t_x{l}"], ws[f"t_lu{l}"], ws["t_ldu"], lo.gA(l), lo.gB(l), ws["t_lsc"], lo.targets, lo.scale, rng,
                                   rows_dev=tp.cnt)
            if below and l >= tp.first_sel:                          # hidden_states[l] is one of the summed states too
                dy.add_(dH)
        if lo is None:
            self._text_embed_backward(tp, dy)

    def _text_embed_backward(self, tp, dy):
        """d hidden_states[0] -> the gradients of the embedding LayerNorm and the three embedding tables (full tower only)."""
        c, ws = self.cfg, self.ws
        B, T, Dt = self.B, c.max_len, c.d_t
        f32, grad = self.tstore.f32, self.tstore.grad
        rng = tp.rng(ops.DROPOUT_SITE_EMBED, c.text_hidden_dropout)
        if rng is not None:                                       # hidden_states[0] is the embedding output AFTER its dropout
            ops.dropout_apply(dy, dy, rng)
        a = (tp.ids32, tp.tt32, f32("word_embeddings"), f32("position_embeddings"), f32("token_type_embeddings"), f32("emb_layernorm.weight"), dy,
             ws["t_dxemb"], grad("emb_layernorm.weight"), grad("emb_layernorm.bias"), grad("word_embeddings"), B, T, Dt, c.vocab, c.eps_t)
        if tp.packed:              # d x lands at the tokens' PADDED rows of the zeroed buffer: the position / token-type sums below stay as they are
            ws["t_dxemb"].zero_()
            ops.call("text_embed_ln_bwd_packed", *a, tp.src_row, tp.cnt)
        else:
            ops.call("text_embed_ln_bwd", *a)
        dxe = ws["t_dxemb"].view(B, T, Dt)
        grad("position_embeddings").add_(dxe.sum(dim=0))
        tt = tp.tt32.view(-1).long() if tp.tt32 is not None else torch.zeros(B * T, device=self.device, dtype=torch.long)
        grad("token_type_embeddings").index_add_(0, tt, ws["t_dxemb"])

    def text_soft_target(self) -> torch.Tensor:
        """Caption-to-caption scores of the Soft-GLoRIA losses (medmoe_module.py:258-281 get_text_soft_target): the frozen text model's last
        hidden state at [CLS] (token_pooling :243-244), L2-normalised, all pairwise products -> fp32 [B, B].  The reference runs a second
        pretrained BertModel (`tool_bert`) for it; with `freeze_bert: true` that is the text tower's own BERT, whose last layer the
        forward pass just produced.  Call after forward_text."""
        h, seq_off = self._rows.last, self._rows.seq_off
        B, T, Dt = self.B, self.cfg.max_len, self.cfg.d_t
        rows = seq_off[:B].long() if seq_off is not None else torch.arange(B, device=self.device) * T
        cls = h.view(-1, Dt).index_select(0, rows).float().contiguous()
        n = torch.empty(B, device=self.device); S = torch.empty(B, B, device=self.device)
        ops.call("rownorm", cls, n, B, Dt)
        ops.call("sgemm", cls, cls, S, B, B, Dt, Dt, 1, 1, Dt, B, 1.0, 0.0)
        ops.call("cos_scale", S, n, n, B, B, 1e-24)
        return S

    def _head(self, S, dS, rs, cs, w, accumulate, loss):
        """Cross-entropy against the diagonal, or (cfg.soft_label) the Soft-GLoRIA head, over the rows / columns of a [B, B] matrix."""
        c, B = self.cfg, self.B
        if self.deterministic:
            if c.soft_label:
                ops.call("soft_xent_strided_det", S, dS, self._soft, B, B, rs, cs, c.temp3, c.threshold0, c.threshold1, w, accumulate, loss, self._parts(B))
            else:
                ops.call("ce_strided_det", S, dS, B, B, rs, cs, 0, c.temp3, w, accumulate, loss, self._parts(B))
        elif c.soft_label:
            ops.call("soft_xent_strided", S, dS, self._soft, B, B, rs, cs, c.temp3, c.threshold0, c.threshold1, w, accumulate, loss)
        else:
            ops.call("ce_strided", S, dS, B, B, rs, cs, 0, c.temp3, w, accumulate, loss)

    def _ce(self, S, dS, rows, cols, rs, cs, off, w, accumulate, loss):
        """medmoe_ce_strided with a label offset (the data-parallel heads), or its deterministic form."""
        if self.deterministic:
            ops.call("ce_strided_det", S, dS, rows, cols, rs, cs, off, self.cfg.temp3, w, accumulate, loss, self._parts(rows))
        else:
            ops.call("ce_strided", S, dS, rows, cols, rs, cs, off, self.cfg.temp3, w, accumulate, loss)

    def _cos_scale_bwd(self, *a):
        ops.call("cos_scale_bwd_det" if self.deterministic else "cos_scale_bwd", *a)

    def prefetch_cap_lens(self, ids: torch.Tensor):
        """Word-piece segment map + caption lengths (text_encoder.py:32-90) and an ASYNCHRONOUS copy of the lengths to
        the host.  train_step calls this first, when the device queue is empty, so the one host-side read of the
        step (class tables of the ragged local-loss layout) never waits for the towers and the host keeps issuing
        launches ahead of the device."""
        out = None
        if ids.is_cuda and "seg" in self.ws and tuple(self.ws["seg"].shape) == tuple(ids.shape):
            out = (self.ws["seg"], self.ws["cap"])                  # persistent buffers: no allocation per step, stable addresses for graph capture
        seg, cap = self.vocab.segment_map(ids, out) if out is not None else self.vocab.segment_map(ids)
        self._seg, self.cap_lens = seg, cap
        if cap.is_cuda:
            if self._cap_host is None or self._cap_host.numel() != cap.numel():
                self._cap_host = torch.empty(cap.numel(), dtype=cap.dtype, pin_memory=True)
                self._cap_event = torch.cuda.Event()
            self._cap_host.copy_(cap, non_blocking=True)
            self._cap_event.record()
        else:
            self._cap_host = cap

    def _cap_lens_host(self) -> np.ndarray:
        if self.cap_lens.is_cuda:
            self._cap_event.synchronize()
        return self._cap_host.numpy().astype(np.int64)

    # ------------------------------------------------------------------------------------------
    # losses: forward values + gradients w.r.t. img_g / img_l (text is frozen)
    # ------------------------------------------------------------------------------------------
    def global_loss(self, loss_scale: float = 1.0, grad: bool = True):
        """GLoRIA global loss (losses.py:766-794) of ws["img_g"] against ws["txt_g"], forward and backward: zeroes ws["loss_parts"], adds the
        weighted loss to loss_parts[2], leaves dL/d img_g in ws["d_img_g"] (and dL/d txt_g in ws["d_txt_g"] when the text tower trains).
        Any image encoder that fills ws["img_g"] can call it (the ViT towers here, the Swin-T encoder in medmoe_amd.swin_engine).
        grad=False (eval_step): the loss value only - the heads still write d loss / d S into the scratch ws["dS"] (/ ws["dS2"]), nothing
        reads it and no gradient buffer is touched."""
        c, ws = self.cfg, self.ws
        B, Do = self.B, c.d_out
        ws["loss_parts"].zero_()
        lp = ws["loss_parts"]
        # ---- rows = images, cols = captions ----
        img_g, txt_g = ws["img_g"], ws["txt_g"]
        wg = c.w_global * loss_scale / B
        if c.soft_label:
            if self.dist:
                raise NotImplementedError("soft_label with more than one rank: the reference's Soft-GLoRIA losses are written for one process "
                                          "(losses.py:826-883 has no gather)")
            self._soft = self.text_soft_target()
        if not self.dist:
            ops.call("rownorm", img_g, ws["na"], B, Do)
            ops.call("rownorm", txt_g, ws["nb"], B, Do)
            ops.call("sgemm", img_g, txt_g, ws["S"], B, B, Do, Do, 1, 1, Do, B, 1.0, 0.0)
            ops.call("cos_scale", ws["S"], ws["na"], ws["nb"], B, B, 1e-8)
            self._head(ws["S"], ws["dS"], B, 1, wg, 0, lp[2:])
            self._head(ws["S"], ws["dS"], 1, B, wg, 1, lp[2:])
            if not grad:
                return
            cb = None
            if self.train_text:
                cb = ws["cb"]; cb.zero_()
            self._cos_scale_bwd(ws["dS"], ws["S"], ws["na"], ws["nb"], ws["ca"], cb, B, B, 1e-8)
            ops.call("sgemm", ws["dS"], txt_g, ws["d_img_g"], B, Do, B, B, 1, Do, 1, Do, 1.0, 0.0)
            ops.call("add_rowscaled", ws["d_img_g"], img_g, ws["ca"], B, Do)
            if self.train_text:                                   # the caption side of the same matrix: d txt_g = dS^T img_g + cb txt_g
                ops.call("sgemm", ws["dS"], img_g, ws["d_txt_g"], B, Do, B, 1, B, Do, 1, Do, 1.0, 0.0)
                ops.call("add_rowscaled", ws["d_txt_g"], txt_g, cb, B, Do)
        else:
            # all-gather + local-rows InfoNCE (losses.py:503-524,566-572 with GLoRIA's cosine/temp3):
            # rows = my images vs ALL captions, and my captions vs ALL images; labels offset by rank
            from . import dist as D_
            Bg = B * self.world
            off = D_.label_offset(B)
            img_all, txt_all = D_.gather_embeddings(img_g, txt_g)
            ops.call("rownorm", img_g, ws["na"], B, Do); ops.call("rownorm", txt_all, ws["nb"], Bg, Do)
            ops.call("sgemm", img_g, txt_all, ws["S"], B, Bg, Do, Do, 1, 1, Do, Bg, 1.0, 0.0)
            ops.call("cos_scale", ws["S"], ws["na"], ws["nb"], B, Bg, 1e-8)
            self._ce(ws["S"], ws["dS"], B, Bg, Bg, 1, off, wg, 0, lp[2:])
            if grad:
                cb1 = None
                if self.train_text:
                    cb1 = ws["cb1"]; cb1.zero_()
                self._cos_scale_bwd(ws["dS"], ws["S"], ws["na"], ws["nb"], ws["ca"], cb1, B, Bg, 1e-8)
                ops.call("sgemm", ws["dS"], txt_all, ws["d_img_g"], B, Do, Bg, Bg, 1, Do, 1, Do, 1.0, 0.0)
                ops.call("add_rowscaled", ws["d_img_g"], img_g, ws["ca"], B, Do)
                if self.train_text:       # my images against ALL captions: the gathered captions' gradient, summed over ranks, my slice comes back
                    ops.call("sgemm", ws["dS"], img_g, ws["d_txt_all"], Bg, Do, B, 1, Bg, Do, 1, Do, 1.0, 0.0)
                    ops.call("add_rowscaled", ws["d_txt_all"], txt_all, cb1, Bg, Do)
            ops.call("rownorm", txt_g, ws["na2"], B, Do); ops.call("rownorm", img_all, ws["nb2"], Bg, Do)
            ops.call("sgemm", txt_g, img_all, ws["S2"], B, Bg, Do, Do, 1, 1, Do, Bg, 1.0, 0.0)
            ops.call("cos_scale", ws["S2"], ws["na2"], ws["nb2"], B, Bg, 1e-8)
            self._ce(ws["S2"], ws["dS2"], B, Bg, Bg, 1, off, wg, 0, lp[2:])
            if not grad:
                return
            ws["cb2"].zero_()
            self._cos_scale_bwd(ws["dS2"], ws["S2"], ws["na2"], ws["nb2"], ws["ca2"], ws["cb2"], B, Bg, 1e-8)
            # d img_all = dM^T txt_local + cb * img_all ; summed over ranks, my slice comes back
            ops.call("sgemm", ws["dS2"], txt_g, ws["d_img_all"], Bg, Do, B, 1, Bg, Do, 1, Do, 1.0, 0.0)
            ops.call("add_rowscaled", ws["d_img_all"], img_all, ws["cb2"], Bg, Do)
            ws["d_img_g"].add_(D_.scatter_key_grads(ws["d_img_all"]))
            if self.train_text:       # my captions against ALL images (rows of S2): d txt_g = dS2 img_all + ca2 txt_g, plus the scattered part
                ops.call("sgemm", ws["dS2"], img_all, ws["d_txt_g"], B, Do, Bg, Bg, 1, Do, 1, Do, 1.0, 0.0)
                ops.call("add_rowscaled", ws["d_txt_g"], txt_g, ws["ca2"], B, Do)
                ws["d_txt_g"].add_(D_.scatter_key_grads(ws["d_txt_all"]))

    def _local_loss_object(self):
        """THE local-loss object (GLoRIA local loss, losses.py:961-1026) of this engine for the current batch size, created on first use,
        and whether it scores this rank's images against the gathered captions of every rank (cfg.local_loss_global):
        a trainable text tower takes the word-gradient variant - transposed pair matrices (medmoe_amd/local_transposed.py) where
        pair3.hip has the geometry, else the generic GEMM formulation (local_generic.py); geometries without LDS-tiled pair kernels the
        generic one; gathered captions and 196 / 64 regions the transposed one; 256 regions the [region][word] one (local_ragged.py).
        Each owns its buffers; only ws["sim"] (for B captions) is the engine's."""
        c, B = self.cfg, self.B
        gather = self.dist and c.local_loss_global
        word_grad, Bc = self.train_text, B
        if self.train_text:
            if gather:
                raise NotImplementedError("trainable text tower: the word gradient of the local loss is built for rank-local captions "
                                          "(local_loss_global gathers them)")
            kind, gather = (TransposedLocalLoss if self.local_t else GenericLocalLoss), False
        elif not self.local_fast:
            kind, gather = GenericLocalLoss, False
        elif gather:
            if not self.local_t:
                raise NotImplementedError("local_loss_global needs the transposed local-loss path (196 / 64 regions)")
            kind, Bc = TransposedLocalLoss, B * self.world
        else:
            kind = TransposedLocalLoss if self.local_t else RaggedLocalLoss
        loc = self._local
        if type(loc) is not kind or (loc.B, loc.Bc) != (B, Bc):
            self._local = None                                    # release before allocating
            args = (B, c.n_patch, c.max_len, c.d_out, self.device)
            sim = self.ws["sim"] if Bc == B else None
            if kind is TransposedLocalLoss:
                self._local = kind(*args, gram=self.local_gram, Bc=Bc, word_grad=word_grad, pitch=self.HWq, sim=sim)
            elif kind is GenericLocalLoss:
                self._local = kind(*args, word_grad=word_grad, sim=sim)
            else:
                self._local = kind(*args, sim=sim)
        self._local.det = self._det
        return self._local, gather

    def _local_heads(self, sim, gsim, w: float):
        """The two heads of the local loss (_head) over the rows, then the columns of `sim`: w times their sum is added to loss_parts[3],
        d loss / d sim is left in `gsim`."""
        B, lp = self.B, self.ws["loss_parts"]
        self._head(sim, gsim, B, 1, w, 0, lp[3:])
        self._head(sim, gsim, 1, B, w, 1, lp[3:])

    def _gathered_local_heads(self, sim, w: float):
        """The rank's [B, B_g] block of similarities is all-gathered into the [B_g, B_g] matrix (rows = images in rank order, columns =
        captions) and both cross-entropies run over it on every rank (1 M elements) -> d loss / d of the whole matrix."""
        from . import dist as D_
        c, Bg, lp = self.cfg, self.B * self.world, self.ws["loss_parts"]
        S = D_.gather_rows(sim)
        G = torch.empty_like(S)
        self._ce(S, G, Bg, Bg, Bg, 1, 0, w, 0, lp[3:])
        self._ce(S, G, Bg, Bg, 1, Bg, 0, w, 1, lp[3:])
        return G

    def forward_backward_losses(self, labels: torch.Tensor, loss_scale: float = 1.0):
        """Global and local GLoRIA losses of ws["img_g"] / ws["img_l"] against ws["txt_g"] / ws["words"], forward and backward: the weighted
        values in ws["loss_parts"], the gradients in ws["d_img_g"] / ws["d_img_l"] (and ws["d_txt_g"] / self._d_words with a trainable
        text tower)."""
        c, ws, B = self.cfg, self.ws, self.B
        self.global_loss(loss_scale)
        loc, gather = self._local_loss_object()
        ctx = ws["img_l"].view(B * c.n_patch, c.d_out)
        if gather:
            return self._local_loss_global(loc, ctx, loss_scale)
        lens = (self.cap_lens, self._cap_lens_host()) if loc.host_lens else (self.cap_lens,)     # the ONE host sync of the step, where needed
        sim = loc.forward(ctx, ws["words"], *lens, c.temp1, c.temp2)
        self._local_heads(sim, ws["gsim"], c.w_local * loss_scale / B)
        self._d_words = loc.backward(ws["gsim"], out=ws["d_img_l"])

    def _local_loss_global(self, loc, ctx, loss_scale: float):
        """cfg.local_loss_global under data parallelism: this rank's images against the captions of every rank (the
        variant the reference does not have - its local loss stays rank-local, losses.py:961-1026).  Words and caption lengths are
        all-gathered (the text tower is frozen: no gradient goes back), the heads run over the gathered similarities, and the rank
        back-propagates its own rows.  Gradients are averaged over ranks afterwards, so the rows carry W / B_g = 1 / B."""
        from . import dist as D_
        c, ws, B, W = self.cfg, self.ws, self.B, self.world
        words_all = D_.gather_rows(ws["words"])
        caps_all = D_.gather_rows(self.cap_lens)
        sim = loc.forward(ctx, words_all, caps_all, caps_all.cpu().numpy().astype(np.int64), c.temp1, c.temp2)
        G = self._gathered_local_heads(sim, c.w_local * loss_scale / (B * W))
        r0 = D_.label_offset(B)
        self._d_words = loc.backward((G[r0:r0 + B] * float(W)).contiguous(), out=ws["d_img_l"])

    # ------------------------------------------------------------------------------------------
    # backward through MoE and the ViT
    # ------------------------------------------------------------------------------------------
    def backward(self, labels: Optional[torch.Tensor], loss_scale: float = 1.0, dprobs_ext: Optional[torch.Tensor] = None,
                 bucket_ready=None):
        """Back-propagate ws["d_img_l"] / ws["d_img_g"] (+ the router CE when `labels` is given, + an
        external dL/dprobs) through MoE and the ViT into the flat gradient buffer."""
        c, p, ws = self.cfg, self.params, self.ws
        B, P, Nt, Dv = self.B, c.n_patch, c.n_tok_v, c.d_v
        self._wgrad_begin()
        w_moe = self._moe_backward(labels, loss_scale, dprobs_ext)
        if self.vit_frozen and self.vlora is None:
            # freeze_vit without adapters: the router's and the experts' gradients are complete here, and nothing in or under the tower
            # has a gradient anyone reads - the tower's backward is not run at all
            self._wait(w_moe)
            if bucket_ready is not None:
                bucket_ready(0)
            return
        # ---- mean-pool backward: the router-input gradient onto every patch token of the final LayerNorm's output ----
        ops.call("broadcast_tokens", ws["drouter_in"], ws["dln"], B, Nt, Dv, 1, P, 1.0 / P)
        w_last = self._vit_backward(w_moe, bucket_ready)
        if self.vit_frozen:              # no patch-embedding, class-token or position-embedding backward; _vit_backward joined the second stream
            return
        # ---- embeddings backward ----
        dx = ws["dxa"]
        ops.call("pos_cls_grad", dx, p.grad("vit.pos_embed"), p.grad("vit.cls_token"), B, Nt, Dv)
        ops.gemm_tn(dx, ws["im2col"], p.grad("vit.patch_embed.weight"), db=p.grad("vit.patch_embed.bias"),
                    g_rowmap=ws["rowmap_patch"], M=B * P, det=self._det)
        self._wait(w_last)                                   # join: every weight gradient is final before the optimiser / the caller
        if bucket_ready is not None:
            bucket_ready(0)              # patch / CLS / position embeddings: complete

    # The four weight-gradient GEMMs of a layer run on a SECOND stream: each only needs its gradient operand (event from the
    # main stream) and nothing downstream needs its result before the bucket all-reduce / the optimiser.  At small per-rank
    # batches the dgrad GEMMs leave most CUs idle in their last round of tiles (B = 128: 296 tiles of a K = 2304 dgrad on
    # 256 CUs); the concurrent wgrad fills them.  The scratch gradients (dx, dx2, dz, dqkv) are rewritten one layer later: the
    # main stream waits for the wgrad that read a buffer before the kernel that overwrites it.
    # (measured on one box, cfg2: per-rank batch 128 31.2 -> 29.8 ms, 256 55.9 -> 54.7 ms; at 1024 every GEMM already fills the chip for
    # ~28 rounds and the second stream costs 1.4 %, so it is used up to 131072 token rows)
    def _wgrad_begin(self):
        ws = self.ws
        M = self.B * self.cfg.n_tok_v
        self._wg_side = self._side_stream() if (self.overlap_wgrad and ws["dxa"].is_cuda and M <= 131072) else None
        self._wg_main = torch.cuda.current_stream() if self._wg_side is not None else None

    def _wgrad(self, *a, **kw):
        side, main = self._wg_side, self._wg_main
        if self.deterministic:
            kw["det"] = self._det                                # medmoe_gemm_tn_det with the launch stream's own scratch (ops.DetScratch)
        elif self.wgrad_staged and "row_off" not in kw and "x_rowmap" not in kw and "g_rowmap" not in kw:
            # plain wgrads: partial tiles through a scratch buffer + one summing kernel instead of 64 MB of fp32 atomics per launch
            # (medmoe_gemm_tn_staged); every launch of this method runs on one stream, so one scratch serves them all
            sc = self.ws.get("wg_scratch")
            if sc is None:
                # at most 256 partial tiles per launch, each with its 512 column sums of G behind the tiles: db is staged too
                sc = self.ws["wg_scratch"] = torch.empty(256 * (65536 + 512), device=self.device, dtype=F32)
            kw["scratch"] = sc
        if side is None:
            ops.gemm_tn(*a, **kw)
            return None
        ev = torch.cuda.Event(); ev.record(main); side.wait_event(ev)
        with torch.cuda.stream(side):
            ops.gemm_tn(*a, **kw)
        done = torch.cuda.Event(); done.record(side)
        return done

    def _wait(self, ev):
        if ev is not None:
            self._wg_main.wait_event(ev)

    def _moe_backward(self, labels: Optional[torch.Tensor], loss_scale: float = 1.0, dprobs_ext: Optional[torch.Tensor] = None):
        """MoE backward (swin.py:32-117): from ws["d_img_l"] / ws["d_img_g"] (+ router CE on `labels`, + an external dL/dprobs) to the
        stage-feature gradients ws["dF"], the router-input gradient ws["drouter_in"] and every expert / router weight gradient.
        Returns the event of the last expert wgrad on the second stream (None without one).  Call _wgrad_begin() first."""
        c, p, ws = self.cfg, self.params, self.ws
        B = self.B
        E, k, Do, Dh, Dv, P = c.n_expert, c.top_k, c.d_out, c.d_out // 2, c.d_v, c.n_patch
        R = self.R
        lab32 = labels.to(I32).contiguous() if labels is not None else None
        wgrad = self._wgrad
        use_gate = k > 1
        if use_gate:
            ws["dgate"].zero_()
        sa = (ws["d_img_l"], ws["d_img_g"], ws["G"], ws["H1"], ws["wts"], p.f32("moe.attn2.weight"),
              ws["eout"], ws["expert_of_slot"], ws["item_of_slot"], ws["gates"], k, P, ws["dG"], ws["dH1"],
              p.grad("moe.attn2.weight"), p.grad("moe.attn2.bias"), ws["dgate"] if use_gate else None, R, Do, Dh)
        if self.deterministic:
            sc = self._det.get(ops._scratch_query("scale_attn_bwd_det_scratch", R, P, Dh))
            ops.call("scale_attn_bwd_det", *sa, ws["row_off"], E, sc, sc.numel())
        else:
            ops.call("scale_attn_bwd", *sa)
        grp = self._expert_tiles
        w_moe = None
        for s, l in enumerate(c.stage_layers()):
            wgrad(ws["dH1"][s], ws["G"][s], p.grad("moe.attn0.weight"), db=p.grad("moe.attn0.bias"),
                  row_off=ws["row_off"], n_groups=E, stride_w=Dh * Do, stride_db=Dh, nsplit=4, M=R)
            if c.expert_fp8:      # dgrad on the TRANSPOSED e4m3 weights; their output-channel scales ride on the gradient rows
                self._fp8_gemm(ws["dH1"][s], Dh, None, p.s8("moe.attn0.weight"), p.q8t("moe.attn0.weight"), None, None, ws["dG"][s], Do, Dh, 2,
                               residual=ws["dG"][s], aux=ws["G"][s])
            elif c.expert_mx:     # dgrad on the weight copies quantised along N (the contraction here); no scale folding: the scales are per block
                self._mx_gemm(ws["dH1"][s], Dh, None, p.qmxt("moe.attn0.weight"), None, ws["dG"][s], Do, 2, residual=ws["dG"][s], aux=ws["G"][s])
            else:
                ops.gemm_nt(ws["dH1"][s], p.w16t("moe.attn0.weight"), ws["dG"][s], residual=ws["dG"][s], aux=ws["G"][s],
                            stride_b=Dh * Do, epi=ops.EPI_MUL_DRELU, **grp(Dh))
            w_moe = wgrad(ws["dG"][s], ws[f"x{l}"], p.grad(f"moe.proj.{s}.weight"), db=p.grad(f"moe.proj.{s}.bias"),
                          x_rowmap=ws["rowmap"], row_off=ws["row_off"], n_groups=E, stride_w=Do * Dv, stride_db=Do,
                          nsplit=4, M=R)
            if c.expert_fp8:
                self._fp8_gemm(ws["dG"][s], Do, None, p.s8(f"moe.proj.{s}.weight"), p.q8t(f"moe.proj.{s}.weight"), None, None, ws["dF"][s], Dv, Do, 0)
            elif c.expert_mx:
                self._mx_gemm(ws["dG"][s], Do, None, p.qmxt(f"moe.proj.{s}.weight"), None, ws["dF"][s], Dv, 0)
            else:
                ops.gemm_nt(ws["dG"][s], p.w16t(f"moe.proj.{s}.weight"), ws["dF"][s], stride_b=Do * Dv, **grp(Do))
        # ---- router backward: CE on probabilities (medmoe_module.py:235-237) + gate gradients ----
        Hd = c.router_hidden
        rb = (ws["probs"], ws["router_h"], p.f32("moe.router.2.weight"), ws["idx"],
              ws["dgate"] if use_gate else None, lab32, dprobs_ext, c.w_cls * loss_scale / B, ws["dlogits"], ws["drouter_h"],
              ws["loss_parts"], B, Hd, E, k)
        if self.deterministic:
            ops.call("router_bwd_det", *rb, self._parts(2 * B))
        else:
            ops.call("router_bwd", *rb)
        sg = lambda *a: ops.call("sgemm", *a)
        sg(ws["dlogits"], ws["router_h"], p.grad("moe.router.2.weight"), E, Hd, B, 1, E, Hd, 1, Hd, 1.0, 1.0)
        sg(ws["ones"], ws["dlogits"], p.grad("moe.router.2.bias"), 1, E, B, 0, 1, E, 1, E, 1.0, 1.0)
        sg(ws["drouter_h"], ws["router_in"], p.grad("moe.router.0.weight"), Hd, Dv, B, 1, Hd, Dv, 1, Dv, 1.0, 1.0)
        sg(ws["ones"], ws["drouter_h"], p.grad("moe.router.0.bias"), 1, Hd, B, 0, 1, Hd, 1, Hd, 1.0, 1.0)
        sg(ws["drouter_h"], p.f32("moe.router.0.weight"), ws["drouter_in"], B, Dv, Hd, Hd, 1, Dv, 1, Dv, 1.0, 0.0)
        return w_moe

    def _vit_backward(self, w_moe=None, bucket_ready=None, stage_grads: bool = True):
        """Final LayerNorm + the pre-norm blocks backward: ws["dln"] (gradient w.r.t. the final LayerNorm's output) -> ws["dxa"]
        (gradient w.r.t. ws["x0"]) and every block weight gradient; `stage_grads`: add the experts' stage-feature gradients ws["dF"]
        at the tapped layers.  Returns the event of the last wgrad on the second stream.  Call _wgrad_begin() first.
        Frozen backbone with adapters: the same chain of dgrad GEMMs, LayerNorm and attention backwards WITHOUT any tower
        parameter gradient - the gradient targets are None, which skips the weight-gradient GEMMs and the LayerNorm gamma / beta sums.
        Per layer, after the attention backward has written d qkv: medmoe_lora_bwd_dx (d U, and the adapters' term of d ln1 added into
        the base dgrad GEMM's output) and medmoe_lora_bwd_wgrad_runs (the adapters' gradients, += into their arena).  At layer 0 nothing
        below trains: the dgrad GEMM, the d ln1 term and the first LayerNorm's backward are skipped, and ws["dxa"] is not written.  The one
        bucket of the image arena (router + experts) is reported once the experts' weight gradients are final."""
        c, p, ws = self.cfg, self.params, self.ws
        B = self.B
        k, Dv, P, Nt, H = c.top_k, c.d_v, c.n_patch, c.n_tok_v, c.n_head_v
        wait = self._wait
        fz, lo = self.vit_frozen, self.vlora
        grad = (lambda name: None) if fz else p.grad
        wgrad = (lambda *a, **kw: None) if fz else self._wgrad     # no gradient target: no launch
        L = c.n_layer_v
        dx, dx2 = ws["dxa"], ws["dxb"]
        ops.layernorm_bwd(ws["dln"], ws[f"x{L}"], ws["stf"][0], ws["stf"][1], p.f32("vit.final_layer_norm.weight"), dx,
                          grad("vit.final_layer_norm.weight"), grad("vit.final_layer_norm.bias"), det=self._det)
        if fz:
            wait(w_moe)                  # nothing else runs on the second stream: this is the join
            if bucket_ready is not None:
                bucket_ready(0)          # router + experts: the image arena's only bucket
            bucket_ready = None
        elif bucket_ready is not None:
            wait(w_moe)                  # the experts' weight gradients ran on the second stream
            bucket_ready(L + 1)          # final LN + router + experts: complete
        stage_of = {l: s for s, l in enumerate(c.stage_layers())} if stage_grads else {}
        dp = self._vit_drop_layers()
        w_dz = w_dx2 = w_dqkv = None                       # last wgrad that READ the scratch buffer
        w_set = [None, None]                               # cfg.vit_checkpoint: last wgrad that read a buffer of the shared set
        for l in range(L - 1, -1, -1):
            pre = f"vit.layer.{l}."
            act = lambda name: self._act(l, name)
            if self._ck_shared:
                # recompute what the mode did not keep into the shared set of this parity.  Layer l + 2 used the set: its weight-gradient
                # GEMMs may still be reading h, ln2, att, ln1 on the second stream, which runs in order - the last one's event covers all four
                wait(w_set[l & 1])
                if dp[l] is not None and self.vit_checkpoint == "full":
                    wait(w_dx2)                            # the out-proj branch passes through dp_a again: layer l + 1's out-proj wgrad read it
                self._vit_layer_forward(l, dp[l], recompute=True)
            if (l + 1) in stage_of:
                ops.call("stage_grad_add", ws["dF"][stage_of[l + 1]], ws["slot_of"], dx, B, k, P, Nt, Dv)
            st1, st2 = ws[f"st1_{l}"], ws[f"st2_{l}"]
            # FFN: x_out = h W2^T + b2 + xmid
            # stochastic depth: the branch gradient is s[l, 1] (.) dx, a copy of its own (after stage_grad_add; the LayerNorm-backward below
            # keeps the unscaled dx for the identity path).  dp_b was last read by layer l + 1's FC2 wgrad, which that layer waited for
            g2 = dx
            if dp[l] is not None:
                g2 = ws["dp_b"]
                ops.call("drop_path", dx, None, dp[l][1], g2, B, Nt * Dv)
            w_dx = wgrad(g2, act("h"), grad(pre + "feedforward.model.2.weight"), db=grad(pre + "feedforward.model.2.bias"))
            wait(w_dz)
            ops.gemm_nt(g2, p.w16t(pre + "feedforward.model.2.weight"), ws["dz"], aux=act("z"), epi=ops.EPI_MUL_AUX)
            w_dz = wgrad(ws["dz"], act("ln2"), grad(pre + "feedforward.model.0.weight"), db=grad(pre + "feedforward.model.0.bias"))
            ops.gemm_nt(ws["dz"], p.w16t(pre + "feedforward.model.0.weight"), ws["dln"])
            wait(w_dx2)
            ops.layernorm_bwd(ws["dln"], act("xmid"), st2[0], st2[1], p.f32(pre + "feedforward_layernorm.weight"), dx2,
                              grad(pre + "feedforward_layernorm.weight"), grad(pre + "feedforward_layernorm.bias"), add=dx, det=self._det)
            # attention: xmid = att Wo^T + bo + x
            # dp_a was last read by layer l + 1's out-proj wgrad: wait(w_dx2) above covers it
            g1 = dx2
            if dp[l] is not None:
                g1 = ws["dp_a"]
                ops.call("drop_path", dx2, None, dp[l][0], g1, B, Nt * Dv)
            w_dx2 = wgrad(g1, act("att"), grad(pre + "attention.output_proj.weight"), db=grad(pre + "attention.output_proj.bias"))
            ops.gemm_nt(g1, p.w16t(pre + "attention.output_proj.weight"), ws["datt"])
            wait(w_dqkv)
            ops.attn_bwd(act("qkv"), act("att"), ws["datt"], ws[f"lse{l}"], None, ws["dqkv"], ws["delta"], B, Nt, H)
            w_dqkv = wgrad(ws["dqkv"], act("ln1"), grad(pre + "attention.input_proj.weight"), db=grad(pre + "attention.input_proj.bias"))
            w_set[l & 1] = w_dqkv
            below = not fz or l > 0                          # something that trains reads this layer's input
            if below:
                ops.gemm_nt(ws["dqkv"], p.w16t(pre + "attention.input_proj.weight"), ws["dln"])
            if lo is not None:
                rng = self._vit_lora_rng(l)
                ops.lora_bwd_dx(ws["dqkv"], lo.B16t(l), lo.A16t(l), ws["v_ldu"], ws["dln"] if below else None, lo.targets, lo.scale, rng)
                ops.lora_bwd_wgrad_runs(ws["dqkv"], act("ln1"), ws[f"v_lu{l}"], ws["v_ldu"], lo.gA(l), lo.gB(l), ws["v_lsc"], lo.targets, lo.scale,
                                        self._vlora_run, rng)
            if not below:
                break
            wait(w_dx)                                       # the FC2 wgrad read dx (or dp_b): done before LayerNorm-backward rewrites dx
                                                             # (and before the next layer rewrites dp_b)
            ops.layernorm_bwd(ws["dln"], ws[f"x{l}"], st1[0], st1[1], p.f32(pre + "attention_layernorm.weight"), dx,
                              grad(pre + "attention_layernorm.weight"), grad(pre + "attention_layernorm.bias"), add=dx2, det=self._det)
            if bucket_ready is not None:
                wait(w_dqkv)                                 # the side stream runs in order: its last wgrad of the layer covers all four
                bucket_ready(l + 1)      # layer l: complete
        return w_dqkv

    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    # ------------------------------------------------------------------------------------------
    def train_step(self, batch: Dict[str, torch.Tensor], optimizer: bool = True, zero_grad: bool = True, loss_scale: float = 1.0):
        """medmoe_module.py:284-316 model_step + backward + clip + Adam.  Returns device scalars.
        Gradient accumulation (accumulate_grad_batches of the trainer config): call with optimizer=False for all but the
        last micro-batch, zero_grad=False for all but the first, loss_scale = 1 / number of micro-batches; the reported
        losses are scaled the same way."""
        if self._ema_active:
            raise RuntimeError("train_step inside ema_weights(): the working copies hold the averaged weights - evaluate only")
        if self.use_graph and not self.dist and not self.train_text and batch["image"].is_cuda and ops.PROFILE is None:
            return self._train_step_graphed(batch, optimizer, zero_grad, loss_scale)
        B = batch["image"].shape[0]
        self._alloc(B)
        self.prefetch_cap_lens(batch["ids"])
        if zero_grad:
            self.params.zero_grad()
            if self.train_text:
                self.text_arena().zero_grad()
            if self.vlora is not None:
                self.vlora.zero_grad()
            if self.mlm is not None:
                self.mlm.store.zero_grad()
        try:
            if self.mlm is not None:                                # this step's mask; the head's loss carries mlm_weight and loss_scale
                self._mlm_pass = (self.dropout_step, self.cfg.mlm_weight * loss_scale)
            self._forward_both(batch, training=True)
            out = self._train_step_rest(batch, optimizer, loss_scale)
            if self.mlm is not None:
                out.update(self._mlm_result(self.cfg.mlm_weight))
                out["loss"] = out["loss"] + self.cfg.mlm_weight * out["mlm_loss"]
            return out
        finally:
            self._end_training_pass()
            self._mlm_pass = None

    def _mlm_result(self, weight: float):
        """mlm_loss (the head's loss without mlm_weight; it follows loss_scale like the other parts) and mlm_acc (the share of the masked
        positions whose target is the arg max) of the last MLM pass: device scalars."""
        b = self.mlm.buf
        return {"mlm_loss": b.loss[0] / weight, "mlm_acc": b.counts[1].float() / b.counts[0].clamp(min=1).float()}

    def mlm_eval(self, batch: Dict[str, torch.Tensor], step: int = 0, ema: bool = False):
        """mlm_loss / mlm_acc of a batch under the FIXED mask of `step` (the same step gives the same mask), forward only: the text pass of
        an evaluation (no dropout) on the masked ids and the head; no gradient, Adam moment, master or working parameter is written."""
        if self.mlm is None:
            raise RuntimeError("mlm_eval: this engine has no MLM head (cfg.text_mlm)")
        with self._weights(ema):
            self._alloc(batch["ids"].shape[0])
            self.prefetch_cap_lens(batch["ids"])
            self._mlm_pass = (int(step), 1.0)
            try:
                self.forward_text(batch["ids"], batch["attn_mask"], batch.get("token_type"))
                return self._mlm_result(1.0)
            finally:
                self._mlm_pass = None

    def _forward_image_train(self, images: torch.Tensor):
        """forward_image of a training step: with cfg.vit_drop_path > 0 under the stochastic-depth scales of self.dropout_step, drawn here by
        ONE launch for all 2 L sites ahead of the tower (column offset = this rank's first sample; they stay in ws["vit_dp"] for the backward
        of the same step)."""
        c = self.cfg
        if c.vit_drop_path > 0.0:
            probs = [pl for pl in c.vit_drop_path_rates() for _ in range(2)]
            ops.drop_path_scales(self.ws["vit_dp"], probs, self.B, self.rank * self.B, c.dropout_seed, self.dropout_step)
            self.vit_drop_scales = self.ws["vit_dp"]
        if self.vlora is not None and c.vit_lora_dropout > 0.0:     # the adapters' masks of this step, for the forward and the backward
            self._vit_lora_drop_step = self.dropout_step
        self.forward_image(images)

    def _end_training_pass(self):
        """Whatever runs after a training pass (evaluation, a bare forward_image) drops nothing: in the `finally` of every step that ran
        _forward_image_train."""
        self.vit_drop_scales = None
        self._vit_lora_drop_step = None

    def _train_step_rest(self, batch: Dict[str, torch.Tensor], optimizer: bool, loss_scale: float):
        """train_step from the losses on: backward, gradient exchange, optimiser."""
        self.forward_backward_losses(batch["label"], loss_scale)
        if self.dist:
            from . import dist as D_
            if optimizer:
                # the arena (bf16 exchange) or None.  The fp32 exchange keeps the two-argument call: reducers that stand in
                # for the class (tests/test_host_logic.py's dry run) take (flat, bounds) and nothing else
                comm = self.grad_comm(self.params)
                red = D_.BucketedAllReduce(self.params.g32, self.bucket_bounds) if comm is None else \
                    D_.BucketedAllReduce(self.params.g32, self.bucket_bounds, comm=comm)
                self.backward(batch["label"], loss_scale, bucket_ready=red.ready)     # all-reduce overlapped with backward
                red.finish()
            else:
                self.backward(batch["label"], loss_scale)                             # accumulate locally, reduce with the last micro-batch
        else:
            self.backward(batch["label"], loss_scale)
        if self.train_text:
            self.backward_text(self._d_words, self.ws["d_txt_g"])
            if self.dist and optimizer:                           # the text tower's gradient: one more all-reduce (not overlapped)
                from . import dist as D_
                D_.allreduce_mean_(self.text_arena().g32, comm=self.grad_comm(self.text_arena()))
        if self.vlora is not None and self.dist and optimizer:    # the image adapters' gradient: one more all-reduce, as the text arena's
            from . import dist as D_
            D_.allreduce_mean_(self.vlora.g32, comm=self.grad_comm(self.vlora))
        if self.mlm is not None and self.dist and optimizer:      # the MLM head's gradient likewise
            from . import dist as D_
            D_.allreduce_mean_(self.mlm.store.g32, comm=self.grad_comm(self.mlm.store))
        self.dropout_step += 1                                      # the next call draws new masks (evaluation never advances it)
        if optimizer:
            self.optimizer_step()
        return self._step_result(loss_scale)

    def _step_result(self, loss_scale: Optional[float]):
        """The dict a step returns (device scalars).  loss_parts hold the WEIGHTED global/local parts; report the reference's unweighted
        names too.  The router CE kernel reports the plain mean: a training step scales it here so that every reported loss follows
        loss_scale; an evaluation (None) reports a copy of it as it is."""
        lp, c = self.ws["loss_parts"], self.cfg
        cls = lp[0].clone() if loss_scale is None else lp[0] * loss_scale
        return {"loss": c.w_cls * cls + lp[2] + lp[3], "classifier_loss": cls, "classifier_acc": lp[1],
                "g_loss": lp[2] / c.w_global, "l_loss": lp[3] / c.w_local}

    def optimizer_step(self, lr: Optional[float] = None):
        """clip_grad_norm_(cfg.clip) + torch.optim.Adam(lr, weight_decay) (cfg.optimizer = "adamw": torch.optim.AdamW; cfg.adam_betas /
        adam_eps; the parameter groups the stores carry), fused, on the gradients the stores hold; the working copies follow.  ONE clip
        norm over both towers' gradients when the text tower trains, as clip_grad_norm_ over all parameters computes it.
        cfg.ema_decay > 0: the same launches also advance every stepped arena's weight average.
        cfg.optimizer = "lamb": behind the same clip norm every arena takes FlatArena.lamb_step instead - three launches, one trust ratio per
        parameter tensor."""
        c, image, text = self.cfg, self.params, self.text_arena() if self.train_text else None
        if self._ema_active:
            raise RuntimeError("optimizer_step inside ema_weights(): the working copies hold the averaged weights - evaluate only")
        lr = c.lr if lr is None else lr
        mlm = self.mlm.store if self.mlm is not None else None
        side = [a for a in (text, self.vlora, mlm) if a is not None]     # the arenas next to the image one: ONE clip norm over all of them
        total = self._clip_total([image] + side)
        step, kw = fused_step_of(c)                                 # adam_step, or lamb_step (cfg.optimizer = "lamb")
        if c.ema_decay > 0.0:                                       # the same launches in their _ema form: every arena, the same decay arguments
            ema_.prepare([image] + side)
            kw.update(ema_.step_kwargs(c))
        for a in [image] + side:
            getattr(a, step)(total, lr, c.weight_decay, c.clip, **kw)

    @staticmethod
    def _clip_total(arenas):
        """The squared gradient norm over `arenas` (the image arena first): a device scalar, the image arena's own sumsq() buffer.  The
        others' partials are launched first and then added in list order - fp32 addition is not associative, so that order decides the
        bits of the clip factor."""
        parts = [a.sumsq() for a in arenas[1:]]
        total = arenas[0].sumsq()
        for part in parts:
            total.add_(part)
        return total

    def _weights(self, ema: bool):
        """The context of a forward-only method's body: ema_weights() for ema=True (unless the caller is already inside it), else nothing."""
        return self.ema_weights() if ema and not self._ema_active else contextlib.nullcontext()

    # ------------------------------------------------------------------------------------------
    # evaluation (medmoe_module.py:114-134 validation_step / test_step: model_step without a backward)
    # ------------------------------------------------------------------------------------------
    def eval_step(self, batch: Dict[str, torch.Tensor], ema: bool = False):
        """The losses of `train_step` on a batch, forward only: same dict, same weighting, device scalars.  No gradient, Adam moment, master
        or working parameter is written.  The towers and the global loss are the training launches; the local loss of the 196 / 64-region
        geometries runs medmoe_local_sim_fwd (csrc/local_eval.hip), which keeps a pair's scores and attention on the chip - an engine that
        only evaluates never allocates the ragged pair matrices; other geometries run the forward launches of the generic formulation.
        The router's cross-entropy and accuracy come from medmoe_router_eval.  Always eager (no hipGraph replay).
        ema=True: this one evaluation runs on the averaged weights (inside ema_weights())."""
        with self._weights(ema):
            B = batch["image"].shape[0]
            self._alloc(B)
            self.prefetch_cap_lens(batch["ids"])
            self._forward_both(batch)
            self.global_loss(grad=False)
            self._local_loss_eval()
            ops.call("router_eval", self.ws["probs"], batch["label"].to(I32).contiguous(), self.ws["loss_parts"], B, self.cfg.n_expert)
            return self._step_result(None)

    # -- embeddings without a loss (retrieval and zero-shot evaluation) ---------------------------------------------------------
    def embed(self, batch: Dict[str, torch.Tensor], ema: bool = False):
        """(img_g, txt_g): the global image and sentence embeddings of a batch, fp32 [B, d_out] VIEWS of ws["img_g"] / ws["txt_g"], valid until
        the next engine call.  The forward launches of `eval_step` and nothing after them: no loss, and no parameter, gradient, Adam or EMA
        buffer is written.  ema=True: on the averaged weights (inside ema_weights()), as eval_step(ema=True)."""
        with self._weights(ema):
            self._alloc(batch["image"].shape[0])
            self.prefetch_cap_lens(batch["ids"])
            self._forward_both(batch)
            return self.ws["img_g"], self.ws["txt_g"]

    def embed_image(self, images: torch.Tensor, ema: bool = False):
        """The image half of `embed` alone: fp32 [B, d_out] view of ws["img_g"], valid until the next engine call."""
        with self._weights(ema):
            self.forward_image(images)
            return self.ws["img_g"]

    def embed_text(self, ids: torch.Tensor, attn_mask: torch.Tensor, token_type: Optional[torch.Tensor] = None, ema: bool = False):
        """The text half of `embed` alone - needs no image pass before it (a set of class prompts has none): fp32 [B, d_out] view of
        ws["txt_g"], valid until the next engine call."""
        with self._weights(ema):
            self._alloc(ids.shape[0])
            self.prefetch_cap_lens(ids)
            self.forward_text(ids, attn_mask, token_type)
            return self.ws["txt_g"]

    # -- supervised heads on the image features: classification on the global embedding, segmentation on the regions (3t) ------
    def _head_refuse(self, spec: HeadSpec, train_tower: Optional[bool]):
        """What the head steps are not built for; train_tower None: an evaluation."""
        if self.dist:
            raise NotImplementedError(f"{spec.step} / {spec.eval} under data parallelism (self.dist: WORLD_SIZE > 1, trainer.devices > 1): "
                                      f"{spec.unreduced} no all-reduce yet - data-parallel {spec.task} is a named follow-up (DESIGN {spec.design})")
        if train_tower and self.cfg.ema_decay > 0.0:
            raise NotImplementedError(f"{spec.step}(train_tower=True) with cfg.ema_decay > 0 (model.ema.decay): the head keeps no average, so the "
                                      f"towers' averages would pair with an un-averaged head - EMA of the head is a named follow-up (DESIGN {spec.design})")
        if train_tower is not None and self.cfg.optimizer == "lamb":
            raise NotImplementedError(f"{spec.step} with cfg.optimizer = 'lamb' (model.optimizer._target_: src.optim.Lamb): the head's fused step "
                                      f"carries its own Adam - LAMB for the {spec.task} head is a named follow-up (DESIGN 3s)")

    def _head_step(self, batch: Dict[str, torch.Tensor], head, spec: HeadSpec, train_tower: bool, optimizer: bool, zero_grad: bool,
                   loss_scale: float, head_lr: Optional[float]):
        """One supervised step of `head` (a head.LinearHead) on ws[spec.feat] of batch["image"] against batch[spec.target]: what
        classify_step and segment_step document."""
        self._head_refuse(spec, train_tower)
        if self._ema_active:
            raise RuntimeError(f"{spec.step} inside ema_weights(): the working copies hold the averaged weights - evaluate only")
        c, images = self.cfg, batch["image"]
        self._alloc(images.shape[0])
        ws = self.ws
        lr = c.lr if head_lr is None else float(head_lr)
        kw = dict(betas=tuple(c.adam_betas), eps=c.adam_eps, decoupled=c.optimizer == "adamw")
        if not train_tower:
            self.forward_image(images)
            if zero_grad:
                head.store.zero_grad()
            out = head.step(ws[spec.feat], batch[spec.target], loss_scale)
            if optimizer:
                head.adam_step(lr, c.weight_decay, c.clip, **kw)
            return spec.result(out)
        towers = [self.params] + ([self.vlora] if self.vlora is not None else [])
        if zero_grad:
            for a in towers:
                a.zero_grad()
            head.store.zero_grad()
        try:
            self._forward_image_train(images)
            out = head.step(ws[spec.feat], batch[spec.target], loss_scale, dfeat=ws[spec.d_written])
            ws[spec.d_zeroed].zero_()
            self.backward(None, loss_scale)
        finally:
            self._end_training_pass()
        self.dropout_step += 1
        if optimizer:
            total = self._clip_total(towers + [head.store])
            for a in towers:
                a.adam_step(total, c.lr, c.weight_decay, c.clip, **kw)
            head.adam_step(lr, c.weight_decay, c.clip, normsq_total=total, **kw)
        return spec.result(out)

    def _head_eval(self, batch: Dict[str, torch.Tensor], head, spec: HeadSpec, ema: bool):
        """(logits, loss dict) of `head` on a batch, forward only: what classify_eval and segment_eval document."""
        self._head_refuse(spec, None)
        with self._weights(ema):
            self.forward_image(batch["image"])
            out = head.evaluate(self.ws[spec.feat], batch[spec.target])
            return head.last_logits, spec.result(out)

    def classify_step(self, batch: Dict[str, torch.Tensor], head, train_tower: bool, optimizer: bool = True, zero_grad: bool = True,
                      loss_scale: float = 1.0, head_lr: Optional[float] = None):
        """One supervised step of `head` (medmoe_amd.classify.ClassifierHead) on ws["img_g"] of batch["image"] against batch["label"] (int
        [B] class indices, or int [B, C] in {0, 1, -1} for a multilabel head; -1 = not counted).  No caption is read, the text tower is not run.
        train_tower=False, the online linear probe: forward_image in its evaluation form (no drop path, no adapter dropout), the head's
        fused forward / loss / backward launch, the head's Adam step - not one parameter, gradient, Adam or EMA buffer of the engine's own
        stores is written, and dropout_step stays.
        train_tower=True, fine-tuning: the training form of the image pass (drop path, adapter dropout and recomputation as in train_step),
        the head launch writes d loss / d img_g into ws["d_img_g"], ws["d_img_l"] is zeroed and backward(None) runs unchanged - so a
        freeze_vit engine fine-tunes MoE + head and a vit_lora engine adapters + MoE + head.  ONE clip norm over the image arena, the
        adapters and the head, then Adam on each, the head at head_lr (default cfg.lr); dropout_step advances.
        Gradient accumulation as in train_step: optimizer=False for all but the last micro-batch, zero_grad=False for all but the first,
        loss_scale = 1 / number of micro-batches.  Always eager.  Returns device scalars: loss, n_valid, n_correct, acc."""
        return self._head_step(batch, head, CLASSIFY, train_tower, optimizer, zero_grad, loss_scale, head_lr)

    def classify_eval(self, batch: Dict[str, torch.Tensor], head, ema: bool = False):
        """(logits, loss dict) of `head` on a batch, forward only: the evaluation form of the image pass, then the head launch with
        loss_scale 1 into gradient buffers of its own that nobody reads (ClassifierHead.evaluate) - no parameter, gradient or optimiser
        state of the engine or the head is written.  logits: fp32 [B, C] view of the head's workspace, valid until its next launch.
        ema=True: the image pass runs on the averaged weights (inside ema_weights()); the head keeps no average."""
        return self._head_eval(batch, head, CLASSIFY, ema)

    def segment_step(self, batch: Dict[str, torch.Tensor], head, train_tower: bool, optimizer: bool = True, zero_grad: bool = True,
                     loss_scale: float = 1.0, head_lr: Optional[float] = None):
        """One supervised step of `head` (medmoe_amd.segment.SegmenterHead) on ws["img_l"] of batch["image"] against batch["mask"] (int8
        [B, C, H, W] in {0, 1, -1}, -1 = ignored; the other forms of segment.prepare_masks are accepted).  The mask size is free: any
        H, W >= the patch grid.  No caption is read, the text tower is not run.
        train_tower=False, the online probe: forward_image in its evaluation form (no drop path, no adapter dropout), the head's four
        launches, the head's Adam step - not one parameter, gradient, Adam or EMA buffer of the engine's own stores is written, and
        dropout_step stays.
        train_tower=True, fine-tuning: the training form of the image pass (drop path, adapter dropout and recomputation as in train_step),
        the head WRITES d loss / d img_l into all of ws["d_img_l"], ws["d_img_g"] is zeroed and backward(None) runs unchanged - so a
        freeze_vit engine fine-tunes MoE + head and a vit_lora engine adapters + MoE + head.  ONE clip norm over the image arena, the
        adapters and the head, then Adam on each, the head at head_lr (default cfg.lr); dropout_step advances.
        Gradient accumulation as in train_step (optimizer=False for all but the last micro-batch, zero_grad=False for all but the first,
        loss_scale = 1 / number of micro-batches) reproduces the one-batch step only for a head with w_dice = 0: the Dice sums run over the
        micro-batch a call sees (batch Dice is not additive).  Always eager.  Returns device tensors: loss, counts int64 [C, 4] =
        (n_valid, TP, FP, FN), n_valid (their sum over the classes)."""
        return self._head_step(batch, head, SEGMENT, train_tower, optimizer, zero_grad, loss_scale, head_lr)

    def segment_eval(self, batch: Dict[str, torch.Tensor], head, ema: bool = False):
        """(patch logits, loss dict) of `head` on a batch, forward only: the evaluation form of the image pass, the head's row pass and the
        stats half of its loss launch at loss_scale 1 - no parameter, gradient or optimiser state of the engine or the head is written.
        patch logits: fp32 [B, P, C] view of the head's workspace, valid until its next launch (head.predict / ops.seg_predict turn them
        into masks); dict["counts"] feeds a segment.SegBank.  ema=True: the image pass runs on the averaged weights; the head keeps no average."""
        return self._head_eval(batch, head, SEGMENT, ema)

    # -- phrase grounding: word-region heat maps scored against boxes ---------------------------------------------------------
    def _ground_refuse(self):
        c = self.cfg
        if c.d_t != c.d_out:
            raise NotImplementedError(f"Engine.ground: word features of width d_t = {c.d_t} against regions of d_out = {c.d_out} - the score of a "
                                      "word against a region needs one width")

    def ground(self, batch: Dict[str, torch.Tensor], mode: str = "attention", thetas=(0.5,), size=None, ema: bool = False, want_map: bool = False):
        """Phrase grounding of the matched pairs of a batch: the forward launches of `embed` and nothing after them, then the two launches
        of csrc/ground.hip (`ground_workspace`).  batch["span"]: int [B, 2] half-open WORD spans (rows of ws["words"]), or batch["tok_span"]:
        int [B, 2] token spans, mapped through the word-piece segment map (ground.word_spans); batch["box"]: int [B, NB, 4] = (x0, y0, x1, y1)
        half-open pixel rectangles of the `size` = (H, W) frame (default: the image size), absent ones empty.  Returns the records of
        ops.ground_score (a dict of device tensors, what a ground.GroundBank adds) with "h", the grid maps fp32 [B, P], and with want_map
        "hf" fp32 [B, H, W].  No parameter, gradient, moment or EMA buffer is written.  ema=True: on the averaged weights.  More than one
        rank: every rank scores its own shard."""
        self._ground_refuse()
        with self._weights(ema):
            self.embed(batch)
            return self.ground_workspace(batch, mode, thetas, size, want_map)

    def ground_workspace(self, batch: Dict[str, torch.Tensor], mode: str = "attention", thetas=(0.5,), size=None, want_map: bool = False,
                         span_key: str = "span", box_key: str = "box"):
        """The two grounding launches on the features the last forward of this batch left in the workspace (ws["img_l"], ws["words"],
        cap_lens) - `ground` without its forward; a validation step that already ran the towers calls this."""
        from . import ground as ground_
        self._ground_refuse()
        ws, B = self.ws, self.B
        if span_key in batch:
            spans = torch.as_tensor(batch[span_key]).detach().cpu().to(torch.int64).reshape(-1, 2)
        elif "tok_span" in batch:
            tok = torch.as_tensor(batch["tok_span"]).detach().cpu().to(torch.int64).reshape(-1, 2)
            seg = ws.get("seg")                                      # the segment map prefetch_cap_lens wrote for this batch
            if seg is None or tuple(seg.shape) != tuple(batch["ids"].shape):
                seg = self.vocab.segment_map(batch["ids"])[0]
            spans = ground_.word_spans(seg, tok[:, 0], tok[:, 1])
        else:
            raise KeyError(f"Engine.ground: the batch holds neither '{span_key}' (word spans) nor 'tok_span' (token spans)")
        if box_key not in batch:
            raise KeyError(f"Engine.ground: the batch holds no '{box_key}'")
        if spans.shape[0] != B:
            raise ValueError(f"Engine.ground: {spans.shape[0]} spans for a batch of {B}")
        if size is None:
            size = tuple(batch["image"].shape[-2:])
        pair = torch.arange(B, dtype=torch.int64)
        entries = torch.stack([pair, pair, spans[:, 0], spans[:, 1]], dim=1)
        h = ops.ground_maps(ws["img_l"], ws["words"], self.cap_lens, entries, mode=mode, temp1=self.cfg.temp1, cap_lens_host=self._cap_lens_host())
        out = ops.ground_score(h, batch[box_key], size, thetas=thetas, want_map=want_map)
        out["h"] = h
        return out

    def _local_loss_eval(self):
        """GLoRIA local loss value (losses.py:961-1026) of ws["img_l"] against ws["words"] into loss_parts[3]; ws["gsim"] is the heads' scratch.
        The transposed object lends medmoe_local_sim_fwd its Gram matrices, tile tables and word norms - its pair matrices are not touched
        (nor allocated, if no training step came before)."""
        c, ws, B = self.cfg, self.ws, self.B
        P, T, Do = c.n_patch, c.max_len, c.d_out
        ctx = ws["img_l"].view(B * P, Do)
        loc, gather = self._local_loss_object()
        words, caps = ws["words"], self.cap_lens
        if gather:      # this rank's images against the captions of every rank, the heads of _local_loss_global
            from . import dist as D_
            words, caps = D_.gather_rows(words), D_.gather_rows(caps)
        if isinstance(loc, TransposedLocalLoss):
            caps_host = caps.cpu().numpy().astype(np.int64) if gather else self._cap_lens_host()
            sim = local_sim_forward(ctx, words, caps, caps_host, c.temp1, c.temp2, P=P, gm3=loc.gm3, gm3_crowmap=loc.gm3_crowmap,
                                    img_tiles=loc.img_tiles, img_tile_count=loc.img_tile_count, wn=loc.wn, sim=loc.sim)
        elif isinstance(loc, GenericLocalLoss):
            sim = loc.forward(ctx, words, caps, c.temp1, c.temp2)
        else:           # 256 regions: training uses the LDS-tiled pair kernels, whose forward and backward are one launch
            if self._gle is None:
                self._gle = GenericLocalLoss(B, P, T, Do, self.device, sim=ws["sim"])
            self._gle.det = self._det
            sim = self._gle.forward(ctx, words, caps, c.temp1, c.temp2)
        if gather:
            self._gathered_local_heads(sim, c.w_local / (B * self.world))
        else:
            self._local_heads(sim, ws["gsim"], c.w_local / B)

    def _forward_both(self, b, training: bool = False):
        """Both towers' forward passes; `training`: those of a training step (the image tower's stochastic depth, the text tower's dropouts)."""
        forward_image = self._forward_image_train if training else self.forward_image
        if self.overlap_wgrad and b["image"].is_cuda and self.B * self.cfg.n_tok_v <= 131072:
            # the text tower is independent of the image tower: at small per-rank batches its GEMMs (77 tokens per pair) fill
            # a fraction of the chip, so it runs on the second stream underneath the image tower
            main, side = torch.cuda.current_stream(), self._side_stream()
            ev = torch.cuda.Event(); ev.record(main); side.wait_event(ev)
            with torch.cuda.stream(side):
                self.forward_text(b["ids"], b["attn_mask"], b.get("token_type"), training=training)
                done = torch.cuda.Event(); done.record(side)
            forward_image(b["image"])
            main.wait_event(done)
        else:
            forward_image(b["image"])
            self.forward_text(b["ids"], b["attn_mask"], b.get("token_type"), training=training)

    def _train_step_graphed(self, batch, optimizer, zero_grad, loss_scale):
        """train_step with the forward and the backward replayed from hipGraphs (MEDMOE_GRAPH=1).  The first two steps of a (batch size,
        loss_scale, zero_grad) combination run eagerly (every buffer gets allocated, the library's lazy state settles), the third is captured."""
        B = batch["image"].shape[0]
        self._alloc(B)
        key = (B, float(loss_scale), bool(zero_grad), tuple(sorted(batch.keys())))
        st = self._graph
        if st is None or st["key"] != key:
            st = self._graph = {"key": key, "in": {k: torch.empty_like(v) for k, v in batch.items()}, "fwd": None, "bwd": None, "warm": 0}
        b = st["in"]
        for k, v in batch.items():
            b[k].copy_(v)
        self.prefetch_cap_lens(b["ids"])                          # eager: its copy to the host and the event the losses wait on

        def fwd():
            if zero_grad:
                self.params.zero_grad()
                if self.vlora is not None:
                    self.vlora.zero_grad()
            self._forward_both(b)

        if st["warm"] < 2:
            st["warm"] += 1
            fwd()
            self.forward_backward_losses(b["label"], loss_scale)
            self.backward(b["label"], loss_scale)
        else:
            if st["fwd"] is None:
                torch.cuda.synchronize()
                st["fwd"] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(st["fwd"]):
                    fwd()
            st["fwd"].replay()
            self._seg = None                                      # forward_text consumed it at capture time
            self.forward_backward_losses(b["label"], loss_scale)
            if st["bwd"] is None:
                torch.cuda.synchronize()
                st["bwd"] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(st["bwd"]):
                    self.backward(b["label"], loss_scale)
            st["bwd"].replay()
        if optimizer:
            self.optimizer_step()
        return self._step_result(loss_scale)

    # reference-layout views (med_moe.py:102-108)
    def outputs(self):
        c, ws = self.cfg, self.ws
        B, P = self.B, c.n_patch
        Hh = int(P ** 0.5)
        return {"img_g": ws["img_g"], "img_l": ws["img_l"].float().transpose(1, 2).reshape(B, c.d_out, Hh, Hh),
                "txt_g": ws["txt_g"], "txt_l": ws["words32"].transpose(1, 2), "probs": ws["probs"], "idx": ws["idx"],
                "cap_lens": self.cap_lens}
