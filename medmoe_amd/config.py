"""Model / loss configuration of the MedMoE hot path (mirrors the reference's Hydra keys:
configs/model/med-moe.yaml, configs/model/med-moe_pretraining.yaml; ViT/MoE geometry per
BASELINE.json configs)."""
from dataclasses import dataclass
from typing import List, Tuple

VIT_CHECKPOINT_MODES = ("none", "selective", "full")


@dataclass
class MedMoEConfig:
    # image tower: pre-norm ViT blocks (reference transformer.py:98-114), eps 1e-6, final LN
    img_size: int = 224
    patch: int = 16
    d_v: int = 768
    n_layer_v: int = 12
    n_head_v: int = 12
    ff_v: int = 3072
    eps_v: float = 1e-6
    # text tower: post-norm BERT-geometry blocks (transformer.py:116-130), eps 1e-12, frozen
    vocab: int = 28996
    max_len: int = 77
    d_t: int = 768
    n_layer_t: int = 12
    n_head_t: int = 12
    ff_t: int = 3072
    eps_t: float = 1e-12
    last_n_layers: int = 4
    freeze_text: bool = True      # configs/model/med-moe.yaml:35 freeze_bert: true (the experiment); False = the text tower trains too
                                  # (text_encoder.py:27-30): padded text pass with saved activations, text backward, word gradients of the local loss
    # train-mode dropout of the TRAINABLE text tower (Hugging Face BertConfig hidden_dropout_prob / attention_probs_dropout_prob; BERT's
    # default for both is 0.1): after the embedding LayerNorm, on the attention probabilities, after the attention output projection and
    # after FC2.  The masks are a function of (dropout_seed, step, site, element) regenerated in the backward kernels (csrc/philox.h)
    text_hidden_dropout: float = 0.0
    text_attn_dropout: float = 0.0
    dropout_seed: int = 0
    # LoRA adapters on the text tower's attention projections (reference configs/model/med-moe.yaml:27-30 lora / lora_r / lora_alpha /
    # lora_dropout; peft's LoraConfig(target_modules=["query", "value"]) sketched in vision_encoder.py:30-36): the base tower stays frozen
    # (freeze_text = True), rank-r adapters A [r, D], B [D, r] on the chosen slices of the fused q / k / v projection train.
    # text_lora_dropout acts on the side path's input only, one mask per layer shared by its targets (site 4 * layer + 3 of csrc/philox.h)
    text_lora: bool = False
    text_lora_r: int = 8
    text_lora_alpha: float = 16.0
    text_lora_dropout: float = 0.0
    text_lora_targets: Tuple[str, ...] = ("query", "value")
    # frozen image tower and LoRA adapters on it (reference configs/model/med-moe.yaml:18-30 vision.freeze_cnn / lora / lora_r / lora_alpha /
    # lora_dropout, vision_encoder.py:20-36).  freeze_vit: the backbone - embeddings, blocks and the final LayerNorm - keeps no
    # gradient, Adam state, average or bf16 gradient copy and no per-step launch touches it; the router and the experts train.  vit_lora:
    # rank-r adapters on the chosen slices of every block's fused q / k / v projection train as well; it implies a frozen base, as peft's
    # get_peft_model does (`vit_frozen`).  vit_lora_dropout acts on the side path's input (the block's first LayerNorm output), one mask per
    # layer shared by its targets (site DROPOUT_SITE_VIT_LORA + layer of csrc/philox.h).  Fused step only
    freeze_vit: bool = False
    vit_lora: bool = False
    vit_lora_r: int = 8
    vit_lora_alpha: float = 16.0
    vit_lora_dropout: float = 0.0
    vit_lora_targets: Tuple[str, ...] = ("query", "value")
    # stochastic depth of the image tower (reference TransformerEncoder(drop_path_rate=), transformer.py:45-68, 188-192): in train mode
    # sample b skips the attention / the feed-forward branch of layer l with probability p_l = linspace(0, vit_drop_path, n_layer_v)[l], survivors
    # are scaled by 1 / (1 - p_l); the two branches draw independently.  The keep bits are a function of (dropout_seed, step, site, global sample)
    vit_drop_path: float = 0.0
    # activation recomputation of the image tower (open_clip's --grad-checkpointing).  "none": every layer keeps all its
    # activations for the backward (16 d_v bf16 per token and layer).  "selective": the layer input, qkv, the attention output and the
    # mid-block residual stay (6 d_v); both LayerNorm outputs come back from the saved statistics and FC1 is run again before the layer's
    # backward.  "full": only the layer input stays (1 d_v); the layer's forward up to FC1 is run again.  MEDMOE_VIT_CHECKPOINT=selective|full
    # switches it on too (vit_checkpoint_mode).  The text tower is not checkpointed
    vit_checkpoint: str = "none"
    # variable-length pass of the TRAINABLE text tower (full or LoRA): forward and backward run on the packed non-padding tokens,
    # as the frozen tower's forward does (same rule: B <= 1024 and T <= 80, else the padded pass).  Opt-in; MEDMOE_TEXT_TRAIN_VARLEN=1 switches
    # it on too.  Hidden / LoRA dropout masks are then functions of the PACKED (row, column); attention dropout has no packed kernels
    text_train_varlen: bool = False
    # deterministic mode (trainer.deterministic): no launch of a step whose result depends on the order in which workgroups or waves arrive -
    # staged or single-writer forms of every weight-gradient GEMM, LayerNorm / scale-attention parameter gradient and loss sum
    deterministic: bool = False
    # data parallelism: the number format of the gradient all-reduces.  "fp32": the flat fp32 gradient as it is.  "bf16": each arena is scaled
    # by 1 / world and rounded to bf16 on the chip, the bf16 copy is summed over the ranks, and the clip norm and Adam read it -
    # half the bytes on the wire.  Acts only where an all-reduce happens; a single process ignores it.  MEDMOE_GRAD_COMM=bf16 switches it on too.
    grad_comm_dtype: str = "fp32"
    # MoE (swin.py:82-92)
    n_expert: int = 4
    top_k: int = 1
    router_hidden: int = 128
    d_out: int = 768
    expert_fp8: bool = False      # BASELINE configs[4]: e4m3 expert weights (per-output-channel scales) on the fp8 MFMA
    expert_mx: bool = False       # MXFP8 expert weights (e4m3 + one E8M0 scale per 32 along the contraction) on the block-scaled MFMA
    # losses (med-moe_pretraining.yaml:20-41)
    temp1: float = 4.0
    temp2: float = 5.0
    temp3: float = 10.0
    w_local: float = 0.5
    w_global: float = 0.5
    w_cls: float = 2.0
    # Soft-GLoRIA (med-moe_pretraining.yaml:25-28; losses.py:814-883, 1111-1214): positives = captions whose frozen-BERT [CLS] cosine with the
    # row's caption exceeds threshold0, negatives = those at or below threshold1 (medmoe_module.py:258-281, 290-295)
    # data-parallel variant of the local loss (NOT the reference's behaviour, which keeps the local loss
    # rank-local): every rank scores its images against the captions of ALL ranks (words all-gathered: 15 MB per rank at batch 128), the
    # [B_g, B_g] similarity matrix is assembled by one more all-gather and both cross-entropies run over the global batch - the
    # W-rank step then equals the one-process step on the concatenated batch for the local loss too.  196 / 64 regions only.
    local_loss_global: bool = False
    soft_label: bool = False
    threshold0: float = 0.98
    threshold1: float = 0.97
    # optimiser (med-moe_pretraining.yaml:7-11, pretraining_medmoe.yaml:23)
    lr: float = 5e-5
    weight_decay: float = 0.0
    clip: float = 0.25
    # optimiser family and parameter groups (medmoe_amd/optim_groups.py; the defaults are the experiment's torch.optim.Adam, ungrouped):
    # "adamw" = decoupled weight decay; no_decay: fnmatch patterns over parameter names that get no decay; no_decay_1d: no decay for
    # biases, LayerNorms and the position / class / token-type / relative-position embeddings; text_lr_mult: learning-rate multiplier
    # of the trainable text tower; layer_decay: depth-wise learning-rate decay (BEiT convention), 1.0 = off
    optimizer: str = "adam"
    adam_betas: Tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8
    no_decay: Tuple[str, ...] = ()
    no_decay_1d: bool = False
    text_lr_mult: float = 1.0
    layer_decay: float = 1.0
    # optimizer = "lamb" (DESIGN 3s): Adam's moments (adam_betas / adam_eps), the decay inside the update and one trust ratio per parameter
    # tensor.  lamb_always_adapt: the ratio also for tensors without decay (apex use_nvlamb, timm always_adapt); lamb_trust_clip: min(ratio, 1)
    lamb_always_adapt: bool = False
    lamb_trust_clip: bool = False
    # exponential moving average of the weights (no reference counterpart): 0 = off.  Every arena the fused step steps keeps an fp32
    # average e <- e + (1 - d_t) (p - e), updated inside the Adam launch; d_t = ema_decay, or with ema_warmup min(ema_decay, (1 + t) / (10 + t))
    # at the t-th update.  Engine.ema_weights() / eval_step(ema=True) evaluate on it, checkpoints and exports carry it
    ema_decay: float = 0.0
    ema_warmup: bool = False
    # masked-language-model objective of the TRAINABLE text tower (reference losses.py:150-245, FLAVA's MaskedPredictionLoss): a
    # training step draws a BERT 80 / 10 / 10 mask over mlm_prob of the non-special tokens on the chip (stream: dropout_seed, the step), runs
    # the tower ONCE on the masked ids - the contrastive losses read that pass too - and adds mlm_weight * cross-entropy of the masked
    # positions under a head tied to the word-embedding table.  mlm_mask_id: the [MASK] id of the tokenizer (103 in BERT's vocabularies)
    text_mlm: bool = False
    mlm_prob: float = 0.15
    mlm_weight: float = 1.0
    mlm_mask_id: int = 103

    @property
    def vit_frozen(self) -> bool:
        """The engine's notion of a frozen image backbone: asked for, or implied by adapters on it."""
        return bool(self.freeze_vit or self.vit_lora)

    @property
    def n_patch(self) -> int:
        return (self.img_size // self.patch) ** 2

    @property
    def n_tok_v(self) -> int:
        return self.n_patch + 1

    @property
    def patch_dim(self) -> int:
        return 3 * self.patch * self.patch

    @property
    def patch_dim_pad(self) -> int:
        """im2col row pitch: the patch row padded to the GEMM k-step (patch 14: 588 -> 640); pad columns are zero."""
        return (self.patch_dim + 63) // 64 * 64

    def stage_layers(self) -> List[int]:
        L = self.n_layer_v
        return [max(1, (L * (s + 1)) // 4) for s in range(4)]

    def vit_drop_path_rates(self) -> List[float]:
        """torch.linspace(0, vit_drop_path, n_layer_v) as the reference computes it (fp32 values): one probability per layer."""
        import torch
        return [float(v) for v in torch.linspace(0, float(self.vit_drop_path), self.n_layer_v)]

    def vit_checkpoint_mode(self) -> str:
        """The recomputation mode an engine built from this config runs: MEDMOE_VIT_CHECKPOINT (none | selective | full) when set, else
        vit_checkpoint."""
        import os
        env = os.environ.get("MEDMOE_VIT_CHECKPOINT", "")
        if env not in ("",) + VIT_CHECKPOINT_MODES:
            raise ValueError(f"MEDMOE_VIT_CHECKPOINT must be one of {VIT_CHECKPOINT_MODES}, got {env!r}")
        return env or self.vit_checkpoint

    def validate(self):
        if not 0.0 <= float(self.vit_drop_path) < 1.0:
            raise ValueError(f"vit_drop_path must be in [0, 1), got {self.vit_drop_path}")
        if self.vit_checkpoint not in VIT_CHECKPOINT_MODES:
            raise ValueError(f"vit_checkpoint (model.model.vision.grad_checkpointing) must be one of {VIT_CHECKPOINT_MODES}, "
                             f"got {self.vit_checkpoint!r}")
        if self.grad_comm_dtype not in ("fp32", "bf16"):
            raise ValueError(f"grad_comm_dtype must be 'fp32' or 'bf16', got {self.grad_comm_dtype!r}")
        if not 0.0 <= float(self.ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1) (0 = off), got {self.ema_decay}")
        if self.optimizer not in ("adam", "adamw", "lamb"):
            raise ValueError(f"optimizer must be 'adam', 'adamw' or 'lamb', got {self.optimizer!r}")
        for key in ("lamb_always_adapt", "lamb_trust_clip"):
            if not isinstance(getattr(self, key), bool):
                raise ValueError(f"{key} must be a bool, got {getattr(self, key)!r}")
        if len(tuple(self.adam_betas)) != 2 or not all(0.0 <= float(b) < 1.0 for b in self.adam_betas):
            raise ValueError(f"adam_betas must be two values in [0, 1), got {self.adam_betas}")
        if not float(self.adam_eps) > 0.0:
            raise ValueError(f"adam_eps must be > 0, got {self.adam_eps}")
        for key in ("text_lr_mult", "layer_decay"):
            if not float(getattr(self, key)) > 0.0:
                raise ValueError(f"{key} must be > 0, got {getattr(self, key)}")
        if isinstance(self.no_decay, str) or not all(isinstance(p, str) for p in self.no_decay):
            raise ValueError(f"no_decay must be a list of name patterns, got {self.no_decay!r}")
        for key in ("text_hidden_dropout", "text_attn_dropout"):
            if not 0.0 <= float(getattr(self, key)) < 1.0:
                raise ValueError(f"{key} must be in [0, 1), got {getattr(self, key)}")
        if not 0.0 <= float(self.text_lora_dropout) < 1.0:
            raise ValueError(f"text_lora_dropout must be in [0, 1), got {self.text_lora_dropout}")
        if self.text_train_varlen and float(self.text_attn_dropout) > 0.0:
            raise NotImplementedError("text_train_varlen (text.train_varlen: true) with text_attn_dropout > 0 (text.attention_probs_dropout_prob): "
                                      "the attention-probability dropout kernels have no packed form yet - a named follow-up (DESIGN 3i); hidden "
                                      "and LoRA dropout are supported")
        if self.text_lora:
            if not self.freeze_text:
                raise ValueError("text_lora with freeze_text=False (text.freeze_bert: false): the adapters train on a FROZEN base tower - "
                                 "set freeze_text=True (or train the whole tower without adapters)")
            if not 1 <= int(self.text_lora_r) <= 16:
                raise ValueError(f"text_lora_r must be in 1..16 (the side path runs on the 16-wide MFMA), got {self.text_lora_r}")
            tg = (self.text_lora_targets,) if isinstance(self.text_lora_targets, str) else tuple(self.text_lora_targets)
            if not tg or len(set(tg)) != len(tg) or any(t not in ("query", "key", "value") for t in tg):
                raise ValueError(f"text_lora_targets must be a non-empty list of distinct names out of query / key / value, got {tg!r}")
            if not float(self.text_lora_alpha) > 0.0:
                raise ValueError(f"text_lora_alpha must be > 0, got {self.text_lora_alpha}")
            if self.deterministic:
                raise NotImplementedError("deterministic with text_lora (text.lora: true): the trainable text path (the local loss' word gradients, "
                                          "the text backward) has no deterministic form yet - a named follow-up (DESIGN 3e); the adapters' own "
                                          "weight gradients are summed in a fixed order already")
        if not 0.0 <= float(self.vit_lora_dropout) < 1.0:
            raise ValueError(f"vit_lora_dropout must be in [0, 1), got {self.vit_lora_dropout}")
        if self.vit_lora:
            if not 1 <= int(self.vit_lora_r) <= 16:
                raise ValueError(f"vit_lora_r must be in 1..16 (the side path runs on the 16-wide MFMA), got {self.vit_lora_r}")
            tg = (self.vit_lora_targets,) if isinstance(self.vit_lora_targets, str) else tuple(self.vit_lora_targets)
            if not tg or len(set(tg)) != len(tg) or any(t not in ("query", "key", "value") for t in tg):
                raise ValueError(f"vit_lora_targets must be a non-empty list of distinct names out of query / key / value, got {tg!r}")
            if not float(self.vit_lora_alpha) > 0.0:
                raise ValueError(f"vit_lora_alpha must be > 0, got {self.vit_lora_alpha}")
        if self.text_mlm:
            if self.freeze_text or self.text_lora:
                raise ValueError("text_mlm (model.mlm) with freeze_text=True (text.freeze_bert: true) or text_lora (text.lora: true): the decoder "
                                 "is tied to the word-embedding table, which must train - set freeze_text=False without adapters")
            if not 0.0 < float(self.mlm_prob) < 1.0:
                raise ValueError(f"mlm_prob (model.mlm.prob) must be in (0, 1), got {self.mlm_prob}")
            if not 0 <= int(self.mlm_mask_id) < self.vocab:
                raise ValueError(f"mlm_mask_id (model.mlm.mask_token_id) must be in [0, vocab = {self.vocab}), got {self.mlm_mask_id}")
            if not float(self.mlm_weight) > 0.0:
                raise ValueError(f"mlm_weight (model.mlm.weight) must be > 0, got {self.mlm_weight}")
            if self.deterministic:
                raise NotImplementedError("text_mlm with deterministic: the objective needs the trainable text tower, which has no "
                                          "deterministic form yet - a named follow-up (DESIGN 3e)")
        if self.expert_fp8 and self.expert_mx:
            raise ValueError("expert_fp8 and expert_mx are two formats of the same weights: set one")
        if self.expert_mx and (self.d_v % 32 or self.d_out % 64):
            raise ValueError("MXFP8 experts quantise in blocks of 32 along d_v, d_out and d_out/2")
        if self.d_v % self.n_head_v or self.d_v // self.n_head_v != 64:
            raise ValueError("image tower head_dim must be 64")
        if self.d_t % self.n_head_t or self.d_t // self.n_head_t != 64:
            raise ValueError("text tower head_dim must be 64")
        if self.d_t != self.d_out:
            raise ValueError("text width must equal the expert output width (no projection in the reference path)")
        for d in (self.d_v, self.ff_v, self.d_t, self.ff_t, self.d_out):
            if d % 64:
                raise ValueError(f"GEMM contraction dims must be multiples of 64, got {d}")
        if (self.d_out // 2) % 64:
            raise ValueError("expert attention hidden (d_out/2) must be a multiple of 64")
        if self.patch_dim % 4:
            raise ValueError("3*patch^2 must be a multiple of 4")
        if int(self.n_patch ** 0.5) ** 2 != self.n_patch:
            raise ValueError("patch grid must be square")


def config_by_name(name: str) -> MedMoEConfig:
    """BASELINE.json configs[0..2], the bf16 geometry of configs[4] (ViT-L/14, 16 experts) + unit-test scales."""
    if name == "cfg0":
        return MedMoEConfig(d_v=192, n_layer_v=12, n_head_v=3, ff_v=768, max_len=25, n_layer_t=2,
                            n_expert=2, top_k=1)
    if name == "cfg1":
        return MedMoEConfig(n_expert=4, top_k=1)
    if name == "cfg2":
        return MedMoEConfig(n_expert=8, top_k=2)
    if name == "cfg4":
        return MedMoEConfig(patch=14, d_v=1024, n_layer_v=24, n_head_v=16, ff_v=4096, n_expert=16, top_k=2, expert_fp8=True)
    if name == "cfg4_bf16":  # the same geometry with bf16 expert weights
        return MedMoEConfig(patch=14, d_v=1024, n_layer_v=24, n_head_v=16, ff_v=4096, n_expert=16, top_k=2)
    if name == "cfg4_mx":    # the same geometry with MXFP8 expert weights on the block-scaled MFMA
        return MedMoEConfig(patch=14, d_v=1024, n_layer_v=24, n_head_v=16, ff_v=4096, n_expert=16, top_k=2, expert_mx=True)
    if name == "tinyL8mx":   # tinyL with MXFP8 expert weights
        c = config_by_name("tinyL")
        c.expert_mx = True
        return c
    if name == "tinyL8":     # tinyL with fp8 expert weights (configs[4]'s expert arithmetic at unit-test width)
        c = config_by_name("tinyL")
        c.expert_fp8 = True
        return c
    if name == "tinyL":       # cfg4's geometry (patch 14 -> 256 regions, 257 tokens) at unit-test width
        return MedMoEConfig(img_size=224, patch=14, d_v=64, n_layer_v=4, n_head_v=1, ff_v=128, vocab=97,
                            max_len=40, d_t=128, n_layer_t=2, n_head_t=2, ff_t=256, n_expert=3, top_k=2,
                            d_out=128)
    if name == "tiny":
        return MedMoEConfig(img_size=64, patch=8, d_v=64, n_layer_v=4, n_head_v=1, ff_v=128, vocab=97,
                            max_len=16, d_t=128, n_layer_t=4, n_head_t=2, ff_t=256, n_expert=3, top_k=1,
                            d_out=128)
    if name == "tiny2":
        c = config_by_name("tiny")
        c.top_k = 2
        return c
    if name == "cfg3":       # BASELINE.json configs[3]: ViT-L/14 at 336 px (577 tokens, 576 regions), 8 experts top-2
        return MedMoEConfig(img_size=336, patch=14, d_v=1024, n_layer_v=24, n_head_v=16, ff_v=4096, n_expert=8, top_k=2)
    if name == "tinyL336":   # cfg3's token geometry (336 px / patch 14 -> 576 regions, 577 tokens) at unit-test width
        return MedMoEConfig(img_size=336, patch=14, d_v=64, n_layer_v=4, n_head_v=1, ff_v=128, vocab=97,
                     max_len=40, d_t=128, n_layer_t=2, n_head_t=2, ff_t=256, n_expert=3, top_k=2, d_out=128)
    if name == "tiny5":       # top-1 over five experts: the routing tests need >= 3 active experts AND an empty one
        c = config_by_name("tiny")
        c.n_expert = 5
        return c
    raise KeyError(name)
