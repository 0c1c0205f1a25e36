"""Mirror of reference src/models/components/med_moe.py:21-108: `MedMoE(vision, text, lora)` with
`encode_image`, `encode_text`, `forward(batch) -> (img_emb_g, img_emb_l, text_emb_g, text_emb_l,
sents, router_probs)`, running on the MI355X engine (medmoe_amd).

Differences forced by the environment (documented in DESIGN.md): images arrive as a normalised
[B,3,H,W] tensor (PIL + AutoImageProcessor are a "next" row) and captions as pre-tokenised ids
(`batch['caption']` = dict(ids, attn_mask[, token_type]) or an ids tensor; the HF tokenizer hookup
is a "next" row).  All parameters of the image tower + MoE are ONE flat `nn.Parameter` (the engine's
fp32 master buffer), so any torch optimizer / Lightning sees and updates them.  The GEMMs read bf16
working copies of that buffer: `encode_image` refreshes them whenever the parameter's version counter
moved (an optimizer step, `load_state_dict`, any in-place edit) or the module was moved / re-typed, so
an external optimizer trains every weight (`Engine.train_step` fuses clip + Adam + the refresh itself).
"""
from typing import Any, Dict

import torch
from torch import nn

from medmoe_amd.config import MedMoEConfig, config_by_name
from medmoe_amd.engine import Engine


def _get(cfg: Any, key: str, default=None):
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default) if not hasattr(cfg, "get") else cfg.get(key, default)


_ARCH = {"vit_ti16": dict(d_v=192, n_layer_v=12, n_head_v=3, ff_v=768), "vit_b16": dict(),
         "vit_l14": dict(patch=14, d_v=1024, n_layer_v=24, n_head_v=16, ff_v=4096),
         "vit_l14_336": dict(img_size=336, patch=14, d_v=1024, n_layer_v=24, n_head_v=16, ff_v=4096),
         # the reference's own tower (swin.py:119-149, model_name 'swin'): Swin-T + pyramid experts on src.models.components.swin.SWIN behind torch
         # autograd; the engine then only hosts the (frozen) text tower - its ViT is a one-layer ViT-Ti placeholder that is never run
         "swin_t": dict(d_v=192, n_layer_v=1, n_head_v=3, ff_v=768),
         }          # unit-test geometries: `vision.config_name: tiny` (medmoe_amd.config.config_by_name)

# reference keys (configs/model/med-moe.yaml:18-44) whose other values select code outside the hot path: rejected loudly
_FIXED = {"vision": {"use_moe": True, "projection": False, "lora": False},
          "text": {"aggregate_method": "sum", "agg_tokens": True, "norm": False, "projection": False}}


def config_from_hydra(vision: Any, text: Any) -> MedMoEConfig:
    """Extends the reference keys (configs/model/med-moe.yaml:18-44) with arch / num_experts / top_k / expert_dtype (vision)
    and n_layer (text); `config_name` picks a named geometry of medmoe_amd.config outright."""
    for side, cfg_ in (("vision", vision), ("text", text)):
        for k, want in _FIXED[side].items():
            got = _get(cfg_, k, want)
            if got != want:
                raise NotImplementedError(f"model.model.{side}.{k}={got!r}: only {want!r} is on the pretraining_medmoe hot path")
    name = _get(vision, "config_name")
    if name:
        c = config_by_name(name)
        c.freeze_text = bool(_get(text, "freeze_bert", True))
        return _text_dropout(_vit_drop_path(c, vision), text)
    c = MedMoEConfig(**_ARCH[_get(vision, "arch", "vit_b16")])
    c.n_expert = int(_get(vision, "num_experts", 6))          # swin.py:83 default K=6 modalities
    c.top_k = int(_get(vision, "top_k", 1))
    c.d_out = int(_get(vision, "embed_dim", c.d_out))
    c.max_len = int(_get(text, "max_length", 25))             # med-moe.yaml:40
    c.n_layer_t = int(_get(text, "n_layer", 12))
    c.last_n_layers = int(_get(text, "last_n_layers", 4))
    c.d_t = int(_get(text, "embed_dim", c.d_t))
    c.freeze_text = bool(_get(text, "freeze_bert", True))     # false: the text tower trains too (text_encoder.py:27-30) - fused step only
    dt = str(_get(vision, "expert_dtype", "bf16"))
    if dt not in ("bf16", "fp8", "mxfp8"):
        raise NotImplementedError(f"vision.expert_dtype={dt!r}: bf16, fp8 (e4m3 expert weights, per-row / per-channel scales, BASELINE configs[4]) "
                                  f"or mxfp8 (e4m3 with one power-of-two scale per block of 32, the block-scaled MFMA)")
    c.expert_fp8 = dt == "fp8"
    c.expert_mx = dt == "mxfp8"
    return _text_dropout(_vit_drop_path(c, vision), text)


def _vit_drop_path(c: MedMoEConfig, vision: Any) -> MedMoEConfig:
    """model.model.vision.drop_path_rate: stochastic depth of the ViT tower (the reference's TransformerEncoder(drop_path_rate=)).
    Absent: 0.0, nothing changes.  With arch: swin_t the same key sets the Swin tower's rate instead (MedMoE.__init__): the engine's ViT is a
    placeholder there."""
    if _get(vision, "arch", "vit_b16") != "swin_t" or _get(vision, "config_name"):
        c.vit_drop_path = float(_get(vision, "drop_path_rate", 0.0))
    return _vit_checkpoint(c, vision)


def _vit_checkpoint(c: MedMoEConfig, vision: Any) -> MedMoEConfig:
    """model.model.vision.grad_checkpointing: activation recomputation of the ViT tower (open_clip's --grad-checkpointing).
    false / absent: none, nothing changes; true: full; "selective" / "full" / "none" by name."""
    key = _get(vision, "grad_checkpointing", False)
    mode = "none" if key is None or key is False else "full" if key is True else str(key)
    if mode != "none" and _get(vision, "arch", "vit_b16") == "swin_t" and not _get(vision, "config_name"):
        raise NotImplementedError(f"vit_checkpoint={mode!r} (model.model.vision.grad_checkpointing) with vision.arch=swin_t: the recomputation "
                                  "is built for the engine's ViT tower; the Swin tower runs behind torch autograd and is not covered")
    c.vit_checkpoint = mode
    return _vit_lora(c, vision)


def _vit_lora(c: MedMoEConfig, vision: Any) -> MedMoEConfig:
    """model.model.vision.freeze_cnn (the reference's key, med-moe.yaml:50): the ViT backbone is frozen.  model.model.vision.lora_vit: LoRA
    adapters on the ViT tower's attention projections, parameters from the reference's own lora_r / lora_alpha / lora_dropout (yaml default
    0.1: counts only with lora_vit) plus lora_targets.  `vision.lora` itself stays rejected (_FIXED): it names peft on the
    reference's Swin tower.  Absent keys change nothing.  With arch: swin_t both are refused: the Swin tower runs behind torch autograd."""
    freeze, lora = bool(_get(vision, "freeze_cnn", False)), bool(_get(vision, "lora_vit", False))
    if (freeze or lora) and _get(vision, "arch", "vit_b16") == "swin_t" and not _get(vision, "config_name"):
        raise NotImplementedError(f"model.model.vision.{'lora_vit' if lora else 'freeze_cnn'}=true with vision.arch=swin_t: the frozen backbone "
                                  "and its adapters are built for the engine's ViT tower (DESIGN 3n); adapters on the Swin tower are out of scope")
    c.freeze_vit, c.vit_lora = freeze, lora
    if lora:
        c.vit_lora_r = int(_get(vision, "lora_r", c.vit_lora_r))
        c.vit_lora_alpha = float(_get(vision, "lora_alpha", c.vit_lora_alpha))
        c.vit_lora_dropout = float(_get(vision, "lora_dropout", 0.0))
        tg = _get(vision, "lora_targets", None)
        if tg is not None:
            c.vit_lora_targets = (tg,) if isinstance(tg, str) else tuple(str(t) for t in tg)
    return c


def _text_dropout(c: MedMoEConfig, text: Any) -> MedMoEConfig:
    """Hugging Face's BertConfig names (both 0.1 there; 0.0 here unless set): train-mode dropout of a trainable text tower."""
    c.text_hidden_dropout = float(_get(text, "hidden_dropout_prob", 0.0))
    c.text_attn_dropout = float(_get(text, "attention_probs_dropout_prob", 0.0))
    c.dropout_seed = int(_get(text, "dropout_seed", 0))
    return _text_lora(c, text)


def _text_lora(c: MedMoEConfig, text: Any) -> MedMoEConfig:
    """model.model.text.lora / lora_r / lora_alpha / lora_dropout / lora_targets (the reference's names, med-moe.yaml:27-30, on the text tower:
    peft-style adapters on the attention projections of a frozen BERT).  Absent keys leave the defaults: no adapters.
    model.model.text.train_varlen: the trainable tower's (full or LoRA) pass on the packed non-padding tokens."""
    c.text_lora = bool(_get(text, "lora", False))
    c.text_lora_r = int(_get(text, "lora_r", c.text_lora_r))
    c.text_lora_alpha = float(_get(text, "lora_alpha", c.text_lora_alpha))
    c.text_lora_dropout = float(_get(text, "lora_dropout", 0.0))
    tg = _get(text, "lora_targets", None)
    if tg is not None:
        c.text_lora_targets = (tg,) if isinstance(tg, str) else tuple(str(t) for t in tg)
    c.text_train_varlen = bool(_get(text, "train_varlen", False))
    return c


class _ImageTowerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights: torch.Tensor, images: torch.Tensor, engine: Engine):
        engine.forward_image(images)
        ctx.engine = engine
        ws = engine.ws
        return ws["img_g"].clone(), ws["img_l"].float(), ws["probs"].clone()

    @staticmethod
    def backward(ctx, d_img_g, d_img_l, d_probs):
        eng = ctx.engine
        ws = eng.ws
        ws["d_img_g"].copy_(d_img_g if d_img_g is not None else torch.zeros_like(ws["d_img_g"]))
        ws["d_img_l"].copy_(d_img_l if d_img_l is not None else torch.zeros_like(ws["d_img_l"]))
        eng.params.zero_grad()
        ws["loss_parts"].zero_()
        eng.backward(None, dprobs_ext=d_probs.float().contiguous() if d_probs is not None else None)
        return eng.params.g32.clone(), None, None


class MedMoE(nn.Module):
    def __init__(self, vision: Any, text: Any, lora: bool = False) -> None:
        super().__init__()
        if lora:
            raise NotImplementedError("lora: true is not on the pretraining_medmoe path (med-moe.yaml:27)")
        self.text, self.vision = text, vision
        self.cfg = config_from_hydra(vision, text)
        self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        if self.device is None:
            raise RuntimeError("MedMoE (MI355X build) needs a GPU: there is no CPU fallback")
        self.engine = Engine(self.cfg, self.device)
        self.swin = None
        if _get(vision, "arch", "vit_b16") == "swin_t" and not _get(vision, "config_name"):
            from .swin import SWIN
            self.swin = SWIN(num_experts=self.cfg.n_expert, state_dict=_get(vision, "state_dict")).to(self.device)
            rate = _get(vision, "drop_path_rate")                   # absent: SwinConfig.drop_path_rate of the checkpoint's config (0.1)
            if rate is not None:
                if not 0.0 <= float(rate) < 1.0:
                    raise ValueError(f"model.model.vision.drop_path_rate must be in [0, 1), got {rate}")
                self.swin.drop_path_rate = float(rate)
        self.weights = nn.Parameter(self.engine.params.p32, requires_grad=self.swin is None)          # flat fp32 master, shared storage
        self._synced_version = self.weights._version                 # bf16 working copies are current for this version
        # medmoe_module.py:196 calls .image_encoder.train(), :208 reads .text_encoder.tokenizer: both towers live in this
        # one object.  Plain attributes, NOT registered submodules (a module that contains itself would recurse in
        # state_dict() / named_modules()).
        object.__setattr__(self, "image_encoder", self)
        object.__setattr__(self, "text_encoder", self)
        self.idxtoword = None                                        # set_vocabulary(): tokenizer vocabulary hookup
        self.tokenizer = None
        # checkpoints carry the reference's key layout (`image_encoder.moe.experts.{e}.proj_convs.{s}.0.weight`, `image_encoder.moe.router.*`,
        # swin.py:83-92 under med_moe.py:32; `image_encoder.model.*` for the Swin tower, `image_encoder.vit.*` for the ViT one;
        # `text_encoder.*` for the frozen text tower) instead of the flat buffer's private layout
        self._register_state_dict_hook(MedMoE._to_reference_keys)
        self._register_load_state_dict_pre_hook(self._from_reference_keys)

    @staticmethod
    def _to_reference_keys(module, state_dict, prefix, local_metadata):
        flat = state_dict.pop(prefix + "weights", None)
        if module.swin is None:
            if flat is not None:
                for k, v in module.engine.params.named_views(flat.detach()).items():
                    state_dict[prefix + "image_encoder." + k] = v
        else:
            for k in [k for k in state_dict if k.startswith(prefix + "swin.")]:
                state_dict[prefix + "image_encoder." + k[len(prefix + "swin."):]] = state_dict.pop(k)
        for k, v in module.engine.params.text.items():
            state_dict[prefix + "text_encoder." + k] = v
        if module.engine.lora is not None:                           # text.lora: true - the adapters in peft's shapes ([r, D] / [D, r])
            lo = module.engine.lora
            for n in lo.true_names():
                state_dict[prefix + "text_encoder." + n + ".weight"] = lo.true_view(lo.p32, n)
        if module.engine.vlora is not None:                          # vision.lora_vit: true - the same convention under the image encoder's prefix
            lo = module.engine.vlora
            for n in lo.true_names():
                state_dict[prefix + "image_encoder." + lo.prefix + n + ".weight"] = lo.true_view(lo.p32, n)
        return state_dict

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """state_dict() with the weights the fused step trains replaced by their fp32 averages (cfg.ema_decay > 0), under the
        same reference keys: `image_encoder.*` from the image arena's average, `text_encoder.*` from the trainable text tower's or the
        adapters'.  Clones: the dict stays what it was when the training goes on."""
        from medmoe_amd import ema as ema_
        eng = self.engine
        if not eng.cfg.ema_decay > 0.0:
            raise RuntimeError("ema_state_dict: cfg.ema_decay is 0 (model.ema.decay) - this model keeps no average")
        if self.swin is not None:
            raise NotImplementedError("ema_state_dict with vision.arch = swin_t: the Swin stores' averages are exported under the stores' own "
                                      "names (SwinEngine.ema_params); the mapping to the module's keys is a named follow-up (DESIGN 3k)")
        ema_.prepare(eng.optimizer_stores().values())
        out = {k: v.detach().clone() for k, v in self.state_dict().items()}
        p = eng.params
        for k, v in p.named_views(p.e32).items():
            out["image_encoder." + k] = v.detach().clone()
        if eng.tstore is not None:
            for n in eng.tstore.shapes:
                out["text_encoder." + n] = eng.tstore.view(eng.tstore.e32, n).detach().clone()
        if eng.lora is not None:
            for n in eng.lora.true_names():
                out["text_encoder." + n + ".weight"] = eng.lora.true_view(eng.lora.e32, n).detach().clone()
        if eng.vlora is not None:
            for n in eng.vlora.true_names():
                out["image_encoder." + eng.vlora.prefix + n + ".weight"] = eng.vlora.true_view(eng.vlora.e32, n).detach().clone()
        return out

    def _from_reference_keys(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        ie, te = prefix + "image_encoder.", prefix + "text_encoder."
        named = {k[len(ie):]: state_dict.pop(k) for k in [k for k in state_dict if k.startswith(ie)]}
        text = {"text." + k[len(te):]: state_dict.pop(k) for k in [k for k in state_dict if k.startswith(te)]}
        p = self.engine.params
        if self.swin is not None:
            for k, v in named.items():
                state_dict[prefix + "swin." + k] = v
            named = {}
        if named or text:
            if p.p32.data_ptr() != self.weights.data_ptr():
                self.refresh_working_copies()                        # re-attach the engine to the parameter's storage first
            if named and self.engine.vlora is not None:           # vision.lora_vit: true - the adapters into their arena, the rest into the tower
                lora = {k: named.pop(k) for k in [k for k in named if ".lora_" in k]}
                if lora:
                    self.engine.vlora.load_named(lora)
            if named:
                want = set(p.named_views())
                got = set(named)
                if strict and want - got:
                    error_msgs.append(f"MedMoE: checkpoint lacks image-encoder keys {sorted(want - got)[:3]} ... ({len(want - got)} names)")
                    return
                unexpected_keys.extend(ie + k for k in sorted(got - want))
                views = p.named_views()
                for k in want & got:
                    views[k].copy_(named[k].to(views[k].device, views[k].dtype).reshape(views[k].shape))
            if text and self.engine.lora is not None:             # text.lora: true - adapters into their arena, the rest into the frozen base
                lora = {k: text.pop(k) for k in [k for k in text if ".lora_" in k]}
                if lora:
                    self.engine.lora.load_named(lora)
            if text:
                if self.engine.tstore is not None:                # trainable text tower: into its flat master buffer
                    self.engine.tstore.load_named(text)
                else:
                    p.load_named_text(text)
            p.refresh()
        # the flat parameter itself: legacy checkpoints hold it under `weights`; otherwise present the (just updated) buffer so that the
        # default loader finds its key
        if prefix + "weights" not in state_dict:
            state_dict[prefix + "weights"] = self.weights.detach().clone()

    def set_vocabulary(self, idxtoword, tokenizer=None):
        """Hook a tokenizer vocabulary up (text_encoder.py:23 idxtoword): the on-device word-piece aggregation then merges
        its '##' pieces and `sents` holds the real merged words.  `tokenizer`: optional callable
        (list[str], max_length) -> dict(ids, attn_mask[, token_type]) for raw caption strings (med_moe.py:72-85)."""
        from medmoe_amd.text import vocab_tables
        self.idxtoword = idxtoword
        self.tokenizer = tokenizer
        self.engine.vocab = vocab_tables(idxtoword, self.device)

    def refresh_working_copies(self):
        """fp32 master -> bf16 working copies (and their transposes) when the master changed since the last refresh."""
        p = self.engine.params
        w = self.weights
        if w.data_ptr() != p.p32.data_ptr():
            # the module was moved / cast (`.to()`, `.cuda()`): re-attach the engine to the parameter's new storage
            if w.dtype != torch.float32 or w.device != p.p32.device or w.numel() != p.numel:
                raise RuntimeError("MedMoE.weights must stay a flat fp32 tensor on the engine's GPU")
            p.p32 = w.data
            self._synced_version = -1
        if w._version != self._synced_version:
            p.refresh()
            self._synced_version = w._version

    def encode_image(self, images: torch.Tensor):
        """med_moe.py:67-70 -> (img_feat_g [B,D], local_feats [B,D,H,W], router_probs [B,E])."""
        if self.swin is not None:                                    # (global [B,768], local [B,768,56,56], router probabilities), swin.py:149
            self.engine._alloc(images.shape[0])                      # the text pass' buffers
            return self.swin(images)
        if self.cfg.vit_drop_path > 0.0 and self.training and torch.is_grad_enabled():
            raise NotImplementedError("vit_drop_path > 0 (model.model.vision.drop_path_rate) trains through the fused step (model.fused_step=true "
                                      "-> Engine.train_step draws the stochastic-depth masks and scales the branch gradients); the torch-autograd "
                                      "mirror runs the tower without drops, which is right for evaluation only")
        if self.cfg.vit_frozen and torch.is_grad_enabled():
            raise NotImplementedError("vision.freeze_cnn / vision.lora_vit: true train through the fused step (model.fused_step: true -> "
                                      "Engine.train_step skips the frozen backbone's gradients and has the adapters' backward); the "
                                      "torch-autograd mirror hands the whole flat parameter a gradient, which a frozen backbone does not keep")
        self.refresh_working_copies()
        img_g, img_l, probs = _ImageTowerFn.apply(self.weights, images.contiguous(), self.engine)
        B, P, D = img_l.shape
        h = int(P ** 0.5)
        return img_g, img_l.transpose(1, 2).reshape(B, D, h, h), probs

    def encode_text(self, texts: Any):
        """med_moe.py:72-100 -> (text_emb_l [B,D,T], text_emb_g [B,D], sents)."""
        if isinstance(texts, dict):
            ids, mask, tt = texts["ids"], texts["attn_mask"], texts.get("token_type")
        elif torch.is_tensor(texts):
            ids, mask, tt = texts, (texts != 0).long(), None
        elif self.tokenizer is not None:
            tok = self.tokenizer(list(texts), self.cfg.max_len)
            ids, mask, tt = tok["ids"].to(self.device), tok["attn_mask"].to(self.device), tok.get("token_type")
        else:
            raise NotImplementedError("raw caption strings need a tokenizer: set_vocabulary(idxtoword, tokenizer) or pass token ids")
        if self.cfg.text_lora and torch.is_grad_enabled():
            raise NotImplementedError("text.lora: true trains through the fused step (model.fused_step: true -> Engine.train_step has the adapters' "
                                      "backward); the torch-autograd mirror keeps the text tower frozen")
        if not self.cfg.freeze_text and torch.is_grad_enabled():
            raise NotImplementedError("text.freeze_bert: false trains through the fused step (model.fused_step: true -> Engine.train_step has the "
                                      "text backward); the torch-autograd mirror keeps the text tower frozen")
        with torch.no_grad():                                        # freeze_bert: true (med-moe.yaml:35)
            self.engine.forward_text(ids, mask, tt)
        ws = self.engine.ws
        cap = self.engine.cap_lens.tolist()                          # the reference contract hands host lists around
        T = ids.shape[1]
        if self.idxtoword is not None:
            from medmoe_amd.text import merge_sents
            sents = merge_sents(ids.cpu(), self.idxtoword)
        else:
            sents = [["w"] * (c - 1) + ["[SEP]"] + ["[PAD]"] * (T - c) for c in cap]
        return ws["words32"].transpose(1, 2).clone(), ws["txt_g"].clone(), sents

    def text_soft_target(self) -> torch.Tensor:
        """fp32 [B, B] caption-to-caption scores for the Soft-GLoRIA losses (medmoe_module.py:258-281), from the text pass just run."""
        return self.engine.text_soft_target()

    def forward(self, batch: Dict[str, Any]):
        images, text = batch["image"], batch["caption"]
        # the engine's text pass needs the image pass' batch allocation: run the image tower first
        img_emb_g, img_emb_l, router_logits = self.encode_image(images)
        text_emb_l, text_emb_g, sents = self.encode_text(text)
        return img_emb_g, img_emb_l, text_emb_g, text_emb_l, sents, router_logits
