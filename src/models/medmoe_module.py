"""Mirror of reference src/models/medmoe_module.py:172-339 (`MedMoEPretrainingLightningModule`):
same constructor arguments and `model_step` composition.  Lightning is optional in this image: with
`lightning` importable the class is a LightningModule, otherwise a plain nn.Module with the same
methods (so the parity test runs without it)."""
from typing import Any, Dict

import torch
import torch.nn.functional as F
from torch import nn

try:                                                     # pragma: no cover - not installed in this image
    from lightning import LightningModule as _Base
except Exception:                                        # noqa: BLE001
    _Base = nn.Module


def _get(cfg: Any, key: str, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


class MedMoEPretrainingLightningModule(_Base):
    def __init__(self, model: nn.Module, loss: Any, optimizer: Any = None, scheduler: Any = None,
                 compile: bool = False, num_classes: int = 5, fused_step: bool = False, optimizer_groups: Any = None,
                 grad_comm_dtype: str = "fp32", ema: Any = None, retrieval: Any = None, mlm: Any = None, grounding: Any = None):
        """`fused_step` (MI355X build, `model.fused_step` in the config tree): training steps run `Engine.train_step` - the hand-scheduled
        forward / losses / backward with the embedding all-gather, the reduce-scatter of the gathered-key gradients, the per-layer
        gradient all-reduce overlapped with backward and the fused clip + Adam - instead of torch autograd + a torch optimizer.
        Same losses, same update rule (tests/test_fused_module_gpu.py); needs the ViT image tower, the two GLoRIA losses (or their
        Soft variants) and torch.optim.Adam or torch.optim.AdamW in the config, and refuses anything else at construction.
        `optimizer_groups` (fused step only): the rule set of medmoe_amd.optim_groups - no_decay (name patterns), no_decay_1d,
        text_lr_mult, layer_decay - that cuts the engine's flat stores into parameter groups; the scheduler keeps driving the base
        learning rate, the groups multiply it.
        `grad_comm_dtype` (`model.grad_comm_dtype`, fused step only): "fp32" or "bf16" - the number format of the data-parallel gradient
        all-reduces (MedMoEConfig.grad_comm_dtype); a single process ignores it.
        `ema` (`+model.ema.decay=0.9999 +model.ema.warmup=true +model.ema.validate=true`, fused step only): an exponential moving average
        of every trained weight, kept in fp32 next to the master and updated inside the fused Adam launch (MedMoEConfig.ema_decay /
        ema_warmup); `validate`: validation_step / test_step evaluate on the average.  It travels with the checkpoint
        (`fused_ema`) and `ema_state_dict()` exports it under the reference's key names.
        `retrieval` (`+model.retrieval.ks=[1,5,10]`, fused step with the ViT towers only): validation / test epochs also report
        image <-> text retrieval over the whole evaluation set - val/i2t_R@k, val/t2i_R@k, mean and median ranks.  validation_step returns
        the same loss dict from the same Engine.eval_step call and adds the batch's global embeddings (already in the workspace: no second
        forward) to a medmoe_amd.retrieval.EmbeddingBank; `on_validation_epoch_start` resets the bank, `on_validation_epoch_end` scores it.
        `zero_shot` = path of a .pt holding prompt_ids / prompt_mask [C, Pn, T] and class_names: zero-shot accuracy (`zero_shot_ks`,
        default [1, 5]) of the images against the prompt-ensembled class embeddings, the true class read from batch[`label_key`]
        (default "label").  With model.ema.validate everything runs on the averaged weights.
        `local` (`+model.retrieval.local=true`, `local_k` 1..16, `local_agg` sum | mean): the epoch also keeps the batches' region
        and word features (medmoe_amd.retrieval.LocalBank) and reports val/i2t_local_R@k, val/t2i_local_* - every query's local_k best keys
        re-ranked with the weighted global + GLoRIA local similarity - and, with `zero_shot`, val/zs_local_acc@k.  Every key logged without
        it keeps its value.
        `mlm` (`+model.mlm.weight=1.0 +model.mlm.prob=0.15 +model.mlm.mask_token_id=103 +model.mlm.validate=true`, fused step with a
        trainable text tower - text.freeze_bert: false - and the ViT towers only): masked-token prediction as an auxiliary
        objective.  A training step masks `prob` of the caption tokens on the chip, runs the text tower once on the masked ids and adds
        `weight` x the cross-entropy of the masked positions under a head tied to the word embeddings (Engine.enable_mlm); the step reports
        mlm_loss / mlm_acc.  `validate`: validation_step / test_step add val/mlm_loss and val/mlm_acc under the fixed mask of step 0.  The
        head travels with the checkpoint (`mlm_head`, the reference's key names cls.dense.weight ... cls.bias) with its Adam state.
        `grounding` (`model.grounding`: mode attention | cosine, thetas, size, span_key, box_key; fused step with the ViT towers only; DESIGN
        3u): validation / test epochs also report phrase grounding - val/pg_acc, val/cnr_mean, val/ground_iou@<theta>.  The maps of a
        batch's (image, caption, batch[span_key]) pairs are formed from the features the validation forward left in the workspace
        (Engine.ground_workspace: no second forward) and scored against batch[box_key]; a medmoe_amd.ground.GroundBank keeps the epoch's
        sums on the device, ranks add theirs.  Every key logged without the block keeps its value."""
        super().__init__()
        self.model = model
        self.loss_cfg = loss
        self.local_loss = _get(loss, "local_loss")
        self.global_loss = _get(loss, "global_loss")
        self.local_loss_weight = _get(loss, "local_loss_weight", 0.4)          # medmoe_module.py:186-188
        self.global_loss_weight = _get(loss, "global_loss_weight", 0.4)
        self.classifier_loss_weight = _get(loss, "classifier_loss_weight", 0.2)
        self._optimizer, self._scheduler = optimizer, scheduler
        self.soft_label = bool(_get(loss, "soft_label", False))                 # :207-210: the reference loads `tool_bert` here
        self.fused_step = bool(fused_step)
        self._fused_acc, self._fused_clip, self._fused_opt = 1, None, None
        self._optimizer_groups = dict(optimizer_groups) if optimizer_groups else {}
        if self._optimizer_groups and not self.fused_step:
            raise NotImplementedError("optimizer_groups needs fused_step=true: the autograd path steps ONE flat parameter, which cannot be "
                                      "cut into groups (the fused step groups runs of the engine's flat stores)")
        from src.optim import Lamb
        if not self.fused_step and getattr(optimizer, "func", None) is Lamb:
            raise NotImplementedError("model.optimizer._target_ = src.optim.Lamb needs fused_step=true (model.fused_step=true): the autograd "
                                      "path steps ONE flat parameter, and a trust ratio over the whole model would be meaningless (the fused "
                                      "step keeps one ratio per parameter tensor of the engine's flat stores)")
        self._grad_comm_dtype = str(grad_comm_dtype)
        if self._grad_comm_dtype not in ("fp32", "bf16"):
            raise ValueError(f"grad_comm_dtype must be 'fp32' or 'bf16', got {grad_comm_dtype!r}")
        if self._grad_comm_dtype != "fp32" and not self.fused_step:
            raise NotImplementedError("grad_comm_dtype needs fused_step=true: the bf16 exchange packs the engine's flat gradient arenas, the "
                                      "autograd path all-reduces torch's own .grad tensors in fp32")
        unknown = set(dict(ema).keys()) - {"decay", "warmup", "validate"} if ema else set()
        if unknown:
            raise KeyError(f"model.ema: unknown keys {sorted(unknown)} (decay, warmup, validate)")
        self._ema_decay = float(_get(ema, "decay", 0.0)) if ema else 0.0
        self._ema_warmup = bool(_get(ema, "warmup", False)) if ema else False
        self._ema_validate = bool(_get(ema, "validate", False)) if ema else False
        if not 0.0 <= self._ema_decay < 1.0:
            raise ValueError(f"model.ema.decay must be in [0, 1) (0 = off), got {self._ema_decay}")
        if self._ema_decay > 0.0 and not self.fused_step:
            raise NotImplementedError("model.ema.decay > 0 needs fused_step=true (model.fused_step=true): the average is kept in the engine's "
                                      "flat stores and updated inside the fused Adam launch; the autograd path steps a torch optimizer")
        if self._ema_validate and not self._ema_decay > 0.0:
            raise ValueError("model.ema.validate=true needs model.ema.decay > 0: there is no average to validate on")
        self._mlm = None
        if mlm:
            unknown = set(dict(mlm).keys()) - {"weight", "prob", "mask_token_id", "validate"}
            if unknown:
                raise KeyError(f"model.mlm: unknown keys {sorted(unknown)} (weight, prob, mask_token_id, validate)")
            if not self.fused_step:
                raise NotImplementedError("model.mlm needs fused_step=true (model.fused_step=true): the mask, the head and the fused vocabulary "
                                          "loss run inside Engine.train_step")
            if getattr(self.model, "swin", None) is not None:
                raise NotImplementedError("model.mlm with vision.arch = swin_t: the objective is wired into the ViT Engine's training step "
                                          "(DESIGN 3r)")
            self._mlm = {"weight": float(_get(mlm, "weight", 1.0)), "prob": float(_get(mlm, "prob", 0.15)),
                         "mask_token_id": int(_get(mlm, "mask_token_id", 103)), "validate": bool(_get(mlm, "validate", False))}
        self._retrieval, self._bank, self._zs, self._class_emb = self._retrieval_block(retrieval), None, None, None
        self._lbank, self._class_words = None, None              # model.retrieval.local: the local features of the epoch, the prompts' words
        self._grounding, self._gbank = self._grounding_block(grounding), None
        if self.fused_step:
            self.automatic_optimization = False                                  # Lightning: manual optimisation (the engine steps itself)
            self._configure_engine()

    def _retrieval_block(self, retrieval: Any):
        """The validated `model.retrieval` block (None when absent)."""
        if retrieval is None:
            return None
        r = dict(retrieval)
        unknown = set(r) - {"ks", "zero_shot", "zero_shot_ks", "label_key", "local", "local_k", "local_agg"}
        if unknown:
            raise KeyError(f"model.retrieval: unknown keys {sorted(unknown)} (ks, zero_shot, zero_shot_ks, label_key, local, local_k, local_agg)")
        if not self.fused_step:
            raise NotImplementedError("model.retrieval needs fused_step=true (model.fused_step=true): the embeddings are read from the HIP "
                                      "engine's workspace after Engine.eval_step; the autograd path keeps none")
        if getattr(self.model, "swin", None) is not None:
            raise NotImplementedError("model.retrieval with vision.arch = swin_t: that model validates through model_step, not Engine.eval_step - "
                                      "retrieval metrics for the Swin engine are a named follow-up (DESIGN 3o)")
        ks = tuple(int(k) for k in r.get("ks", (1, 5, 10)))
        zks = tuple(int(k) for k in r.get("zero_shot_ks", (1, 5)))
        if not ks or min(ks) < 1 or min(zks or (1,)) < 1:
            raise ValueError(f"model.retrieval: ks / zero_shot_ks must hold integers >= 1, got {ks} / {zks}")
        blk = {"ks": ks, "zero_shot": r.get("zero_shot"), "zero_shot_ks": zks, "label_key": str(r.get("label_key", "label"))}
        local_k, local_agg = r.get("local_k", 16), str(r.get("local_agg", "sum"))
        if isinstance(local_k, bool) or int(local_k) != local_k or not 1 <= int(local_k) <= 16:
            raise ValueError(f"model.retrieval.local_k must be an integer in 1 .. 16 (the depth of sim_topk), got {local_k!r}")
        if local_agg not in ("sum", "mean"):
            raise ValueError(f"model.retrieval.local_agg must be 'sum' or 'mean', got {local_agg!r}")
        if bool(r.get("local", False)):
            if max(ks) > int(local_k):
                raise ValueError(f"model.retrieval: ks = {ks} with local=true needs local_k >= {max(ks)}, got {int(local_k)} (at most 16: a target "
                                 "outside its candidate list keeps its global rank; deeper lists are a named follow-up, DESIGN 3q)")
            cfg = getattr(getattr(self.model, "engine", None), "cfg", None)
            if cfg is not None:
                from medmoe_amd import ops
                if not ops.local_pair3_supported(cfg.n_patch, cfg.max_len) or cfg.d_out % 64:
                    raise NotImplementedError(f"model.retrieval.local with {cfg.n_patch} regions x {cfg.max_len} words at width {cfg.d_out}: the "
                                              "listed-pair kernel covers 196 regions (up to 80 words) and 64 regions (up to 16); the 256 / 576 "
                                              "regions of cfg4 / cfg3 are a named follow-up (DESIGN 3q)")
            blk.update({"local": True, "local_k": int(local_k), "local_agg": local_agg})     # absent without local: the block of DESIGN 3o as it was
        return blk

    def _grounding_block(self, grounding: Any):
        """The validated `model.grounding` block (None when absent)."""
        if grounding is None:
            return None
        r = dict(grounding)
        valid = ("mode", "thetas", "size", "span_key", "box_key")
        unknown = set(r) - set(valid)
        if unknown:
            raise KeyError(f"model.grounding: unknown keys {sorted(unknown)} ({', '.join(valid)})")
        if not self.fused_step:
            raise NotImplementedError("model.grounding needs fused_step=true (model.fused_step=true): the region and word features are read "
                                      "from the HIP engine's workspace after Engine.eval_step; the autograd path keeps none")
        if getattr(self.model, "swin", None) is not None:
            raise NotImplementedError("model.grounding with vision.arch = swin_t: that model validates through model_step, not Engine.eval_step - "
                                      "maps for the Swin engine are a named follow-up (DESIGN 3u)")
        from medmoe_amd import ops
        mode = str(r.get("mode", "attention"))
        if mode not in ops.GROUND_MODES:
            raise ValueError(f"model.grounding.mode must be one of {sorted(ops.GROUND_MODES)}, got {mode!r}")
        thetas = r.get("thetas", (0.5,))
        thetas = tuple(float(t) for t in ((thetas,) if isinstance(thetas, (int, float)) else thetas))
        if not 1 <= len(thetas) <= ops.GROUND_MAX_THETAS:
            raise ValueError(f"model.grounding.thetas must hold 1 .. {ops.GROUND_MAX_THETAS} thresholds, got {thetas}")
        size = r.get("size")
        if size is not None:
            size = (int(size), int(size)) if isinstance(size, (int, float)) else tuple(int(v) for v in size)
            if len(size) != 2 or min(size) < 1:
                raise ValueError(f"model.grounding.size must be a side or (H, W), got {r.get('size')!r}")
        cfg = getattr(getattr(self.model, "engine", None), "cfg", None)
        if cfg is not None and cfg.d_t != cfg.d_out:
            raise NotImplementedError(f"model.grounding: word features of width d_t = {cfg.d_t} against regions of d_out = {cfg.d_out}")
        return {"mode": mode, "thetas": thetas, "size": size, "span_key": str(r.get("span_key", "span")), "box_key": str(r.get("box_key", "box"))}

    def forward(self, batch):
        return self.model(batch)

    def _calc_global_loss(self, img_emb_g, text_emb_g, idx=None, probs=None):           # :212-218
        return self.global_loss(img_emb_g, text_emb_g, temp3=_get(self.loss_cfg, "temp3", 4.0), idx=idx, probs=probs)

    def _calc_local_loss(self, img_emb_l, text_emb_l, sents, idx=None, probs=None):     # :220-233
        cap_lens = [len([w for w in sent if not w.startswith("[")]) + 1 for sent in sents]
        out = self.local_loss(img_emb_l, text_emb_l, cap_lens, temp1=_get(self.loss_cfg, "temp1", 4.0),
                              temp2=_get(self.loss_cfg, "temp2", 5.0), temp3=_get(self.loss_cfg, "temp3", 10.0),
                              idx=idx, probs=probs)
        return out.loss0 + out.loss1

    def _calc_classifier_loss(self, router_logits, labels):                             # :235-237
        return F.cross_entropy(router_logits, labels)

    def _calc_classifier_acc(self, router_logits, labels):                              # :239-241
        return (torch.argmax(router_logits, dim=1) == labels).float().mean()

    def get_text_soft_target(self, raw_txt, topK, threshold):                            # :258-281
        """(caption-to-caption scores [B, B], thresholds).  The reference runs a second frozen pretrained BertModel over `raw_txt`; with
        the text tower frozen that is the tower's own BERT, so the scores come from the text pass `forward` just ran
        (`Engine.text_soft_target`: [CLS] of the last layer, L2-normalised, pairwise products); `raw_txt` / `topK` are unused, as in
        the reference (its top-k filter is commented out, :278-280)."""
        with torch.no_grad():
            return self.model.text_soft_target(), threshold

    def model_step(self, batch: Dict[str, Any]):                                         # :284-316
        img_emb_g, img_emb_l, text_emb_g, text_emb_l, sents, router_logits = self.forward(batch)
        if self.soft_label:                                                              # :291-296
            idx, filt = self.get_text_soft_target(batch["caption"], _get(self.loss_cfg, "topk", 5),
                                                  (_get(self.loss_cfg, "threshold0", 0.98), _get(self.loss_cfg, "threshold1", 0.97)))
            l_loss = self._calc_local_loss(img_emb_l, text_emb_l, sents, idx, filt)
            g_loss = self._calc_global_loss(img_emb_g, text_emb_g, idx, filt)
        else:
            l_loss = self._calc_local_loss(img_emb_l, text_emb_l, sents)
            g_loss = self._calc_global_loss(img_emb_g, text_emb_g)
        classifier_loss = self._calc_classifier_loss(router_logits, batch["label"])
        classifier_acc = self._calc_classifier_acc(router_logits, batch["label"])
        loss = self.local_loss_weight * l_loss + self.global_loss_weight * g_loss + self.classifier_loss_weight * classifier_loss
        return {"loss": loss, "l_loss": l_loss, "g_loss": g_loss, "classifier_loss": classifier_loss,
                "classifier_acc": classifier_acc}

    def training_step(self, batch, batch_idx: int = 0):                                  # :318-339
        if self.fused_step:
            acc = self._fused_acc
            return self.fused_training_step(batch, optimizer_step=(batch_idx + 1) % acc == 0, zero_grad=batch_idx % acc == 0,
                                            loss_scale=1.0 / acc)["loss"]
        return self.model_step(batch)["loss"]

    # ---- fused mode --------------------------------------------------------------------------------------------------
    def _configure_engine(self):
        """Carry the module's loss / optimiser configuration into the engine's (medmoe_amd.config.MedMoEConfig); refuse what the fused
        step does not compute."""
        import functools

        import src.losses as L
        eng = getattr(self.model, "engine", None)
        if eng is None:
            raise NotImplementedError("fused_step needs the HIP engine behind self.model (src.models.components.med_moe.MedMoE)")
        # arch = swin_t (the reference's own encoder): medmoe_amd.swin_engine.SwinEngine, built on the first step (the encoder's arenas exist
        # once the module sits on the GPU); the ViT towers: Engine.train_step
        self._swin_engine = None
        soft = (type(self.global_loss) is L.SoftGLORIAGlobalContrastiveLoss, type(self.local_loss) is L.SoftGLORIALocalContrastiveLoss)
        hard = (type(self.global_loss) is L.GLORIAGlobalContrastiveLoss, type(self.local_loss) is L.GLORIALocalContrastiveLoss)
        if not (all(hard) or all(soft)) or all(soft) != self.soft_label:
            raise NotImplementedError("fused_step computes GLORIA{Global,Local}ContrastiveLoss (or both Soft variants with loss.soft_label: true); "
                                      f"got {type(self.global_loss).__name__} / {type(self.local_loss).__name__}, soft_label={self.soft_label}")
        if _get(self.loss_cfg, "agg", "sum") != "sum":
            raise NotImplementedError("fused_step: only loss.agg = 'sum' (the reference default)")
        from src.optim import Lamb
        opt = self._optimizer
        lamb = isinstance(opt, functools.partial) and opt.func is Lamb
        if not isinstance(opt, functools.partial) or opt.func not in (torch.optim.Adam, torch.optim.AdamW, Lamb) or opt.args \
                or set(opt.keywords) - ({"lr", "weight_decay", "betas", "eps"} | ({"always_adapt", "trust_clip"} if lamb else set())):
            raise NotImplementedError("fused_step fuses torch.optim.Adam or torch.optim.AdamW (lr, weight_decay, betas, eps; the experiment's "
                                      "optimizer is Adam, med-moe_pretraining.yaml:7-11) or src.optim.Lamb (the same keywords, always_adapt, "
                                      "trust_clip); no other optimizer and no other keyword")
        c = eng.cfg
        c.temp1, c.temp2 = float(_get(self.loss_cfg, "temp1", 4.0)), float(_get(self.loss_cfg, "temp2", 5.0))
        c.temp3 = float(_get(self.loss_cfg, "temp3", 10.0))
        c.w_local, c.w_global, c.w_cls = float(self.local_loss_weight), float(self.global_loss_weight), float(self.classifier_loss_weight)
        c.soft_label = self.soft_label
        c.local_loss_global = bool(_get(self.loss_cfg, "local_loss_global", False))
        c.threshold0, c.threshold1 = float(_get(self.loss_cfg, "threshold0", 0.98)), float(_get(self.loss_cfg, "threshold1", 0.97))
        adamw = opt.func is torch.optim.AdamW
        c.lr = float(opt.keywords.get("lr", 1e-3))
        c.weight_decay = float(opt.keywords.get("weight_decay", 1e-2 if adamw or lamb else 0.0))      # the classes' own defaults
        c.optimizer = "lamb" if lamb else "adamw" if adamw else "adam"
        c.adam_betas = tuple(float(b) for b in opt.keywords.get("betas", (0.9, 0.999)))
        c.adam_eps = float(opt.keywords.get("eps", 1e-6 if lamb else 1e-8))
        c.lamb_always_adapt = bool(opt.keywords.get("always_adapt", False)) if lamb else False
        c.lamb_trust_clip = bool(opt.keywords.get("trust_clip", False)) if lamb else False
        c.grad_comm_dtype = self._grad_comm_dtype
        c.ema_decay, c.ema_warmup = self._ema_decay, self._ema_warmup
        c.validate()
        if self._mlm is not None:                                    # refuses a frozen tower, adapters, a bad probability or [MASK] id
            eng.enable_mlm(self._mlm["prob"], self._mlm["weight"], self._mlm["mask_token_id"])
        if self._ema_validate and getattr(self.model, "swin", None) is not None:
            raise NotImplementedError("model.ema.validate=true with vision.arch = swin_t: this model validates through its torch modules, "
                                      "which read the masters - evaluation on the averaged weights is a named follow-up (DESIGN 3k); the "
                                      "average itself is maintained, checkpointed and exportable")
        from medmoe_amd.optim_groups import set_rules
        set_rules(c, self._optimizer_groups)                         # validates the rule set and the optimiser keys above
        if getattr(self.model, "swin", None) is None:                # arch = swin_t: the SwinEngine groups its own arenas when it is built
            eng.apply_optimizer_groups()
            if c.ema_decay > 0.0:                                    # (and its stores start their averages at the first step)
                from medmoe_amd import ema as ema_
                ema_.prepare(eng.optimizer_stores().values())

    def set_deterministic(self, flag: bool):
        """trainer.deterministic: hand the flag to the HIP engine behind self.model (medmoe_amd.Engine.set_deterministic - every launch of
        a step in its staged / single-writer form); the engine refuses the configurations the mode is not built for."""
        flag = bool(flag)
        eng = getattr(self.model, "engine", None)
        if eng is None:
            if flag:
                raise NotImplementedError("trainer.deterministic=true needs the HIP engine behind self.model")
            return
        if flag and getattr(self.model, "swin", None) is not None:
            raise NotImplementedError("deterministic with the Swin-T encoder (vision.arch = swin_t, SwinEngine): the relative-position bias "
                                      "tables' gradients are summed by index_add_")
        eng.set_deterministic(flag)

    def configure_fused(self, accumulate_grad_batches: int = 1, gradient_clip_val=None):
        """The trainer's two keys the fused step has to honour itself (trainer.accumulate_grad_batches, trainer.gradient_clip_val;
        pretraining_medmoe.yaml:23-24).  gradient_clip_val None / 0 = no clipping."""
        self._fused_acc = max(1, int(accumulate_grad_batches))
        self._fused_clip = float(gradient_clip_val) if gradient_clip_val else None
        self.model.engine.cfg.clip = self._fused_clip if self._fused_clip is not None else 0.0

    def _fused_engine(self):
        """The engine a fused step runs on: the SwinEngine around the reference's encoder (arch = swin_t) or the ViT Engine, its working
        copies and learning rate brought up to date."""
        m = self.model
        if getattr(m, "swin", None) is not None:
            from medmoe_amd.swin_engine import SwinEngine
            enc = m.swin._encoder()                                  # (re)builds the arenas / refreshes the bf16 copies after an external edit
            if self._swin_engine is None or self._swin_engine.enc is not enc:
                self._swin_engine = SwinEngine(m.engine, enc, drop_path_rate=m.swin.drop_path_rate)
            eng = self._swin_engine
            eng.training = self.training
        else:
            m.refresh_working_copies()                               # a load_state_dict / external edit of the flat parameter since the last step
            eng = m.engine
        if self._fused_opt is not None:                              # the scheduler acts on this optimizer's lr; the engine applies it
            eng.cfg.lr = float(self._fused_opt.param_groups[0]["lr"])
        return eng

    @staticmethod
    def _engine_batch(batch: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        """The module's batch (image, caption = dict(ids, attn_mask[, token_type]) or an ids tensor, label) as the engine takes it."""
        cap = batch["caption"]
        if isinstance(cap, dict):
            ids, mask, tt = cap["ids"], cap["attn_mask"], cap.get("token_type")
        elif torch.is_tensor(cap):
            ids, mask, tt = cap, (cap != 0).long(), None
        else:
            raise NotImplementedError("fused_step takes pre-tokenised captions (dict(ids, attn_mask) or an ids tensor)")
        eb = {"image": batch["image"].contiguous(), "ids": ids, "attn_mask": mask, "label": batch["label"]}
        if tt is not None:
            eb["token_type"] = tt
        return eb

    def fused_training_step(self, batch: Dict[str, Any], optimizer_step: bool = True, zero_grad: bool = True, loss_scale: float = 1.0):
        """One micro-batch through Engine.train_step; returns the reference's loss names (device scalars)."""
        if not self.fused_step:
            raise RuntimeError("fused_training_step: construct the module with fused_step=True (model.fused_step=true)")
        eng, eb = self._fused_engine(), self._engine_batch(batch)
        out = eng.train_step(eb, optimizer=optimizer_step, zero_grad=zero_grad, loss_scale=loss_scale)
        res = {"loss": out["loss"], "l_loss": out["l_loss"], "g_loss": out["g_loss"], "classifier_loss": out["classifier_loss"],
               "classifier_acc": out["classifier_acc"]}
        if "mlm_loss" in out:                                        # model.mlm
            res["mlm_loss"], res["mlm_acc"] = out["mlm_loss"], out["mlm_acc"]
        return res

    def fused_eval_step(self, batch: Dict[str, Any]):
        """One batch through Engine.eval_step - the losses of `fused_training_step` forward only, nothing of the model or the optimiser
        state written; returns the reference's loss names (device scalars); with model.ema.validate on the averaged weights
        (eval_step(ema=True)).  With vision.arch = swin_t the batch takes the `model_step`
        route under no_grad: a SwinEngine.eval_step is a separate piece of work."""
        if not self.fused_step:
            raise RuntimeError("fused_eval_step: construct the module with fused_step=True (model.fused_step=true)")
        if getattr(self.model, "swin", None) is not None:
            with torch.no_grad():
                return self.model_step(batch)
        eng, eb = self._fused_engine(), self._engine_batch(batch)
        out = eng.eval_step(eb, ema=True) if self._ema_validate else eng.eval_step(eb)
        if self._grounding is not None:                              # on the features this forward left, before anything overwrites them
            self._ground_add(eng, batch)
        res = {"loss": out["loss"], "l_loss": out["l_loss"], "g_loss": out["g_loss"], "classifier_loss": out["classifier_loss"],
               "classifier_acc": out["classifier_acc"]}
        if self._mlm is not None and self._mlm["validate"]:          # val/mlm_loss, val/mlm_acc under the fixed mask of step 0
            res.update(eng.mlm_eval(eb, step=0, ema=self._ema_validate))
        return res

    def validation_step(self, batch, batch_idx: int = 0):                                # :114-125
        """The loss dict of a validation batch (`val/loss` is its "loss"): Engine.eval_step in fused mode, `model_step` otherwise."""
        if self.fused_step:
            out = self.fused_eval_step(batch)
            if self._retrieval is not None:
                self._bank_add(batch)
            return out
        return self.model_step(batch)

    def test_step(self, batch, batch_idx: int = 0):                                      # :127-134
        return self.validation_step(batch, batch_idx)

    # ---- phrase grounding of an evaluation epoch (model.grounding) -----------------------------------------------------------
    def _ground_add(self, eng, batch: Dict[str, Any]):
        from medmoe_amd.ground import GroundBank
        g = self._grounding
        if self._gbank is None:
            self._gbank = GroundBank(g["thetas"], eng.device)
        rec = eng.ground_workspace(batch, mode=g["mode"], thetas=g["thetas"], size=g["size"], span_key=g["span_key"], box_key=g["box_key"])
        self._gbank.add(rec)

    def _ground_metrics(self) -> Dict[str, float]:
        """pg_acc, cnr_mean and ground_iou@<theta> of the epoch; under data parallelism the ranks' sums are added first."""
        if self._grounding is None or self._gbank is None or len(self._gbank) == 0:
            return {}
        from medmoe_amd.ground import grounding_metrics, theta_key
        import torch.distributed as tdist
        if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            tdist.all_reduce(self._gbank.ints)
            tdist.all_reduce(self._gbank.sums)
        met = grounding_metrics(self._gbank)
        out = {"pg_acc": met["pg_acc"], "cnr_mean": met["cnr_mean"]}
        out.update({f"ground_iou@{theta_key(t)}": met[f"iou@{theta_key(t)}"] for t in self._gbank.thetas})
        return out

    # ---- retrieval / zero-shot metrics of an evaluation epoch (model.retrieval) ----------------------------------------------
    def _bank_add(self, batch: Dict[str, Any]):
        """The global embeddings Engine.eval_step has just left in the workspace (on the averaged weights under model.ema.validate) go
        into the bank, normalised, with the batch's labels."""
        from medmoe_amd.retrieval import EmbeddingBank
        eng = self.model.engine
        if self._bank is None:
            self._bank = EmbeddingBank(eng.cfg.d_out, eng.device)
        lab = batch.get(self._retrieval["label_key"]) if isinstance(batch, dict) else None
        self._bank.add(eng.ws["img_g"], eng.ws["txt_g"], lab if torch.is_tensor(lab) else None)
        if self._retrieval.get("local"):
            if self._lbank is None:
                from medmoe_amd.retrieval import LocalBank
                self._lbank = LocalBank.for_engine(eng)
            self._lbank.add(eng)

    def on_validation_epoch_start(self):
        """Empty the bank; with model.retrieval.zero_shot, embed the class prompts under the weights this epoch validates on."""
        if self._gbank is not None:
            self._gbank.reset()
        if self._retrieval is None:
            return
        if self._bank is not None:
            self._bank.reset()
        if self._lbank is not None:
            self._lbank.reset()
        path = self._retrieval["zero_shot"]
        if path:
            from medmoe_amd.retrieval import class_embeddings
            if self._zs is None:
                self._zs = torch.load(str(path), map_location="cpu", weights_only=True)
                missing = {"prompt_ids", "prompt_mask", "class_names"} - set(self._zs)
                if missing:
                    raise KeyError(f"model.retrieval.zero_shot: {path} lacks {sorted(missing)}")
            eng = self._fused_engine()
            self._class_emb = class_embeddings(eng, self._zs["prompt_ids"].to(eng.device), self._zs["prompt_mask"].to(eng.device),
                                               ema=self._ema_validate)
            if self._retrieval.get("local"):
                from medmoe_amd.retrieval import class_prompt_words
                self._class_words = class_prompt_words(eng, self._zs["prompt_ids"].to(eng.device), self._zs["prompt_mask"].to(eng.device),
                                                       ema=self._ema_validate)

    def on_validation_epoch_end(self):
        """The epoch's retrieval (and zero-shot) metrics as plain floats; the trainer files them under val/... or test/...."""
        ground = self._ground_metrics()
        if self._retrieval is None or self._bank is None:
            return ground or None
        from medmoe_amd.retrieval import retrieval_metrics, zero_shot_metrics
        loc = dict(local=self._lbank, local_k=self._retrieval["local_k"], local_agg=self._retrieval["local_agg"]) if self._lbank is not None else {}
        out = {k: float(v) for k, v in retrieval_metrics(self._bank, self._retrieval["ks"], **loc).items()}
        if self._class_emb is not None:
            zloc = dict(local=(self._lbank,) + tuple(self._class_words), local_agg=self._retrieval["local_agg"]) if self._class_words is not None else {}
            zs = zero_shot_metrics(self._bank, self._class_emb, ks=self._retrieval["zero_shot_ks"], **zloc)
            names = list(self._zs["class_names"])
            for k, v in zs.items():
                if torch.is_tensor(v):
                    out.update({f"{k}/{names[c]}": float(x) for c, x in enumerate(v.tolist())})
                else:
                    out[k] = float(v)
        out.update(ground)
        return out

    def on_test_epoch_start(self):
        return self.on_validation_epoch_start()

    def on_test_epoch_end(self):
        return self.on_validation_epoch_end()

    # ---- fused mode: the optimiser state lives in the engine's flat stores, not in a torch optimizer -----------------------------------
    def _fused_stores(self) -> Dict[str, Any]:
        """name -> flat store (`medmoe_amd.flat.FlatArena`) holding Adam's state of the fused step."""
        m = self.model
        if getattr(m, "swin", None) is not None:
            enc = m.swin._encoder()
            out = {"swin_tower": enc.tower.store, "swin_moe": enc.store}
            if m.engine.text_arena() is not None:                    # text.freeze_bert: false / text.lora: true - the text arena's Adam state travels too
                out["text"] = m.engine.text_arena()
            return out
        out = {"image": m.engine.params}
        if m.engine.text_arena() is not None:
            out["text"] = m.engine.text_arena()
        if m.engine.vlora is not None:                               # vision.lora_vit: true - the image adapters' Adam state and average travel too
            out["vit_lora"] = m.engine.vlora
        if getattr(m.engine, "mlm", None) is not None:               # model.mlm: the head's arena
            out["mlm"] = m.engine.mlm.store
        return out

    def on_save_checkpoint(self, checkpoint: Dict[str, Any]) -> None:
        """Lightning hook (the stand-in trainer calls it too): Adam's moments and step counts of the fused step travel with the checkpoint
        (`fused_adam`: per store `exp_avg` / `exp_avg_sq` in the store's flat layout + `step`), what `optimizer_states` holds for the
        torch-optimizer path, so that `fit(ckpt_path=...)` resumes the SAME optimisation."""
        if not self.fused_step:
            return
        state = {}
        for name, st in self._fused_stores().items():
            if not st.has_adam_state():
                continue                                             # no optimiser step taken yet
            m, v = st.adam_state()
            state[name] = {"step": int(st.step_count), "numel": int(m.numel()), "exp_avg": m.detach().cpu().clone(),
                           "exp_avg_sq": v.detach().cpu().clone()}
        checkpoint["fused_adam"] = state
        # the weight averages (model.ema): per store that keeps one, the flat fp32 average in the store's layout + the number of
        # updates it has seen.  One that has seen none is the master by definition (medmoe_amd.ema.prepare): saved as such
        averaged = {name: st for name, st in self._fused_stores().items() if getattr(st, "e32", None) is not None}
        if averaged:
            checkpoint["fused_ema"] = {name: {"updates": int(st.ema_updates), "numel": int(st.e32.numel()),
                                              "ema": (st.e32 if st.ema_updates else st.p32[st.train_from:]).detach().cpu().clone()} for name, st in averaged.items()}
        # the text tower's dropout masks are a function of (seed, step, site, element): the step counter resumes where it stopped
        checkpoint["text_dropout_step"] = int(self.model.engine.dropout_step)
        # model.mlm: the head is no torch module - its masters travel here under the reference's names (cls.dense.weight ... cls.bias)
        if getattr(self.model.engine, "mlm", None) is not None:
            from medmoe_amd.mlm import HEAD_PREFIX
            checkpoint["mlm_head"] = {k[len(HEAD_PREFIX):]: v for k, v in self.model.engine.mlm.store.export_named().items()}

    def on_load_checkpoint(self, checkpoint: Dict[str, Any]) -> None:
        if self.fused_step and "text_dropout_step" in checkpoint:
            self.model.engine.dropout_step = int(checkpoint["text_dropout_step"])
        if not self.fused_step:
            return
        if "mlm_head" in checkpoint and getattr(self.model.engine, "mlm", None) is not None:
            from medmoe_amd.mlm import HEAD_PREFIX
            self.model.engine.mlm.store.load_named({HEAD_PREFIX + k: v for k, v in checkpoint["mlm_head"].items()})
        stores = self._fused_stores()
        for name, rec in (checkpoint.get("fused_adam") or {}).items():
            if name not in stores:
                raise KeyError(f"checkpoint holds fused Adam state for {name!r}; this module has {sorted(stores)}")
            st = stores[name]
            m, v = st.adam_state()
            if int(rec["numel"]) != m.numel():
                raise ValueError(f"fused Adam state {name!r}: {rec['numel']} elements in the checkpoint, {m.numel()} in this model")
            m.copy_(rec["exp_avg"]); v.copy_(rec["exp_avg_sq"])
            st.step_count = int(rec["step"])
        if getattr(self, "_ema_decay", 0.0) > 0.0:                   # a module without the key ignores a checkpoint's averages
            self._load_fused_ema(checkpoint.get("fused_ema") or {}, stores)

    def _load_fused_ema(self, state: Dict[str, Any], stores: Dict[str, Any]) -> None:
        """The averages of a checkpoint into the stores.  A store the checkpoint holds no average for (one written with EMA off) starts
        again from its master - the one the checkpoint's state dict has just loaded - with no update counted."""
        for name in state:
            if name not in stores:
                raise KeyError(f"checkpoint holds a weight average for {name!r}; this module has {sorted(stores)}")
        for name, st in stores.items():
            st.enable_ema()
            rec = state.get(name)
            if rec is None:
                continue
            if int(rec["numel"]) != st.e32.numel():
                raise ValueError(f"fused weight average {name!r}: {rec['numel']} elements in the checkpoint, {st.e32.numel()} in this model")
            st.e32.copy_(rec["ema"])
            st.ema_updates = int(rec["updates"])

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """`self.model.state_dict()` with every trained weight replaced by its average: the reference's key names, through the key mapping
        of the model's own state-dict hook (MedMoE.ema_state_dict)."""
        if not self._ema_decay > 0.0:
            raise RuntimeError("ema_state_dict: model.ema.decay is 0 - this module keeps no average")
        return self.model.ema_state_dict()

    def configure_optimizers(self):                                                      # :148-169
        opt = self._optimizer(params=self.parameters())
        if self.fused_step:
            self._fused_opt = opt                                    # never stepped: it carries lr for the scheduler / checkpoints
        if self._scheduler is None:
            return {"optimizer": opt}
        return {"optimizer": opt, "lr_scheduler": {"scheduler": self._scheduler(optimizer=opt), "monitor": "val/loss",
                                                   "interval": "epoch", "frequency": 1}}
