"""Parameter storage for the MedMoE hot path on one MI355X.

Trainable (image tower + MoE) parameters live in ONE flat arena (`flat.FlatArena`: fp32 master with
matching flat fp32 grad / Adam-m / Adam-v buffers - a single fused clip+Adam launch, a single RCCL
all-reduce - plus a flat bf16 working copy in the reference's nn.Linear [out,in] layout and a
second bf16 buffer holding every GEMM weight TRANSPOSED ([in,out]) so dgrad is the same NT MFMA
kernel as the forward).  Expert weights are stacked [E, ...] for the grouped GEMMs.  This class holds
what is specific to the tower: the spec list (its order IS the layout), the seeded init, the 8-bit
expert copies and the reference-style names.

Names follow the reference modules (transformer.py / multi_head_attention.py / mlp.py /
swin.py) so state_dicts map 1:1; `load_named` / `export_named` translate the per-expert
reference names (moe.experts.{e}.proj_convs.{s}.0.weight ...) to the stacked storage.
The text tower is frozen (configs/model/med-moe.yaml:35) and kept separately.
"""
from typing import Dict, List, Tuple

import torch

from . import ops
from .config import MedMoEConfig
from .flat import FlatArena


class ParamStore(FlatArena):
    def __init__(self, cfg: MedMoEConfig, device, seed: int = 0, std: float = 0.02):
        cfg.validate()
        self.cfg = cfg
        self.specs: List[Tuple[str, Tuple[int, ...], str]] = []   # (name, shape, kind) kind: w|wt|v
        c = cfg
        pp = c.patch_dim_pad           # padded to the GEMM k-step; the pad columns stay zero (zero im2col columns -> zero grads)
        E, Do, Dh, Dv = c.n_expert, c.d_out, c.d_out // 2, c.d_v

        def add(name, shape, kind):
            self.specs.append((name, tuple(shape), kind))

        add("vit.patch_embed.weight", (Dv, pp), "w")
        add("vit.patch_embed.bias", (Dv,), "v")
        add("vit.cls_token", (Dv,), "v")
        add("vit.pos_embed", (c.n_tok_v, Dv), "v")
        for i in range(c.n_layer_v):
            b = f"vit.layer.{i}"
            add(b + ".attention_layernorm.weight", (Dv,), "v"); add(b + ".attention_layernorm.bias", (Dv,), "v")
            add(b + ".attention.input_proj.weight", (3 * Dv, Dv), "wt"); add(b + ".attention.input_proj.bias", (3 * Dv,), "v")
            add(b + ".attention.output_proj.weight", (Dv, Dv), "wt"); add(b + ".attention.output_proj.bias", (Dv,), "v")
            add(b + ".feedforward_layernorm.weight", (Dv,), "v"); add(b + ".feedforward_layernorm.bias", (Dv,), "v")
            add(b + ".feedforward.model.0.weight", (c.ff_v, Dv), "wt"); add(b + ".feedforward.model.0.bias", (c.ff_v,), "v")
            add(b + ".feedforward.model.2.weight", (Dv, c.ff_v), "wt"); add(b + ".feedforward.model.2.bias", (Dv,), "v")
        add("vit.final_layer_norm.weight", (Dv,), "v"); add("vit.final_layer_norm.bias", (Dv,), "v")
        add("moe.router.0.weight", (c.router_hidden, Dv), "v"); add("moe.router.0.bias", (c.router_hidden,), "v")
        add("moe.router.2.weight", (E, c.router_hidden), "v"); add("moe.router.2.bias", (E,), "v")
        for s in range(4):
            add(f"moe.proj.{s}.weight", (E, Do, Dv), "wt"); add(f"moe.proj.{s}.bias", (E, Do), "v")
        add("moe.attn0.weight", (E, Dh, Do), "wt"); add("moe.attn0.bias", (E, Dh), "v")
        add("moe.attn2.weight", (E, Dh), "v"); add("moe.attn2.bias", (E,), "v")

        self.kinds = {n: k for n, _, k in self.specs}
        # transpose table: one entry per 2-D matrix (per expert for stacked weights)
        # cfg.freeze_vit / cfg.vit_lora: the backbone - everything stored before the router, the final LayerNorm included, as
        # under peft - is frozen: no gradient, Adam state, average or bf16 gradient copy over it, and no per-step launch touches it
        super().__init__(device, [(n, s) for n, s, _ in self.specs], gemm=[(n, len(s) == 3) for n, s, k in self.specs if k == "wt"],
                         train_from="moe.router.0.weight" if cfg.vit_frozen else None)
        self.adam_state()
        dev = self.device
        # fp8 expert weights (BASELINE configs[4]): e4m3 copies [E,N,K] + transposes [E,K,N] + per-output-channel scales [E,N] of
        # the five expert projections, re-derived from the fp32 master after every update (requantise_experts)
        self.fp8: Dict[str, Tuple[torch.Tensor, ...]] = {}
        if cfg.expert_fp8:
            for name in [f"moe.proj.{s_}.weight" for s_ in range(4)] + ["moe.attn0.weight"]:
                Eg, N, K = self.shapes[name]
                self.fp8[name] = (torch.empty(Eg, N, K, device=dev, dtype=torch.uint8), torch.empty(Eg, K, N, device=dev, dtype=torch.uint8),
                                  torch.empty(Eg, N, device=dev, dtype=torch.float32))
        # MXFP8 expert weights (cfg.expert_mx; the same dict: it holds the 8-bit working copies of whichever format is on, and whoever
        # saves / restores the parameter state walks it): per projection (q [E,N,K], scale bytes [E,N,K/32]) for the forward and,
        # quantised again with blocks along N, (qT [E,K,N], scale bytes [E,K,N/32]) for dgrad
        if cfg.expert_mx:
            for name in [f"moe.proj.{s_}.weight" for s_ in range(4)] + ["moe.attn0.weight"]:
                Eg, N, K = self.shapes[name]
                self.fp8[name] = (torch.empty(Eg, N, K, device=dev, dtype=torch.uint8), torch.empty(Eg, N, K // 32, device=dev, dtype=torch.uint8),
                                  torch.empty(Eg, K, N, device=dev, dtype=torch.uint8), torch.empty(Eg, K, N // 32, device=dev, dtype=torch.uint8))
        self._init_random(seed, std)
        # ---- frozen text tower ----
        self.text: Dict[str, torch.Tensor] = {}
        self._init_text(seed + 1, std)

    # -- init / sync ---------------------------------------------------------------------------
    def _init_random(self, seed, std):
        g = torch.Generator(device="cpu").manual_seed(seed)
        for name, shape, kind in self.specs:
            if name.endswith("layernorm.weight") or name.endswith("layer_norm.weight"):
                val = torch.ones(shape)
            elif name.endswith(".bias"):
                val = torch.zeros(shape)
            elif name == "vit.patch_embed.weight":
                val = self._pad_patch(torch.randn(shape[0], self.cfg.patch_dim, generator=g) * std)
            else:
                val = torch.randn(shape, generator=g) * std     # init rule multimodal_transformer.py:298-312
            self.f32(name).copy_(val.to(self.device))
        self.refresh()

    def _init_text(self, seed, std):
        c, dev = self.cfg, self.device
        g = torch.Generator(device="cpu").manual_seed(seed)
        t = self.text

        def rn(*shape):
            return (torch.randn(*shape, generator=g) * std).to(dev)
        t["word_embeddings"] = rn(c.vocab, c.d_t)
        t["word_embeddings"][0].zero_()
        t["position_embeddings"] = rn(c.max_len, c.d_t)
        t["token_type_embeddings"] = rn(2, c.d_t)
        t["emb_layernorm.weight"] = torch.ones(c.d_t, device=dev); t["emb_layernorm.bias"] = torch.zeros(c.d_t, device=dev)
        for i in range(c.n_layer_t):
            b = f"layer.{i}"
            for nm, (o, k) in (("attention.input_proj", (3 * c.d_t, c.d_t)), ("attention.output_proj", (c.d_t, c.d_t)),
                               ("feedforward.model.0", (c.ff_t, c.d_t)), ("feedforward.model.2", (c.d_t, c.ff_t))):
                t[f"{b}.{nm}.weight"] = rn(o, k).to(torch.bfloat16)
                t[f"{b}.{nm}.bias"] = torch.zeros(o, device=dev)
            for nm in ("attention_layernorm", "feedforward_layernorm"):
                t[f"{b}.{nm}.weight"] = torch.ones(c.d_t, device=dev); t[f"{b}.{nm}.bias"] = torch.zeros(c.d_t, device=dev)

    def _pad_patch(self, w):
        c = self.cfg
        w = w.reshape(c.d_v, c.patch_dim)
        if c.patch_dim_pad == c.patch_dim:
            return w
        return torch.cat([w, w.new_zeros(c.d_v, c.patch_dim_pad - c.patch_dim)], 1)

    def after_update(self, src=None):
        self.requantise_experts(src)

    def requantise_experts(self, src=None):
        """The 8-bit expert copies from the fp32 master (after every refresh() / adam_step(): FlatArena's hook) - or from `src`, the flat fp32
        buffer of this layout the working copies were just cast from (load_ema(): the average)."""
        for name, copies in self.fp8.items():
            Eg, N, K = self.shapes[name]
            w = self.f32(name) if src is None else self.view(src, name)
            if self.cfg.expert_mx:
                q, sq, qT, sT = copies
                ops.call("quant_weights_mx", w, q, sq, qT, sT, Eg, N, K)
            else:
                q, qT, s = copies
                ops.call("quant_weights_e4m3", w, q, qT, s, Eg, N, K)

    def q8(self, name): return self.fp8[name][0]
    def q8t(self, name): return self.fp8[name][1]
    def s8(self, name): return self.fp8[name][2]
    def qmx(self, name): return self.fp8[name][0], self.fp8[name][1]      # MXFP8 forward copy + scale bytes: blocks along K
    def qmxt(self, name): return self.fp8[name][2], self.fp8[name][3]     # MXFP8 dgrad copy + scale bytes: blocks along N

    # -- reference-style names ------------------------------------------------------------------
    def load_named(self, named: Dict[str, torch.Tensor]):
        """Load a reference-style name->tensor dict (e.g. oracle.init_params / a state_dict)."""
        c = self.cfg
        dev = self.device
        used = set()
        for name in self.shapes:
            if name.startswith("moe.proj.") or name.startswith("moe.attn0") or name.startswith("moe.attn2"):
                continue
            if name in named:
                v = named[name].to(dev)
                if name == "vit.patch_embed.weight":
                    v = self._pad_patch(v)
                self.f32(name).copy_(v.reshape(self.shapes[name])); used.add(name)
        for e in range(c.n_expert):
            for s in range(4):
                w = named[f"moe.experts.{e}.proj_convs.{s}.0.weight"].to(dev)
                self.f32(f"moe.proj.{s}.weight")[e].copy_(w.reshape(c.d_out, c.d_v))
                self.f32(f"moe.proj.{s}.bias")[e].copy_(named[f"moe.experts.{e}.proj_convs.{s}.0.bias"].to(dev))
            self.f32("moe.attn0.weight")[e].copy_(named[f"moe.experts.{e}.attn_proj.0.weight"].to(dev))
            self.f32("moe.attn0.bias")[e].copy_(named[f"moe.experts.{e}.attn_proj.0.bias"].to(dev))
            self.f32("moe.attn2.weight")[e].copy_(named[f"moe.experts.{e}.attn_proj.2.weight"].to(dev).reshape(-1))
            self.f32("moe.attn2.bias")[e].copy_(named[f"moe.experts.{e}.attn_proj.2.bias"].to(dev).reshape(()))
        self.load_named_text(named)
        self.refresh()

    def load_named_text(self, named: Dict[str, torch.Tensor]):
        """`text.<name>` entries of a reference-style dict into the frozen text tower (in place: views handed out earlier stay valid)."""
        for k, v in named.items():
            if k.startswith("text."):
                kk = k[len("text."):]
                if kk not in self.text:
                    raise KeyError(f"unknown text parameter {k}")
                if tuple(v.shape) != tuple(self.text[kk].shape):
                    raise ValueError(f"{k}: shape {tuple(v.shape)} != {tuple(self.text[kk].shape)}")
                self.text[kk] = v.to(self.device).to(self.text[kk].dtype).contiguous()

    def named_views(self, flat=None) -> Dict[str, torch.Tensor]:
        """Reference-style names -> VIEWS of the flat buffer on the device (flat = p32 for weights, g32 for grads): the per-expert
        names of swin.py:12-30 are slices of the stacked [E, ...] storage; the patch-embedding weight loses its k-step padding."""
        flat = self.p32 if flat is None else flat
        c = self.cfg
        out = {}
        tail = self.train_from and flat.numel() == self.n_train      # a gradient / moment / average buffer of a frozen backbone: the tail's names
        for name in self.shapes:
            if tail and self.is_frozen(name):
                continue
            v = self.view(flat, name)
            if name.startswith("moe.proj."):
                s = int(name.split(".")[2]); leaf = name.split(".")[3]
                for e in range(c.n_expert):
                    t = v[e]
                    out[f"moe.experts.{e}.proj_convs.{s}.0.{leaf}"] = t.reshape(c.d_out, c.d_v, 1) if leaf == "weight" else t
            elif name.startswith("moe.attn0."):
                leaf = name.split(".")[2]
                for e in range(c.n_expert):
                    out[f"moe.experts.{e}.attn_proj.0.{leaf}"] = v[e]
            elif name.startswith("moe.attn2."):
                leaf = name.split(".")[2]
                for e in range(c.n_expert):
                    out[f"moe.experts.{e}.attn_proj.2.{leaf}"] = v[e].reshape(1, -1) if leaf == "weight" else v[e].reshape(1)
            elif name == "vit.patch_embed.weight":
                out[name] = v[:, :c.patch_dim]
            else:
                out[name] = v
        return out

    def _segment_parts(self, name):
        """LAMB's segments (FlatArena.segments): a stacked per-expert entry is one parameter tensor PER EXPERT in the reference
        model, so it gives E segments under named_views()' names - the table agrees one to one with named_views().  The patch-embedding
        weight is one segment with its zero k-step padding columns."""
        E = self.cfg.n_expert
        per = 1
        for d in self.shapes[name][1:]:
            per *= int(d)
        if name.startswith("moe.proj."):
            s, leaf = name.split(".")[2], name.split(".")[3]
            return [(f"moe.experts.{e}.proj_convs.{s}.0.{leaf}", per) for e in range(E)]
        if name.startswith("moe.attn0.") or name.startswith("moe.attn2."):
            k, leaf = name.split(".")[1][-1], name.split(".")[2]
            return [(f"moe.experts.{e}.attn_proj.{k}.{leaf}", per) for e in range(E)]
        return super()._segment_parts(name)

    def export_named(self, flat=None) -> Dict[str, torch.Tensor]:
        """Reference-style names -> fp32 CPU tensors (flat = p32 for weights, g32 for grads)."""
        return {k: v.detach().float().cpu().contiguous() for k, v in self.named_views(flat).items()}
