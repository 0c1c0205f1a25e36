"""Parameter groups of the fused optimiser step: one rule set (`GroupRules`) -> per store the `assign` dict of
`FlatArena.set_param_groups` (entry name -> (lr_mult, wd_mult)).

    no_decay      fnmatch patterns over the stores' own names: wd_mult = 0.  A pattern that matches nothing in any store raises.
    no_decay_1d   wd_mult = 0 for every parameter that is one-dimensional in the model (biases, LayerNorm weights and biases: entries of
                  one dimension, and the stacked per-expert biases `*.bias`, [E, n] in a ParamStore) and for the embeddings named in
                  EMBED_NO_DECAY (position, class, token-type, Swin's relative-position bias tables).
    text_lr_mult  multiplies the learning rate of every entry of the text store.
    layer_decay   depth-wise learning-rate decay in the BEiT convention: the front-end / embeddings are depth 0, transformer block k is
                  depth k + 1, everything behind the tower (final norm, router, experts) depth L + 1; lr_mult = layer_decay ** (L + 1 - depth).
                  Depths are parsed from the names: `vit.layer.{l}.` (ViT tower), `layer.{i}.` (text tower; composes with text_lr_mult),
                  the running ordinal of `encoder.layers.{s}.blocks.{b}.` (Swin; a stage's patch merging has the depth of the stage's last
                  block, as SimMIM assigns it).

Store kinds: "vit" (ParamStore: image tower + MoE), "text" (TextStore, or the text tower's LoraStore), "vit_lora" (the image tower's LoraStore:
layer l's adapters get the multipliers of layer l's weights, and the no_decay rules see them as the 2-D weights they are), "swin_tower" and "swin_moe" (the two FlatStores of the Swin-T model)."""
import re
from dataclasses import dataclass
from fnmatch import fnmatchcase
from typing import Dict, Iterable, List, Sequence, Tuple

EMBED_NO_DECAY = ("vit.pos_embed", "vit.cls_token", "position_embeddings", "token_type_embeddings", "*.relative_position_bias_table")

_VIT_BLOCK = re.compile(r"^vit\.layer\.(\d+)\.")
_TEXT_BLOCK = re.compile(r"^layer\.(\d+)\.")
_SWIN_BLOCK = re.compile(r"^encoder\.layers\.(\d+)\.blocks\.(\d+)\.")
_SWIN_MERGE = re.compile(r"^encoder\.layers\.(\d+)\.downsample\.")


@dataclass
class GroupRules:
    no_decay: Tuple[str, ...] = ()
    no_decay_1d: bool = False
    text_lr_mult: float = 1.0
    layer_decay: float = 1.0

    @classmethod
    def from_config(cls, cfg) -> "GroupRules":
        return cls(tuple(cfg.no_decay), bool(cfg.no_decay_1d), float(cfg.text_lr_mult), float(cfg.layer_decay))

    def is_default(self) -> bool:
        return not self.no_decay and not self.no_decay_1d and self.text_lr_mult == 1.0 and self.layer_decay == 1.0


def entry_names(store) -> List[str]:
    """The stored entries of an arena (group aliases name concatenations of them and are left out)."""
    return [n for n in store.offsets if n not in store.groups]


def _swin_depths(names: Iterable[str]) -> List[int]:
    depths: Dict[int, int] = {}
    for n in names:
        mt = _SWIN_BLOCK.match(n)
        if mt:
            s, b = int(mt.group(1)), int(mt.group(2))
            depths[s] = max(depths.get(s, 0), b + 1)
    return [depths[s] for s in sorted(depths)]


def depth_of(kind: str, names: Sequence[str]) -> Tuple[Dict[str, int], int]:
    """(name -> depth, L) of a store's entries; L = the number of transformer blocks of the store's tower."""
    out: Dict[str, int] = {}
    if kind == "vit":
        L = 1 + max(int(mt.group(1)) for mt in map(_VIT_BLOCK.match, names) if mt)
        for n in names:
            mt = _VIT_BLOCK.match(n)
            out[n] = int(mt.group(1)) + 1 if mt else (0 if n in ("vit.patch_embed.weight", "vit.patch_embed.bias", "vit.cls_token", "vit.pos_embed") else L + 1)
    elif kind in ("text", "vit_lora"):     # vit_lora: the image tower's adapters (`layer.{l}.`): layer l's adapters have layer l's depth
        L = 1 + max(int(mt.group(1)) for mt in map(_TEXT_BLOCK.match, names) if mt)
        for n in names:
            mt = _TEXT_BLOCK.match(n)
            out[n] = int(mt.group(1)) + 1 if mt else 0              # what is no block is the embedding front-end
    elif kind == "swin_tower":
        depths = _swin_depths(names)
        L = sum(depths)
        for n in names:
            mb, mm = _SWIN_BLOCK.match(n), _SWIN_MERGE.match(n)
            if mb:
                out[n] = sum(depths[:int(mb.group(1))]) + int(mb.group(2)) + 1
            elif mm:
                out[n] = sum(depths[:int(mm.group(1)) + 1])
            else:
                out[n] = 0 if n.startswith("embeddings.") else L + 1
    elif kind in ("swin_moe", "mlm"):      # mlm: the masked-prediction head behind the text tower
        L = 0
        out = {n: 1 for n in names}                                  # behind the tower: depth L + 1, multiplier 1
    else:
        raise KeyError(f"unknown store kind {kind!r}")
    return out, L


def _one_dimensional(name: str, shape) -> bool:
    return len(shape) == 1 or name.endswith(".bias")


def build_assign(stores: Dict[str, object], rules: GroupRules) -> Dict[str, Dict[str, Tuple[float, float]]]:
    """kind -> assign dict for each store of `stores` (kind -> FlatArena).  Raises ValueError for a `no_decay` pattern that matches nothing."""
    unmatched = set(rules.no_decay)
    out: Dict[str, Dict[str, Tuple[float, float]]] = {}
    for kind, st in stores.items():
        names = entry_names(st)
        depth, L = depth_of(kind, names)
        assign = {}
        for n in names:
            lm = float(rules.layer_decay) ** (L + 1 - depth[n])
            if kind == "text":
                lm *= float(rules.text_lr_mult)
            wm = 1.0
            for pat in rules.no_decay:
                if fnmatchcase(n, pat):
                    unmatched.discard(pat)
                    wm = 0.0
            if rules.no_decay_1d and (_one_dimensional(n, st.shapes[n]) or any(fnmatchcase(n, pat) for pat in EMBED_NO_DECAY)):
                wm = 0.0
            if (lm, wm) != (1.0, 1.0):
                assign[n] = (lm, wm)
        out[kind] = assign
    if unmatched:
        raise ValueError(f"optimizer_groups.no_decay: no parameter matches {sorted(unmatched)}")
    return out


def apply_rules(stores: Dict[str, object], rules: GroupRules):
    """Set (or, for the default rule set, clear) the parameter groups of every store."""
    if rules.is_default():
        for st in stores.values():
            st.clear_param_groups()
        return
    for kind, assign in build_assign(stores, rules).items():
        if assign:
            stores[kind].set_param_groups(assign)
        else:
            stores[kind].clear_param_groups()                        # nothing of this store is named: it keeps the ungrouped step


def set_rules(cfg, rules: Dict[str, object]):
    """Write a (partial) rule set into a MedMoEConfig and validate it."""
    for key, val in rules.items():
        if key not in ("no_decay", "no_decay_1d", "text_lr_mult", "layer_decay"):
            raise KeyError(f"optimizer_groups: unknown key {key!r} (no_decay, no_decay_1d, text_lr_mult, layer_decay)")
        setattr(cfg, key, tuple(val) if key == "no_decay" else val)
    cfg.validate()
