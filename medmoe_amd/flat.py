"""Flat parameter arenas.  Every trainable tower keeps its parameters the same way (`FlatArena`): ONE flat fp32 master buffer `p32` with a
gradient buffer `g32` of the same layout (one memset zeroes every gradient of a step, one all-reduce averages them), Adam's `m` / `v`, a bf16
working copy `p16` in the nn.Linear [out, in] layout and a second one, `p16t`, holding every GEMM weight transposed ([in, out]: dgrad runs on
the same NT kernel as forward).  `refresh()` is two kernels (cast + batched transpose) whatever the number of parameters, the clip norm is
summed in a fixed order (`sumsq`), and clip + Adam + the bf16 copy are one launch (`adam_step`) - also with parameter groups
(`set_param_groups`: contiguous runs of the arena with their own learning-rate / weight-decay multipliers) and AdamW.
With the weight EMA (`enable_ema`) an arena also holds `e32`, the fp32 average of the master in the same layout: `adam_step` takes the
`_ema` form of its launch, which averages the parameter it has just updated, and `load_ema()` / `restore_master()` point the working copies at
the average and back.
With `lamb_step` the step is LAMB instead: `segments()` cuts the trainable range into one segment per parameter tensor, three
launches form Adam's moments, one trust ratio per segment from norms summed in a fixed order, and the step; the state is Adam's.
With the bf16 gradient exchange an arena also holds `g16`, the bf16 copy that `pack` fills and the ranks all-reduce: `g32` keeps
the rank-local fp32 sum (what accumulation over micro-batches needs), and while `g16_reduced` is set the clip norm and Adam read `g16`.

The stores say what is specific to them: `ParamStore` (ViT tower + MoE: its spec list, seeded init, the 8-bit expert copies) and
`TextStore` (trainable text tower) build the arena from their spec lists; `FlatStore` below takes any name -> tensor dict (Swin tower,
pyramid experts).

`groups` lays parameters out back to back so that a concatenation the kernels want is a free view: the q / k / v projections of a Swin block
([C, C] each) are one [3C, C] GEMM weight and one [3C] bias (modeling_swin.py SwinSelfAttention keeps them as three nn.Linear)."""
from typing import Dict, List, Sequence, Tuple

import torch

from . import ops
from .ema import one_minus_decay

_ALIGN = 8


def _numel(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _pad(n: int) -> int:
    return (n + _ALIGN - 1) // _ALIGN * _ALIGN


def fused_step_of(cfg):
    """(name of the arena method, its keyword arguments) of the optimiser a configuration names: `adam_step` for "adam" / "adamw",
    `lamb_step` for "lamb" (DESIGN 3s).  The engines call it on every arena they step, behind the one clip norm."""
    kw = dict(betas=tuple(cfg.adam_betas), eps=cfg.adam_eps)
    if cfg.optimizer == "lamb":
        return "lamb_step", dict(kw, always_adapt=bool(cfg.lamb_always_adapt), trust_clip=bool(cfg.lamb_trust_clip))
    return "adam_step", dict(kw, decoupled=cfg.optimizer == "adamw")


class FlatArena:
    def __init__(self, device, entries: Sequence[Tuple[str, Tuple[int, ...]]], groups: Sequence[Tuple[str, List[str]]] = (),
                 gemm: Sequence[Tuple[str, bool]] = (), train_from: str = None):
        """entries: (name, shape) in storage order.  groups: (alias, member names) - the members are stored first, back to back in that order
        (no padding between them, the group padded as a whole), and `alias` names their concatenation along dim 0; every other entry is
        padded to 8 elements.  gemm: (name or alias, stacked) of the GEMM weights, in the order of their rows in the transpose table: one
        row per 2-D matrix - a stacked [E, r, c] weight gives E rows, any other one row (out, in) ([out, in] or [out, in, 1]; the two forms
        cannot be told apart from the shape).  Adam's state is allocated on first need (`adam_state`).
        train_from (an entry name; None: the whole arena trains, today's layout and launches bit for bit): everything stored BEFORE that
        entry is frozen.  `self.train_from` is its offset (a multiple of 8); the master and the working copies still cover the
        whole arena, but g32, m, v, e32 and g16 are TAIL buffers - they hold [train_from, numel) only, `view` finds an entry in either kind
        of buffer, and asking for a frozen entry's gradient, moment or average raises.  No per-step launch touches the frozen range: not
        zero_grad, sumsq, pack, the Adam launch, nor the transposes that follow it."""
        self.device = dev = torch.device(device)
        self.shapes: Dict[str, Tuple[int, ...]] = {n: tuple(s) for n, s in entries}
        member_of = {m for _, ms in groups for m in ms}
        self.offsets: Dict[str, int] = {}
        off = 0
        for _, ms in groups:
            for n in ms:
                self.offsets[n] = off
                off += _numel(self.shapes[n])
            off = _pad(off)
        for n, s in entries:
            if n not in member_of:
                self.offsets[n] = off
                off = _pad(off + _numel(s))
        for a, ms in groups:
            self.shapes[a] = (sum(self.shapes[m][0] for m in ms),) + self.shapes[ms[0]][1:]
            self.offsets[a] = self.offsets[ms[0]]
        self.numel = off
        self.train_from = 0 if train_from is None else self.offsets[train_from]
        if self.train_from % _ALIGN or any(o < self.train_from < o + _numel(self.shapes[n]) for n, o in self.offsets.items()):
            raise ValueError(f"FlatArena: train_from={train_from!r} (offset {self.train_from}) must start an entry at a multiple of {_ALIGN}")
        self.n_train = off - self.train_from                        # elements of a tail buffer
        self.groups: Dict[str, List[str]] = {a: list(ms) for a, ms in groups}
        self.runs = None                                            # parameter groups: [(end, lr_mult, wd_mult)] in storage order, None = none set
        self._run_table = self._one_run = None                      # the device form of `runs` / of the one-run table ((numel, 1, 1))
        self._views: Dict[tuple, tuple] = {}
        z = lambda dt: torch.zeros(off, device=dev, dtype=dt)
        self.p32, self.p16, self.p16t = z(torch.float32), z(torch.bfloat16), z(torch.bfloat16)
        self.g32 = torch.zeros(self.n_train, device=dev, dtype=torch.float32)
        rows = []
        self._mat: Dict[str, Tuple[int, ...]] = {}                  # GEMM weight -> its matrix form, (r, c) or (E, r, c)
        for n, stacked in gemm:
            s, o = self.shapes[n], self.offsets[n]
            form = self._mat[n] = tuple(s) if stacked else (int(s[0]), _numel(s[1:]))
            r, c = form[-2:]
            rows += [[o + e * r * c, o + e * r * c, r, c] for e in range(_numel(form[:-2]))]
        self.tr_table = torch.tensor(rows, device=dev, dtype=torch.int64) if rows else None
        self.tr_max_tiles = max(((r[2] + 63) // 64) * ((r[3] + 63) // 64) for r in rows) if rows else 0
        # what an optimiser step re-derives: the trainable matrices only (the whole table when nothing is frozen)
        self._tr_step, self._tr_step_tiles = self.tr_table, self.tr_max_tiles
        if self.train_from:
            rows = [r for r in rows if r[0] >= self.train_from]
            self._tr_step = torch.tensor(rows, device=dev, dtype=torch.int64) if rows else None
            self._tr_step_tiles = max(((r[2] + 63) // 64) * ((r[3] + 63) // 64) for r in rows) if rows else 0
        self.m = self.v = self.normsq = self.norm_scratch = None
        self.step_count = 0
        # bf16 gradient exchange: `g16` (bf16, this layout, allocated on first need) receives pack()'s bf16(g32 * scale) and is
        # what the ranks all-reduce; `g16_reduced` says that it holds the reduced gradient of the current step, and sumsq() / adam_step()
        # then read it instead of g32.  g32 keeps the rank-local fp32 sum throughout: micro-batches accumulate there, unrounded.
        self._g16 = None
        self.g16_reduced = False
        # weight EMA: `e32` (fp32, this layout) exists from enable_ema() on, `ema_updates` counts the updates it has seen (the
        # warm-up schedule's t); `ema_loaded` says that the working copies currently hold the average (load_ema .. restore_master)
        self.e32 = None
        self.ema_updates = 0
        self.ema_loaded = False
        # LAMB: the segment table (one segment per parameter tensor; built lazily, dropped with the parameter groups) and, from the
        # first lamb_step on, the record scratch of the segmented norms and the trust ratios of the last step
        self._segments = self._seg_table = None
        self._lamb_scratch = self._lamb_ratios = None
        self._lamb_floats, self._lamb_coef_slot = 2, 0

    # -- views: built once per buffer (a backward asks for a few hundred of them per step) -----------------------------------------------
    def view(self, flat, name, shape=None):
        """`name`'s elements of a flat buffer of this layout, in its own shape or any other of no more elements."""
        shape = self.shapes[name] if shape is None else shape
        o = self.offsets[name]
        if self.train_from and flat.numel() == self.n_train:        # a tail buffer: g32, m, v, e32, g16
            o -= self.train_from
            if o < 0:
                raise KeyError(f"{name} is frozen (stored before offset {self.train_from}): it has no gradient, Adam state or average")
        return flat[o: o + _numel(shape)].view(shape)

    def is_frozen(self, name) -> bool:
        return self.offsets[name] < self.train_from

    def _cached(self, kind, flat, name, shape=None):
        key = (kind, name)
        hit = self._views.get(key)
        if hit is None or hit[0] is not flat:
            hit = self._views[key] = (flat, self.view(flat, name, shape))
        return hit[1]

    def _form(self, name):
        return self._mat.get(name) or self.shapes[name]

    def f32(self, name):
        """fp32 view of `name` as the passes read it: of the master - of the average while load_ema() holds (biases, LayerNorms, embeddings
        and the router are read in fp32, not from p16)."""
        return self.ema(name) if self.ema_loaded and not self.is_frozen(name) else self._cached(0, self.p32, name)

    def ema(self, name):
        """fp32 view of `name`'s average (enable_ema() first)."""
        if self.e32 is None:
            raise RuntimeError("FlatArena.ema: this arena keeps no average (enable_ema())")
        return self._cached(5, self.e32, name)
    def grad(self, name): return self._cached(1, self.g32, name)

    def w16(self, name):
        """bf16 view in the matrix form ([out, in]; [E, out, in] of a stacked weight)."""
        return self._cached(2, self.p16, name, self._form(name))

    def w16t(self, name):
        """bf16 [in, out] ([E, in, out]) view of a GEMM weight: the transposed copy."""
        f = self._form(name)
        return self._cached(3, self.p16t, name, f[:-2] + (f[-1], f[-2]))

    def grad2d(self, name):
        return self._cached(4, self.g32, name, self._form(name))

    # -- working copies ------------------------------------------------------------------------------------------------------------------
    def refresh(self):
        """bf16 working copies after the fp32 master changed (an initialisation, a loaded checkpoint)."""
        ops.call("cast_bf16", self.p32, self.p16, self.numel)
        self._derive()

    sync_working_copies = refresh                                   # the stores' earlier name for it: the same method

    def _derive(self, src=None, step: bool = False):
        """What follows p16 after every update: the transposed copies, then the store's own derived copies.  `src`: the fp32 buffer p16 was
        just cast from (None: the master).  step: after an optimiser step or a switch to the average - only what trains changed (restore_master takes the full refresh())."""
        table, tiles = (self._tr_step, self._tr_step_tiles) if step else (self.tr_table, self.tr_max_tiles)
        if table is not None:
            ops.call("transpose_many", self.p16, self.p16t, table, table.shape[0], tiles)
        if src is None:
            self.after_update()
        else:
            self.after_update(src)

    def after_update(self, src=None):
        """Hook: copies a store derives from the fp32 buffer itself, not from p16 (ParamStore's 8-bit expert weights).  `src`: the flat fp32
        buffer the working copies were just cast from - None: the master; load_ema() passes the average."""

    # -- weight EMA ----------------------------------------------------------------------------------------------------------------------
    def enable_ema(self):
        """Keep an average of the master from here on: `e32` is allocated on the first call, and every call sets it to the master as it is
        now with no update counted (so a call after a checkpoint was loaded drops whatever the average held before)."""
        if self.ema_loaded:
            raise RuntimeError("FlatArena.enable_ema: the working copies hold the average (restore_master() first)")
        if self.e32 is None:
            self.e32 = torch.zeros(self.n_train, device=self.device, dtype=torch.float32)
        self.e32.copy_(self.p32[self.train_from:])
        self.ema_updates = 0

    def load_ema(self):
        """The working copies (p16, p16t, the store's derived copies) from the average instead of the master, and f32() hands out views of
        the average: the forward passes then run on the averaged weights.  The master, the gradient and Adam's state are not touched;
        restore_master() undoes it.  Views of f32() taken BEFORE the call stay views of the master: whoever keeps some asks again."""
        if self.e32 is None:
            raise RuntimeError("FlatArena.load_ema: this arena keeps no average (enable_ema())")
        ops.call("cast_bf16", self.e32, self.p16[self.train_from:], self.n_train)
        self._derive(self.e32, step=True)
        self.ema_loaded = True

    def restore_master(self):
        """The working copies from the master again (refresh())."""
        self.ema_loaded = False                                     # first: the hook's f32() views are the master's again
        self.refresh()

    # -- bf16 gradient exchange ----------------------------------------------------------------------------------------------------------
    @property
    def g16(self) -> torch.Tensor:
        if self._g16 is None:
            self._g16 = torch.zeros(self.n_train, device=self.device, dtype=torch.bfloat16)
        return self._g16

    def pack(self, lo: int, hi: int, scale: float):
        """g16[lo:hi] = bf16(g32[lo:hi] * scale) on the current stream (medmoe_grad_pack_bf16; lo a multiple of 8, as every entry's offset
        is).  g32 is left as it is: the rank-local fp32 sum that accumulation over micro-batches needs.  lo / hi index the gradient buffer
        (with a frozen head: the trainable tail, as `grad_bounds` maps arena offsets)."""
        ops.call("grad_pack_bf16", self.g32[lo:hi], self.g16[lo:hi], hi - lo, scale)

    def reduced_grad(self) -> torch.Tensor:
        """The gradient the optimiser will see, as fp32: the reduced bf16 gradient up-cast while it is current, g32 otherwise."""
        return self.g16.float() if self.g16_reduced else self.g32

    # -- fused clip + Adam ---------------------------------------------------------------------------------------------------------------
    def zero_grad(self):
        self.g32.zero_()
        self.g16_reduced = False

    def has_adam_state(self) -> bool:
        return self.m is not None

    def adam_state(self):
        """(m, v), allocated with the clip norm's buffers on first need: an arena that is never stepped (the autograd Swin path) holds none."""
        if self.m is None:
            self.m, self.v = torch.zeros_like(self.g32), torch.zeros_like(self.g32)
            self.normsq = torch.zeros(1, device=self.device, dtype=torch.float32)
            self.norm_scratch = torch.zeros(2049, device=self.device, dtype=torch.float32)   # per-block partials + arrival counter
        return self.m, self.v

    def sumsq(self) -> torch.Tensor:
        """Sum of squares of the gradient arena, summed in a fixed order (identical on every rank): this arena's share of the clip norm."""
        self.adam_state()
        if self.g16_reduced:                                        # the bf16-reduced gradient: the same sum in the same order, read as bf16
            ops.call("sumsq_det_bf16", self.g16, self.n_train, self.normsq, self.norm_scratch)
        else:
            ops.call("sumsq_det", self.g32, self.n_train, self.normsq, self.norm_scratch)
        return self.normsq

    # -- parameter groups: contiguous runs of the arena with their own learning-rate and weight-decay multipliers ---------------------------
    def grad_bounds(self, bounds):
        """Arena offsets -> indices of the gradient buffer: shifted by train_from, whatever lies in the frozen head dropped (the first
        bound that survives is 0)."""
        tf = self.train_from
        out = [b - tf for b in bounds if b > tf]
        return ([0] + out) if tf else list(bounds)

    def _upload_runs(self, runs):
        dev, tf = self.device, self.train_from
        runs = [(r[0] - tf, r[1], r[2]) for r in runs if r[0] > tf]  # the Adam launch sees the trainable tail only
        return (torch.tensor([r[0] for r in runs], device=dev, dtype=torch.int64), torch.tensor([r[1] for r in runs], device=dev, dtype=torch.float32),
                torch.tensor([r[2] for r in runs], device=dev, dtype=torch.float32))

    def set_param_groups(self, assign: Dict[str, Tuple[float, float]]):
        """assign: entry name or group alias -> (lr_mult, wd_mult); an alias covers all its members, a member's own entry wins over its
        alias, everything unnamed gets (1, 1).  The arena is cut into runs in storage order: adjacent entries of equal multipliers are one
        run, an entry's padding belongs to its run (so to the run of the entry before the next one), and because group members lie back to
        back a boundary may fall on any element.  The table goes to the device once, here: a step reads nothing from the host."""
        for name in assign:
            if name not in self.shapes:
                raise KeyError(f"set_param_groups: unknown parameter or group {name!r}")
        alias_of = {m: a for a, ms in self.groups.items() for m in ms}
        entries = sorted((o, n) for n, o in self.offsets.items() if n not in self.groups)
        runs: List[Tuple[int, float, float]] = []
        for k, (_, name) in enumerate(entries):
            lm, wm = assign.get(name, assign.get(alias_of.get(name), (1.0, 1.0)))
            end = entries[k + 1][0] if k + 1 < len(entries) else self.numel
            if runs and runs[-1][1:] == (float(lm), float(wm)):
                runs[-1] = (end, float(lm), float(wm))
            else:
                runs.append((end, float(lm), float(wm)))
        self.runs = runs
        self._run_table = self._upload_runs(runs)
        self._segments = self._seg_table = None                      # the segment table carries the runs' multipliers: rebuilt on next need

    def clear_param_groups(self):
        self.runs = self._run_table = None
        self._segments = self._seg_table = None

    def adam_step(self, normsq_total: torch.Tensor, lr: float, weight_decay: float, clip: float, grad_scale: float = 1.0, *,
                  betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, decoupled: bool = False, ema_decay: float = 0.0,
                  ema_warmup: bool = False):
        """clip (against `normsq_total`, the squared norm over ALL arenas of the model, as clip_grad_norm_ over all parameters computes it)
        + torch.optim.Adam's update (L2 weight decay; decoupled: torch.optim.AdamW's) on the fp32 master, the bf16 copy written by the same
        kernel; the derived copies follow.  Without parameter groups, with Adam's default betas / eps and L2 decay this is medmoe_adam_step;
        anything else is ONE medmoe_adam_groups_step over the arena's run table (a single run when no groups are set).  Gradients must be
        in THIS arena's g32 (no new_grad_arena() since the backward) - or, after a bf16 gradient exchange (`g16_reduced`), in g16: the
        same two launches in their _g16 form read it as bf16, and the flag is cleared with the step.
        ema_decay > 0 (enable_ema() first): the `_ema` form of whichever launch this would have been - the same update, and
        e32 <- e32 + (1 - d_t) (p32_new - e32) by the lane that holds the new parameter, d_t = ema.ema_decay_at(ema_updates, ema_decay,
        ema_warmup); 1 - d_t is a by-value launch argument."""
        if self.ema_loaded:
            raise RuntimeError("FlatArena.adam_step: the working copies hold the average (restore_master() first)")
        ema_args = ()
        if float(ema_decay) > 0.0:
            if self.e32 is None:
                raise RuntimeError("FlatArena.adam_step(ema_decay > 0): this arena keeps no average (enable_ema())")
            ema_args = (self.e32, one_minus_decay(self.ema_updates, ema_decay, ema_warmup))
        m, v = self.adam_state()
        self.step_count += 1
        b1, b2 = float(betas[0]), float(betas[1])
        g, sfx = (self.g16, "_g16") if self.g16_reduced else (self.g32, "")
        if ema_args:
            sfx = "_ema" + sfx
        tf = self.train_from
        p32, p16 = (self.p32[tf:], self.p16[tf:]) if tf else (self.p32, self.p16)
        if self.runs is None and not decoupled and (b1, b2) == (0.9, 0.999) and float(eps) == 1e-8:
            ops.call("adam_step" + sfx, p32, g, m, v, p16, self.n_train, lr, 0.9, 0.999, 1e-8, weight_decay, self.step_count,
                     normsq_total, clip, grad_scale, *ema_args)
        else:
            if self.runs is None and self._one_run is None:
                self._one_run = self._upload_runs([(self.numel, 1.0, 1.0)])
            ends, lrm, wdm = self._run_table if self.runs is not None else self._one_run
            ops.call("adam_groups_step" + sfx, p32, g, m, v, p16, self.n_train, ends, lrm, wdm, ends.numel(), lr, b1, b2, eps,
                     weight_decay, 1 if decoupled else 0, self.step_count, normsq_total, clip, grad_scale, *ema_args)
        if ema_args:
            self.ema_updates += 1
        self.g16_reduced = False
        self._derive(step=True)

    # -- LAMB: per-tensor trust ratios -----------------------------------------------------------------------------------------
    def _segment_parts(self, name) -> List[Tuple[str, int]]:
        """Hook: the parameter tensors of the reference model one stored entry holds, as (name, elements) in storage order - the entry itself
        unless a store stacks several tensors in one entry (ParamStore's per-expert weights)."""
        return [(name, _numel(self.shapes[name]))]

    def segments(self) -> List[Tuple[str, int]]:
        """[(name, end)] in storage order: segment k is elements [end_{k-1}, end_k) of the trainable tail (of g32, m, v), the last end is
        n_train.  One segment per stored entry - the members of a group alias individually, never the alias - split further by
        `_segment_parts`; an entry's alignment padding belongs to the segment in front of it.  With a frozen head only the tail has
        segments.  Built on first need and again after the parameter groups changed; the device form (ends, the run multipliers of every
        segment, the first record of every segment) is uploaded once, then."""
        if self._segments is None:
            self._build_segments()
        return self._segments

    def _build_segments(self):
        tf, dev = self.train_from, self.device
        entries = sorted((o, n) for n, o in self.offsets.items() if n not in self.groups)
        segs: List[Tuple[str, int]] = []
        for k, (o, name) in enumerate(entries):
            if o < tf:
                continue
            nxt = entries[k + 1][0] if k + 1 < len(entries) else self.numel
            parts = self._segment_parts(name)
            if sum(c for _, c in parts) != _numel(self.shapes[name]):
                raise AssertionError(f"FlatArena.segments: the parts of {name} do not add up to its {_numel(self.shapes[name])} elements")
            pos = o
            for j, (pn, cnt) in enumerate(parts):
                pos += cnt
                segs.append((pn, (nxt if j + 1 == len(parts) else pos) - tf))
        runs = self.runs if self.runs is not None else [(self.numel, 1.0, 1.0)]
        lrm, wdm, r, start = [], [], 0, 0
        for name, end in segs:
            while runs[r][0] - tf <= start and r + 1 < len(runs):
                r += 1
            # runs break at entry boundaries, so a tensor lies in ONE run: its trust ratio belongs to one (lr_mult, wd_mult)
            assert end <= runs[r][0] - tf or end == start, f"FlatArena.segments: {name} [{start}, {end}) straddles the run ending at {runs[r][0] - tf}"
            lrm.append(runs[r][1]); wdm.append(runs[r][2])
            start = end
        assert segs and segs[-1][1] == self.n_train
        ends = torch.tensor([e for _, e in segs], dtype=torch.int64)
        self._seg_table = (ends.to(dev), torch.tensor(lrm, device=dev, dtype=torch.float32), torch.tensor(wdm, device=dev, dtype=torch.float32),
                           ops.lamb_plan(ends, self.n_train).to(dev))
        self._lamb_floats = max(ops.lamb_scratch_floats(self.n_train, len(segs)), 2)   # the record scratch this table needs
        self._lamb_coef_slot = ops.lamb_coef_slot(self.n_train, len(segs))
        self._segments = segs

    def trust_ratios(self):
        """(segment names, fp32 device tensor of their trust ratios) of the last lamb_step - for logging and for the tests."""
        if self._lamb_ratios is None:
            raise RuntimeError("FlatArena.trust_ratios: no lamb_step yet")
        segs = self.segments()
        return [n for n, _ in segs], self._lamb_ratios[:len(segs)]

    def last_clip_coef(self) -> torch.Tensor:
        """fp32 device scalar: grad_scale * the clip coefficient the last lamb_step scaled this arena's gradient by (the moments launch forms
        it as the Adam launches do and leaves it behind its records) - for logging and for the tests."""
        if self._lamb_scratch is None:
            raise RuntimeError("FlatArena.last_clip_coef: no lamb_step yet")
        return self._lamb_scratch[self._lamb_coef_slot]

    def lamb_step(self, normsq_total: torch.Tensor, lr: float, weight_decay: float, clip: float, grad_scale: float = 1.0, *,
                  betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-6, always_adapt: bool = False, trust_clip: bool = False,
                  ema_decay: float = 0.0, ema_warmup: bool = False):
        """clip (against `normsq_total`, as adam_step) + LAMB on the fp32 master: Adam's moments, u = m_hat / (sqrt(v_hat) + eps) + wd p, and
        per segment (`segments()`: one parameter tensor) the trust ratio r = |p| / |u| - 1 where either norm is 0, and where the tensor has
        no decay unless always_adapt; min(r, 1) with trust_clip - then p -= lr r u.  Three launches (medmoe_lamb_moments / _ratios /
        _apply): the norms are summed from per-chunk records in a fixed order, no atomics, nothing read from the host.  adam_step's
        contract otherwise: the gradient in g32 or, after a bf16 exchange, in g16 (the moments launch in its _g16 form; the flag is
        cleared), the bf16 copy written by the applying launch, ema_decay > 0 selects its _ema form, the derived copies follow.  The state
        is Adam's (m, v, step_count); the scratch and the ratios are allocated on the first call."""
        if self.ema_loaded:
            raise RuntimeError("FlatArena.lamb_step: the working copies hold the average (restore_master() first)")
        ema_args = ()
        if float(ema_decay) > 0.0:
            if self.e32 is None:
                raise RuntimeError("FlatArena.lamb_step(ema_decay > 0): this arena keeps no average (enable_ema())")
            ema_args = (self.e32, one_minus_decay(self.ema_updates, ema_decay, ema_warmup))
        m, v = self.adam_state()
        n_seg = len(self.segments())
        ends, lrm, wdm, base = self._seg_table
        if self._lamb_scratch is None or self._lamb_scratch.numel() < self._lamb_floats:
            self._lamb_scratch = torch.zeros(self._lamb_floats, device=self.device, dtype=torch.float32)
        if self._lamb_ratios is None or self._lamb_ratios.numel() != 3 * n_seg:
            self._lamb_ratios = torch.zeros(3 * n_seg, device=self.device, dtype=torch.float32)
        self.step_count += 1
        b1, b2 = float(betas[0]), float(betas[1])
        g, sfx = (self.g16, "_g16") if self.g16_reduced else (self.g32, "")
        tf = self.train_from
        p32, p16 = (self.p32[tf:], self.p16[tf:]) if tf else (self.p32, self.p16)
        scratch, ratios = self._lamb_scratch, self._lamb_ratios
        ops.call("lamb_moments" + sfx, p32, g, m, v, self.n_train, ends, wdm, base, n_seg, scratch, scratch.numel(), b1, b2, eps,
                 weight_decay, self.step_count, normsq_total, clip, grad_scale)
        ops.call("lamb_ratios", scratch, scratch.numel(), ends, wdm, base, n_seg, self.n_train, weight_decay, 1 if always_adapt else 0,
                 1 if trust_clip else 0, ratios)
        ops.call("lamb_apply" + ("_ema" if ema_args else ""), p32, m, v, p16, self.n_train, ends, lrm, wdm, n_seg, ratios, lr, b1, b2, eps,
                 weight_decay, self.step_count, *ema_args)
        if ema_args:
            self.ema_updates += 1
        self.g16_reduced = False
        self._derive(step=True)


class FlatStore(FlatArena):
    def __init__(self, weights: Dict[str, torch.Tensor], device, groups: Sequence[Tuple[str, List[str]]] = (), gemm: Sequence[str] = ()):
        """weights: name -> floating tensor.  groups: (alias, member names) - members are stored contiguously in that order, `alias` then names the
        concatenation along dim 0.  gemm: names or aliases that are GEMM weights ([out, in] or [out, in, 1]): they get a transposed bf16 copy
        (16-byte accesses: a GEMM weight inside a group must have a multiple of 8 elements, as must every member before it)."""
        for a, ms in groups:
            if any(tuple(weights[m].shape[1:]) != tuple(weights[ms[0]].shape[1:]) for m in ms):
                raise ValueError(f"FlatStore: group {a} concatenates parameters of different trailing shapes")
        super().__init__(device, [(n, v.shape) for n, v in weights.items()], groups, [(n, False) for n in gemm])
        for n in gemm:
            if self.offsets[n] % _ALIGN:
                raise ValueError(f"FlatStore: GEMM weight {n} starts at element {self.offsets[n]}, not a multiple of {_ALIGN}")
        self.names = list(weights)
        for n in self.names:
            self.f32(n).copy_(weights[n].detach().to(self.device, torch.float32))
        self.refresh()

    def new_grad_arena(self):
        """A fresh gradient buffer (the previous one stays alive through whoever still holds views of it: parameter .grad tensors that were
        not released before this backward)."""
        self.g32 = torch.zeros_like(self.g32)
        self.g16_reduced = False

    def grads(self) -> Dict[str, torch.Tensor]:
        return {n: self.grad(n) for n in self.names}
