"""Exponential moving average of the weights inside the fused optimiser step: the schedule of the decay.  The averaging itself is
part of the Adam launch (csrc/optim.hip, the EMA instantiations; `FlatArena.adam_step(ema_decay=...)`); the host only says how much of the
new parameter the update takes."""
import ctypes


def ema_decay_at(t: int, decay: float, warmup: bool = False) -> float:
    """The decay d_t of update t (0-based: t = the number of updates the average has seen).  Constant `decay`, or with `warmup` the usual
    ramp min(decay, (1 + t) / (10 + t)): 0.1 at the first update, so that an average started at the initial weights forgets them quickly."""
    t, decay = int(t), float(decay)
    if t < 0:
        raise ValueError(f"ema update index must be >= 0, got {t}")
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1), got {decay}")
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def one_minus_decay(t: int, decay: float, warmup: bool = False) -> float:
    """1 - d_t as the kernels take it: formed in double, rounded ONCE to float (the value returned is that float, exactly)."""
    return ctypes.c_float(1.0 - ema_decay_at(t, decay, warmup)).value


def step_kwargs(cfg) -> dict:
    """The EMA arguments of FlatArena.adam_step for a configuration: none while cfg.ema_decay is 0 (the step is then the one it was)."""
    return {"ema_decay": float(cfg.ema_decay), "ema_warmup": bool(cfg.ema_warmup)} if float(cfg.ema_decay) > 0.0 else {}


def prepare(arenas):
    """Before a step or an evaluation on the average: every arena keeps one, and one that has seen no update yet is (re)started from the
    master as it is NOW - whatever rewrote the master since construction (a loaded state dict) leaves no stale average behind."""
    for a in arenas:
        if a.e32 is None or a.ema_updates == 0:
            a.enable_ema()
