"""The training step under AdamW against LAMB, alternated on ONE engine: `Engine.optimizer_step` reads cfg.optimizer at every step, so the
same engine, the same batch and the same buffers take an `adamw` step and a `lamb` step in turn (parameter groups of the LAMB experiment:
no_decay_1d, weight decay 0.01).  Every step between its own pair of HIP events after a warm-up of both; reported are the median and the
10th / 90th percentile per optimiser and the difference of the medians.

    python tools/bench_lamb_step.py [--config cfg2] [--batch 1024] [--steps 12] [--warmup 3]

One JSON line.  Needs the GPU: there is no other path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=12, help="timed steps per optimiser")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps per optimiser")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lamb_step: no GPU")
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name(args.config)
    cfg.weight_decay, cfg.adam_eps, cfg.clip, cfg.no_decay_1d, cfg.lr = 0.01, 1e-6, 1.0, True, 1e-4
    eng = Engine(cfg, "cuda:0", seed=0)
    batch = bench.synthetic_batch(cfg, args.batch, 0, eng.device)
    times = {"adamw": [], "lamb": []}
    for it in range(args.warmup + args.steps):
        for name in ("adamw", "lamb"):
            eng.cfg.optimizer = name
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); eng.train_step(batch); b.record()
            b.synchronize()
            if it >= args.warmup:
                times[name].append(a.elapsed_time(b))
    out = {"config": args.config, "batch": args.batch, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        ts = sorted(ts)
        out[name] = {"median_ms": round(statistics.median(ts), 3), "p10_ms": round(ts[len(ts) // 10], 3), "p90_ms": round(ts[(len(ts) * 9) // 10], 3)}
    out["lamb_minus_adamw_ms"] = round(out["lamb"]["median_ms"] - out["adamw"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
