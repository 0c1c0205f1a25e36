"""Time one training step of a configuration (default cfg2) with and without stochastic depth of the ViT tower (vit_drop_path),
ALTERNATED on one box, at each batch size of `--batches` (default 1024 and 128): every round builds the two engines one after the other (one
engine alive at a time), warms each up and times `--steps` steps as bench.py times a step (the parameters restored from a snapshot before the
start event, HIP events around train_step); the rounds repeat, so a drift of the box shows in both modes alike.  Reported per batch and mode:
the median / min / max step time over all rounds and the peak allocated memory; and from one extra step of the last round with every launch
between its own pair of events, the time of the launches the feature adds (drop_path_scales, scale_add_layernorm_fwd, drop_path) and of the
stand-alone LayerNorm forward launches it replaces.

    python tools/bench_drop_path.py [--config cfg2] [--batches 1024,128] [--rate 0.1] [--rounds 3] [--steps 5] [--warmup 2]

One JSON line.  Needs the GPU: there is no other path."""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WATCH = ("drop_path_scales_kernel", "scale_add_layernorm_fwd_kernel", "drop_path_kernel", "layernorm_fwd_kernel")


def kernel_table(prof):
    rows, total = {}, 0.0
    for label, _, _, e0, e1, _ in prof:
        ms = e0.elapsed_time(e1)
        total += ms
        if label in WATCH:
            k = rows.setdefault(label, [0, 0.0])
            k[0] += 1; k[1] += ms
    out = {label: {"launches": n, "ms": round(ms, 3)} for label, (n, ms) in rows.items()}
    out["all_launches_ms"] = round(total, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--batches", default="1024,128")
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_drop_path: no GPU")
    import bench
    from medmoe_amd import ops
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    modes = {"rate_0": 0.0, f"rate_{args.rate:g}": args.rate}
    out = {"config": args.config, "rate": args.rate, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        times, peak, kernels = {m: [] for m in modes}, {m: 0 for m in modes}, {}
        for rnd in range(args.rounds):
            for mode, rate in modes.items():
                torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                cfg = config_by_name(args.config)
                cfg.vit_drop_path = rate
                eng = Engine(cfg, "cuda:0", seed=0)
                batch = bench.synthetic_batch(eng.cfg, B, 12345, eng.device)
                start = bench.StepStart(eng)
                for _ in range(args.warmup):
                    start.restore()
                    eng.train_step(batch)
                torch.cuda.synchronize()
                spans = []
                for _ in range(args.steps):
                    start.restore()                                # before the start event: outside the timed span
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); eng.train_step(batch); b.record()
                    spans.append((a, b))
                torch.cuda.synchronize()
                times[mode] += [a.elapsed_time(b) for a, b in spans]
                peak[mode] = max(peak[mode], torch.cuda.max_memory_allocated() - start.nbytes)
                if rnd == args.rounds - 1:
                    ops.PROFILE = []
                    start.restore()
                    eng.train_step(batch)
                    torch.cuda.synchronize()
                    kernels[mode] = kernel_table(ops.PROFILE)
                    ops.PROFILE = None
                    if rate > 0.0:
                        kernels[mode]["dropped_fraction"] = round(float((eng.ws["vit_dp"] == 0).float().mean()), 4)
                del eng, batch, start
                gc.collect()
        res = {}
        for m in modes:
            ts = sorted(times[m])
            res[m] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3),
                      "peak_GB": round(peak[m] / 2 ** 30, 3), "kernels": kernels.get(m, {})}
        on, off = [m for m in modes if m != "rate_0"][0], "rate_0"
        res["on_over_off"] = round(res[on]["median_ms"] / res[off]["median_ms"], 4)
        out["batches"][str(B)] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
