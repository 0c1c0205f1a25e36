"""Time one training step of a configuration (default cfg2 at the `bench.py --train-text` geometry: the global batch on one GPU) in the three
text modes - frozen tower, fully trainable tower (freeze_text = False), LoRA adapters on the frozen tower (text_lora) - ALTERNATED on one box:
each round builds the modes' engines one after the other (one engine alive at a time: three cfg2 workspaces do not have to fit together),
warms each up and times `--steps` steps between HIP events; the rounds repeat, so a drift of the box shows in every mode alike.  Reported per
mode: the median / min step time over all rounds, the peak allocated memory, and for the LoRA mode every adapter kernel's time and achieved
bytes per second against its own algorithmic byte count (ops._COSTS: x once, the targeted qkv / dqkv columns, U / dU, dy), taken from one
extra step with every launch between its own pair of events.

    python tools/bench_text_lora.py [--config cfg2] [--batch 1024] [--rounds 3] [--steps 5] [--warmup 2] [--rank 8] [--dropout 0.1]

One JSON line.  Needs the GPU: there is no other path."""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("frozen", "trainable", "lora")


def build(mode, args):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name(args.config)
    if mode == "trainable":
        cfg.freeze_text = False
    elif mode == "lora":
        cfg.text_lora, cfg.text_lora_r, cfg.text_lora_alpha, cfg.text_lora_dropout = True, args.rank, 2.0 * args.rank, args.dropout
    return Engine(cfg, "cuda:0", seed=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--modes", default=",".join(MODES))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_lora: no GPU")
    import bench
    from medmoe_amd import ops
    modes = [m for m in args.modes.split(",") if m]
    times = {m: [] for m in modes}
    peak = {m: 0 for m in modes}
    kernels = {}
    for rnd in range(args.rounds):
        for mode in modes:
            torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            eng = build(mode, args)
            if mode == "lora":                                     # B = 0 would leave d A = 0: the timing does not care, the arithmetic should be live
                lo = eng.lora
                g = torch.Generator().manual_seed(1)
                lo.load_named({"text." + n: 0.02 * torch.randn(lo.D, lo.r, generator=g) for n in lo.true_names() if n.endswith("lora_B")})
            batch = bench.synthetic_batch(eng.cfg, args.batch, 12345, eng.device)
            for _ in range(args.warmup):
                eng.train_step(batch)
            torch.cuda.synchronize()
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); eng.train_step(batch); b.record()
                b.synchronize()
                times[mode].append(a.elapsed_time(b))
            peak[mode] = max(peak[mode], torch.cuda.max_memory_allocated())
            if mode == "lora" and rnd == args.rounds - 1:
                ops.PROFILE = []
                eng.train_step(batch)
                torch.cuda.synchronize()
                for label, work, unit, e0, e1, _ in ops.PROFILE:
                    if label.startswith("lora_"):
                        k = kernels.setdefault(label, {"launches": 0, "ms": 0.0, "bytes": 0.0})
                        k["launches"] += 1; k["ms"] += e0.elapsed_time(e1); k["bytes"] += work
                ops.PROFILE = None
            del eng, batch
            gc.collect()
    out = {"config": args.config, "batch": args.batch, "rounds": args.rounds, "steps": args.steps, "rank": args.rank, "dropout": args.dropout,
           "device": torch.cuda.get_device_name(0)}
    for m in modes:
        ts = sorted(times[m])
        out[m] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3),
                  "peak_GB": round(peak[m] / 2 ** 30, 3)}
    for label, k in kernels.items():
        k["ms"] = round(k["ms"], 4)
        k["TB_per_s"] = round(k["bytes"] / (k["ms"] * 1e-3) / 1e12, 3) if k["ms"] > 0 else None
        k["bytes"] = int(k["bytes"])
    out["lora_kernels"] = kernels
    if "trainable" in out and "lora" in out:
        out["lora_over_trainable"] = round(out["lora"]["median_ms"] / out["trainable"]["median_ms"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
