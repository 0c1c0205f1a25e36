"""Time one training step under each activation-recomputation mode of the ViT tower (vit_checkpoint = none | selective | full),
ALTERNATED on one box, at each `config:batch` of `--cases` (default cfg2 at 1024 and 128, cfg4 at 256): every round builds the three engines
one after the other (one engine alive at a time), warms each up and times `--steps` steps as bench.py times a step (the parameters restored
from a snapshot before the start event, HIP events around train_step); the rounds repeat, so a drift of the box shows in every mode alike.
Reported per case and mode: the median / min / max step time over all rounds, torch.cuda.max_memory_allocated (less the snapshot), the bytes
vit_activation_plan states for the tower, and the ratio of each mode's median to mode none's.

`--kernel`: instead, medmoe_layernorm_apply against a device-to-device copy of the same bytes (x read, y written) at the token counts of cfg2
batch 1024 and cfg4 batch 256, HIP events around `--steps` back-to-back launches after a warm-up.

    python tools/bench_vit_checkpoint.py [--cases cfg2:1024,cfg2:128,cfg4:256] [--modes none,selective,full] [--rounds 3] [--steps 5] [--warmup 2]
    python tools/bench_vit_checkpoint.py --kernel [--steps 20]

One JSON line.  Needs the GPU: there is no other path."""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_kernel(args, torch):
    from medmoe_amd import ops
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "shapes": {}}
    for rows, D in ((1024 * 197, 768), (256 * 257, 1024), (128 * 197, 768)):
        x = torch.randn(rows, D, device="cuda").bfloat16()
        y, y2, st = torch.empty_like(x), torch.empty_like(x), torch.empty(2, rows, device="cuda")
        gam, bet = torch.rand(D, device="cuda") + 0.5, torch.randn(D, device="cuda")
        ops.layernorm_fwd(x, gam, bet, y, st[0], st[1], 1e-6)
        runs = {"layernorm_apply": lambda: ops.layernorm_apply(x, st[0], st[1], gam, bet, y2), "copy": lambda: y2.copy_(x),
                "layernorm_fwd": lambda: ops.layernorm_fwd(x, gam, bet, y2, st[0], st[1], 1e-6)}
        res = {}
        for rnd in range(3):                                      # alternated
            for name, fn in runs.items():
                for _ in range(3):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                res.setdefault(name, []).append(a.elapsed_time(b) / args.steps)
        ops.layernorm_apply(x, st[0], st[1], gam, bet, y2)
        torch.cuda.synchronize()
        nbytes = 4.0 * rows * D                                   # 2 B read + 2 B written per element
        out["shapes"][f"{rows}x{D}"] = {"equal_to_layernorm_fwd": bool(torch.equal(y2.view(torch.int16), y.view(torch.int16))),
                                        "MB": round(nbytes / 1e6, 1),
                                        **{n: {"us": round(1e3 * min(t), 2), "GB_per_s": round(nbytes / (min(t) * 1e-3) / 1e9, 1)} for n, t in res.items()}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cfg2:1024,cfg2:128,cfg4:256")
    ap.add_argument("--modes", default="none,selective,full")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_vit_checkpoint: no GPU")
    if args.kernel:
        return bench_kernel(args, torch)
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine, plan_bytes, vit_activation_plan
    modes = args.modes.split(",")
    out = {"rounds": args.rounds, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "cases": {}}
    for case in args.cases.split(","):
        name, B = case.split(":")[0], int(case.split(":")[1])
        times, peak, loss = {m: [] for m in modes}, {m: 0 for m in modes}, {}
        for rnd in range(args.rounds):
            for mode in modes:
                gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                cfg = config_by_name(name)
                cfg.vit_checkpoint = mode
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
                    a.record(); res = eng.train_step(batch); b.record()
                    spans.append((a, b))
                torch.cuda.synchronize()
                times[mode] += [a.elapsed_time(b) for a, b in spans]
                peak[mode] = max(peak[mode], torch.cuda.max_memory_allocated() - start.nbytes)
                loss[mode] = float(res["loss"])
                del eng, batch, start, res
        res = {}
        for m in modes:
            ts = sorted(times[m])
            res[m] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3),
                      "peak_GB": round(peak[m] / 2 ** 30, 3), "loss": loss[m],
                      "tower_plan_GB": round(plan_bytes(vit_activation_plan(config_by_name(name), B, m)) / 2 ** 30, 3)}
        if "none" in res:
            for m in modes:
                res[m]["over_none"] = round(res[m]["median_ms"] / res["none"]["median_ms"], 4)
        out["cases"][case] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
