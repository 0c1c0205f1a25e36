"""Time one training step of a configuration (default cfg2) with the image tower trainable / frozen (freeze_vit) / frozen with LoRA adapters
(vit_lora, dropout 0 and --dropout), ALTERNATED on one box as tools/bench_text_lora.py does: each round builds the variants' engines one after
the other (one engine alive at a time), warms each up and times `--steps` steps between HIP events; the rounds repeat, so a drift of the box
shows in every variant alike.  Reported per variant: the median / min / max step time over all rounds and the peak allocated memory; for the
adapter variants every adapter kernel's time and achieved bytes per second against its own algorithmic byte count (ops._COSTS: ln1 once, the
targeted qkv / dqkv columns, U / dU, d ln1), taken from one extra step with every launch between its own pair of events.

--sweep: the adapter weight-gradient launch alone (medmoe_lora_bwd_wgrad_runs) for run in 1, 2, 4, 8, 16 at M = B * 197 rows of D = 768 with
two targets, B = 1024 and 128 (M = 201 728 and 25 216), dropout 0 and --dropout, the runs alternated; next to them medmoe_lora_bwd_wgrad
(run "base") and the run Engine.vit_lora_wgrad_run picks.

    python tools/bench_vit_lora.py [--config cfg2] [--batch 1024] [--rounds 3] [--steps 5] [--warmup 2] [--rank 8] [--dropout 0.1] [--sweep]

One JSON line.  Needs the GPU: there is no other path."""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("trainable", "frozen", "lora", "lora_drop")


def build(variant, args):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name(args.config)
    if variant == "frozen":
        cfg.freeze_vit = True
    elif variant in ("lora", "lora_drop"):
        cfg.vit_lora, cfg.vit_lora_r, cfg.vit_lora_alpha = True, args.rank, 2.0 * args.rank
        cfg.vit_lora_dropout = args.dropout if variant == "lora_drop" else 0.0
    return Engine(cfg, "cuda:0", seed=0)


def sweep(args, torch, ops):
    from medmoe_amd.engine import Engine
    BF = torch.bfloat16
    D, n, tg = 768, 2, ("query", "value")
    out = {}
    for B in (1024, 128):
        M = B * 197
        g = torch.Generator().manual_seed(0)
        x, dqkv = torch.randn(M, D, generator=g).to(BF).cuda(), (0.1 * torch.randn(M, 3 * D, generator=g)).to(BF).cuda()
        U, dU = torch.randn(M, n * 16, generator=g).to(BF).cuda(), torch.randn(M, n * 16, generator=g).to(BF).cuda()
        gA, gB = torch.zeros(n * 16, D, device="cuda"), torch.zeros(n * D, 16, device="cuda")
        runs = ("base", 1, 2, 4, 8, 16)
        sc = {r: torch.empty(ops.lora_wgrad_scratch(M, D, n) if r == "base" else ops.lora_wgrad_runs_scratch(M, D, n, r), device="cuda") for r in runs}
        rec = {"M": M, "algorithmic_MB": round(2.0 * M * (n * D + D + 2 * n * 16) / 1e6, 1), "engine_run": Engine.vit_lora_wgrad_run(M, D)}
        for p in (0.0, args.dropout):
            rng = ops.dropout_rng(1, 2, ops.DROPOUT_SITE_VIT_LORA, p) if p > 0 else None
            us = {r: [] for r in runs}

            def launch(r):
                if r == "base":
                    ops.lora_bwd_wgrad(dqkv, x, U, dU, gA, gB, sc[r], tg, 2.0, rng)
                else:
                    ops.lora_bwd_wgrad_runs(dqkv, x, U, dU, gA, gB, sc[r], tg, 2.0, r, rng)
            for _ in range(args.rounds):
                for r in runs:
                    launch(r); torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(10):
                        launch(r)
                    b.record(); b.synchronize()
                    us[r].append(a.elapsed_time(b) * 100.0)
            rec[f"dropout_{p}"] = {str(r): {"us": [round(v, 1) for v in us[r]], "scratch_MB": round(sc[r].numel() * 4 / 1e6, 1)} for r in runs}
        out[f"batch_{B}"] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--sweep", action="store_true", help="the weight-gradient launch's run sweep instead of the step timings")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_vit_lora: no GPU")
    import bench
    from medmoe_amd import ops
    out = {"config": args.config, "batch": args.batch, "rounds": args.rounds, "steps": args.steps, "rank": args.rank, "dropout": args.dropout,
           "device": torch.cuda.get_device_name(0)}
    if args.sweep:
        out["wgrad_runs"] = sweep(args, torch, ops)
        print(json.dumps(out), flush=True)
        return
    variants = [v for v in args.variants.split(",") if v]
    times, peak, kernels = {v: [] for v in variants}, {v: 0 for v in variants}, {}
    for rnd in range(args.rounds):
        for v in variants:
            torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            eng = build(v, args)
            if eng.vlora is not None:                              # B = 0 would leave d A = 0: the timing does not care, the arithmetic should be live
                lo = eng.vlora
                g = torch.Generator().manual_seed(1)
                lo.load_named({"vit." + n: 0.02 * torch.randn(lo.D, lo.r, generator=g) for n in lo.true_names() if n.endswith("lora_B")})
            batch = bench.synthetic_batch(eng.cfg, args.batch, 12345, eng.device)
            for _ in range(args.warmup):
                eng.train_step(batch)
            torch.cuda.synchronize()
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); eng.train_step(batch); b.record()
                b.synchronize()
                times[v].append(a.elapsed_time(b))
            peak[v] = max(peak[v], torch.cuda.max_memory_allocated())
            if eng.vlora is not None and rnd == args.rounds - 1:
                ops.PROFILE = []
                eng.train_step(batch)
                torch.cuda.synchronize()
                ks = kernels.setdefault(v, {})
                for label, work, unit, e0, e1, _ in ops.PROFILE:
                    if label.startswith("lora_"):
                        k = ks.setdefault(label, {"launches": 0, "ms": 0.0, "bytes": 0.0})
                        k["launches"] += 1; k["ms"] += e0.elapsed_time(e1); k["bytes"] += work
                ops.PROFILE = None
                out["engine_run"] = eng._vlora_run
            del eng, batch
            gc.collect()
    for v in variants:
        ts = sorted(times[v])
        out[v] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3),
                  "peak_GB": round(peak[v] / 2 ** 30, 3)}
    for ks in kernels.values():
        for k in ks.values():
            k["ms"] = round(k["ms"], 4)
            k["TB_per_s"] = round(k["bytes"] / (k["ms"] * 1e-3) / 1e12, 3) if k["ms"] > 0 else None
            k["bytes"] = int(k["bytes"])
    out["lora_kernels"] = kernels
    for v in variants:
        if v != "trainable" and "trainable" in out:
            out[f"{v}_over_trainable"] = round(out[v]["median_ms"] / out["trainable"]["median_ms"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
