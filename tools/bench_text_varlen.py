"""Time one training step of a configuration (default cfg2) in five text modes - frozen tower, fully trainable tower padded / packed
(text_train_varlen), LoRA adapters padded / packed - ALTERNATED on one box, at each batch size of `--batches` (default 1024 and
128): every round builds the modes' engines one after the other (one engine alive at a time), warms each up and times `--steps` steps as
bench.py times a step (the parameters restored from a snapshot before the start event, HIP events around train_step); the rounds repeat, so a
drift of the box shows in every mode alike.  Reported per batch and mode: the median / min / max step time over all rounds and the peak
allocated memory; and for the two fully trainable modes the per-kernel table of one extra step with every launch between its own pair of
events (the text tower's launches carry no tag of their own: the table holds every label, the text side shows in the differences).

    python tools/bench_text_varlen.py [--config cfg2] [--batches 1024,128] [--rounds 3] [--steps 5] [--warmup 2] [--modes ...]
                                      [--hidden-dropout 0.1] [--dropout 0.1] [--rank 8] [--top 24]

One JSON line.  Needs the GPU: there is no other path."""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("frozen", "full_padded", "full_packed", "lora_padded", "lora_packed")


def build(mode, args):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name(args.config)
    if mode.startswith("full"):
        cfg.freeze_text = False
    elif mode.startswith("lora"):
        cfg.text_lora, cfg.text_lora_r, cfg.text_lora_alpha, cfg.text_lora_dropout = True, args.rank, 2.0 * args.rank, args.dropout
    cfg.text_train_varlen = mode.endswith("packed")
    if mode != "frozen":
        cfg.text_hidden_dropout = args.hidden_dropout
    return Engine(cfg, "cuda:0", seed=0)


def kernel_table(prof, top):
    rows = {}
    for label, _, _, e0, e1, _ in prof:
        k = rows.setdefault(label, [0, 0.0])
        k[0] += 1; k[1] += e0.elapsed_time(e1)
    order = sorted(rows.items(), key=lambda kv: -kv[1][1])[:top]
    return {label: {"launches": n, "ms": round(ms, 3)} for label, (n, ms) in order}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--batches", default="1024,128")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.0, help="LoRA dropout of the two LoRA modes")
    ap.add_argument("--hidden-dropout", type=float, default=0.0, help="hidden dropout of the four trainable modes (its launches run over all rows)")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--top", type=int, default=24, help="rows of the per-kernel tables")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_varlen: no GPU")
    import bench
    from medmoe_amd import ops
    modes = [m for m in args.modes.split(",") if m]
    out = {"config": args.config, "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup, "hidden_dropout": args.hidden_dropout, "lora_dropout": args.dropout, "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        times, peak, kernels, tokens = {m: [] for m in modes}, {m: 0 for m in modes}, {}, None
        for rnd in range(args.rounds):
            for mode in modes:
                torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                eng = build(mode, args)
                if eng.lora is not None:                           # B = 0 would leave d A = 0: the arithmetic should be live
                    lo = eng.lora
                    g = torch.Generator().manual_seed(1)
                    lo.load_named({"text." + n: 0.02 * torch.randn(lo.D, lo.r, generator=g) for n in lo.true_names() if n.endswith("lora_B")})
                batch = bench.synthetic_batch(eng.cfg, B, 12345, eng.device)
                tokens = float(batch["attn_mask"].float().sum(1).mean())
                start = bench.StepStart(eng)
                for _ in range(args.warmup):
                    start.restore()
                    eng.train_step(batch)
                torch.cuda.synchronize()
                assert eng.text_train_varlen_active == mode.endswith("packed"), mode
                spans = []
                for _ in range(args.steps):
                    start.restore()                                # before the start event: outside the timed span
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); eng.train_step(batch); b.record()
                    spans.append((a, b))
                torch.cuda.synchronize()
                times[mode] += [a.elapsed_time(b) for a, b in spans]
                peak[mode] = max(peak[mode], torch.cuda.max_memory_allocated() - start.nbytes)
                if mode.startswith("full") and rnd == args.rounds - 1:
                    ops.ROWS_HINT = int(batch["attn_mask"].sum()) if mode.endswith("packed") else 0
                    ops.PROFILE = []
                    start.restore()
                    eng.train_step(batch)
                    torch.cuda.synchronize()
                    kernels[mode] = kernel_table(ops.PROFILE, args.top)
                    ops.PROFILE, ops.ROWS_HINT = None, 0
                del eng, batch, start
                gc.collect()
        res = {"mean_tokens": round(tokens, 2)}
        for m in modes:
            ts = sorted(times[m])
            res[m] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3),
                      "peak_GB": round(peak[m] / 2 ** 30, 3)}
        for a, b in (("full_packed", "full_padded"), ("lora_packed", "lora_padded")):
            if a in res and b in res:
                res[a + "_over_padded"] = round(res[a]["median_ms"] / res[b]["median_ms"], 4)
        res["kernels"] = kernels
        out["batches"][str(B)] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
