"""What the weight EMA of the fused step costs, two measurements on one box:

  launch   medmoe_adam_step against medmoe_adam_step_ema (and the grouped pair under the run table of pretraining_medmoe_cfg2_adamw.yaml) on the
           ParamStore arena of a configuration (default cfg2), ALTERNATED launch by launch, every launch between its own pair of HIP events,
           after a warm-up of all; the median, the 10th / 90th percentile and the achieved bytes per second of the 34 / 42 B per element
           the two move.  All update the same buffers in place (their values do not matter to the time).
  step     one training step with ema_decay = 0 and with `--decay`, ALTERNATED per round at each batch size of `--batches` (default 1024 and
           128): every round builds the two engines one after the other (one alive at a time), warms each up and times `--steps` steps as
           bench.py times a step (the parameters restored from a snapshot before the start event, HIP events around train_step); reported
           per mode the median / min / max over all rounds and the peak allocated memory.

    python tools/bench_ema.py [--config cfg2] [--what launch,step] [--launches 40] [--batches 1024,128] [--decay 0.9999] [--rounds 3] [--steps 5]

One JSON line per measurement.  Needs the GPU: there is no other path."""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_launch(args, torch):
    from medmoe_amd import ops
    from medmoe_amd.config import config_by_name
    from medmoe_amd.ema import one_minus_decay
    from medmoe_amd.optim_groups import GroupRules, apply_rules
    from medmoe_amd.params import ParamStore
    st = ParamStore(config_by_name(args.config), "cuda:0")
    apply_rules({"vit": st}, GroupRules(no_decay_1d=True, layer_decay=0.75))
    ends, lrm, wdm = st._run_table
    n, n_runs = st.numel, int(ends.numel())
    st.g32.normal_(0.0, 0.01, generator=torch.Generator(device="cuda").manual_seed(0))
    m, v = st.adam_state()
    st.enable_ema()
    nsq = st.sumsq()
    omd = one_minus_decay(10 ** 6, args.decay)
    step = [0]

    def plain(sfx, *extra):
        def fn():
            step[0] += 1
            ops.call("adam_step" + sfx, st.p32, st.g32, m, v, st.p16, n, 5e-5, 0.9, 0.999, 1e-8, 0.0, step[0], nsq, 0.25, 1.0, *extra)
        return fn

    def grouped(sfx, *extra):
        def fn():
            step[0] += 1
            ops.call("adam_groups_step" + sfx, st.p32, st.g32, m, v, st.p16, n, ends, lrm, wdm, n_runs, 5e-5, 0.9, 0.98, 1e-6, 0.05, 1, step[0],
                     nsq, 0.25, 1.0, *extra)
        return fn

    cands = [("plain", plain(""), 34.0), ("plain_ema", plain("_ema", st.e32, omd), 42.0),
             ("grouped", grouped(""), 34.0), ("grouped_ema", grouped("_ema", st.e32, omd), 42.0)]
    for _ in range(args.warmup):
        for _, fn, _ in cands:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cands}
    for _ in range(args.launches):
        for name, fn, _ in cands:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    out = {"what": "launch", "config": args.config, "numel": n, "n_runs": n_runs, "launches": args.launches, "device": torch.cuda.get_device_name(0)}
    for name, _, nbytes in cands:
        ts = sorted(times[name])
        med = statistics.median(ts)
        out[name] = {"median_ms": round(med, 4), "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[(len(ts) * 9) // 10], 4),
                     "min_ms": round(ts[0], 4), "B_per_element": nbytes, "TB_per_s": round(nbytes * n / (med * 1e-3) / 1e12, 3)}
    out["plain_ema_over_plain"] = round(out["plain_ema"]["median_ms"] / out["plain"]["median_ms"], 4)
    out["grouped_ema_over_grouped"] = round(out["grouped_ema"]["median_ms"] / out["grouped"]["median_ms"], 4)
    print(json.dumps(out), flush=True)
    del st, m, v
    gc.collect(); torch.cuda.empty_cache()


def bench_step(args, torch):
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    modes = {"ema_off": 0.0, "ema_on": args.decay}
    out = {"what": "step", "config": args.config, "decay": args.decay, "rounds": args.rounds, "steps": args.steps, "warmup": args.step_warmup,
           "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        times, peak = {m: [] for m in modes}, {m: 0 for m in modes}
        for _ in range(args.rounds):
            for mode, decay in modes.items():
                torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                cfg = config_by_name(args.config)
                cfg.ema_decay, cfg.ema_warmup = decay, decay > 0.0
                eng = Engine(cfg, "cuda:0", seed=0)
                batch = bench.synthetic_batch(eng.cfg, B, 12345, eng.device)
                start = bench.StepStart(eng)
                for _ in range(args.step_warmup):
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
                assert (eng.params.e32 is not None) == (decay > 0.0) and eng.params.ema_updates == (args.step_warmup + args.steps if decay > 0.0 else 0)
                del eng, batch, start
                gc.collect()
        res = {}
        for m in modes:
            ts = sorted(times[m])
            res[m] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3),
                      "peak_GB": round(peak[m] / 2 ** 30, 3)}
        res["on_minus_off_ms"] = round(res["ema_on"]["median_ms"] - res["ema_off"]["median_ms"], 3)
        res["on_over_off"] = round(res["ema_on"]["median_ms"] / res["ema_off"]["median_ms"], 4)
        out["batches"][str(B)] = res
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--what", default="launch,step")
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5, help="warm-up launches of every kernel")
    ap.add_argument("--batches", default="1024,128")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--step-warmup", type=int, default=2, help="warm-up steps of every engine")
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches: at least 20 (the median of fewer is noise)")
    if not 0.0 < args.decay < 1.0:
        ap.error("--decay: in (0, 1)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema: no GPU")
    what = args.what.split(",")
    if "launch" in what:
        bench_launch(args, torch)
    if "step" in what:
        bench_step(args, torch)


if __name__ == "__main__":
    main()
