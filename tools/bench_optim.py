"""Time the two optimiser kernels on one arena: medmoe_adam_step against medmoe_adam_groups_step, on the ParamStore arena of a configuration
(default cfg2), with (a) a one-run table and (b) the run table of configs/experiment/pretraining_medmoe_cfg2_adamw.yaml (no_decay_1d,
layer_decay 0.75).  Each configuration runs in a fresh child process; inside it the two kernels ALTERNATE, every launch between its own pair
of HIP events, after a warm-up of both; reported are the median, the 10th / 90th percentile and the achieved bytes per second of the
34 B / element both kernels move.  Both kernels update the same buffers in place (their values do not matter to the time).
LAMB's three launches (medmoe_lamb_moments / _ratios / _apply) join the same alternation on the same arena and groups: together, as
a step issues them (`lamb`, TB/s of 42 B / element), and each alone (24 B, a few KB, 18 B per element).

    python tools/bench_optim.py [--config cfg2] [--launches 40] [--warmup 5] [--other-lib path/to/another/libmedmoe_hip.so]

One JSON line per configuration.  Needs the GPU: there is no other path."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: no GPU")
    from medmoe_amd import ops
    from medmoe_amd.config import config_by_name
    from medmoe_amd.optim_groups import GroupRules, apply_rules
    from medmoe_amd.params import ParamStore
    st = ParamStore(config_by_name(args.config), "cuda:0")
    if args.table == "experiment":
        apply_rules({"vit": st}, GroupRules(no_decay_1d=True, layer_decay=0.75))
        ends, lrm, wdm = st._run_table
    else:
        ends, lrm, wdm = st._upload_runs([(st.numel, 1.0, 1.0)])
    n, n_runs = st.numel, int(ends.numel())
    st.g32.normal_(0.0, 0.01, generator=torch.Generator(device="cuda").manual_seed(0))
    m, v = st.adam_state()
    nsq = st.sumsq()
    step = [0]

    def plain():
        step[0] += 1
        ops.call("adam_step", st.p32, st.g32, m, v, st.p16, n, 5e-5, 0.9, 0.999, 1e-8, 0.0, step[0], nsq, 0.25, 1.0)

    def grouped():
        step[0] += 1
        ops.call("adam_groups_step", st.p32, st.g32, m, v, st.p16, n, ends, lrm, wdm, n_runs, 5e-5, 0.9, 0.98, 1e-6, 0.05, 1, step[0], nsq, 0.25, 1.0)

    # LAMB: its three launches on the same buffers with the same groups - together (what a step issues) and each alone
    st.segments()
    s_ends, s_lrm, s_wdm, s_base = st._seg_table
    n_seg = int(s_ends.numel())
    scratch = torch.zeros(max(ops.lamb_scratch_floats(n, n_seg), 2), device="cuda:0")
    ratios = torch.ones(3 * n_seg, device="cuda:0")

    def l_moments():
        step[0] += 1
        ops.call("lamb_moments", st.p32, st.g32, m, v, n, s_ends, s_wdm, s_base, n_seg, scratch, scratch.numel(), 0.9, 0.999, 1e-6, 0.01, step[0],
                 nsq, 1.0, 1.0)

    def l_ratios():
        ops.call("lamb_ratios", scratch, scratch.numel(), s_ends, s_wdm, s_base, n_seg, n, 0.01, 0, 0, ratios)

    def l_apply():
        ops.call("lamb_apply", st.p32, m, v, st.p16, n, s_ends, s_lrm, s_wdm, n_seg, ratios, 1e-3, 0.9, 0.999, 1e-6, 0.01, max(step[0], 1))

    def lamb():
        l_moments(); l_ratios(); l_apply()

    cands = [("plain", plain), ("grouped", grouped), ("lamb", lamb), ("lamb_moments", l_moments), ("lamb_ratios", l_ratios),
             ("lamb_apply", l_apply)]
    nbytes = {"lamb": 42.0, "lamb_moments": 24.0, "lamb_ratios": 0.0, "lamb_apply": 18.0}     # B / element; the Adam kernels move 34
    if args.other_lib:                                              # medmoe_adam_step of another build of the library (a parent commit's)
        import ctypes
        f = ctypes.CDLL(os.path.abspath(args.other_lib)).medmoe_adam_step
        f.argtypes = [ops._CTYPES[ch] for ch in ops._SIGS["adam_step"]] + [ctypes.c_void_p]
        f.restype = ctypes.c_int

        def other():
            step[0] += 1
            rc = f(st.p32.data_ptr(), st.g32.data_ptr(), m.data_ptr(), v.data_ptr(), st.p16.data_ptr(), n, 5e-5, 0.9, 0.999, 1e-8, 0.0, step[0],
                   nsq.data_ptr(), 0.25, 1.0, ops.current_stream_handle())
            if rc != 0:
                raise RuntimeError(f"medmoe_adam_step of {args.other_lib}: error {rc}")
        cands.insert(0, ("plain_other_lib", other))
    for _ in range(args.warmup):
        for _, fn in cands:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cands}
    for _ in range(args.launches):
        for name, fn in cands:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    out = {"config": args.config, "table": args.table, "numel": n, "n_runs": n_runs, "n_segments": n_seg, "launches": args.launches,
           "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        ts = sorted(ts)
        med = statistics.median(ts)
        out[name] = {"median_ms": round(med, 4), "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[(len(ts) * 9) // 10], 4),
                     "min_ms": round(ts[0], 4), "TB_per_s": round(nbytes.get(name, 34.0) * n / (med * 1e-3) / 1e12, 3)}
    out["grouped_over_plain"] = round(out["grouped"]["median_ms"] / out["plain"]["median_ms"], 4)
    out["lamb_over_grouped"] = round(out["lamb"]["median_ms"] / out["grouped"]["median_ms"], 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--other-lib", default=None, help="a second libmedmoe_hip.so: its medmoe_adam_step is timed in the same alternation")
    ap.add_argument("--table", choices=["one", "experiment"], default=None, help="(child) the run table to time")
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches: at least 20 (the median of fewer is noise)")
    if args.table is not None:
        return child(args)
    for table in ("one", "experiment"):                             # a fresh process per configuration
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", args.config, "--launches", str(args.launches),
                             "--warmup", str(args.warmup), "--table", table] + (["--other-lib", args.other_lib] if args.other_lib else [])).returncode
        if rc != 0:
            raise SystemExit(rc)


if __name__ == "__main__":
    main()
