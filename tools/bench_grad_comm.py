"""Time the kernels of the bf16 gradient exchange on the ParamStore arena of a configuration (default cfg2): the pack
(medmoe_grad_pack_bf16, whole arena in one launch, against its 6 B / element HBM floor), the clip norm over fp32 and bf16 gradients, and
medmoe_adam_step / medmoe_adam_groups_step (the run table of configs/experiment/pretraining_medmoe_cfg2_adamw.yaml) with fp32 against bf16
gradients.  All candidates ALTERNATE in one process, every launch between its own pair of HIP events, after a warm-up of all; reported are
the median, the 10th / 90th percentile and the achieved bytes per second of what each kernel moves.  The Adam kernels update the same
buffers in place (their values do not matter to the time).

    python tools/bench_grad_comm.py [--config cfg2] [--launches 40] [--warmup 5]

--step fp32|bf16 times whole training steps instead: Engine.train_step at --batch pairs (default 128, the 8-GPU point's per-rank batch) in a
one-rank "nccl" group with MEDMOE_DIST_WORLD1=1, so the packs and the all-reduces are launched for real (with no wire to win anything back on:
this is the cost of the added launches, not the gain).  --tree PATH imports the package from another checkout (a parent commit, built), for
an alternated comparison of fp32 steps across commits; each call is one process, alternate the calls.

    python tools/bench_grad_comm.py --step bf16 [--batch 128] [--steps 30] [--warmup 5] [--tree PATH]

One JSON line.  Needs the GPU: there is no other path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_mode(args):
    tree = os.path.abspath(args.tree) if args.tree else ROOT
    sys.path.insert(0, tree)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29559"), RANK="0", WORLD_SIZE="1",
                      MEDMOE_DIST_WORLD1="1")
    os.environ.pop("MEDMOE_GRAD_COMM", None)
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_comm: no GPU")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    torch.cuda.set_device(0)
    import bench
    import medmoe_amd
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    assert os.path.abspath(medmoe_amd.__file__).startswith(tree + os.sep), medmoe_amd.__file__
    cfg = config_by_name(args.config)
    if args.step == "bf16":
        cfg.grad_comm_dtype = "bf16"
    eng = Engine(cfg, "cuda:0", seed=0)
    assert eng.dist and eng.world == 1
    batch = bench.synthetic_batch(cfg, args.batch, 12345, eng.device)
    for _ in range(args.warmup):
        eng.train_step(batch)
    torch.cuda.synchronize()
    spans = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = eng.train_step(batch); b.record()
        spans.append((a, b))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in spans)
    print(json.dumps({"mode": "step", "grad_comm_dtype": args.step, "tree": tree, "config": args.config, "batch": args.batch, "steps": args.steps,
                      "median_ms": round(statistics.median(ts), 4), "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[(len(ts) * 9) // 10], 4),
                      "min_ms": round(ts[0], 4), "loss": float(out["loss"]), "numel": eng.params.numel, "device": torch.cuda.get_device_name(0)}),
          flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", choices=["fp32", "bf16"], default=None, help="time whole steps in a one-rank nccl group with this exchange")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--tree", default=None, help="(--step) import medmoe_amd and bench from this checkout instead of this one")
    args = ap.parse_args()
    if args.step is not None:
        return step_mode(args)
    if args.launches < 20:
        ap.error("--launches: at least 20 (the median of fewer is noise)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_comm: no GPU")
    from medmoe_amd import ops
    from medmoe_amd.config import config_by_name
    from medmoe_amd.optim_groups import GroupRules, apply_rules
    from medmoe_amd.params import ParamStore
    st = ParamStore(config_by_name(args.config), "cuda:0")
    apply_rules({"vit": st}, GroupRules(no_decay_1d=True, layer_decay=0.75))
    ends, lrm, wdm = st._run_table
    n, n_runs = st.numel, int(ends.numel())
    st.g32.normal_(0.0, 0.01, generator=torch.Generator(device="cuda").manual_seed(0))
    m, v = st.adam_state()
    g16 = st.g16
    st.pack(0, n, 0.125)
    nsq = st.sumsq().clone()
    step = [0]

    def adam(name, g):
        def f():
            step[0] += 1
            ops.call(name, st.p32, g, m, v, st.p16, n, 5e-5, 0.9, 0.999, 1e-8, 0.0, step[0], nsq, 0.25, 1.0)
        return f

    def groups(name, g):
        def f():
            step[0] += 1
            ops.call(name, st.p32, g, m, v, st.p16, n, ends, lrm, wdm, n_runs, 5e-5, 0.9, 0.98, 1e-6, 0.05, 1, step[0], nsq, 0.25, 1.0)
        return f

    # name -> (launch, bytes moved per element)
    cands = {
        "pack": (lambda: ops.call("grad_pack_bf16", st.g32, g16, n, 0.125), 6.0),
        "sumsq_fp32": (lambda: ops.call("sumsq_det", st.g32, n, st.normsq, st.norm_scratch), 4.0),
        "sumsq_bf16": (lambda: ops.call("sumsq_det_bf16", g16, n, st.normsq, st.norm_scratch), 2.0),
        "adam_fp32": (adam("adam_step", st.g32), 34.0),
        "adam_bf16": (adam("adam_step_g16", g16), 32.0),
        "adam_groups_fp32": (groups("adam_groups_step", st.g32), 34.0),
        "adam_groups_bf16": (groups("adam_groups_step_g16", g16), 32.0),
    }
    for _ in range(args.warmup):
        for fn, _ in cands.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.launches):
        for name, (fn, _) in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    out = {"config": args.config, "numel": n, "n_runs": n_runs, "launches": args.launches, "device": torch.cuda.get_device_name(0),
           "fp32_message_MB": round(4.0 * n / 1e6, 1), "bf16_message_MB": round(2.0 * n / 1e6, 1)}
    for name, ts in times.items():
        ts = sorted(ts)
        med = statistics.median(ts)
        out[name] = {"median_ms": round(med, 4), "p10_ms": round(ts[len(ts) // 10], 4), "p90_ms": round(ts[(len(ts) * 9) // 10], 4),
                     "min_ms": round(ts[0], 4), "bytes_per_element": cands[name][1], "TB_per_s": round(cands[name][1] * n / (med * 1e-3) / 1e12, 3)}
    for pair in ("adam", "adam_groups", "sumsq"):
        out[f"{pair}_bf16_over_fp32"] = round(out[f"{pair}_bf16"]["median_ms"] / out[f"{pair}_fp32"]["median_ms"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
