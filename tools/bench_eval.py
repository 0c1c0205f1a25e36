#!/usr/bin/env python3
"""Measurement aid for the evaluation step (bench.py measures training and stays as it is).  One JSON line per run.

  python tools/bench_eval.py                      every part below (sim-error once, the timed parts at cfg2, batch 1024 and 128), each in a
                                                  child process of its own under `timeout -k 10`, stopping at the first that fails
  python tools/bench_eval.py --part step          (a) Engine.eval_step: ms per step, torch.cuda.max_memory_allocated
  python tools/bench_eval.py --part local         (b) the local-loss forward through medmoe_local_sim_fwd and (c) through medmoe_local_scores_t +
                                                  the forward launch of medmoe_local_pair3, alternating on the same inputs; max |sim_b - sim_c|
  python tools/bench_eval.py --part model_step    (d) module.model_step under no_grad: ms per step, peak memory
  python tools/bench_eval.py --part sim-error     max abs error of the existing path's and the new kernel's sim against the fp32 oracle on
                                                  the inputs of tests/test_eval_step_gpu.py (the source of that test's constants)

Times are device-event times around `--iters` calls after `--warmup` calls, repeated `--repeats` times: median, quartiles, min and max
of the repeats are reported, so a difference can be held against the spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, iters, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "repeats": len(ms)}


def part_step(a):
    import torch
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name(a.config)
    eng = Engine(cfg, "cuda:0", seed=0)
    b = bench.synthetic_batch(cfg, a.batch, 777, eng.device)
    torch.cuda.reset_peak_memory_stats()
    ms = timed(lambda: eng.eval_step(b), a.warmup, a.iters, a.repeats)
    return {"part": "eval_step", **stats(ms), "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), "pair_cap": eng._local.cap}


def part_local(a):
    import torch
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    from medmoe_amd.local_transposed import TransposedLocalLoss, local_sim_forward
    cfg = config_by_name(a.config)
    eng = Engine(cfg, "cuda:0", seed=0)
    b = bench.synthetic_batch(cfg, a.batch, 777, eng.device)
    eng._alloc(a.batch)
    eng.prefetch_cap_lens(b["ids"])
    eng._forward_both(b)
    ws, B, P, T, Do = eng.ws, a.batch, cfg.n_patch, cfg.max_len, cfg.d_out
    ctx, caps_host = ws["img_l"].view(B * P, Do), eng._cap_lens_host()
    sim_new = torch.empty(B, B, device=eng.device)
    tl = TransposedLocalLoss(B, P, T, Do, eng.device, gram=eng.local_gram, pitch=eng.HWq)
    new = lambda: local_sim_forward(ctx, ws["words"], eng.cap_lens, caps_host, cfg.temp1, cfg.temp2, P=P, gm3=tl.gm3,
                                    gm3_crowmap=tl.gm3_crowmap, img_tiles=tl.img_tiles, img_tile_count=tl.img_tile_count,
                                    wn=tl.wn, sim=sim_new)
    old = lambda: tl.forward(ctx, ws["words"], eng.cap_lens, caps_host, cfg.temp1, cfg.temp2)
    new(); old()
    torch.cuda.synchronize()
    diff = float((sim_new - tl.sim).abs().max())
    t_new, t_old = [], []
    for _ in range(a.repeats):                                   # alternating: both see the same neighbours on a shared host
        t_new += timed(new, a.warmup, a.iters, 1)
        t_old += timed(old, a.warmup, a.iters, 1)
    return {"part": "local_forward", "new_sim_fwd": stats(t_new), "old_scores_pair3_fwd": stats(t_old), "max_abs_sim_diff": diff,
            "mean_cap_len": float(caps_host.mean())}


def part_model_step(a):
    import torch
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.hydra_lite import compose, instantiate
    os.environ.setdefault("PROJECT_ROOT", ROOT)
    over = [f"experiment=pretraining_medmoe_{a.config}"] if a.config.startswith("cfg") else ["experiment=pretraining_medmoe_cfg2", f"model.model.vision.config_name={a.config}"]
    lit = instantiate(compose(os.path.join(ROOT, "configs"), "train.yaml", over).model)
    cfg = config_by_name(a.config)
    b = bench.synthetic_batch(cfg, a.batch, 777, lit.model.engine.device)
    mb = {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"]}}

    def step():
        with torch.no_grad():
            return lit.model_step(mb)
    torch.cuda.reset_peak_memory_stats()
    ms = timed(step, a.warmup, a.iters, a.repeats)
    return {"part": "model_step_no_grad", **stats(ms), "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}


def part_sim_error(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_eval_step_gpu as t
    out = {"part": "sim_error"}
    for name, case in (("fixture64", t.fixture_case(os.path.join(ROOT, "tests", "golden"))[:3]), ("seeded196", t.seeded_case())):
        ref = t.oracle_sim(*case)
        out[name] = {"existing_path_max_abs_err": float((t.old_sim(*case).cpu() - ref).abs().max()),
                     "local_sim_fwd_max_abs_err": float((t.new_sim(*case).cpu() - ref).abs().max()), "max_abs_sim": float(ref.abs().max())}
    return out


PARTS = {"step": part_step, "local": part_local, "model_step": part_model_step, "sim-error": part_sim_error}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=sorted(PARTS))
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child process (driver mode)")
    a = ap.parse_args()
    if a.part:
        r = PARTS[a.part](a)
        r.update(config=a.config, batch=a.batch, warmup=a.warmup, iters=a.iters)
        print(json.dumps(r), flush=True)
        return 0
    jobs = [("sim-error", a.batch)] + [(part, batch) for batch in (1024, 128) for part in ("local", "step", "model_step")]
    for part, batch in jobs:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--part", part, "--config", a.config,
               "--batch", str(batch), "--warmup", str(a.warmup), "--iters", str(a.iters), "--repeats", str(a.repeats)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:                                          # a fault, an abort or a time limit: nothing more is started on the GPU
            print(json.dumps({"part": part, "batch": batch, "failed_with": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
