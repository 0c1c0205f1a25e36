"""Time the streaming retrieval kernels next to what a user would write without them, ALTERNATED in one process at D = 768 and
Nq = Nk = N for each N of `--sizes` (default 1024, 8192, 32768), on seeded unit rows:

    sim_topk   ops.sim_topk(q, keys, K = 10): the K best keys per query, no [N, N] matrix
    sim_rank   ops.sim_rank(q, keys, arange(N)): the rank of the paired key per query, no list and no matrix
    baseline   medmoe_sgemm into an fp32 [N, N] matrix, then torch.topk(K = 10) on it - existing code, the yardstick

Every call sits between its own pair of HIP events, after a warm-up of every mode; per size and mode the tool reports the median / min / max
milliseconds over the rounds, the peak device memory the mode allocated on top of the inputs, and - for the two kernels and for the
baseline's GEMM alone - the achieved FLOP/s (2 N^2 D) against the 157.3 TFLOP/s fp32-matrix peak of the MI355X.  `agree` is the share of
(query, position) pairs at which the kernel's and the baseline's index lists coincide (the baseline's scores are another summation order, so
near ties may swap).

    python tools/bench_retrieval.py [--sizes 1024,8192,32768] [--dim 768] [--k 10] [--rounds 5]

One JSON line.  Needs the GPU: there is no other path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MATRIX_PEAK = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,8192,32768")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval: no GPU")
    from medmoe_amd import ops
    D, K = args.dim, args.k
    out = {"dim": D, "k": K, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for N in (int(n) for n in args.sizes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(N)
        q = ops.l2_normalize(torch.randn(N, D, generator=g, device="cuda"))
        keys = ops.l2_normalize(torch.randn(N, D, generator=g, device="cuda"))
        target = torch.arange(N, device="cuda", dtype=torch.int32)
        flops = 2.0 * N * N * D
        gemm_ms = []

        def baseline():
            S = torch.empty(N, N, device="cuda", dtype=torch.float32)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.call("sgemm", q, keys, S, N, N, D, D, 1, 1, D, N, 1.0, 0.0)
            e1.record()
            res = torch.topk(S, K, dim=1)
            gemm_ms.append((e0, e1))
            return res

        modes = {"sim_topk": lambda: ops.sim_topk(q, keys, K), "sim_rank": lambda: ops.sim_rank(q, keys, target), "baseline": baseline}
        res, peak = {}, {}
        for name, fn in modes.items():                               # warm-up, and each mode's peak memory on top of the inputs
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            res[name] = fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
        gemm_ms.clear()
        agree = float((res["sim_topk"][1].long() == res["baseline"].indices).double().mean())
        res.clear()
        times = {name: [] for name in modes}
        for _ in range(args.rounds):
            for name, fn in modes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
                del r
        rec = {"agree": agree}
        for name, t in times.items():
            rec[name] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "peak_bytes": int(peak[name])}
            if name != "baseline":
                rec[name]["tflops"] = flops / (statistics.median(t) * 1e-3) / 1e12
                rec[name]["of_f32_matrix_peak"] = flops / (statistics.median(t) * 1e-3) / F32_MATRIX_PEAK
        gm = statistics.median(a.elapsed_time(b) for a, b in gemm_ms)
        rec["baseline"].update({"gemm_ms_median": gm, "gemm_tflops": flops / (gm * 1e-3) / 1e12, "gemm_of_f32_matrix_peak": flops / (gm * 1e-3) / F32_MATRIX_PEAK})
        out["sizes"][str(N)] = rec
        del q, keys, target
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
