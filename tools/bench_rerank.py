#!/usr/bin/env python3
"""Measurement aid for candidate re-ranking with the local similarity (bench.py measures training and stays as it is).  One JSON
line per run, on random bf16 features at cfg2's local geometry (196 regions, 77 words, width 768), K = 16 candidates per query.

  python tools/bench_rerank.py            N = 1024 and N = 8192, each in a child process of its own under `timeout -k 10`, stopping at the
                                          first that fails
  python tools/bench_rerank.py --n 1024   one evaluation set of N pairs:
      pairs_i2t / pairs_t2i   the medmoe_local_sim_pairs launches of one direction (every image chunk, every length class; tables on the
                              device, Gram matrices in place) - and pairs/s = N K / time
      all_pairs_block         medmoe_local_sim_fwd over one 1024 x 1024 block (every length class; Gram matrices and word norms in place),
                              alternated with the pair launches in the same process - and pairs/s = 1024^2 / time
      gram                    the Gram GEMMs of all N images, `chunk` at a time
      metrics_global / metrics_local   retrieval_metrics without and with `local` (host work, table uploads and the Gram GEMMs included)

Times are device-event times (host clock around a device synchronise for the two metrics calls) around `--iters` calls after `--warmup`
calls, repeated `--repeats` times: median, quartiles, min and max of the repeats."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, T, D, K = 196, 77, 768, 16


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


def wall(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    return {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "repeats": len(ms)}


def run(a):
    import numpy as np
    import torch
    from medmoe_amd import ops
    from medmoe_amd.local_transposed import LocalSimScratch, local_gram, local_word_norms
    from medmoe_amd.retrieval import EmbeddingBank, LocalBank, build_pair_units, retrieval_metrics
    dev, N, chunk = torch.device("cuda:0"), a.n, min(a.chunk, a.n)
    g = torch.Generator(device=dev).manual_seed(777)
    bank, lb = EmbeddingBank(D, dev, capacity=N), LocalBank(P, T, D, dev, capacity=N)
    for s in range(0, N, 1024):
        n = min(1024, N - s)
        e = torch.randn(n, D, generator=g, device=dev)
        bank.add(e, e + 0.5 * torch.randn(n, D, generator=g, device=dev))
        lb.add_features(0.3 * torch.randn(n, P, D, generator=g, device=dev), 0.3 * torch.randn(n, T, D, generator=g, device=dev),
                        torch.randint(8, T + 1, (n,), generator=g, device=dev).to(torch.int32))
    lens_host = lb.cap_lens.cpu().numpy().astype(np.int64)
    GR = (P + 31) // 32 * 32
    scratch = LocalSimScratch(chunk, P, dev)
    gm_all = torch.zeros(N * GR, GR, device=dev, dtype=torch.bfloat16)          # every image's Gram matrix in place: the pair launches alone are timed
    ctx_all = lb.img_l.view(N * P, D)

    def gram():
        for lo in range(0, N, chunk):
            n = min(chunk, N - lo)
            local_gram(ctx_all[lo * P:(lo + n) * P], gm_all[lo * GR:(lo + n) * GR], **scratch.gram_kw(n))
    gram()
    wn = torch.empty(N, T, device=dev, dtype=torch.float32)
    d_perm, classes = local_word_norms(lb.words, lens_host, wn, P)
    out = {"n": N, "k": K, "chunk": chunk, "unit_cap": a.unit_cap, "mean_cap_len": float(lens_host.mean())}
    out["gram"] = stats(timed(gram, a.warmup, a.iters, a.repeats))

    # the pair launches of a direction, tables on the device
    loc = torch.empty(N * K, device=dev, dtype=torch.float32)
    launches = {}
    for name, q, keys, q_is_img in (("i2t", bank.img, bank.txt, True), ("t2i", bank.txt, bank.img, False)):
        idx = ops.sim_topk(q, keys, K)[1]
        todo, units_n, per_unit = [], 0, []
        for ntt, (units, pc, ps) in build_pair_units(idx, q_is_img, lens_host, T, a.unit_cap).items():
            assert units[:, 0].min() >= 0 and units[:, 0].max() < N and pc.min() >= 0 and pc.max() < N and ps.min() >= 0 and ps.max() < N * K
            assert (((lens_host[pc] + 15) // 16) == ntt).all() and (units[:, 1] + units[:, 2]).max() <= pc.shape[0]
            todo.append((ntt, units.shape[0], *(torch.from_numpy(x).to(dev) for x in (units, pc, ps))))
            units_n += units.shape[0]; per_unit += units[:, 2].tolist()
        launches[name] = todo
        out[f"units_{name}"] = {"units": units_n, "mean_entries_per_unit": round(float(np.mean(per_unit)), 2)}

    def pairs(name):
        def fn():
            for ntt, n_units, units, pc, ps in launches[name]:
                ops.call("local_sim_pairs", ctx_all, lb.words, lb.cap_lens, gm_all, wn, loc, units, n_units, pc, ps, N, N, P, T, D, lb.temp1, lb.temp2,
                         1e-8, ntt)
        return fn

    # the all-pairs kernel over one 1024 x 1024 block
    nb = min(1024, N)
    wn_b = torch.empty(nb, T, device=dev, dtype=torch.float32)
    perm_b, classes_b = local_word_norms(lb.words[:nb], lens_host[:nb], wn_b, P)
    sim = torch.empty(nb, nb, device=dev, dtype=torch.float32)

    def block():
        for ntt, start, n_c, _ in classes_b:
            ops.call("local_sim_fwd", ctx_all[:nb * P], lb.words[:nb], lb.cap_lens[:nb], gm_all[:nb * GR], wn_b, sim, nb, nb, P, T, D, lb.temp1, lb.temp2,
                     1e-8, perm_b[start:start + n_c], n_c, ntt)

    t = {"i2t": [], "t2i": [], "block": []}
    for _ in range(a.repeats):                                   # alternating: all three see the same neighbours on a shared host
        t["i2t"] += timed(pairs("i2t"), a.warmup, a.iters, 1)
        t["t2i"] += timed(pairs("t2i"), a.warmup, a.iters, 1)
        t["block"] += timed(block, 1, 1, 1)
    for name in ("i2t", "t2i"):
        out[f"pairs_{name}"] = {**stats(t[name]), "pairs_per_s": round(N * K / (1e-3 * statistics.median(t[name])), 1)}
    out["all_pairs_block"] = {**stats(t["block"]), "block": nb, "pairs_per_s": round(nb * nb / (1e-3 * statistics.median(t["block"])), 1)}
    torch.cuda.synchronize()
    del gm_all                                                   # the metrics below bring their own chunk-sized workspace
    out["metrics_global"] = stats(wall(lambda: retrieval_metrics(bank, (1, 5, 10)), 1, a.repeats))
    out["metrics_local"] = stats(wall(lambda: retrieval_metrics(bank, (1, 5, 10), local=lb, local_k=K, local_chunk=chunk), 1, a.repeats))
    out["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, help="pairs in the evaluation set (default: the driver, 1024 then 8192)")
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--unit-cap", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child process (driver mode)")
    a = ap.parse_args()
    if a.n:
        print(json.dumps(run(a)), flush=True)
        return 0
    for n in (1024, 8192):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--n", str(n), "--chunk", str(a.chunk),
               "--unit-cap", str(a.unit_cap), "--warmup", str(a.warmup), "--iters", str(a.iters), "--repeats", str(a.repeats)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:                                              # a fault, an abort or a time limit: nothing more is started on the GPU
            print(json.dumps({"n": n, "failed_with": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
