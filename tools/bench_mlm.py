"""Time the masked-language-model launches, ALTERNATED in one process with what they replace:

  1. kernels   the fused decoder + cross-entropy - ops.vocab_ce_fwd, then ops.vocab_ce_bwd (dz, dE, dbias) - against the MATERIALISING form
               on the same operands: ops.gemm_nt into fp32 logits [M, V], torch.logsumexp, softmax minus one-hot rounded to bf16, and the two
               GEMMs (ops.gemm_nt for dz = P E on a transposed copy of E, ops.gemm_tn for dE = P^T z).  Default M = 6144, V = 28996,
               D = 768.  Reported per arm: median / min / max milliseconds, TFLOP/s on the algorithm's count (forward 2 M V D, backward
               6 M V D for the fused arm - the score recompute in each of its two kernels and the two products - 4 M V D for the
               materialising one), and the peak of torch's allocator over the arm's calls (the operands are allocated before the window).
  2. step      Engine.train_step on cfg2 with a trainable text tower, text_mlm off and on, at the batches of `--batches` (default
               1024,128): one engine, the head taken away and put back between alternated steps.

Every call sits between its own pair of HIP events after a warm-up of every arm.  One JSON line.  Needs the GPU: there is no other path.

    python tools/bench_mlm.py [--rows 6144] [--vocab 28996] [--dim 768] [--rounds 7] [--step] [--batches 1024,128] [--no-kernels]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def _alternate(modes, rounds):
    import torch
    peak = {}
    for name, fn in modes.items():                                   # warm-up of every arm, and its allocator peak
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _timed(fn)
        peak[name] = torch.cuda.max_memory_allocated() - base
    times = {name: [] for name in modes}
    for _ in range(rounds):
        for name, fn in modes.items():
            times[name].append(_timed(fn)[0])
    return {name: {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "peak_bytes_over_operands": int(peak[name])}
            for name, t in times.items()}


def bench_kernels(M, V, D, rounds):
    import torch
    from medmoe_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + V)
    z = torch.randn(M, D, generator=g, device="cuda").bfloat16()
    E = (torch.randn(V, D, generator=g, device="cuda") * D ** -0.5).bfloat16()
    bias = torch.randn(V, generator=g, device="cuda") * 0.1
    labels = torch.randint(0, V, (M,), generator=g, device="cuda").to(torch.int32)
    count = torch.tensor([M], dtype=torch.int32, device="cuda")
    dE, dbias = torch.zeros(V, D, device="cuda"), torch.zeros(V, device="cuda")
    dz = torch.empty(M, D, device="cuda", dtype=torch.bfloat16)
    bufs = dict(lse=torch.empty(M, device="cuda"), terms=torch.empty(M, device="cuda"), loss=torch.empty(1, device="cuda"),
                counts=torch.empty(2, device="cuda", dtype=torch.int32), scratch=torch.empty(ops.vocab_ce_scratch(M, V, D), device="cuda"))
    Vp = (V + 63) // 64 * 64                                         # the dz GEMM contracts over V: the NT kernels want K in whole k-steps
    Et = torch.zeros(D, Vp, device="cuda", dtype=torch.bfloat16)
    Et[:, :V] = E.t()
    dEp, dbp = torch.zeros(Vp, D, device="cuda"), torch.zeros(Vp, device="cuda")      # the baseline's gradients, padded like its P
    lab64 = labels.long()
    state = {}

    def fused_fwd():
        return ops.vocab_ce_fwd(z, E, bias, labels, count, 1.0, **bufs)[0]

    def fused_bwd():
        ops.vocab_ce_bwd(z, E, bias, labels, bufs["lse"], count, 1.0, dz=dz, dE=dE, dbias=dbias)

    def mat_fwd():
        logits = torch.empty(M, V, device="cuda")
        ops.gemm_nt(z, E, logits, bias=bias)
        lse = torch.logsumexp(logits, dim=1)
        state["logits"], state["lse"] = logits, lse
        return (lse - logits.gather(1, lab64[:, None])[:, 0]).mean()

    def mat_bwd():
        logits, lse = state["logits"], state["lse"]
        p = torch.exp(logits - lse[:, None])
        p[torch.arange(M, device="cuda"), lab64] -= 1.0
        p16 = torch.zeros(M, Vp, device="cuda", dtype=torch.bfloat16)
        p16[:, :V] = (p / M).bfloat16()
        out = torch.empty(M, D, device="cuda", dtype=torch.bfloat16)
        ops.gemm_nt(p16, Et, out)
        ops.gemm_tn(p16, z, dEp, db=dbp)
        return out

    rec = _alternate({"fused_fwd": fused_fwd, "materialising_fwd": mat_fwd, "fused_bwd": fused_bwd, "materialising_bwd": mat_bwd}, rounds)
    mvd = 2.0 * M * V * D
    for name, k in (("fused_fwd", 1), ("materialising_fwd", 1), ("fused_bwd", 3), ("materialising_bwd", 2)):
        rec[name]["tflops"] = k * mvd / (rec[name]["ms_median"] * 1e-3) / 1e12
    rec["loss_fused"], rec["loss_materialising"] = float(fused_fwd()), float(mat_fwd())
    dE.zero_(); dbias.zero_()
    fused_bwd()
    a = dE.clone()
    dEp.zero_(); dbp.zero_()
    ref = mat_bwd()
    rec["dE_rel_l2_between_arms"] = float((a - dEp[:V]).norm() / dEp[:V].norm())
    rec["dz_rel_l2_between_arms"] = float((dz.float() - ref.float()).norm() / ref.float().norm())
    rec["shape"] = {"M": M, "V": V, "D": D}
    rec["logits_bytes_not_written_by_the_fused_arm"] = 4 * M * V
    return rec


def bench_step(batches, rounds):
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    out = {}
    import torch
    for B in batches:
        # ONE engine (two trainable-text engines of cfg2 at batch 1024 do not fit next to each other): every switch of the feature in the
        # engine is `self.mlm is not None`, so a step with the head taken away is the step of an engine built without it
        cfg = config_by_name("cfg2")
        cfg.freeze_text, cfg.text_mlm = False, True
        eng = Engine(cfg, "cuda:0")
        head = eng.mlm
        b = bench.synthetic_batch(cfg, B, 0, eng.device)

        def step(on):
            eng.mlm = head if on else None
            return eng.train_step(b)

        rec = _alternate({"mlm_off": lambda: step(False), "mlm_on": lambda: step(True)}, rounds)
        eng.mlm = head
        rec["masked_tokens"] = int(head.buf.counts[0])
        rec["tokens"] = int(b["attn_mask"].sum())
        out[f"batch{B}"] = rec
        del eng, head, b
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6144)
    ap.add_argument("--vocab", type=int, default=28996)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true", help="also time train_step on cfg2 (trainable text tower) with text_mlm off and on")
    ap.add_argument("--batches", default="1024,128")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlm: no GPU")
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    if not args.no_kernels:
        out["kernels"] = bench_kernels(args.rows, args.vocab, args.dim, args.rounds)
    if args.step:
        out["step"] = bench_step([int(b) for b in args.batches.split(",")], args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
