"""Time the classification launches next to what a user would write without them, ALTERNATED in one process:

  1. head      ops.cls_head_step (forward + loss + dz + dW + db, no dx: the linear probe's launch) against the torch composition
               F.linear + F.cross_entropy / F.binary_cross_entropy_with_logits + autograd on W and b, at D = 768, C = 5 (multiclass) and
               14 (multilabel), N of `--sizes` (default 8192, 65536, 262144).  Reported: median / min / max milliseconds, and the achieved
               share of the HBM bandwidth the MI355X sustains (6.29 TB/s, float4 copy) against the FLOOR of one read of the features,
               N D 4 bytes - the kernel reads them twice by design, so 50 % is its ceiling.
  2. auroc     ops.auroc_counts against a torch.sort-based midrank AUROC (per class: sort the counted scores, average the ranks of ties,
               Mann-Whitney U) at the same N and C.
  3. step      Engine.classify_step(train_tower=True) against Engine.train_step on cfg2 at batch 128 (`--step`; seeded synthetic batch).

Every call sits between its own pair of HIP events after a warm-up of every mode.  One JSON line.  Needs the GPU: there is no other path.

    python tools/bench_classify.py [--sizes 8192,65536,262144] [--rounds 7] [--step] [--no-kernels]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SUSTAINED = 6.29e12


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def _alternate(modes, rounds):
    for fn in modes.values():                                        # warm-up of every mode
        _timed(fn)
    times = {name: [] for name in modes}
    for _ in range(rounds):
        for name, fn in modes.items():
            times[name].append(_timed(fn)[0])
    return {name: {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)} for name, t in times.items()}


def midrank_auroc_torch(scores, targets):
    """Per-class midrank AUROC by sorting (what a user would write in torch): float64 [C], NaN for a one-sided class."""
    import torch
    out = []
    for c in range(scores.shape[1]):
        keep = targets[:, c] >= 0
        s, t = scores[keep, c], targets[keep, c]
        n_pos = int((t == 1).sum())
        n_neg = int(t.numel()) - n_pos
        if n_pos == 0 or n_neg == 0:
            out.append(float("nan"))
            continue
        order = torch.argsort(s)
        ss = s[order]
        uniq, inv, cnt = torch.unique_consecutive(ss, return_inverse=True, return_counts=True)
        last = torch.cumsum(cnt, 0).double()                          # 1-based rank of the last member of each tie group
        mid = (last - (cnt.double() - 1.0) / 2.0)[inv]
        u = mid[t[order] == 1].sum() - n_pos * (n_pos + 1) / 2.0
        out.append(float(u / (n_pos * n_neg)))
    return torch.tensor(out, dtype=torch.float64)


def bench_kernels(sizes, D, rounds):
    import torch
    import torch.nn.functional as F
    from medmoe_amd import ops
    from medmoe_amd.classify import auroc_from_counts
    out = {}
    for N in sizes:
        for task, C in (("multiclass", 5), ("multilabel", 14)):
            g = torch.Generator(device="cuda").manual_seed(N + C)
            x = torch.randn(N, D, generator=g, device="cuda")
            W = torch.randn(C, D, generator=g, device="cuda") * D ** -0.5
            b = torch.zeros(C, device="cuda")
            if task == "multiclass":
                t = torch.randint(0, C, (N,), generator=g, device="cuda")
                tk, tt = t.to(torch.int32), t
            else:
                t = (torch.rand(N, C, generator=g, device="cuda") < 0.4)
                tk, tt = t.to(torch.int8), t.float()
            dW, db = torch.zeros(C, D, device="cuda"), torch.zeros(C, device="cuda")
            bufs = dict(z=torch.empty(N, C, device="cuda"), loss=torch.empty(1, device="cuda"), counts=torch.empty(2, device="cuda", dtype=torch.int32),
                        scratch=torch.empty(ops.cls_head_scratch(N, D, C), device="cuda"))
            Wt, bt = W.clone().requires_grad_(True), b.clone().requires_grad_(True)

            def kernel():
                return ops.cls_head_step(x, W, b, tk, dW, db, task=task, **bufs)

            def torch_step():
                Wt.grad = bt.grad = None
                z = F.linear(x, Wt, bt)
                loss = F.cross_entropy(z, tt) if task == "multiclass" else F.binary_cross_entropy_with_logits(z, tt)
                loss.backward()
                return loss

            rec = _alternate({"cls_head_step": kernel, "torch": torch_step}, rounds)
            floor = 4.0 * N * D
            for r in rec.values():
                r["share_of_hbm_at_one_read"] = floor / (r["ms_median"] * 1e-3) / HBM_SUSTAINED
            dW.zero_(); db.zero_()
            _, (z, loss, _) = _timed(kernel)
            lt = torch_step()
            rec["loss_kernel"], rec["loss_torch"] = float(loss), float(lt.detach())
            rec["dW_max_abs_diff"] = float((dW - Wt.grad).abs().max())
            # AUROC on the head's own logits
            t8 = tk if task == "multilabel" else (t.reshape(-1, 1) == torch.arange(C, device="cuda").reshape(1, -1)).to(torch.int8)
            scores = z.clone()
            au = _alternate({"auroc_counts": lambda: ops.auroc_counts(scores, t8), "torch_sort": lambda: midrank_auroc_torch(scores, t8)}, max(3, rounds // 2))
            per = auroc_from_counts(ops.auroc_counts(scores, t8))[0].cpu()
            au["max_abs_diff"] = float((per - midrank_auroc_torch(scores, t8)).abs().nan_to_num(0.0).max())
            au["pairs"] = float((ops.auroc_counts(scores, t8)[:, 0].double() * ops.auroc_counts(scores, t8)[:, 1].double()).sum())
            out[f"N{N}_{task}_C{C}"] = {"head": rec, "auroc": au}
            del x, scores, bufs
            torch.cuda.empty_cache()
    return out


def bench_step(rounds, batch=128):
    import torch
    import bench
    from medmoe_amd.classify import ClassifierHead
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("cfg2")
    eng = Engine(cfg, "cuda:0")
    b = bench.synthetic_batch(cfg, batch, 0, eng.device)
    head = ClassifierHead(cfg.d_out, 5, eng.device, init="normal")
    cb = {"image": b["image"], "label": b["label"] % 5}
    rec = _alternate({"classify_step(train_tower=True)": lambda: eng.classify_step(cb, head, train_tower=True),
                      "classify_step(train_tower=False)": lambda: eng.classify_step(cb, head, train_tower=False),
                      "train_step": lambda: eng.train_step(b)}, rounds)
    rec["batch"] = batch
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,65536,262144")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true", help="also time classify_step against train_step on cfg2 at batch 128")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_classify: no GPU")
    out = {"dim": args.dim, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "hbm_sustained_bytes_per_s": HBM_SUSTAINED}
    if not args.no_kernels:
        out["kernels"] = bench_kernels([int(n) for n in args.sizes.split(",")], args.dim, args.rounds)
    if args.step:
        out["step"] = bench_step(args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
