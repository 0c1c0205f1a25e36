"""Time the two grounding launches next to the same maths in torch, ALTERNATED in one process:

  1. kernels   ops.ground_maps + ops.ground_score on n entries (default 1024 matched pairs: 196 regions, 77 words, width 768, 224 x 224, two
               boxes, one threshold) against bmm -> softmax over the words -> softmax over the regions -> span mean -> F.interpolate(bilinear)
               -> argmax / min / max -> masked sums and threshold counts, in both modes.  Reported: median / min / max milliseconds per mode and
               the peak device memory each adds over the inputs; and that the two agree (hits, largest map difference).
  2. bench     `bench.py --gpus 1` of this tree (the feature unused) alternated with the same command in another checkout (`--parent DIR`, a
               built tree of the parent commit), each run a fresh process; the JSON lines are reported as they come.

Every call sits between its own pair of HIP events after a warm-up of every mode.  One JSON line.  Needs the GPU: there is no other path.

    python tools/bench_ground.py [--n 1024] [--rounds 7] [--parent DIR --steps 10 --warmup 3 --repeats 2]"""
import argparse
import json
import os
import statistics
import subprocess
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
    for fn in modes.values():                                        # warm-up of every mode
        _timed(fn)
    times = {name: [] for name in modes}
    for _ in range(rounds):
        for name, fn in modes.items():
            times[name].append(_timed(fn)[0])
    return {name: {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)} for name, t in times.items()}


def _peak(fn):
    """Peak device memory one call of `fn` adds over what is allocated before it, in MiB."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def bench_kernels(n, g, T, D, size, rounds):
    import torch
    import torch.nn.functional as F
    from medmoe_amd import ops
    dev, P = "cuda", g * g
    gen = torch.Generator(device=dev).manual_seed(0)
    ctx = torch.randn(n, P, D, generator=gen, device=dev).to(torch.bfloat16)
    words = (torch.randn(n, T, D, generator=gen, device=dev) * (3.0 / D ** 0.5)).to(torch.bfloat16)
    lens = torch.randint(8, T + 1, (n,), generator=gen, device=dev).to(torch.int32)
    lo = (torch.rand(n, generator=gen, device=dev) * (lens - 1)).long()
    hi = torch.minimum(lo + 1 + torch.randint(0, 3, (n,), generator=gen, device=dev), lens.long())
    pair = torch.arange(n, device=dev)
    entries = torch.stack([pair, pair, lo, hi], dim=1).cpu()
    lens_h = lens.cpu()
    x0 = torch.randint(0, size // 2, (n, 2, 2), generator=gen, device=dev)
    boxes = torch.cat([x0, x0 + torch.randint(8, size // 2, (n, 2, 2), generator=gen, device=dev)], dim=2).to(torch.int32).cpu()
    theta, temp1 = 0.5, 4.0
    ys, xs = torch.arange(size, device=dev).reshape(1, size, 1), torch.arange(size, device=dev).reshape(1, 1, size)
    bd = boxes.to(dev).long()
    union = torch.zeros(n, size, size, dtype=torch.bool, device=dev)
    for k in range(2):
        union |= (xs >= bd[:, k, 0].reshape(n, 1, 1)) & (xs < bd[:, k, 2].reshape(n, 1, 1)) & (ys >= bd[:, k, 1].reshape(n, 1, 1)) & (ys < bd[:, k, 3].reshape(n, 1, 1))
    tmask = torch.arange(T, device=dev).reshape(1, T) < lens.reshape(n, 1)
    smask = ((torch.arange(T, device=dev).reshape(1, T) >= lo.reshape(n, 1)) & (torch.arange(T, device=dev).reshape(1, T) < hi.reshape(n, 1))).float()
    out = {}
    for mode in ("attention", "cosine"):
        def kernel():
            h = ops.ground_maps(ctx, words, lens, entries, mode=mode, temp1=temp1, cap_lens_host=lens_h)
            return h, ops.ground_score(h, boxes, (size, size), thetas=(theta,))

        def torch_same():
            if mode == "attention":
                s = torch.bmm(words.float(), ctx.float().transpose(1, 2))                               # [n, T, P]: exact products, fp32 sums
                s = torch.softmax(s.masked_fill(~tmask.reshape(n, T, 1), float("-inf")), dim=1)
                a = torch.softmax(temp1 * s, dim=2)
                h = (a * smask.reshape(n, T, 1)).sum(dim=1) / smask.sum(dim=1, keepdim=True)
            else:
                u = (words.float() * smask.reshape(n, T, 1)).sum(dim=1)
                cf = ctx.float()
                h = torch.bmm(cf, u.reshape(n, D, 1))[:, :, 0] / (cf.norm(dim=2) * u.norm(dim=1, keepdim=True)).clamp(min=1e-8)
            hf = F.interpolate(h.reshape(n, 1, g, g), size=(size, size), mode="bilinear", align_corners=False)[:, 0]
            flat = hf.reshape(n, -1)
            mx, am = flat.max(dim=1)
            mn = flat.min(dim=1).values
            thr = mn + theta * (mx - mn)
            on = hf >= thr.reshape(n, 1, 1)
            hit = union.reshape(n, -1).gather(1, am.reshape(n, 1))[:, 0]
            d = hf.double()
            sums = torch.stack([(d * union).sum(dim=(1, 2)), (d * d * union).sum(dim=(1, 2)), d.sum(dim=(1, 2)), (d * d).sum(dim=(1, 2))], dim=1)
            counts = torch.stack([union.sum(dim=(1, 2)), (on & union).sum(dim=(1, 2)), on.sum(dim=(1, 2))], dim=1)
            return h, hit, counts, sums

        name = "ground (2 launches)"
        rec = _alternate({name: kernel, "torch": torch_same}, rounds)
        rec[name]["peak_mib"] = _peak(kernel)
        rec["torch"]["peak_mib"] = _peak(torch_same)
        (hk, rk), (ht, hit, counts, _) = kernel(), torch_same()
        rec["h_max_abs_diff"] = float((hk - ht).abs().max())
        rec["hits_kernel"], rec["hits_torch"] = int(rk["rec_i"][:, 2].sum()), int(hit.sum())
        rec["area_equal"] = bool(torch.equal(rk["rec_i"][:, 3].long(), counts[:, 0]))
        out[f"{mode}_n{n}_g{g}_T{T}_D{D}_{size}x{size}"] = rec
    return out


def bench_trees(parent, steps, warmup, repeats):
    """bench.py of this tree and of `parent`, alternated, each run a fresh process; the last JSON line of every run."""
    runs = []
    for _ in range(repeats):
        for name, tree in (("this", ROOT), ("parent", parent)):
            r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               cwd=tree, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(f"bench_ground: bench.py of {tree} failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            runs.append({"tree": name, "result": json.loads(line)})
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=14)
    ap.add_argument("--words", type=int, default=77)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py of both trees, alternated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ground: no GPU")
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    if not args.no_kernels:
        out["kernels"] = bench_kernels(args.n, args.grid, args.words, args.dim, args.size, args.rounds)
    if args.parent:
        torch.cuda.empty_cache()
        out["bench"] = bench_trees(os.path.abspath(args.parent), args.steps, args.warmup, args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
