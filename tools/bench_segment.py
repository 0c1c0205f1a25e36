"""Time the segmentation launches next to what a user would write without them, ALTERNATED in one process:

  1. head      the four head launches of a training step (ops.seg_head_fwd, seg_loss with its gradient pass, seg_head_bwd with dfeat) against
               the torch composition F.linear -> F.interpolate(bilinear) -> BCE-with-logits + batch Dice under autograd (gradients of W, b
               and the features), at B = 128, g = 14, 224 x 224, D = 768, C = 1 and C = 4.  Reported: median / min / max milliseconds per
               mode and the peak device memory each mode adds over the inputs.
  2. step      Engine.segment_step (probe and fine-tune) next to Engine.classify_step and Engine.train_step on cfg2 at batch 128
               (`--step`; seeded synthetic batch).

Every call sits between its own pair of HIP events after a warm-up of every mode.  One JSON line.  Needs the GPU: there is no other path.

    python tools/bench_segment.py [--batch 128] [--rounds 7] [--step] [--no-kernels]"""
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


def bench_kernels(B, g, size, D, rounds):
    import torch
    import torch.nn.functional as F
    from medmoe_amd import ops
    out = {}
    for C in (1, 4):
        gen = torch.Generator(device="cuda").manual_seed(C)
        feat = torch.randn(B * g * g, D, generator=gen, device="cuda").to(torch.bfloat16)
        W = torch.randn(C, D, generator=gen, device="cuda") * D ** -0.5
        b = torch.zeros(C, device="cuda")
        masks = (F.interpolate(torch.randn(B, C, 7, 7, generator=gen, device="cuda"), size=(size, size), mode="bilinear") > 0.3).to(torch.int8)
        masks[torch.rand(B, C, size, size, generator=gen, device="cuda") < 0.02] = -1
        dW, db = torch.zeros(C, D, device="cuda"), torch.zeros(C, device="cuda")
        z, dz = torch.empty(B, g * g, C, device="cuda"), torch.empty(B, g * g, C, device="cuda")
        dfeat = torch.empty_like(feat)
        bufs = dict(loss=torch.empty(1, device="cuda"), counts=torch.empty(C, 4, device="cuda", dtype=torch.int64),
                    scratch=torch.empty(ops.seg_scratch(B, g, size, size, D, C), device="cuda"))
        featf = feat.float().requires_grad_(True)
        Wt, bt = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        valid, t = (masks >= 0).float(), (masks > 0).float()

        def kernel():
            ops.seg_head_fwd(feat, W, b, z)
            ops.seg_loss(z, masks, dz=dz, **bufs)
            ops.seg_head_bwd(dz, feat, W, dW, db, dfeat=dfeat, scratch=bufs["scratch"])
            return bufs["loss"]

        def torch_step():
            Wt.grad = bt.grad = featf.grad = None
            zz = F.linear(featf, Wt, bt).reshape(B, g, g, C).permute(0, 3, 1, 2)
            zf = F.interpolate(zz, size=(size, size), mode="bilinear", align_corners=False)
            bce = (F.binary_cross_entropy_with_logits(zf, t, reduction="none") * valid).sum() / valid.sum()
            p = torch.sigmoid(zf) * valid
            dice = 1.0 - ((2.0 * (p * t).sum(dim=(0, 2, 3)) + 1.0) / (p.sum(dim=(0, 2, 3)) + (t * valid).sum(dim=(0, 2, 3)) + 1.0)).mean()
            loss = bce + dice
            loss.backward()
            return loss

        rec = _alternate({"seg_head (4 launches)": kernel, "torch": torch_step}, rounds)
        rec["seg_head (4 launches)"]["peak_mib"] = _peak(kernel)
        rec["torch"]["peak_mib"] = _peak(torch_step)
        dW.zero_(); db.zero_()
        lk = float(kernel())
        lt = float(torch_step().detach())
        rec["loss_kernel"], rec["loss_torch"] = lk, lt
        rec["dW_max_abs_diff"] = float((dW - Wt.grad).abs().max())
        rec["predict_ms"] = _alternate({"seg_predict": lambda: ops.seg_predict(z, (size, size))}, rounds)["seg_predict"]
        out[f"B{B}_g{g}_{size}x{size}_D{D}_C{C}"] = rec
        del feat, featf, masks, valid, t, bufs
        torch.cuda.empty_cache()
    return out


def bench_step(rounds, batch=128):
    import torch
    import bench
    from medmoe_amd.classify import ClassifierHead
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    from medmoe_amd.segment import SegmenterHead
    from src.data.components.unimed import synthetic_mask
    cfg = config_by_name("cfg2")
    eng = Engine(cfg, "cuda:0")
    b = bench.synthetic_batch(cfg, batch, 0, eng.device)
    seg = SegmenterHead(cfg.d_out, 1, eng.device, init="normal")
    cls = ClassifierHead(cfg.d_out, 5, eng.device, init="normal")
    masks = torch.stack([synthetic_mask(1, cfg.img_size, 0.02, 100 + i) for i in range(batch)]).to(eng.device)
    sb, cb = {"image": b["image"], "mask": masks}, {"image": b["image"], "label": b["label"] % 5}
    rec = _alternate({"segment_step(train_tower=True)": lambda: eng.segment_step(sb, seg, train_tower=True),
                      "segment_step(train_tower=False)": lambda: eng.segment_step(sb, seg, train_tower=False),
                      "classify_step(train_tower=True)": lambda: eng.classify_step(cb, cls, train_tower=True),
                      "classify_step(train_tower=False)": lambda: eng.classify_step(cb, cls, train_tower=False),
                      "train_step": lambda: eng.train_step(b)}, rounds)
    rec["batch"] = batch
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--grid", type=int, default=14)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", action="store_true", help="also time segment_step next to classify_step and train_step on cfg2 at batch 128")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment: no GPU")
    out = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    if not args.no_kernels:
        out["kernels"] = bench_kernels(args.batch, args.grid, args.size, args.dim, args.rounds)
    if args.step:
        out["step"] = bench_step(args.rounds, args.batch)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
