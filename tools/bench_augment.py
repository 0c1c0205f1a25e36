"""Time the on-device augmentation next to the resize it follows, ALTERNATED over the same bytes at each batch size of
`--batches` (default 1024 and 128): B seeded uint8 images with the sides of the synthetic UniMed stand-in (160 .. 320) are resized once to
S x S (default 256); every round then times, each between its own pair of HIP events and after a warm-up of every mode,

    pair_jitter     medmoe_augment_params + medmoe_augment_apply with the GLoRIA block of configs/data/unimed_aug.yaml (crop C = 224, flip,
                    affine, brightness and contrast: the two-pass form of the apply kernel for every image)
    pair_no_jitter  the same block with color_jitter off (one pass)
    resize          the existing preprocess_images_bicubic launch pair at size C on the source images - existing code, the yardstick

and reports per batch and mode the median / min / max over all rounds (the span between the events holds the call's host work too: for
resize the coefficient tables and three small copies), the bytes the pair has to move at the least, B (3 S^2 + 6 C^2), the rate that makes
of the median and its fraction of the 8.0 TB/s HBM peak of the MI355X (the floor is a bound on the PAIR alone; the gather reads the S x S
image out of order and, with contrast on, twice - the second time from L2).  One more pass per pair mode puts every launch between its
own events (ops.PROFILE): `kernels` holds the median span of the parameter and of the apply launch, and the apply launch's share of the peak.

    python tools/bench_augment.py [--batches 1024,128] [--size 256] [--crop 224] [--rounds 5] [--iters 10]

One JSON line.  Needs the GPU: there is no other path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,128")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: no GPU")
    from medmoe_amd import ops
    from medmoe_amd.data import AugmentConfig, augment_apply, augment_params, preprocess_images_bicubic, resize_images_bicubic
    S, C = args.size, args.crop
    block = {"norm": "imagenet", "imsize": S, "random_crop": {"crop_size": C}, "random_horizontal_flip": 0.5,
             "random_affine": {"degrees": 20, "translate": [0.1, 0.1], "scale": [0.95, 1.05]},
             "color_jitter": {"brightness": [0.8, 1.2], "contrast": [0.8, 1.2]}}
    cfgs = {"pair_jitter": AugmentConfig.from_hydra(block), "pair_no_jitter": AugmentConfig.from_hydra(dict(block, color_jitter=False))}
    out = {"size": S, "crop": C, "rounds": args.rounds, "iters": args.iters, "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        g = torch.Generator(device="cuda").manual_seed(B)
        sides = torch.randint(160, 321, (B, 2), generator=torch.Generator().manual_seed(B))
        imgs = [torch.randint(0, 256, (int(h), int(w), 3), generator=g, dtype=torch.uint8, device="cuda") for h, w in sides]
        u8 = resize_images_bicubic(imgs, S)
        dst = torch.empty(B, 3, C, C, device="cuda", dtype=torch.bfloat16)
        step = [0]

        def pair(cfg):
            step[0] += 1
            augment_apply(u8, augment_params(cfg, B, 0, step[0], True, "cuda"), cfg, out=dst)
        modes = {"pair_jitter": lambda: pair(cfgs["pair_jitter"]), "pair_no_jitter": lambda: pair(cfgs["pair_no_jitter"]),
                 "resize": lambda: preprocess_images_bicubic(imgs, size=C, out=dst)}
        for fn in modes.values():
            fn(); fn()
        torch.cuda.synchronize()
        times = {m: [] for m in modes}
        for _ in range(args.rounds):
            for m, fn in modes.items():
                spans = []
                for _ in range(args.iters):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); fn(); b.record()
                    spans.append((a, b))
                torch.cuda.synchronize()
                times[m] += [a.elapsed_time(b) for a, b in spans]
        floor_bytes = B * (3.0 * S * S + 6.0 * C * C)
        res = {"floor_bytes": floor_bytes, "floor_ms_at_hbm_peak": round(floor_bytes / HBM_PEAK * 1e3, 4)}
        kernels = {}
        for m in ("pair_jitter", "pair_no_jitter"):
            ops.PROFILE = []
            for _ in range(args.iters):
                modes[m]()
            torch.cuda.synchronize()
            spans = {}
            for label, _, _, e0, e1, _ in ops.PROFILE:
                spans.setdefault(label, []).append(e0.elapsed_time(e1))
            ops.PROFILE = None
            kernels[m] = {label: round(statistics.median(v), 4) for label, v in spans.items()}
            kernels[m]["apply_fraction_of_hbm_peak"] = round(floor_bytes / (kernels[m]["augment_apply_kernel"] * 1e-3) / HBM_PEAK, 4)
        for m, ts in times.items():
            ts = sorted(ts)
            res[m] = {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}
            if m != "resize":
                rate = floor_bytes / (statistics.median(ts) * 1e-3)
                res[m]["floor_GB_per_s"] = round(rate / 1e9, 1)
                res[m]["fraction_of_hbm_peak"] = round(rate / HBM_PEAK, 4)
                res[m]["kernels"] = kernels[m]
        res["pair_jitter_over_resize"] = round(res["pair_jitter"]["median_ms"] / res["resize"]["median_ms"], 4)
        out["batches"][str(B)] = res
        del imgs, u8, dst
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
