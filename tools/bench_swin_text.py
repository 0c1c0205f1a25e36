#!/usr/bin/env python3
"""The reference's own model (Swin-T + pyramid experts, 3136 local regions, 12-layer text tower, 25-token captions) on the fused step at the
reference's per-device batch of 32: `SwinEngine.train_step` with the text tower frozen (`bench.py --config ref_swin`) and trained
(`text.freeze_bert: false`), the same warm-up / step counts as bench.py; one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PROJECT_ROOT", ROOT)


def measure(train_text: bool, B: int, steps: int, warmup: int):
    import bench
    from medmoe_amd.hydra_lite import compose, instantiate
    ov = ["experiment=pretraining_medmoe_swin"] + (["model.model.text.freeze_bert=false"] if train_text else [])
    hc = compose(os.path.join(ROOT, "configs"), "train.yaml", ov)
    lit = instantiate(hc.model)
    lit.train(); lit.configure_optimizers(); lit.configure_fused(1, float(hc.trainer.gradient_clip_val))
    cfg = lit.model.cfg
    b = bench.synthetic_batch(cfg, B, 12345, lit.model.device)
    b["label"] = b["label"] % int(hc.model.model.vision.num_experts)
    mb = {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"], "token_type": b["token_type"]}}
    for _ in range(warmup):
        lit.training_step(mb, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = lit.training_step(mb, 0)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out = {"ms_per_step": dt * 1e3, "pairs_per_s": B / dt, "loss": float(loss.detach()), "hbm_peak_gb": torch.cuda.max_memory_allocated() / 1e9}
    del lit
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_swin_text.py needs an MI355X")
    frozen = measure(False, args.batch, args.steps, args.warmup)
    trained = measure(True, args.batch, args.steps, args.warmup)
    print(json.dumps({"metric": f"SwinEngine.train_step ms at batch {args.batch}, text tower frozen vs trained", "batch": args.batch,
                      "steps": args.steps, "warmup": args.warmup, "frozen": frozen, "trained": trained,
                      "added_ms": trained["ms_per_step"] - frozen["ms_per_step"]}), flush=True)


if __name__ == "__main__":
    main()
