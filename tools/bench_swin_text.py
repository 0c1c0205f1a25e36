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


def measure(train_text: bool, B: int, steps: int, warmup: int, dropout: float = 0.0):
    import bench
    from medmoe_amd.hydra_lite import compose, instantiate
    ov = ["experiment=pretraining_medmoe_swin"] + (["model.model.text.freeze_bert=false"] if train_text else [])
    if dropout > 0.0:
        ov += [f"model.model.text.hidden_dropout_prob={dropout}", f"model.model.text.attention_probs_dropout_prob={dropout}"]
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
    ap.add_argument("--text-dropout", type=float, default=0.0, metavar="P",
                    help="also time the trained tower with hidden and attention dropout P (BERT's default: 0.1), interleaved with dropout 0")
    ap.add_argument("--rounds", type=int, default=1, help="repeat the trained measurements this many times (run-to-run spread)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_swin_text.py needs an MI355X")
    frozen = measure(False, args.batch, args.steps, args.warmup)
    rounds = [measure(True, args.batch, args.steps, args.warmup)]
    dropped = []
    for r in range(args.rounds):
        if r:
            rounds.append(measure(True, args.batch, args.steps, args.warmup))
        if args.text_dropout > 0.0:
            dropped.append(measure(True, args.batch, args.steps, args.warmup, args.text_dropout))
    trained = rounds[0]
    out = {"metric": f"SwinEngine.train_step ms at batch {args.batch}, text tower frozen vs trained", "batch": args.batch,
           "steps": args.steps, "warmup": args.warmup, "frozen": frozen, "trained": trained,
           "added_ms": trained["ms_per_step"] - frozen["ms_per_step"]}
    if args.rounds > 1:
        out["trained_ms_rounds"] = [r["ms_per_step"] for r in rounds]
    if dropped:
        out["text_dropout"] = args.text_dropout
        out["trained_dropout"] = dropped[0]
        out["trained_dropout_ms_rounds"] = [r["ms_per_step"] for r in dropped]
        out["dropout_added_ms"] = dropped[0]["ms_per_step"] - trained["ms_per_step"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
