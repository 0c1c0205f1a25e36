#!/usr/bin/env python3
"""LAMB (MedMoEConfig.optimizer = "lamb") behind the bf16 gradient exchange (grad_comm_dtype = "bf16") on ONE GPU over
the REAL backend: a one-rank process group on "nccl" (= RCCL) with MEDMOE_DIST_WORLD1=1, as tools/rccl_world1_bf16.py sets it up, both towers
trainable, parameter groups on.  Checked in front of and behind every arena's lamb_step, three optimiser steps:
  * the flag g16_reduced is set by the exchange and g16 == bf16(g32) bit for bit (one rank: scale 1, a sum over one rank);
  * the step takes the `_g16` moments launch - no fp32-gradient moments launch and no Adam launch is issued;
  * p, m, v, the bf16 copy and the trust ratios equal, bit for bit, those of the fp32-gradient launches (medmoe_lamb_moments / _ratios /
    _apply) run on clones of the arena's state with g16.float() as the gradient;
  * the flag is cleared behind the step.
Must run in a fresh process: the group is created before any GPU work."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29561"), RANK="0", WORLD_SIZE="1",
                  MEDMOE_DIST_WORLD1="1", PROJECT_ROOT=ROOT)
os.environ.pop("MEDMOE_GRAD_COMM", None)
import torch
import torch.distributed as dist

dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
torch.cuda.set_device(0)
import bench
from medmoe_amd import ops
from medmoe_amd.config import config_by_name
from medmoe_amd.engine import Engine

BF = torch.bfloat16
bits = lambda t: t.view(torch.int16 if t.dtype == BF else torch.int32)
launches = []
_call = ops.call
def call_spy(name, *a):
    launches.append(name)
    return _call(name, *a)
ops.call = call_spy


def spy_on(arena, seen):
    orig = arena.lamb_step

    def spy(normsq, lr, wd, clip, grad_scale=1.0, **k):
        torch.cuda.synchronize()
        rec = {"flag": arena.g16_reduced, "g16_is_bf16_g32": torch.equal(bits(arena.g16), bits(arena.g32.to(BF)))}
        m, v = arena.adam_state()
        n_seg = len(arena.segments())
        ends, lrm, wdm, base = arena._seg_table
        p, m, v, p16, up = arena.p32.clone(), m.clone(), v.clone(), arena.p16.clone(), arena.g16.float()
        first = len(launches)
        orig(normsq, lr, wd, clip, grad_scale, **k)
        mine = [n for n in launches[first:] if n.startswith(("lamb_", "adam_"))]
        rec["g16_launches"] = mine == ["lamb_moments_g16", "lamb_ratios", "lamb_apply"]
        scratch, ratios = torch.zeros_like(arena._lamb_scratch), torch.zeros_like(arena._lamb_ratios)
        b1, b2 = k["betas"]
        t = arena.step_count
        _call("lamb_moments", p, up, m, v, arena.n_train, ends, wdm, base, n_seg, scratch, scratch.numel(), b1, b2, k["eps"], wd, t, normsq, clip,
              grad_scale)
        _call("lamb_ratios", scratch, scratch.numel(), ends, wdm, base, n_seg, arena.n_train, wd, int(k["always_adapt"]), int(k["trust_clip"]), ratios)
        _call("lamb_apply", p, m, v, p16, arena.n_train, ends, lrm, wdm, n_seg, ratios, lr, b1, b2, k["eps"], wd, t)
        torch.cuda.synchronize()
        rec["same_step"] = all(torch.equal(bits(x), bits(y)) for x, y in ((p, arena.p32), (m, arena.m), (v, arena.v), (p16, arena.p16),
                                                                          (ratios, arena._lamb_ratios)))
        rec["ratios_differ_from_one"] = bool((ratios[:n_seg] != 1.0).any())
        rec["cleared"] = not arena.g16_reduced
        seen.append(rec)
    arena.lamb_step = spy


cfg = config_by_name("tiny2")
cfg.grad_comm_dtype, cfg.freeze_text = "bf16", False
cfg.optimizer, cfg.lr, cfg.weight_decay, cfg.clip, cfg.adam_eps = "lamb", 1e-3, 0.01, 1.0, 1e-6
cfg.no_decay_1d, cfg.layer_decay = True, 0.75
eng = Engine(cfg, "cuda:0", seed=0)
assert eng.dist and eng.world == 1 and dist.get_backend() == "nccl" and eng.grad_comm(eng.params) is eng.params
assert eng.params.train_from == 0 and eng.tstore.train_from == 0
batch = bench.synthetic_batch(cfg, 16, 99, eng.device)
seen = {"image": [], "text": []}
spy_on(eng.params, seen["image"]); spy_on(eng.tstore, seen["text"])
p0 = eng.params.p32.clone()
losses = [float(eng.train_step(batch)["loss"]) for _ in range(3)]
torch.cuda.synchronize()
for kind, recs in seen.items():
    assert len(recs) == 3 and all(all(r.values()) for r in recs), (kind, recs)
assert not any(n.startswith("adam_") for n in launches) and "lamb_moments" not in launches
assert all(l == l and abs(l) < 1e4 for l in losses) and bool(torch.isfinite(eng.params.p32).all()) and not torch.equal(eng.params.p32, p0)
assert eng.params.step_count == 3 and eng.tstore.step_count == 3
print(f"lamb behind the bf16 exchange: losses {losses}, spies {seen['image'][0]}")
dist.destroy_process_group()
print("rccl world-1 lamb bf16 path OK")
