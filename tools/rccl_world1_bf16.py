#!/usr/bin/env python3
"""The bf16 gradient exchange (MedMoEConfig.grad_comm_dtype = "bf16") on ONE GPU over the REAL backend: a one-rank process group
on "nccl" (= RCCL) with MEDMOE_DIST_WORLD1=1, so the packs on the compute stream, the asynchronous bf16 all-reduces behind them and Adam on
the bf16 sum execute for real.  Checked:
  * bf16: in front of every arena's adam_step the flag is set and g16 == bf16(g32) bit for bit (one rank: scale 1, a sum over one rank),
    and the stepped parameters equal those of a cloned arena stepped by the fp32-gradient kernel on g16.float();
  * fp32 (the default): no pack, no g16, and the step agrees with a non-distributed engine as tools/rccl_world1.py asserts;
  * one SwinEngine step through the Hydra module (model.grad_comm_dtype=bf16): the flags are set on the tower and the MoE arena, the
    parameters stay finite.
`python tools/rccl_world1_bf16.py swin` runs the third part alone, without an argument the first two.  Must run in a fresh process: the
group is created before any GPU work."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29547"), RANK="0", WORLD_SIZE="1",
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
from medmoe_amd.flat import FlatArena

BF = torch.bfloat16
SWIN = sys.argv[1:2] == ["swin"]
name, B = "tiny2", 16
bits = lambda t: t.view(torch.int16 if t.dtype == BF else torch.int32)
packs = []
_pack = FlatArena.pack
def pack_spy(self, lo, hi, scale):
    packs.append((self, lo, hi, scale))
    return _pack(self, lo, hi, scale)
FlatArena.pack = pack_spy


def spy_on(arena, seen):
    """In front of arena.adam_step: the flag, g16 against g32; behind it: the same step by the fp32-gradient kernel on a clone."""
    orig = arena.adam_step

    def spy(normsq, lr, wd, clip, *a, **k):
        torch.cuda.synchronize()
        rec = {"flag": arena.g16_reduced, "g16_is_bf16_g32": torch.equal(bits(arena.g16), bits(arena.g32.to(BF)))}
        m, v = arena.adam_state()
        p, m, v, p16, up = arena.p32.clone(), m.clone(), v.clone(), arena.p16.clone(), arena.g16.float()
        orig(normsq, lr, wd, clip, *a, **k)
        ops.call("adam_step", p, up, m, v, p16, arena.numel, lr, 0.9, 0.999, 1e-8, wd, arena.step_count, normsq, clip, 1.0)
        torch.cuda.synchronize()
        rec["same_step"] = all(torch.equal(bits(x), bits(y)) for x, y in ((p, arena.p32), (m, arena.m), (v, arena.v), (p16, arena.p16)))
        rec["cleared"] = not arena.g16_reduced
        seen.append(rec)
    arena.adam_step = spy


def engine_part():
    # ---- bf16, both towers trainable: the bucketed reduce of the image arena and the text arena's reduce -------------------------------------
    cfg = config_by_name(name)
    cfg.grad_comm_dtype, cfg.freeze_text = "bf16", False
    eng = Engine(cfg, "cuda:0", seed=0)
    assert eng.dist and eng.world == 1 and dist.get_backend() == "nccl" and eng.grad_comm(eng.params) is eng.params
    batch = bench.synthetic_batch(cfg, B, 99, eng.device)
    seen = {"image": [], "text": []}
    spy_on(eng.params, seen["image"]); spy_on(eng.tstore, seen["text"])
    p0 = eng.params.p32.clone()
    eng.train_step(batch, optimizer=False)                              # an accumulating micro-batch: no pack, no collective
    assert not packs and not eng.params.g16_reduced and not eng.tstore.g16_reduced
    losses = [float(eng.train_step(batch, zero_grad=False)["loss"])] + [float(eng.train_step(batch)["loss"]) for _ in range(2)]
    torch.cuda.synchronize()
    n_b = cfg.n_layer_v + 2
    assert len(packs) == 3 * (n_b + 1) and all(s == 1.0 for *_, s in packs), len(packs)
    assert [(lo, hi) for a, lo, hi, _ in packs[:n_b]] == [(eng.bucket_bounds[i], eng.bucket_bounds[i + 1]) for i in [n_b - 1] + list(range(n_b - 2, 0, -1)) + [0]]
    assert packs[n_b][0] is eng.tstore and packs[n_b][1:3] == (0, eng.tstore.numel)
    for kind, recs in seen.items():
        assert len(recs) == 3 and all(all(r.values()) for r in recs), (kind, recs)
    assert all(l == l and abs(l) < 1e4 for l in losses) and bool(torch.isfinite(eng.params.p32).all()) and not torch.equal(eng.params.p32, p0)
    print(f"bf16 exchange: {len(packs)} packs, losses {losses}, spies {seen['image'][0]}")

    # ---- fp32 (the default) against a non-distributed engine, as tools/rccl_world1.py ----------------------------------------------------------
    del packs[:]
    cfg = config_by_name(name)
    assert cfg.grad_comm_dtype == "fp32"
    eng = Engine(cfg, "cuda:0", seed=0)
    assert eng.dist and eng.grad_comm(eng.params) is None
    batch = bench.synthetic_batch(cfg, B, 99, eng.device)
    p0 = eng.params.p32.clone()
    out_d = {k: float(v) for k, v in eng.train_step(batch, optimizer=False).items()}
    torch.cuda.synchronize()
    g_d = eng.params.g32.clone()
    steps_d = [float(eng.train_step(batch)["loss"]) for _ in range(3)]
    torch.cuda.synchronize()
    p_d = eng.params.p32.clone()
    assert not packs and eng.params._g16 is None                        # the default never packs and never allocates the bf16 buffer
    os.environ["MEDMOE_DIST_WORLD1"] = "0"
    ref = Engine(cfg, "cuda:0", seed=0)
    assert not ref.dist and torch.equal(ref.params.p32, p0)
    out_s = {k: float(v) for k, v in ref.train_step(batch, optimizer=False).items()}
    torch.cuda.synchronize()
    g_s = ref.params.g32.clone()
    steps_s = [float(ref.train_step(batch)["loss"]) for _ in range(3)]
    torch.cuda.synchronize()
    p_s = ref.params.p32.clone()
    os.environ["MEDMOE_DIST_WORLD1"] = "1"
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    for k in out_s:
        assert abs(out_d[k] - out_s[k]) <= 1e-5 * max(1.0, abs(out_s[k])), (k, out_d[k], out_s[k])
    assert rel(g_d, g_s) < 2e-3, rel(g_d, g_s)
    assert abs(steps_d[0] - steps_s[0]) <= 1e-5 * max(1.0, abs(steps_s[0])), (steps_d, steps_s)
    for a, b in zip(steps_d[1:], steps_s[1:]):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (steps_d, steps_s)
    ud, us = p_d - p0, p_s - p0
    cos = float((ud * us).sum() / (ud.norm() * us.norm()))
    assert cos > 0.97 and rel(p_d, p_s) < 2e-3, (cos, rel(p_d, p_s))
    print(f"fp32 exchange: losses {out_d['loss']:.6f} / {out_s['loss']:.6f}; grad rel {rel(g_d, g_s):.2e}; update cos {cos:.4f}")


def swin_part():
    # ---- one SwinEngine step in the same group, through the Hydra key ---------------------------------------------------------------------------
    from medmoe_amd.hydra_lite import compose, instantiate
    hcfg = compose(os.path.join(ROOT, "configs"), "train.yaml",
                   ["experiment=pretraining_medmoe", "model.model.vision.arch=swin_t", "model.fused_step=true", "model.model.vision.num_experts=3",
                    "model.model.text.n_layer=2", "model.optimizer.lr=0.0005", "model.grad_comm_dtype=bf16"])
    lit = instantiate(hcfg.model)
    lit.train(); lit.configure_optimizers(); lit.configure_fused(1, 0.25)
    lit.model.swin.drop_path_rate = 0.0
    assert lit.model.engine.dist and lit.model.engine.cfg.grad_comm_dtype == "bf16"
    b = bench.synthetic_batch(lit.model.cfg, 4, 4242, lit.model.device)
    b["label"] = b["label"] % 3
    flags = []
    _adam = FlatArena.adam_step
    def adam_spy(self, *a, **k):
        flags.append((self, self.g16_reduced))
        return _adam(self, *a, **k)
    FlatArena.adam_step = adam_spy
    del packs[:]
    out = lit.fused_training_step({"image": b["image"], "label": b["label"],
                                   "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"], "token_type": b["token_type"]}})
    torch.cuda.synchronize()
    FlatArena.adam_step = _adam
    enc = lit._swin_engine.enc
    assert [a for a, _ in flags] == [enc.tower.store, enc.store] and all(f for _, f in flags), flags
    assert [(a, lo, hi) for a, lo, hi, _ in packs] == [(enc.store, 0, enc.store.numel), (enc.tower.store, 0, enc.tower.store.numel)]
    assert not enc.store.g16_reduced and not enc.tower.store.g16_reduced
    assert bool(torch.isfinite(enc.store.p32).all()) and bool(torch.isfinite(enc.tower.store.p32).all()) and float(out["loss"]) == float(out["loss"])
    print(f"swin step with the bf16 exchange: loss {float(out['loss']):.4f}")


(swin_part if SWIN else engine_part)()
dist.destroy_process_group()
print("rccl world-1 bf16 path OK")
