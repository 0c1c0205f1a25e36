#!/usr/bin/env python3
"""The bf16 gradient exchange (MedMoEConfig.grad_comm_dtype = "bf16") under two ranks sharing ONE GPU (gloo backend, as
tools/two_rank_gpu.py; config tiny, 8 pairs per rank).  Each rank captures its local fp32 gradient bucket by bucket just before the packs,
the ranks exchange the captures, and every rank checks:
  * what Adam reads, g16, equals bf16(g32_rank0 * 0.5) + bf16(g32_rank1 * 0.5) evaluated in bf16 - with two ranks the sum is ONE rounding
    of an exact value, so this holds bit for bit whatever the reduction order;
  * both ranks' clip norms (normsq) are bit-identical, and both replicas end two consecutive steps with identical fp32 masters.
TWO_RANK_BF16_CASE=text: freeze_text = False, the text arena's reduce is checked the same way.
TWO_RANK_BF16_CASE=accum: two micro-batches (optimizer=False, then zero_grad=False): no pack and no collective on the first, and the reduced
gradient is the bf16 average of the sums accumulated in g32."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

CASE = os.environ.get("TWO_RANK_BF16_CASE", "")
BF = torch.bfloat16
bits = lambda t: t.view(torch.int16 if t.dtype == BF else torch.int32)


def gathered(t, world):
    parts = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(parts, t.contiguous())
    return parts


def worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("MEDMOE_GRAD_COMM", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    from medmoe_amd import dist as D
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny")
    cfg.grad_comm_dtype = "bf16"
    cfg.freeze_text = CASE != "text"
    eng = Engine(cfg, "cuda:0", seed=0)
    assert eng.dist and eng.world == world
    arenas = {"image": eng.params}
    if CASE == "text":
        arenas["text"] = eng.tstore
    local = {k: torch.zeros_like(a.g32) for k, a in arenas.items()}      # the rank-local fp32 gradient as the packs saw it
    seen = {k: {} for k in arenas}
    counts = {"pack": 0, "collective": 0}

    def spy_on(kind, arena):
        pack, adam = arena.pack, arena.adam_step

        def pack_spy(lo, hi, scale):
            torch.cuda.synchronize()
            assert scale == 1.0 / world
            counts["pack"] += 1
            local[kind][lo:hi] = arena.g32[lo:hi]
            return pack(lo, hi, scale)

        def adam_spy(normsq, *a, **k):
            torch.cuda.synchronize()
            seen[kind].update(flag=arena.g16_reduced, g16=arena.g16.clone(), normsq=normsq.clone(), g32=arena.g32.clone())
            return adam(normsq, *a, **k)
        arena.pack, arena.adam_step = pack_spy, adam_spy
    for kind, arena in arenas.items():
        spy_on(kind, arena)
    reduce_bf16 = D._all_reduce_bf16

    def reduce_spy(t, async_op=False):
        counts["collective"] += 1
        return reduce_bf16(t, async_op=async_op)
    D._all_reduce_bf16 = reduce_spy

    ok = {}
    n_b = cfg.n_layer_v + 2
    for step in range(2):
        full = bench.synthetic_batch(cfg, 32, 777 + step, eng.device)
        counts.update(pack=0, collective=0)
        for v in local.values():
            v.zero_()
        if CASE == "accum":
            first = {k: v[rank * 8: rank * 8 + 8].contiguous() for k, v in full.items()}
            second = {k: v[16 + rank * 8: 16 + rank * 8 + 8].contiguous() for k, v in full.items()}
            eng.train_step(first, optimizer=False, loss_scale=0.5)
            torch.cuda.synchronize()
            ok[f"no_pack_on_first_{step}"] = counts == {"pack": 0, "collective": 0} and not eng.params.g16_reduced
            g_first = eng.params.g32.clone()
            eng.train_step(second, zero_grad=False, loss_scale=0.5)
        else:
            eng.train_step({k: v[rank * 8: rank * 8 + 8].contiguous() for k, v in full.items()})
        torch.cuda.synchronize()
        ok[f"counts_{step}"] = counts == {"pack": n_b + len(arenas) - 1, "collective": n_b + len(arenas) - 1}
        for kind, arena in arenas.items():
            s = seen[kind]
            g = gathered(local[kind], world)
            want = (g[0] * 0.5).to(BF) + (g[1] * 0.5).to(BF)        # evaluated in bf16: one rounding of the exact sum
            ok[f"{kind}_g16_{step}"] = bool(s["flag"]) and torch.equal(bits(s["g16"]), bits(want))
            ok[f"{kind}_g32_kept_{step}"] = torch.equal(s["g32"], local[kind]) and float(local[kind].abs().max()) > 0
            ok[f"{kind}_differs_{step}"] = not torch.equal(g[0], g[1])
            ns = gathered(s["normsq"], world)
            ok[f"{kind}_normsq_{step}"] = torch.equal(bits(ns[0]), bits(ns[1])) and float(ns[0]) > 0
            p = gathered(arena.p32, world)
            ok[f"{kind}_replicas_{step}"] = torch.equal(bits(p[0]), bits(p[1])) and bool(torch.isfinite(p[0]).all())
            ok[f"{kind}_cleared_{step}"] = not arena.g16_reduced
        if CASE == "accum":
            ok[f"accumulated_{step}"] = not torch.equal(local["image"], g_first) and float(g_first.abs().max()) > 0
    ret[f"rank{rank}"] = {k: bool(v) for k, v in ok.items()}
    dist.destroy_process_group()


def main():
    mgr = mp.Manager(); ret = mgr.dict()
    mp.spawn(worker, args=(2, int(os.environ.get("MASTER_PORT", "29551")), ret), nprocs=2, join=True)
    for rank in range(2):
        ok = dict(ret[f"rank{rank}"])
        print(f"case {CASE or 'plain'}, rank {rank}:", ok)
        assert ok and all(ok.values()), (rank, [k for k, v in ok.items() if not v])
    print("two-rank bf16 exchange OK")


if __name__ == "__main__":
    main()
