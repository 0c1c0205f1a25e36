#!/usr/bin/env python3
"""LoRA adapters of the text tower (MedMoEConfig.text_lora) under two ranks sharing ONE GPU (gloo backend, as
tools/two_rank_bf16.py; config tiny, 8 pairs per rank, adapters on query and value with B random so that both A and B receive a gradient).
TWO_RANK_LORA_COMM = fp32 | bf16 picks the number format of the gradient exchange.  Every rank checks, after each of two steps:
  * the adapters' arena and the image arena are bit-identical on both ranks, finite, and moved;
  * the ranks' local adapter gradients differed before the exchange (each rank saw its own captions);
  * with bf16: what Adam read for the adapters was the reduced bf16 gradient (g16_reduced set in front of adam_step, cleared after)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

COMM = os.environ.get("TWO_RANK_LORA_COMM", "fp32")
bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def gathered(t, world):
    parts = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(parts, t.contiguous())
    return parts


def worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("MEDMOE_GRAD_COMM", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny")
    cfg.grad_comm_dtype = COMM
    cfg.text_lora, cfg.text_lora_r, cfg.lr = True, 8, 1e-3
    eng = Engine(cfg, "cuda:0", seed=0)
    lo = eng.lora
    assert eng.dist and eng.world == world and lo is not None and eng.optimizer_stores()["text"] is lo
    g = torch.Generator().manual_seed(3)
    lo.load_named({"text." + n: 0.05 * torch.randn(lo.D, lo.r, generator=g) for n in lo.true_names() if n.endswith("lora_B")})
    seen = {}
    adam = lo.adam_step

    def adam_spy(normsq, *a, **k):
        torch.cuda.synchronize()
        seen.update(flag=lo.g16_reduced, normsq=normsq.clone())
        return adam(normsq, *a, **k)
    lo.adam_step = adam_spy
    ok = {}
    for step in range(2):
        full = bench.synthetic_batch(cfg, 16, 777 + step, eng.device)
        mine = {k: v[rank * 8: rank * 8 + 8].contiguous() for k, v in full.items()}
        before = lo.p32.clone()
        eng.train_step(mine, optimizer=False)                        # the rank-local gradient, no exchange
        torch.cuda.synchronize()
        gl = gathered(lo.g32, world)
        ok[f"local_grads_differ_{step}"] = not torch.equal(gl[0], gl[1]) and float(gl[0].abs().max()) > 0
        eng.train_step(mine)
        torch.cuda.synchronize()
        ok[f"exchange_format_{step}"] = bool(seen["flag"]) == (COMM == "bf16") and not lo.g16_reduced
        ns = gathered(seen["normsq"], world)
        ok[f"normsq_{step}"] = torch.equal(bits(ns[0]), bits(ns[1])) and float(ns[0]) > 0
        for kind, arena in (("adapters", lo), ("image", eng.params)):
            p = gathered(arena.p32, world)
            ok[f"{kind}_replicas_{step}"] = torch.equal(bits(p[0]), bits(p[1])) and bool(torch.isfinite(p[0]).all())
        ok[f"adapters_moved_{step}"] = float((lo.p32 - before).abs().max()) > 0 and lo.pad_is_zero()
    ret[f"rank{rank}"] = {k: bool(v) for k, v in ok.items()}
    dist.destroy_process_group()


def main():
    mgr = mp.Manager(); ret = mgr.dict()
    mp.spawn(worker, args=(2, int(os.environ.get("MASTER_PORT", "29561")), ret), nprocs=2, join=True)
    for rank in range(2):
        ok = dict(ret[f"rank{rank}"])
        print(f"exchange {COMM}, rank {rank}:", ok)
        assert ok and all(ok.values()), (rank, [k for k, v in ok.items() if not v])
    print("two-rank LoRA OK")


if __name__ == "__main__":
    main()
