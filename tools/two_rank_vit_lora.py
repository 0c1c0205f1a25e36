#!/usr/bin/env python3
"""LoRA adapters on the frozen ViT tower (MedMoEConfig.vit_lora) under two ranks sharing ONE GPU (gloo backend, as
tools/two_rank_lora.py; config tiny, 8 pairs per rank, adapters on query and value with B random so that both A and B receive a gradient).
TWO_RANK_LORA_COMM = fp32 | bf16 picks the number format of the gradient exchange.  Every rank checks, after each of two steps:
  * the adapters' arena and the image arena are bit-identical on both ranks, finite; the adapters, the router and the experts moved and
    the frozen backbone did not;
  * the ranks' local adapter gradients differed before the exchange (each rank saw its own images);
  * with bf16: what Adam read for the adapters and for the image arena's trainable tail was the reduced bf16 gradient (g16_reduced set in
    front of adam_step, cleared after), and the image arena's bf16 copy covers that tail only."""
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
    cfg.vit_lora, cfg.vit_lora_r, cfg.lr = True, 8, 1e-3
    eng = Engine(cfg, "cuda:0", seed=0)
    lo, P = eng.vlora, eng.params
    assert eng.dist and eng.world == world and lo is not None and eng.optimizer_stores()["vit_lora"] is lo and eng.vit_frozen
    g = torch.Generator().manual_seed(3)
    lo.load_named({"vit." + n: 0.05 * torch.randn(lo.D, lo.r, generator=g) for n in lo.true_names() if n.endswith("lora_B")})
    seen = {}

    def spy(arena, tag):
        adam = arena.adam_step

        def adam_spy(normsq, *a, **k):
            torch.cuda.synchronize()
            seen[tag] = arena.g16_reduced
            seen["normsq"] = normsq.clone()
            return adam(normsq, *a, **k)
        arena.adam_step = adam_spy
    spy(lo, "adapters"); spy(P, "image")
    ok = {}
    tf = P.train_from
    for step in range(2):
        full = bench.synthetic_batch(cfg, 16, 777 + step, eng.device)
        mine = {k: v[rank * 8: rank * 8 + 8].contiguous() for k, v in full.items()}
        before, before_img = lo.p32.clone(), P.p32.clone()
        eng.train_step(mine, optimizer=False)                        # the rank-local gradient, no exchange
        torch.cuda.synchronize()
        gl = gathered(lo.g32, world)
        ok[f"local_grads_differ_{step}"] = not torch.equal(gl[0], gl[1]) and float(gl[0].abs().max()) > 0
        eng.train_step(mine)
        torch.cuda.synchronize()
        ok[f"exchange_format_{step}"] = all(bool(seen[t]) == (COMM == "bf16") for t in ("adapters", "image")) and not lo.g16_reduced \
            and not P.g16_reduced
        ns = gathered(seen["normsq"], world)
        ok[f"normsq_{step}"] = torch.equal(bits(ns[0]), bits(ns[1])) and float(ns[0]) > 0
        for kind, arena in (("adapters", lo), ("image", P)):
            p = gathered(arena.p32, world)
            ok[f"{kind}_replicas_{step}"] = torch.equal(bits(p[0]), bits(p[1])) and bool(torch.isfinite(p[0]).all())
        ok[f"adapters_moved_{step}"] = float((lo.p32 - before).abs().max()) > 0 and lo.pad_is_zero()
        ok[f"tail_moved_backbone_frozen_{step}"] = float((P.p32[tf:] - before_img[tf:]).abs().max()) > 0 and torch.equal(P.p32[:tf], before_img[:tf])
    if COMM == "bf16":
        ok["g16_covers_the_tail"] = P.g16.numel() == P.n_train and lo.g16.numel() == lo.numel
    ret[f"rank{rank}"] = {k: bool(v) for k, v in ok.items()}
    dist.destroy_process_group()


def main():
    mgr = mp.Manager(); ret = mgr.dict()
    mp.spawn(worker, args=(2, int(os.environ.get("MASTER_PORT", "29571")), ret), nprocs=2, join=True)
    for rank in range(2):
        ok = dict(ret[f"rank{rank}"])
        print(f"exchange {COMM}, rank {rank}:", ok)
        assert ok and all(ok.values()), (rank, [k for k, v in ok.items() if not v])
    print("two-rank ViT LoRA OK")


if __name__ == "__main__":
    main()
