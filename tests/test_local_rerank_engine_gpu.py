"""Candidate re-ranking end to end on the `tiny` engine (64 regions, 16 words, width 128): LocalBank, local_rerank and the
`local` keys of retrieval_metrics / zero_shot_metrics against the re-rank definition applied on the CPU to the full matrices - the global
cosines with torch, the local similarities from the all-pairs kernel (local_sim_forward) on the same banked features - and the module's
`model.retrieval.local` keys.  The banks and the full matrices are built once and shared."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I32 = torch.float32, torch.float64, torch.int32
KS = (1, 5, 10)


def _engine():
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny")
    torch.manual_seed(0)
    return Engine(cfg, "cuda:0"), cfg


@functools.lru_cache(maxsize=None)
def banks(n_batches, B):
    """(engine, cfg, EmbeddingBank, LocalBank, G, L): n_batches synthetic batches of B pairs through Engine.embed; G float64 [N, N] = the
    cosines image x text with torch, L float64 [N, N] = the local similarities image x caption of the all-pairs kernel."""
    import bench
    from medmoe_amd.local_transposed import LocalSimScratch, local_sim_forward
    from medmoe_amd.retrieval import EmbeddingBank, LocalBank
    eng, cfg = _engine()
    bank, lb = EmbeddingBank(cfg.d_out, eng.device, capacity=B), LocalBank.for_engine(eng, capacity=B)      # both grow on the way
    for s in range(n_batches):
        b = bench.synthetic_batch(cfg, B, 70 + s, eng.device)
        img_g, txt_g = eng.embed(b)
        bank.add(img_g, txt_g, b["label"])
        lb.add(eng)
    N = n_batches * B
    assert len(bank) == len(lb) == N and (lb.w_global, lb.w_local, lb.temp1, lb.temp2) == (cfg.w_global, cfg.w_local, cfg.temp1, cfg.temp2)
    P, T = cfg.n_patch, cfg.max_len
    sc = LocalSimScratch(N, P, eng.device)
    L = torch.full((N, N), float("nan"), device=eng.device, dtype=F32)
    local_sim_forward(lb.img_l.view(N * P, cfg.d_out), lb.words, lb.cap_lens, lb.cap_lens.cpu().numpy(), cfg.temp1, cfg.temp2, gm3=sc.gm3,
                      wn=torch.empty(N, T, device=eng.device, dtype=F32), sim=L, **sc.gram_kw(N))
    G = bank.img.cpu().double() @ bank.txt.cpu().double().t()
    assert torch.isfinite(L).all()
    return eng, cfg, bank, lb, G, L.cpu().double()


def order_of(scores):
    """Key indices of every row under (score descending, index ascending)."""
    return torch.sort(scores, dim=1, descending=True, stable=True).indices


def reference_ranks(G, comb, k):
    """The re-rank definition on full [Nq, Nk] matrices: the k best keys by G; a target (key i for query i) inside that list ranks by the
    number of listed keys before it under (comb descending, index ascending), one outside keeps its rank under G."""
    N = G.shape[0]
    og = order_of(G)
    out = []
    for i in range(N):
        lst = og[i, :k].tolist()
        if i in lst:
            ranked = sorted(lst, key=lambda j: (-float(comb[i, j]), j))
            out.append(ranked.index(i))
        else:
            out.append(og[i].tolist().index(i))
    return torch.tensor(out)


def combined_of(cfg, G, L, agg="sum", lens=None, T=None):
    if agg == "mean":
        L = L - torch.log(lens.clamp(min=1, max=T).double())[None, :]
    return (cfg.w_global * G + cfg.w_local * L) / (cfg.w_global + cfg.w_local)


def test_rerank_of_48_pairs_matches_the_definition_on_the_full_matrices():
    from medmoe_amd.retrieval import local_rerank, rank_stats, recall_at_k, retrieval_metrics
    eng, cfg, bank, lb, G, L = banks(3, 16)
    N, k = 48, 16
    comb = combined_of(cfg, G, L)
    got = local_rerank(bank, lb, k)
    m = retrieval_metrics(bank, KS, local=lb, local_k=k)
    plain = retrieval_metrics(bank, KS)
    moved = 0
    for d, g_, c_ in (("i2t", G, comb), ("t2i", G.t(), comb.t())):
        want = reference_ranks(g_, c_, k)
        glob = reference_ranks(g_, g_, k)                                             # re-ranking with the global score itself: the global ranks
        assert torch.equal(got[d]["rank"].cpu(), want), d
        assert got[d]["top_idx"].shape == (N, k) and torch.equal(got[d]["top_idx"].cpu().long(), order_of(g_)[:, :k])
        inside = (got[d]["top_idx"].cpu().long() == torch.arange(N)[:, None]).any(dim=1)
        moved += int((want != glob).sum())
        print(f"{d}: {int(inside.sum())} of {N} targets inside their list of {k}, {int((want != glob).sum())} ranks changed by the local score")
        assert 0 < int(inside.sum()) and torch.equal(want[~inside], glob[~inside])
        for kk, v in recall_at_k(want, KS).items():
            assert m[f"{d}_local_R@{kk}"] == v
        assert (m[f"{d}_local_mean_rank"], m[f"{d}_local_median_rank"]) == rank_stats(want)
    assert moved > 0                                                                  # the local score does re-order something here
    assert set(m) == set(plain) | {f"{d}_local_{s}" for d in ("i2t", "t2i") for s in ("R@1", "R@5", "R@10", "mean_rank", "median_rank")}
    assert all(m[key] == v for key, v in plain.items())                               # the global-only keys keep their values
    # agg = "mean": log(len) of the caption off the local similarity
    got_m = local_rerank(bank, lb, k, agg="mean")
    comb_m = combined_of(cfg, G, L, "mean", lb.cap_lens.cpu(), cfg.max_len)
    for d, g_, c_ in (("i2t", G, comb_m), ("t2i", G.t(), comb_m.t())):
        assert torch.equal(got_m[d]["rank"].cpu(), reference_ranks(g_, c_, k)), d
    # a chunk smaller than the bank and small units: other Gram launches and unit tables, the same ranks (the Gram GEMM of another batch
    # size may round differently, so the ranks are compared, not the bits)
    got_c = local_rerank(bank, lb, k, chunk=20, unit_cap=3)
    for d in ("i2t", "t2i"):
        assert torch.equal(got_c[d]["rank"], got[d]["rank"]) and not torch.isnan(got_c[d]["local"]).any()


def test_a_list_as_deep_as_the_bank_ranks_by_the_full_combined_matrix():
    from medmoe_amd.retrieval import local_rerank
    eng, cfg, bank, lb, G, L = banks(1, 12)
    comb = combined_of(cfg, G, L)
    got = local_rerank(bank, lb, 16)                                                  # local_k = 16 >= N = 12: every key is a candidate
    for d, c_ in (("i2t", comb), ("t2i", comb.t())):
        st = torch.gather(c_, 1, torch.arange(12).reshape(-1, 1))
        j = torch.arange(12).reshape(1, -1)
        want = ((c_ > st) | ((c_ == st) & (j < torch.arange(12).reshape(-1, 1)))).sum(dim=1)
        assert got[d]["top_idx"].shape == (12, 12) and int(got[d]["top_idx"].min()) >= 0
        assert torch.equal(got[d]["rank"].cpu(), want), d
        # both directions' regrouping: every local value sits at its (query, candidate) place
        idx = got[d]["top_idx"].cpu().long()
        Ld = L if d == "i2t" else L.t()
        assert torch.equal(got[d]["local"].cpu().double(), torch.gather(Ld, 1, idx)), d


def test_zero_shot_local_accuracy():
    from medmoe_amd.local_transposed import LocalSimScratch, local_sim_forward
    from medmoe_amd.retrieval import class_embeddings, class_prompt_words, zero_shot_metrics
    import bench
    eng, cfg, bank, lb, _, _ = banks(3, 16)
    C, Pn, T, N, P = 3, 2, cfg.max_len, 48, cfg.n_patch
    pb = bench.synthetic_batch(cfg, C * Pn, 5, eng.device)
    ids, mask = pb["ids"].view(C, Pn, T), pb["attn_mask"].view(C, Pn, T)
    cls = class_embeddings(eng, ids, mask, chunk=4)
    words, lens = class_prompt_words(eng, ids, mask, chunk=4)
    assert tuple(words.shape) == (C * Pn, T, cfg.d_out) and words.dtype == torch.bfloat16 and lens.dtype == I32
    eng.embed_text(pb["ids"][:4], pb["attn_mask"][:4])                                # the first pass again: its words and lengths
    assert torch.equal(words[:4], eng.ws["words"][:4]) and torch.equal(lens[:4], eng.cap_lens[:4]) and 1 <= int(lens.min()) <= int(lens.max()) <= T
    plain = zero_shot_metrics(bank, cls, ks=(1, 2))
    m = zero_shot_metrics(bank, cls, ks=(1, 2), local=(lb, words, lens))
    assert all(torch.equal(m[k_], v) if torch.is_tensor(v) else m[k_] == v for k_, v in plain.items())          # zs_acc@k is unchanged
    # torch, from the all-pairs local matrix and the class embeddings
    sc = LocalSimScratch(N, P, eng.device)
    L = torch.empty(N, C * Pn, device=eng.device, dtype=F32)
    local_sim_forward(lb.img_l.view(N * P, cfg.d_out), words, lens, lens.cpu().numpy(), cfg.temp1, cfg.temp2, gm3=sc.gm3,
                      wn=torch.empty(C * Pn, T, device=eng.device, dtype=F32), sim=L, **sc.gram_kw(N))
    score = (cfg.w_global * (bank.img.cpu().double() @ cls.cpu().double().t())
             + cfg.w_local * L.cpu().double().view(N, C, Pn).mean(dim=2)) / (cfg.w_global + cfg.w_local)
    order = order_of(score)
    lab = bank.labels.cpu()
    for k in (1, 2):
        hit = (order[:, :k] == lab[:, None]).any(dim=1)
        assert m[f"zs_local_acc@{k}"] == float(hit.sum()) / N
        per = torch.stack([hit[lab == c].double().mean() for c in range(C)])
        assert torch.equal(m[f"zs_local_per_class_acc@{k}"].cpu(), per)
    top2 = torch.sort(score, dim=1, descending=True).values
    print(f"zero-shot: local acc@1 {m['zs_local_acc@1']:.3f}, global acc@1 {m['zs_acc@1']:.3f}, smallest gap between the two best classes "
          f"{float((top2[:, 0] - top2[:, 1]).min()):.3e}")


def test_refusals_name_the_key():
    from medmoe_amd.retrieval import EmbeddingBank, LocalBank, local_rerank
    bank = EmbeddingBank(128, "cuda")
    bank.add(torch.randn(4, 128, device="cuda"), torch.randn(4, 128, device="cuda"))
    for P, T, D in ((256, 40, 128), (576, 40, 128), (64, 40, 128), (64, 16, 96)):      # cfg4's / cfg3's regions, 64 regions with 40 words, width 96
        lb = LocalBank(P, T, D, "cuda", capacity=4)
        lb.add_features(torch.zeros(4, P, D), torch.zeros(4, T, D), torch.ones(4, dtype=I32))
        with pytest.raises(NotImplementedError, match="model.retrieval.local"):
            local_rerank(bank, lb, 4)
    lb = LocalBank(64, 16, 128, "cuda", capacity=4)
    with pytest.raises(ValueError, match="same batches"):
        local_rerank(bank, lb, 4)


def _mb(b):
    return {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"]}}


def test_module_logs_the_local_keys_next_to_unchanged_global_ones(monkeypatch, tmp_path):
    import bench
    from medmoe_amd.config import config_by_name
    from medmoe_amd.hydra_lite import compose, instantiate
    from medmoe_amd.trainer import Trainer
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    over = ["experiment=pretraining_medmoe", "model.fused_step=true", "model.model.vision.config_name=tiny2", "+model.retrieval.ks=[1,5]"]
    c2 = config_by_name("tiny2")

    def run(extra):
        torch.manual_seed(0)
        lit = instantiate(compose(os.path.join(ROOT, "configs"), "train.yaml", over + extra).model)
        dev = lit.model.engine.device
        batches = [_mb(bench.synthetic_batch(c2, 8, s, dev)) for s in (41, 42)]

        class DM:
            def val_dataloader(self):
                return batches

        return lit, Trainer().validate(lit, DM())

    _, base = run([])
    lit, got = run(["+model.retrieval.local=true", "+model.retrieval.local_k=8"])
    new = {f"val/{d}_local_{s}" for d in ("i2t", "t2i") for s in ("R@1", "R@5", "mean_rank", "median_rank")}
    assert set(got) == set(base) | new
    for key, v in base.items():
        if key == "val/loss":         # the loss heads add with fp32 atomics in arrival order: a few ulp (tests/test_eval_step_gpu.py)
            assert abs(got[key] - v) <= 1e-5 * abs(v)
        else:
            assert got[key] == v, key
    for d in ("i2t", "t2i"):
        assert 0.0 <= got[f"val/{d}_local_R@1"] <= got[f"val/{d}_local_R@5"] <= 1.0 and 0.0 <= got[f"val/{d}_local_median_rank"] <= 15.0
    assert len(lit._bank) == len(lit._lbank) == 16
    with pytest.raises(ValueError, match="local_k"):
        run(["+model.retrieval.local=true", "+model.retrieval.local_k=4"])            # ks = [1, 5] needs a list of 5
    # with zero_shot: val/zs_local_acc@k beside an unchanged val/zs_acc@k (3 classes x 2 prompts; the labels of the batches are in [0, 3))
    pb = bench.synthetic_batch(c2, 6, 5, torch.device("cuda:0"))
    path = str(tmp_path / "prompts.pt")
    torch.save({"prompt_ids": pb["ids"].view(3, 2, -1).cpu(), "prompt_mask": pb["attn_mask"].view(3, 2, -1).cpu(), "class_names": ["a", "b", "c"]}, path)
    zs = [f"+model.retrieval.zero_shot={path}", "+model.retrieval.zero_shot_ks=[1,2]"]
    _, zbase = run(zs)
    _, zgot = run(zs + ["+model.retrieval.local=true"])
    znew = {f"val/zs_local_acc@{k}" for k in (1, 2)} | {f"val/zs_local_per_class_acc@{k}/{n}" for k in (1, 2) for n in "abc"}
    assert set(zgot) == set(zbase) | new | znew and "val/zs_acc@1" in zbase
    same = lambda x, y: x == y or (x != x and y != y)                                 # NaN: a class without a sample
    assert all(same(zgot[key], v) for key, v in zbase.items() if key != "val/loss")
    assert 0.0 <= zgot["val/zs_local_acc@1"] <= zgot["val/zs_local_acc@2"] <= 1.0
