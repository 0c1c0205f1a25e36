"""Candidate re-ranking with the GLoRIA local similarity, host side (no GPU): the re-rank reducer and the pair-unit builder of
medmoe_amd/retrieval.py against brute-force loops, the header / signature table of medmoe_local_sim_pairs, and the module's keys."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")


def test_header_declares_the_pair_entry_and_the_kernel_body_is_shared():
    from medmoe_amd import ops
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    m = re.search(r"^int medmoe_local_sim_pairs\((.*)\);", hdr, re.M)
    assert m and m.group(1).endswith("hipStream_t stream")
    assert len(m.group(1).split(",")) == len(ops._SIGS["local_sim_pairs"]) + 1                # + the stream
    src = open(os.path.join(ROOT, "medmoe_amd", "csrc", "local_eval.hip")).read()
    # one device body behind a template flag, not a copy: one kernel definition, one MFMA score loop
    assert len(re.findall(r"__global__", src)) == 1 and "template <int HW, int NTT, bool PAIRS>" in src
    assert not re.search(r"atomic\w*\s*\(", src)                                              # one owner per slot: no atomic call


# ------------------------------------------------------------------------------------------------------------------------------------------
# rerank_ranks against a brute force
# ------------------------------------------------------------------------------------------------------------------------------------------
def _rerank_case():
    """N = 40 queries with K = 8 candidates each out of 40 keys, target i for query i.  Integer-valued scores (exact ties on purpose):
    queries 0..9 target inside and moved up, 10..19 inside and moved down, 20..29 inside and tied with a lower index, 30..39 outside."""
    g = torch.Generator().manual_seed(11)
    N, K = 40, 8
    top = torch.empty(N, K, dtype=torch.int32)
    comb = torch.empty(N, K)
    grank = torch.empty(N, dtype=torch.int32)
    for i in range(N):
        others = [j for j in torch.randperm(N, generator=g).tolist() if j != i]
        if i < 30:
            pos = 1 + int(torch.randint(0, K - 2, (1,), generator=g))                        # the target's place in the global order: 1 .. K - 2
            row = others[:K - 1]
            row.insert(pos, i)
            grank[i] = pos
        else:
            row = others[:K]
            grank[i] = K + int(torch.randint(0, N - K, (1,), generator=g))
        if i % 7 == 3:
            row[-1] = -1                                                                      # a short list
        top[i] = torch.tensor(row)
        sc = torch.randint(0, 6, (K,), generator=g).float() * 2.0                             # even values, ties among the others
        if i < 10:
            sc[pos] = 100.0                                                                   # best: moves up to 0
        elif i < 20:
            sc[pos] = -100.0                                                                  # worst: moves down
        elif i < 30:
            sc[pos] = 4.0
            lower = [p for p in range(K) if row[p] >= 0 and row[p] < i]
            higher = [p for p in range(K) if row[p] > i]
            if lower:
                sc[lower[0]] = 4.0                                                            # an equal score at a lower key index: ordered before
            if higher:
                sc[higher[0]] = 4.0                                                           # ... and at a higher one: ordered behind
        comb[i] = sc
        comb[i][top[i] < 0] = float("nan")                                                    # never scored
    return top, comb, torch.arange(N), grank


def _brute_rank(top, comb, target, grank):
    out = []
    for i in range(top.shape[0]):
        row = [(int(j), float(s)) for j, s in zip(top[i].tolist(), comb[i].tolist()) if j >= 0]
        t = int(target[i])
        mine = [s for j, s in row if j == t]
        if not mine:
            out.append(int(grank[i]))
            continue
        order = sorted(row, key=lambda js: (-js[1], js[0]))
        out.append([j for j, _ in order].index(t))
    return out


def test_rerank_ranks_matches_brute_force():
    from medmoe_amd.retrieval import rerank_ranks
    top, comb, target, grank = _rerank_case()
    got = rerank_ranks(top, comb, target, grank)
    want = _brute_rank(top, comb, target, grank)
    assert got.dtype == torch.int64 and got.tolist() == want
    inside = [(top[i] == i).any().item() for i in range(40)]
    up = [i for i in range(40) if inside[i] and want[i] < int(grank[i])]
    down = [i for i in range(40) if inside[i] and want[i] > int(grank[i])]
    tied = [i for i in range(40) if inside[i] and any(int(j) >= 0 and int(j) < i and float(s) == float(comb[i][top[i] == i])
                                                      for j, s in zip(top[i].tolist(), comb[i].tolist()))]
    outside = [i for i in range(40) if not inside[i]]
    assert up and down and tied and outside                                                   # every group is there
    assert all(want[i] == int(grank[i]) >= 8 for i in outside)                                # outside: the global rank, >= K
    assert all(want[i] >= 1 for i in tied)                                                    # the lower index with the same score goes first


# ------------------------------------------------------------------------------------------------------------------------------------------
# build_pair_units against a brute-force grouping
# ------------------------------------------------------------------------------------------------------------------------------------------
def _unit_case():
    g = torch.Generator().manual_seed(5)
    Nq, K, T = 30, 6, 77
    lens = [1, 16, 17, 32, 33, 48, 49, 64, 65, 77, 90, 0] + torch.randint(1, T + 1, (Nq - 12,), generator=g).tolist()      # 90, 0: clamped to T, 1
    cand = torch.stack([torch.randperm(Nq, generator=g)[:K] for _ in range(Nq)]).numpy().astype(np.int64)
    cand[:, 0] = 4                                                  # key 4 is everybody's candidate: 30 entries for one image in t2i
    cand[np.arange(Nq) == 4, 0] = 7
    for i in range(Nq):                                             # ... no key twice in a row (a top-K list names a key once)
        seen = set()
        for p in range(K):
            if int(cand[i, p]) in seen:
                cand[i, p] = -1
            seen.add(int(cand[i, p]))
    cand[3, 2:] = -1; cand[9, :] = -1                               # short and empty lists
    return cand, lens, T


@pytest.mark.parametrize("unit_cap", [4, 16])
@pytest.mark.parametrize("query_is_image", [True, False])
def test_build_pair_units_matches_brute_force(query_is_image, unit_cap):
    from medmoe_amd.retrieval import build_pair_units
    cand, lens, T = _unit_case()
    Nq, K = cand.shape
    tables = build_pair_units(cand, query_is_image, lens, T, unit_cap)
    cls_of = lambda c: (min(max(lens[c], 1), T) + 15) // 16
    want = {}                                                       # (image, caption) -> slot, every pair of the matrix with a candidate
    for q in range(Nq):
        for p in range(K):
            if cand[q, p] >= 0:
                pair = (q, int(cand[q, p])) if query_is_image else (int(cand[q, p]), q)
                assert pair not in want
                want[pair] = q * K + p
    got = {}
    for ntt, (units, pair_cap, pair_slot) in tables.items():
        assert units.dtype == pair_cap.dtype == pair_slot.dtype == np.int32 and units.shape[1] == 4
        assert pair_cap.shape == pair_slot.shape and (pair_cap >= 0).all() and (pair_slot >= 0).all()
        assert all(cls_of(int(c)) == ntt for c in pair_cap)         # the class table holds captions of its class only
        covered = np.zeros(pair_cap.shape[0], np.int64)
        for b, first, count, zero in units.tolist():
            assert zero == 0 and 1 <= count <= unit_cap and 0 <= first and first + count <= pair_cap.shape[0]
            covered[first:first + count] += 1
            for e in range(first, first + count):
                pair = (b, int(pair_cap[e]))
                assert pair not in got
                got[pair] = int(pair_slot[e])
        assert (covered == 1).all()                                 # every entry belongs to exactly one unit
        assert (np.diff(units[:, 0]) >= 0).all()                    # grouped by image, ascending
        per_image = {}
        for b, _, count, _ in units.tolist():
            per_image.setdefault(b, []).append(count)
        for b, counts in per_image.items():                         # an image's run is cut greedily: full units, then the remainder
            assert all(c == unit_cap for c in counts[:-1])
    assert got == want                                              # every (query, candidate) pair once, with its slot; the -1 entries are gone
    if not query_is_image and unit_cap == 4:
        n4 = sum(int((u[:, 0] == 4).sum()) for u, _, _ in tables.values())
        assert n4 > len(tables)                                     # image 4 (29 captions) is cut into several units in some class


def test_build_pair_units_of_an_empty_matrix():
    from medmoe_amd.retrieval import build_pair_units
    assert build_pair_units(np.full((3, 4), -1), True, [5, 5, 5], 16, 8) == {}
    with pytest.raises(ValueError, match="unit_cap"):
        build_pair_units(np.zeros((1, 1), np.int64), True, [5], 16, 0)


# ------------------------------------------------------------------------------------------------------------------------------------------
# module keys, configuration
# ------------------------------------------------------------------------------------------------------------------------------------------
class _Fused:
    fused_step, model = True, None


def test_module_key_validation():
    from src.models.medmoe_module import MedMoEPretrainingLightningModule as M
    with pytest.raises(KeyError, match=r"locl.*local, local_k, local_agg"):
        M._retrieval_block(_Fused(), {"ks": [1], "locl": True})
    with pytest.raises(ValueError, match="local_k"):
        M._retrieval_block(_Fused(), {"ks": [1, 5], "local": True, "local_k": 17})
    with pytest.raises(ValueError, match="local_k"):
        M._retrieval_block(_Fused(), {"ks": [1, 5], "local": True, "local_k": 0})
    with pytest.raises(ValueError, match="local_k"):
        M._retrieval_block(_Fused(), {"ks": [1, 20], "local": True})
    with pytest.raises(ValueError, match="local_agg"):
        M._retrieval_block(_Fused(), {"ks": [1], "local": True, "local_agg": "max"})
    blk = M._retrieval_block(_Fused(), {"ks": [1, 5], "local": True, "local_k": 8, "local_agg": "mean"})
    assert blk["local"] is True and blk["local_k"] == 8 and blk["local_agg"] == "mean" and blk["ks"] == (1, 5)
    off = M._retrieval_block(_Fused(), {"ks": [1, 20], "local": False})                      # without local the list depth does not bind ks
    assert "local" not in off and off["ks"] == (1, 20)


def test_retrieval_metrics_refuses_ks_deeper_than_the_list():
    from medmoe_amd.retrieval import EmbeddingBank, LocalBank, retrieval_metrics
    bank, lb = EmbeddingBank(64, "cpu"), LocalBank(64, 16, 64, "cpu", capacity=2)
    with pytest.raises(ValueError, match="local_k"):
        retrieval_metrics(bank, ks=(1, 20), local=lb)
    with pytest.raises(ValueError, match="local_k"):
        retrieval_metrics(bank, ks=(1, 10), local=lb, local_k=8)


def test_local_bank_grows_and_keeps_rows():
    from medmoe_amd.retrieval import LocalBank
    g = torch.Generator().manual_seed(2)
    P, T, D = 4, 3, 8
    img, words = torch.randn(11, P, D, generator=g).bfloat16(), torch.randn(11, T, D, generator=g).bfloat16()
    lens = torch.randint(1, T + 1, (11,), generator=g).to(torch.int32)
    lb = LocalBank(P, T, D, "cpu", capacity=2)
    for s, e in ((0, 3), (3, 4), (4, 11)):
        lb.add_features(img[s:e], words[s:e], lens[s:e])
    assert len(lb) == 11 and torch.equal(lb.img_l, img) and torch.equal(lb.words, words) and torch.equal(lb.cap_lens, lens)
    assert lb.img_l.dtype == torch.bfloat16 and lb.cap_lens.dtype == torch.int32
    with pytest.raises(ValueError):
        lb.add_features(img[:2, :2], words[:2], lens[:2])
    lb.reset()
    assert len(lb) == 0 and lb.words.shape == (0, T, D)


def test_the_local_experiment_composes(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_retrieval_local"])
    r = dict(cfg.model.retrieval)
    assert cfg.model.fused_step is True and r["local"] is True and r["local_k"] == 16 and r["local_agg"] == "sum" and list(r["ks"]) == [1, 5, 10]
    on = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2", "+model.retrieval.ks=[1,5]", "+model.retrieval.local=true"])
    assert on.model.retrieval.local is True
