"""The MLM launches (csrc/mlm.hip): the mask against the host restatement of tests/mlm_reference.py, bit for bit, and the fused
decoder + cross-entropy with both backward kernels against float64 torch on the same bf16-rounded operands.

Tolerances (profiles/r23_notes.md has the measured values every test prints):
  lse, terms, loss   fp32 accumulation of exact bf16 products: the bar is 2 x the largest deviation measured over the cases below.
  dz, dE, dbias      two bf16 roundings (P, and the stored dz): rel-L2, the bar 2 x the measured maximum and never above 2^-7."""
import functools

import numpy as np
import pytest
import torch

import mlm_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 2 x the largest value the cases below measured on the MI355X (profiles/r23_notes.md lists them per case)
LSE_ABS_TOL = 3.9e-5       # lse / terms, absolute; measured 1.90e-5 / 1.94e-5 (the +-60 variant at D = 1024: |lse| = 60, 5 ulp)
LOSS_REL_TOL = 1.0e-7      # measured 5.0e-8
GRAD_REL_L2_TOL = 2.0 ** -7                                             # the two bf16 roundings: no measured bar may pass it
GRAD_MEASURED_TOL = {"dz": 4.3e-3, "dE": 3.5e-3, "dbias": 3.2e-6}       # measured 2.11e-3, 1.72e-3, 1.56e-6 (dbias sums the fp32 P)

IDS = dict(cls_id=2, sep_id=3, pad_id=0, mask_id=4)


# ------------------------------------------------------------------------------------------------------------------------------------------
# mask
# ------------------------------------------------------------------------------------------------------------------------------------------
def _batch(B, T, V, seed, all_candidates=False):
    """[CLS] words [SEP] [PAD]... captions of random lengths (or B x T plain words with attention 1 everywhere)"""
    g = np.random.default_rng(seed)
    ids = g.integers(5, V, size=(B, T)).astype(np.int32)
    attn = np.ones((B, T), np.uint8)
    if not all_candidates:
        for b in range(B):
            n = int(g.integers(3, T + 1))
            ids[b, 0], ids[b, n - 1] = IDS["cls_id"], IDS["sep_id"]
            ids[b, n:], attn[b, n:] = IDS["pad_id"], 0
        attn[0, 1] = 0                                                 # an ordinary word with attention 0: not a candidate either
    return ids, attn


def _gpu_mask(ids, attn, V, seed, step, p, sample_offset=0, tok_row=None):
    from medmoe_amd import ops
    out = ops.mlm_mask(torch.from_numpy(ids).to(DEV), torch.from_numpy(attn).to(DEV), vocab=V, seed=seed, step=step, p=p,
                       sample_offset=sample_offset, tok_row=None if tok_row is None else torch.from_numpy(tok_row).to(DEV), **IDS)
    torch.cuda.synchronize()
    ids_masked, labels, rows, row_labels, count = (t.cpu().numpy() for t in out)
    n = int(count[0])
    return {"ids_masked": ids_masked, "labels": labels, "rows": rows[:n], "row_labels": row_labels[:n], "count": n}


@pytest.mark.parametrize("B,T", [(5, 16), (64, 80)])
@pytest.mark.parametrize("sample_offset", [0, 7])
def test_mask_is_bit_equal_to_the_host_rule(B, T, sample_offset):
    V = 97
    ids, attn = _batch(B, T, V, seed=B)
    kw = dict(seed=0x1234567890ABCDEF, step=11, p=0.15, sample_offset=sample_offset)
    want = R.mlm_mask_ref(ids, attn, vocab=V, **IDS, **kw)
    got = _gpu_mask(ids, attn, V, **kw)
    assert got["count"] == want["count"] and (B == 5 or want["count"] > 100)
    for k in ("ids_masked", "labels", "rows", "row_labels"):
        assert np.array_equal(got[k], want[k]), k
    sel = got["labels"] >= 0
    special = (attn == 0) | (ids == IDS["cls_id"]) | (ids == IDS["sep_id"]) | (ids == IDS["pad_id"])
    assert not (sel & special).any()
    assert np.array_equal(got["labels"][sel], ids[sel]) and (got["labels"][~sel] == -1).all()
    assert np.array_equal(got["ids_masked"][~sel], ids[~sel])
    assert (np.diff(got["rows"]) > 0).all() and np.array_equal(got["rows"], np.flatnonzero(sel.reshape(-1)))
    assert np.array_equal(got["row_labels"], ids.reshape(-1)[got["rows"]])
    if sample_offset:                                                  # the draw belongs to the GLOBAL sample: rank 1's sample 0 is sample 7
        base = R.mlm_mask_ref(np.concatenate([ids[:1]] * 8), np.concatenate([attn[:1]] * 8), vocab=V, **IDS, **dict(kw, sample_offset=0))
        assert np.array_equal(base["labels"][7], got["labels"][0])


def test_mask_padded_and_packed_row_lists_name_the_same_tokens():
    from medmoe_amd import ops
    B, T, V = 64, 80, 97
    ids, attn = _batch(B, T, V, seed=3)
    attn[0, 1] = 1
    tok_row = torch.empty(B * T, dtype=torch.int32, device=DEV)
    src_of_row = torch.empty(B * T, dtype=torch.int32, device=DEV)
    seq_off = torch.empty(B + 1, dtype=torch.int32, device=DEV)
    cnt = torch.empty(1, dtype=torch.int32, device=DEV)
    ops.call("text_pack", torch.from_numpy(attn).to(DEV), tok_row, src_of_row, seq_off, cnt, B, T)
    kw = dict(seed=5, step=2, p=0.15)
    padded = _gpu_mask(ids, attn, V, **kw)
    packed = _gpu_mask(ids, attn, V, tok_row=tok_row.cpu().numpy(), **kw)
    assert padded["count"] == packed["count"] > 100
    assert (np.diff(packed["rows"]) > 0).all()
    assert np.array_equal(src_of_row.cpu().numpy()[packed["rows"]], padded["rows"])          # the same (caption, position) set
    assert np.array_equal(packed["row_labels"], padded["row_labels"]) and np.array_equal(packed["ids_masked"], padded["ids_masked"])
    want = R.mlm_mask_ref(ids, attn, vocab=V, tok_row=tok_row.cpu().numpy(), **IDS, **kw)
    assert np.array_equal(packed["rows"], want["rows"])


def test_mask_repeats_per_step_and_moves_with_it():
    V = 97
    ids, attn = _batch(64, 80, V, seed=4)
    a = _gpu_mask(ids, attn, V, seed=9, step=3, p=0.15)
    b = _gpu_mask(ids, attn, V, seed=9, step=3, p=0.15)
    c = _gpu_mask(ids, attn, V, seed=9, step=4, p=0.15)
    d = _gpu_mask(ids, attn, V, seed=10, step=3, p=0.15)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["labels"], c["labels"]) and not np.array_equal(a["labels"], d["labels"])


@pytest.mark.parametrize("p", [0.15, 0.5])
def test_mask_rates_lie_within_four_sigma(p):
    B, T, V = 64, 80, 28996
    ids, attn = _batch(B, T, V, seed=6, all_candidates=True)
    n = B * T
    kw = dict(seed=77, step=1, p=p)
    want = R.mlm_mask_ref(ids, attn, vocab=V, **IDS, **kw)
    # the rule itself first (the host restatement), then the kernel bit for bit against it
    k = want["count"]
    assert abs(k / n - p) <= 4 * (p * (1 - p) / n) ** 0.5, (k, n)
    for action, q in ((0, 0.8), (1, 0.1), (2, 0.1)):
        share = float((want["action"] == action).sum()) / k
        assert abs(share - q) <= 4 * (q * (1 - q) / k) ** 0.5, (action, share)
    rand = want["ids_masked"][want["action"] == 1]
    assert rand.min() >= 0 and rand.max() < V and rand.max() > V // 2
    got = _gpu_mask(ids, attn, V, **kw)
    assert got["count"] == k
    for key in ("ids_masked", "labels", "rows", "row_labels"):
        assert np.array_equal(got[key], want[key]), key
    assert (got["ids_masked"][want["action"] == 0] == IDS["mask_id"]).all()


def test_mask_of_an_all_padding_batch_is_empty():
    ids = np.full((5, 16), IDS["pad_id"], np.int32)
    got = _gpu_mask(ids, np.zeros((5, 16), np.uint8), 97, seed=1, step=1, p=0.5)
    assert got["count"] == 0 and (got["labels"] == -1).all() and np.array_equal(got["ids_masked"], ids)
    ids, attn = _batch(5, 16, 97, seed=8)
    ids[attn == 1] = IDS["cls_id"]                                     # attended, but every token is special
    assert _gpu_mask(ids, attn, 97, seed=1, step=1, p=0.5)["count"] == 0


# ------------------------------------------------------------------------------------------------------------------------------------------
# gather / scatter-add / product over the listed rows
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_rows_gather_scatter_add_and_mul():
    from medmoe_amd import ops
    g = torch.Generator().manual_seed(0)
    R_, D, Mb, n = 300, 64, 100, 37
    src = torch.randn(R_, D, generator=g).bfloat16().to(DEV)
    rows = torch.sort(torch.randperm(R_, generator=g)[:n]).values.to(torch.int32)
    rows_d = torch.cat([rows, torch.full((Mb - n,), 10 ** 9, dtype=torch.int32)]).to(DEV)      # the tail is never read
    count = torch.tensor([n], dtype=torch.int32, device=DEV)
    dst = torch.full((Mb, D), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.rows_gather(src, rows_d, count, dst)
    assert torch.equal(dst[:n].cpu(), src.cpu()[rows.long()]) and (dst[n:] == 7.0).all()
    upd = torch.randn(Mb, D, generator=g).bfloat16()
    upd[n:] = float("nan")
    base = src.clone()
    ops.rows_scatter_add(upd.to(DEV), rows_d, count, base)
    want = src.cpu().clone()
    want[rows.long()] = (want[rows.long()].float() + upd[:n].float()).bfloat16()
    assert torch.equal(base.cpu(), want)
    a, b = torch.randn(Mb, D, generator=g).bfloat16(), torch.randn(Mb, D, generator=g).bfloat16()
    a[n:] = float("nan")
    out = torch.full((Mb, D), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.rows_mul(a.to(DEV), b.to(DEV), count, out)
    assert torch.equal(out[:n].cpu(), (a[:n].float() * b[:n].float()).bfloat16()) and (out[n:] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------------
# decoder + cross-entropy
# ------------------------------------------------------------------------------------------------------------------------------------------
# (M_bound, count, V, D): one partial vocabulary tile; tile + 1 rows with two 64-tiles + a remainder of the vocabulary; the real width; empty;
# the real vocabulary (114 forward tiles per row); the widest build of the backward template (D = 1024: the one that spills to scratch)
CASES = [(1, 1, 97, 64), (70, 65, 300, 64), (130, 130, 1000, 768), (64, 0, 97, 64), (200, 137, 28996, 64), (70, 65, 300, 1024)]
VARIANTS = ["unit", "big"]          # big: z scaled until the logits reach +-60 (the running maximum must carry the sum)


@functools.lru_cache(maxsize=None)
def _case(i, variant):
    Mb, n, V, D = CASES[i]
    g = torch.Generator().manual_seed(500 + i)
    E = (torch.randn(V, D, generator=g) / D ** 0.5).bfloat16()
    bias = torch.randn(V, generator=g) * 0.1
    z = torch.randn(Mb, D, generator=g)
    if variant == "big" and n:
        top = float((z[:n].double() @ E.double().t()).abs().max())
        z = z * (63.0 / top)
    z = z.bfloat16()
    labels = torch.randint(0, V, (Mb,), generator=g).to(torch.int32)
    labels[0] = V - 1                                                  # the last column
    if n > 1:
        labels[n - 1] = V - 2                                          # the last partial tile (64-wide backward, 256-wide forward)
        labels[1] = 0
    scale = 0.25 if i % 2 else 1.0
    ref = R.vocab_ce_ref(z.float(), E.float(), bias, labels.numpy(), n, scale)
    if variant == "big" and n:
        assert ref["logit_max"] >= 60.0
    z = z.clone()
    z[n:] = float("nan")                                               # data past the count: must leave no trace
    return z, E, bias, labels, scale, ref


def _run(i, variant):
    from medmoe_amd import ops
    Mb, n, V, D = CASES[i]
    z, E, bias, labels, scale, _ = _case(i, variant)
    zd, Ed, bd, ld = z.to(DEV), E.to(DEV), bias.to(DEV), labels.to(DEV)
    count = torch.tensor([n], dtype=torch.int32, device=DEV)
    loss, counts, lse, terms = ops.vocab_ce_fwd(zd, Ed, bd, ld, count, scale)
    dz = torch.full((Mb, D), 7.0, dtype=torch.bfloat16, device=DEV)
    dE = torch.zeros(V, D, device=DEV)
    dbias = torch.zeros(V, device=DEV)
    ops.vocab_ce_bwd(zd, Ed, bd, ld, lse, count, scale, dz=dz, dE=dE, dbias=dbias)
    dE1, db1 = dE.clone(), dbias.clone()
    ops.vocab_ce_bwd(zd, Ed, bd, ld, lse, count, scale, dE=dE, dbias=dbias)                      # accumulates
    torch.cuda.synchronize()
    return {"loss": loss.cpu(), "counts": counts.cpu(), "lse": lse.cpu(), "terms": terms.cpu(), "dz": dz.cpu(), "dE": dE1.cpu(), "dbias": db1.cpu(),
            "dE2": dE.cpu(), "dbias2": dbias.cpu()}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"M{m}-n{n}-V{v}-D{d}" for m, n, v, d in CASES])
def test_vocab_ce_matches_float64(i, variant):
    Mb, n, V, D = CASES[i]
    ref = _case(i, variant)[5]
    a = _run(i, variant)
    b = _run(i, variant)
    for k in a:                                                        # two runs: the same bits
        assert torch.equal(a[k], b[k]), k
    for k in ("loss", "lse", "terms", "dE", "dbias", "dE2", "dbias2"):
        assert torch.isfinite(a[k]).all(), k                           # the NaN rows past the count left no trace
    assert a["counts"].tolist() == [n, ref["hits"]]
    assert (a["lse"][n:] == 0).all() and (a["terms"][n:] == 0).all()
    assert (a["dz"][n:] == 7.0).all()                                  # rows past the count: untouched
    assert torch.equal(a["dE2"], 2 * a["dE"]) and torch.equal(a["dbias2"], 2 * a["dbias"])       # += : x + x is exact
    if n == 0:
        assert float(a["loss"]) == 0.0 and not a["dE"].any() and not a["dbias"].any()
        return
    assert torch.isfinite(a["dz"][:n].float()).all()
    e_lse = float((a["lse"][:n].double() - ref["lse"]).abs().max())
    e_terms = float((a["terms"][:n].double() - ref["terms"]).abs().max())
    e_loss = abs(float(a["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    e_grad = {k: R.rel_l2(a[k][:n] if k == "dz" else a[k], ref[k]) for k in ("dz", "dE", "dbias")}
    print(f"\nvocab_ce {CASES[i]} {variant}: |lse| max {float(ref['lse'].abs().max()):.1f} err lse {e_lse:.3g} terms {e_terms:.3g} loss(rel) {e_loss:.3g} "
          + " ".join(f"{k} {v:.3g}" for k, v in e_grad.items()))
    assert e_lse <= LSE_ABS_TOL and e_terms <= LSE_ABS_TOL and e_loss <= LOSS_REL_TOL
    for k, v in e_grad.items():
        assert v <= min(GRAD_MEASURED_TOL[k], GRAD_REL_L2_TOL), (k, v)


def test_vocab_ce_refuses_bad_shapes_before_a_launch():
    from medmoe_amd import ops
    count = torch.ones(1, dtype=torch.int32, device=DEV)
    lab = torch.zeros(4, dtype=torch.int32, device=DEV)
    for D in (32, 96, 1088):
        z, E, b = torch.zeros(4, D, dtype=torch.bfloat16, device=DEV), torch.zeros(8, D, dtype=torch.bfloat16, device=DEV), torch.zeros(8, device=DEV)
        with pytest.raises(ValueError, match="multiple of 64"):
            ops.vocab_ce_fwd(z, E, b, lab, count)
        with pytest.raises(RuntimeError, match="code -2"):             # the library's own refusal, behind the wrapper's
            ops.call("vocab_ce_bwd_dx", z, E, b, lab, b, count, 1.0, z, 4, 8, D)
    z, E, b = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV), torch.zeros(1, 64, dtype=torch.bfloat16, device=DEV), torch.zeros(1, device=DEV)
    with pytest.raises(ValueError, match=">= 2"):
        ops.vocab_ce_fwd(z, E, b, lab, count)
