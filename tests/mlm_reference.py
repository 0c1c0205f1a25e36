"""Host restatements the MLM tests share: the mask rule of medmoe_mlm_mask on a numpy Philox, and the tied decoder + cross-entropy
with its gradients in float64 torch.  Not a test module."""
from fractions import Fraction

import numpy as np
import torch

SITE_MLM = 0x60000000
T80 = int(Fraction(8, 10) * 2 ** 32)           # floor(0.8 * 2^32)
T90 = int(Fraction(9, 10) * 2 ** 32)


# Philox4x32-10 (Salmon et al., SC'11) as tests/test_text_dropout_host.py states it (its known-answer test covers these lines)
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint32 arrays (or scalars) in, the four output words out"""
    c = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF)]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def mlm_mask_ref(ids, attn, *, cls_id, sep_id, pad_id, mask_id, vocab, seed, step, p, sample_offset=0, tok_row=None):
    """The mask rule: token t of global sample g = sample_offset + b owns group g * T + t of (seed, step, SITE_MLM); word 0 < floor(p 2^32)
    selects a candidate, word 1 picks [MASK] (< T80) / random id mulhi(word 2, V) (< T90) / keep.  ids, attn: integer arrays [B, T].
    Returns a dict: ids_masked, labels [B, T]; rows, row_labels [count]; count; action [B, T] (-1 not selected, 0 mask, 1 random, 2 keep)."""
    ids = np.asarray(ids, dtype=np.int64)
    attn = np.asarray(attn)
    B, T = ids.shape
    group = ((np.arange(B, dtype=np.uint64)[:, None] + np.uint64(sample_offset)) * np.uint64(T) + np.arange(T, dtype=np.uint64)[None, :]).reshape(-1)
    seed &= 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(group & np.uint64(0xFFFFFFFF), group >> np.uint64(32), np.full(group.shape, SITE_MLM, np.uint64),
                      np.full(group.shape, step & 0xFFFFFFFF, np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    w0, w1, w2 = (v.reshape(B, T).astype(np.uint64) for v in w[:3])
    cand = (attn != 0) & (ids != cls_id) & (ids != sep_id) & (ids != pad_id)
    sel = cand & (w0 < np.uint64(int(Fraction(p) * 2 ** 32)))
    action = np.where(sel, np.where(w1 < np.uint64(T80), 0, np.where(w1 < np.uint64(T90), 1, 2)), -1)
    rand_id = ((w2 * np.uint64(vocab)) >> np.uint64(32)).astype(np.int64)
    ids_masked = np.where(action == 0, mask_id, np.where(action == 1, rand_id, ids))
    labels = np.where(sel, ids, -1)
    flat = np.flatnonzero(sel.reshape(-1))                             # ascending b * T + t
    rows = flat if tok_row is None else np.asarray(tok_row).reshape(-1)[flat]
    return {"ids_masked": ids_masked.astype(np.int32), "labels": labels.astype(np.int32), "rows": rows.astype(np.int32),
            "row_labels": ids.reshape(-1)[flat].astype(np.int32), "count": int(flat.size), "action": action, "tokens": flat}


def vocab_ce_ref(z, E, bias, labels, count, loss_scale=1.0):
    """float64: logits = z[:count] E^T + bias, loss = loss_scale * mean(lse - logit[target]) (0 for count 0) and its gradients.  z, E: the
    bf16-rounded operands (any float dtype), labels integer [>= count].  Returns a dict of float64 tensors (dz / lse / terms of `count` rows)."""
    z = z[:count].double().clone().requires_grad_(True)
    E = E.double().clone().requires_grad_(True)
    bias = bias.double().clone().requires_grad_(True)
    V, D = E.shape
    if count == 0:
        zero = torch.zeros((), dtype=torch.float64)
        return {"loss": zero, "lse": torch.zeros(0, dtype=torch.float64), "terms": torch.zeros(0, dtype=torch.float64), "hits": 0,
                "dz": torch.zeros(0, D, dtype=torch.float64), "dE": torch.zeros(V, D, dtype=torch.float64), "dbias": torch.zeros(V, dtype=torch.float64),
                "logit_max": 0.0}
    y = torch.as_tensor(np.asarray(labels[:count]), dtype=torch.int64)
    logits = z @ E.t() + bias
    lse = torch.logsumexp(logits, dim=1)
    terms = lse - logits.gather(1, y[:, None])[:, 0]
    loss = loss_scale * terms.mean()
    loss.backward()
    hits = int((logits.gather(1, y[:, None])[:, 0] == logits.max(dim=1).values).sum())
    return {"loss": loss.detach(), "lse": lse.detach(), "terms": terms.detach(), "hits": hits, "dz": z.grad, "dE": E.grad, "dbias": bias.grad,
            "logit_max": float(logits.detach().abs().max())}


def rel_l2(got, want):
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    return float((got - want).norm() / want.norm().clamp_min(1e-300))
