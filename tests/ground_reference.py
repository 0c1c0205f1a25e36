"""Plain-torch restatement of phrase grounding for the tests of csrc/ground.hip: the two heat maps, the bilinear upsample
(F.interpolate, align_corners=False) and the record fields.  Every function runs in any floating dtype: float64 is the reference, float32 on
the CPU is the "twin" whose own deviation from float64 sets the tolerance of a kernel output (classify_reference.tolerance).  The features
are handed in already rounded to bf16 and converted exactly, so input rounding is no error source."""
import numpy as np
import torch
import torch.nn.functional as F

from classify_reference import tolerance, ulp32  # noqa: F401  (the project's rule, re-exported for the tests)


def maps_reference(ctx, words, cap_lens, entries, mode="attention", temp1=4.0, eps=1e-8, dtype=torch.float64):
    """h [n, P] of the entries (image b, caption i, word_lo, word_hi) on CPU tensors in `dtype`.  ctx [B, P, D], words [Bc, T, D]."""
    c, w = ctx.detach().cpu().to(dtype), words.detach().cpu().to(dtype)
    out = torch.zeros(len(entries), c.shape[1], dtype=dtype)
    for k, (b, i, lo, hi) in enumerate(np.asarray(entries).reshape(-1, 4).tolist()):
        if mode == "attention":
            s_raw = w[i, : int(cap_lens[i])] @ c[b].t()                       # [len, P]
            s = torch.softmax(s_raw, dim=0)                                   # over the caption's words
            a = torch.softmax(temp1 * s, dim=1)                               # over the regions
            out[k] = a[lo:hi].mean(dim=0)
        else:
            u = w[i, lo:hi].sum(dim=0)
            den = (c[b].norm(dim=1) * u.norm()).clamp(min=eps)
            out[k] = (c[b] @ u) / den
    return out


def upsample_reference(h, size, dtype=torch.float64):
    """hf [n, H, W]: the bilinear upsample of grid maps h [n, g * g]."""
    n, P = h.shape
    g = int(round(P ** 0.5))
    assert g * g == P, P
    if n == 0:
        return torch.zeros(0, int(size[0]), int(size[1]), dtype=dtype)
    return F.interpolate(h.detach().cpu().to(dtype).reshape(n, 1, g, g), size=tuple(int(v) for v in size), mode="bilinear", align_corners=False)[:, 0]


def union_mask(boxes, size):
    """bool numpy [n, H, W]: the union of the half-open rectangles (x0, y0, x1, y1) of every entry, clipped to the frame."""
    H, W = int(size[0]), int(size[1])
    bx = np.asarray(boxes).astype(np.int64)
    out = np.zeros((bx.shape[0], H, W), dtype=bool)
    for k in range(bx.shape[0]):
        for x0, y0, x1, y1 in bx[k].tolist():
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
            if x1 > x0 and y1 > y0:
                out[k, y0:y1, x0:x1] = True
    return out


def records_reference(hf, boxes, thetas, thr=None):
    """The record fields of full-resolution maps hf (numpy [n, H, W], any float dtype) against `boxes`, by numpy: a dict of max, min, y, x, hit,
    area, thr [n, NTH] (computed in hf's dtype unless given), inter / pred [n, NTH] and the float64 sums S_in, Q_in, S_all, Q_all."""
    hf = np.asarray(hf)
    n, H, W = hf.shape
    un = union_mask(boxes, (H, W))
    flat = hf.reshape(n, -1)
    mx, mn = flat.max(axis=1), flat.min(axis=1)
    am = np.array([int(np.flatnonzero(flat[k] == mx[k])[0]) for k in range(n)], dtype=np.int64)
    y, x = am // W, am % W
    if thr is None:
        thr = np.stack([mn + hf.dtype.type(t) * (mx - mn) for t in thetas], axis=1) if len(thetas) else np.zeros((n, 0), dtype=hf.dtype)
    pred = np.stack([(flat >= thr[:, k:k + 1]).sum(axis=1) for k in range(thr.shape[1])], axis=1) if thr.shape[1] else np.zeros((n, 0), dtype=np.int64)
    inter = np.stack([((flat >= thr[:, k:k + 1]) & un.reshape(n, -1)).sum(axis=1) for k in range(thr.shape[1])], axis=1) if thr.shape[1] else np.zeros((n, 0), dtype=np.int64)
    d = flat.astype(np.float64)
    u = un.reshape(n, -1)
    return {"max": mx, "min": mn, "y": y, "x": x, "hit": un[np.arange(n), y, x].astype(np.int64), "area": u.sum(axis=1), "thr": thr, "pred": pred, "inter": inter,
            "S_in": (d * u).sum(axis=1), "Q_in": (d * d * u).sum(axis=1), "S_all": d.sum(axis=1), "Q_all": (d * d).sum(axis=1), "union": un}


def metrics_reference(rec_i, rec_d, size, n_thetas):
    """pg_acc, cnr_mean, iou / dice per threshold by entry loops over records (numpy int [n, 4 + 2 NTH], float64 [n, 4])."""
    HW = int(size[0]) * int(size[1])
    hits, boxed, cnr = 0, 0, []
    iou, dice = [[] for _ in range(n_thetas)], [[] for _ in range(n_thetas)]
    for ri, rd in zip(np.asarray(rec_i).tolist(), np.asarray(rec_d, dtype=np.float64).tolist()):
        area = ri[3]
        if area <= 0:
            continue
        boxed += 1
        hits += ri[2]
        for k in range(n_thetas):
            inter, pred = ri[4 + 2 * k], ri[5 + 2 * k]
            iou[k].append(inter / (pred + area - inter))
            dice[k].append(2.0 * inter / (pred + area))
        if area < HW:
            mu_in, mu_out = rd[0] / area, (rd[2] - rd[0]) / (HW - area)
            var = max(rd[1] / area - mu_in * mu_in, 0.0) + max((rd[3] - rd[1]) / (HW - area) - mu_out * mu_out, 0.0)
            if var > 0.0:
                cnr.append(abs(mu_in - mu_out) / var ** 0.5)
    mean = lambda v: float(np.mean(v)) if len(v) else float("nan")
    return {"pg_acc": hits / boxed if boxed else float("nan"), "cnr_mean": mean(cnr), "iou": [mean(v) for v in iou], "dice": [mean(v) for v in dice],
            "n_entries": len(rec_i), "n_cnr": len(cnr), "n_boxed": boxed}
