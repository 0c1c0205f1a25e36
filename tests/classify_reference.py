"""Plain-torch restatement of the classification head, its loss and gradients, and of the AUROC pair counts, for the tests of
csrc/classify.hip.  `head_reference` runs in any floating dtype: float64 is the reference, float32 on the CPU is the "twin" whose own
deviation from float64 sets the tolerance of a kernel output (`tolerance`)."""
import math

import numpy as np
import torch


def head_reference(x, W, b, targets, task, label_smoothing=0.0, pos_weight=None, loss_scale=1.0, dtype=torch.float64):
    """z, loss, dz, dx, dW, db, n_valid (and, multiclass, pred = argmax z with ties to the lowest class) of the head on CPU tensors in `dtype`.
    multiclass: targets int [N], -1 = not counted; multilabel: targets int [N, C] in {0, 1, -1}."""
    x, W, b = x.detach().cpu().to(dtype), W.detach().cpu().to(dtype), b.detach().cpu().to(dtype)
    t = targets.detach().cpu().long()
    N, C = x.shape[0], W.shape[0]
    z = x @ W.t() + b
    out = {"z": z}
    if task == "multiclass":
        valid = t >= 0
        n = int(valid.sum())
        scale = loss_scale / n if n else 0.0
        logp = z - torch.logsumexp(z, dim=1, keepdim=True)
        q = torch.zeros(N, C, dtype=dtype)
        q[valid, t[valid]] = 1.0
        q = (1.0 - label_smoothing) * q + label_smoothing / C
        rows = -(q * logp).sum(dim=1)
        loss = scale * rows[valid].sum()
        dz = scale * (torch.softmax(z, dim=1) - q) * valid.reshape(N, 1).to(dtype)
        out["pred"] = (z == z.max(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)
    else:
        valid = t >= 0
        n = int(valid.sum())
        scale = loss_scale / n if n else 0.0
        tf = t.clamp(min=0).to(dtype)
        pw = torch.ones(C, dtype=dtype) if pos_weight is None else pos_weight.detach().cpu().to(dtype)
        l1p = torch.log1p(torch.exp(-z.abs()))
        sp, sn = z.clamp(min=0) + l1p, (-z).clamp(min=0) + l1p                   # softplus(z), softplus(-z)
        ell = pw * tf * sn + (1.0 - tf) * sp
        loss = scale * ell[valid].sum()
        dz = scale * ((1.0 - tf) * torch.sigmoid(z) - pw * tf * torch.sigmoid(-z)) * valid.to(dtype)
    out.update(loss=loss.reshape(()), dz=dz, dx=dz @ W, dW=dz.t() @ x, db=dz.sum(dim=0), n_valid=n)
    return out


def ulp32(magnitude: float) -> float:
    """The spacing of fp32 numbers at `magnitude`."""
    if magnitude == 0.0:
        return 0.0
    return 2.0 ** (max(math.floor(math.log2(magnitude)), -126) - 23)


def tolerance(ref64: torch.Tensor, twin32: torch.Tensor) -> float:
    """8 x the largest absolute deviation of the fp32 CPU evaluation from the float64 one, at least 4 ulp (fp32) at the output's largest
    magnitude.  The factor 8 covers the different summation order and a few ulp of exp / log."""
    dev = float((twin32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    return max(8.0 * dev, 4.0 * ulp32(float(ref64.abs().max()) if ref64.numel() else 0.0))


def auroc_counts_reference(scores: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """int64 [C, 4] = (n_pos, n_neg, n_less, n_equal) by brute force over all (positive, negative) pairs."""
    N, C = scores.shape
    out = np.zeros((C, 4), dtype=np.int64)
    for c in range(C):
        pos, neg = scores[targets[:, c] == 1, c], scores[targets[:, c] == 0, c]
        out[c, 0], out[c, 1] = pos.size, neg.size
        if pos.size and neg.size:
            out[c, 2] = int((neg[None, :] < pos[:, None]).sum())
            out[c, 3] = int((neg[None, :] == pos[:, None]).sum())
    return out


def auroc_reference(scores: np.ndarray, targets: np.ndarray):
    """(per_class float64 [C] with NaN for a one-sided class, mean over the other classes) from the brute-force counts."""
    c = auroc_counts_reference(scores, targets).astype(np.float64)
    pairs = c[:, 0] * c[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.where(pairs > 0, (c[:, 2] + 0.5 * c[:, 3]) / pairs, np.nan)
    ok = pairs > 0
    return per, (float(per[ok].mean()) if ok.any() else float("nan"))
