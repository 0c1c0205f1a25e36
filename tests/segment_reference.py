"""Plain-torch restatement of the segmentation head for the tests of csrc/segment.hip: linear -> F.interpolate(bilinear,
align_corners=False) -> BCE + batch Dice, gradients by autograd.  `seg_reference` runs in any floating dtype: float64 is the reference,
float32 on the CPU is the "twin" whose own deviation from float64 sets the tolerance of a kernel output (classify_reference.tolerance).
The features are handed in already rounded to bf16, so input rounding is no error source."""
import torch
import torch.nn.functional as F

from classify_reference import tolerance  # noqa: F401  (the project's rule, re-exported for the tests)


def _grid(P):
    g = int(round(P ** 0.5))
    assert g * g == P, P
    return g


def loss_of_zf(zf, masks, pos_weight=None, w_bce=1.0, w_dice=1.0, eps=1.0, loss_scale=1.0):
    """L = s (w_bce L_bce + w_dice L_dice) of full-resolution logits zf [B, C, H, W] against masks in {0, 1, -1}; 0 when nothing is valid."""
    dt = zf.dtype
    C = zf.shape[1]
    valid = masks >= 0
    v, t = valid.to(dt), (masks > 0).to(dt)
    K = int(valid.sum())
    if K == 0:
        return zf.sum() * 0.0
    pw = torch.ones(C, dtype=dt) if pos_weight is None else pos_weight.detach().cpu().to(dt)
    ell = pw.reshape(1, C, 1, 1) * t * -F.logsigmoid(zf) + (1.0 - t) * -F.logsigmoid(-zf)           # softplus(-z), softplus(z)
    l_bce = (ell * v).sum() / K
    p = torch.sigmoid(zf)
    I, Pm, T = (p * t * v).sum(dim=(0, 2, 3)), (p * v).sum(dim=(0, 2, 3)), (t * v).sum(dim=(0, 2, 3))
    cv = valid.sum(dim=(0, 2, 3)) > 0
    l_dice = 1.0 - ((2.0 * I + eps) / (Pm + T + eps))[cv].mean()
    return loss_scale * (w_bce * l_bce + w_dice * l_dice)


def dzf_formula(zf, masks, pos_weight=None, w_bce=1.0, w_dice=1.0, eps=1.0, loss_scale=1.0):
    """d L / d zf written out by hand, as the gradient pass forms it: the BCE term / |K| and the Dice term
    -(1 / C_v) (2 t (P + T + eps) - (2 I + eps)) / (P + T + eps)^2 p (1 - p)."""
    dt = zf.dtype
    C = zf.shape[1]
    valid = masks >= 0
    v, t = valid.to(dt), (masks > 0).to(dt)
    K = int(valid.sum())
    if K == 0:
        return torch.zeros_like(zf)
    pw = (torch.ones(C, dtype=dt) if pos_weight is None else pos_weight.detach().cpu().to(dt)).reshape(1, C, 1, 1)
    p = torch.sigmoid(zf)
    I, Pm, T = (p * t * v).sum(dim=(0, 2, 3)), (p * v).sum(dim=(0, 2, 3)), (t * v).sum(dim=(0, 2, 3))
    cv = int((valid.sum(dim=(0, 2, 3)) > 0).sum())
    U = (Pm + T + eps).reshape(1, C, 1, 1)
    bce = ((1.0 - t) * p - pw * t * (1.0 - p)) / K
    dice = -(1.0 / cv) * (2.0 * t * U - (2.0 * I.reshape(1, C, 1, 1) + eps)) / (U * U) * p * (1.0 - p)
    return loss_scale * (w_bce * bce + w_dice * dice) * v


def seg_reference(feat, W, b, masks, pos_weight=None, w_bce=1.0, w_dice=1.0, eps=1.0, loss_scale=1.0, dtype=torch.float64):
    """z [B, P, C], zf [B, C, H, W], loss, dzf, dz, dfeat, dW, db and the integer counts [C, 4] = (n_valid, TP, FP, FN) at zf > 0 of the head on
    CPU tensors in `dtype`.  feat [B, P, D] (bf16 values), masks int [B, C, H, W] in {0, 1, -1}."""
    x = feat.detach().cpu().to(dtype).requires_grad_(True)
    Wd, bd = W.detach().cpu().to(dtype).requires_grad_(True), b.detach().cpu().to(dtype).requires_grad_(True)
    m = masks.detach().cpu().long()
    B, P, _ = x.shape
    C, g = Wd.shape[0], _grid(P)
    H, Wm = m.shape[2], m.shape[3]
    z = x @ Wd.t() + bd
    z.retain_grad()
    zf = F.interpolate(z.reshape(B, g, g, C).permute(0, 3, 1, 2), size=(H, Wm), mode="bilinear", align_corners=False)
    zf.retain_grad()
    loss = loss_of_zf(zf, m, pos_weight, w_bce, w_dice, eps, loss_scale)
    loss.backward()
    valid, pos, pred = m >= 0, m > 0, zf.detach() > 0
    counts = torch.stack([valid.sum(dim=(0, 2, 3)), (valid & pos & pred).sum(dim=(0, 2, 3)), (valid & ~pos & pred).sum(dim=(0, 2, 3)),
                          (valid & pos & ~pred).sum(dim=(0, 2, 3))], dim=1)
    zero = lambda t, like: torch.zeros_like(like) if t is None else t
    return {"z": z.detach(), "zf": zf.detach(), "loss": loss.detach().reshape(()), "dzf": zero(zf.grad, zf.detach()), "dz": zero(z.grad, z.detach()),
            "dfeat": zero(x.grad, x.detach()), "dW": zero(Wd.grad, Wd.detach()), "db": zero(bd.grad, bd.detach()), "counts": counts}


def counts_where(zf, masks, safe):
    """[C, 4] = (n_valid, TP, FP, FN) at zf > 0 over the pixels where `safe` holds."""
    valid, pos, pred = (masks >= 0) & safe, masks > 0, zf > 0
    return torch.stack([valid.sum(dim=(0, 2, 3)), (valid & pos & pred).sum(dim=(0, 2, 3)), (valid & ~pos & pred).sum(dim=(0, 2, 3)),
                        (valid & pos & ~pred).sum(dim=(0, 2, 3))], dim=1)
