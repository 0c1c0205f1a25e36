"""The segmentation head launches (csrc/segment.hip) against the float64 restatement of tests/segment_reference.py.

Tolerance of an output: the project's rule (classify_reference.tolerance) - 8 x the largest absolute deviation a torch fp32 CPU evaluation
of the same formulas shows from the float64 one on the same inputs, at least 4 ulp at the output's largest magnitude.  The bf16 output
dfeat adds 2^-8 |ref| elementwise: one bf16 rounding.  Every case prints the kernel's and the twin's deviation."""
import functools

import pytest
import torch
import torch.nn.functional as F

import segment_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, g, H, W, D, C, options)
CASES = [
    (1, 8, 64, 64, 64, 1, {}),                                                       # one image, integer scale
    (2, 16, 16, 16, 64, 2, {"ignore": "some", "pw": True, "scale": 0.25}),          # scale 1: the upsample is the identity
    (2, 14, 100, 75, 128, 8, {"ignore": "class", "pw": True, "w_dice": 0.0}),       # non-integer scales, non-square, widest head, byte path
    (3, 14, 224, 224, 768, 3, {"ignore": "image", "big": True}),                    # the cfg2 geometry
    (1, 24, 336, 336, 64, 1, {"ignore": "some", "w_bce": 0.0}),                     # the cfg3 grid
    (2, 14, 15, 14, 64, 1, {"big": True, "scale": 0.25}),                           # H barely above g, W = g
    (1, 8, 32, 40, 2048, 8, {"ignore": "some", "pw": True}),                        # the largest head: W fills 64 KiB of LDS, four loads per lane and row
    (1, 8, 64, 64, 64, 1, {"ignore": "all"}),
    (2, 14, 100, 75, 128, 8, {"ignore": "all", "pw": True}),
]
IDS = [f"B{b}-g{g}-{h}x{w}-D{d}-C{c}-" + "+".join(f"{k}={v}" for k, v in o.items()) for b, g, h, w, d, c, o in CASES]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs (CPU) and the float64 / fp32-twin references of case i, computed once and shared."""
    B, g, H, Wm, D, C, o = CASES[i]
    gen = torch.Generator().manual_seed(300 + i)
    feat = torch.randn(B, g * g, D, generator=gen).to(torch.bfloat16)
    # logits of magnitude ~40 ("big") exercise the stable softplus / sigmoid; otherwise of magnitude ~2
    W = torch.randn(C, D, generator=gen) * ((40.0 if o.get("big") else 2.0) / (3.0 * D ** 0.5))
    b = torch.randn(C, generator=gen) * 0.1
    masks = (F.interpolate(torch.randn(B, C, 5, 5, generator=gen), size=(H, Wm), mode="bilinear") > 0.2).to(torch.int8)
    ign = o.get("ignore")
    if ign == "some":
        masks[torch.rand(B, C, H, Wm, generator=gen) < 0.1] = -1
    elif ign == "class":
        masks[:, C // 2] = -1
    elif ign == "image":
        masks[B - 1] = -1
    elif ign == "all":
        masks[:] = -1
    pw = (0.5 + 2.0 * torch.rand(C, generator=gen)) if o.get("pw") else None
    kw = dict(pos_weight=pw, w_bce=o.get("w_bce", 1.0), w_dice=o.get("w_dice", 1.0), eps=1.0, loss_scale=o.get("scale", 1.0))
    ref = R.seg_reference(feat, W, b, masks, dtype=torch.float64, **kw)
    twin = R.seg_reference(feat, W, b, masks, dtype=torch.float32, **kw)
    return feat, W, b, masks, pw, kw, ref, twin


def _run(i):
    from medmoe_amd import ops
    B, g, H, Wm, D, C, _ = CASES[i]
    feat, W, b, masks, pw, kw, _, _ = _case(i)
    x, Wg, bg, mg = feat.to(DEV).reshape(B * g * g, D), W.to(DEV), b.to(DEV), masks.to(DEV)
    pwg = None if pw is None else pw.to(DEV)
    z = ops.seg_head_fwd(x, Wg, bg).reshape(B, g * g, C)
    dz = torch.full_like(z, float("nan"))
    loss, counts = ops.seg_loss(z, mg, pos_weight=pwg, w_bce=kw["w_bce"], w_dice=kw["w_dice"], dice_eps=kw["eps"], loss_scale=kw["loss_scale"], dz=dz)
    dfeat = torch.full((B * g * g, D), float("nan"), device=DEV, dtype=torch.bfloat16)       # must be written, not accumulated into
    dW, db = torch.zeros(C, D, device=DEV), torch.zeros(C, device=DEV)
    ops.seg_head_bwd(dz, x, Wg, dW, db, dfeat=dfeat)
    pred, zf = ops.seg_predict(z, (H, Wm), want_logits=True)
    torch.cuda.synchronize()
    return {"z": z, "loss": loss[0], "dz": dz, "dfeat": dfeat.reshape(B, g * g, D), "dW": dW, "db": db, "counts": counts, "pred": pred, "zf": zf}


def _check(name, got, ref, twin, extra=None):
    got = got.detach().double().cpu()
    tol = R.tolerance(ref, twin)
    err = (got - ref).abs()
    dev = float(err.max()) if ref.numel() else 0.0
    tdev = float((twin.double() - ref).abs().max()) if ref.numel() else 0.0
    print(f"  {name}: kernel dev {dev:.3e}, twin dev {tdev:.3e}, tol {tol:.3e}" + ("" if extra is None else " (+ 2^-8 |ref|)"))
    assert bool(torch.isfinite(got).all()), name
    bound = tol if extra is None else tol + extra
    assert bool((err <= bound).all()), (name, dev, tol)
    return tol


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_parity_counts_and_corners(i):
    B, g, H, Wm, D, C, o = CASES[i]
    _, _, _, masks, _, _, ref, twin = _case(i)
    out = _run(i)
    print(f"case {IDS[i]}")
    for name in ("z", "loss", "dz", "dW", "db"):
        _check(name, out[name], ref[name], twin[name])
    _check("dfeat", out["dfeat"], ref["dfeat"], twin["dfeat"], extra=ref["dfeat"].abs() * 2.0 ** -8)
    tol_zf = _check("zf", out["zf"], ref["zf"], twin["zf"])
    # corners: the border pixels of zf and the corner patches of dz on their own - an off-by-one in a support range shows there
    zf, dz = out["zf"].double().cpu(), out["dz"].double().cpu().reshape(B, g, g, C)
    rdz, tol_dz = ref["dz"].reshape(B, g, g, C), R.tolerance(ref["dz"], twin["dz"])
    for sl in ((..., 0, slice(None)), (..., H - 1, slice(None)), (..., slice(None), 0), (..., slice(None), Wm - 1)):
        assert float((zf[sl] - ref["zf"][sl]).abs().max()) <= tol_zf
    for ci, cj in ((0, 0), (0, g - 1), (g - 1, 0), (g - 1, g - 1)):
        assert float((dz[:, ci, cj] - rdz[:, ci, cj]).abs().max()) <= tol_dz
    for sl in ((slice(None), 0), (slice(None), g - 1), (slice(None), slice(None), 0), (slice(None), slice(None), g - 1)):
        assert float((dz[sl] - rdz[sl]).abs().max()) <= tol_dz
    # exact counts: n_valid (and |K|, their sum) against the masks; TP / FP / FN against the kernel's own predicted masks
    counts, pred = out["counts"].cpu(), out["pred"].cpu().bool()
    valid, pos = masks >= 0, masks > 0
    assert counts[:, 0].tolist() == valid.sum(dim=(0, 2, 3)).tolist() and int(counts[:, 0].sum()) == int(valid.sum())
    assert bool((pred == (out["zf"].cpu() > 0)).all())
    own = torch.stack([(valid & pos & pred).sum(dim=(0, 2, 3)), (valid & ~pos & pred).sum(dim=(0, 2, 3)), (valid & pos & ~pred).sum(dim=(0, 2, 3))], dim=1)
    assert counts[:, 1:].tolist() == own.tolist()
    # ... and against float64 on the safe pixels, those whose reference logit is further from 0 than the tolerance of zf
    safe = ref["zf"].abs() > tol_zf
    unsafe = 1.0 - float(safe.double().mean())
    print(f"  unsafe pixels: {unsafe:.3e}")
    assert unsafe <= 1e-3, "the case is invalid: too many logits at the threshold"
    assert R.counts_where(out["zf"].double().cpu(), masks.long(), safe).tolist() == R.counts_where(ref["zf"], masks.long(), safe).tolist()
    if o.get("ignore") == "all":
        assert float(out["loss"]) == 0.0 and int(counts.sum()) == 0
        for name in ("dz", "dfeat", "dW", "db"):
            assert bool((out[name] == 0).all()), name


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_two_runs_are_bit_identical_and_no_nondeterministic_launch_is_counted(i):
    from medmoe_amd import ops
    before = ops.nondet_launches()
    a, b = _run(i), _run(i)
    assert ops.nondet_launches() == before
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_scale_one_is_the_identity_and_masks_follow_the_sign():
    """H = W = g: zf is z itself, bit for bit, and the predicted mask is its sign; without want_logits the same masks."""
    from medmoe_amd import ops
    out = _run(1)
    B, g, H, Wm, D, C, _ = CASES[1]
    z = out["z"].reshape(B, g, g, C).permute(0, 3, 1, 2)
    assert torch.equal(out["zf"], z.contiguous()) and torch.equal(out["pred"].bool(), z > 0)
    assert torch.equal(ops.seg_predict(out["z"], (H, Wm)), out["pred"])


def test_library_refuses_a_mask_smaller_than_the_grid():
    """MM_ERR_SHAPE from the library itself (the wrapper's own check bypassed)."""
    from medmoe_amd import ops
    z = torch.zeros(1, 64, 1, device=DEV)
    m = torch.zeros(1, 1, 7, 8, dtype=torch.int8, device=DEV)
    loss, counts, sc = torch.zeros(1, device=DEV), torch.zeros(1, 4, dtype=torch.int64, device=DEV), torch.zeros(4096, device=DEV)
    with pytest.raises(RuntimeError, match="seg_loss failed with code -2"):
        ops.call("seg_loss", z, m, None, 1.0, 1.0, 1.0, 1.0, None, loss, counts, sc, sc.numel(), 1, 8, 7, 8, 1)
    assert ops.seg_scratch(1, 8, 7, 8, 64, 1) == 0
