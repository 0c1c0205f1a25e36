"""The two grounding launches (csrc/ground.hip) against the float64 restatement of tests/ground_reference.py.

Tolerance of a floating output: the project's rule (classify_reference.tolerance) - 8 x the largest absolute deviation a torch fp32 CPU
evaluation of the same formulas shows from the float64 one on the same inputs, at least 4 ulp at the output's largest magnitude.  The sums
of the attention maps are an output like any other: the same rule on the sums (their magnitude is 1).  Every case prints the kernel's and
the twin's deviation.  The records are exact against the kernel's own full-resolution map: integers and comparisons only; the fp64 sums
within the order-of-summation bound H W 2^-52 sum |x|."""
import functools

import numpy as np
import pytest
import torch

import ground_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (g, D, T, caption lengths, score scale): lengths on both sides of every multiple of 16 the geometry reaches, 1 and T among them
GEOMS = [
    (8, 64, 16, [1, 15, 16, 7], 3.0),
    (14, 128, 80, [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80], 3.0),
    (14, 768, 77, [1, 16, 17, 32, 33, 48, 49, 64, 65, 77], 3.0),
    (16, 64, 33, [1, 15, 16, 17, 31, 32, 33], 3.0),
    (24, 64, 48, [1, 16, 17, 32, 33, 47, 48], 3.0),
    (8, 64, 16, [1, 15, 16, 7], 30.0),                                   # the word softmax saturates
]
MODES = ("attention", "cosine")
IDS = [f"g{g}-D{d}-T{t}-x{s:g}" for g, d, t, _, s in GEOMS]
B_IMG = 3


@functools.lru_cache(maxsize=None)
def _inputs(gi):
    g, D, T, lens, scale = GEOMS[gi]
    gen = torch.Generator().manual_seed(500 + gi)
    ctx = torch.randn(B_IMG, g * g, D, generator=gen).to(torch.bfloat16)
    words = (torch.randn(len(lens), T, D, generator=gen) * (scale / D ** 0.5)).to(torch.bfloat16)
    ent = []
    for i, n in enumerate(lens):
        ent.append((i % B_IMG, i, 0, n))                                 # the whole caption (a matched pair where i < B)
        ent.append(((i + 1) % B_IMG, i, n - 1, n))                       # one word, ending at the last word; a non-matched pair
        lo = int(torch.randint(0, n, (1,), generator=gen))
        hi = int(torch.randint(lo + 1, n + 1, (1,), generator=gen))
        ent.append((0, i, lo, hi))                                       # many entries on image 0
        ent.append((i % B_IMG, i, 0, 1))                                 # the first word: several entries on one caption
    return ctx, words, torch.tensor(lens, dtype=torch.int32), np.asarray(ent, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _refs(gi, mode):
    """float64 reference and fp32 twin of case (gi, mode), computed once and shared."""
    ctx, words, lens, ent = _inputs(gi)
    return (R.maps_reference(ctx, words, lens.tolist(), ent, mode, dtype=torch.float64),
            R.maps_reference(ctx, words, lens.tolist(), ent, mode, dtype=torch.float32))


def _maps(gi, mode):
    from medmoe_amd import ops
    ctx, words, lens, ent = _inputs(gi)
    return ops.ground_maps(ctx.to(DEV), words.to(DEV), lens.to(DEV), ent, mode=mode, cap_lens_host=lens)


def _check(name, got, ref, twin):
    got = got.detach().double().cpu()
    tol = R.tolerance(ref, twin)
    dev = float((got - ref).abs().max()) if ref.numel() else 0.0
    tdev = float((twin.double() - ref).abs().max()) if ref.numel() else 0.0
    print(f"  {name}: kernel dev {dev:.3e}, twin dev {tdev:.3e}, tol {tol:.3e}")
    assert bool(torch.isfinite(got).all()), name
    assert dev <= tol, (name, dev, tol)
    return tol


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=IDS)
def test_maps_against_float64(gi, mode):
    ref, twin = _refs(gi, mode)
    h = _maps(gi, mode)
    torch.cuda.synchronize()
    print(f"case {IDS[gi]} {mode}: {ref.shape[0]} entries")
    assert tuple(h.shape) == tuple(ref.shape) and h.dtype == torch.float32
    _check("h", h, ref, twin)
    if mode == "attention":
        _check("sum h", h.double().sum(dim=1), ref.sum(dim=1), twin.double().sum(dim=1).float())
        assert float((ref.sum(dim=1) - 1.0).abs().max()) < 1e-12
    else:
        assert float(ref.abs().max()) <= 1.0 + 1e-12


def test_empty_list_launches_nothing_and_only_the_listed_slots_are_written():
    from medmoe_amd import ops
    ctx, words, lens, ent = _inputs(0)
    c, w, l = ctx.to(DEV), words.to(DEV), lens.to(DEV)
    before = ops.nondet_launches()
    h0 = ops.ground_maps(c, w, l, np.zeros((0, 4), dtype=np.int64))
    assert tuple(h0.shape) == (0, 64)
    B, P, D = ctx.shape
    n = ent.shape[0]
    buf = torch.full((n + 2, P), float("nan"), device=DEV)
    ent_d = torch.from_numpy(ent.astype(np.int32)).to(DEV)
    ops.call("ground_maps", c, w, l, ent_d, buf, 0, B, words.shape[0], P, words.shape[1], D, 0, 4.0, 1e-8)       # n = 0: returns before a launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    ops.call("ground_maps", None, None, None, None, None, 0, B, words.shape[0], P, words.shape[1], D, 0, 4.0, 1e-8)
    ops.call("ground_maps", c, w, l, ent_d, buf, n - 1, B, words.shape[0], P, words.shape[1], D, 0, 4.0, 1e-8)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf[:n - 1]).all()) and bool(torch.isnan(buf[n - 1:]).all())
    assert torch.equal(buf[:n - 1], _maps(0, "attention")[:n - 1])
    assert ops.nondet_launches() == before
    # the library's own refusals (the wrapper's checks bypassed): a shape it has no kernel for, a temperature past 64
    with pytest.raises(RuntimeError, match="ground_maps failed with code -2"):
        ops.call("ground_maps", c, w, l, ent_d, buf, n, B, words.shape[0], P, 81, D, 0, 4.0, 1e-8)
    with pytest.raises(RuntimeError, match="ground_maps failed with code -2"):
        ops.call("ground_maps", c, w, l, ent_d, buf, n, B, words.shape[0], 63, words.shape[1], D, 0, 4.0, 1e-8)
    with pytest.raises(RuntimeError, match="ground_maps failed with code -1"):
        ops.call("ground_maps", c, w, l, ent_d, buf, n, B, words.shape[0], P, words.shape[1], D, 0, 65.0, 1e-8)
    with pytest.raises(RuntimeError, match="ground_score failed with code -2"):
        ops.call("ground_score", buf, ent_d, None, None, buf, ent_d, buf, 1, 8, 7, 8, 1, 0)


# (geometry, mode, (H, W)): scale 1, an integer scale, non-integer and non-square, H = g + 1
UPSAMPLE = [(0, "attention", (8, 8)), (0, "cosine", (32, 32)), (1, "attention", (100, 75)), (1, "cosine", (15, 14)), (3, "cosine", (16, 16)),
            (4, "attention", (25, 50))]


@pytest.mark.parametrize("gi,mode,size", UPSAMPLE, ids=[f"{IDS[g]}-{m}-{s[0]}x{s[1]}" for g, m, s in UPSAMPLE])
def test_full_resolution_map_against_float64(gi, mode, size):
    from medmoe_amd import ops
    ref, twin = _refs(gi, mode)
    n = ref.shape[0]
    rf, tw = R.upsample_reference(ref, size, torch.float64), R.upsample_reference(twin, size, torch.float32)
    h = _maps(gi, mode)
    out = ops.ground_score(h, torch.zeros(n, 1, 4, dtype=torch.int32), size, want_map=True)
    torch.cuda.synchronize()
    hf = out["hf"]
    assert tuple(hf.shape) == (n, size[0], size[1])
    print(f"case {IDS[gi]} {mode} -> {size}")
    tol = _check("hf", hf, rf, tw)
    got = hf.double().cpu()
    for sl in ((slice(None), 0), (slice(None), size[0] - 1), (slice(None), slice(None), 0), (slice(None), slice(None), size[1] - 1)):
        assert float((got[sl] - rf[sl]).abs().max()) <= tol
    if tuple(size) == (GEOMS[gi][0],) * 2:                             # scale 1: the identity, bit for bit
        assert torch.equal(hf.reshape(n, -1), h)


def _score_cases():
    """(name, h [n, g*g], boxes [n, NB, 4], size, thetas): hand-made grids passed straight to ground_score."""
    gen = torch.Generator().manual_seed(77)
    cases = []
    # random grids, boxes of every kind: none, the frame, overlapping, one-pixel corners, past the frame (clipped), empty rectangles
    for g, (H, W), th in ((8, (32, 40), (0.25, 0.5, 0.75, 1.0)), (14, (100, 75), (0.5,)), (3, (4, 3), ()), (32, (33, 47), (0.0, 0.5))):
        n = 6
        h = torch.randn(n, g * g, generator=gen)
        bx = torch.zeros(n, 4, 4, dtype=torch.int32)
        bx[1, 0] = torch.tensor([0, 0, W, H])
        bx[2, 0] = torch.tensor([1, 1, W // 2 + 1, H // 2 + 1])
        bx[2, 1] = torch.tensor([W // 4, H // 4, W - 1, H - 1])
        bx[2, 3] = torch.tensor([W // 4, H // 4, W // 2, H // 2])
        bx[3] = torch.tensor([[0, 0, 1, 1], [W - 1, 0, W, 1], [0, H - 1, 1, H], [W - 1, H - 1, W, H]])
        bx[4, 1] = torch.tensor([-5, -5, W + 9, 2])
        bx[4, 2] = torch.tensor([2, 1, 2, H])
        bx[5, 0] = torch.tensor([W // 3, 0, W // 3 + 1, H])
        cases.append((f"random-g{g}", h, bx, (H, W), th))
    g, H, W = 4, 16, 16
    h = torch.zeros(5, g * g)
    h[0, 5] = h[0, 10] = 2.0                                             # two equal maximal patches: the first in row-major order wins
    h[1, 0] = 3.0                                                        # the top-left corner patch: its clamped border is a plateau
    h[2, :] = 0.375                                                      # a constant grid: max == min
    h[3, g * g - 1] = 1.0                                                # the bottom-right corner patch
    h[4] = -torch.arange(g * g, dtype=torch.float32)                     # all negative, maximum first
    bx = torch.zeros(5, 2, 4, dtype=torch.int32)
    bx[0, 0] = torch.tensor([4, 4, 8, 8])
    bx[1, 0] = torch.tensor([0, 0, 1, 1])
    bx[2, 1] = torch.tensor([3, 2, 9, 7])
    bx[3, 0] = torch.tensor([0, 0, 12, 12])
    bx[4, 0] = torch.tensor([0, 0, 16, 16])
    cases.append(("hand-made", h, bx, (H, W), (0.5, 1.0)))
    return cases


SCORE_CASES = _score_cases()


@pytest.mark.parametrize("ci", range(len(SCORE_CASES)), ids=[c[0] for c in SCORE_CASES])
def test_records_are_exact_against_the_kernels_own_map(ci):
    from medmoe_amd import ops
    name, h, bx, (H, W), th = SCORE_CASES[ci]
    n, nth = h.shape[0], len(th)
    out = ops.ground_score(h.to(DEV), bx, (H, W), thetas=th, want_map=True)
    torch.cuda.synchronize()
    hf = out["hf"].cpu().numpy()
    rec_f, rec_i, rec_d = out["rec_f"].cpu().numpy(), out["rec_i"].cpu().numpy().astype(np.int64), out["rec_d"].cpu().numpy()
    assert rec_f.shape == (n, 2 + nth) and rec_i.shape == (n, 4 + 2 * nth) and rec_d.shape == (n, 4)
    want = R.records_reference(hf, bx.numpy(), th, thr=rec_f[:, 2:])      # the counts at the STORED thresholds
    assert np.array_equal(rec_f[:, 0], want["max"]) and np.array_equal(rec_f[:, 1], want["min"])
    assert rec_i[:, 0].tolist() == want["y"].tolist() and rec_i[:, 1].tolist() == want["x"].tolist()
    assert rec_i[:, 2].tolist() == want["hit"].tolist() and rec_i[:, 3].tolist() == want["area"].tolist()
    for k in range(nth):
        assert rec_i[:, 4 + 2 * k].tolist() == want["inter"][:, k].tolist() and rec_i[:, 5 + 2 * k].tolist() == want["pred"][:, k].tolist()
        exact = want["min"].astype(np.float64) + float(np.float32(th[k])) * (want["max"].astype(np.float64) - want["min"].astype(np.float64))
        for e in range(n):
            ulp = R.ulp32(max(abs(float(want["max"][e])), abs(float(want["min"][e]))))
            assert abs(float(rec_f[e, 2 + k]) - exact[e]) <= 4.0 * ulp, (e, k)
    d = hf.reshape(n, -1).astype(np.float64)
    bound1, bound2 = H * W * 2.0 ** -52 * np.abs(d).sum(axis=1), H * W * 2.0 ** -52 * (d * d).sum(axis=1)
    for col, key, bound in ((0, "S_in", bound1), (1, "Q_in", bound2), (2, "S_all", bound1), (3, "Q_all", bound2)):
        err = np.abs(rec_d[:, col] - want[key])
        print(f"  {key}: max error {err.max():.3e}, bound {bound.min():.3e} ..")
        assert (err <= bound).all(), key
    if name == "hand-made":
        # patches (1, 1) and (2, 2): the pixels (6, 6) and (9, 9) between their centres read both and tie, bit for bit (dyadic weights)
        assert hf[0, 6, 6] == hf[0, 9, 9] == np.float32(1.5625) and rec_i[0, :3].tolist() == [6, 6, 1] and float(rec_f[0, 0]) == 1.5625
        assert rec_i[1, :3].tolist() == [0, 0, 1] and (hf[1, :2, :2] == 3.0).all()                           # the plateau: pixel (0, 0) wins
        assert rec_f[2, 0] == rec_f[2, 1] == np.float32(0.375) and (rec_f[2, 2:] == rec_f[2, 0]).all()
        assert rec_i[2, 5] == rec_i[2, 7] == H * W and rec_i[2, 4] == rec_i[2, 3] == 30 and rec_i[2, :3].tolist() == [0, 0, 0]
        assert rec_i[3, 2] == 0 and rec_i[3, :2].tolist() == [14, 14]
        assert rec_i[4, :4].tolist() == [0, 0, 1, H * W]
        # the host side on these records: the constant map has no contrast and the frame-filling box no outside, both are left out
        from medmoe_amd.ground import GroundBank, grounding_metrics
        bank = GroundBank((0.5, 1.0), DEV)
        bank.add(out)
        met, ref = grounding_metrics(bank), R.metrics_reference(rec_i, rec_d, (H, W), 2)
        assert met["n_entries"] == 5 and ref["n_cnr"] == 3 and int(bank.ints[3]) == 3
        assert abs(met["pg_acc"] - ref["pg_acc"]) < 1e-15 and abs(met["cnr_mean"] - ref["cnr_mean"]) <= 1e-12 * ref["cnr_mean"]
        assert abs(met["iou@0.5"] - ref["iou"][0]) < 1e-15 and abs(met["dice@1"] - ref["dice"][1]) < 1e-15
    if name == "random-g8":
        assert rec_i[0, 2:4].tolist() == [0, 0] and rec_i[1, 2:4].tolist() == [1, H * W] and rec_i[3, 3] == 4 and rec_i[4, 3] == 2 * W
        assert rec_i[2, 3] < (W // 2) * (H // 2) + (W - 1 - W // 4) * (H - 1 - H // 4)                      # overlapping: the union is no sum


def _planted(mode_seed=0):
    """Random regions; the regions under each entry's box are aligned with the span's word vectors.  Strength 6: checked on the CPU when
    this test was written - the float64 reference alone hits on every entry in both modes."""
    g, D, T, px = 14, 64, 16, 4
    gen = torch.Generator().manual_seed(900 + mode_seed)
    n = 8
    lens = [int(v) for v in torch.randint(4, T + 1, (n,), generator=gen)]
    words = torch.randn(n, T, D, generator=gen) * (3.0 / D ** 0.5)
    ctx = 0.25 * torch.randn(n, g * g, D, generator=gen)             # raw scores of about 0.75 outside the boxes: no word owns a random region
    ent, boxes = [], torch.zeros(n, 1, 4, dtype=torch.int32)
    for i in range(n):
        lo = int(torch.randint(0, lens[i], (1,), generator=gen))
        hi = min(lens[i], lo + 1 + (i % 3))
        r0, c0 = int(torch.randint(0, g - 4, (1,), generator=gen)), int(torch.randint(0, g - 4, (1,), generator=gen))
        r1, c1 = r0 + 3 + (i % 2), c0 + 2 + (i % 3)
        u = words[i, lo:hi].sum(dim=0)
        sel = torch.zeros(g, g, dtype=torch.bool)
        sel[r0:r1, c0:c1] = True
        ctx[i, sel.reshape(-1)] += 6.0 * D ** 0.5 * u / u.norm() / 3.0
        ent.append((i, i, lo, hi))
        boxes[i, 0] = torch.tensor([c0 * px, r0 * px, c1 * px, r1 * px])
    return ctx.to(torch.bfloat16), words.to(torch.bfloat16), torch.tensor(lens, dtype=torch.int32), np.asarray(ent), boxes, (g * px, g * px)


@pytest.mark.parametrize("mode", MODES)
def test_planted_signal_is_hit_by_the_reference_and_by_the_kernel(mode):
    from medmoe_amd import ops
    ctx, words, lens, ent, boxes, size = _planted()
    ref = R.records_reference(R.upsample_reference(R.maps_reference(ctx, words, lens.tolist(), ent, mode), size).numpy(), boxes.numpy(), ())
    assert ref["hit"].tolist() == [1] * len(ent), ref["hit"]
    h = ops.ground_maps(ctx.to(DEV), words.to(DEV), lens.to(DEV), ent, mode=mode)
    out = ops.ground_score(h, boxes, size, thetas=(0.5,))
    assert out["rec_i"][:, 2].tolist() == [1] * len(ent)
    assert out["rec_i"][:, 3].tolist() == ref["area"].tolist()


def test_two_launches_give_the_same_bits():
    from medmoe_amd import ops
    before = ops.nondet_launches()
    for gi in (1, 4):
        for mode in MODES:
            a, b = _maps(gi, mode), _maps(gi, mode)
            assert torch.equal(a, b), (gi, mode)
    _, h, bx, size, th = SCORE_CASES[1]
    a, b = ops.ground_score(h.to(DEV), bx, size, thetas=th, want_map=True), ops.ground_score(h.to(DEV), bx, size, thetas=th, want_map=True)
    for k in ("rec_f", "rec_i", "rec_d", "hf"):
        assert torch.equal(a[k], b[k]), k
    c = ops.ground_score(h.to(DEV), bx, size, thetas=th)                 # without the stored map: the same records
    assert "hf" not in c and all(torch.equal(a[k], c[k]) for k in ("rec_f", "rec_i", "rec_d"))
    assert ops.nondet_launches() == before
