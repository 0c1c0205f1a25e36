"""On-device training augmentation (csrc/augment.hip medmoe_augment_params / medmoe_augment_apply, medmoe_amd/data.py).

The reference of this file is written here from the definitions of DESIGN 3m, in float64 (`ref_apply`, `matrix64`, `host_draws`): the crop,
the flip, the nearest-neighbour affine gather about the crop's centre, brightness / contrast in pixel space with the gray mean, the
normalisation.  Where the device computes in fp32 without jitter (one fma, one division) the reference rounds its float64 values to fp32 at
the same two points - both roundings are exact images of the fp32 operations - so those comparisons are bit for bit.

1. identity parameters give the bits of preprocess_images_bicubic, the centre crop its slice;
2. hand-made parameters (crop corners, flip, a quarter turn with a shift, zoom by 2) on a non-square source: every pixel bit-equal;
3. general affine matrices: every pixel outside a 1e-3 band round the rounding ties bit-equal, the band at most 2 % of the pixels; the
   convention itself against torch's affine_grid + grid_sample on the CPU;
4. jitter against float64 at |got - ref| <= 2^-8 |ref| + 1e-5 per element, both orders, fill pixels in the gray mean;
5. the draws against a host Philox: integers and bits exactly, floats to two fp32 roundings, the matrix from the raw draws, statistics;
6. the datamodule: different batches, resume, validation = centre crop, nothing order-dependent, the error codes."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_text_dropout_host import philox4x32_10

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SITE_AUGMENT = 0x20000000
REC = 16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ------------------------------------------------------------------------------------------------------------------------------
def matrix64(angle, tx, ty, s, C):
    """the six numbers of DESIGN 3m: u = (cos (x - c - tx) + sin (y - c - ty)) / s + c, v = (-sin (x - c - tx) + cos (y - c - ty)) / s + c"""
    c, th = (C - 1) / 2.0, math.radians(angle)
    cs, sn = math.cos(th), math.sin(th)
    return [cs / s, sn / s, c - (cs * (c + tx) + sn * (c + ty)) / s, -sn / s, cs / s, c - (-sn * (c + tx) + cs * (c + ty)) / s]


def record(m=(1, 0, 0, 0, 1, 0), fb=1.0, fc=1.0, order=0, flip=0, x0=0, y0=0, raw=(0, 0, 0, 1)):
    return [*m, fb, fc, order, flip, *raw, x0, y0]


def coords64(p, C):
    """u, v [C(y), C(x)] in float64 FROM THE fp32 RECORD p"""
    m = p[:6].astype(np.float64)
    y, x = np.meshgrid(np.arange(C, dtype=np.float64), np.arange(C, dtype=np.float64), indexing="ij")
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


def tie_band(u, v, eps=1e-3):
    """pixels whose u or v lies within eps of a half-integer: the tie of rint and the -0.5 / C - 0.5 edges"""
    d = lambda t: np.abs((t - 0.5) - np.rint(t - 0.5))
    return (d(u) < eps) | (d(v) < eps)


def gather64(u8, p, C):
    """(bytes [C, C, 3] uint8, inside [C, C] bool, band [C, C] bool) of one sample: crop at (x0, y0), flip, rint(u), rint(v)"""
    Hs, Ws = u8.shape[:2]
    u, v = coords64(p, C)
    ix, iy = np.rint(u), np.rint(v)                                       # half to even
    inside = (ix >= 0) & (ix <= C - 1) & (iy >= 0) & (iy <= C - 1)
    ix, iy = np.where(inside, ix, 0).astype(np.int64), np.where(inside, iy, 0).astype(np.int64)
    if p[9] != 0:
        ix = C - 1 - ix
    x0 = int(min(max(float(p[14]), 0.0), Ws - C))
    y0 = int(min(max(float(p[15]), 0.0), Hs - C))
    return u8[y0 + iy, x0 + ix], inside, tie_band(u, v)


def ref_apply(u8, params, C, mean, std, rescale=np.float32(1.0 / 255.0)):
    """u8 [B, Hs, Ws, 3] uint8, params [B, 16] fp32 -> (out [B, 3, C, C] float64, fill [B, C, C], band [B, C, C], exact [B]).
    exact[b]: sample b is not jittered, and out[b] then holds the device's fp32 values exactly (see the module docstring)."""
    B = u8.shape[0]
    mean32, std32 = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    mean64, std64, r64 = mean32.astype(np.float64), std32.astype(np.float64), float(np.float32(rescale))
    out, fill, band, exact = np.zeros((B, 3, C, C)), np.zeros((B, C, C), bool), np.zeros((B, C, C), bool), np.zeros(B, bool)
    for b in range(B):
        p = params[b]
        px, inside, band[b] = gather64(u8[b], p, C)
        fill[b] = ~inside
        fb, fc, order = float(p[6]), float(p[7]), p[8] != 0
        if fb == 1.0 and fc == 1.0:
            num = (px.astype(np.float64) * r64 - mean64).astype(np.float32).astype(np.float64)      # = fma(byte, rescale, -mean) in fp32
            val = (num / std64).astype(np.float32).astype(np.float64)                               # = the fp32 division
            val[~inside] = 0.0
            out[b], exact[b] = val.transpose(2, 0, 1), True
            continue
        val = np.where(inside[..., None], (px.astype(np.float32) * np.float32(rescale)).astype(np.float64), mean64)      # pixel space
        gray = lambda t: 0.2989 * t[..., 0] + 0.587 * t[..., 1] + 0.114 * t[..., 2]
        bright = lambda t: np.clip(fb * t, 0.0, 1.0) if fb != 1.0 else t
        contrast = lambda t: np.clip(fc * t + (1.0 - fc) * gray(t).mean(), 0.0, 1.0) if fc != 1.0 else t
        val = bright(contrast(val)) if order else contrast(bright(val))
        out[b] = ((val - mean64) / std64).transpose(2, 0, 1)
    return out, fill, band, exact


def to_bf16(x64):
    return torch.from_numpy(np.asarray(x64)).float().to(BF)


def source(B, Hs, Ws, seed):
    """smooth + noise, every byte value likely present"""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 3, Hs // 4 + 2, Ws // 4 + 2, generator=g)
    up = torch.nn.functional.interpolate(base, size=(Hs, Ws), mode="bilinear").permute(0, 2, 3, 1)
    return (up * 300 - 20 + torch.randn(B, Hs, Ws, 3, generator=g) * 25).clamp(0, 255).to(torch.uint8).contiguous()


def run_apply(u8, params, cfg):
    from medmoe_amd.data import augment_apply
    out = augment_apply(u8.to(DEV), torch.from_numpy(np.asarray(params, np.float32)).to(DEV), cfg)
    torch.cuda.synchronize()
    return out.cpu()


def grid_sample_check(C, cases=((17, 3, -2, 0.8), (-33.5, -4, 5, 1.25), (7.25, 0, 0, 0.9))):
    """The convention of matrix64 / gather64 against torch.nn.functional.affine_grid + grid_sample(nearest, zeros, align_corners=False) on
    the CPU, for a square C: theta = [[m00, m01, 2 t0 / C], [m10, m11, 2 t1 / C]], t0 = m02 - c + (m00 + m01) c, t1 likewise.
    Returns the excluded fractions."""
    F = torch.nn.functional
    src = source(len(cases), C, C, 11 + C)
    c, left = (C - 1) / 2.0, []
    for b, case in enumerate(cases):
        p = np.asarray(record(matrix64(*case, C), raw=case), np.float32)
        px, inside, band = gather64(src[b].numpy(), p, C)
        m = p[:6].astype(np.float64)
        t0, t1 = m[2] - c + (m[0] + m[1]) * c, m[5] - c + (m[3] + m[4]) * c
        theta = torch.tensor([[m[0], m[1], 2 * t0 / C], [m[3], m[4], 2 * t1 / C]], dtype=torch.float64)[None]
        img = src[b].permute(2, 0, 1)[None].double() + 1.0                 # + 1: a gathered 0 is not the padding's 0
        got = F.grid_sample(img, F.affine_grid(theta, (1, 3, C, C), align_corners=False), mode="nearest", padding_mode="zeros",
                            align_corners=False)[0].permute(1, 2, 0).numpy()
        want = np.where(inside[..., None], px.astype(np.float64) + 1.0, 0.0)
        assert np.array_equal(got[~band], want[~band]), (C, case, int((got[~band] != want[~band]).sum()))
        left.append(band.mean())
    return left


# ------------------------------------------------------------------------------------------------------------------------------
# 1. identity
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain64(ops):
    """4 images of different sizes, and what the existing path makes of them at size 64"""
    from medmoe_amd.data import preprocess_images_bicubic
    g = torch.Generator().manual_seed(3)
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(DEV) for h, w in ((90, 131), (64, 64), (33, 200), (257, 70))]
    out, u8 = preprocess_images_bicubic(imgs, size=64, return_uint8=True)
    torch.cuda.synchronize()
    return imgs, out, u8


def test_identity_is_the_existing_path_and_the_centre_crop_its_slice(ops, plain64):
    from medmoe_amd.data import AugmentConfig, augment_apply, augment_params, preprocess_augmented, resize_images_bicubic
    imgs, want, want_u8 = plain64
    cfg = AugmentConfig(imsize=64).validate()
    params = augment_params(cfg, 4, 0, 0, False, DEV)
    assert torch.equal(params.cpu(), torch.tensor([record()] * 4, dtype=torch.float32))
    u8 = resize_images_bicubic(imgs, 64)
    assert torch.equal(u8, want_u8)
    got = augment_apply(u8, params, cfg)
    assert got.dtype == BF and tuple(got.shape) == (4, 3, 64, 64)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(preprocess_augmented(imgs, cfg, 5, train=False)), bits(want))
    # augmentation on, every step off: the training path is the identity too
    assert torch.equal(bits(preprocess_augmented(imgs, cfg, 5, train=True)), bits(want))
    for C, off in ((56, 4), (57, 4), (59, 2)):                            # (64 - C) / 2 = 4, 3.5 -> 4, 2.5 -> 2: Python's round
        cfgc = AugmentConfig(imsize=64, crop_size=C).validate()
        pc = augment_params(cfgc, 4, 0, 0, False, DEV)
        assert torch.equal(pc.cpu(), torch.tensor([record(x0=off, y0=off)] * 4, dtype=torch.float32)), C
        got = augment_apply(u8, pc, cfgc)
        assert torch.equal(bits(got), bits(want[:, :, off:off + C, off:off + C])), C


# ------------------------------------------------------------------------------------------------------------------------------
# 2. exact geometry
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 30])
def test_hand_made_geometry_is_exact_on_every_pixel(ops, C):
    from medmoe_amd.data import AugmentConfig
    Hs, Ws = 36, 40
    src = source(5, Hs, Ws, 21)
    c = (C - 1) / 2.0
    quarter = [0.0, 1.0, 3.0, -1.0, 0.0, 2.0 * c + 2.0]                   # 90 degrees, tx = 2, ty = -3: entries 0 / +-1
    assert np.allclose(quarter, matrix64(90.0, 2, -3, 1.0, C), atol=1e-12)
    zoom = matrix64(0.0, 0, 0, 2.0, C)                                    # u = x / 2 + c / 2: never a tie
    params = np.asarray([record(), record(x0=Ws - C, y0=Hs - C), record(flip=1, x0=3, y0=2),
                         record(quarter, x0=1, y0=4, raw=(90, 2, -3, 1)), record(zoom, x0=5, y0=0, raw=(0, 0, 0, 2))], np.float32)
    cfg = AugmentConfig(imsize=64, crop_size=C).validate()
    mean, std = cfg.mean_std()
    ref, fill, band, exact = ref_apply(src.numpy(), params, C, mean, std)
    assert exact.all() and not band.any()
    assert fill[3].any() and not fill[[0, 1, 2, 4]].any()                 # only the shifted quarter turn looks outside the crop
    got = run_apply(src, params, cfg)
    assert torch.equal(bits(got), bits(to_bf16(ref)))
    f = torch.from_numpy(fill)[:, None].expand(-1, 3, -1, -1)
    assert not bool(bits(got)[f].any())                                   # fill = normalised zero, the bit pattern
    # not square: a swapped axis would read other bytes
    assert torch.equal(got[1], to_bf16(ref_apply(src.numpy()[1:2, Hs - C:, Ws - C:], params[:1], C, mean, std)[0][0]))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. general affine
# ------------------------------------------------------------------------------------------------------------------------------
AFFINE = ((17, 3, -2, 0.8), (-33.5, -4, 5, 1.25), (7.25, 0, 0, 0.9))


@pytest.mark.parametrize("C", [32, 40])
def test_general_affine_matches_float64_outside_the_tie_band(ops, C):
    from medmoe_amd.data import AugmentConfig
    Hs, Ws = 44, 48
    src = source(len(AFFINE), Hs, Ws, 31)
    params = np.asarray([record(matrix64(*case, C), x0=5, y0=3, raw=case) for case in AFFINE], np.float32)
    cfg = AugmentConfig(imsize=64, crop_size=C).validate()
    ref, fill, band, exact = ref_apply(src.numpy(), params, C, *cfg.mean_std())
    assert exact.all()
    left = band.reshape(len(AFFINE), -1).mean(1)
    print("excluded fraction per case:", left)
    assert (left <= 0.02).all(), left
    assert fill.any(1).any(1).all()                                       # every case has fill pixels
    got = run_apply(src, params, cfg)
    keep = torch.from_numpy(~band)[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(bits(got)[keep], bits(to_bf16(ref))[keep])
    assert max(grid_sample_check(C, AFFINE)) <= 0.02


# ------------------------------------------------------------------------------------------------------------------------------
# 4. jitter
# ------------------------------------------------------------------------------------------------------------------------------
JITTER = ((0.6, 1.4), (1.3, 0.7), (1.0, 1.5), (0.5, 1.0))
JITTER_TURN = (29.0, 2, -1, 0.9)      # sample 1 is also turned: fill pixels enter its gray mean (no pixel of it within 1e-3 of a tie)


def jitter_params(C, order, factors=JITTER):
    rows = []
    for b, (fb, fc) in enumerate(factors):
        m, raw = (matrix64(*JITTER_TURN, C), JITTER_TURN) if b == 1 else ((1, 0, 0, 0, 1, 0), (0, 0, 0, 1))
        rows.append(record(m, fb=fb, fc=fc, order=order, flip=b & 1, x0=2 + b, y0=b, raw=raw))
    return np.asarray(rows, np.float32)


@pytest.mark.parametrize("order", [0, 1])
def test_jitter_matches_float64(ops, order):
    from medmoe_amd.data import AugmentConfig
    C = 32
    src = source(4, 36, 40, 41)
    cfg = AugmentConfig(imsize=64, crop_size=C).validate()
    params = jitter_params(C, order)
    ref, fill, band, exact = ref_apply(src.numpy(), params, C, *cfg.mean_std())
    assert not band.any() and fill[1].any() and not exact.any()           # no pixel near a tie: the gray mean is determined
    got = run_apply(src, params, cfg)
    ref_t = torch.from_numpy(ref)
    err = (got.double() - ref_t).abs()
    bar = 2.0 ** -8 * ref_t.abs() + 1e-5
    print("order", order, "worst error / bar:", float((err / bar).max()))
    assert bool((err <= bar).all()), float((err / bar).max())
    assert torch.equal(bits(run_apply(src, params, cfg)), bits(got))       # two runs
    # the jitter does something, in both orders differently where both operations are on
    plain = run_apply(src, jitter_params(C, order, ((1.0, 1.0),) * 4), cfg)
    other = run_apply(src, jitter_params(C, 1 - order), cfg)
    assert not torch.equal(got[0], plain[0]) and not torch.equal(got[0], other[0])
    assert torch.equal(bits(got[2:]), bits(other[2:]))                    # one operation on: the order bit changes nothing


def test_factors_of_exactly_one_leave_the_bits_alone(ops):
    from medmoe_amd.data import AugmentConfig
    C = 32
    src = source(4, 36, 40, 41)
    cfg = AugmentConfig(imsize=64, crop_size=C).validate()
    ones = ((1.0, 1.0),) * 4
    a, b = run_apply(src, jitter_params(C, 0, ones), cfg), run_apply(src, jitter_params(C, 1, ones), cfg)
    params = jitter_params(C, 0, ones)
    ref, fill, band, exact = ref_apply(src.numpy(), params, C, *cfg.mean_std())
    assert exact.all() and not band.any()
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(to_bf16(ref)))


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the draws
# ------------------------------------------------------------------------------------------------------------------------------
def host_draws(B, sample0, seed, step, S, C, cfg):
    """float64 / integer restatement of the draw layout: group 4 g + j, counter (lo, hi, site, step), key = the halves of the seed"""
    g = np.arange(sample0, sample0 + B, dtype=np.uint64)
    seed &= 0xFFFFFFFFFFFFFFFF

    def block(j):
        grp = np.uint64(4) * g + np.uint64(j)
        w = philox4x32_10(grp & np.uint64(0xFFFFFFFF), grp >> np.uint64(32), np.full(B, SITE_AUGMENT, np.uint64),
                          np.full(B, step & 0xFFFFFFFF, np.uint64), seed & 0xFFFFFFFF, seed >> 32)
        return [x.astype(np.uint64) for x in w]

    uni = lambda w, lo, hi: lo + (hi - lo) * ((w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24)
    w0, w1, w2 = block(0), block(1), block(2)
    n = np.uint64(S - C + 1)
    return {"x0": ((w0[0] * n) >> np.uint64(32)).astype(np.int64), "y0": ((w0[1] * n) >> np.uint64(32)).astype(np.int64),
            "flip": w0[2] < np.uint64(min(int(cfg.flip_p * 4294967296.0), 0xFFFFFFFF)), "order": (w0[3] >> np.uint64(31)).astype(np.int64),
            "angle": uni(w1[0], *cfg.degrees), "tx": uni(w1[1], -cfg.translate[0] * C, cfg.translate[0] * C),
            "ty": uni(w1[2], -cfg.translate[1] * C, cfg.translate[1] * C), "scale": uni(w1[3], *cfg.scale),
            "fb": uni(w2[0], *cfg.brightness), "fc": uni(w2[1], *cfg.contrast)}


def draw_cfg(S=40, C=32, seed=1234):
    from medmoe_amd.data import AugmentConfig
    return AugmentConfig(imsize=S, crop_size=C, flip_p=0.5, degrees=(-20.0, 20.0), translate=(0.1, 0.1), scale=(0.8, 1.25),
                         brightness=(0.6, 1.4), contrast=(0.6, 1.4), seed=seed).validate()


def test_the_draws_are_the_host_philox_values(ops):
    from medmoe_amd.data import augment_params
    B, S, C, step = 4096, 40, 32, 7
    cfg = draw_cfg(S, C)
    p = augment_params(cfg, B, 0, step, True, DEV).cpu().numpy()
    assert p.shape == (B, REC) and p.dtype == np.float32
    h = host_draws(B, 0, cfg.seed, step, S, C, cfg)
    assert np.array_equal(p[:, 14], h["x0"]) and np.array_equal(p[:, 15], h["y0"])
    assert np.array_equal(p[:, 9], h["flip"]) and np.array_equal(p[:, 8], h["order"])
    for col, key, (lo, hi) in ((10, "angle", cfg.degrees), (13, "scale", cfg.scale), (6, "fb", cfg.brightness), (7, "fc", cfg.contrast)):
        tol = 2.0 ** -22 * max(abs(lo), abs(hi), 1.0)
        assert np.abs(p[:, col].astype(np.float64) - h[key]).max() <= tol, key
        assert lo - tol <= p[:, col].min() and p[:, col].max() <= hi + tol, key
        assert abs(p[:, col].astype(np.float64).mean() - 0.5 * (lo + hi)) <= 6.0 * (hi - lo) / math.sqrt(12.0 * B), key
    lim = float(np.rint(0.1 * C))
    for col, key in ((11, "tx"), (12, "ty")):
        t = p[:, col].astype(np.float64)
        assert np.array_equal(t, np.rint(t)) and np.abs(t).max() <= lim, key
        clear = ~tie_band(h[key], h[key], 1e-5)                           # a raw shift that close to a tie may round either way in fp32
        assert clear.mean() > 0.99 and np.array_equal(t[clear], np.rint(h[key])[clear]), key
        assert set(np.unique(t)) == set(np.arange(-lim, lim + 1)), key
    # the matrix from the raw draws of the record
    want = np.asarray([matrix64(*row.astype(np.float64), C) for row in p[:, 10:14]])
    s = p[:, 13].astype(np.float64)
    d = np.abs(p[:, :6].astype(np.float64) - want)
    assert (d[:, [0, 1, 3, 4]] <= (1e-5 / s)[:, None]).all()
    assert (d[:, [2, 5]] <= 1e-5 * C * (1.0 + 1.0 / cfg.scale[0])).all()
    # statistics
    assert set(np.unique(p[:, 14])) == set(range(S - C + 1)) and set(np.unique(p[:, 15])) == set(range(S - C + 1))
    assert abs(int(p[:, 9].sum()) - B // 2) <= 192 and abs(int(p[:, 8].sum()) - B // 2) <= 192
    assert set(np.unique(p[:, 8])) == {0.0, 1.0} and set(np.unique(p[:, 9])) == {0.0, 1.0}


def test_a_sample_draws_the_same_whatever_the_launch(ops):
    from medmoe_amd.data import augment_params
    cfg = draw_cfg()
    full = augment_params(cfg, 8, 0, 3, True, DEV)
    tail = augment_params(cfg, 4, 4, 3, True, DEV)
    assert torch.equal(full[4:].view(torch.int32), tail.view(torch.int32))
    assert torch.equal(augment_params(cfg, 8, 0, 3, True, DEV).view(torch.int32), full.view(torch.int32))
    for other in (augment_params(cfg, 8, 0, 4, True, DEV), augment_params(draw_cfg(seed=1235), 8, 0, 3, True, DEV),
                  augment_params(draw_cfg(seed=1234 + (1 << 32)), 8, 0, 3, True, DEV)):
        assert not torch.equal(other[:, 6:], full[:, 6:])
    # a sample index past 2^30: the group 4 g + j needs its high word
    far = augment_params(cfg, 2, (1 << 31) + 5, 3, True, DEV).cpu().numpy()
    h = host_draws(2, (1 << 31) + 5, cfg.seed, 3, 40, 32, cfg)
    assert np.array_equal(far[:, 14], h["x0"]) and np.array_equal(far[:, 9], h["flip"])
    # validation: the centre crop, Python's round for an odd difference, identity everything else
    for S, want in ((40, 4), (41, 4), (43, 6)):
        ev = augment_params(draw_cfg(S, 32), 3, 0, 3, False, DEV).cpu()
        assert torch.equal(ev, torch.tensor([record(x0=want, y0=want)] * 3, dtype=torch.float32)), S


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the pipeline
# ------------------------------------------------------------------------------------------------------------------------------
BLOCK = {"norm": "imagenet", "imsize": 64, "random_crop": {"crop_size": 56}, "random_horizontal_flip": 0.5,
         "random_affine": {"degrees": 20, "translate": [0.1, 0.1], "scale": [0.95, 1.05]},
         "color_jitter": {"bightness": [0.8, 1.2], "contrast": [0.8, 1.2]}, "seed": 9}


def test_datamodule_augments_resumes_and_validates_with_the_centre_crop(ops, plain64):
    from src.data.unimed_datamodule import UnimedDataModule
    imgs, want, _ = plain64
    batch = {"image": [im.cpu() for im in imgs], "caption": [torch.arange(1, 7)] * 4, "label": torch.zeros(4, dtype=torch.long)}
    before = ops.nondet_launches()
    dm = UnimedDataModule(transformations=BLOCK, batch_size=4, synthetic_size=8)
    a = dm.device_batch(batch, DEV, 56, True)
    b = dm.device_batch(batch, DEV, 56, True)
    assert tuple(a["image"].shape) == (4, 3, 56, 56) and a["image"].dtype == BF and torch.equal(a["ids"], b["ids"])
    assert all(not torch.equal(a["image"][i], b["image"][i]) for i in range(4))
    assert dm.state_dict() == {"augment_step": 2}
    dm2 = UnimedDataModule(transformations=BLOCK, batch_size=4, synthetic_size=8)
    dm2.load_state_dict(dm.state_dict())
    ev = dm.device_batch(batch, DEV, 56, False)                            # evaluation does not move the counter
    assert torch.equal(bits(ev["image"]), bits(want[:, :, 4:60, 4:60]))
    assert torch.equal(bits(dm.device_batch(batch, DEV, 56, True)["image"]), bits(dm2.device_batch(batch, DEV, 56, True)["image"]))
    fresh = UnimedDataModule(transformations=BLOCK, batch_size=4, synthetic_size=8)
    assert torch.equal(bits(fresh.device_batch(batch, DEV, 56, True)["image"]), bits(a["image"]))
    # no block: the existing path, the same bits
    none = UnimedDataModule(batch_size=4, synthetic_size=8).device_batch(batch, DEV, 64, True)
    assert torch.equal(bits(none["image"]), bits(want))
    with pytest.raises(ValueError, match=r"data\.transformations\.random_crop\.crop_size.*64"):
        dm.device_batch(batch, DEV, 64, True)
    torch.cuda.synchronize()
    assert ops.nondet_launches() == before


def test_bad_shapes_return_the_error_codes(ops):
    fp, fa = ops._fn("augment_params"), ops._fn("augment_apply")
    buf = torch.zeros(4, REC, device=DEV)
    src = torch.zeros(4, 8, 10, 3, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(4, 3, 8, 8, dtype=BF, device=DEV)
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    ma = ctypes.addressof(m)
    stream = ops._stream_handle()
    ranges = (0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)

    def par(B=4, S=10, C=8, s0=1.0, s1=1.0, ptr=buf.data_ptr()):
        r = list(ranges); r[4], r[5] = s0, s1
        return fp(ptr, B, 0, 0, 0, S, C, 1, 0, *r, stream)

    def app(B=4, Hs=8, Ws=10, C=8, s=src.data_ptr(), p=buf.data_ptr(), d=dst.data_ptr(), mean=ma, std=ma):
        return fa(s, p, d, B, Hs, Ws, C, 1.0 / 255.0, mean, std, stream)
    assert par() == 0 and app() == 0
    assert par(ptr=None) == -1
    assert [par(B=0), par(C=0), par(C=11), par(s0=0.0), par(s0=-1.0, s1=1.0), par(s0=1.0, s1=0.5)] == [-2] * 6
    assert [app(s=None), app(p=None), app(d=None), app(mean=None), app(std=None)] == [-1] * 5
    assert [app(B=0), app(C=0), app(C=9), app(Hs=10, Ws=8, C=9)] == [-2] * 4
    torch.cuda.synchronize()
