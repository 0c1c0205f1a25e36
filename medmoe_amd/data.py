"""Device-side image preprocessing.

The reference hands lists of PIL images to HF AutoImageProcessor on the CPU every step (swin.py:131; for
microsoft/swin-tiny-patch4-window7-224 that is a PIL BICUBIC resize to 224x224 on uint8, x 1/255, ImageNet mean/std).  Here decoded
images are uint8 HWC tensors (any size) already on the device; two launches (horizontal, vertical pass) resize with Pillow's own
fixed-point arithmetic, rescale, normalise and lay the batch out as the bf16 [B,3,H,W] tensor the patch-embedding kernels read.

Train-time augmentation: the reference's `transformations` block (src/utils/utils.py:16-68, build_transformation) as an
AugmentConfig and two more launches behind the resize - medmoe_augment_params draws every sample's crop, flip, affine and colour-jitter
parameters on the device, medmoe_augment_apply gathers, jitters, normalises (csrc/augment.hip).  preprocess_augmented runs the three.
"""
import ctypes as _c
import dataclasses
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import load_library

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


_COEF_CACHE = {}


def _cubic(x: float) -> float:
    """Keys cubic a = -0.5, the kernel of Pillow's BICUBIC filter (support 2)."""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bicubic_coeffs(in_size: int, out_size: int):
    """Per-output-coordinate source window [xmin, xmin + n) and 22-bit fixed-point weights of Pillow's antialiased BICUBIC resampler
    (what the reference's HF image processor calls, swin.py:131).  Plain-Python double arithmetic in the order Pillow's C code
    uses, so the integer weights are the same.  Returns (bounds int32 [out, 2], weights int32 [out, ksize], ksize)."""
    key = (in_size, out_size)
    if key in _COEF_CACHE:
        return _COEF_CACHE[key]
    import math

    import numpy as np
    scale = in_size / out_size
    fscale = scale if scale >= 1.0 else 1.0
    support = 2.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / fscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = _cubic((x + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * (1 << 22)) if k < 0 else int(0.5 + k * (1 << 22))
        bounds[xx] = (xmin, xmax)
    _COEF_CACHE[key] = (bounds, kk, ksize)
    return _COEF_CACHE[key]


def preprocess_images_bicubic(images: Sequence[torch.Tensor], size: int = 224, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                              rescale: float = 1.0 / 255.0, out: torch.Tensor = None, return_uint8: bool = False):
    """The reference's preprocessing (HF image processor: PIL BICUBIC resize to size x size on uint8, x 1/255, (x - mean) / std),
    on the device.  images: B uint8 tensors [H_b, W_b, 3] on the GPU (contiguous).  Returns bf16 [B, 3, size, size]
    (and the resized uint8 [B, size, size, 3] when return_uint8)."""
    return _bicubic(images, size, mean, std, rescale, out, return_uint8, True)


def resize_images_bicubic(images: Sequence[torch.Tensor], size: int) -> torch.Tensor:
    """The resize of preprocess_images_bicubic alone: the uint8 [B, size, size, 3] image, no normalised tensor written."""
    return _bicubic(images, size, IMAGENET_MEAN, IMAGENET_STD, 1.0 / 255.0, None, True, False)


def _bicubic(images, size, mean, std, rescale, out, return_uint8, normalised):
    import numpy as np
    lib = load_library()
    B = len(images)
    if B == 0:
        raise ValueError("preprocess_images_bicubic: empty batch")
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous():
            raise TypeError("preprocess_images_bicubic: every image must be a contiguous uint8 [H, W, 3] tensor")
        ops._require_gpu(im, "medmoe_preprocess_bicubic")
    dev = images[0].device
    coef, offs, meta, row0 = [], {}, [], 0

    def table(n_in):
        if n_in not in offs:
            b, k, ks = bicubic_coeffs(n_in, size)
            pos = sum(c.size for c in coef)
            coef.append(b.reshape(-1)); coef.append(k.reshape(-1))
            offs[n_in] = (pos, pos + b.size, ks)
        return offs[n_in]
    for im in images:
        H, W = int(im.shape[0]), int(im.shape[1])
        bh, kh, ksh = table(W)
        bv, kv, ksv = table(H)
        meta.append([H, W, ksh, ksv, bh, kh, bv, kv, row0])
        row0 += H
    coef_t = torch.from_numpy(np.concatenate(coef).astype(np.int32)).to(dev, non_blocking=True)
    meta_t = torch.tensor(meta, dtype=torch.int64).to(dev, non_blocking=True)
    ptrs = torch.tensor([im.data_ptr() for im in images], dtype=torch.int64).to(dev, non_blocking=True)
    tmp = torch.empty(row0 * size * 3, device=dev, dtype=torch.uint8)
    if out is None and normalised:
        out = torch.empty(B, 3, size, size, device=dev, dtype=torch.bfloat16)
    u8 = torch.empty(B, size, size, 3, device=dev, dtype=torch.uint8) if return_uint8 else None
    m = (_c.c_float * 3)(*mean)
    s_ = (_c.c_float * 3)(*std)
    rc = lib.medmoe_preprocess_bicubic(_c.c_void_p(ptrs.data_ptr()), _c.c_void_p(meta_t.data_ptr()), _c.c_void_p(coef_t.data_ptr()),
                                       _c.c_void_p(tmp.data_ptr()), _c.c_void_p(out.data_ptr() if normalised else 0),
                                       _c.c_void_p(u8.data_ptr() if u8 is not None else 0),
                                       _c.c_int(B), _c.c_int(size), _c.c_int(size), _c.c_longlong(row0), _c.c_float(rescale), m, s_, ops._stream())
    ops._chk(rc, "preprocess_bicubic")
    if not normalised:
        return u8
    return (out, u8) if return_uint8 else out


def preprocess_images(images: Sequence[torch.Tensor], size: int = 224, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                      rescale: float = 1.0 / 255.0, out: torch.Tensor = None, resample: str = "bicubic") -> torch.Tensor:
    """images: B uint8 tensors [H_b, W_b, 3] on the GPU (contiguous).  Returns bf16 [B, 3, size, size].
    resample "bicubic" (default) = the reference's filter (preprocess_images_bicubic); "bilinear" = torch's half-pixel bilinear."""
    if resample == "bicubic":
        return preprocess_images_bicubic(images, size, mean, std, rescale, out)
    if resample != "bilinear":
        raise ValueError("resample must be 'bicubic' or 'bilinear'")
    lib = load_library()
    B = len(images)
    if B == 0:
        raise ValueError("preprocess_images: empty batch")
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous():
            raise TypeError("preprocess_images: every image must be a contiguous uint8 [H, W, 3] tensor")
        ops._require_gpu(im, "medmoe_preprocess")
    dev = images[0].device
    ptrs = torch.tensor([im.data_ptr() for im in images], dtype=torch.int64).to(dev, non_blocking=True)
    hw = torch.tensor([[im.shape[0], im.shape[1]] for im in images], dtype=torch.int32).to(dev, non_blocking=True)
    if out is None:
        out = torch.empty(B, 3, size, size, device=dev, dtype=torch.bfloat16)
    m = (_c.c_float * 3)(*mean)
    s = (_c.c_float * 3)(*std)
    rc = lib.medmoe_preprocess(_c.c_void_p(ptrs.data_ptr()), _c.c_void_p(hw.data_ptr()), _c.c_void_p(out.data_ptr()), _c.c_int(B),
                               _c.c_int(size), _c.c_int(size), _c.c_float(rescale), m, s, ops._stream())
    ops._chk(rc, "preprocess")
    return out


# ---------------------------------------------------------------------------------------------
# train-time augmentation (csrc/augment.hip)
# ---------------------------------------------------------------------------------------------
NORMS = {"imagenet": (IMAGENET_MEAN, IMAGENET_STD), "half": ((0.5,) * 3, (0.5,) * 3), "slake": ((0.2469,) * 3, (0.2292,) * 3),
         "pmcoa": ((0.1307,) * 3, (0.3081,) * 3), "false": ((0.0,) * 3, (1.0,) * 3)}          # utils.py:27-37
AUG_REC = 16                                                         # floats per sample, layout in include/medmoe_hip.h
_KEY = "data.transformations."


def _pair(v, key) -> Tuple[float, float]:
    try:
        a, b = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"{_KEY}{key}: expected two numbers, got {v!r}") from None
    return (a, b)


def center_crop_offset(S: int, C: int) -> int:
    """torchvision's center_crop: int(round((S - C) / 2.0)) with Python's round (half to even)"""
    return int(round((S - C) / 2.0))


@dataclasses.dataclass
class AugmentConfig:
    """The reference's `transformations` block (configs/data/*.yaml of the reference; read by build_transformation, utils.py:16-68).  A step
    that is off holds the value that makes it the identity: no crop (crop_size None), flip probability 0, a zero angle / shift range, scale
    and jitter ranges (1, 1)."""
    imsize: int = 224
    norm: str = "imagenet"
    crop_size: Optional[int] = None                    # random_crop.crop_size
    flip_p: float = 0.0                                # random_horizontal_flip
    degrees: Tuple[float, float] = (0.0, 0.0)          # random_affine.degrees: d -> (-d, d)
    translate: Tuple[float, float] = (0.0, 0.0)        # random_affine.translate, fractions of the output size
    scale: Tuple[float, float] = (1.0, 1.0)            # random_affine.scale
    brightness: Tuple[float, float] = (1.0, 1.0)       # color_jitter.brightness (the reference spells it `bightness`)
    contrast: Tuple[float, float] = (1.0, 1.0)         # color_jitter.contrast
    seed: int = 0

    @property
    def out_size(self) -> int:
        return self.imsize if self.crop_size is None else self.crop_size

    def mean_std(self):
        return NORMS[self.norm]

    @classmethod
    def from_hydra(cls, block) -> "AugmentConfig":
        if block is None:
            raise ValueError(f"{_KEY[:-1]}: no block to build an AugmentConfig from")
        if "imsize" not in block:
            raise ValueError(f"{_KEY}imsize: missing (the size the images are resized to)")
        cfg = cls(imsize=block.get("imsize"), seed=block.get("seed", 0))
        norm = block.get("norm", "imagenet")
        cfg.norm = "false" if norm is None or norm is False else norm          # utils.py:27 `if cfg.norm:`
        crop = block.get("random_crop")
        if crop:
            if "crop_size" not in crop:
                raise ValueError(f"{_KEY}random_crop.crop_size: missing")
            cfg.crop_size = crop.get("crop_size")
        flip = block.get("random_horizontal_flip")
        if flip:
            cfg.flip_p = flip
        aff = block.get("random_affine")
        if aff:
            d = aff.get("degrees", 0.0)
            if isinstance(d, (int, float)):
                if d < 0:
                    raise ValueError(f"{_KEY}random_affine.degrees: a single number must be >= 0, got {d}")
                cfg.degrees = (-float(d), float(d))
            else:
                cfg.degrees = _pair(d, "random_affine.degrees")
            if aff.get("translate") is not None:
                cfg.translate = _pair(aff.get("translate"), "random_affine.translate")
            if aff.get("scale") is not None:
                cfg.scale = _pair(aff.get("scale"), "random_affine.scale")
        jit = block.get("color_jitter")
        if jit:
            for key in ("brightness", "bightness", "contrast"):            # `bightness`: the reference's spelling (utils.py:60)
                if jit.get(key) is not None:
                    setattr(cfg, "contrast" if key == "contrast" else "brightness", _pair(jit.get(key), "color_jitter." + key))
        cfg.validate()
        return cfg

    def validate(self) -> "AugmentConfig":
        def bad(key, what):
            raise ValueError(f"{_KEY}{key}: {what}")
        if not isinstance(self.imsize, int) or isinstance(self.imsize, bool) or self.imsize <= 0:
            bad("imsize", f"must be a positive integer, got {self.imsize!r}")
        if not isinstance(self.norm, str) or self.norm not in NORMS:
            bad("norm", f"must be one of {sorted(NORMS)} (or absent = imagenet), got {self.norm!r}")
        if self.crop_size is not None and (not isinstance(self.crop_size, int) or isinstance(self.crop_size, bool)
                                           or not 1 <= self.crop_size <= self.imsize):
            bad("random_crop.crop_size", f"must be an integer in [1, imsize = {self.imsize}], got {self.crop_size!r}")
        if not isinstance(self.flip_p, (int, float)) or isinstance(self.flip_p, bool) or not 0.0 <= self.flip_p <= 1.0:
            bad("random_horizontal_flip", f"must be false or a probability in [0, 1], got {self.flip_p!r}")
        d0, d1 = self.degrees
        if not (math.isfinite(d0) and math.isfinite(d1) and d0 <= d1):
            bad("random_affine.degrees", f"must be d >= 0 or [d0, d1] with d0 <= d1, got {self.degrees!r}")
        if not all(0.0 <= t <= 1.0 for t in self.translate):
            bad("random_affine.translate", f"must be two fractions in [0, 1], got {self.translate!r}")
        s0, s1 = self.scale
        if not (0.0 < s0 <= s1 and math.isfinite(s1)):
            bad("random_affine.scale", f"must be [s0, s1] with 0 < s0 <= s1, got {self.scale!r}")
        for key, (lo, hi) in (("color_jitter.brightness", self.brightness), ("color_jitter.contrast", self.contrast)):
            if not (0.0 <= lo <= hi and math.isfinite(hi)):
                bad(key, f"must be [lo, hi] with 0 <= lo <= hi, got {(lo, hi)!r}")
        if not isinstance(self.seed, int) or isinstance(self.seed, bool):
            bad("seed", f"must be an integer, got {self.seed!r}")
        return self


def flip_thresh(p: float) -> int:
    """floor(p * 2^32) as ops.dropout_thresh builds its own, capped at 2^32 - 1: a sample is flipped iff its random word is below this"""
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"flip probability must be in [0, 1], got {p}")
    return min(int(p * 4294967296.0), 0xFFFFFFFF)


def augment_params(cfg: AugmentConfig, B: int, sample0: int, step: int, train: bool, device) -> torch.Tensor:
    """fp32 [B, 16]: the parameter records of the samples sample0 .. sample0 + B - 1 at `step` (layout: include/medmoe_hip.h), drawn on the
    device - a function of (cfg.seed, step, sample0 + b) and the ranges only.  train False: the centre crop, identity everything else."""
    if B <= 0 or sample0 < 0:
        raise ValueError(f"augment_params: B must be positive and sample0 >= 0, got B = {B}, sample0 = {sample0}")
    params = torch.empty(B, AUG_REC, device=device, dtype=torch.float32)
    ops._require_gpu(params, "medmoe_augment_params")
    seed = ops.dropout_rng(cfg.seed, step, ops.DROPOUT_SITE_AUGMENT, 0.0)[0]
    fn = ops._fn("augment_params")
    with ops._Timed("augment_params_kernel", 4.0 * AUG_REC * B, "byte"):
        ops._chk(fn(params.data_ptr(), int(B), int(sample0), seed, step & 0xFFFFFFFF, cfg.imsize, cfg.out_size, 1 if train else 0,
                    flip_thresh(cfg.flip_p), *cfg.degrees, *cfg.translate, *cfg.scale, *cfg.brightness, *cfg.contrast, ops._stream_handle()),
                 "augment_params")
    return params


def augment_apply(u8: torch.Tensor, params: torch.Tensor, cfg: AugmentConfig, out: torch.Tensor = None, rescale: float = 1.0 / 255.0):
    """u8: uint8 [B, Hs, Ws, 3] (the resized images), params: fp32 [B, 16] (augment_params', or any other) -> bf16 [B, 3, C, C],
    C = cfg.out_size: crop, flip, nearest-neighbour affine, brightness / contrast, (x - mean) / std of cfg.norm."""
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3 or not u8.is_contiguous():
        raise TypeError("augment_apply: u8 must be a contiguous uint8 [B, Hs, Ws, 3] tensor")
    B, Hs, Ws, C = int(u8.shape[0]), int(u8.shape[1]), int(u8.shape[2]), cfg.out_size
    if params.dtype != torch.float32 or tuple(params.shape) != (B, AUG_REC) or not params.is_contiguous():
        raise TypeError(f"augment_apply: params must be a contiguous fp32 [{B}, {AUG_REC}] tensor")
    if B <= 0 or C > min(Hs, Ws):
        raise ValueError(f"augment_apply: the output size {C} does not fit the {Hs} x {Ws} source (B = {B})")
    ops._require_gpu(u8, "medmoe_augment_apply"); ops._require_gpu(params, "medmoe_augment_apply")
    if out is None:
        out = torch.empty(B, 3, C, C, device=u8.device, dtype=torch.bfloat16)
    elif out.dtype != torch.bfloat16 or tuple(out.shape) != (B, 3, C, C) or not out.is_contiguous():
        raise TypeError(f"augment_apply: out must be a contiguous bf16 [{B}, 3, {C}, {C}] tensor")
    ops._require_gpu(out, "medmoe_augment_apply")
    mean, std = cfg.mean_std()
    m, s_ = (_c.c_float * 3)(*mean), (_c.c_float * 3)(*std)
    fn = ops._fn("augment_apply")
    with ops._Timed("augment_apply_kernel", B * (3.0 * Hs * Ws + 6.0 * C * C), "byte"):
        ops._chk(fn(u8.data_ptr(), params.data_ptr(), out.data_ptr(), B, Hs, Ws, C, rescale, _c.addressof(m), _c.addressof(s_),
                    ops._stream_handle()), "augment_apply")
    return out


def preprocess_augmented(images: Sequence[torch.Tensor], cfg: AugmentConfig, step: int, sample0: int = 0, train: bool = True) -> torch.Tensor:
    """images: B uint8 tensors [H_b, W_b, 3] on the GPU -> bf16 [B, 3, C, C], C = cfg.out_size: the bicubic resize to cfg.imsize, the
    parameters of (cfg.seed, step, sample0 + b), the augmentation.  train False: resize, centre crop, normalise (utils.py:64-66)."""
    u8 = resize_images_bicubic(images, cfg.imsize)
    params = augment_params(cfg, len(images), sample0, step, train, u8.device)
    return augment_apply(u8, params, cfg)
