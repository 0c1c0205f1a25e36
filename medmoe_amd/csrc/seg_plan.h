// Bilinear upsample geometry of the segmentation head, shared by csrc/segment.hip (device) and tools/seg_plan_check.cpp (host).
// The map is torch.nn.functional.interpolate(mode="bilinear", align_corners=False): src = (dst + 0.5) (g / H) - 0.5 clamped below at 0,
// i0 = floor(src), i1 = min(i0 + 1, g - 1), lambda = src - i0; the pixel reads patch i0 with weight 1 - lambda and patch i1 with lambda.
// The ADJOINT in gather form needs, per patch i, the pixels that read it with a non-zero weight: because src is monotone in dst (every step
// of seg_src is monotone under round-to-nearest) they are ONE contiguous range, found by bisection on seg_src itself - no closed form whose
// rounding could disagree with the forward map.
#pragma once

#if defined(__HIPCC__)
#define SEG_HD __host__ __device__ __forceinline__
#else
#define SEG_HD inline
#endif

struct SegSrc {
  int i0, i1;
  float lam;
};

SEG_HD float seg_scale(int g, int H) { return (float)g / (float)H; }

// dst may lie past the last pixel (a padded lane): i0 stays <= g - 1, so whatever it indexes is inside the patch grid.
SEG_HD SegSrc seg_src(int dst, float scale, int g) {
#if defined(__clang__)
#pragma clang fp contract(off)                                  // the same bits on the host and on the device: no fused multiply-add
#endif
  float src = ((float)dst + 0.5f) * scale - 0.5f;
  if (!(src > 0.f)) src = 0.f;
  int i0 = (int)src;                                            // src >= 0: truncation is floor
  if (i0 > g - 1) i0 = g - 1;
  SegSrc s;
  s.i0 = i0;
  s.i1 = i0 + 1 < g ? i0 + 1 : g - 1;
  s.lam = src - (float)i0;
  if (s.lam > 1.f) s.lam = 1.f;
  return s;
}

// the weight with which the pixel of `s` reads patch i (both corners when they coincide at the last patch)
SEG_HD float seg_weight(SegSrc s, int i) { return (s.i0 == i ? 1.f - s.lam : 0.f) + (s.i1 == i ? s.lam : 0.f); }

// true from the first pixel on that reads patch i with a non-zero weight (monotone in dst)
SEG_HD bool seg_reaches(int dst, float scale, int g, int i) {
  const SegSrc s = seg_src(dst, scale, g);
  return s.i0 >= i || (s.i0 == i - 1 && s.lam > 0.f);
}

// [lo, hi): the pixels of an axis of H pixels over g patches that read patch i with a non-zero weight
SEG_HD void seg_support(int i, int g, int H, int* lo, int* hi) {
  const float scale = seg_scale(g, H);
  int a = 0, b = H;
  while (a < b) {
    const int m = (a + b) >> 1;
    if (seg_reaches(m, scale, g, i)) b = m; else a = m + 1;
  }
  *lo = a;
  b = H;
  while (a < b) {
    const int m = (a + b) >> 1;
    if (seg_src(m, scale, g).i0 > i) b = m; else a = m + 1;
  }
  *hi = a;
}
