// Train-time image augmentation on the device: the reference's `transformations` block (src/utils/utils.py:16-68,
// build_transformation: RandomCrop, RandomHorizontalFlip, RandomAffine, ColorJitter, Normalize; the centre crop at validation) as two
// launches behind the bicubic resize of embed.hip, which leaves the resized uint8 image [B][S][S][3].
//
//   medmoe_augment_params   one thread per sample draws the sample's parameters from the Philox stream of philox.h and writes one record
//                           of 16 floats; the trigonometry of the affine step happens here, once per sample
//   medmoe_augment_apply    one workgroup per image: crop -> flip -> nearest-neighbour affine about the crop's centre -> brightness /
//                           contrast in pixel space -> (x - mean) / std -> bf16 [B][3][C][C].  Takes ANY record buffer (the tests hand it
//                           matrices of their own), so it trusts nothing in it: the crop box is clamped into the source and every
//                           gathered index lies inside the crop box, a fill pixel's included.
//
//   record[b] = {m00 m01 m02 m10 m11 m12 | fb fc | order flip | angle tx ty scale | x0 y0}
//     output pixel (x, y) of the C x C image reads position u = m00 x + m01 y + m02, v = m10 x + m11 y + m12 of the (flipped) crop, pixel
//     (rint(u), rint(v)) with ties to even; outside [0, C) on either axis the pixel is fill = mean_c, normalised zero
//     crop pixel (i, j) is resized pixel (x0 + (flip ? C - 1 - i : i), y0 + j)
//     fb / fc: brightness / contrast factors; a factor of exactly 1 skips its operation, bits untouched
//     order 0: brightness, then contrast (the gray mean is of the brightened image); 1: contrast, then brightness
//     angle (degrees), tx, ty, scale: the raw draws the matrix was built from
//
//   draws (sample g = sample0 + b): key = seed, counter = (group lo, group hi, DROPOUT_SITE_AUGMENT, step), group = 4 g + j
//     j = 0: x0, y0, flip, order     j = 1: angle, tx, ty, scale     j = 2: brightness, contrast
//     integer in [0, n) = (uint64(w) * n) >> 32;  flip = w < flip_thresh;  order = w >> 31;  uniform = lo + (hi - lo) * ((w >> 8) * 2^-24)
//   Nothing of B or the launch geometry enters.  No atomics: the output is a pure function of the inputs.
#include "common.h"
#include "philox.h"

#define AUG_REC 16
#define AUG_THREADS 512
#define AUG_WAVES (AUG_THREADS / 64)

__device__ __forceinline__ float aug_uniform(uint32_t w, float lo, float hi) {
  return fmaf(hi - lo, (float)(w >> 8) * 5.9604644775390625e-8f, lo);              // (w >> 8) * 2^-24 is exact
}

// Python's round((S - C) / 2): half to even, what torchvision's center_crop computes
__device__ __forceinline__ int aug_center(int d) {
  const int h = d >> 1;
  return (d & 1) ? h + (h & 1) : h;
}

__global__ __launch_bounds__(256) void augment_params_kernel(float* __restrict__ params, int B, unsigned long long sample0, uint32_t k0, uint32_t k1,
                                                             uint32_t step, int S, int C, int train, uint32_t flip_thresh, float d0, float d1,
                                                             float tr_x, float tr_y, float s0, float s1, float b0, float b1, float c0, float c1) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float* p = params + (long long)b * AUG_REC;
  const float c = 0.5f * (float)(C - 1);
  float m[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  float fb = 1.f, fc = 1.f, order = 0.f, flip = 0.f, angle = 0.f, tx = 0.f, ty = 0.f, sc = 1.f;
  int x0 = aug_center(S - C), y0 = x0;
  if (train) {
    const unsigned long long g = 4ull * (sample0 + (unsigned long long)b);
    const uint4 w0 = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), DROPOUT_SITE_AUGMENT, step, k0, k1);
    const uint4 w1 = philox4x32_10((uint32_t)(g + 1), (uint32_t)((g + 1) >> 32), DROPOUT_SITE_AUGMENT, step, k0, k1);
    const uint4 w2 = philox4x32_10((uint32_t)(g + 2), (uint32_t)((g + 2) >> 32), DROPOUT_SITE_AUGMENT, step, k0, k1);
    const unsigned long long n = (unsigned long long)(S - C + 1);
    x0 = (int)(((unsigned long long)w0.x * n) >> 32);
    y0 = (int)(((unsigned long long)w0.y * n) >> 32);
    flip = w0.z < flip_thresh ? 1.f : 0.f;
    order = (float)(w0.w >> 31);
    angle = aug_uniform(w1.x, d0, d1);
    const float ax = tr_x * (float)C, ay = tr_y * (float)C;
    tx = rintf(aug_uniform(w1.y, -ax, ax));
    ty = rintf(aug_uniform(w1.z, -ay, ay));
    sc = aug_uniform(w1.w, s0, s1);
    fb = aug_uniform(w2.x, b0, b1);
    fc = aug_uniform(w2.y, c0, c1);
    // inverse of rotate by angle, scale by sc, shift by (tx, ty) about the centre c:  u = ( cos (x - c - tx) + sin (y - c - ty)) / sc + c
    //                                                                                v = (-sin (x - c - tx) + cos (y - c - ty)) / sc + c
    float sn, cs;
    sincosf(angle * 0.017453292519943295f, &sn, &cs);
    const float px = c + tx, py = c + ty;
    m[0] = cs / sc; m[1] = sn / sc; m[2] = c - (cs * px + sn * py) / sc;
    m[3] = -sn / sc; m[4] = cs / sc; m[5] = c - (cs * py - sn * px) / sc;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) p[i] = m[i];
  p[6] = fb; p[7] = fc; p[8] = order; p[9] = flip; p[10] = angle; p[11] = tx; p[12] = ty; p[13] = sc;
  p[14] = (float)x0; p[15] = (float)y0;
}

extern "C" int medmoe_augment_params(float* params, int B, long long sample0, long long seed, long long step, int S, int C, int train,
                                     unsigned flip_thresh, float d0, float d1, float tr_x, float tr_y, float s0, float s1, float b0, float b1,
                                     float c0, float c1, hipStream_t stream) {
  if (!params) return MM_ERR_ARG;
  if (B <= 0 || C <= 0 || C > S || sample0 < 0 || !(s0 > 0.f) || !(s1 >= s0)) return MM_ERR_SHAPE;
  if (!(d1 >= d0) || !(tr_x >= 0.f) || !(tr_y >= 0.f) || !(b0 >= 0.f) || !(b1 >= b0) || !(c0 >= 0.f) || !(c1 >= c0)) return MM_ERR_ARG;
  hipLaunchKernelGGL(augment_params_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, params, B, (unsigned long long)sample0,
                     (uint32_t)((unsigned long long)seed & 0xffffffffull), (uint32_t)((unsigned long long)seed >> 32), (uint32_t)step, S, C, train,
                     (uint32_t)flip_thresh, d0, d1, tr_x, tr_y, s0, s1, b0, b1, c0, c1);
  return mm_check_launch();
}

// ------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------
struct AugSample {
  float m00, m01, m02, m10, m11, m12;
  float fb, fc;
  int order, flip, x0, y0;
};

// Source of output pixel (x, y).  true: inside the crop, off = byte offset of the pixel within the image.  false: fill, and off is that of
// a corner pixel of the crop, so the load behind it needs no branch and a run's 24 loads are in flight together.  Either way the offset
// is inside the crop box, and the box is inside the source (the caller clamped x0 / y0), whatever the matrix holds: a NaN coordinate
// fails the comparisons.
__device__ __forceinline__ bool aug_source(const AugSample& p, int C, int Ws, int x, int y, int& off) {
  const float fx = (float)x, fy = (float)y;
  const float ru = rintf(fmaf(p.m00, fx, fmaf(p.m01, fy, p.m02)));
  const float rv = rintf(fmaf(p.m10, fx, fmaf(p.m11, fy, p.m12)));
  const float hi = (float)(C - 1);
  const bool in = ru >= 0.f && ru <= hi && rv >= 0.f && rv <= hi;
  const int ix = (int)(in ? ru : 0.f), iy = (int)(in ? rv : 0.f);
  off = ((p.y0 + iy) * Ws + p.x0 + (p.flip ? C - 1 - ix : ix)) * 3;
  return in;
}

struct AugNorm {
  float rescale;
  float mean[3], sd[3];
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// the three pixel-space values of output pixel (x, y) before any jitter
__device__ __forceinline__ void aug_load(const unsigned char* __restrict__ img, const AugSample& p, const AugNorm& nm, int C, int Ws, int x, int y,
                                         float val[3]) {
  int off;
  const bool in = aug_source(p, C, Ws, x, y, off);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = __fmul_rn((float)img[off + c], nm.rescale);
    val[c] = in ? v : nm.mean[c];
  }
}

// what output pixel (x, y) adds to the gray mean of the contrast step: the image as it stands then (brightened already when brightness
// comes first)
__device__ __forceinline__ float aug_gray_px(const unsigned char* __restrict__ img, const AugSample& p, const AugNorm& nm, int C, int Ws, int x,
                                             int y, bool bright_first) {
  float v[3];
  aug_load(img, p, nm, C, Ws, x, y, v);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = bright_first ? clamp01(p.fb * v[c]) : v[c];      // selects, not branches: the loads of a run stay together
  return 0.2989f * v[0] + 0.587f * v[1] + 0.114f * v[2];
}

// the three normalised values of output pixel (x, y).  JIT = false is the expression of bicubic_v_kernel (embed.hip), one fma and one
// IEEE division, so identity parameters give that kernel's bits; a fill pixel is then exactly 0.
template <bool JIT>
__device__ __forceinline__ void aug_pixel(const unsigned char* __restrict__ img, const AugSample& p, const AugNorm& nm, int C, int Ws, int x, int y,
                                          bool do_b, bool do_c, float blend, float out[3]) {
  if constexpr (!JIT) {
    int off;
    const bool in = aug_source(p, C, Ws, x, y, off);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = __fmaf_rn((float)img[off + c], nm.rescale, -nm.mean[c]) / nm.sd[c];
      out[c] = in ? v : 0.f;
    }
  } else {
    float v[3];
    aug_load(img, p, nm, C, Ws, x, y, v);
    const bool b_first = do_b && !p.order, b_last = do_b && p.order;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float t = v[c];
      t = b_first ? clamp01(p.fb * t) : t;                   // an operation that is off leaves t as it is
      t = do_c ? clamp01(fmaf(p.fc, t, blend)) : t;
      t = b_last ? clamp01(p.fb * t) : t;
      out[c] = __fsub_rn(t, nm.mean[c]) / nm.sd[c];
    }
  }
}

template <bool JIT>
__device__ __forceinline__ void aug_store_pass(const unsigned char* __restrict__ img, bf16_t* __restrict__ dst, const AugSample& p, const AugNorm& nm,
                                               int C, int Ws, bool do_b, bool do_c, float blend) {
  const int nr = C >> 3, tail0 = nr << 3, tcols = C - tail0;
  const long long plane = (long long)C * C;
  const bool vec = tcols == 0;                               // rows of the planes start on 16 bytes iff C % 8 == 0
  for (int idx = threadIdx.x; idx < C * nr; idx += AUG_THREADS) {
    const int y = idx / nr, x8 = (idx - y * nr) << 3;
    float o[3][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t[3];
      aug_pixel<JIT>(img, p, nm, C, Ws, x8 + e, y, do_b, do_c, blend, t);
      o[0][e] = t[0]; o[1][e] = t[1]; o[2][e] = t[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bf16_t* row = dst + c * plane + (long long)y * C + x8;
      if (vec) {
        *(uint4*)row = make_uint4(pack2bf(o[c][0], o[c][1]), pack2bf(o[c][2], o[c][3]), pack2bf(o[c][4], o[c][5]), pack2bf(o[c][6], o[c][7]));
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) row[e] = f2bf(o[c][e]);
      }
    }
  }
  for (int idx = threadIdx.x; idx < C * tcols; idx += AUG_THREADS) {      // columns beyond the last multiple of 8
    const int y = idx / tcols, x = tail0 + (idx - y * tcols);
    float t[3];
    aug_pixel<JIT>(img, p, nm, C, Ws, x, y, do_b, do_c, blend, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * plane + (long long)y * C + x] = f2bf(t[c]);
  }
}

__global__ __launch_bounds__(AUG_THREADS) void augment_apply_kernel(const unsigned char* __restrict__ src, const float* __restrict__ params,
                                                                    bf16_t* __restrict__ dst, int Hs, int Ws, int C, AugNorm nm) {
  __shared__ float s_wave[AUG_WAVES];
  const int b = blockIdx.x;
  const float* r = params + (long long)b * AUG_REC;
  AugSample p;
  p.m00 = r[0]; p.m01 = r[1]; p.m02 = r[2]; p.m10 = r[3]; p.m11 = r[4]; p.m12 = r[5];
  p.fb = r[6]; p.fc = r[7];
  p.order = r[8] != 0.f; p.flip = r[9] != 0.f;
  // the crop box goes inside the source whatever the record says (fmaxf / fminf drop a NaN)
  p.x0 = (int)fminf(fmaxf(r[14], 0.f), (float)(Ws - C));
  p.y0 = (int)fminf(fmaxf(r[15], 0.f), (float)(Hs - C));
  const unsigned char* img = src + (long long)b * Hs * Ws * 3;
  bf16_t* out = dst + (long long)b * 3 * C * C;
  const bool do_b = p.fb != 1.f, do_c = p.fc != 1.f;         // uniform over the workgroup
  if (!do_b && !do_c) {
    aug_store_pass<false>(img, out, p, nm, C, Ws, false, false, 0.f);
    return;
  }
  float blend = 0.f;                                          // (1 - fc) x the gray mean
  if (do_c) {
    // first pass: the gray mean.  Per-lane sums over the lane's runs and tail pixels in the order of the second pass, butterfly over the
    // wave, the waves' sums added in wave order: the same bits every run
    const bool bright_first = do_b && !p.order;
    const int nr = C >> 3, tail0 = nr << 3, tcols = C - tail0;
    float s = 0.f;
    for (int idx = threadIdx.x; idx < C * nr; idx += AUG_THREADS) {
      const int y = idx / nr, x8 = (idx - y * nr) << 3;
      float g[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = aug_gray_px(img, p, nm, C, Ws, x8 + e, y, bright_first);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += g[e];
    }
    for (int idx = threadIdx.x; idx < C * tcols; idx += AUG_THREADS) {
      const int y = idx / tcols;
      s += aug_gray_px(img, p, nm, C, Ws, tail0 + (idx - y * tcols), y, bright_first);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < AUG_WAVES; ++w) t += s_wave[w];
    blend = (1.f - p.fc) * (t / (float)(C * C));
  }
  aug_store_pass<true>(img, out, p, nm, C, Ws, do_b, do_c, blend);
}

extern "C" int medmoe_augment_apply(const void* src_u8, const float* params, void* dst, int B, int Hs, int Ws, int C, float rescale,
                                    const float* mean3, const float* std3, hipStream_t stream) {
  if (!src_u8 || !params || !dst || !mean3 || !std3) return MM_ERR_ARG;
  if (B <= 0 || C <= 0 || Hs <= 0 || Ws <= 0 || C > min(Hs, Ws)) return MM_ERR_SHAPE;
  if ((long long)Hs * Ws * 3 >= (1ll << 31) || (long long)C * C >= (1ll << 30)) return MM_ERR_SHAPE;      // int offsets within an image
  if ((uintptr_t)dst & 15) return MM_ERR_ARG;                // 16-byte stores
  AugNorm nm;
  nm.rescale = rescale;
  for (int c = 0; c < 3; ++c) {
    if (!(std3[c] > 0.f)) return MM_ERR_ARG;
    nm.mean[c] = mean3[c]; nm.sd[c] = std3[c];
  }
  hipLaunchKernelGGL(augment_apply_kernel, dim3(B), dim3(AUG_THREADS), 0, stream, (const unsigned char*)src_u8, params, (bf16_t*)dst, Hs, Ws, C, nm);
  return mm_check_launch();
}
