// Dropout of the trainable text tower (BERT's hidden_dropout_prob / attention_probs_dropout_prob).  The keep mask is the pure function
// of (seed, step, site, element) of philox.h: every kernel here regenerates it in registers, none stores it (medmoe_dropout_mask writes
// it out for tests only).
//
//   medmoe_dropout_mask                the keep mask as bytes (tests, debugging)
//   medmoe_dropout_apply               y = keep * x / (1 - p): the embedding site's forward, every hidden site's backward
//   medmoe_dropout_add_layernorm_fwd   x1 = residual + keep * z / (1 - p), y = LayerNorm(x1): the two post-norm sites of a block in one
//                                      launch (layout and statistics of layernorm_fwd, so medmoe_layernorm_bwd runs on x1 unchanged)
//   medmoe_drop_path_scales            stochastic depth of the image tower: the per-sample scales 0 | 1 / (1 - p) of every site of a step
//   medmoe_scale_add_layernorm_fwd     x1 = residual + scale[sample] * z, y = LayerNorm(x1): the per-sample sibling of the launch above
//   medmoe_attn_drop_fwd / _bwd        text-geometry attention (N <= 80 keys, head_dim 64, key mask) with dropout on the probabilities;
//                                      one workgroup per (batch, head), the backward is ONE kernel that reads qkv once
#include "common.h"
#include "philox.h"

#define HD 64

// ------------------------------------------------------------------------------------------
// mask export, elementwise apply
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned char* __restrict__ out, long long rows, int cols, int gpr, DropRng rng) {
  const long long n = rows * gpr;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
    const long long row = idx / gpr;
    const int c0 = (int)(idx - row * gpr) * 4;
    const uint32_t keep = drop_keep4(rng, (unsigned long long)idx);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < cols) out[row * cols + c0 + j] = (unsigned char)((keep >> j) & 1u);
  }
}

template <bool F32>
__global__ __launch_bounds__(256) void dropout_apply_kernel(const void* __restrict__ x, void* __restrict__ y, long long groups, DropRng rng) {
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < groups; idx += (long long)gridDim.x * 256) {
    const uint32_t keep = drop_keep4(rng, (unsigned long long)idx);
    if constexpr (F32) {
      const float4 v = ((const float4*)x)[idx];
      ((float4*)y)[idx] = make_float4(keep & 1u ? v.x * rng.scale : 0.f, keep & 2u ? v.y * rng.scale : 0.f,
                                      keep & 4u ? v.z * rng.scale : 0.f, keep & 8u ? v.w * rng.scale : 0.f);
    } else {
      const uint2 v = ((const uint2*)x)[idx];
      const float a = keep & 1u ? __uint_as_float(v.x << 16) * rng.scale : 0.f, b = keep & 2u ? __uint_as_float(v.x & 0xffff0000u) * rng.scale : 0.f;
      const float c = keep & 4u ? __uint_as_float(v.y << 16) * rng.scale : 0.f, d = keep & 8u ? __uint_as_float(v.y & 0xffff0000u) * rng.scale : 0.f;
      uint2 o; o.x = pack2bf(a, b); o.y = pack2bf(c, d);
      ((uint2*)y)[idx] = o;
    }
  }
}

extern "C" int medmoe_dropout_mask(unsigned char* out, long long rows, int cols, int cols_padded, long long seed, long long step, long long site,
                                   long long thresh, hipStream_t stream) {
  if (!out) return MM_ERR_ARG;
  if (rows <= 0 || cols <= 0 || cols_padded < cols || (cols_padded & 3)) return MM_ERR_SHAPE;
  const int gpr = cols_padded / 4;
  const long long n = rows * gpr;
  const int grid = (int)min((n + 255) / 256, (long long)256 * 16);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid), dim3(256), 0, stream, out, rows, cols, gpr, make_drop_rng(seed, step, site, thresh, 1.f));
  return mm_check_launch();
}

extern "C" int medmoe_dropout_apply(const void* x, void* y, long long rows, int cols, int is_f32, long long seed, long long step, long long site,
                                    long long thresh, float scale, hipStream_t stream) {
  if (!x || !y) return MM_ERR_ARG;
  if (rows <= 0 || cols <= 0 || (cols & 3)) return MM_ERR_SHAPE;
  const long long groups = rows * (cols / 4);
  const int grid = (int)min((groups + 255) / 256, (long long)256 * 16);
  const DropRng rng = make_drop_rng(seed, step, site, thresh, scale);
  if (is_f32) hipLaunchKernelGGL(dropout_apply_kernel<true>, dim3(grid), dim3(256), 0, stream, x, y, groups, rng);
  else hipLaunchKernelGGL(dropout_apply_kernel<false>, dim3(grid), dim3(256), 0, stream, x, y, groups, rng);
  return mm_check_launch();
}

// ------------------------------------------------------------------------------------------
// x1 = residual + keep * z / (1 - p);  y = LayerNorm(x1) (fp32 statistics of the bf16-rounded x1, as layernorm_fwd computes them on a
// stored x1).  One wave per row, 16-byte loads, the row stays in registers between the passes.
// ------------------------------------------------------------------------------------------
#define DLN_MAX_CHUNKS 4   // D <= 64 lanes * 8 * 4 = 2048
__global__ __launch_bounds__(256) void dropout_add_layernorm_fwd_kernel(const bf16_t* __restrict__ z, const bf16_t* __restrict__ res,
                                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                        bf16_t* __restrict__ x1, bf16_t* __restrict__ y,
                                                                        float* __restrict__ mean_out, float* __restrict__ rstd_out, int rows, int D,
                                                                        float eps, DropRng rng) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nchunk = D >> 3;
  const int gpr = D >> 2;
  for (int row = blockIdx.x * 4 + wid; row < rows; row += gridDim.x * 4) {
    const long long ro = (long long)row * D;
    float v[DLN_MAX_CHUNKS][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < DLN_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
      if (c < nchunk) {
        const uint4 zr = *(const uint4*)(z + ro + c * 8), rr = *(const uint4*)(res + ro + c * 8);
        const uint32_t zw[4] = {zr.x, zr.y, zr.z, zr.w}, rw[4] = {rr.x, rr.y, rr.z, rr.w};
        const unsigned long long g0 = (unsigned long long)row * gpr + 2 * c;
        const uint32_t keep = drop_keep4(rng, g0) | (drop_keep4(rng, g0 + 1) << 4);
        uint32_t pk[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float za = __uint_as_float(zw[e] << 16), zb = __uint_as_float(zw[e] & 0xffff0000u);
          const float ra = __uint_as_float(rw[e] << 16), rb = __uint_as_float(rw[e] & 0xffff0000u);
          const float xa = ra + ((keep >> (2 * e)) & 1u ? za * rng.scale : 0.f);
          const float xb = rb + ((keep >> (2 * e + 1)) & 1u ? zb * rng.scale : 0.f);
          pk[e] = pack2bf(xa, xb);
          v[i][2 * e] = __uint_as_float(pk[e] << 16);
          v[i][2 * e + 1] = __uint_as_float(pk[e] & 0xffff0000u);
          s += v[i][2 * e] + v[i][2 * e + 1];
        }
        *(uint4*)(x1 + ro + c * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
      }
    }
    const float mean = wave_sum(s) / (float)D;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < DLN_MAX_CHUNKS; ++i)
      if (lane + i * 64 < nchunk)
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; sq += d * d; }
    const float rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
#pragma unroll
    for (int i = 0; i < DLN_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        const float4 g0 = *(const float4*)(gamma + c * 8), g1 = *(const float4*)(gamma + c * 8 + 4);
        const float4 b0 = *(const float4*)(beta + c * 8), b1 = *(const float4*)(beta + c * 8 + 4);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * rstd * gg[e] + bb[e];
        *(uint4*)(y + ro + c * 8) = make_uint4(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7]));
      }
    }
  }
}

extern "C" int medmoe_dropout_add_layernorm_fwd(const void* z, const void* residual, const float* gamma, const float* beta, void* x1, void* y,
                                                float* mean, float* rstd, int rows, int D, float eps, long long seed, long long step,
                                                long long site, long long thresh, float scale, hipStream_t stream) {
  if (!z || !residual || !gamma || !beta || !x1 || !y || !mean || !rstd) return MM_ERR_ARG;
  if (rows <= 0 || D <= 0 || (D % 8) || D > 64 * 8 * DLN_MAX_CHUNKS) return MM_ERR_SHAPE;
  const int grid = min((rows + 3) / 4, 256 * 8);
  hipLaunchKernelGGL(dropout_add_layernorm_fwd_kernel, dim3(grid), dim3(256), 0, stream, (const bf16_t*)z, (const bf16_t*)residual, gamma, beta,
                     (bf16_t*)x1, (bf16_t*)y, mean, rstd, rows, D, eps, make_drop_rng(seed, step, site, thresh, scale));
  return mm_check_launch();
}

// ------------------------------------------------------------------------------------------
// Stochastic depth of the image tower (reference transformer.py:45-68: StochasticDepth(p_l, mode="row") on both branches of a pre-norm
// layer).  out[site][b] = 0 | 1 / (1 - p_site): sample b survives at site s iff word (sample0 + b) % 4 of group (sample0 + b) / 4 of
// site site0 + s is >= thresh_s - the bit medmoe_dropout_mask writes at (row 0, column sample0 + b).  The per-site thresholds and scales
// travel by value in the launch arguments (computed on the host from the probabilities, as ops.dropout_thresh computes them).
// ------------------------------------------------------------------------------------------
#define DP_MAX_SITES 128
struct DropPathSites {
  uint32_t thresh[DP_MAX_SITES];
  float scale[DP_MAX_SITES];
};

__global__ __launch_bounds__(256) void drop_path_scales_kernel(float* __restrict__ out, DropPathSites sites, int n_sites, int B,
                                                               unsigned long long sample0, DropRng rng, uint32_t site0) {
  const long long n = (long long)n_sites * B;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
    const int s = (int)(idx / B);
    const unsigned long long col = sample0 + (unsigned long long)(idx - (long long)s * B);
    DropRng r = rng;
    r.site = site0 + (uint32_t)s;
    const uint4 w = drop_words(r, col >> 2);
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
    out[idx] = ww[col & 3] >= sites.thresh[s] ? sites.scale[s] : 0.f;
  }
}

extern "C" int medmoe_drop_path_scales(float* out, const double* p_host, int n_sites, int B, long long sample0, long long seed, long long step,
                                       long long site0, hipStream_t stream) {
  if (!out || !p_host) return MM_ERR_ARG;
  if (n_sites <= 0 || n_sites > DP_MAX_SITES || B <= 0 || sample0 < 0) return MM_ERR_SHAPE;
  DropPathSites sites;
  for (int s = 0; s < DP_MAX_SITES; ++s) { sites.thresh[s] = 0u; sites.scale[s] = 1.f; }
  for (int s = 0; s < n_sites; ++s) {
    const double p = p_host[s];
    if (!(p >= 0.0 && p < 1.0)) return MM_ERR_ARG;
    sites.thresh[s] = (uint32_t)(unsigned long long)(p * 4294967296.0);      // floor(p * 2^32), exact in a double
    sites.scale[s] = (float)(1.0 / (1.0 - p));
  }
  const long long n = (long long)n_sites * B;
  const int grid = (int)min((n + 255) / 256, (long long)256 * 16);
  hipLaunchKernelGGL(drop_path_scales_kernel, dim3(grid), dim3(256), 0, stream, out, sites, n_sites, B, (unsigned long long)sample0,
                     make_drop_rng(seed, step, site0, 0, 1.f), (uint32_t)site0);
  return mm_check_launch();
}

// x1 = bf16(residual + scale[row / rows_per_sample] * z) (product and sum in fp32);  y = LayerNorm(x1) with the statistics of the
// bf16-rounded x1.  Geometry of dropout_add_layernorm_fwd_kernel.  A row whose scale is 0 COPIES residual: z is not loaded, so whatever
// it holds there (inf, nan) cannot reach x1.  The branch is uniform over the wave (one row per wave).
__global__ __launch_bounds__(256) void scale_add_layernorm_fwd_kernel(const bf16_t* __restrict__ z, const bf16_t* __restrict__ res,
                                                                      const float* __restrict__ scale, int rows_per_sample,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      bf16_t* __restrict__ x1, bf16_t* __restrict__ y,
                                                                      float* __restrict__ mean_out, float* __restrict__ rstd_out, int rows, int D,
                                                                      float eps) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nchunk = D >> 3;
  for (int row = blockIdx.x * 4 + wid; row < rows; row += gridDim.x * 4) {
    const long long ro = (long long)row * D;
    const float sc = scale[row / rows_per_sample];
    const bool kept = sc != 0.f;
    float v[DLN_MAX_CHUNKS][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < DLN_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
      if (c < nchunk) {
        const uint4 rr = *(const uint4*)(res + ro + c * 8);
        uint32_t pk[4] = {rr.x, rr.y, rr.z, rr.w};
        if (kept) {
          const uint4 zr = *(const uint4*)(z + ro + c * 8);
          const uint32_t zw[4] = {zr.x, zr.y, zr.z, zr.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float xa = __uint_as_float(pk[e] << 16) + sc * __uint_as_float(zw[e] << 16);
            const float xb = __uint_as_float(pk[e] & 0xffff0000u) + sc * __uint_as_float(zw[e] & 0xffff0000u);
            pk[e] = pack2bf(xa, xb);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[i][2 * e] = __uint_as_float(pk[e] << 16);
          v[i][2 * e + 1] = __uint_as_float(pk[e] & 0xffff0000u);
          s += v[i][2 * e] + v[i][2 * e + 1];
        }
        *(uint4*)(x1 + ro + c * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
      }
    }
    const float mean = wave_sum(s) / (float)D;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < DLN_MAX_CHUNKS; ++i)
      if (lane + i * 64 < nchunk)
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; sq += d * d; }
    const float rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
#pragma unroll
    for (int i = 0; i < DLN_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
        const float4 g0 = *(const float4*)(gamma + c * 8), g1 = *(const float4*)(gamma + c * 8 + 4);
        const float4 b0 = *(const float4*)(beta + c * 8), b1 = *(const float4*)(beta + c * 8 + 4);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * rstd * gg[e] + bb[e];
        *(uint4*)(y + ro + c * 8) = make_uint4(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7]));
      }
    }
  }
}

extern "C" int medmoe_scale_add_layernorm_fwd(const void* z, const void* residual, const float* scale, int rows_per_sample, const float* gamma,
                                              const float* beta, void* x1, void* y, float* mean, float* rstd, int rows, int D, float eps,
                                              hipStream_t stream) {
  if (!z || !residual || !scale || !gamma || !beta || !x1 || !y || !mean || !rstd) return MM_ERR_ARG;
  if (rows <= 0 || rows_per_sample <= 0 || (rows % rows_per_sample) || D <= 0 || (D % 8) || D > 64 * 8 * DLN_MAX_CHUNKS) return MM_ERR_SHAPE;
  const int grid = min((rows + 3) / 4, 256 * 8);
  hipLaunchKernelGGL(scale_add_layernorm_fwd_kernel, dim3(grid), dim3(256), 0, stream, (const bf16_t*)z, (const bf16_t*)residual, scale,
                     rows_per_sample, gamma, beta, (bf16_t*)x1, (bf16_t*)y, mean, rstd, rows, D, eps);
  return mm_check_launch();
}

// ------------------------------------------------------------------------------------------
// attention with dropout on the probabilities.  Geometry of the 5-tile resident kernels of attention.hip: up to 80 keys = 5 tiles of 16,
// row-major [96][64] bf16 LDS images with chunk ^= row & 7, score tiles computed TRANSPOSED (S^T = K Q^T: the accumulator's registers
// run over 4 consecutive keys of one query - exactly one Philox group - and are the B operand of the products that sum over keys).
// ------------------------------------------------------------------------------------------
#define DNKT 5                        // key / query tiles
#define DKS 3                         // 32-wide contraction steps over keys / queries
#define DROWS 96                      // rows of a row-major image (whole 32-row steps; rows >= N are copies of row N - 1)
#define DRM_BYTES (DROWS * 128)
#define DNKP 80
#define DKEEP_LD 24                   // keep nibbles per query row in LDS (20 groups of 4 keys, padded)

// [rows][64] bf16 -> LDS rows of 128 B with chunk ^= row & 7; every thread issues all its loads before the first LDS write
__device__ __forceinline__ void fill_rowmajor96(char* lds, const bf16_t* src, long long row_stride, int n_valid, int tid) {
  constexpr int CNT = DROWS * 8, PER = CNT / 256;
  uint4 v[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int idx = tid + i * 256;
    const int row = idx >> 3, c = idx & 7;
    v[i] = *(const uint4*)(src + (long long)min(row, n_valid - 1) * row_stride + c * 8);
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int idx = tid + i * 256;
    const int row = idx >> 3, c = idx & 7;
    *(uint4*)(lds + row * 128 + ((c ^ (row & 7)) << 4)) = v[i];
  }
}

// 8 contiguous elements (chunk) of a row of a swizzled row-major image: an MFMA operand whose contraction index is the column
__device__ __forceinline__ bf16x8_t row_frag(const char* img, int row, int chunk) {
  return *(const bf16x8_t*)(img + row * 128 + ((chunk ^ (row & 7)) << 4));
}

// MFMA operand whose contraction index is the ROW of a swizzled row-major image: two ds_read_b64_tr_b16; EXEC must be all ones.
// Elements 0..3 = rows row0 + 4 * (lane >> 4) + {0..3}, elements 4..7 = the same rows + 16; column = col0 + (lane & 15).
__device__ __forceinline__ bf16x8_t tr_frag(const char* img, int row0, int col0, int lane) {
  const int q = (lane & 15) >> 2, pp = lane & 3;
  const int ra = row0 + 4 * (lane >> 4) + q, rb = ra + 16;
  const int col = col0 + 4 * pp;
  const int ch = col >> 3, within = (col & 7) << 1;
  const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4_t*)(img + ra * 128 + ((ch ^ (ra & 7)) << 4) + within));
  const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4_t*)(img + rb * 128 + ((ch ^ (rb & 7)) << 4) + within));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ bf16x8_t pack_frag(const f32x4_t& a, const f32x4_t& b) {
  uint4 v;
  v.x = pack2bf(a[0], a[1]); v.y = pack2bf(a[2], a[3]);
  v.z = pack2bf(b[0], b[1]); v.w = pack2bf(b[2], b[3]);
  return __builtin_bit_cast(bf16x8_t, v);
}

// Forward.  A wave owns 16 query rows and holds their 5 score tiles; softmax over the unmasked keys (lse is of the UNDROPPED softmax),
// then the dropped keys' probabilities are zeroed and 1 / (1 - p) rides on the 1 / rowsum of the 16 output values.
__global__ __launch_bounds__(256, 2) void attn_drop_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, float* __restrict__ lse,
                                                               const unsigned char* __restrict__ key_mask, int N, int H, float scale,
                                                               DropRng rng) {
  __shared__ __attribute__((aligned(16))) char smem[2 * DRM_BYTES + DNKP * 4];
  char* sK = smem;
  char* sV = smem + DRM_BYTES;
  float* sMask = (float*)(smem + 2 * DRM_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int D = H * HD;
  const long long rs = 3LL * D;
  const bf16_t* base = qkv + (long long)b * N * rs + h * HD;

  fill_rowmajor96(sK, base + D, rs, N, tid);
  fill_rowmajor96(sV, base + 2 * D, rs, N, tid);
  for (int k = tid; k < DNKP; k += 256)
    sMask[k] = (k < N && (!key_mask || key_mask[(long long)b * N + k])) ? 0.f : -INFINITY;
  __syncthreads();

  const int fr = lane & 15, g = lane >> 4;
  const int nqb = (N + 15) >> 4;
  const int gpr = (N + 3) >> 2;                              // groups of 4 keys per query row (key axis padded to a multiple of 4)
  const float c2 = scale * 1.44269504088896f;
  for (int qb = wid; qb < nqb; qb += 4) {
    const int q = qb * 16 + fr;
    const int qc = min(q, N - 1);
    bf16x8_t qf[2];
    qf[0] = *(const bf16x8_t*)(base + (long long)qc * rs + g * 8);
    qf[1] = *(const bf16x8_t*)(base + (long long)qc * rs + (4 + g) * 8);
    f32x4_t s[DNKT + 1];
    float bm = -INFINITY;
#pragma unroll
    for (int u = 0; u < DNKT; ++u) {
      s[u] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) s[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, u * 16 + fr, ks * 4 + g), qf[ks], s[u], 0, 0, 0);
      const float4 mk = *(const float4*)(sMask + u * 16 + g * 4);
      s[u][0] = s[u][0] * c2 + mk.x; s[u][1] = s[u][1] * c2 + mk.y; s[u][2] = s[u][2] * c2 + mk.z; s[u][3] = s[u][3] * c2 + mk.w;
      bm = fmaxf(fmaxf(bm, fmaxf(s[u][0], s[u][1])), fmaxf(s[u][2], s[u][3]));
    }
    s[DNKT] = (f32x4_t){0.f, 0.f, 0.f, 0.f};                 // the missing sixth tile of the last 32-key step
    bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float ms = (bm == -INFINITY) ? 0.f : bm;           // nothing but masked keys: 2^(-inf - 0) = 0 instead of nan
    float l = 0.f;
    const unsigned long long grow = ((unsigned long long)(b * H + h) * N + qc) * gpr;
#pragma unroll
    for (int u = 0; u < DNKT; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) s[u][r] = __builtin_amdgcn_exp2f(s[u][r] - ms);
      l += (s[u][0] + s[u][1]) + (s[u][2] + s[u][3]);
      const int kg = u * 4 + g;
      const uint32_t keep = kg < gpr ? drop_keep4(rng, grow + kg) : 0u;    // groups past the padded key axis hold masked keys only (p = 0)
#pragma unroll
      for (int r = 0; r < 4; ++r) s[u][r] = (keep >> r) & 1u ? s[u][r] : 0.f;
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    f32x4_t o[4];
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) {
      o[nd] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < DKS; ++t) {                        // UNNORMALISED probabilities (<= 1), dropped ones zero
        const bf16x8_t pf = pack_frag(s[2 * t], s[2 * t + 1]);
        const bf16x8_t vf = tr_frag(sV, t * 32, nd * 16, lane);
        o[nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[nd], 0, 0, 0);
      }
    }
    const float inv = (l > 0.f ? 1.f / l : 0.f) * rng.scale;
    if (q < N) {
      if (g == 0) lse[((long long)b * H + h) * N + q] = (ms + __log2f(l)) * 0.693147180559945f;
#pragma unroll
      for (int nd = 0; nd < 4; ++nd) {
        const f32x4_t v = o[nd] * inv;
        uint2 pk; pk.x = pack2bf(v[0], v[1]); pk.y = pack2bf(v[2], v[3]);
        *(uint2*)(out + ((long long)b * N + q) * D + h * HD + nd * 16 + g * 4) = pk;
      }
    }
  }
}

// Backward, one kernel: Q, K, V and dO of the (batch, head) are read once into LDS.
//   phase A (a wave owns 16 queries): delta = rowsum(dO * out), P from the saved lse, the keep bits regenerated in registers (and left
//            in LDS as one nibble per (query, 4 keys) for phase B), dP = keep * (dO V^T) / (1 - p), dS = P (dP - delta), dQ = scale dS K
//   phase B (a wave owns 16 keys): the same tiles in the [query][key] orientation, dV = P~^T dO with P~ = keep * P / (1 - p),
//            dK = scale dS^T Q
__global__ __launch_bounds__(256, 2) void attn_drop_bwd_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o,
                                                               const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                               const unsigned char* __restrict__ key_mask, bf16_t* __restrict__ dqkv,
                                                               float* __restrict__ delta, int N, int H, float scale, DropRng rng) {
  __shared__ __attribute__((aligned(16))) char smem[4 * DRM_BYTES + 3 * DNKP * 4 + DNKP * DKEEP_LD];
  char* sQ = smem;
  char* sK = smem + DRM_BYTES;
  char* sV = smem + 2 * DRM_BYTES;
  char* sDO = smem + 3 * DRM_BYTES;
  float* sMask = (float*)(smem + 4 * DRM_BYTES);
  float* sLse = sMask + DNKP;
  float* sDelta = sLse + DNKP;
  unsigned char* sKeep = (unsigned char*)(sDelta + DNKP);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int D = H * HD;
  const long long rs = 3LL * D;
  const bf16_t* base = qkv + (long long)b * N * rs + h * HD;
  const bf16_t* obase = o + (long long)b * N * D + h * HD;
  const bf16_t* dobase = dout + (long long)b * N * D + h * HD;
  const long long bh = (long long)b * H + h;

  fill_rowmajor96(sQ, base, rs, N, tid);
  fill_rowmajor96(sK, base + D, rs, N, tid);
  fill_rowmajor96(sV, base + 2 * D, rs, N, tid);
  fill_rowmajor96(sDO, dobase, D, N, tid);
  for (int k = tid; k < DNKP; k += 256) {
    sMask[k] = (k < N && (!key_mask || key_mask[(long long)b * N + k])) ? 0.f : -INFINITY;
    sLse[k] = INFINITY;                                      // exp2 domain; query rows >= N keep it: p = 0
    sDelta[k] = 0.f;
  }
  for (int k = tid; k < DNKP * DKEEP_LD / 4; k += 256) ((uint32_t*)sKeep)[k] = 0u;
  __syncthreads();

  const int fr = lane & 15, g = lane >> 4;
  const int nb = (N + 15) >> 4;
  const int gpr = (N + 3) >> 2;
  const float c2 = scale * 1.44269504088896f;

  // ---- phase A ----
  for (int qb = wid; qb < nb; qb += 4) {
    const int q = qb * 16 + fr;
    const int qc = min(q, N - 1);
    bf16x8_t qf[2], dof[2];
    float dl = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = row_frag(sQ, q, ks * 4 + g);
      dof[ks] = row_frag(sDO, q, ks * 4 + g);
      const bf16x8_t of = *(const bf16x8_t*)(obase + (long long)qc * D + (ks * 4 + g) * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) dl += (float)dof[ks][e] * (float)of[e];
    }
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    const float L2 = lse[bh * N + qc] * 1.44269504088896f;   // p = 2^(s c2 - L log2 e)
    if (g == 0 && q < N) {
      delta[bh * N + q] = dl;
      sDelta[q] = dl;
      sLse[q] = L2;
    }
    const unsigned long long grow = ((unsigned long long)bh * N + qc) * gpr;
    f32x4_t acc[4];
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) acc[nd] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < DKS; ++t) {
      f32x4_t ds[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int kt = 2 * t + u;
        ds[u] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        if (kt < DNKT) {
          f32x4_t s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, kt * 16 + fr, ks * 4 + g), qf[ks], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sV, kt * 16 + fr, ks * 4 + g), dof[ks], dp, 0, 0, 0);
          }
          const int kg = kt * 4 + g;
          const uint32_t keep = kg < gpr ? drop_keep4(rng, grow + kg) : 0u;
          if (q < N) sKeep[q * DKEEP_LD + kg] = (unsigned char)keep;
          const float4 mk = *(const float4*)(sMask + kt * 16 + g * 4);
          const float mkv[4] = {mk.x, mk.y, mk.z, mk.w};
          // dS / scale = p (dP - delta): the softmax scale is applied once, to the 16 accumulated dQ values
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(s[r] * c2 + (mkv[r] - L2));
            ds[u][r] = p * (((keep >> r) & 1u ? dp[r] * rng.scale : 0.f) - dl);
          }
        }
      }
      const bf16x8_t dsf = pack_frag(ds[0], ds[1]);
#pragma unroll
      for (int nd = 0; nd < 4; ++nd) acc[nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sK, t * 32, nd * 16, lane), dsf, acc[nd], 0, 0, 0);
    }
    if (q < N) {
#pragma unroll
      for (int nd = 0; nd < 4; ++nd) {
        const f32x4_t v = acc[nd] * scale;
        uint2 pk; pk.x = pack2bf(v[0], v[1]); pk.y = pack2bf(v[2], v[3]);
        *(uint2*)(dqkv + ((long long)b * N + q) * rs + h * HD + nd * 16 + g * 4) = pk;
      }
    }
  }
  __syncthreads();                                           // sLse, sDelta, sKeep of every query block are in LDS

  // ---- phase B ----
  for (int kb = wid; kb < nb; kb += 4) {
    const int key = kb * 16 + fr;
    bf16x8_t kf[2], vf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) { kf[ks] = row_frag(sK, key, ks * 4 + g); vf[ks] = row_frag(sV, key, ks * 4 + g); }
    const float mk = sMask[key];
    const int kbyte = key >> 2, kbit = key & 3;
    f32x4_t dk[4], dv[4];
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) { dk[nd] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; dv[nd] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int t = 0; t < DKS; ++t) {
      f32x4_t pp[2], dss[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int qt = 2 * t + u;
        pp[u] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        dss[u] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        if (qt < DNKT) {
          // S[q][key] tile: rows q = qt * 16 + 4 g + r (registers), column key = lane & 15
          f32x4_t s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sQ, qt * 16 + fr, ks * 4 + g), kf[ks], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sDO, qt * 16 + fr, ks * 4 + g), vf[ks], dp, 0, 0, 0);
          }
          const float4 L4 = *(const float4*)(sLse + qt * 16 + g * 4);
          const float4 D4 = *(const float4*)(sDelta + qt * 16 + g * 4);
          const float Lv[4] = {L4.x, L4.y, L4.z, L4.w}, Dv[4] = {D4.x, D4.y, D4.z, D4.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool keep = (sKeep[(qt * 16 + g * 4 + r) * DKEEP_LD + kbyte] >> kbit) & 1;
            const float p = __builtin_amdgcn_exp2f(s[r] * c2 + (mk - Lv[r]));
            pp[u][r] = keep ? p * rng.scale : 0.f;
            dss[u][r] = p * ((keep ? dp[r] * rng.scale : 0.f) - Dv[r]);
          }
        }
      }
      const bf16x8_t pf = pack_frag(pp[0], pp[1]);
      const bf16x8_t dsf = pack_frag(dss[0], dss[1]);
#pragma unroll
      for (int nd = 0; nd < 4; ++nd) {
        dv[nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sDO, t * 32, nd * 16, lane), pf, dv[nd], 0, 0, 0);
        dk[nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sQ, t * 32, nd * 16, lane), dsf, dk[nd], 0, 0, 0);
      }
    }
    if (key < N) {
      bf16_t* row = dqkv + ((long long)b * N + key) * rs + h * HD;
#pragma unroll
      for (int nd = 0; nd < 4; ++nd) {
        const f32x4_t kv = dk[nd] * scale;
        uint2 pk; pk.x = pack2bf(kv[0], kv[1]); pk.y = pack2bf(kv[2], kv[3]);
        *(uint2*)(row + D + nd * 16 + g * 4) = pk;
        pk.x = pack2bf(dv[nd][0], dv[nd][1]); pk.y = pack2bf(dv[nd][2], dv[nd][3]);
        *(uint2*)(row + 2 * D + nd * 16 + g * 4) = pk;
      }
    }
  }
}

static int attn_drop_shape(int B, int N, int H, int head_dim) {
  if (head_dim != HD || B <= 0 || H <= 0 || N <= 0 || N > DNKP) return MM_ERR_SHAPE;
  return MM_OK;
}

extern "C" int medmoe_attn_drop_fwd(const void* qkv, void* out, float* lse, const unsigned char* key_mask, int B, int N, int H, int head_dim,
                                    long long seed, long long step, long long site, long long thresh, float scale, hipStream_t stream) {
  if (!qkv || !out || !lse) return MM_ERR_ARG;
  if (attn_drop_shape(B, N, H, head_dim) != MM_OK) return MM_ERR_SHAPE;
  hipLaunchKernelGGL(attn_drop_fwd_kernel, dim3(B * H), dim3(256), 0, stream, (const bf16_t*)qkv, (bf16_t*)out, lse, key_mask, N, H, 0.125f,
                     make_drop_rng(seed, step, site, thresh, scale));
  return mm_check_launch();
}

extern "C" int medmoe_attn_drop_bwd(const void* qkv, const void* out, const void* dout, const float* lse, const unsigned char* key_mask, void* dqkv,
                                    float* delta, int B, int N, int H, int head_dim, long long seed, long long step, long long site,
                                    long long thresh, float scale, hipStream_t stream) {
  if (!qkv || !out || !dout || !lse || !dqkv || !delta) return MM_ERR_ARG;
  if (attn_drop_shape(B, N, H, head_dim) != MM_OK) return MM_ERR_SHAPE;
  hipLaunchKernelGGL(attn_drop_bwd_kernel, dim3(B * H), dim3(256), 0, stream, (const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse,
                     key_mask, (bf16_t*)dqkv, delta, N, H, 0.125f, make_drop_rng(seed, step, site, thresh, scale));
  return mm_check_launch();
}
