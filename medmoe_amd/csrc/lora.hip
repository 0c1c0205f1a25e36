// LoRA adapters on the text tower's fused q / k / v projection (frozen base, trainable rank-r side path).
//
// Conventions: X [M][D] bf16 is a layer's input, qkv [M][ldq] the fused projection's output row [q | k | v]; target t of n_t (query / key /
// value in any subset) owns the D columns from c_t on.  Adapters are stored PADDED to rank 16 (the arena keeps the pad rows of A and the pad
// columns of B at exactly zero: they receive exactly zero gradient), stacked over the targets:
//   A   [n_t*16][D]   (lora_A, peft's [r, D])          At  [D][n_t*16]   its transpose
//   Bw  [n_t*D][16]   (lora_B, peft's [D, r])          Bt  [16][n_t*D]   its transpose
// so that every MFMA operand below is read with the contraction index contiguous.  s = lora_alpha / r.
// Dropout: Xd = keep * X * scale with the keep mask of philox.h over the [M][D] array of site 4*layer+3; keep * X is formed exactly (dropped
// elements zeroed) and `scale` multiplies the fp32 accumulator, so no operand is rounded a second time.  thresh = 0 means no dropout.
//
//   medmoe_lora_fwd        U = Xd A^T (bf16, stored: the backward needs it), qkv[:, c_t:c_t+D] += s U_t B_t^T.  One launch, X read once, U goes
//                          from the first product's accumulators straight into the second product's operand registers (no LDS, no HBM).
//   medmoe_lora_bwd_dx     dU_t = s dqkv_t B_t (bf16, stored), dy += keep * scale * (dU A)   (dy = nullptr: layer 0, nothing below trains)
//   medmoe_lora_bwd_wgrad  gB_t += s dqkv_t^T U_t, gA_t += dU_t^T Xd: per 256-row chunk partial sums in a scratch buffer, then a second
//                          kernel adds them up in chunk order into the fp32 gradients.  No atomics: two runs are bit-identical.
//   medmoe_lora_merge      W[c_t + d][:] = bf16(W + s B_t A_t) on a copy of the base weight (export, evaluation)
#include "common.h"
#include "philox.h"

#define LR 16          // stored rank
#define WG_ROWS 256    // rows per chunk of the weight-gradient kernel
#define WG_COLS 128    // columns per workgroup of it (4 waves x 2 tiles of 16)
#define WG_PITCH (WG_COLS + 2)   // 65 dwords: the 8-row stride of an operand fragment's lane groups lands 8 banks apart

struct LoraCols { int c[3]; };

__device__ __forceinline__ f32x4_t mfma16(uint2 a, uint2 b, f32x4_t c) {      // 16x16x16: lane holds k = 4 (lane >> 4) + j of row / column lane & 15
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(short4_t, a), __builtin_bit_cast(short4_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4_t mfma32(uint4 a, uint4 b, f32x4_t c) {      // 16x16x32: lane holds k = 8 (lane >> 4) + j
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
// a dword of two bf16 with the dropped ones zeroed: bit 0 of `keep` = the low element
__device__ __forceinline__ uint32_t keep2(uint32_t w, uint32_t keep) { return w & ((keep & 1u ? 0xffffu : 0u) | (keep & 2u ? 0xffff0000u : 0u)); }
// 8 consecutive elements of row `row` from column `col` (col % 8 == 0) of the [rows][4 * gpr] mask array
__device__ __forceinline__ uint4 keep8(uint4 v, const DropRng& rng, long long row, int gpr, int col) {
  const unsigned long long g0 = (unsigned long long)row * gpr + (col >> 2);
  const uint32_t k = drop_keep4(rng, g0) | (drop_keep4(rng, g0 + 1) << 4);
  return make_uint4(keep2(v.x, k), keep2(v.y, k >> 2), keep2(v.z, k >> 4), keep2(v.w, k >> 6));
}

// ------------------------------------------------------------------------------------------
// forward.  One wave per 16 rows.  First product transposed (A-operand = adapter rows, B-operand = X): the accumulator then holds, for
// row m = lane & 15, the 4 consecutive ranks 4 (lane >> 4) .. + 3 - one 8-byte store of U, and exactly the B-operand fragment of the
// 16x16x16 MFMA of the second product.  Second product transposed too, with the rows of B_t taken in the order that leaves every lane 16
// consecutive columns of its row (4 tiles): a 16-lane group covers 128 contiguous bytes of a qkv row.
// ------------------------------------------------------------------------------------------
template <int NT, bool DROP>
__global__ __launch_bounds__(256) void lora_fwd_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bw,
                                                       bf16_t* __restrict__ U, bf16_t* __restrict__ qkv, int ldq, int M, int D, LoraCols cols,
                                                       float s, DropRng rng, const int* __restrict__ rows_dev) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const long long row0 = ((long long)blockIdx.x * 4 + wid) * 16;
  if (rows_dev) M = min(M, *rows_dev);             // the *_rows entry points: the first *rows_dev rows only (packed variable-length batches)
  if (row0 >= M) return;
  const long long m = row0 + r;
  const bool mok = m < M;
  const bf16_t* xrow = X + (mok ? m : (long long)M - 1) * D;
  const int gpr = D >> 2;
  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < D; k0 += 32) {
    const int k = k0 + 8 * g;
    uint4 xv = mok ? *(const uint4*)(xrow + k) : make_uint4(0, 0, 0, 0);
    if constexpr (DROP) xv = keep8(xv, rng, m, gpr, k);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma32(*(const uint4*)(A + (long long)(t * LR + r) * D + k), xv, acc[t]);
  }
  uint2 ub[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if constexpr (DROP) acc[t] *= rng.scale;
    ub[t] = make_uint2(pack2bf(acc[t][0], acc[t][1]), pack2bf(acc[t][2], acc[t][3]));
    if (mok) *(uint2*)(U + m * (NT * LR) + t * LR + 4 * g) = ub[t];
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const bf16_t* bt = Bw + (long long)t * D * LR;
    for (int n0 = 0; n0 < D; n0 += 64) {
      f32x4_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = n0 + (r >> 2) * 16 + j * 4 + (r & 3);
        o[j] = mfma16(*(const uint2*)(bt + (long long)d * LR + 4 * g), ub[t], (f32x4_t){0.f, 0.f, 0.f, 0.f});
      }
      if (mok) {
        bf16_t* p = qkv + m * ldq + cols.c[t] + n0 + g * 16;
        const uint4 q0 = *(const uint4*)p, q1 = *(const uint4*)(p + 8);
        const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        uint32_t y[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float lo = __uint_as_float(w[e] << 16) + s * o[e >> 1][(2 * e) & 3];
          const float hi = __uint_as_float(w[e] & 0xffff0000u) + s * o[e >> 1][(2 * e + 1) & 3];
          y[e] = pack2bf(lo, hi);
        }
        *(uint4*)p = make_uint4(y[0], y[1], y[2], y[3]);
        *(uint4*)(p + 8) = make_uint4(y[4], y[5], y[6], y[7]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// backward, first launch: dU and the LoRA term of dX.  Same shape as the forward: dU^T = B_t^T dqkv_t^T in the accumulators is the operand of
// dX^T = A^T dU^T.
// ------------------------------------------------------------------------------------------
template <int NT, bool DROP>
__global__ __launch_bounds__(256) void lora_bwd_dx_kernel(const bf16_t* __restrict__ dqkv, int ldq, const bf16_t* __restrict__ Bt,
                                                          const bf16_t* __restrict__ At, bf16_t* __restrict__ dU, bf16_t* __restrict__ dy, int M,
                                                          int D, LoraCols cols, float s, DropRng rng, const int* __restrict__ rows_dev) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const long long row0 = ((long long)blockIdx.x * 4 + wid) * 16;
  if (rows_dev) M = min(M, *rows_dev);
  if (row0 >= M) return;
  const long long m = row0 + r;
  const bool mok = m < M;
  const bf16_t* grow = dqkv + (mok ? m : (long long)M - 1) * ldq;
  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < D; k0 += 32) {
    const int k = k0 + 8 * g;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint4 gv = mok ? *(const uint4*)(grow + cols.c[t] + k) : make_uint4(0, 0, 0, 0);
      acc[t] = mfma32(*(const uint4*)(Bt + (long long)r * (NT * D) + (long long)t * D + k), gv, acc[t]);
    }
  }
  uint2 du[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] *= s;
    du[t] = make_uint2(pack2bf(acc[t][0], acc[t][1]), pack2bf(acc[t][2], acc[t][3]));
    if (mok) *(uint2*)(dU + m * (NT * LR) + t * LR + 4 * g) = du[t];
  }
  if (!dy) return;
  const int gpr = D >> 2;
  for (int n0 = 0; n0 < D; n0 += 64) {
    f32x4_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int d = n0 + (r >> 2) * 16 + j * 4 + (r & 3);
      o[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NT; ++t) o[j] = mfma16(*(const uint2*)(At + (long long)d * (NT * LR) + t * LR + 4 * g), du[t], o[j]);
    }
    if (mok) {
      const int c = n0 + g * 16;
      bf16_t* p = dy + m * D + c;
      const uint4 q0 = *(const uint4*)p, q1 = *(const uint4*)(p + 8);
      const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
      uint32_t keep = 0xffffu;
      float sc = 1.f;
      if constexpr (DROP) {
        const unsigned long long g0 = (unsigned long long)m * gpr + (c >> 2);
        keep = drop_keep4(rng, g0) | (drop_keep4(rng, g0 + 1) << 4) | (drop_keep4(rng, g0 + 2) << 8) | (drop_keep4(rng, g0 + 3) << 12);
        sc = rng.scale;
      }
      uint32_t y[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = (keep >> (2 * e)) & 1u ? sc * o[e >> 1][(2 * e) & 3] : 0.f;
        const float b = (keep >> (2 * e + 1)) & 1u ? sc * o[e >> 1][(2 * e + 1) & 3] : 0.f;
        y[e] = pack2bf(__uint_as_float(w[e] << 16) + a, __uint_as_float(w[e] & 0xffff0000u) + b);
      }
      *(uint4*)p = make_uint4(y[0], y[1], y[2], y[3]);
      *(uint4*)(p + 8) = make_uint4(y[4], y[5], y[6], y[7]);
    }
  }
}

// ------------------------------------------------------------------------------------------
// backward, second launch: the adapter gradients.  Both are sums over the rows, the slow axis of every operand in memory: a workgroup
// brings 32 rows x 128 columns of dqkv_t (each target) and of keep * X into LDS with 16-byte loads, the 32 rows of U and dU next to them,
// and the waves read their operand fragments column-wise.  part[chunk][t][0][rank][d] = s sum_m U[m][t, rank] dqkv_t[m][d] (gB_t
// transposed), part[chunk][t][1][rank][d] = scale sum_m dU[m][t, rank] keep X[m][d] (gA_t).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 lds_col8(const bf16_t* p, int pitch) {       // 8 consecutive rows of one column
  uint32_t w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = (uint32_t)p[(2 * e) * pitch] | ((uint32_t)p[(2 * e + 1) * pitch] << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int NT, bool DROP>
__global__ __launch_bounds__(256) void lora_bwd_wgrad_kernel(const bf16_t* __restrict__ dqkv, int ldq, const bf16_t* __restrict__ X,
                                                             const bf16_t* __restrict__ U, const bf16_t* __restrict__ dU, float* __restrict__ part,
                                                             int M, int D, LoraCols cols, float s, DropRng rng,
                                                             const int* __restrict__ rows_dev) {
  constexpr int PP = NT * LR + 2;
  __shared__ __attribute__((aligned(16))) bf16_t Qs[NT + 1][32][WG_PITCH];
  __shared__ __attribute__((aligned(16))) bf16_t Ps[2][32][PP];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int chunk = blockIdx.x, cb = blockIdx.y * WG_COLS;
  if (rows_dev) M = min(M, *rows_dev);             // a chunk past the count runs no step and stores exact zeros: the second pass keeps its chunk order
  const long long mbeg = (long long)chunk * WG_ROWS;
  const long long mend = mbeg + WG_ROWS < M ? mbeg + WG_ROWS : M;
  const int gpr = D >> 2;
  f32x4_t accB[NT][2], accA[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) accB[t][j] = accA[t][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (long long m0 = mbeg; m0 < mend; m0 += 32) {
    __syncthreads();                               // the previous step's fragments are read
#pragma unroll
    for (int h = 0; h < 2; ++h) {                  // 32 rows x 16 column groups of 8
      const int lr = (tid >> 4) + 16 * h, c8 = (tid & 15) * 8;
      const long long m = m0 + lr;
      const bool ok = m < mend && cb + c8 < D;
#pragma unroll
      for (int q = 0; q <= NT; ++q) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) {
          if (q < NT) v = *(const uint4*)(dqkv + m * ldq + cols.c[q] + cb + c8);
          else {
            v = *(const uint4*)(X + m * D + cb + c8);
            if constexpr (DROP) v = keep8(v, rng, m, gpr, cb + c8);
          }
        }
        uint32_t* dst = (uint32_t*)&Qs[q][lr][c8];
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
      }
    }
    for (int i = tid; i < 2 * 32 * NT * 4; i += 256) {       // U and dU: 32 rows x NT * 4 groups of 4 ranks each
      const int which = i / (32 * NT * 4), j = i - which * (32 * NT * 4);
      const int lr = j / (NT * 4), c4 = (j - lr * (NT * 4)) * 4;
      const long long m = m0 + lr;
      uint2 v = make_uint2(0, 0);
      if (m < mend) v = *(const uint2*)((which ? dU : U) + m * (NT * LR) + c4);
      uint32_t* dst = (uint32_t*)&Ps[which][lr][c4];
      dst[0] = v.x; dst[1] = v.y;
    }
    __syncthreads();
    uint4 xf[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) xf[j] = lds_col8(&Qs[NT][8 * g][wid * 32 + j * 16 + r], WG_PITCH);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint4 uf = lds_col8(&Ps[0][8 * g][t * LR + r], PP), df = lds_col8(&Ps[1][8 * g][t * LR + r], PP);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        accB[t][j] = mfma32(uf, lds_col8(&Qs[t][8 * g][wid * 32 + j * 16 + r], WG_PITCH), accB[t][j]);
        accA[t][j] = mfma32(df, xf[j], accA[t][j]);
      }
    }
  }
  const float sa = DROP ? rng.scale : 1.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int d = cb + wid * 32 + j * 16 + r;
      if (d >= D) continue;
      float* pb = part + (((long long)chunk * NT + t) * 2) * LR * D + d;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pb[(long long)(4 * g + e) * D] = s * accB[t][j][e];
        pb[(long long)(LR + 4 * g + e) * D] = sa * accA[t][j][e];
      }
    }
}

// The same sums at the image tower's row counts (M = B * n_tok: 200 k rows, 788 chunks): a workgroup walks `run` CONSECUTIVE
// chunks with the accumulators kept in its registers and stores ONE partial, part[blockIdx.x][t][which][rank][d] - 1 / run of the scratch
// traffic and of the second kernel's walk.  Rows are still summed in row order inside a run and the runs in run order by the same second
// kernel: no atomics, two launches give the same bits, and run = 1 gives those of lora_bwd_wgrad_kernel (the same steps in the same order).
template <int NT, bool DROP>
__global__ __launch_bounds__(256) void lora_bwd_wgrad_runs_kernel(const bf16_t* __restrict__ dqkv, int ldq, const bf16_t* __restrict__ X,
                                                                  const bf16_t* __restrict__ U, const bf16_t* __restrict__ dU,
                                                                  float* __restrict__ part, int M, int D, int run, LoraCols cols, float s,
                                                                  DropRng rng) {
  constexpr int PP = NT * LR + 2;
  __shared__ __attribute__((aligned(16))) bf16_t Qs[NT + 1][32][WG_PITCH];
  __shared__ __attribute__((aligned(16))) bf16_t Ps[2][32][PP];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int cb = blockIdx.y * WG_COLS;
  const long long mbeg = (long long)blockIdx.x * run * WG_ROWS;          // the host checked run >= 1 and sized the grid: mbeg < M
  const long long mend = mbeg + (long long)run * WG_ROWS < M ? mbeg + (long long)run * WG_ROWS : M;
  const int gpr = D >> 2;
  f32x4_t accB[NT][2], accA[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) accB[t][j] = accA[t][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (long long m0 = mbeg; m0 < mend; m0 += 32) {                        // WG_ROWS is a multiple of 32: a step never straddles two chunks
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int lr = (tid >> 4) + 16 * h, c8 = (tid & 15) * 8;
      const long long m = m0 + lr;
      const bool ok = m < mend && cb + c8 < D;
#pragma unroll
      for (int q = 0; q <= NT; ++q) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) {
          if (q < NT) v = *(const uint4*)(dqkv + m * ldq + cols.c[q] + cb + c8);
          else {
            v = *(const uint4*)(X + m * D + cb + c8);
            if constexpr (DROP) v = keep8(v, rng, m, gpr, cb + c8);
          }
        }
        uint32_t* dst = (uint32_t*)&Qs[q][lr][c8];
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
      }
    }
    for (int i = tid; i < 2 * 32 * NT * 4; i += 256) {
      const int which = i / (32 * NT * 4), j = i - which * (32 * NT * 4);
      const int lr = j / (NT * 4), c4 = (j - lr * (NT * 4)) * 4;
      const long long m = m0 + lr;
      uint2 v = make_uint2(0, 0);
      if (m < mend) v = *(const uint2*)((which ? dU : U) + m * (NT * LR) + c4);
      uint32_t* dst = (uint32_t*)&Ps[which][lr][c4];
      dst[0] = v.x; dst[1] = v.y;
    }
    __syncthreads();
    uint4 xf[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) xf[j] = lds_col8(&Qs[NT][8 * g][wid * 32 + j * 16 + r], WG_PITCH);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint4 uf = lds_col8(&Ps[0][8 * g][t * LR + r], PP), df = lds_col8(&Ps[1][8 * g][t * LR + r], PP);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        accB[t][j] = mfma32(uf, lds_col8(&Qs[t][8 * g][wid * 32 + j * 16 + r], WG_PITCH), accB[t][j]);
        accA[t][j] = mfma32(df, xf[j], accA[t][j]);
      }
    }
  }
  const float sa = DROP ? rng.scale : 1.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int d = cb + wid * 32 + j * 16 + r;
      if (d >= D) continue;
      float* pb = part + (((long long)blockIdx.x * NT + t) * 2) * LR * D + d;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pb[(long long)(4 * g + e) * D] = s * accB[t][j][e];
        pb[(long long)(LR + 4 * g + e) * D] = sa * accA[t][j][e];
      }
    }
}

// gA[t*16 + rank][d] += sum over chunks (chunk order) of part[chunk][t][1][rank][d];  gB[t*D + d][rank] += ... of part[chunk][t][0][rank][d]
__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(const float* __restrict__ part, int nchunk, int NT, int D, float* __restrict__ gA,
                                                                float* __restrict__ gB) {
  const long long total = (long long)NT * 2 * LR * D;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float sum = 0.f;
  for (int c = 0; c < nchunk; ++c) sum += part[(long long)c * total + e];
  const int d = (int)(e % D);
  const int rank = (int)((e / D) % LR);
  const int which = (int)((e / ((long long)D * LR)) % 2);
  const int t = (int)(e / ((long long)D * LR * 2));
  if (which) gA[((long long)t * LR + rank) * D + d] += sum;
  else gB[((long long)t * D + d) * LR + rank] += sum;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(bf16_t* __restrict__ W, int ldw, const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bw,
                                                         int D, int NT, LoraCols cols, float s) {
  const long long total = (long long)NT * D * D;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int i = (int)(e % D), o = (int)((e / D) % D), t = (int)(e / ((long long)D * D));
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < LR; ++k) acc += bf2f(Bw[((long long)t * D + o) * LR + k]) * bf2f(A[((long long)t * LR + k) * D + i]);
  bf16_t* w = W + (long long)(cols.c[t] + o) * ldw + i;
  *w = f2bf(bf2f(*w) + s * acc);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int lora_check(int ld, int M, int D, int n, int c0, int c1, int c2, LoraCols* out) {
  if (M <= 0 || D <= 0 || (D & 63) || n < 1 || n > 3 || (ld & 7)) return MM_ERR_SHAPE;
  const int c[3] = {c0, c1, c2};
  for (int t = 0; t < n; ++t) {
    if (c[t] < 0 || (c[t] & 7) || (long long)c[t] + D > ld) return MM_ERR_SHAPE;
    for (int u = 0; u < t; ++u)
      if (c[t] < c[u] + D && c[u] < c[t] + D) return MM_ERR_SHAPE;       // two targets on the same columns
  }
  for (int t = 0; t < 3; ++t) out->c[t] = t < n ? c[t] : 0;
  return MM_OK;
}

#define LORA_DISPATCH(KERNEL, grid, ...)                                                                                       \
  do {                                                                                                                         \
    const bool drop_ = rng.thresh != 0;                                                                                        \
    if (n == 1) { if (drop_) hipLaunchKernelGGL((KERNEL<1, true>), grid, dim3(256), 0, stream, __VA_ARGS__);                   \
                  else hipLaunchKernelGGL((KERNEL<1, false>), grid, dim3(256), 0, stream, __VA_ARGS__); }                      \
    else if (n == 2) { if (drop_) hipLaunchKernelGGL((KERNEL<2, true>), grid, dim3(256), 0, stream, __VA_ARGS__);              \
                       else hipLaunchKernelGGL((KERNEL<2, false>), grid, dim3(256), 0, stream, __VA_ARGS__); }                 \
    else { if (drop_) hipLaunchKernelGGL((KERNEL<3, true>), grid, dim3(256), 0, stream, __VA_ARGS__);                          \
           else hipLaunchKernelGGL((KERNEL<3, false>), grid, dim3(256), 0, stream, __VA_ARGS__); }                             \
  } while (0)

static int lora_fwd_impl(const void* X, const void* A, const void* Bw, void* U, void* qkv, int ldq, int M, int D, int n, int c0, int c1,
                         int c2, float s, long long seed, long long step, long long site, long long thresh, float scale,
                         const int* rows_dev, hipStream_t stream) {
  if (!X || !A || !Bw || !U || !qkv) return MM_ERR_ARG;
  LoraCols cols;
  if (int rc = lora_check(ldq, M, D, n, c0, c1, c2, &cols)) return rc;
  const DropRng rng = make_drop_rng(seed, step, site, thresh, scale);
  const dim3 grid((unsigned)((M + 63) / 64));
  LORA_DISPATCH(lora_fwd_kernel, grid, (const bf16_t*)X, (const bf16_t*)A, (const bf16_t*)Bw, (bf16_t*)U, (bf16_t*)qkv, ldq, M, D, cols, s, rng,
                rows_dev);
  return mm_check_launch();
}
extern "C" int medmoe_lora_fwd(const void* X, const void* A, const void* Bw, void* U, void* qkv, int ldq, int M, int D, int n, int c0, int c1,
                               int c2, float s, long long seed, long long step, long long site, long long thresh, float scale,
                               hipStream_t stream) {
  return lora_fwd_impl(X, A, Bw, U, qkv, ldq, M, D, n, c0, c1, c2, s, seed, step, site, thresh, scale, nullptr, stream);
}
// the *_rows forms: the same kernels over the first min(M, *rows_dev) rows (rows_dev: device int; M bounds the grid).  Rows at and past the
// count are neither read nor written; the dropout mask of element (row, column) is the one the plain form draws.
extern "C" int medmoe_lora_fwd_rows(const void* X, const void* A, const void* Bw, void* U, void* qkv, int ldq, int M, int D, int n, int c0,
                                    int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale,
                                    const int* rows_dev, hipStream_t stream) {
  if (!rows_dev) return MM_ERR_ARG;
  return lora_fwd_impl(X, A, Bw, U, qkv, ldq, M, D, n, c0, c1, c2, s, seed, step, site, thresh, scale, rows_dev, stream);
}

static int lora_bwd_dx_impl(const void* dqkv, int ldq, const void* Bt, const void* At, void* dU, void* dy, int M, int D, int n, int c0,
                            int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale,
                            const int* rows_dev, hipStream_t stream) {
  if (!dqkv || !Bt || !At || !dU) return MM_ERR_ARG;
  LoraCols cols;
  if (int rc = lora_check(ldq, M, D, n, c0, c1, c2, &cols)) return rc;
  const DropRng rng = make_drop_rng(seed, step, site, thresh, scale);
  const dim3 grid((unsigned)((M + 63) / 64));
  LORA_DISPATCH(lora_bwd_dx_kernel, grid, (const bf16_t*)dqkv, ldq, (const bf16_t*)Bt, (const bf16_t*)At, (bf16_t*)dU, (bf16_t*)dy, M, D, cols, s,
                rng, rows_dev);
  return mm_check_launch();
}
extern "C" int medmoe_lora_bwd_dx(const void* dqkv, int ldq, const void* Bt, const void* At, void* dU, void* dy, int M, int D, int n, int c0,
                                  int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale,
                                  hipStream_t stream) {
  return lora_bwd_dx_impl(dqkv, ldq, Bt, At, dU, dy, M, D, n, c0, c1, c2, s, seed, step, site, thresh, scale, nullptr, stream);
}
extern "C" int medmoe_lora_bwd_dx_rows(const void* dqkv, int ldq, const void* Bt, const void* At, void* dU, void* dy, int M, int D, int n, int c0,
                                       int c1, int c2, float s, long long seed, long long step, long long site, long long thresh, float scale,
                                       const int* rows_dev, hipStream_t stream) {
  if (!rows_dev) return MM_ERR_ARG;
  return lora_bwd_dx_impl(dqkv, ldq, Bt, At, dU, dy, M, D, n, c0, c1, c2, s, seed, step, site, thresh, scale, rows_dev, stream);
}

extern "C" long long medmoe_lora_wgrad_scratch(int M, int D, int n) {
  if (M <= 0 || D <= 0 || n < 1 || n > 3) return 0;
  return (long long)((M + WG_ROWS - 1) / WG_ROWS) * n * 2 * LR * D;
}

static int lora_bwd_wgrad_impl(const void* dqkv, int ldq, const void* X, const void* U, const void* dU, float* gA, float* gB, float* scratch,
                               long long scratch_floats, int M, int D, int n, int c0, int c1, int c2, float s, long long seed,
                               long long step, long long site, long long thresh, float scale, const int* rows_dev, hipStream_t stream) {
  if (!dqkv || !X || !U || !dU || !gA || !gB || !scratch) return MM_ERR_ARG;
  LoraCols cols;
  if (int rc = lora_check(ldq, M, D, n, c0, c1, c2, &cols)) return rc;
  if (scratch_floats < medmoe_lora_wgrad_scratch(M, D, n)) return MM_ERR_SHAPE;
  const DropRng rng = make_drop_rng(seed, step, site, thresh, scale);
  const int nchunk = (M + WG_ROWS - 1) / WG_ROWS;
  const dim3 grid((unsigned)nchunk, (unsigned)((D + WG_COLS - 1) / WG_COLS));
  LORA_DISPATCH(lora_bwd_wgrad_kernel, grid, (const bf16_t*)dqkv, ldq, (const bf16_t*)X, (const bf16_t*)U, (const bf16_t*)dU, scratch, M, D, cols,
                s, rng, rows_dev);
  if (int rc = mm_check_launch()) return rc;
  const long long total = (long long)n * 2 * LR * D;
  hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const float*)scratch, nchunk, n, D, gA,
                     gB);
  return mm_check_launch();
}
extern "C" int medmoe_lora_bwd_wgrad(const void* dqkv, int ldq, const void* X, const void* U, const void* dU, float* gA, float* gB, float* scratch,
                                     long long scratch_floats, int M, int D, int n, int c0, int c1, int c2, float s, long long seed,
                                     long long step, long long site, long long thresh, float scale, hipStream_t stream) {
  return lora_bwd_wgrad_impl(dqkv, ldq, X, U, dU, gA, gB, scratch, scratch_floats, M, D, n, c0, c1, c2, s, seed, step, site, thresh, scale, nullptr,
                             stream);
}
// scratch: medmoe_lora_wgrad_scratch(M, D, n) floats (M chunks); a 256-row chunk past the count contributes exact zeros to the fixed-order sum
extern "C" int medmoe_lora_bwd_wgrad_rows(const void* dqkv, int ldq, const void* X, const void* U, const void* dU, float* gA, float* gB,
                                          float* scratch, long long scratch_floats, int M, int D, int n, int c0, int c1, int c2, float s,
                                          long long seed, long long step, long long site, long long thresh, float scale, const int* rows_dev,
                                          hipStream_t stream) {
  if (!rows_dev) return MM_ERR_ARG;
  return lora_bwd_wgrad_impl(dqkv, ldq, X, U, dU, gA, gB, scratch, scratch_floats, M, D, n, c0, c1, c2, s, seed, step, site, thresh, scale, rows_dev,
                             stream);
}

// the image tower's form: one partial per `run` consecutive 256-row chunks.  scratch: medmoe_lora_wgrad_runs_scratch floats
extern "C" long long medmoe_lora_wgrad_runs_scratch(int M, int D, int n, int run) {
  if (M <= 0 || D <= 0 || n < 1 || n > 3 || run < 1) return 0;
  const long long nchunk = ((long long)M + WG_ROWS - 1) / WG_ROWS;
  return ((nchunk + run - 1) / run) * n * 2 * LR * D;
}

extern "C" int medmoe_lora_bwd_wgrad_runs(const void* dqkv, int ldq, const void* X, const void* U, const void* dU, float* gA, float* gB,
                                          float* scratch, long long scratch_floats, int M, int D, int n, int c0, int c1, int c2, int run,
                                          float s, long long seed, long long step, long long site, long long thresh, float scale,
                                          hipStream_t stream) {
  if (!dqkv || !X || !U || !dU || !gA || !gB || !scratch) return MM_ERR_ARG;
  if (run < 1) return MM_ERR_SHAPE;
  LoraCols cols;
  if (int rc = lora_check(ldq, M, D, n, c0, c1, c2, &cols)) return rc;
  if (scratch_floats < medmoe_lora_wgrad_runs_scratch(M, D, n, run)) return MM_ERR_SHAPE;
  const DropRng rng = make_drop_rng(seed, step, site, thresh, scale);
  const long long nchunk = ((long long)M + WG_ROWS - 1) / WG_ROWS;
  const int nrun = (int)((nchunk + run - 1) / run);
  const dim3 grid((unsigned)nrun, (unsigned)((D + WG_COLS - 1) / WG_COLS));
  LORA_DISPATCH(lora_bwd_wgrad_runs_kernel, grid, (const bf16_t*)dqkv, ldq, (const bf16_t*)X, (const bf16_t*)U, (const bf16_t*)dU, scratch, M, D,
                run, cols, s, rng);
  if (int rc = mm_check_launch()) return rc;
  const long long total = (long long)n * 2 * LR * D;
  hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const float*)scratch, nrun, n, D, gA,
                     gB);
  return mm_check_launch();
}

extern "C" int medmoe_lora_merge(void* W, int ldw, const void* A, const void* Bw, int D, int n, int c0, int c1, int c2, float s,
                                 hipStream_t stream) {
  if (!W || !A || !Bw) return MM_ERR_ARG;
  if (D <= 0 || ldw < D || n < 1 || n > 3 || c0 < 0 || c1 < 0 || c2 < 0) return MM_ERR_SHAPE;
  LoraCols cols = {{c0, n > 1 ? c1 : 0, n > 2 ? c2 : 0}};
  const long long total = (long long)n * D * D;
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (bf16_t*)W, ldw, (const bf16_t*)A,
                     (const bf16_t*)Bw, D, n, cols, s);
  return mm_check_launch();
}
