// Masked-language-model objective of the text tower: the step's mask drawn on the chip, and the tied decoder fused with its
// cross-entropy so that no [rows][vocab] array exists anywhere - forward or backward.
//
//   medmoe_mlm_mask          one workgroup: every thread owns a contiguous run of the B T tokens, counts its selected tokens (Philox word 0 of
//                            the token's own group), the 1024 counts are scanned in LDS and the run is walked a second time to write the
//                            ascending row list - no atomics, the list does not depend on the launch
//   medmoe_rows_gather / medmoe_rows_scatter_add   the selected rows of the last hidden state into [M_bound][D] and the head's gradient back
//   medmoe_vocab_ce_fwd      logits^T tile = E_tile z_tile^T on v_mfma_f32_32x32x16_bf16: the token row is the accumulator's COLUMN (a lane),
//                            its 16 registers are 16 vocabulary entries, so (max, sum exp, target logit) of a row reduce in registers, one
//                            exchange between the lane halves and one pass through LDS over the four waves.  A workgroup owns 64 rows x 256
//                            vocabulary entries and stores one (max, sum) pair per row; a second kernel merges the ceil(V / 256) pairs of a
//                            row in tile order, a third sums the row terms in a fixed order.
//   medmoe_vocab_ce_bwd_dx / _dw   one kernel template, attention's structure with K = V = E.  A workgroup OWNS 64 rows of one operand
//                            (token rows for dx, vocabulary rows for dw) and STREAMS 64-row tiles of the other.  Per streamed tile: the
//                            score tile is recomputed in k-chunks of 64 through LDS (owned index on the lane, streamed index in the
//                            registers), P = (exp(s - lse) - onehot) loss_scale / count is formed in fp32, rounded to bf16 into LDS as
//                            [owned][streamed], and a second product out[owned][d] += P Y accumulates in registers (64 x D fp32 over four
//                            waves), its B operand read from the row-major streamed chunk with the transposing LDS read.  One owner per
//                            output element: dz is written once, dE / dbias are read-modify-written once - no atomics, two calls give the
//                            same bits.
// Rows at and past the device-side count are never read into a result: their z is replaced by zeros as it is staged.
#include "common.h"
#include "medmoe_hip.h"
#include "philox.h"

namespace {

constexpr int PITCH = 72;                      // bf16 elements of an LDS row: a 64-element chunk + 16 bytes, so 16-byte fragment reads of 32 rows spread over the banks
constexpr int FWD_BN = 256;                    // vocabulary entries of a forward tile
constexpr unsigned MLM_T80 = 3435973836u;      // floor(0.8 * 2^32)
constexpr unsigned MLM_T90 = 3865470566u;      // floor(0.9 * 2^32)

__device__ __forceinline__ int live_count(const int* count, int bound) { return min(max(*count, 0), bound); }

// ---------------------------------------------------------------------------------------------------------------------------------------
// mask
// ---------------------------------------------------------------------------------------------------------------------------------------
struct MlmTok { bool sel; int id_new; };

__device__ __forceinline__ MlmTok mlm_draw(const DropRng& rng, int id, bool cand, unsigned long long group, int mask_id, int V) {
  MlmTok r = {false, id};
  if (!cand) return r;
  const uint4 w = drop_words(rng, group);
  if (w.x >= rng.thresh) return r;
  r.sel = true;
  r.id_new = w.y < MLM_T80 ? mask_id : (w.y < MLM_T90 ? (int)__umulhi(w.z, (unsigned)V) : id);
  return r;
}

__global__ __launch_bounds__(1024) void mlm_mask_kernel(const int* __restrict__ ids, const unsigned char* __restrict__ attn,
                                                        const int* __restrict__ tok_row, int* __restrict__ ids_masked, int* __restrict__ labels,
                                                        int* __restrict__ rows, int* __restrict__ row_labels, int* __restrict__ count, int B, int T,
                                                        int V, int cls_id, int sep_id, int pad_id, int mask_id, long long sample_offset, DropRng rng) {
  __shared__ int sh[1024];
  const int tid = threadIdx.x;
  const long long n = (long long)B * T;
  const long long per = (n + 1023) / 1024;
  const long long lo = min(n, tid * per), hi = min(n, lo + per);
  int c = 0;
  for (long long i = lo; i < hi; ++i) {
    const int id = ids[i];
    const bool cand = attn[i] != 0 && id != cls_id && id != sep_id && id != pad_id;
    c += mlm_draw(rng, id, cand, (unsigned long long)(sample_offset * T + i), mask_id, V).sel ? 1 : 0;
  }
  sh[tid] = c;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {                    // inclusive scan
    const int v = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += v;
    __syncthreads();
  }
  int k = sh[tid] - c;
  for (long long i = lo; i < hi; ++i) {
    const int id = ids[i];
    const bool cand = attn[i] != 0 && id != cls_id && id != sep_id && id != pad_id;
    const MlmTok m = mlm_draw(rng, id, cand, (unsigned long long)(sample_offset * T + i), mask_id, V);
    ids_masked[i] = m.id_new;
    labels[i] = m.sel ? id : -1;
    if (m.sel) {
      rows[k] = tok_row ? tok_row[i] : (int)i;
      row_labels[k] = id;
      ++k;
    }
  }
  if (tid == 1023) count[0] = sh[1023];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// gather / scatter-add of the selected rows, and the head's GELU' product (rows past the count become zeros: the weight-gradient GEMM
// behind it runs over all M_bound rows)
// ---------------------------------------------------------------------------------------------------------------------------------------
template <int MODE>      // 0 dst[k] = src[rows[k]], 1 dst[rows[k]] += src[k], 2 dst[k] = src[k] * aux[k] (k < count) or 0
__global__ __launch_bounds__(256) void mlm_rows_kernel(const bf16_t* __restrict__ src, const bf16_t* __restrict__ aux, const int* __restrict__ rows,
                                                       const int* __restrict__ count, bf16_t* __restrict__ dst, int M_bound, int D) {
  const int n = live_count(count, M_bound);
  const int d8 = D >> 3;
  const long long total = (long long)(MODE == 2 ? M_bound : n) * d8;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i / d8), c = (int)(i % d8) * 8;
    if (MODE == 2) {
      uint4 o = make_uint4(0, 0, 0, 0);
      if (k < n) {
        const uint4 a = *(const uint4*)(src + (long long)k * D + c), b = *(const uint4*)(aux + (long long)k * D + c);
        const uint32_t* ap = (const uint32_t*)&a; const uint32_t* bp = (const uint32_t*)&b; uint32_t* op = (uint32_t*)&o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          op[e] = pack2bf(bf2f((bf16_t)(ap[e] & 0xffffu)) * bf2f((bf16_t)(bp[e] & 0xffffu)), bf2f((bf16_t)(ap[e] >> 16)) * bf2f((bf16_t)(bp[e] >> 16)));
      }
      *(uint4*)(dst + (long long)k * D + c) = o;
    } else if (MODE == 0) {
      *(uint4*)(dst + (long long)k * D + c) = *(const uint4*)(src + (long long)rows[k] * D + c);
    } else {
      bf16_t* dp = dst + (long long)rows[k] * D + c;
      const uint4 a = *(const uint4*)(src + (long long)k * D + c), b = *(const uint4*)dp;
      uint4 o;
      const uint32_t* ap = (const uint32_t*)&a; const uint32_t* bp = (const uint32_t*)&b; uint32_t* op = (uint32_t*)&o;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        op[e] = pack2bf(bf2f((bf16_t)(ap[e] & 0xffffu)) + bf2f((bf16_t)(bp[e] & 0xffffu)), bf2f((bf16_t)(ap[e] >> 16)) + bf2f((bf16_t)(bp[e] >> 16)));
      *(uint4*)dp = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// staging: a [ROWS][64] bf16 chunk (rows row0 .. of a [*][ld] array, columns col0 ..) -> registers -> LDS rows of PITCH elements.  A row at or
// past `limit` is read from row limit - 1 (a valid address) and replaced by zeros.
// ---------------------------------------------------------------------------------------------------------------------------------------
template <int ROWS>
__device__ __forceinline__ void chunk_load(uint4 (&r)[ROWS / 32], const bf16_t* __restrict__ base, int ld, int row0, int limit, int col0) {
#pragma unroll
  for (int i = 0; i < ROWS / 32; ++i) {
    const int p = threadIdx.x + 256 * i, row = row0 + (p >> 3);
    const uint4 v = *(const uint4*)(base + (long long)min(row, limit - 1) * ld + col0 + (p & 7) * 8);
    r[i] = row < limit ? v : make_uint4(0, 0, 0, 0);
  }
}
template <int ROWS>
__device__ __forceinline__ void chunk_store(const uint4 (&r)[ROWS / 32], bf16_t* s) {
#pragma unroll
  for (int i = 0; i < ROWS / 32; ++i) {
    const int p = threadIdx.x + 256 * i;
    *(uint4*)(s + (p >> 3) * PITCH + (p & 7) * 8) = r[i];
  }
}
// fragment of v_mfma_f32_32x32x16_bf16 for an operand stored [row][k]: lane l holds row l & 31, k = 16 ks + 8 (l >> 5) + 0..7
__device__ __forceinline__ bf16x8_t row_frag(const bf16_t* s, int row, int ks, int h) {
  return *(const bf16x8_t*)(s + row * PITCH + ks * 16 + 8 * h);
}
// the same fragment for an operand stored [k][col] (the transposing LDS read: in each 16-lane group lane 4 q + p supplies row q, columns
// 4 p .. 4 p + 3 of a 4 x 16 block and receives column lane & 15): lane l holds column col0 + (l & 31), k = 16 ks + 8 (l >> 5) + 0..7
__device__ __forceinline__ bf16x8_t col_frag(const bf16_t* s, int col0, int ks, int lane) {
  const int h = lane >> 5, gam = (lane >> 4) & 1, q = (lane & 15) >> 2, pp = lane & 3;
  const bf16_t* a = s + (ks * 16 + 8 * h + q) * PITCH + col0 + gam * 16 + 4 * pp;
  const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)a);
  const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)(a + 4 * PITCH));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// accumulator register r of lane half h -> row of the 32 x 32 tile
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// (max, sum exp) pairs merged in the order (a, b); a pair with max = -inf holds nothing
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm == -INFINITY) { m = mm; s = 0.f; return; }
  s = s * expf(m - mm) + s2 * expf(m2 - mm);
  m = mm;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vocab_ce_fwd_kernel(const bf16_t* __restrict__ z, const bf16_t* __restrict__ E, const float* __restrict__ bias,
                                                           const int* __restrict__ row_labels, const int* __restrict__ count,
                                                           float* __restrict__ pmax, float* __restrict__ psum, float* __restrict__ tgt, int M_bound,
                                                           int V, int D, int NT) {
  __shared__ __attribute__((aligned(16))) bf16_t sZ[64 * PITCH];
  __shared__ __attribute__((aligned(16))) bf16_t sE[FWD_BN * PITCH];
  __shared__ float redm[4][64], reds[4][64];
  const int n = live_count(count, M_bound);
  const int m0 = blockIdx.y * 64, v0 = blockIdx.x * FWD_BN;
  if (m0 >= n) return;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane >> 5, lc = lane & 31;
  f32x16_t acc[2][2];                                        // [vocabulary tile of the wave][row tile]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  uint4 rz[2], re[8];
  const int nk = D >> 6;
  chunk_load<64>(rz, z, D, m0, n, 0);
  chunk_load<FWD_BN>(re, E, D, v0, V, 0);
  for (int k = 0; k < nk; ++k) {
    chunk_store<64>(rz, sZ);
    chunk_store<FWD_BN>(re, sE);
    __syncthreads();
    if (k + 1 < nk) {
      chunk_load<64>(rz, z, D, m0, n, (k + 1) * 64);
      chunk_load<FWD_BN>(re, E, D, v0, V, (k + 1) * 64);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8_t fe[2], fz[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) fe[a] = row_frag(sE, w * 64 + a * 32 + lc, ks, h);
#pragma unroll
      for (int b = 0; b < 2; ++b) fz[b] = row_frag(sZ, b * 32 + lc, ks, h);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fe[a], fz[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
  }
  // the wave's 64 vocabulary entries of every row: 2 x 16 registers in each lane half
  float bv[2][16];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int v = v0 + w * 64 + a * 32 + acc_row(r, h);
      bv[a][r] = v < V ? bias[v] : -INFINITY;                // a column past V: excluded from max and sum
    }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int m = m0 + b * 32 + lc;
    const int label = m < n ? row_labels[m] : -1;
    float mx = -INFINITY;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[a][b][r] += bv[a][r];
        mx = fmaxf(mx, acc[a][b][r]);
      }
    float sum = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = v0 + w * 64 + a * 32 + acc_row(r, h);
        sum += mx == -INFINITY ? 0.f : expf(acc[a][b][r] - mx);
        if (v == label && v < V) tgt[m] = acc[a][b][r];      // one owner: the lane and register that hold (m, label)
      }
    const float mo = __shfl_xor(mx, 32, 64), so = __shfl_xor(sum, 32, 64);
    if (h == 0) {
      lse_merge(mx, sum, mo, so);                            // (lower half, upper half)
      redm[w][b * 32 + lc] = mx;
      reds[w][b * 32 + lc] = sum;
    }
  }
  __syncthreads();
  if (tid < 64 && m0 + tid < n) {
    float mx = redm[0][tid], sum = reds[0][tid];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) lse_merge(mx, sum, redm[ww][tid], reds[ww][tid]);
    pmax[(long long)(m0 + tid) * NT + blockIdx.x] = mx;
    psum[(long long)(m0 + tid) * NT + blockIdx.x] = sum;
  }
}

// a row's NT pairs merged in tile order; rows at and past the count get lse = term = 0
__global__ __launch_bounds__(256) void vocab_ce_rows_kernel(const float* __restrict__ pmax, const float* __restrict__ psum, const float* __restrict__ tgt,
                                                            const int* __restrict__ count, float* __restrict__ lse, float* __restrict__ terms,
                                                            int* __restrict__ hits, int M_bound, int NT) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M_bound) return;
  const int n = live_count(count, M_bound);
  if (m >= n) { lse[m] = 0.f; terms[m] = 0.f; hits[m] = 0; return; }
  const float* pm = pmax + (long long)m * NT;
  const float* ps = psum + (long long)m * NT;
  float mx = -INFINITY;
  for (int t = 0; t < NT; ++t) mx = fmaxf(mx, pm[t]);
  float sum = 0.f;
  for (int t = 0; t < NT; ++t) sum += ps[t] * expf(pm[t] - mx);
  const float l = mx + logf(sum);
  lse[m] = l;
  terms[m] = l - tgt[m];
  hits[m] = tgt[m] == mx ? 1 : 0;
}

// loss = loss_scale * (sum of the live rows' terms) / count, 0 for count 0; thread t sums rows t, t + 1024, ..., the threads meet in a tree
__global__ __launch_bounds__(1024) void vocab_ce_loss_kernel(const float* __restrict__ terms, const int* __restrict__ hits, const int* __restrict__ count,
                                                             float loss_scale, float* __restrict__ loss, int* __restrict__ counts, int M_bound) {
  __shared__ float sf[1024];
  __shared__ int si[1024];
  const int n = live_count(count, M_bound), tid = threadIdx.x;
  float s = 0.f;
  int c = 0;
  for (int m = tid; m < n; m += 1024) { s += terms[m]; c += hits[m]; }
  sf[tid] = s; si[tid] = c;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) { sf[tid] += sf[tid + o]; si[tid] += si[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    loss[0] = n > 0 ? loss_scale * sf[0] / (float)n : 0.f;
    counts[0] = n;
    counts[1] = si[0];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// backward: DW = false owns 64 token rows and streams the vocabulary (dz), DW = true owns 64 vocabulary rows and streams the token rows
// (dE, dbias).  ND: 64-column chunks of D the accumulator array is sized for (D / 64 <= ND).
// ---------------------------------------------------------------------------------------------------------------------------------------
template <bool DW, int ND>
__global__ __launch_bounds__(256) void vocab_ce_bwd_kernel(const bf16_t* __restrict__ z, const bf16_t* __restrict__ E, const float* __restrict__ bias,
                                                           const int* __restrict__ row_labels, const float* __restrict__ lse,
                                                           const int* __restrict__ count, float loss_scale, bf16_t* __restrict__ dz,
                                                           float* __restrict__ dE, float* __restrict__ dbias, int M_bound, int V, int D) {
  __shared__ __attribute__((aligned(16))) bf16_t sX[64 * PITCH];      // owned rows, one k-chunk
  __shared__ __attribute__((aligned(16))) bf16_t sY[64 * PITCH];      // streamed rows, one k-chunk (scores) or one d-chunk (second product)
  __shared__ __attribute__((aligned(16))) bf16_t sP[64 * PITCH];      // P [owned][streamed]
  __shared__ float redb[4][32];
  const int n = live_count(count, M_bound);
  if (n == 0) return;
  const bf16_t* X = DW ? E : z;
  const bf16_t* Y = DW ? z : E;
  const int Li = DW ? V : n, Lj = DW ? n : V;
  const int i0 = blockIdx.x * 64;
  if (i0 >= Li) return;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane >> 5, lc = lane & 31;
  const int jh = w & 1, ih = w >> 1;                         // the wave's quadrant of the score tile; (ih, w & 1) is also its (row half, 32-column tile) of every d-chunk
  const int nd = D >> 6, njt = (Lj + 63) >> 6;
  const float scale = loss_scale / (float)n;
  const int i = i0 + ih * 32 + lc;                           // the owned index of this lane
  const bool i_ok = i < Li;
  // per-lane constants of the owned index: bias (dw) or lse and label (dx)
  const float own_f = i_ok ? (DW ? bias[i] : lse[i]) : 0.f;
  const int own_label = (!DW && i_ok) ? row_labels[i] : -1;

  f32x16_t acc[ND];
#pragma unroll
  for (int c = 0; c < ND; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  float bsum = 0.f;

  uint4 rx[2], ry[2];
  chunk_load<64>(rx, X, D, i0, Li, 0);
  chunk_load<64>(ry, Y, D, 0, Lj, 0);
  for (int jt = 0; jt < njt; ++jt) {
    const int j0 = jt * 64;
    f32x16_t s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    for (int k = 0; k < nd; ++k) {
      chunk_store<64>(rx, sX);
      chunk_store<64>(ry, sY);
      __syncthreads();
      if (k + 1 < nd) {
        chunk_load<64>(rx, X, D, i0, Li, (k + 1) * 64);
        chunk_load<64>(ry, Y, D, j0, Lj, (k + 1) * 64);
      } else {
        chunk_load<64>(ry, Y, D, j0, Lj, 0);                 // d-chunk 0 of the second product
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(sY, jh * 32 + lc, ks, h), row_frag(sX, ih * 32 + lc, ks, h), s, 0, 0, 0);
      __syncthreads();
    }
    // P of the quadrant: lane = owned index, register r = streamed index j0 + 32 jh + acc_row(r, h)
    float p[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + jh * 32 + acc_row(r, h);
      const bool ok = i_ok && j < Lj;
      const int jc = min(j, Lj - 1);
      float lse_m, b_v;
      int label, v;
      if (DW) { lse_m = lse[jc]; label = row_labels[jc]; b_v = own_f; v = i; }
      else { lse_m = own_f; label = own_label; b_v = bias[jc]; v = j; }
      const float e = __expf(s[r] + b_v - lse_m);
      p[r] = ok ? (e - (label == v ? 1.f : 0.f)) * scale : 0.f;
      bsum += p[r];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *(uint2*)(sP + (ih * 32 + lc) * PITCH + jh * 32 + 8 * g + 4 * h) = make_uint2(pack2bf(p[4 * g], p[4 * g + 1]), pack2bf(p[4 * g + 2], p[4 * g + 3]));
    // out[owned][d] += P [owned][streamed] Y [streamed][d], one 64-column chunk of d at a time
#pragma unroll
    for (int c = 0; c < ND; ++c) {
      if (c < nd) {
        chunk_store<64>(ry, sY);
        __syncthreads();                                     // also: sP is complete
        if (c + 1 < nd) chunk_load<64>(ry, Y, D, j0, Lj, (c + 1) * 64);
        else if (jt + 1 < njt) {
          chunk_load<64>(rx, X, D, i0, Li, 0);
          chunk_load<64>(ry, Y, D, j0 + 64, Lj, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(sP, ih * 32 + lc, ks, h), col_frag(sY, (w & 1) * 32, ks, lane), acc[c], 0, 0, 0);
        __syncthreads();
      }
    }
  }
  // accumulator of chunk c: rows i0 + 32 ih + acc_row(r, h), column 64 c + 32 (w & 1) + lc
#pragma unroll
  for (int c = 0; c < ND; ++c) {
    if (c < nd) {
      const int d = c * 64 + (w & 1) * 32 + lc;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i0 + ih * 32 + acc_row(r, h);
        if (row < Li) {
          if (DW) dE[(long long)row * D + d] += acc[c][r];
          else dz[(long long)row * D + d] = f2bf(acc[c][r]);
        }
      }
    }
  }
  if (DW) {
    bsum += __shfl_xor(bsum, 32, 64);
    if (h == 0) redb[w][lc] = bsum;
    __syncthreads();
    if (tid < 64 && i0 + tid < V) dbias[i0 + tid] += redb[(tid >> 5) * 2][tid & 31] + redb[(tid >> 5) * 2 + 1][tid & 31];
  }
}

inline bool ce_shape_ok(int M_bound, int V, int D) { return M_bound >= 1 && V >= 2 && D >= 64 && D <= 1024 && D % 64 == 0; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int fwd_tiles(int V) { return (V + FWD_BN - 1) / FWD_BN; }

template <bool DW>
void launch_bwd(int blocks, hipStream_t stream, const bf16_t* z, const bf16_t* E, const float* bias, const int* row_labels, const float* lse,
                const int* count, float loss_scale, bf16_t* dz, float* dE, float* dbias, int M_bound, int V, int D) {
#define CE_BWD(ND)                                                                                                                              \
  hipLaunchKernelGGL((vocab_ce_bwd_kernel<DW, ND>), dim3(blocks), dim3(256), 0, stream, z, E, bias, row_labels, lse, count, loss_scale, dz, dE, \
                     dbias, M_bound, V, D)
  const int nd = D >> 6;
  if (nd <= 1) CE_BWD(1);
  else if (nd <= 2) CE_BWD(2);
  else if (nd <= 4) CE_BWD(4);
  else if (nd <= 8) CE_BWD(8);
  else if (nd <= 12) CE_BWD(12);
  else CE_BWD(16);
#undef CE_BWD
}

}  // namespace

extern "C" int medmoe_mlm_mask(const int* ids, const unsigned char* attn, const int* tok_row, int* ids_masked, int* labels, int* rows,
                               int* row_labels, int* count, int B, int T, int V, int cls_id, int sep_id, int pad_id, int mask_id,
                               long long sample_offset, long long seed, long long step, long long thresh, hipStream_t stream) {
  if (!ids || !attn || !ids_masked || !labels || !rows || !row_labels || !count) return MM_ERR_ARG;
  if (B < 1 || T < 1 || (long long)B * T > 0x7fffffffll || V < 2 || mask_id < 0 || mask_id >= V || sample_offset < 0 || thresh < 0 ||
      thresh > 0xffffffffll)
    return MM_ERR_SHAPE;
  const DropRng rng = make_drop_rng(seed, step, DROPOUT_SITE_MLM, thresh, 1.f);
  hipLaunchKernelGGL(mlm_mask_kernel, dim3(1), dim3(1024), 0, stream, ids, attn, tok_row, ids_masked, labels, rows, row_labels, count, B, T, V,
                     cls_id, sep_id, pad_id, mask_id, sample_offset, rng);
  return mm_check_launch();
}

static int rows_launch(int mode, const void* src, const void* aux, const int* rows, const int* count, void* dst, int M_bound, int D,
                       hipStream_t stream) {
  if (!src || !count || !dst || (mode != 2 && !rows) || (mode == 2 && !aux)) return MM_ERR_ARG;
  if (M_bound < 1 || D < 8 || D % 8) return MM_ERR_SHAPE;
  if (!aligned16(src) || !aligned16(dst) || (aux && !aligned16(aux))) return MM_ERR_ARG;
  const int grid = (int)min(((long long)M_bound * (D >> 3) + 255) / 256, 4096ll);
  if (mode == 0)
    hipLaunchKernelGGL(mlm_rows_kernel<0>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)src, (const bf16_t*)aux, rows, count, (bf16_t*)dst, M_bound, D);
  else if (mode == 1)
    hipLaunchKernelGGL(mlm_rows_kernel<1>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)src, (const bf16_t*)aux, rows, count, (bf16_t*)dst, M_bound, D);
  else
    hipLaunchKernelGGL(mlm_rows_kernel<2>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)src, (const bf16_t*)aux, rows, count, (bf16_t*)dst, M_bound, D);
  return mm_check_launch();
}

extern "C" int medmoe_rows_gather(const void* src, const int* rows, const int* count, void* dst, int M_bound, int D, hipStream_t stream) {
  return rows_launch(0, src, nullptr, rows, count, dst, M_bound, D, stream);
}
extern "C" int medmoe_rows_scatter_add(const void* src, const int* rows, const int* count, void* dst, int M_bound, int D, hipStream_t stream) {
  return rows_launch(1, src, nullptr, rows, count, dst, M_bound, D, stream);
}
extern "C" int medmoe_rows_mul(const void* a, const void* b, const int* count, void* dst, int M_bound, int D, hipStream_t stream) {
  return rows_launch(2, a, b, nullptr, count, dst, M_bound, D, stream);
}

extern "C" long long medmoe_vocab_ce_scratch(int M_bound, int V, int D) {
  if (!ce_shape_ok(M_bound, V, D)) return 0;
  return (2ll * fwd_tiles(V) + 2) * M_bound;
}

extern "C" int medmoe_vocab_ce_fwd(const void* z, const void* E, const float* bias, const int* row_labels, const int* count, float loss_scale,
                                   float* lse, float* terms, float* loss, int* counts, float* scratch, long long scratch_floats, int M_bound,
                                   int V, int D, hipStream_t stream) {
  if (!z || !E || !bias || !row_labels || !count || !lse || !terms || !loss || !counts || !scratch) return MM_ERR_ARG;
  if (!ce_shape_ok(M_bound, V, D)) return MM_ERR_SHAPE;
  if (!aligned16(z) || !aligned16(E) || scratch_floats < medmoe_vocab_ce_scratch(M_bound, V, D)) return MM_ERR_ARG;
  const int NT = fwd_tiles(V);
  float* pmax = scratch;
  float* psum = pmax + (long long)M_bound * NT;
  float* tgt = psum + (long long)M_bound * NT;
  int* hits = (int*)(tgt + M_bound);
  if (hipMemsetAsync(tgt, 0, (size_t)M_bound * sizeof(float), stream) != hipSuccess) return MM_ERR_LAUNCH;      // a label outside [0, V) finds no logit
  hipLaunchKernelGGL(vocab_ce_fwd_kernel, dim3(NT, (M_bound + 63) / 64), dim3(256), 0, stream, (const bf16_t*)z, (const bf16_t*)E, bias, row_labels,
                     count, pmax, psum, tgt, M_bound, V, D, NT);
  hipLaunchKernelGGL(vocab_ce_rows_kernel, dim3((M_bound + 255) / 256), dim3(256), 0, stream, pmax, psum, tgt, count, lse, terms, hits, M_bound, NT);
  hipLaunchKernelGGL(vocab_ce_loss_kernel, dim3(1), dim3(1024), 0, stream, terms, hits, count, loss_scale, loss, counts, M_bound);
  return mm_check_launch();
}

extern "C" int medmoe_vocab_ce_bwd_dx(const void* z, const void* E, const float* bias, const int* row_labels, const float* lse, const int* count,
                                      float loss_scale, void* dz, int M_bound, int V, int D, hipStream_t stream) {
  if (!z || !E || !bias || !row_labels || !lse || !count || !dz) return MM_ERR_ARG;
  if (!ce_shape_ok(M_bound, V, D)) return MM_ERR_SHAPE;
  if (!aligned16(z) || !aligned16(E)) return MM_ERR_ARG;
  launch_bwd<false>((M_bound + 63) / 64, stream, (const bf16_t*)z, (const bf16_t*)E, bias, row_labels, lse, count, loss_scale, (bf16_t*)dz, nullptr,
                    nullptr, M_bound, V, D);
  return mm_check_launch();
}

extern "C" int medmoe_vocab_ce_bwd_dw(const void* z, const void* E, const float* bias, const int* row_labels, const float* lse, const int* count,
                                      float loss_scale, float* dE, float* dbias, int M_bound, int V, int D, hipStream_t stream) {
  if (!z || !E || !bias || !row_labels || !lse || !count || !dE || !dbias) return MM_ERR_ARG;
  if (!ce_shape_ok(M_bound, V, D)) return MM_ERR_SHAPE;
  if (!aligned16(z) || !aligned16(E)) return MM_ERR_ARG;
  launch_bwd<true>((V + 63) / 64, stream, (const bf16_t*)z, (const bf16_t*)E, bias, row_labels, lse, count, loss_scale, nullptr, dE, dbias, M_bound, V,
                   D);
  return mm_check_launch();
}
