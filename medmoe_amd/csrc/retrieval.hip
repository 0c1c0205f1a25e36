// Retrieval and zero-shot evaluation: row L2 normalisation, and ONE streaming similarity kernel with two epilogues - the K best
// keys of every query (medmoe_sim_topk) and the rank of one target key per query (medmoe_sim_rank).  The [Nq][Nk] score matrix is never
// stored: scores live in MFMA accumulators, the lists / counts in registers.
//
// Ownership.  A workgroup of 4 waves owns 64 queries (16 per wave) and one contiguous chunk of the keys (blockIdx.y of S splits).  Scores
// come from v_mfma_f32_16x16x4_f32 with the keys on the M side and the queries on the N side: lane l supplies key[16 a + (l & 15)][4 kk + (l >> 4)]
// as A and q[l & 15][4 kk + (l >> 4)] as B, and accumulator a then holds, in register r of lane l, the score of query (l & 15) against key
// 16 a + 4 (l >> 4) + r of the tile.  Four accumulators per wave (64 keys per tile) are independent chains, which also covers the
// instruction's dependent latency.  Every score is ONE chain over D in ascending order starting from zero: the same bits as an fmaf chain, a
// function of its (query, key) pair alone - not of the tile, the split, the accumulator or the lane that computed it.
//
// The wave's query fragment stays in registers for the whole key stream (D / 4 VGPRs; kernels are instantiated for D = 64 .. 1024 in the
// sizes below, any other multiple of 64 re-reads the fragment through the cache).  Key tiles of 64 keys x 64 floats pass through a
// double-buffered LDS ring, rows padded to 68 floats: the fragment read of lane (m, g) hits bank (4 m + g) % 64, all distinct.  The next
// chunk is fetched into registers before the MFMAs of the current one and stored after them: one barrier per chunk.
//
// Out-of-range queries and keys are zero rows (the MFMAs run with full EXEC); their candidates are dropped by INDEX, never by score.
#include "common.h"
#include "medmoe_hip.h"
#include "topk_list.h"

namespace {

constexpr int LDT = 68;                       // floats per key row of an LDS tile (64 + 4 pad)
constexpr int TILE_FLOATS = 64 * LDT;
constexpr int EPI_TOPK = 0, EPI_RANK = 1;
constexpr int MAX_SPLITS = 64;

// DQ = D / 64 with the query fragment in registers, 0 = any D (fragment re-read from memory).
// TOPK: out_val / out_idx [Nq][S][K] (S = gridDim.y; the final arrays themselves when S == 1, `fin` set: empty slots leave as -1).
// RANK: out_idx [Nq][S] = keys of this chunk ordered before keys[target[q]].
template <int DQ, int EPI>
__global__ __launch_bounds__(256) void sim_stream_kernel(const float* __restrict__ q, const float* __restrict__ keys, const int* __restrict__ target,
                                                         int Nq, int Nk, int D, int K, int tiles_per, float* __restrict__ out_val,
                                                         int* __restrict__ out_idx, int fin) {
  __shared__ __attribute__((aligned(16))) float tile[2 * TILE_FLOATS];
  constexpr bool RES = DQ > 0;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int S = gridDim.y, s = blockIdx.y;
  const int qrow = blockIdx.x * 64 + wave * 16 + n;
  const bool qok = qrow < Nq;
  const int DC = RES ? DQ : D / 64;
  const long long k0 = (long long)s * tiles_per * 64;
  const int kbeg = (int)(k0 < Nk ? k0 : Nk);
  const int kend = (int)(k0 + (long long)tiles_per * 64 < Nk ? k0 + (long long)tiles_per * 64 : Nk);
  const int ntiles = (kend - kbeg + 63) / 64;
  const int srow = tid >> 4, scol = (tid & 15) * 4;         // staging: rows srow + 16 i, one float4 each

  float qf[RES ? DQ * 16 : 1];
  const float* qp = q + (long long)(qok ? qrow : 0) * D + g;
  if (RES) {
#pragma unroll
    for (int kk = 0; kk < (RES ? DQ * 16 : 1); ++kk) qf[kk] = qok ? qp[4 * kk] : 0.f;
  }

  // global offsets of the rows this thread stages for tile t (-1: a zero row).  t = -1 is the gathered tile of the RANK epilogue: row j
  // holds keys[target[64 blockIdx.x + j]], so that the target's score is computed by the very instructions that compute the streamed ones.
  auto tile_rows = [&](int t, long long (&off)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = srow + 16 * i;
      long long o = -1;
      if (t < 0) {
        const int qi = blockIdx.x * 64 + r;
        if (qi < Nq) {
          const int tg = target[qi];
          if (tg >= 0 && tg < Nk) o = (long long)tg * D + scol;
        }
      } else {
        const int kj = kbeg + t * 64 + r;
        if (kj < kend) o = (long long)kj * D + scol;
      }
      off[i] = o;
    }
  };
  auto fetch = [&](const long long (&off)[4], int c, float4 (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = off[i] >= 0 ? *(const float4*)(keys + off[i] + c * 64) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto stash = [&](int buf, const float4 (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *(float4*)(tile + buf * TILE_FLOATS + (srow + 16 * i) * LDT + scol) = r[i];
  };

  float val[TOPK_MAX]; int idx[TOPK_MAX];
  float thr_v = -INFINITY; int thr_i = TOPK_EMPTY;           // the list's K-th entry
  if (EPI == EPI_TOPK) topk_init(val, idx);
  int count = 0; float tgt_v = 0.f; int tgt_i = -1;
  if (EPI == EPI_RANK && qok) tgt_i = target[qrow];

  if (ntiles > 0) {
    long long off[4]; float4 pre[4];
    const int t0 = EPI == EPI_RANK ? -1 : 0;
    tile_rows(t0, off); fetch(off, 0, pre); stash(0, pre);
    __syncthreads();
    int it = 0;
    for (int t = t0; t < ntiles; ++t) {
      f32x4_t acc[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) acc[a] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < DC; ++c, ++it) {
        const bool last_c = c + 1 == DC;
        const bool more = !last_c || t + 1 < ntiles;           // uniform over the workgroup
        if (last_c && more) tile_rows(t + 1, off);
        if (more) fetch(off, last_c ? 0 : c + 1, pre);
        const float* tb = tile + (it & 1) * TILE_FLOATS + n * LDT + g;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
          const float b = RES ? qf[RES ? c * 16 + kk : 0] : (qok ? qp[c * 64 + 4 * kk] : 0.f);
#pragma unroll
          for (int a = 0; a < 4; ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(tb[a * 16 * LDT + 4 * kk], b, acc[a], 0, 0, 0);
        }
        if (more) stash((it + 1) & 1, pre);
        __syncthreads();
      }
      const int kb = kbeg + t * 64 + 4 * g;                   // key of (a, r): kb + 16 a + r
      if (EPI == EPI_TOPK) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int kj = kb + 16 * a + r;
            const float v = acc[a][r];
            const bool cand = kj < kend && topk_before(v, kj, thr_v, thr_i);
            if (__any(cand)) {                                 // wave-wide skip: past the first tiles almost nothing enters a list
              if (cand) topk_insert(val, idx, K, v, kj);
              topk_kth(val, idx, K, thr_v, thr_i);
            }
          }
      } else if (t < 0) {
        // the diagonal of the gathered tile: query n of wave w against row 16 w + n, i.e. accumulator w, lane (n, g = n >> 2), register n & 3
        float d = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (a == wave && r == (n & 3)) d = acc[a][r];
        tgt_v = __shfl(d, n + 16 * (n >> 2), 64);
      } else {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int kj = kb + 16 * a + r;
            count += (kj < kend && topk_before(acc[a][r], kj, tgt_v, tgt_i)) ? 1 : 0;
          }
      }
    }
  }

  if (EPI == EPI_RANK) {
    count += __shfl_xor(count, 16, 64);
    count += __shfl_xor(count, 32, 64);
    if (g == 0 && qok) out_idx[(long long)qrow * S + s] = count;
    return;
  }

  // the four lanes of a query (g = 0 .. 3) meet in LDS; lane g = 0 merges.  The ring is free: the loop ended on a barrier.
  float* lv = tile;
  int* li = (int*)(tile + 256 * TOPK_MAX);
#pragma unroll
  for (int i = 0; i < TOPK_MAX; ++i) { lv[tid * TOPK_MAX + i] = val[i]; li[tid * TOPK_MAX + i] = idx[i]; }
  __syncthreads();
  if (g == 0 && qok) {
    for (int gg = 1; gg < 4; ++gg) topk_merge(val, idx, K, lv + (tid + 16 * gg) * TOPK_MAX, li + (tid + 16 * gg) * TOPK_MAX, K);
    const long long o = ((long long)qrow * S + s) * K;
#pragma unroll
    for (int i = 0; i < TOPK_MAX; ++i)
      if (i < K) {
        out_val[o + i] = val[i];
        out_idx[o + i] = (fin && idx[i] == TOPK_EMPTY) ? -1 : idx[i];
      }
  }
}

// one thread per query: the S partial lists of `part` [Nq][S][K] merged under the same order
__global__ __launch_bounds__(64) void topk_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int Nq, int S, int K,
                                                        float* __restrict__ top_val, int* __restrict__ top_idx) {
  const int qi = blockIdx.x * 64 + threadIdx.x;
  if (qi >= Nq) return;
  float val[TOPK_MAX]; int idx[TOPK_MAX];
  topk_init(val, idx);
  for (int s = 0; s < S; ++s) {
    const long long o = ((long long)qi * S + s) * K;
    topk_merge(val, idx, K, pv + o, pi + o, K);
  }
#pragma unroll
  for (int i = 0; i < TOPK_MAX; ++i)
    if (i < K) {
      top_val[(long long)qi * K + i] = val[i];
      top_idx[(long long)qi * K + i] = idx[i] == TOPK_EMPTY ? -1 : idx[i];
    }
}

__global__ __launch_bounds__(64) void rank_sum_kernel(const int* __restrict__ part, int Nq, int S, int* __restrict__ rank) {
  const int qi = blockIdx.x * 64 + threadIdx.x;
  if (qi >= Nq) return;
  int c = 0;
  for (int s = 0; s < S; ++s) c += part[(long long)qi * S + s];
  rank[qi] = c;
}

// one wave per row; the sum of squares in double, so that the norm is rounded to fp32 once and the quotient once
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ x, float* __restrict__ y, int rows, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (long long)row * D;
  float* yr = y + (long long)row * D;
  double ss = 0.0;
  for (int c = lane; c < D; c += 64) { const double v = xr[c]; ss += v * v; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float nrm = fmaxf((float)sqrt(ss), eps);
  for (int c = lane; c < D; c += 64) yr[c] = xr[c] / nrm;    // each element is read and written by the same lane: y may be x
}

int g_sim_splits = 0;

int pick_splits(int Nq, int Nk) {
  const int qt = (Nq + 63) / 64, kt = (Nk + 63) / 64;
  int s = g_sim_splits > 0 ? g_sim_splits : min((256 + qt - 1) / qt, kt);      // one workgroup per CU of the 256; a split holds >= 1 tile
  return max(1, min(s, MAX_SPLITS));
}

template <int EPI>
int launch_stream(const float* q, const float* keys, const int* target, int Nq, int Nk, int D, int K, int S, float* ov, int* oi, int fin,
                  hipStream_t stream) {
  const int kt = (Nk + 63) / 64, tiles_per = (kt + S - 1) / S;
  const dim3 grid((Nq + 63) / 64, S), block(256);
#define SIM_LAUNCH(DQ) hipLaunchKernelGGL((sim_stream_kernel<DQ, EPI>), grid, block, 0, stream, q, keys, target, Nq, Nk, D, K, tiles_per, ov, oi, fin)
  switch (D / 64) {
    case 1: SIM_LAUNCH(1); break;
    case 2: SIM_LAUNCH(2); break;
    case 4: SIM_LAUNCH(4); break;
    case 8: SIM_LAUNCH(8); break;
    case 12: SIM_LAUNCH(12); break;
    case 16: SIM_LAUNCH(16); break;
    default: SIM_LAUNCH(0); break;
  }
#undef SIM_LAUNCH
  return mm_check_launch();
}

}  // namespace

extern "C" int medmoe_sim_topk_splits(int n) {
  if (n < 0) return MM_ERR_ARG;
  g_sim_splits = n;
  return MM_OK;
}

extern "C" long long medmoe_sim_topk_scratch(int Nq, int Nk, int D, int K) {
  if (Nq <= 0 || Nk <= 0 || D <= 0 || K < 1 || K > TOPK_MAX) return 0;
  const int S = pick_splits(Nq, Nk);
  return S == 1 ? 0 : 2ll * Nq * S * K;
}

extern "C" int medmoe_l2_normalize(const float* x, float* y, int rows, int D, float eps, hipStream_t stream) {
  if (!x || !y) return MM_ERR_ARG;
  if (rows < 0 || D <= 0) return MM_ERR_SHAPE;
  if (rows == 0) return MM_OK;
  hipLaunchKernelGGL(l2_normalize_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, y, rows, D, eps);
  return mm_check_launch();
}

extern "C" int medmoe_sim_topk(const float* q, const float* keys, int Nq, int Nk, int D, int K, float* top_val, int* top_idx, float* scratch,
                               long long scratch_elems, hipStream_t stream) {
  if (!q || !keys || !top_val || !top_idx) return MM_ERR_ARG;
  if (Nq <= 0 || Nk <= 0 || D <= 0 || D % 64 || K < 1 || K > TOPK_MAX) return MM_ERR_SHAPE;
  const int S = pick_splits(Nq, Nk);
  if (S == 1) return launch_stream<EPI_TOPK>(q, keys, nullptr, Nq, Nk, D, K, 1, top_val, top_idx, 1, stream);
  const long long half = (long long)Nq * S * K;
  if (!scratch || scratch_elems < 2 * half) return MM_ERR_ARG;
  float* pv = scratch;
  int* pi = (int*)(scratch + half);
  const int rc = launch_stream<EPI_TOPK>(q, keys, nullptr, Nq, Nk, D, K, S, pv, pi, 0, stream);
  if (rc != MM_OK) return rc;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((Nq + 63) / 64), dim3(64), 0, stream, pv, pi, Nq, S, K, top_val, top_idx);
  return mm_check_launch();
}

extern "C" int medmoe_sim_rank(const float* q, const float* keys, const int* target, int Nq, int Nk, int D, int* rank, float* scratch,
                               long long scratch_elems, hipStream_t stream) {
  if (!q || !keys || !target || !rank) return MM_ERR_ARG;
  if (Nq <= 0 || Nk <= 0 || D <= 0 || D % 64) return MM_ERR_SHAPE;
  const int S = pick_splits(Nq, Nk);
  if (S == 1) return launch_stream<EPI_RANK>(q, keys, target, Nq, Nk, D, 1, 1, nullptr, rank, 1, stream);
  if (!scratch || scratch_elems < (long long)Nq * S) return MM_ERR_ARG;
  int* part = (int*)scratch;
  const int rc = launch_stream<EPI_RANK>(q, keys, target, Nq, Nk, D, 1, S, nullptr, part, 0, stream);
  if (rc != MM_OK) return rc;
  hipLaunchKernelGGL(rank_sum_kernel, dim3((Nq + 63) / 64), dim3(64), 0, stream, part, Nq, S, rank);
  return mm_check_launch();
}
