// Supervised image classification: a linear head on the global image embedding with its loss and backward, and the pair counts of
// the Mann-Whitney AUROC.  Everything is fp32; no fp32 atomic anywhere - the loss is summed from per-row terms in a fixed order
// (mm_launch_det_sum), dW / db leave as per-row-range records summed in range order - so two runs give the same bits and
// medmoe_nondet_launches() never moves.  The only atomics are integer adds (row / element counts, pair counts): order-independent, exact.
//
// Head, N rows x D features x C <= 64 classes: a class maps to a LANE.  medmoe_cls_head_step is three small memsets, these four launches
// and the loss sum:
//   1. cls_count_kernel    |V| (rows with a target >= 0) or |K| (elements with a target >= 0) into counts[0], integer adds
//   2. cls_row_kernel      one pass over the features: a wave owns 4 rows at a time, holds them in registers (float4 per lane: columns
//                          256 j + 4 lane), forms z_c = <x, W_c> + b_c by a wave reduction per class and leaves it in lane c; the softmax /
//                          sigmoid, the row's loss term and dz_c are then lane-local + wave reductions.  z and dz [N][C] are stored, the
//                          loss term goes to parts[row], dx = dz W is formed from the same W rows (dz_c broadcast from lane c) and WRITTEN.
//                          W is staged in LDS once per workgroup when C D <= 16384 floats, read through the caches otherwise.
//   3. cls_wgrad_kernel    the second (and last) read of the features: workgroup (s, t) owns the row range s and the column tile t, a lane
//                          1 / 2 / 4 columns with C accumulators each, dz[row][c] is wave-uniform; its four waves take rows lo + w,
//                          lo + w + 4, ... and meet in LDS in wave order; the record [C][D] (+ the C sums of dz behind it) is stored, not added
//   4. cls_wgrad_sum_kernel  dW[i] += rec[0][i] + rec[1][i] + ... in range order, db likewise
// The loss goes through mm_launch_det_sum, in two stages past 1024 rows: that helper sums a segment with ONE workgroup.  Nothing of size
// [N][C][D] exists.  medmoe_cls_head_logits is launch 2 without the loss half.
#include "common.h"
#include "medmoe_hip.h"

namespace {

constexpr int TASK_MULTICLASS = 0, TASK_MULTILABEL = 1;
constexpr int RW = 4;                          // rows a wave holds at a time
constexpr int W_LDS_MAX = 16384;               // floats of W a workgroup stages in LDS (64 KiB)
constexpr int MAX_RECORDS = 256;               // row ranges of the staged dW / db, fewer where 256 records would pass 16 Mi floats
constexpr int REC_PAD = 64;                    // floats behind a record's [C][D]: the C sums of dz
constexpr int LOSS_SEG = 1024;                 // row terms per segment of the loss sum's first stage

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The sum of v over the 64 lanes, the same value in every lane, on the vector ALU alone: an inclusive scan along each row of 16 lanes
// (row_shr 1, 2, 4, 8), row 0's total into row 1 and row 2's into row 3 (row_bcast:15), lane 31's into rows 2 and 3 (row_bcast:31); lane
// 63 then holds the total and one v_readlane hands it to all.  wave_sum (six __shfl_xor = six LDS crossbar ops) costs the row pass its
// C reductions per row several times over.  Must be reached by all 64 lanes.
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, BOUND));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v = dpp_add<0x111, 0xf, true>(v);
  v = dpp_add<0x112, 0xf, true>(v);
  v = dpp_add<0x114, 0xf, true>(v);
  v = dpp_add<0x118, 0xf, true>(v);
  v = dpp_add<0x142, 0xa, false>(v);
  v = dpp_add<0x143, 0xc, false>(v);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// counts[0] += #{i < n : target_i >= 0}; targets are int32 (multiclass, one per row) or int8 (multilabel, one per element).  The body is read
// 16 bytes per lane (the base is 16-byte aligned, checked by the host): an element is counted when its sign bit is clear.
__global__ __launch_bounds__(256) void cls_count_kernel(const void* __restrict__ targets, long long n, int task, int* __restrict__ counts) {
  const int per = task == TASK_MULTICLASS ? 4 : 16;           // elements per 16 bytes
  const unsigned sign = task == TASK_MULTICLASS ? 0x80000000u : 0x80808080u;
  const long long nvec = n / per;
  int c = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
    const uint4 w = ((const uint4*)targets)[i];
    c += per - (__popc(w.x & sign) + __popc(w.y & sign) + __popc(w.z & sign) + __popc(w.w & sign));
  }
  if (blockIdx.x == 0)
    for (long long i = nvec * per + threadIdx.x; i < n; i += 256)
      c += task == TASK_MULTICLASS ? (((const int*)targets)[i] >= 0) : (((const int8_t*)targets)[i] >= 0);
  c = wave_sum_int(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(counts, c);
}

// J4: float4 per lane and row (D <= 256 J4).  GRAD: the loss half (counts[0] holds |V| / |K| already).  WLDS: W staged in dynamic LDS.
template <int J4, int TASK, bool GRAD, bool WLDS>
__global__ __launch_bounds__(256) void cls_row_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ b,
                                                      const void* __restrict__ targets, const float* __restrict__ pos_weight, float smooth,
                                                      float loss_scale, int* __restrict__ counts, float* __restrict__ z, float* __restrict__ dz,
                                                      float* __restrict__ dx, float* __restrict__ parts, int N, int D, int C) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (WLDS) {
    for (int i = tid * 4; i < C * D; i += 1024) *(float4*)(wl + i) = *(const float4*)(W + i);
    __syncthreads();
  }
  const float* Wp = WLDS ? wl : W;
  const bool cls = lane < C;
  const float bias = cls ? b[lane] : 0.f;
  float scale = 0.f;
  if (GRAD) {
    const int nv = counts[0];
    scale = nv > 0 ? loss_scale / (float)nv : 0.f;           // nothing counted: L = 0, dz = 0
  }
  const float pw = (GRAD && TASK == TASK_MULTILABEL && pos_weight && cls) ? pos_weight[lane] : 1.f;
  int correct = 0;
  const int ngroups = (N + 4 * RW - 1) / (4 * RW);
  for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int r0 = g * 4 * RW + wave * RW;
    float4 xv[RW][J4];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int j = 0; j < J4; ++j) {
        // every load is issued unconditionally from a clamped address (a row past N repeats row N - 1 and is dropped later, a column
        // past D repeats the row's first columns and meets a zero of W): a load under a branch - which is what the compiler makes of
        // `ok ? load : 0` - is waited for before the next one is issued, and the twelve loads of a group then run one after the other
        const int col = 256 * j + 4 * lane;
        xv[r][j] = *(const float4*)(x + (long long)min(r0 + r, N - 1) * D + (col < D ? col : 0));
      }
    float zr[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) zr[r] = bias;
    for (int c = 0; c < C; ++c) {
      float4 w[J4];
#pragma unroll
      for (int j = 0; j < J4; ++j) {
        const int col = 256 * j + 4 * lane;
        const float m = col < D ? 1.f : 0.f;                  // a product, not a select: the load stays out of a branch
        const float4 v = *(const float4*)(Wp + c * D + (col < D ? col : 0));
        w[j] = make_float4(v.x * m, v.y * m, v.z * m, v.w * m);
      }
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < J4; ++j) p += dot4(xv[r][j], w[j]);
        p = wave_sum_dpp(p);
        if (lane == c) zr[r] += p;
      }
    }
    float dzv[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int row = r0 + r;                                 // wave-uniform
      dzv[r] = 0.f;
      if (row >= N) continue;
      const float zc = zr[r];
      if (cls) z[(long long)row * C + lane] = zc;
      if (!GRAD) continue;
      float term = 0.f, d = 0.f;
      if (TASK == TASK_MULTICLASS) {
        const int y = ((const int*)targets)[row];
        const float m = wave_max(cls ? zc : -INFINITY);
        const float e = cls ? expf(zc - m) : 0.f;
        const float s = wave_sum_dpp(e);
        const float q = (1.f - smooth) * (lane == y ? 1.f : 0.f) + smooth / (float)C;
        const float t = wave_sum_dpp(cls ? -q * (zc - m - logf(s)) : 0.f);
        const int best = __ffsll((unsigned long long)__ballot(cls && zc == m)) - 1;      // ties: the lowest class
        if (y >= 0) {
          term = t;
          d = cls ? scale * (e / s - q) : 0.f;
          correct += best == y;
        }
      } else {
        const int t = cls ? (int)((const int8_t*)targets)[(long long)row * C + lane] : -1;
        const bool on = t >= 0;
        const float tf = (float)t, az = fabsf(zc);
        const float e = expf(-az), l1p = log1pf(e);
        const float sp = fmaxf(zc, 0.f) + l1p, sn = fmaxf(-zc, 0.f) + l1p;               // softplus(z), softplus(-z)
        const float sig_hi = 1.f / (1.f + e), sig_lo = e / (1.f + e);                      // sigmoid(|z|), sigmoid(-|z|)
        const float sg = zc >= 0.f ? sig_hi : sig_lo, sgn = zc >= 0.f ? sig_lo : sig_hi;   // sigmoid(z), sigmoid(-z)
        term = wave_sum_dpp(on ? pw * tf * sn + (1.f - tf) * sp : 0.f);
        d = on ? scale * ((1.f - tf) * sg - pw * tf * sgn) : 0.f;
        correct += __popcll((unsigned long long)__ballot(on && (zc > 0.f) == (t == 1)));
      }
      dzv[r] = d;
      if (cls) dz[(long long)row * C + lane] = d;
      if (lane == 0) parts[row] = scale * term;
    }
    if (GRAD && dx) {
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int j = 0; j < J4; ++j) xv[r][j] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int c = 0; c < C; ++c) {
        float4 w[J4];
#pragma unroll
        for (int j = 0; j < J4; ++j) {
          const int col = 256 * j + 4 * lane;
          const float m = col < D ? 1.f : 0.f;                  // a product, not a select: the load stays out of a branch
        const float4 v = *(const float4*)(Wp + c * D + (col < D ? col : 0));
        w[j] = make_float4(v.x * m, v.y * m, v.z * m, v.w * m);
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          const float d = __shfl(dzv[r], c, 64);
#pragma unroll
          for (int j = 0; j < J4; ++j) {
            xv[r][j].x += d * w[j].x; xv[r][j].y += d * w[j].y; xv[r][j].z += d * w[j].z; xv[r][j].w += d * w[j].w;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int j = 0; j < J4; ++j) {
          const int col = 256 * j + 4 * lane;
          if (r0 + r < N && col < D) *(float4*)(dx + (long long)(r0 + r) * D + col) = xv[r][j];
        }
    }
  }
  if (GRAD && lane == 0 && correct) atomicAdd(counts + 1, correct);
}

// rec[s][c][col] = sum over the rows of range s of dz[row][c] x[row][col], rec[s][C D + c] = sum of dz[row][c]: stored, one writer each.
// A lane owns VEC consecutive columns (64 VEC columns per workgroup; CT VEC = 64 accumulators per lane) and a wave keeps 8 row loads
// (8 x 64 x VEC floats) in flight: the pass is bound by how many bytes a CU has outstanding, not by its C FMAs per element.
template <int CT, int VEC>
__global__ __launch_bounds__(256) void cls_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ rec, int N,
                                                        int D, int C, int rows_per, long long rec_stride) {
  typedef float vec_t __attribute__((ext_vector_type(VEC)));
  constexpr int UR = 8;
  __shared__ __attribute__((aligned(16))) float red[CT][64 * VEC];
  __shared__ float redb[64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int s = blockIdx.x, col = blockIdx.y * 64 * VEC + lane * VEC;
  const bool colok = col < D;                                 // D % 64 == 0 and VEC divides 64: a lane's columns are all in or all out
  const int lo = s * rows_per, hi = min(N, lo + rows_per);
  vec_t acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = (vec_t)(0.f);
  float bsum = 0.f;
#pragma unroll 1
  for (int r = lo + wave; r < hi; r += 4 * UR) {
    vec_t xv[UR];
#pragma unroll
    for (int i = 0; i < UR; ++i)
      xv[i] = *(const vec_t*)(x + (long long)min(r + 4 * i, hi - 1) * D + (colok ? col : 0));   // clamped, never under a branch; rows past hi are skipped below
#pragma unroll
    for (int i = 0; i < UR; ++i) {
      if (r + 4 * i < hi) {                                   // wave-uniform
        const float* dr = dz + (long long)(r + 4 * i) * C;
        bsum += lane < C ? dr[lane] : 0.f;
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < C) acc[c] += dr[c] * xv[i];
      }
    }
  }
  for (int w = 1; w < 4; ++w) {                               // ((wave 0 + wave 1) + wave 2) + wave 3
    if (wave == w) {
#pragma unroll
      for (int c = 0; c < CT; ++c) *(vec_t*)(&red[c][lane * VEC]) = acc[c];
      redb[lane] = bsum;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] += *(const vec_t*)(&red[c][lane * VEC]);
      bsum += redb[lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* out = rec + (long long)s * rec_stride;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C && colok) *(vec_t*)(out + (long long)c * D + col) = acc[c];
    if (blockIdx.y == 0 && lane < C) out[(long long)C * D + lane] = bsum;
  }
}

__global__ __launch_bounds__(256) void cls_wgrad_sum_kernel(const float* __restrict__ rec, int S, long long rec_stride, float* __restrict__ dW,
                                                            float* __restrict__ db, int CD, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= CD + C) return;
  float v = 0.f;
  for (int s = 0; s < S; s += 8) {                            // eight loads in flight, added in record order
    float t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = s + k < S ? rec[(long long)(s + k) * rec_stride + i] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += t[k];
  }
  if (i < CD) dW[i] += v; else db[i - CD] += v;
}

// One class (blockIdx.y), 256 rows i (blockIdx.x) against the rows j of split blockIdx.z: a thread keeps the score of its row when that
// row is a positive (NaN otherwise: every comparison with it is false), the negatives' scores pass through LDS 256 at a time (NaN for a
// row that is no negative) and every thread counts s_j < s_i and s_j == s_i.  Split 0 also counts its rows' positives and negatives.
__global__ __launch_bounds__(256) void auroc_kernel(const float* __restrict__ sc, const int8_t* __restrict__ tg, int N, int C, int chunk,
                                                    unsigned long long* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float neg[256];
  const int tid = threadIdx.x, c = blockIdx.y;
  const int i = blockIdx.x * 256 + tid;
  const int ti = i < N ? (int)tg[(long long)i * C + c] : -1;
  const float si = ti == 1 ? sc[(long long)i * C + c] : NAN;
  const long long j0 = (long long)blockIdx.z * chunk;
  const int jbeg = (int)(j0 < N ? j0 : N), jend = (int)(j0 + chunk < N ? j0 + chunk : N);
  unsigned less = 0, eq = 0;
  for (int jb = jbeg; jb < jend; jb += 256) {
    const int j = jb + tid;
    float v = NAN;
    if (j < jend && tg[(long long)j * C + c] == 0) v = sc[(long long)j * C + c];
    __syncthreads();                                          // the previous tile has been read
    neg[tid] = v;
    __syncthreads();
    if (__any(ti == 1)) {
#pragma unroll 8
      for (int k = 0; k < 256; k += 4) {
        const float4 q = *(const float4*)(neg + k);
        less += (q.x < si) + (q.y < si) + (q.z < si) + (q.w < si);
        eq += (q.x == si) + (q.y == si) + (q.z == si) + (q.w == si);
      }
    }
  }
  unsigned long long l64 = less, e64 = eq;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    l64 += __shfl_xor(l64, o, 64);
    e64 += __shfl_xor(e64, o, 64);
  }
  const int np = __popcll((unsigned long long)__ballot(ti == 1)), nn = __popcll((unsigned long long)__ballot(ti == 0));
  if ((tid & 63) == 0) {
    unsigned long long* o = out + 4ll * c;
    if (blockIdx.z == 0 && np) atomicAdd(o + 0, (unsigned long long)np);
    if (blockIdx.z == 0 && nn) atomicAdd(o + 1, (unsigned long long)nn);
    if (l64) atomicAdd(o + 2, l64);
    if (e64) atomicAdd(o + 3, e64);
  }
}

inline long long align4(long long n) { return (n + 3) / 4 * 4; }
inline int rows_per_record(int N, int D, int C) {
  const int cap = (int)max(1ll, min((long long)MAX_RECORDS, (16ll << 20) / ((long long)C * D)));
  return max(64, (N + cap - 1) / cap);
}
inline bool head_shape_ok(int N, int D, int C) { return N >= 1 && D >= 64 && D % 64 == 0 && D <= 2048 && C >= 1 && C <= 64; }

template <int TASK, bool GRAD>
void launch_rows(const float* x, const float* W, const float* b, const void* targets, const float* pw, float smooth, float loss_scale,
                 int* counts, float* z, float* dz, float* dx, float* parts, int N, int D, int C, hipStream_t stream) {
  const int ngroups = (N + 4 * RW - 1) / (4 * RW);
  const bool wlds = C * D <= W_LDS_MAX;
  const dim3 grid(min(ngroups, 1024)), block(256);
  const size_t lds = wlds ? (size_t)C * D * sizeof(float) : 0;
#define CLS_ROWS(J4)                                                                                                                          \
  do {                                                                                                                                        \
    if (wlds) hipLaunchKernelGGL((cls_row_kernel<J4, TASK, GRAD, true>), grid, block, lds, stream, x, W, b, targets, pw, smooth, loss_scale,   \
                                 counts, z, dz, dx, parts, N, D, C);                                                                          \
    else hipLaunchKernelGGL((cls_row_kernel<J4, TASK, GRAD, false>), grid, block, 0, stream, x, W, b, targets, pw, smooth, loss_scale, counts, \
                            z, dz, dx, parts, N, D, C);                                                                                       \
  } while (0)
  const int j4 = (D + 255) / 256;
  if (j4 <= 1) CLS_ROWS(1);
  else if (j4 == 2) CLS_ROWS(2);
  else if (j4 == 3) CLS_ROWS(3);
  else if (j4 == 4) CLS_ROWS(4);
  else if (j4 <= 6) CLS_ROWS(6);
  else CLS_ROWS(8);
#undef CLS_ROWS
}

}  // namespace

extern "C" long long medmoe_cls_head_scratch(int N, int D, int C) {
  if (!head_shape_ok(N, D, C)) return 0;
  const int rp = rows_per_record(N, D, C), S = (N + rp - 1) / rp;
  const long long nseg = (N + LOSS_SEG - 1) / LOSS_SEG;
  return align4((long long)N * C) + nseg * LOSS_SEG + align4(nseg) + (long long)S * ((long long)C * D + REC_PAD);
}

extern "C" int medmoe_cls_head_logits(const float* x, const float* W, const float* b, float* z, int N, int D, int C, hipStream_t stream) {
  if (!x || !W || !b || !z) return MM_ERR_ARG;
  if (!head_shape_ok(N, D, C)) return MM_ERR_SHAPE;
  launch_rows<TASK_MULTICLASS, false>(x, W, b, nullptr, nullptr, 0.f, 0.f, nullptr, z, nullptr, nullptr, nullptr, N, D, C, stream);
  return mm_check_launch();
}

extern "C" int medmoe_cls_head_step(const float* x, const float* W, const float* b, const void* targets, const float* pos_weight, int task,
                                    float label_smoothing, float loss_scale, float* z, float* dx, float* dW, float* db, float* loss,
                                    int* counts, float* scratch, long long scratch_floats, int N, int D, int C, hipStream_t stream) {
  if (!x || !W || !b || !targets || !z || !dW || !db || !loss || !counts || !scratch) return MM_ERR_ARG;
  if (!head_shape_ok(N, D, C) || (task != TASK_MULTICLASS && task != TASK_MULTILABEL)) return MM_ERR_SHAPE;
  if (scratch_floats < medmoe_cls_head_scratch(N, D, C)) return MM_ERR_ARG;
  float* dz = scratch;
  float* parts = dz + align4((long long)N * C);
  const int nseg = (N + LOSS_SEG - 1) / LOSS_SEG;            // the row terms padded with zeros to whole segments, then one sum per segment
  float* partials = parts + (long long)nseg * LOSS_SEG;
  float* rec = partials + align4(nseg);
  const int rp = rows_per_record(N, D, C), S = (N + rp - 1) / rp;
  const long long stride = (long long)C * D + REC_PAD;
  if (hipMemsetAsync(loss, 0, sizeof(float), stream) != hipSuccess || hipMemsetAsync(counts, 0, 2 * sizeof(int), stream) != hipSuccess ||
      hipMemsetAsync(parts + N, 0, ((long long)nseg * LOSS_SEG - N + align4(nseg)) * sizeof(float), stream) != hipSuccess)
    return MM_ERR_LAUNCH;
  const long long nt = task == TASK_MULTICLASS ? (long long)N : (long long)N * C;
  hipLaunchKernelGGL(cls_count_kernel, dim3((int)min((nt + 1023) / 1024, 1024ll)), dim3(256), 0, stream, targets, nt, task, counts);
  if (task == TASK_MULTICLASS)
    launch_rows<TASK_MULTICLASS, true>(x, W, b, targets, nullptr, label_smoothing, loss_scale, counts, z, dz, dx, parts, N, D, C, stream);
  else
    launch_rows<TASK_MULTILABEL, true>(x, W, b, targets, pos_weight, 0.f, loss_scale, counts, z, dz, dx, parts, N, D, C, stream);
  // the loss: mm_launch_det_sum sums a segment with ONE workgroup, so the row terms go through it in two stages - nseg segments side by
  // side into partials, then the partials into the loss; both in a fixed order
  if (nseg == 1) {
    mm_launch_det_sum(parts, LOSS_SEG, 1, loss, stream);
  } else {
    mm_launch_det_sum(parts, LOSS_SEG, nseg, partials, stream);
    mm_launch_det_sum(partials, nseg, 1, loss, stream);
  }
#define CLS_WGRAD(CT, VEC) \
  hipLaunchKernelGGL((cls_wgrad_kernel<CT, VEC>), dim3(S, (D + 64 * VEC - 1) / (64 * VEC)), dim3(256), 0, stream, x, dz, rec, N, D, C, rp, stride)
  if (C <= 16) CLS_WGRAD(16, 4);
  else if (C <= 32) CLS_WGRAD(32, 2);
  else CLS_WGRAD(64, 1);
#undef CLS_WGRAD
  hipLaunchKernelGGL(cls_wgrad_sum_kernel, dim3((C * D + C + 255) / 256), dim3(256), 0, stream, rec, S, stride, dW, db, C * D, C);
  return mm_check_launch();
}

extern "C" int medmoe_auroc_counts(const float* scores, const signed char* targets, long long* out, int N, int C, hipStream_t stream) {
  if (!scores || !targets || !out) return MM_ERR_ARG;
  if (N < 1 || C < 1 || C > 65535) return MM_ERR_SHAPE;
  if (hipMemsetAsync(out, 0, 4ll * C * sizeof(long long), stream) != hipSuccess) return MM_ERR_LAUNCH;
  const int xt = (N + 255) / 256;
  const int S0 = max(1, min(xt, 2048 / max(1, min(2048, xt * C))));
  const int chunk = (xt + S0 - 1) / S0 * 256, S = (N + chunk - 1) / chunk;
  hipLaunchKernelGGL(auroc_kernel, dim3(xt, C, S), dim3(256), 0, stream, scores, (const int8_t*)targets, N, C, chunk, (unsigned long long*)out);
  return mm_check_launch();
}
