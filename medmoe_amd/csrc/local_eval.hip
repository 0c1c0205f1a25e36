// GLoRIA local similarity, FORWARD ONLY (losses.py:979-1012 with attention_fn :698-736): the evaluation step's local loss.
//
//   sim[b][i] = log sum_{t < len_i} exp(temp2 cos(w_{i,t}, sum_p a_{p,t} ctx_{b,p}))
//
// with a = softmax over the regions of temp1 * (softmax over the caption's words of the scores ctx_b . w_i).  The training path
// (medmoe_local_scores_t + medmoe_local_pair3) stores the word log-probabilities, the attention A and per-word sums in HBM because
// its backward reads them; here nothing has to survive, so the score tile never leaves the registers and the only global store of an
// (image, caption) pair is its sim element (one owner per element, no atomics: two launches give the same bits).
//
// Ownership is pair3's: one WAVE owns one (image b, caption i, 16-word tile tt) unit and lane (fr, g) holds word t = 16 tt + fr and the
// regions 32 s + 8 g + e (s < NS, e < 8); a workgroup = 8 waves (12 / 10 for captions of 3 / 5 word tiles) = 2..8 captions at a time against ONE image, whose Gram matrix
// ctx_b ctx_b^T it stages once as permuted MFMA A fragments (row tile rt = 2 s + h, MFMA row m -> region 32 s + 8 (m >> 2) + 4 h + (m & 3)).
// The same permutation applied to the rows of ctx_b makes the accumulators of the score MFMAs (v_mfma_f32_16x16x32_bf16, regions x words,
// contraction over the embedding) land exactly where the pair stage wants them: accumulator register r of row tile rt is the score
// of the lane's word against region 32 s + 8 g + 4 h + r.  ctx_b (300 KB at 196 regions x 768) does not fit the LDS: its 64-wide
// k-slices go through a double-buffered ring of A fragments that the workgroup's waves fill together and all read (one workgroup barrier per
// k-step); the word operand is 32 bytes per lane and k-step straight from global memory.
// Reductions over a caption's WORDS (the word softmax, sum_t exp(temp2 cos_t)) cross the 16 lanes of a DPP row and, for captions of
// more than 16 words, the caption's waves through LDS.  The waves are in lock step here anyway (the ring), so that exchange uses the
// workgroup barrier instead of pair3's epoch flags; its mailboxes alias the ring, which is idle between two captions' score loops.
//
// The same body serves two launches (template flag PAIRS).  All pairs (medmoe_local_sim_fwd): a workgroup is (image, chunk of the class's
// caption list) and writes sim[b][i].  Listed pairs (medmoe_local_sim_pairs, candidate re-ranking - DESIGN 3q): a workgroup is one UNIT
// (image b, a run of entries of a pair list); entry e names its caption pair_cap[e] and the element pair_slot[e] of `sim` that receives
// the value.  Only where the caption index comes from and where the result goes differs: the arithmetic of a pair is the same
// instructions in the same order, so a listed pair's value is the all-pairs value bit for bit.
#include "common.h"

struct LocalSimArgs {
  const bf16_t* ctx; const bf16_t* words; const bf16_t* gm; const float* wnorm; const int* cap_lens; const int* cap_list; float* sim;
  const int* units; const int* pair_slot;      // PAIRS: [n_units][4] = (image, first entry, entries, 0); cap_list is then pair_cap
  int n_cap, B, Bc, T, D, caps_per_wg, n_chunk;
  float temp1, temp2, eps;
};

template <int CTRL>
__device__ __forceinline__ float ls_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// over the 16 lanes of a DPP row, result in every lane (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror)
__device__ __forceinline__ float ls_row16_sum(float v) {
  v += ls_dpp<0xB1>(v); v += ls_dpp<0x4E>(v); v += ls_dpp<0x141>(v); v += ls_dpp<0x140>(v);
  return v;
}
__device__ __forceinline__ float ls_row16_max(float v) {
  v = fmaxf(v, ls_dpp<0xB1>(v)); v = fmaxf(v, ls_dpp<0x4E>(v)); v = fmaxf(v, ls_dpp<0x141>(v)); v = fmaxf(v, ls_dpp<0x140>(v));
  return v;
}
__device__ __forceinline__ float ls_grp4_sum(float v) {      // over the four 16-lane groups
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// Waves per workgroup: the score tile alone is 52 accumulator registers per lane at 196 regions, and the pair stage works on it with the
// Gram fragments and the packed attention beside it; at 16 waves (128 registers per lane) every 196-region instantiation spilled 100-430
// registers to scratch, i.e. to global memory.  8 waves leave 256 registers (12 / 10 waves where 8 is not a multiple of the caption's
// waves: 168): no instantiation spills.  One workgroup is resident per CU either way (150 KB of LDS).
__host__ __device__ constexpr int ls_waves(int ntt) { return ntt == 3 ? 12 : ntt == 5 ? 10 : 8; }

template <int HW, int NTT, bool PAIRS>
__global__ __launch_bounds__(ls_waves(NTT) * 64) void local_sim_fwd_kernel(LocalSimArgs p) {
  constexpr int NW = ls_waves(NTT);
  constexpr int NS = (HW + 31) / 32, NRT = 2 * NS, GR = NS * 32, CPI = NW / NTT, TP = NTT * 16;
  constexpr int NRTA = (HW - 32 * (NS - 1) > 4) ? NRT : NRT - 1;       // row tiles with a region < HW
  constexpr int NF = 2 * NRTA;                                         // ring fragments per k-step of 64: [rt][k half]
  constexpr int NLD = (NF + NW - 1) / NW;                                  // ... loaded per wave
  constexpr int RING = NF * 1024;
  constexpr int MBOX = NW * GR * 8;                                    // (max, sum) of every (wave, region)
  constexpr int LSEB = (NW / NTT) * GR * 4;                            // merged log-sum-exp of every (caption, region)
  constexpr int OFF_RING = NRT * NS * 1024, OFF_SE = OFF_RING + (2 * RING > MBOX + LSEB ? 2 * RING : MBOX + LSEB);
  static_assert(OFF_SE + 64 <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[OFF_SE + 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, g = lane >> 4;
  // the image and the run [j0, j_end) of the caption list this workgroup walks
  int b, j0, j_end;
  if (PAIRS) {
    const int4 u = *(const int4*)(p.units + 4 * blockIdx.x);
    b = u.x; j0 = u.y; j_end = u.y + u.z;
  } else {
    b = blockIdx.x / p.n_chunk;
    j0 = (blockIdx.x - b * p.n_chunk) * p.caps_per_wg; j_end = min(p.n_cap, j0 + p.caps_per_wg);
  }
  const int D = p.D, nk = D >> 6;
  // ---- the image's Gram matrix, rows permuted, as MFMA A-operand fragments [rt][s][lane] ----
  for (int f = wid; f < NRT * NS; f += NW) {
    const int rt = f / NS, s = f - rt * NS;
    const int row = 32 * (rt >> 1) + 8 * (fr >> 2) + 4 * (rt & 1) + (fr & 3);
    *(uint4*)(smem + f * 1024 + lane * 16) = *(const uint4*)(p.gm + ((long long)b * GR + row) * GR + 32 * s + 8 * g);
  }
  char* ring = smem + OFF_RING;
  float2* mbox = (float2*)(smem + OFF_RING);                 // [NW waves][GR]: aliases the ring
  float* lsebox = (float*)(smem + OFF_RING + MBOX);          // behind the mailboxes, in the idle ring too
  float* sebox = (float*)(smem + OFF_SE);
  const int grp = wid / NTT, tt = wid - grp * NTT, w0 = grp * NTT;
  // this wave's share of a ring fill: fragments wid, wid + NW, ... ; lane (fr, g) of fragment (rt, kh) holds 8 consecutive embedding
  // columns of the permuted region row fr of tile rt (regions >= HW: zeros)
  const bf16_t* csrc[NLD];
  bool cok[NLD];
#pragma unroll
  for (int u = 0; u < NLD; ++u) {
    const int f = wid + NW * u, rt = f >> 1, kh = f & 1;
    const int row = 32 * (rt >> 1) + 8 * (fr >> 2) + 4 * (rt & 1) + (fr & 3);
    cok[u] = f < NF && row < HW;
    csrc[u] = p.ctx + ((long long)b * HW + (cok[u] ? row : 0)) * D + 32 * kh + 8 * g;
  }
  auto ring_load = [&](uint4 (&v)[NLD], int ks) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) v[u] = cok[u] ? *(const uint4*)(csrc[u] + 64 * ks) : make_uint4(0u, 0u, 0u, 0u);
  };
  auto ring_store = [&](const uint4 (&v)[NLD], int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NLD; ++u)
      if (wid + NW * u < NF) *(uint4*)(ring + buf * RING + (wid + NW * u) * 1024 + lane * 16) = v[u];
  };
  const float c1 = p.temp1 * 1.44269504088896f;
  constexpr float LOG2E = 1.44269504088896f;
  const char* gfrag = smem + lane * 16;
  // every wave takes every barrier: the loop count is the workgroup's, a wave without a unit (the tail of the
  // list) fills the ring and skips the arithmetic
  for (int jb = j0; jb < j_end; jb += CPI) {
    const int j = jb + grp;
    const bool active = j < j_end;             // wave-uniform
    const int i = p.cap_list[active ? j : jb];
    const int cap = max(1, min(min(p.cap_lens[i], p.T), TP));
    const int t = tt * 16 + fr;
    const bool tok = t < cap;
    const float nw = p.wnorm[i * p.T + min(t, p.T - 1)];
    const bf16_t* wsrc = p.words + ((long long)i * p.T + min(t, p.T - 1)) * D + 8 * g;
    // ---- scores S[region][word] = ctx_b . w_i over the ring ----
    f32x4_t acc[NRTA];
#pragma unroll
    for (int rt = 0; rt < NRTA; ++rt) acc[rt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    uint4 cv[NLD];
    bf16x8_t wv[2], wn_[2];
    ring_load(cv, 0);
    wv[0] = *(const bf16x8_t*)(wsrc); wv[1] = *(const bf16x8_t*)(wsrc + 32);
    ring_store(cv, 0);
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
      const bool more = ks + 1 < nk;
      if (more) {
        ring_load(cv, ks + 1);
        wn_[0] = *(const bf16x8_t*)(wsrc + 64 * (ks + 1)); wn_[1] = *(const bf16x8_t*)(wsrc + 64 * (ks + 1) + 32);
      }
      if (active) {
        // the two fragments of the next row tile are requested before this tile's MFMAs (the scheduling barriers keep the compiler from
        // hoisting all 26 reads of a k-step: 104 registers)
        const char* rb = ring + (ks & 1) * RING + lane * 16;
        bf16x8_t fa0 = *(const bf16x8_t*)(rb), fa1 = *(const bf16x8_t*)(rb + 1024);
#pragma unroll
        for (int rt = 0; rt < NRTA; ++rt) {
          bf16x8_t fb0 = fa0, fb1 = fa1;
          if (rt + 1 < NRTA) { fb0 = *(const bf16x8_t*)(rb + (2 * rt + 2) * 1024); fb1 = *(const bf16x8_t*)(rb + (2 * rt + 3) * 1024); }
          acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa0, wv[0], acc[rt], 0, 0, 0);
          acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa1, wv[1], acc[rt], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          fa0 = fb0; fa1 = fb1;
        }
      }
      if (more) { ring_store(cv, (ks + 1) & 1); wv[0] = wn_[0]; wv[1] = wn_[1]; }
      __syncthreads();                                      // the next slice is in place, this one is free to be overwritten
    }
    // ---- word softmax (losses.py:716), part 1: per region the maximum and the sum of exp over this wave's 16 words ----
    // the reduction over the words crosses the 16 lanes of a row; masked words (t >= len) take no part
    auto tile_stats = [&](int rt, float (&m)[4], float (&s)[4]) __attribute__((always_inline)) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        m[r] = ls_row16_max(tok ? acc[rt][r] : -1e30f);
        s[r] = ls_row16_sum(tok ? __builtin_amdgcn_exp2f((acc[rt][r] - m[r]) * LOG2E) : 0.f);
      }
    };
    if (NTT > 1 && active) {
#pragma unroll
      for (int rt = 0; rt < NRTA; ++rt) {
        float m[4], s[4];
        tile_stats(rt, m, s);
        if (fr == 0) {
          float2* dst = mbox + wid * GR + 32 * (rt >> 1) + 8 * g + 4 * (rt & 1);
          *(float4*)dst = make_float4(m[0], s[0], m[1], s[1]);
          *(float4*)(dst + 2) = make_float4(m[2], s[2], m[3], s[3]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (NTT > 1) {
      // the caption's log-sum-exp per region: its first wave merges the NTT waves' (max, sum) pairs in wave order, one region per lane and
      // step - a real loop of a dozen registers (merged inside the unrolled tile loop below, all 13 tiles' mailbox reads were hoisted
      // in front of it and spilled) - and hands the result to the caption's waves through LDS
      __syncthreads();
      if (active && tt == 0) {
        for (int hw = lane; hw < GR; hw += 64) {
          float M = -1e30f, L = 0.f;
#pragma unroll
          for (int q = 0; q < NTT; ++q) {
            const float2 v = mbox[(w0 + q) * GR + hw];
            const float Mn = fmaxf(M, v.x);
            L = L * __builtin_amdgcn_exp2f((M - Mn) * LOG2E) + v.y * __builtin_amdgcn_exp2f((v.x - Mn) * LOG2E);
            M = Mn;
          }
          lsebox[grp * GR + hw] = M + __logf(L);
        }
      }
      __syncthreads();
    }
    float se = 0.f;
    if (active) {
      // ---- part 2: a1 = exp(S - lse); then the region softmax of
      // temp1 a1 (losses.py:724-725) unnormalised: x = exp(temp1 a1) over the score in place, cs = sum x, un = sum x S ----
      float cs = 0.f, un = 0.f;
#pragma unroll
      for (int rt = 0; rt < NRTA; ++rt) {
        float lse[4];
        if (NTT > 1) {
          const float4 l4 = *(const float4*)(lsebox + grp * GR + 32 * (rt >> 1) + 8 * g + 4 * (rt & 1));
          lse[0] = l4.x; lse[1] = l4.y; lse[2] = l4.z; lse[3] = l4.w;
        } else {
          float m[4], s[4];
          tile_stats(rt, m, s);
#pragma unroll
          for (int r = 0; r < 4; ++r) lse[r] = m[r] + __logf(s[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float S = acc[rt][r];
          const float a1 = tok ? __builtin_amdgcn_exp2f((S - lse[r]) * LOG2E) : 0.f;
          float x = __builtin_amdgcn_exp2f(c1 * a1);
          if (32 * (rt >> 1) + 24 + 4 * (rt & 1) + r >= HW) x = (32 * (rt >> 1) + 8 * g + 4 * (rt & 1) + r < HW) ? x : 0.f;
          acc[rt][r] = x;
          cs += x;
          un += x * S;                                      // regions >= HW: x = 0 exactly, S = 0 (zero rows in the ring)
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      cs = ls_grp4_sum(cs);
      un = ls_grp4_sum(un);
      const float cinv = (tok ? 1.f : 0.f) / fmaxf(cs, 1e-30f);
      const float num = un * cinv;                          // sum_p a_p S_p = w . (weighted context)
      // ---- n2 = a^T Gm a = |weighted context|^2: a as the bf16 B operand (8 consecutive regions per k-step: tiles 2 s and 2 s + 1) ----
      auto a_of = [&](int rt, int r) -> float { return rt < NRTA ? acc[rt < NRTA ? rt : 0][r] * cinv : 0.f; };
      uint4 af[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = a_of(2 * s + (e >> 2), e & 3);
        af[s] = make_uint4(pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(a[4], a[5]), pack2bf(a[6], a[7]));
      }
      float n2 = 0.f;
#pragma unroll
      for (int rt = 0; rt < NRTA; ++rt) {
        f32x4_t y = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s)
          y = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(gfrag + (rt * NS + s) * 1024), __builtin_bit_cast(bf16x8_t, af[s]), y, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) n2 += a_of(rt, r) * y[r];
        __builtin_amdgcn_sched_barrier(0);
      }
      n2 = ls_grp4_sum(n2);
      // ---- per-word cosine (losses.py:690-695), sum over the wave's words ----
      const float den = nw * sqrtf(fmaxf(n2, 0.f));
      const float cosv = num / fmaxf(den, p.eps);
      se = ls_row16_sum(tok ? __expf(p.temp2 * cosv) : 0.f);
      if (NTT > 1 && lane == 0) sebox[wid] = se;
    }
    if (NTT > 1) {
      __syncthreads();                                      // also: every mailbox read is done before the next ring fill
      if (active && tt == 0) {
        se = 0.f;
#pragma unroll
        for (int q = 0; q < NTT; ++q) se += sebox[w0 + q];
      }
    }
    if (active && tt == 0 && lane == 0) p.sim[PAIRS ? (long long)p.pair_slot[j] : (long long)b * p.Bc + i] = __logf(se);
  }
}

template <bool PAIRS>
static void ls_launch(const LocalSimArgs& p, int HW, int ntt, dim3 grid, dim3 block, hipStream_t stream) {
#define LS(HW_, T_) hipLaunchKernelGGL((local_sim_fwd_kernel<HW_, T_, PAIRS>), grid, block, 0, stream, p);
  if (HW == 64) LS(64, 1)
  else switch (ntt) { case 1: LS(196, 1) break; case 2: LS(196, 2) break; case 3: LS(196, 3) break; case 4: LS(196, 4) break; default: LS(196, 5) break; }
#undef LS
}

// Tests: force the number of caption chunks per image (0 = automatic), as medmoe_local_pair3_chunks does for the training kernels.
static int g_local_sim_chunks = 0;
extern "C" int medmoe_local_sim_chunks(int n) {
  if (n < 0) return MM_ERR_ARG;
  g_local_sim_chunks = n;
  return MM_OK;
}

// Host entry: one launch per caption length class.  ctx bf16 [B*HW][D]; words bf16 [Bc][T][D]; gm bf16 [B][GR][GR], GR = 32 ceil(HW / 32),
// zero outside [HW][HW]; wnorm fp32 [Bc][T]; cap_list: the n_cap captions of the class (16 (ntt - 1) < len <= 16 ntt); sim fp32 [B][Bc].
// There is no pair matrix, hence no column base.  Geometries: medmoe_local_pair3_supported; anything else returns MM_ERR_SHAPE
// before a launch.
extern "C" int medmoe_local_sim_fwd(const void* ctx, const void* words, const int* cap_lens, const void* gm, const float* wnorm, float* sim,
                                    int B, int Bc, int HW, int T, int D, float temp1, float temp2, float eps, const int* cap_list,
                                    int n_cap, int ntt, hipStream_t stream) {
  if (!ctx || !words || !cap_lens || !gm || !wnorm || !sim || !cap_list) return MM_ERR_ARG;
  if (B <= 0 || Bc <= 0 || T <= 0 || n_cap <= 0 || n_cap > Bc || ntt < 1 || ntt > 5 || ntt * 16 > ((T + 15) / 16) * 16) return MM_ERR_SHAPE;
  if (!((HW == 64 && ntt == 1) || HW == 196) || D < 64 || (D % 64)) return MM_ERR_SHAPE;
  LocalSimArgs p;
  p.ctx = (const bf16_t*)ctx; p.words = (const bf16_t*)words; p.gm = (const bf16_t*)gm; p.wnorm = wnorm; p.cap_lens = cap_lens;
  p.cap_list = cap_list; p.sim = sim; p.units = nullptr; p.pair_slot = nullptr; p.n_cap = n_cap; p.B = B; p.Bc = Bc; p.T = T; p.D = D; p.temp1 = temp1; p.temp2 = temp2; p.eps = eps;
  // one workgroup per (image, caption chunk), one resident per CU (LDS): enough chunks that small batches still give every CU a few
  // workgroups (the heuristic of medmoe_local_pair3, not tuned here); chunks are a multiple of the captions per iteration
  const int nw = ls_waves(ntt), cpi = nw / ntt;
  int n_chunk = g_local_sim_chunks > 0 ? g_local_sim_chunks : max(1, (1024 + B - 1) / B);
  const int cpw = ((n_cap + n_chunk - 1) / n_chunk + cpi - 1) / cpi * cpi;
  n_chunk = (n_cap + cpw - 1) / cpw;
  p.caps_per_wg = cpw; p.n_chunk = n_chunk;
  const dim3 grid(B * n_chunk), block(nw * 64);
  ls_launch<false>(p, HW, ntt, grid, block, stream);
  return mm_check_launch();
}

// Host entry of the listed pairs (candidate re-ranking): out[pair_slot[e]] = the similarity of (image units[u][0], caption pair_cap[e]) for
// every entry e of every unit u = (image, first entry, entries, 0), one workgroup per unit, which stages the image's Gram fragments once
// and walks its entries ls_waves(ntt) / ntt captions at a time.  ctx, words, cap_lens, gm, wnorm as medmoe_local_sim_fwd; all captions of a
// launch are of length class ntt.  One owner per written slot (the caller's lists name a slot once), no atomics; slots no entry names
// are not written.  The kernel trusts its tables: the caller validates every index on the host (medmoe_amd/ops.py local_sim_pairs).
extern "C" int medmoe_local_sim_pairs(const void* ctx, const void* words, const int* cap_lens, const void* gm, const float* wnorm, float* out,
                                      const int* units, int n_units, const int* pair_cap, const int* pair_slot, int B, int Bc, int HW, int T,
                                      int D, float temp1, float temp2, float eps, int ntt, hipStream_t stream) {
  if (n_units < 0) return MM_ERR_ARG;
  if (B <= 0 || Bc <= 0 || T <= 0 || ntt < 1 || ntt > 5 || ntt * 16 > ((T + 15) / 16) * 16) return MM_ERR_SHAPE;
  if (!((HW == 64 && ntt == 1) || HW == 196) || D < 64 || (D % 64)) return MM_ERR_SHAPE;
  if (n_units == 0) return MM_OK;
  if (!ctx || !words || !cap_lens || !gm || !wnorm || !out || !units || !pair_cap || !pair_slot) return MM_ERR_ARG;
  LocalSimArgs p;
  p.ctx = (const bf16_t*)ctx; p.words = (const bf16_t*)words; p.gm = (const bf16_t*)gm; p.wnorm = wnorm; p.cap_lens = cap_lens;
  p.cap_list = pair_cap; p.sim = out; p.units = units; p.pair_slot = pair_slot; p.n_cap = 0; p.B = B; p.Bc = Bc; p.T = T; p.D = D;
  p.caps_per_wg = 0; p.n_chunk = 1; p.temp1 = temp1; p.temp2 = temp2; p.eps = eps;
  ls_launch<true>(p, HW, ntt, dim3(n_units), dim3(ls_waves(ntt) * 64), stream);
  return mm_check_launch();
}
