// The local-loss score GEMM with the word-softmax fused, in its two output forms, on the LDS ring of gemm_nt512_kernel.
#include "gemm_nt.h"
#include "options.h"

// ---------------------------------------------------------------------------------------------
// scores512: the local-loss score GEMM S = ctx . words^T of ONE caption length class with the word-softmax fused
// (losses.py:713-716), on the gemm_nt512 structure: 256 region rows x (whole captions) per workgroup, sub-steps of
// 32, ring of four LDS sub-stages, ping-pong wave groups.  The older 128-row kernel (loss.hip) runs a two-stage
// lock-step pipeline at ~680 TFLOP/s.  A wave owns whole captions, so the softmax over a caption's words needs only the
// two cross-lane-group shuffles of the 16x16 accumulator layout (lane: region row fr, words 4g..4g+3 of every 16-tile).
//   NTT 1, 2, 4: waves 2 (rows) x 4 (cols), wave tile 128 x 64 = 4 / 2 / 1 captions;  NTT 3: 128 x 48 = 1 caption;
//   NTT 5: waves 4 x 2, wave tile 64 x 80 = 1 caption.
// Output: the word-softmax as fp16 LOG-probabilities S - lse at the caption's columns of the ragged pair matrix + the row
// log-sum-exp (fp32).  Both a1 = exp(.) and S = . + lse are recovered to 2^-11 relative: bf16 probabilities lost S for
// every word whose probability underflowed, and kept only 2^-9 absolute on the rest (profiles/r02_notes.md).
// ---------------------------------------------------------------------------------------------
struct ScoresArgs {
  const bf16_t* ctx; const bf16_t* words; const int* cap_lens; const int* cap_list;
  bf16_t* a1; float* lse;
  int M, HW, HWP, Bc, T, D, n_cap;
  long long col_base, ldp, bstride;      // bstride: TR output only, elements between two images' blocks
  int skip_epi; float inv_hw;
};

// TR: the TRANSPOSED pair matrix of pair3.hip - rows = caption words (row col_base + cj*TP + t), columns = image regions
// (b*HWP + hw), ldp columns per row, values = fp16 LOG2-probabilities (S - lse) / ln 2.  The MFMA operands swap roles, so a lane
// holds four consecutive regions of one word (8-byte stores; HW % 4 == 0 keeps them inside one image) and the softmax over a
// caption's words runs across the 16 lanes of a DPP row.
template <int CTRL>
__device__ __forceinline__ float sc_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float sc_row16_sum(float v) {
  v += sc_dpp<0xB1>(v); v += sc_dpp<0x4E>(v); v += sc_dpp<0x141>(v); v += sc_dpp<0x140>(v);
  return v;
}
__device__ __forceinline__ float sc_row16_max(float v) {
  v = fmaxf(v, sc_dpp<0xB1>(v)); v = fmaxf(v, sc_dpp<0x4E>(v)); v = fmaxf(v, sc_dpp<0x141>(v)); v = fmaxf(v, sc_dpp<0x140>(v));
  return v;
}

// Four independent row reductions interleaved: a DPP operand needs two wait states behind the VALU write of its register, and three
// other instructions sit between two uses of one register here - no s_nop, no separate v_mov_b32_dpp (the compiler emits mov + op + nop
// per step: 12 issue slots per value against 4).
#define SC_DPP4(OP, CTRL)                                                                                            \
  "v_" OP "_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n\tv_" OP "_f32_dpp %1, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf\n\t" \
  "v_" OP "_f32_dpp %2, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf\n\tv_" OP "_f32_dpp %3, %3, %3 " CTRL " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ void sc_row16_max4(float& a, float& b, float& c, float& d) {
  asm volatile("s_nop 1\n\t" SC_DPP4("max", "quad_perm:[1,0,3,2]") SC_DPP4("max", "quad_perm:[2,3,0,1]") SC_DPP4("max", "row_half_mirror")
               SC_DPP4("max", "row_mirror") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
__device__ __forceinline__ void sc_row16_sum4(float& a, float& b, float& c, float& d) {
  asm volatile("s_nop 1\n\t" SC_DPP4("add", "quad_perm:[1,0,3,2]") SC_DPP4("add", "quad_perm:[2,3,0,1]") SC_DPP4("add", "row_half_mirror")
               SC_DPP4("add", "row_mirror") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}

template <int NTT, bool TR = false>
__global__ __launch_bounds__(512, 2) void scores512_kernel(ScoresArgs p) {
  constexpr int TP = NTT * 16;
  constexpr int WNN = (NTT == 5) ? 2 : 4;                     // waves along the columns
  constexpr int WMM = 8 / WNN;
  constexpr int TMW = 16 / WMM;                               // 16-row tiles per wave (256 rows per workgroup)
  constexpr int CW = (NTT == 1) ? 4 : (NTT == 2) ? 2 : 1;     // captions per wave
  constexpr int TNW = CW * NTT;                               // 16-col tiles per wave
  constexpr int BNS = WNN * TNW * 16;                          // word rows (= score columns) per workgroup
  constexpr int CAPB = WNN * CW;                              // captions per workgroup
  constexpr int NPIECE = (256 + BNS) / 16;                     // 1-KB DMA pieces per sub-stage
  __shared__ __attribute__((aligned(16))) char smem[NRING * SUB3];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid % WMM, wn = wid / WMM;                   // the two waves of a SIMD (w, w+4) take different captions
  const int fr = lane & 15, g = lane >> 4;
  const int G = gridDim.x;
  const int my = xcd_remap(blockIdx.x, G);
  const int tiles_m = (p.M + 255) / 256, tiles_n = (p.n_cap + CAPB - 1) / CAPB;
  const int total = tiles_m * tiles_n;
  const int nu = p.D / 32;
  struct Tile { int m0, c0; };
  // column tiles of one row tile are consecutive: the 32 workgroups of an XCD share a few ctx panels and the words
  auto decode = [&](int id) -> Tile { Tile t; t.m0 = (id / tiles_n) * 256; t.c0 = (id % tiles_n) * CAPB; return t; };

  unsigned src[4];
  bool have[4];
  auto setup = [&](const Tile& t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int piece = i * 8 + wid;
      have[i] = piece < NPIECE;
      const int line = piece * 8 + (lane >> 3);
      const int lc = (lane & 7) ^ (line & 7);
      const int row = 2 * line + (lc >> 2);                   // 0..255 ctx rows, 256.. word rows
      if (i < 2) src[i] = (unsigned)min(t.m0 + row, p.M - 1) * (unsigned)(p.D * 2) + (lc & 3) * 16;
      else {
        const int n = min(row - 256, BNS - 1);
        const int cj = min(t.c0 + n / TP, p.n_cap - 1), tw = min(n % TP, p.T - 1);
        src[i] = (unsigned)(p.cap_list[cj] * p.T + tw) * (unsigned)(p.D * 2) + (lc & 3) * 16;
      }
    }
  };
  auto stage = [&](int buf, int k0) {
    char* sb = smem + buf * SUB3 + wid * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (have[i])
        __builtin_amdgcn_global_load_lds(GLB_PTR((const char*)(i < 2 ? p.ctx : p.words) + k0 * 2 + src[i]), LDS_PTR(sb + i * 8192), 16, 0, 0);
  };
  f32x4_t acc[TMW][TNW];
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < TMW; ++i)
#pragma unroll
      for (int j = 0; j < TNW; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  };
  const int lane_off = (fr >> 1) * 128 + (((((fr & 1) << 2) | g) ^ ((fr >> 1) & 7)) << 4);
  const int offA_nat = (wm * TMW * 16) * 64 + lane_off;
  // word rows are read sigma-permuted (as the B rows of gemm_nt512): lane (fr, g) then owns words pg*4 .. pg*4+3 of every
  // 16-word tile, and one permlane32_swap per tile pair gives each lane 8 consecutive words (16-byte stores)
  const int sig = ((((fr >> 2) & 1) << 1 | (fr >> 3)) << 2) | (fr & 3);
  const int pg = ((g & 1) << 1) | (g >> 1);
  const int sig_off = (sig >> 1) * 128 + (((((sig & 1) << 2) | g) ^ ((sig >> 1) & 7)) << 4);
  // TR: the sigma permutation moves to the ctx rows (they become the accumulator rows), the word rows are read in natural order
  const int offA = TR ? (wm * TMW * 16) * 64 + sig_off : offA_nat;
  const int offB = (256 + wn * TNW * 16) * 64 + (TR ? lane_off : sig_off);
  bf16x8_t af[TMW], bf[TNW];
  auto read_frags = [&](int buf) __attribute__((always_inline)) {
    const char* sA = smem + buf * SUB3 + offA;
    const char* sB = smem + buf * SUB3 + offB;
#pragma unroll
    for (int t = 0; t < TMW; ++t) af[t] = *(const bf16x8_t*)(sA + t * 1024);
#pragma unroll
    for (int t = 0; t < TNW; ++t) bf[t] = *(const bf16x8_t*)(sB + t * 1024);
  };
  auto compute = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
      for (int tn = 0; tn < TNW; ++tn)
        acc[tm][tn] = TR ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[tm], bf[tn], acc[tm][tn], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[tn], af[tm], acc[tm][tn], 0, 0, 0);
  };
  // TR epilogue: lane (fr, g) holds word tn*16 + fr of the caption and regions pg*4 .. pg*4+3 of region tile tm (the ctx rows are read
  // sigma-permuted); one permlane32_swap per pair of region tiles then gives each lane 8 consecutive regions (16-byte stores).
  // The epilogue is instruction-bound (it was 41 % of the kernel: 3000 vector + 1200 scalar instructions per wave and tile), so:
  // the padding words of a caption are set to -inf ONCE (class NTT holds captions of 16 (NTT-1) < len <= 16 NTT words: only the last
  // word tile can have padding) and the max / exp / clamp then need no selects; row -> (image, region) by a reciprocal multiply with one
  // correction step instead of an integer division; store predicates hoisted out of the word-tile loop.
  auto div_hw = [&](int m, int& q, int& r) __attribute__((always_inline)) {
    q = (int)(((float)m + 0.5f) * p.inv_hw);
    r = m - q * p.HW;
    if (r < 0) { --q; r += p.HW; }
    if (r >= p.HW) { ++q; r -= p.HW; }
  };
  auto epilogue_t = [&](const Tile& t) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < CW; ++c) {
      const int cj = t.c0 + wn * CW + c;
      const bool cap_ok = cj < p.n_cap && p.skip_epi != 2;          // skip_epi 2 (measurement): the whole epilogue except its stores
      const int cap_i = p.cap_list[min(cj, p.n_cap - 1)];
      const int cap = max(1, min(min(p.cap_lens[cap_i], p.T), TP));
      if ((NTT - 1) * 16 + fr >= cap) {
#pragma unroll
        for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[tm][c * NTT + NTT - 1][r] = -INFINITY;
      }
      if (NTT > 1 && cap <= (NTT - 1) * 16) {                      // a caption shorter than its class (not what the engine's tables build): every tile
#pragma unroll
        for (int tn = 0; tn < NTT - 1; ++tn)
          if (tn * 16 + fr >= cap) {
#pragma unroll
            for (int tm = 0; tm < TMW; ++tm)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[tm][c * NTT + tn][r] = -INFINITY;
          }
      }
      // Two region-tile pairs (jp = 2 J, 2 J + 1: 64 consecutive regions) per round.  After the permlane32_swap a lane holds 8 consecutive
      // regions of word fr, and one store instruction would write 16 word rows x 64 bytes - the shape a CU's store path drains at 12.5 B/clk
      // (profiles/r02_notes.md, tools/store_bw.hip): the stores, not the softmax arithmetic, set the epilogue's length.  One more exchange, a
      // bank-masked row_ror:8 DPP move per dword, hands the lanes fr >= 8 the NEXT 32 regions of word fr - 8 (and the lanes fr < 8 the first 32
      // regions of word fr + 8): every store instruction then writes 8 word rows x 128 contiguous bytes (39 B/clk).
#pragma unroll
      for (int J = 0; J < TMW / 4; ++J) {
        uint4 vv[2][NTT];
#pragma unroll
        for (int jq = 0; jq < 2; ++jq) {
          const int jp = 2 * J + jq;
          uint2 o[2][NTT];
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int tm = 2 * jp + q;
            // log2 domain: t = S log2 e, lse2 = max + log2 sum 2^(t - max), output t - lse2, stored lse = lse2 ln 2.  The scale rides in the
            // two fused multiply-adds (the maximum is taken on the raw scores: the scale is positive), and the clamp to LOGP_MIN runs on the
            // packed halves (-60000 is an fp16 value; a log-probability below the fp16 range converts to -inf and is clamped the same):
            // 192 of the epilogue's 1850 vector instructions per wave and tile gone.
            constexpr float L2E = 1.44269504088896f;
            float mx[4], sm[4], lse2[4];
  #pragma unroll
            for (int r = 0; r < 4; ++r) {
              mx[r] = acc[tm][c * NTT][r];
  #pragma unroll
              for (int tn = 1; tn < NTT; ++tn) mx[r] = fmaxf(mx[r], acc[tm][c * NTT + tn][r]);
            }
            sc_row16_max4(mx[0], mx[1], mx[2], mx[3]);             // word 0 of every caption is real: finite
  #pragma unroll
            for (int r = 0; r < 4; ++r) {
              mx[r] *= L2E;
              sm[r] = 0.f;
  #pragma unroll
              for (int tn = 0; tn < NTT; ++tn) sm[r] += __builtin_amdgcn_exp2f(__builtin_fmaf(acc[tm][c * NTT + tn][r], L2E, -mx[r]));
            }
            sc_row16_sum4(sm[0], sm[1], sm[2], sm[3]);
            float lse4[4];
  #pragma unroll
            for (int r = 0; r < 4; ++r) { lse2[r] = mx[r] + __builtin_amdgcn_logf(sm[r]); lse4[r] = lse2[r] * 0.6931471805599453f; }
            typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
            const h2_t lo2 = __builtin_bit_cast(h2_t, LOGP_MIN_BITS2);
  #pragma unroll
            for (int tn = 0; tn < NTT; ++tn) {
              float e[4];
  #pragma unroll
              for (int r = 0; r < 4; ++r) e[r] = __builtin_fmaf(acc[tm][c * NTT + tn][r], L2E, -lse2[r]);
              o[q][tn].x = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(h2_t, pack2h(e[0], e[1])), lo2));
              o[q][tn].y = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(h2_t, pack2h(e[2], e[3])), lo2));
            }
            const int m4 = t.m0 + wm * TMW * 16 + tm * 16 + 4 * pg;          // this lane's four regions of tile tm (one image: HW % 4 == 0)
            if (fr == 0 && m4 < p.M && cap_ok) {
              int mb, hw;
              div_hw(m4, mb, hw);
              *(float4*)(p.lse + ((long long)mb * p.Bc + cap_i) * p.HWP + hw) = make_float4(lse4[0], lse4[1], lse4[2], lse4[3]);
            }
          }
  
#pragma unroll
          for (int tn = 0; tn < NTT; ++tn) {
            auto r0 = __builtin_amdgcn_permlane32_swap(o[0][tn].x, o[1][tn].x, false, false);
            auto r1 = __builtin_amdgcn_permlane32_swap(o[0][tn].y, o[1][tn].y, false, false);
            vv[jq][tn] = make_uint4(r0[0], r1[0], r0[1], r1[1]);
          }
        }
        // lane (fr, g): word row (fr & 7) + 8 i of instruction i, regions m8 .. m8 + 7
        const int m8 = t.m0 + wm * TMW * 16 + (4 * J + (g >> 1)) * 16 + (g & 1) * 8 + 32 * (fr >> 3);
        int mb, hw;
        div_hw(min(m8, p.M - 4), mb, hw);
        const bool ok = m8 < p.M && cap_ok;
        const bool whole = hw + 8 <= p.HW;                                  // else the image ends after four of them
        const bool ok2 = m8 + 4 < p.M;
        bf16_t* dst0 = p.a1 + (p.col_base + (long long)cj * TP + (fr & 7)) * p.ldp + (long long)mb * p.bstride + hw;
        bf16_t* dst2 = p.a1 + (p.col_base + (long long)cj * TP + (fr & 7)) * p.ldp + (long long)(mb + 1) * p.bstride;
#pragma unroll
        for (int tn = 0; tn < NTT; ++tn) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const uint4 a = vv[0][tn], b = vv[1][tn];
            uint4 y;
            if (i == 0) {           // lanes 8..15 of every row take the second pair's piece of lane - 8
              y.x = __builtin_amdgcn_update_dpp(a.x, b.x, 0x128, 0xf, 0xC, false); y.y = __builtin_amdgcn_update_dpp(a.y, b.y, 0x128, 0xf, 0xC, false);
              y.z = __builtin_amdgcn_update_dpp(a.z, b.z, 0x128, 0xf, 0xC, false); y.w = __builtin_amdgcn_update_dpp(a.w, b.w, 0x128, 0xf, 0xC, false);
            } else {                // lanes 0..7 take the first pair's piece of lane + 8
              y.x = __builtin_amdgcn_update_dpp(b.x, a.x, 0x128, 0xf, 0x3, false); y.y = __builtin_amdgcn_update_dpp(b.y, a.y, 0x128, 0xf, 0x3, false);
              y.z = __builtin_amdgcn_update_dpp(b.z, a.z, 0x128, 0xf, 0x3, false); y.w = __builtin_amdgcn_update_dpp(b.w, a.w, 0x128, 0xf, 0x3, false);
            }
            const long long ro = (long long)(tn * 16 + 8 * i) * p.ldp;
            if (ok && whole) *(uint4*)(dst0 + ro) = y;
            else if (ok) {
              *(uint2*)(dst0 + ro) = make_uint2(y.x, y.y);
              if (ok2) *(uint2*)(dst2 + ro) = make_uint2(y.z, y.w);
            }
          }
        }
      }
    }
  };
  // word softmax per region row and caption: the row's words are (tn, r) in this lane and the 4 lane groups g
  auto epilogue = [&](const Tile& t) __attribute__((always_inline)) -> int {
    int n_st = 0;
#pragma unroll
    for (int c = 0; c < CW; ++c) {
      const int cj = t.c0 + wn * CW + c;
      const bool cap_ok = cj < p.n_cap;
      const int cap_i = p.cap_list[min(cj, p.n_cap - 1)];
      const int cap = max(1, min(min(p.cap_lens[cap_i], p.T), TP));   // an empty caption counts as its first word (as in epilogue_t)
#pragma unroll
      for (int tm = 0; tm < TMW; ++tm) {
        float mx = -INFINITY;
#pragma unroll
        for (int tn = 0; tn < NTT; ++tn)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (tn * 16 + pg * 4 + r < cap) mx = fmaxf(mx, acc[tm][c * NTT + tn][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sm = 0.f;
#pragma unroll
        for (int tn = 0; tn < NTT; ++tn)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            sm += (tn * 16 + pg * 4 + r < cap) ? __expf(acc[tm][c * NTT + tn][r] - mx) : 0.f;
        sm += __shfl_xor(sm, 16, 64);
        sm += __shfl_xor(sm, 32, 64);
        const float lse = mx + __logf(sm);
        const int m = t.m0 + wm * TMW * 16 + tm * 16 + fr;
        const bool ok = m < p.M && cap_ok;
        const int mb = min(m, p.M - 1) / p.HW, hw = min(m, p.M - 1) - mb * p.HW;
        if (ok && g == 0) p.lse[((long long)mb * p.Bc + cap_i) * p.HWP + hw] = lse;       // [image][caption][region]
        bf16_t* dst = p.a1 + ((long long)mb * p.HWP + hw) * p.ldp + p.col_base + (long long)cj * TP;
        // the tile holds the word-softmax as fp16 LOG-probabilities S - lse (masked words: LOGP_MIN)
        float e[NTT][4];
#pragma unroll
        for (int tn = 0; tn < NTT; ++tn)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            e[tn][r] = (tn * 16 + pg * 4 + r < cap) ? fmaxf(acc[tm][c * NTT + tn][r] - lse, LOGP_MIN) : LOGP_MIN;
        uint2 o[NTT];
#pragma unroll
        for (int tn = 0; tn < NTT; ++tn) {
          o[tn].x = pack2h(e[tn][0], e[tn][1]);
          o[tn].y = pack2h(e[tn][2], e[tn][3]);
        }
#pragma unroll
        for (int j = 0; j < NTT / 2; ++j) {          // tile pairs: 16-byte stores of 8 consecutive words
          auto r0 = __builtin_amdgcn_permlane32_swap(o[2 * j].x, o[2 * j + 1].x, false, false);
          auto r1 = __builtin_amdgcn_permlane32_swap(o[2 * j].y, o[2 * j + 1].y, false, false);
          if (ok) *(uint4*)(dst + (2 * j + (g >> 1)) * 16 + (g & 1) * 8) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
        }
        if ((NTT & 1) && ok) *(uint2*)(dst + (NTT - 1) * 16 + pg * 4) = o[NTT - 1];
        n_st += NTT;
      }
    }
    return n_st + TMW * CW;         // upper bound of the store instructions issued (A1 pieces + lse): see wait below
  };

  if (my >= total) return;
  const int my_tiles = (total - my + G - 1) / G;
  // Where the time goes (tools/scores_probe.py, batch 1024, all five classes): k-loops 15.0 ms, + epilogue arithmetic 3.6 ms, + its stores
  // 4.8 ms (128 KB per tile leave a CU at ~7 B/clk).  Measured and without effect on that: 10 % fewer vector instructions in the epilogue, store
  // instructions of 8 rows x 128 bytes instead of 16 x 64, workgroups started in 2..16 phases a fraction of a tile apart (the store cost is
  // per CU, not a chip-wide burst).
  Tile ct = decode(my);
  setup(ct);
  int lid = my, lk = 0, wb = 0, rb = 0;
  bool lmore = true;
  // The epilogue's stores sit between DMA stages in the vmcnt order; their number depends on predicates, so after a
  // seam the counted wait is replaced by a full drain for the three waits that could still see them (once per tile).
  int drain = 0;
  auto issue = [&]() __attribute__((always_inline)) {
    if (lmore) {
      stage(wb, lk * 32);
      wb = (wb + 1) & 3;
      if (++lk == nu) {
        lk = 0; lid += G;
        if (lid < total) { const Tile lt = decode(lid); setup(lt); } else lmore = false;
      }
    }
  };
  // pieces per stage differ per wave when NPIECE < 32: the wave's own count
  const int my_pieces = (have[0] ? 1 : 0) + (have[1] ? 1 : 0) + (have[2] ? 1 : 0) + (have[3] ? 1 : 0);
  auto wait_third_newest = [&]() __attribute__((always_inline)) {
    if (drain > 0 || !lmore) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (drain > 0) --drain; }
    else if (my_pieces == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (my_pieces == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  };
  const int grp = __builtin_amdgcn_readfirstlane(wid >> 2);
  zero_acc();
  issue(); issue(); issue();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  auto seg_barrier = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
  };
  auto load_seg = [&]() __attribute__((always_inline)) {
    read_frags(rb);
    rb = (rb + 1) & 3;
    issue();
    if (grp == 1) wait_third_newest();
    seg_barrier();
  };
  auto body = [&](bool last) __attribute__((always_inline)) {
    compute();
    if (grp == 0) { wait_third_newest(); seg_barrier(); }
    if (last) {
      if (p.skip_epi != 1) { if constexpr (TR) epilogue_t(ct); else epilogue(ct); }
      zero_acc();
      drain = 3;
    }
    if (grp == 1) seg_barrier();
    load_seg();
  };
  if (grp == 1) seg_barrier();
  load_seg();
  for (int ti = 0; ti < my_tiles; ++ti) {
    for (int k = 1; k < nu; ++k) body(false);
    body(true);
    if (ti + 1 < my_tiles) ct = decode(my + (ti + 1) * G);
  }
  if (grp == 0) seg_barrier();
}

int g_use_scores512 = 1, g_scores_skip_epi = 0;      // options.h, keys 6 and 12

// out: the pair matrix (a1) or its transpose (lpT); col_base / ldp / bstride place a caption's block in it (see ScoresArgs and the TR note)
static ScoresArgs sc_args(const void* ctx, const void* words, const int* cap_lens, const int* cap_list, void* out, float* lse, long long M,
                          int HW, int Bc, int T, int D, int n_cap, long long col_base, long long ldp, long long bstride) {
  ScoresArgs p;
  p.ctx = (const bf16_t*)ctx; p.words = (const bf16_t*)words; p.cap_lens = cap_lens; p.cap_list = cap_list;
  p.a1 = (bf16_t*)out; p.lse = lse;
  p.M = (int)M; p.HW = HW; p.HWP = ((HW + 15) / 16) * 16; p.Bc = Bc; p.T = T; p.D = D; p.n_cap = n_cap;
  p.col_base = col_base; p.ldp = ldp; p.bstride = bstride; p.skip_epi = g_scores_skip_epi; p.inv_hw = 1.0f / (float)HW;
  return p;
}

// one workgroup per (256 region rows, CAPB captions), at most one per CU; ntt = 16-word tiles per caption of this length class
template <bool TR>
static void sc_launch(const ScoresArgs& p, int ntt, hipStream_t stream) {
  const int tiles_m = (p.M + 255) / 256;
#define SC(N_, CAPB_) { const int grid = min(tiles_m * ((p.n_cap + CAPB_ - 1) / CAPB_), 256); \
                        hipLaunchKernelGGL((scores512_kernel<N_, TR>), dim3(grid), dim3(512), 0, stream, p); }
  switch (ntt) { case 1: SC(1, 16) break; case 2: SC(2, 8) break; case 3: SC(3, 4) break; case 4: SC(4, 4) break; default: SC(5, 2) break; }
#undef SC
}

// TRANSPOSED output (see the TR note above scores512_kernel): lpT[(row_base + j*16*ntt + t) * ld + b*bstride + hw] = log2-probability of
// word t of the class's j-th caption at region hw of image b (ld = B*HWP, bstride = HWP: [word rows][image region columns]; ld = HWP,
// bstride = rows*HWP: image-major); lse as in the untransposed kernel.  Any M (rows are clamped in the loads).
extern "C" int medmoe_local_scores_t(const void* ctx, const void* words, const int* cap_lens, void* lpT, float* lse, int B, int Bc,
                                     int HW, int T, int D, const int* cap_list, int n_cap, int ntt, long long row_base, long long ld,
                                     long long bstride, hipStream_t stream) {
  if (!ctx || !words || !cap_lens || !lpT || !lse || !cap_list) return MM_ERR_ARG;
  if (B <= 0 || Bc <= 0 || HW < 4 || (HW % 4) || T <= 0 || n_cap <= 0 || n_cap > Bc || ntt < 1 || ntt > 5 || row_base < 0) return MM_ERR_SHAPE;
  const long long M = (long long)B * HW;
  const int HWP = ((HW + 15) / 16) * 16;
  if ((D % 32) || D < 128 || M * D * 2 >= (1ll << 32) || (long long)Bc * T * D * 2 >= (1ll << 32) || (ld % 4) || (bstride % 4) || ld < HWP || bstride < HWP) return MM_ERR_SHAPE;
  sc_launch<true>(sc_args(ctx, words, cap_lens, cap_list, lpT, lse, M, HW, Bc, T, D, n_cap, row_base, ld, bstride), ntt, stream);
  return mm_check_launch();
}

// launcher used by medmoe_local_scores_ragged (loss.hip); returns false when the shape is not taken
bool mm_launch_scores512(const void* ctx, const void* words, const int* cap_lens, void* a1, float* lse, int B, int Bc, int HW, int T,
                         int D, const int* cap_list, int n_cap, int ntt, long long col_base, long long ldp, hipStream_t stream) {
  const long long M = (long long)B * HW;
  if (!g_use_scores512 || (D % 32) || D < 128 || M < 1024 || M * D * 2 >= (1ll << 32) || (long long)Bc * T * D * 2 >= (1ll << 32)) return false;
  sc_launch<false>(sc_args(ctx, words, cap_lens, cap_list, a1, lse, M, HW, Bc, T, D, n_cap, col_base, ldp, 0), ntt, stream);
  return true;
}
