// What the bf16 MFMA GEMM translation units share: the NT argument block, the epilogue every NT kernel leaves through, the tile and
// ring constants more than one kernel family uses, and the host launch function of each NT family (DESIGN.md has the map of the files).
// The library is built without relocatable device code: a kernel is launched only from the file that defines it, and every __device__
// function here is inlined into its callers.
#pragma once
#include "common.h"
#include <utility>

#define BM 128
#define BN 128
#define BK 64
#define BM2 256        // rows of a gemm_nt256 tile; the dispatch's "plain and tall" threshold is four of them

struct GemmNTArgs {      // filled, every field, by nt_args (gemm_nt.hip) alone: no default initialisers
  const bf16_t* A; const bf16_t* B; void* C;
  const float* bias; const bf16_t* residual; bf16_t* aux;
  const int* a_rowmap; const int* c_rowmap; const int4* tiles; const int* tile_count;
  long long strideB; long long strideBias;
  int M, N, K, lda, ldb, ldc, ldr, ldaux;
  int n_tiles_n, max_tiles_m;      // the tiling of the kernel that is chosen
  float alpha; int epi; int out_f32; int col_perm;
  const int* m_dev;      // plain (ungrouped) launches: if set, the row count M is read from the device (<= the host's M, which sizes the grid)
};

// family launch functions (library-internal).  `spec`: nt_spec() of gemm_nt.hip, -1 = only the generic build applies.  nt4w_launch returns
// false, having launched nothing, when gemm_nt4w_kernel has no build for `spec`; the other two fall back to their generic build.
MM_HIDDEN bool nt4w_launch(const GemmNTArgs& p, int spec, bool grouped, int grid, hipStream_t stream);
MM_HIDDEN void nt512_launch(const GemmNTArgs& p, int spec, bool grouped, int grid, hipStream_t stream);
MM_HIDDEN void nt256_launch(const GemmNTArgs& p, int spec, int grid, hipStream_t stream);

// -DNT_TIMING (tools/nt_timing.hip): per-wave, per-phase shader-clock totals of gemm_nt256_kernel.  The two __device__ variables below are
// DEFINED here: the tool compiles the NT files as ONE translation unit; a library built with these macros would define them once per file.
#ifdef NT_EXPERIMENT
__device__ int g_nt_dbg_skip = 0;        // experiment (wrong results): bit 0 skip the LDS fragment reads, 1 the MFMAs, 2 the epilogue, 3 the DMA
#define NT_X(...) __VA_ARGS__
#else
#define NT_X(...)
#endif
#ifdef NT_TIMING
__device__ unsigned long long g_nt_timing[8 * 8];     // [wave][phase]
#define NT_T(...) __VA_ARGS__
__device__ __forceinline__ long long nt_clk() {      // a clock read the scheduler cannot move MFMAs across
  __builtin_amdgcn_sched_barrier(0); const long long c = clock64(); __builtin_amdgcn_sched_barrier(0); return c;
}
#else
#define NT_T(...)
#endif

// EPI_GELU stores the PRE-activation in aux and EPI_MUL_DGELU evaluates GELU' of it (two transcendentals per element in
// the backward epilogue: measured 21-31k clk per 256x256 tile against 26.5k for its MFMAs).  EPI_GELU_DAUX stores GELU'(z)
// instead and EPI_MUL_AUX multiplies by it: the engine's pair.
enum { EPI_NONE = 0, EPI_GELU = 1, EPI_RELU = 2, EPI_MUL_DGELU = 3, EPI_MUL_DRELU = 4, EPI_GELU_DAUX = 5, EPI_MUL_AUX = 6 };

// SPEC < 0: every epilogue option decided at run time (70 KB of code - more than the instruction cache, and
// the tile seam then runs at instruction-fetch speed).  SPEC >= 0 = epi | bias << 3 | residual << 4 | aux << 5
// for a bf16 C with N % 8 == 0 and alpha == 1: the flags are compile-time constants and only that path is emitted.
#define NT_SPEC(epi, bias, res, aux) ((epi) | ((bias) << 3) | ((res) << 4) | ((aux) << 5))
// The plain (ungrouped) specialised builds that gemm_nt4w_kernel and gemm_nt512_kernel both have
#define NT_PLAIN_SPECS(X)                                                                               \
  X(NT_SPEC(EPI_NONE, 0, 0, 0))          /* dgrad */                                                    \
  X(NT_SPEC(EPI_NONE, 1, 0, 0))          /* QKV */                                                      \
  X(NT_SPEC(EPI_NONE, 1, 1, 0))          /* out-proj, FC2, patch embedding: + bias + residual */        \
  X(NT_SPEC(EPI_NONE, 0, 1, 0))                                                                         \
  X(NT_SPEC(EPI_GELU, 1, 0, 1))          /* FC1 forward, keeps the pre-activation */                    \
  X(NT_SPEC(EPI_GELU, 1, 0, 0))          /* frozen text tower FC1 */                                    \
  X(NT_SPEC(EPI_MUL_DGELU, 0, 0, 1))     /* FC2 dgrad x GELU' */                                        \
  X(NT_SPEC(EPI_GELU_DAUX, 1, 0, 1))     /* FC1 forward, keeps GELU'(z) */                              \
  X(NT_SPEC(EPI_MUL_AUX, 0, 0, 1))       /* FC2 dgrad x stored GELU' */                                 \
  X(NT_SPEC(EPI_NONE, 0, 0, 0) | 64)     /* fp32 C (local-loss context gradient) */

// Shared epilogue.  The B-matrix fragment rows are read through the permutation sigma(i) = 4*perm(i>>2) + (i&3),
// perm = {0,2,1,3} (see compute()), so lane (g = lane>>4) owns C[m][n..n+3] with n = 16*tn + 4*perm(g):
// lanes l and l+32 hold ADJACENT 4-column groups and one v_permlane32_swap per dword turns two 8-byte
// stores into one 16-byte store (cdna guide T21: the bf16 store tail is issue-bound per instruction).
// All operand loads (bias, residual, aux, row map) are issued up front with clamped addresses; only
// the stores are predicated.
// A finished bf16 C tile PARKED in registers as eight ready-to-store 16-byte pieces per lane: the 256x128
// kernel issues them one per LOAD segment of the next tile.  Stored at the seam, the 64 KB per CU leave as
// one burst from all 256 CUs at once (every tile takes the same time) and the chip waits for HBM to absorb
// 16 MB: measured 9200 clk per tile and wave in the epilogue against 13000 for the tile's MFMAs.
struct ParkedTile {
  uint4 c[8];
  int m_base, n_base, n_items, next;
};

// Returns the number of global STORE instructions this wave issued (wave-uniform): vmcnt counts stores
// too, so the counted waits of the DMA ring must leave exactly those youngest ops in flight.
// acc is the wave's whole accumulator array; the 64x64 block handled here starts at its 16-row tile TM0
// (no pointer into the array: it has to stay in registers through every inlined copy of this function).
// LDSX (gemm_nt4w, plain rows, bf16 output): the 16-byte pieces of a 32-row half of the block go through a wave-private 8-KB LDS
// region (C in its first 4 KB, the aux output in the second; 128-byte rows, 16-byte slots XOR-swizzled by (row >> 1) & 7: conflict-free
// both ways) and leave as FULL 128-byte lines, 8 rows per instruction.  The accumulator layout stores 16 rows x 64 bytes per instruction,
// and that shape is what a CU drains at 12.5 B/clk (tools/store_bw.hip: 30 GB/s per CU against 94 with whole lines) - it, not HBM, set
// the 9.2k clocks of a plain tile's epilogue.
typedef unsigned u32x4e_t __attribute__((ext_vector_type(4)));
template <bool PARK, int TM0 = 0, int TMS = 4, int TN0 = 0, int TNS = 4, bool LDSX = false>
__device__ __forceinline__ int nt_epilogue(const GemmNTArgs& p, f32x4_t (&acc)[TMS][TNS], int m_base, int m_end,
                                           int n_base, int group, int frag_row, int frag_q, ParkedTile* park, unsigned lds_x = 0u) {
  int n_stores = 0;
  const int pg = ((frag_q & 1) << 1) | (frag_q >> 1);
  long long mc[4];
  bool mok[4];
#pragma unroll
  for (int tm = 0; tm < 4; ++tm) {
    const int m = m_base + tm * 16 + frag_row;
    mok[tm] = m < m_end;
    const int mr = min(m, m_end - 1);
    mc[tm] = p.c_rowmap ? (long long)p.c_rowmap[mr] : (long long)mr;
  }
  int nn[4];
  bool nok[4];
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) {
    const int n = n_base + tn * 16 + pg * 4;
    nok[tn] = n < p.N;
    nn[tn] = min(n, p.N - 4);
  }
  float4 b4[4];
  if (p.bias) {
    const float* bias = p.bias + (long long)group * p.strideBias;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) b4[tn] = *(const float4*)(bias + nn[tn]);
  }
  uint2 res[4][4], axv[4][4];
  if (p.residual) {
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) res[tm][tn] = *(const uint2*)(p.residual + mc[tm] * p.ldr + nn[tn]);
  }
  const bool mul_epi = p.epi == EPI_MUL_DGELU || p.epi == EPI_MUL_DRELU || p.epi == EPI_MUL_AUX;
  if (mul_epi) {
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) axv[tm][tn] = *(const uint2*)(p.aux + mc[tm] * p.ldaux + nn[tn]);
  }
  const bool wide = !p.out_f32 && !p.col_perm && (p.N & 7) == 0;
  const bool upper = frag_q >= 2;
  // 16-byte store of two adjacent 4-column groups after the half-wave exchange
  auto store_pair = [&](bf16_t* base, long long ld, int tm, int j, uint2 lo, uint2 hi, bool is_aux) {
    // lo = this lane's packed tile 2j, hi = tile 2j+1
    auto r0 = __builtin_amdgcn_permlane32_swap(lo.x, hi.x, false, false);
    auto r1 = __builtin_amdgcn_permlane32_swap(lo.y, hi.y, false, false);
    if constexpr (PARK) {
      if (!is_aux) { park->c[tm * 2 + j] = make_uint4(r0[0], r1[0], r0[1], r1[1]); return; }
    }
    if constexpr (LDSX) {
      const int row_l = (tm & 1) * 16 + frag_row, slot = (2 * j + (upper ? 1 : 0)) * 2 + (frag_q & 1);
      const unsigned a = lds_x + (is_aux ? 4096u : 0u) + row_l * 128 + ((slot ^ ((row_l >> 1) & 7)) << 4);
      const u32x4e_t d = {(unsigned)r0[0], (unsigned)r1[0], (unsigned)r0[1], (unsigned)r1[1]};
      asm volatile("ds_write_b128 %0, %1" :: "v"(a), "v"(d) : "memory");
      return;
    }
    const int col = n_base + (2 * j + (upper ? 1 : 0)) * 16 + (frag_q & 1) * 8;
    const bool pred = mok[tm] && col < p.N;
    n_stores += (__ballot(pred) != 0ull) ? 1 : 0;     // an all-inactive store is branched around by the compiler
    if (pred) *(uint4*)(base + mc[tm] * ld + col) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
  };
#pragma unroll
  for (int tm = 0; tm < 4; ++tm) {
    uint2 o[4], zz[4];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[TM0 + tm][TN0 + tn][r] * p.alpha;
      if (p.bias) { v[0] += b4[tn].x; v[1] += b4[tn].y; v[2] += b4[tn].z; v[3] += b4[tn].w; }
      const bool ok = mok[tm] && nok[tn];
      zz[tn] = make_uint2(0u, 0u);
      if (p.epi == EPI_GELU_DAUX) {
        f32x2_t g0, g1, d0, d1;
        gelu_and_grad2((f32x2_t){v[0], v[1]}, g0, d0); gelu_and_grad2((f32x2_t){v[2], v[3]}, g1, d1);
        v[0] = g0[0]; v[1] = g0[1]; v[2] = g1[0]; v[3] = g1[1];
        if (p.aux) {
          zz[tn].x = pack2bf(d0[0], d0[1]); zz[tn].y = pack2bf(d1[0], d1[1]);
          if (!wide) { n_stores += (__ballot(ok) != 0ull) ? 1 : 0; if (ok) *(uint2*)(p.aux + mc[tm] * p.ldaux + nn[tn]) = zz[tn]; }
        }
      } else       if (p.epi == EPI_GELU) {
        if (p.aux) {
          zz[tn].x = pack2bf(v[0], v[1]); zz[tn].y = pack2bf(v[2], v[3]);
          if (!wide) { n_stores += (__ballot(ok) != 0ull) ? 1 : 0; if (ok) *(uint2*)(p.aux + mc[tm] * p.ldaux + nn[tn]) = zz[tn]; }
        }
        {
          const f32x2_t g0 = gelu2((f32x2_t){v[0], v[1]}), g1 = gelu2((f32x2_t){v[2], v[3]});
          v[0] = g0[0]; v[1] = g0[1]; v[2] = g1[0]; v[3] = g1[1];
        }
      } else if (p.epi == EPI_RELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if (p.residual) {
        const uint2 z = res[tm][tn];
        v[0] += bf2f((bf16_t)(z.x & 0xffff)); v[1] += bf2f((bf16_t)(z.x >> 16));
        v[2] += bf2f((bf16_t)(z.y & 0xffff)); v[3] += bf2f((bf16_t)(z.y >> 16));
      }
      if (mul_epi) {   // (acc + residual) * act'(aux)
        const uint2 z = axv[tm][tn];
        const float zf[4] = {bf2f((bf16_t)(z.x & 0xffff)), bf2f((bf16_t)(z.x >> 16)),
                             bf2f((bf16_t)(z.y & 0xffff)), bf2f((bf16_t)(z.y >> 16))};
        if (p.epi == EPI_MUL_DGELU) {
          const f32x2_t d0 = dgelu2((f32x2_t){zf[0], zf[1]}), d1 = dgelu2((f32x2_t){zf[2], zf[3]});
          v[0] *= d0[0]; v[1] *= d0[1]; v[2] *= d1[0]; v[3] *= d1[1];
        } else if (p.epi == EPI_MUL_AUX) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] *= zf[r];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] *= zf[r] > 0.f ? 1.f : 0.f;
        }
      }
      o[tn].x = pack2bf(v[0], v[1]); o[tn].y = pack2bf(v[2], v[3]);
      if (!wide) n_stores += (__ballot(ok) != 0ull) ? 1 : 0;
      if (!wide && ok) {
        // col_perm: store column n at position lpos(n) (the k-order the local-loss Gm.A product reads)
        const int n = nn[tn];
        const int ns = p.col_perm ? ((n & ~31) + ((((n & 31) & 15) >> 2) << 3) + (((n & 31) >> 4) << 2)) : n;
        if (p.out_f32) *(float4*)((float*)p.C + mc[tm] * p.ldc + ns) = make_float4(v[0], v[1], v[2], v[3]);
        else *(uint2*)((bf16_t*)p.C + mc[tm] * p.ldc + ns) = o[tn];
      }
    }
    if (wide) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        store_pair((bf16_t*)p.C, p.ldc, tm, j, o[2 * j], o[2 * j + 1], false);
        if ((p.epi == EPI_GELU || p.epi == EPI_GELU_DAUX) && p.aux) store_pair(p.aux, p.ldaux, tm, j, zz[2 * j], zz[2 * j + 1], true);
      }
      if constexpr (LDSX) {
        if (tm & 1) {                                   // rows (tm - 1) * 16 .. tm * 16 + 15 of the block are in the LDS: out as whole lines
          const bool has_aux = (p.epi == EPI_GELU || p.epi == EPI_GELU_DAUX) && p.aux;
          const int lane = frag_q * 16 + frag_row, c8 = lane & 7;
          const int col = n_base + c8 * 8;
          u32x4e_t vc[4], va[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row_l = i * 8 + (lane >> 3);
            const unsigned a = lds_x + row_l * 128 + ((c8 ^ ((row_l >> 1) & 7)) << 4);
            asm volatile("ds_read_b128 %0, %1" : "=v"(vc[i]) : "v"(a));
            if (has_aux) asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(va[i]) : "v"(a));
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m = m_base + (tm - 1) * 16 + i * 8 + (lane >> 3);
            const bool pred = m < m_end && col < p.N;
            const int ns = (__ballot(pred) != 0ull) ? 1 : 0;
            n_stores += has_aux ? 2 * ns : ns;
            if (pred) {
              // nontemporal: C is written once and read by a later kernel - streaming it past the L2 keeps the A / B panels of the tiles
              // in flight resident (QKV forward 1040 -> 1163, plain 3072 x 768 1092 -> 1182 TFLOP/s; no change where N = 768)
              __builtin_nontemporal_store(vc[i], (u32x4e_t*)((bf16_t*)p.C + (long long)m * p.ldc + col));
              if (has_aux) __builtin_nontemporal_store(va[i], (u32x4e_t*)(p.aux + (long long)m * p.ldaux + col));
            }
          }
        }
      }
    }
  }
  if constexpr (PARK) { park->m_base = m_base; park->n_base = n_base; park->next = 0; park->n_items = 8; }
  return n_stores;
}

// store the next parked piece (number `item`, 0..7) of the C tile and rotate the queue - the pieces live in
// registers, which cannot be indexed at run time, and an 8-way switch costs more scalar branching per k-step
// than 28 v_mov; returns 1 if a store instruction issued (wave-uniform)
__device__ __forceinline__ int park_store_next(const GemmNTArgs& p, ParkedTile& pk, int m_end, int frag_row, int frag_q) {
  const int item = pk.next++;
  const uint4 v = pk.c[0];
#pragma unroll
  for (int i = 0; i < 7; ++i) pk.c[i] = pk.c[i + 1];
  const int tm = item >> 1, j = item & 1;
  const int row = pk.m_base + tm * 16 + frag_row;
  const int col = pk.n_base + (2 * j + (frag_q >= 2 ? 1 : 0)) * 16 + (frag_q & 1) * 8;
  const bool pred = row < m_end && col < p.N;
  if (__builtin_amdgcn_readfirstlane(__ballot(pred) != 0ull ? 1 : 0) == 0) return 0;
  if (pred) *(uint4*)((bf16_t*)p.C + (long long)row * p.ldc + col) = v;
  return 1;
}

// The ring of four 32 KB LDS sub-stages of gemm_nt512_kernel; gemm_tn512_kernel, gemm_tn4w_kernel and scores512_kernel are built on it.
#define SUB3 (512 * 64)
#define NRING 4        // sub-stages in the LDS ring (5 x 32 KB = the whole 160 KB measured no faster, 3 measured 5 % slower)
__device__ __forceinline__ void wait_vmcnt_ring4(int n) {
  if (n == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if (n == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (n >= 28) asm volatile("s_waitcnt vmcnt(28)" ::: "memory");
  else if (n >= 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
  else if (n >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if (n >= 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <typename F, int... Is>
__device__ __forceinline__ void static_for_seq(F& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void static_for(F& f) { static_for_seq(f, std::make_integer_sequence<int, N>{}); }
