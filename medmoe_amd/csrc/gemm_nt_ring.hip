// The two eight-wave NT GEMM kernels (LDS ring filled by LDS-DMA behind counted vmcnt waits, ping-pong between the two waves of a SIMD, persistent
// over tiles): gemm_nt256_kernel, and gemm_nt512_kernel, which gemm_nt.hip keeps behind gemm_nt4w_kernel for the specs that one has no build for.
#include "gemm_nt.h"

// s_waitcnt vmcnt(<= n): the immediate must be a literal, and a 64-way switch on it costs hundreds of cycles
// of scalar branching per k-step.  Waiting for a smaller count than allowed is always correct (it only waits
// for more), so only the counts the DMA rings actually produce get their own immediate: 6 = one stage in
// flight, +1/+2 parked stores, +8 pre-activation stores of a GELU epilogue; anything else rounds down.
__device__ __forceinline__ void wait_vmcnt(int n) {
  if (n == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if (n == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  else if (n == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (n >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if (n >= 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
  else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// s_waitcnt vmcnt(6 + n): the immediate must be a literal
__device__ __forceinline__ void wait_vmcnt_plus6(int n) {
  switch (n) {
#define WV(k, k6) case k: asm volatile("s_waitcnt vmcnt(" #k6 ")" ::: "memory"); break;
    WV(1, 7) WV(2, 8) WV(3, 9) WV(4, 10) WV(5, 11) WV(6, 12) WV(7, 13) WV(8, 14) WV(9, 15) WV(10, 16) WV(11, 17) WV(12, 18)
    WV(13, 19) WV(14, 20) WV(15, 21) WV(16, 22)
#undef WV
    default: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
  }
}

// ---------------------------------------------------------------------------------------------
// gemm_nt256: 256x128 block tile, 8 waves (4x2 of 64x64), K-step 64, THREE-stage LDS ring filled by
// LDS-DMA with a COUNTED s_waitcnt vmcnt(6) + raw s_barrier per k-step (one stage = 6 DMA ops per
// thread stays in flight across the barrier; cdna guide "Pipelining across barriers"), persistent
// over tiles with separate load / compute cursors so the ring never drains at tile seams.
// 85 flop per LDS-filled byte (vs 64 for the 128x128 kernel): the 128^2 kernel sits on the
// L2->LDS fill rate at K=768.  Used for the plain (ungrouped, unmapped-A) Linear GEMMs.
// ---------------------------------------------------------------------------------------------
#define STAGE2 (384 * 128)
template <int SPEC>
__global__ __launch_bounds__(512, 2) void gemm_nt256_kernel(GemmNTArgs p_in) {
  GemmNTArgs p = p_in;
  if (p.m_dev) { p.M = min(*p.m_dev, p.M); p.max_tiles_m = (p.M + BM2 - 1) / BM2; }
  if constexpr (SPEC >= 0) {
    p.epi = SPEC & 7; p.out_f32 = (SPEC >> 6) & 1; p.col_perm = 0; p.c_rowmap = nullptr; p.a_rowmap = nullptr; p.alpha = 1.f;
    if (!(SPEC & 8)) p.bias = nullptr;
    if (!(SPEC & 16)) p.residual = nullptr;
    if (!(SPEC & 32)) p.aux = nullptr;
    __builtin_assume((p.N & 7) == 0);
    if (SPEC & 8) __builtin_assume(p.bias != nullptr);
    if (SPEC & 16) __builtin_assume(p.residual != nullptr);
    if (SPEC & 32) __builtin_assume(p.aux != nullptr);
  }
  __shared__ __attribute__((aligned(16))) char smem[3 * STAGE2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int frag_row = lane & 15, frag_q = lane >> 4, swz = lane & 7;
  const int G = gridDim.x;
  const int my = xcd_remap(blockIdx.x, G);
  const int total = p.max_tiles_m * p.n_tiles_n;
  const int nt = p.K / BK;

  // Tile order: ids walk "super rows" of SM m-tiles; inside one, blocks of (SM m x SN n) tiles are
  // consecutive, so the 32 tiles an XCD holds at a time share SM A panels and SN B panels (each A chunk is
  // fetched once per SN tiles, each B chunk once per SM tiles) instead of one A panel and every B panel.
  constexpr int SM = 4, SN = 8;   // 2x16 / 8x4 / non-temporal A loads measured within noise of this (profiles/r01_notes.md)
  struct Tile { int m0, n0; };
  auto decode = [&](int id) -> Tile {
    Tile t;
    const int per_super = SM * p.n_tiles_n;
    const int sg = id / per_super, r = id - sg * per_super;
    const int rows = min(SM, p.max_tiles_m - sg * SM);          // m-tiles in this (possibly last) super row
    const int blk = SN * rows;                                  // tiles per (rows x SN) block
    const int nfull = p.n_tiles_n / SN;
    int tile_m, tile_n;
    if (r < nfull * blk) { const int nb = r / blk, w = r - nb * blk; tile_n = nb * SN + (w % SN); tile_m = sg * SM + (w / SN); }
    else {                                                      // ragged tail block: n_tiles_n % SN columns
      const int r2 = r - nfull * blk, nc = p.n_tiles_n - nfull * SN;
      tile_n = nfull * SN + r2 % nc; tile_m = sg * SM + r2 / nc;
    }
    t.m0 = tile_m * BM2; t.n0 = tile_n * BN;
    return t;
  };
  // per-lane sources as 32-bit BYTE offsets from the (uniform) A / B base: the DMA then uses the SGPR-base +
  // VGPR-offset address form and the six cursors cost 6 VGPRs instead of 12 (the host routes operands
  // of 4 GB or more to the 128x128 kernel)
  NT_X(const int dbg_skip = g_nt_dbg_skip;)
  unsigned src[6];
  auto setup = [&](const Tile& t) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int q = i * 512 + tid;
      const int row = q >> 3;
      const int c = (q & 7) ^ (row & 7);
      if (i < 4) src[i] = (unsigned)min(t.m0 + row, p.M - 1) * (unsigned)(p.lda * 2) + c * 16;
      else src[i] = (unsigned)min(t.n0 + row - BM2, p.N - 1) * (unsigned)(p.ldb * 2) + c * 16;
    }
  };
  auto stage = [&](int buf, int k0) {
    char* sb = smem + buf * STAGE2 + wid * 1024;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        __builtin_amdgcn_global_load_lds(GLB_PTR((const char*)(i < 4 ? p.A : p.B) + k0 * 2 + src[i]), LDS_PTR(sb + i * 8192), 16, 0, 0);
  };
  f32x4_t acc[4][4];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  };
  const int sig = ((((frag_row >> 2) & 1) << 1 | (frag_row >> 3)) << 2) | (frag_row & 3);   // sigma(frag_row), see nt_epilogue
  bf16x8_t af[2][4], bf[2][4];          // one k-step of fragments: [k sub-step][16-row tile]
  auto read_frags = [&](int buf) {
    const char* sA = smem + buf * STAGE2 + (wm * 64 + frag_row) * 128;
    const char* sB = smem + buf * STAGE2 + BM2 * 128 + (wn * 64 + sig) * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int coff = ((ks * 4 + frag_q) ^ swz) * 16;
      const int coffb = ((ks * 4 + frag_q) ^ (sig & 7)) * 16;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        af[ks][t] = *(const bf16x8_t*)(sA + t * 2048 + coff);
        bf[ks][t] = *(const bf16x8_t*)(sB + t * 2048 + coffb);
      }
    }
  };
  // the 32 MFMAs of one k-step with the wave's six DMA pieces of a later stage issued IN BETWEEN (after every
  // fifth MFMA): a DMA issue stalls the in-order wave for tens of cycles while the address unit is busy, and
  // here that stall only delays MFMA issue behind MFMAs still executing; in the LOAD segment it was the
  // critical path (measured 1100 clk per LOAD segment against 550 for the partner's MFMAs)
  auto compute = [&](bool dma, int wbuf, int k0) __attribute__((always_inline)) {
    char* sw = smem + wbuf * STAGE2 + wid * 1024;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int tm = 0; tm < 4; ++tm) {
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[ks][tn], af[ks][tm], acc[tm][tn], 0, 0, 0);
        if (tm < 3) {
          const int i = ks * 3 + tm;
          if (dma) __builtin_amdgcn_global_load_lds(GLB_PTR((const char*)(i < 4 ? p.A : p.B) + k0 * 2 + src[i]), LDS_PTR(sw + i * 8192), 16, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
  };
  const bool can_park = !p.out_f32 && !p.col_perm && (p.N & 7) == 0;
  ParkedTile pk;
  pk.n_items = 0; pk.next = 0; pk.m_base = 0; pk.n_base = 0;
  auto epilogue = [&](const Tile& t) -> int {
    if (can_park) return nt_epilogue<true>(p, acc, t.m0 + wm * 64, p.M, t.n0 + wn * 64, 0, frag_row, frag_q, &pk);
    return nt_epilogue<false>(p, acc, t.m0 + wm * 64, p.M, t.n0 + wn * 64, 0, frag_row, frag_q, nullptr);
  };
  auto flush_parked = [&]() -> int {
    int n = 0;
    while (pk.next < pk.n_items) n += park_store_next(p, pk, p.M, frag_row, frag_q);
    return n;
  };

  if (my >= total) return;
  const int my_tiles = (total - my + G - 1) / G;
  Tile ct = decode(my);
  setup(ct);
  // vmcnt bookkeeping: the wait is always for the wave's SECOND-newest stage; younger than it are the stores
  // issued between the two stages (st_old), the newest stage's pieces (dn) and the stores since (st_new)
  int st_old = 0, st_new = 0, dn = 0, wb = 0, rb = 0;
  // DMA cursor: tile lid, k-step lk.  Every wave issues its own six pieces of every stage, in stage order.
  int lid = my, lk = 0;
  bool lmore = true;
  auto advance_load = [&]() {
    wb = (wb == 2) ? 0 : wb + 1;
    if (++lk == nt) {
      lk = 0; lid += G;
      if (lid < total) { const Tile lt = decode(lid); setup(lt); } else lmore = false;
    }
  };
  auto wait_second_newest = [&]() { wait_vmcnt(__builtin_amdgcn_readfirstlane(st_old + dn + st_new)); };
  const int grp = __builtin_amdgcn_readfirstlane(wid >> 2);
  zero_acc();
  // prologue: group 0 starts two stages ahead of its compute, group 1 three (see below)
  for (int i = 0; i < 2 + grp; ++i) { st_old = st_new; st_new = 0; stage(wb, lk * BK); dn = 6; advance_load(); }
  NT_T(long long t_wait = 0, t_bar = 0, t_load = 0, t_comp = 0, t_epi = 0; const long long t_begin = nt_clk();)
  if (grp == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  __builtin_amdgcn_s_barrier();                   // stage 0 landed for every wave
  asm volatile("" ::: "memory");
  // PING-PONG: the two waves of a SIMD (wave w and w+4) alternate roles every segment, separated by one
  // s_barrier: while group 0 runs the 32 MFMAs of its k-step (the matrix pipe is per SIMD and fully paced),
  // group 1 reads its next fragments from LDS, then they swap.  In lock-step (both waves reading, then both
  // computing) the matrix pipe idled through every LDS-read latency: measured 1800 clk per k-step against
  // 1024 of MFMA issue (tools/nt_timing.hip, profiles/r01_notes.md).
  // Every wave runs the same program  { LOAD(t); barrier; COMPUTE(t) [+ epilogue]; barrier }  and group 1 is
  // shifted by one barrier, so its LOAD coincides with group 0's COMPUTE (absolute segment 2t+g for LOAD(t),
  // 2t+1+g for COMPUTE(t)).  Stage s lives in buffer s % 3 and is read in segments 2s (group 0) and 2s+1
  // (group 1).  COMPUTE(t) issues the wave's pieces of stage t+2 (group 0, segment 2t+1) or t+3 (group 1,
  // segment 2t+2) into the buffer last read in segment 2t-1 resp. 2t+1.  A stage must be complete before
  // segment 2s: group 0 waits for its SECOND-newest stage at the end of COMPUTE (segment 2s-1), group 1 at the
  // end of LOAD (segment 2s-1) - three and four segments after issue.
  auto seg_barrier = [&]() {
    NT_T(const long long b0 = nt_clk();)
    __builtin_amdgcn_sched_barrier(0);
    if (true NT_X(&& !(dbg_skip & 16))) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    NT_T(t_bar += nt_clk() - b0;)
  };
  auto step = [&](bool last) __attribute__((always_inline)) {
    NT_T(const long long c0 = nt_clk();)
    if (true NT_X(&& !(dbg_skip & 1))) read_frags(rb);
    rb = (rb == 2) ? 0 : rb + 1;
    if (pk.next < pk.n_items) st_new += park_store_next(p, pk, p.M, frag_row, frag_q);   // one parked piece of the previous tile
    NT_T(const long long c1 = nt_clk(); t_load += c1 - c0;)
    if (grp == 1 NT_X(&& !(dbg_skip & 32))) { wait_second_newest(); NT_T(t_wait += nt_clk() - c1;) }
    seg_barrier();
    NT_T(const long long c2 = nt_clk();)
    const bool dma = lmore NT_X(&& !(dbg_skip & 8));
    st_old = st_new; st_new = 0; dn = dma ? 6 : 0;
    if (true NT_X(&& !(dbg_skip & 2))) compute(dma, wb, lk * BK);
    if (lmore) advance_load();
    NT_T(const long long c3 = nt_clk(); t_comp += c3 - c2;)
    if (last) {
      st_new += flush_parked();                   // only when K is shorter than the piece count
      if (true NT_X(&& !(dbg_skip & 4))) st_new += __builtin_amdgcn_readfirstlane(epilogue(ct));
      zero_acc();
      NT_T(t_epi += nt_clk() - c3;)
    }
    NT_T(const long long c4 = nt_clk();)
    if (grp == 0 NT_X(&& !(dbg_skip & 32))) { wait_second_newest(); NT_T(t_wait += nt_clk() - c4;) }
    seg_barrier();
  };
  if (grp == 1) seg_barrier();
  for (int ti = 0; ti < my_tiles; ++ti) {
    for (int k = 1; k < nt; ++k) step(false);
    step(true);
    if (ti + 1 < my_tiles) ct = decode(my + (ti + 1) * G);
  }
  if (grp == 0) seg_barrier();
  flush_parked();                                 // the last tile
  NT_T(if ((tid & 63) == 0) { unsigned long long* g = g_nt_timing + wid * 8; atomicAdd(&g[0], (unsigned long long)(nt_clk() - t_begin));
         atomicAdd(&g[1], (unsigned long long)t_wait); atomicAdd(&g[2], (unsigned long long)t_bar); atomicAdd(&g[3], (unsigned long long)t_load);
         atomicAdd(&g[4], (unsigned long long)t_comp); atomicAdd(&g[5], (unsigned long long)t_epi); atomicAdd(&g[6], 1ull); })
}

// ---------------------------------------------------------------------------------------------
// gemm_nt512: 256x256 block tile, 8 waves (2x4 of 128x64), for wide-N Linear GEMMs.
// The 256x128 kernel moves 48 KB through the CU's address/L1 path per 1100 clk of MFMA work (43 B/clk of
// the 64 B/clk the path can carry, measured ~46 B/clk with four waves issuing): every DMA issue stalls its
// wave ~90 clk, and that stall, not the matrix pipe, sets the k-step.  256x256 needs 32 KB per 1100 clk.
//   * k sub-step 32 (ONE 16x16x32 MFMA deep): 32 MFMAs per wave and sub-step, 12 ds_read_b128, 4 DMA pieces.
//   * LDS: ring of FOUR 32 KB sub-stages (512 rows x 64 B).  Two 64-B rows share one 128-B LDS line:
//     row r, 16-B k-chunk c lives in line r >> 1 at chunk (((r & 1) << 2 | c) ^ ((r >> 1) & 7)) - conflict
//     free for the b128 fragment reads (same lane-group argument as the 128-B-row image).
//   * ping-pong as in gemm_nt256: { LOAD(u); barrier; COMPUTE(u); barrier }, group 1 shifted by one barrier.
//     LOAD(u) issues sub-stage u+3 into the buffer of u-1 (read one barrier earlier at the latest) and the
//     wave waits for its THIRD-newest sub-stage before the barrier that precedes the first read of it:
//     four to five segments after issue.
// ---------------------------------------------------------------------------------------------

// GROUPED: tiles come from the device-side table p.tiles (group, m0, m_end, -) of 256-ROW tiles, B / bias are
// per group, A rows are gathered through p.a_rowmap and C rows scattered through p.c_rowmap (expert GEMMs, dGm).
template <int SPEC, bool GROUPED = false>
__global__ __launch_bounds__(512, 2) void gemm_nt512_kernel(GemmNTArgs p_in) {
  GemmNTArgs p = p_in;
  if (!GROUPED && p.m_dev) { p.M = min(*p.m_dev, p.M); p.max_tiles_m = (p.M + 255) / 256; }
  if constexpr (SPEC >= 0) {
    p.epi = SPEC & 7; p.out_f32 = (SPEC >> 6) & 1; p.col_perm = 0; p.alpha = 1.f;
    if (!GROUPED) { p.c_rowmap = nullptr; p.a_rowmap = nullptr; }
    if (!(SPEC & 8)) p.bias = nullptr;
    if (!(SPEC & 16)) p.residual = nullptr;
    if (!(SPEC & 32)) p.aux = nullptr;
    __builtin_assume((p.N & 7) == 0);
    if (SPEC & 8) __builtin_assume(p.bias != nullptr);
    if (SPEC & 16) __builtin_assume(p.residual != nullptr);
    if (SPEC & 32) __builtin_assume(p.aux != nullptr);
  }
  __shared__ __attribute__((aligned(16))) char smem[NRING * SUB3];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid & 1, wn = wid >> 1;          // the two waves of a SIMD (w, w+4) take different column strips
  const int frag_row = lane & 15, frag_q = lane >> 4;
  const int G = gridDim.x;
  const int my = xcd_remap(blockIdx.x, G);
  const int total = GROUPED ? *p.tile_count * p.n_tiles_n : p.max_tiles_m * p.n_tiles_n;
  const int nu = p.K / 32;                        // sub-steps per tile

  constexpr int SM = 4, SN = 8;                   // tile order as in gemm_nt256
  struct Tile { int m0, n0, m_end, group; };
  auto decode = [&](int id) -> Tile {
    Tile t;
    if constexpr (GROUPED) {                      // n-tiles of one m-tile are consecutive (they share the gathered A rows)
      const int tm = id / p.n_tiles_n;
      const int4 e = p.tiles[tm];
      t.group = e.x; t.m0 = e.y; t.m_end = e.z; t.n0 = (id - tm * p.n_tiles_n) * 256;
      return t;
    }
    t.group = 0; t.m_end = p.M;
    const int per_super = SM * p.n_tiles_n;
    const int sg = id / per_super, r = id - sg * per_super;
    const int rows = min(SM, p.max_tiles_m - sg * SM);
    const int blk = SN * rows;
    const int nfull = p.n_tiles_n / SN;
    int tile_m, tile_n;
    if (r < nfull * blk) { const int nb = r / blk, w = r - nb * blk; tile_n = nb * SN + (w % SN); tile_m = sg * SM + (w / SN); }
    else {
      const int r2 = r - nfull * blk, nc = p.n_tiles_n - nfull * SN;
      tile_n = nfull * SN + r2 % nc; tile_m = sg * SM + r2 / nc;
    }
    // row tiles are walked from the LAST to the first: the kernel that produced A wrote it front to back, so its tail is
    // what still sits in the Infinity Cache / L2 when this kernel starts
    t.m0 = (p.max_tiles_m - 1 - tile_m) * 256; t.n0 = tile_n * 256;
    return t;
  };
  // DMA piece i of wave w fills LDS bytes [(i * 8 + w) * 1024, +1024) of the sub-stage: 8 lines = 16 rows.
  // Lane l writes chunk l & 7 of line (i * 8 + w) * 8 + (l >> 3): it must FETCH what that slot holds.
  // Per-lane sources are 32-bit byte offsets from a per-TILE base (uniform, 64-bit): a tile's rows span at most
  // 256 * ld elements, so operands beyond 4 GB (the 22 GB pair matrices) still work; gathered A rows (a_rowmap)
  // are offsets from p.A itself and need the whole A below 4 GB (checked on the host).
  unsigned src[4];
  const char* baseA = (const char*)p.A;
  const char* baseB = (const char*)p.B;
  auto setup = [&](const Tile& t_in) {
    Tile t = t_in;
    NT_X(if (g_nt_dbg_skip & 64) { t.m0 = 0; t.n0 = 0; })      // experiment: every workgroup fetches tile 0's operands (all L2 hits)
    const bool gather = GROUPED && p.a_rowmap;
    baseA = (const char*)(p.A + (gather ? 0ll : (long long)t.m0 * p.lda));
    baseB = (const char*)(p.B + (GROUPED ? (long long)t.group * p.strideB : 0ll) + (long long)t.n0 * p.ldb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int line = (i * 8 + wid) * 8 + (lane >> 3);
      const int lc = (lane & 7) ^ (line & 7);
      const int row = 2 * line + (lc >> 2);       // 0..255 A rows, 256..511 B rows
      if (i < 2) {
        const int m = min(t.m0 + row, t.m_end - 1);
        const int r = gather ? p.a_rowmap[m] : m - t.m0;
        src[i] = (unsigned)r * (unsigned)(p.lda * 2) + (lc & 3) * 16;
      } else src[i] = (unsigned)min(row - 256, p.N - 1 - t.n0) * (unsigned)(p.ldb * 2) + (lc & 3) * 16;
    }
  };
  auto stage = [&](int buf, int k0) {
    char* sb = smem + buf * SUB3 + wid * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds(GLB_PTR((i < 2 ? baseA : baseB) + k0 * 2 + src[i]), LDS_PTR(sb + i * 8192), 16, 0, 0);
  };
  f32x4_t acc[8][4];
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  };
  const int sig = ((((frag_row >> 2) & 1) << 1 | (frag_row >> 3)) << 2) | (frag_row & 3);   // sigma(frag_row), see nt_epilogue
  const int offA = (wm * 128) * 64 + (frag_row >> 1) * 128 + (((((frag_row & 1) << 2) | frag_q) ^ ((frag_row >> 1) & 7)) << 4);
  const int offB = (256 + wn * 64) * 64 + (sig >> 1) * 128 + (((((sig & 1) << 2) | frag_q) ^ ((sig >> 1) & 7)) << 4);
  bf16x8_t af[8], bf[4];
  auto read_frags = [&](int buf) __attribute__((always_inline)) {
    const char* sA = smem + buf * SUB3 + offA;
    const char* sB = smem + buf * SUB3 + offB;
#pragma unroll
    for (int t = 0; t < 8; ++t) af[t] = *(const bf16x8_t*)(sA + t * 1024);
#pragma unroll
    for (int t = 0; t < 4; ++t) bf[t] = *(const bf16x8_t*)(sB + t * 1024);
  };
  auto compute = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int tm = 0; tm < 8; ++tm)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn)
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[tn], af[tm], acc[tm][tn], 0, 0, 0);
  };
  auto epilogue = [&](const Tile& t) __attribute__((always_inline)) -> int {
    int n = 0;
    n += nt_epilogue<false, 0, 8>(p, acc, t.m0 + wm * 128, t.m_end, t.n0 + wn * 64, t.group, frag_row, frag_q, nullptr);
    n += nt_epilogue<false, 4, 8>(p, acc, t.m0 + wm * 128 + 64, t.m_end, t.n0 + wn * 64, t.group, frag_row, frag_q, nullptr);
    return n;
  };

  if (my >= total) return;
  const int my_tiles = (total - my + G - 1) / G;
  Tile ct = decode(my);
  setup(ct);
  // vmcnt bookkeeping: the wait is for the wave's THIRD-newest sub-stage; younger than it are s2 stores,
  // d1 pieces, s1 stores, d0 pieces, s0 stores (issue order)
  int s3 = 0, s2 = 0, s1 = 0, s0 = 0, d2 = 0, d1 = 0, d0 = 0, wb = 0, rb = 0;
  int lid = my, lk = 0;
  bool lmore = true;
  auto issue = [&]() __attribute__((always_inline)) {
    s3 = s2; s2 = s1; s1 = s0; s0 = 0; d2 = d1; d1 = d0; d0 = 0;
    if (lmore) {
      stage(wb, lk * 32);
      d0 = 4;
      wb = (wb == NRING - 1) ? 0 : wb + 1;
      if (++lk == nu) {
        lk = 0; lid += G;
        if (lid < total) { const Tile lt = decode(lid); setup(lt); } else lmore = false;
      }
    }
  };
  auto wait_third_newest = [&]() { wait_vmcnt_ring4(__builtin_amdgcn_readfirstlane(NRING == 5 ? s3 + d2 + s2 + d1 + s1 + d0 + s0 : NRING == 3 ? s1 + d0 + s0 : s2 + d1 + s1 + d0 + s0)); };
  const int grp = __builtin_amdgcn_readfirstlane(wid >> 2);
  zero_acc();
  for (int i = 0; i < NRING - 1; ++i) issue();    // sub-stages 0 .. NRING-2 (the host guarantees K >= 128)
  wait_third_newest();
  __builtin_amdgcn_s_barrier();                   // sub-stage 0 landed for every wave
  asm volatile("" ::: "memory");
  NT_T(long long t_wait = 0, t_bar = 0, t_load = 0, t_comp = 0, t_epi = 0; const long long t_begin = nt_clk();)
  auto seg_barrier = [&]() {
    NT_T(const long long b0 = nt_clk();)
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    NT_T(t_bar += nt_clk() - b0;)
  };
  // Tile seam: group 1 runs its epilogue right after its last COMPUTE, before the barrier; group 0 runs its
  // own AFTER that barrier - i.e. during group 1's last COMPUTE + epilogue.  Both epilogues (store issue,
  // operand-load latency) then overlap each other instead of each idling the other group.  One copy of the
  // epilogue code serves both: the loop body is rotated to start at COMPUTE, and the barrier sits before the
  // epilogue for group 0 and after it for group 1 (the GELU epilogue alone is 20 KB of a 64 KB I-cache).
  auto load_seg = [&]() __attribute__((always_inline)) {
    NT_T(const long long c0 = nt_clk();)
    read_frags(rb);
    rb = (rb == NRING - 1) ? 0 : rb + 1;
    issue();
    NT_T(const long long c1 = nt_clk(); t_load += c1 - c0;)
    if (grp == 1) { wait_third_newest(); NT_T(t_wait += nt_clk() - c1;) }
    seg_barrier();
  };
  auto body = [&](bool last) __attribute__((always_inline)) {
    NT_T(const long long c2 = nt_clk();)
    compute();
    NT_T(const long long c3 = nt_clk(); t_comp += c3 - c2;)
    if (grp == 0) { wait_third_newest(); NT_T(t_wait += nt_clk() - c3;) seg_barrier(); }
    if (last) {
      NT_T(const long long c4 = nt_clk();)
      s0 += __builtin_amdgcn_readfirstlane(epilogue(ct));
      zero_acc();
      NT_T(t_epi += nt_clk() - c4;)
    }
    if (grp == 1) seg_barrier();
    load_seg();                                   // the next sub-step's (past the end: reads nothing that is used)
  };
  if (grp == 1) seg_barrier();
  load_seg();
  for (int ti = 0; ti < my_tiles; ++ti) {
    for (int k = 1; k < nu; ++k) body(false);
    body(true);
    if (ti + 1 < my_tiles) ct = decode(my + (ti + 1) * G);
  }
  if (grp == 0) seg_barrier();
  NT_T(if ((tid & 63) == 0) { unsigned long long* g = g_nt_timing + wid * 8; atomicAdd(&g[0], (unsigned long long)(nt_clk() - t_begin));
         atomicAdd(&g[1], (unsigned long long)t_wait); atomicAdd(&g[2], (unsigned long long)t_bar); atomicAdd(&g[3], (unsigned long long)t_load);
         atomicAdd(&g[4], (unsigned long long)t_comp); atomicAdd(&g[5], (unsigned long long)t_epi); atomicAdd(&g[6], 1ull); })
}

void nt256_launch(const GemmNTArgs& p, int spec, int grid, hipStream_t stream) {
  switch (spec) {
#define NT_CASE(s) case s: hipLaunchKernelGGL(gemm_nt256_kernel<s>, dim3(grid), dim3(512), 0, stream, p); break;
    NT_CASE(NT_SPEC(EPI_NONE, 0, 0, 0))          // dgrad
    NT_CASE(NT_SPEC(EPI_NONE, 1, 0, 0))          // QKV
    NT_CASE(NT_SPEC(EPI_NONE, 1, 1, 0))          // out-proj, FC2, patch embedding: + bias + residual
    NT_CASE(NT_SPEC(EPI_NONE, 0, 1, 0))
    NT_CASE(NT_SPEC(EPI_GELU, 1, 0, 1))          // FC1 forward, keeps the pre-activation
    NT_CASE(NT_SPEC(EPI_GELU, 1, 0, 0))          // frozen text tower FC1
    NT_CASE(NT_SPEC(EPI_MUL_DGELU, 0, 0, 1))     // FC2 dgrad x GELU'
    NT_CASE(NT_SPEC(EPI_GELU_DAUX, 1, 0, 1))
    NT_CASE(NT_SPEC(EPI_MUL_AUX, 0, 0, 1))
#undef NT_CASE
    default: hipLaunchKernelGGL(gemm_nt256_kernel<-1>, dim3(grid), dim3(512), 0, stream, p); break;
  }
}

void nt512_launch(const GemmNTArgs& p, int spec, bool grouped, int grid, hipStream_t stream) {
#define NT_CASE(s) case s: hipLaunchKernelGGL((gemm_nt512_kernel<s, false>), dim3(grid), dim3(512), 0, stream, p); return;
#define NT_CASE_G(s) case s: hipLaunchKernelGGL((gemm_nt512_kernel<s, true>), dim3(grid), dim3(512), 0, stream, p); return;
  if (!grouped) switch (spec) {
    NT_PLAIN_SPECS(NT_CASE)
    default: hipLaunchKernelGGL((gemm_nt512_kernel<-1, false>), dim3(grid), dim3(512), 0, stream, p); return;
  }
  switch (spec) {
    NT_CASE_G(NT_SPEC(EPI_NONE, 0, 0, 0))            // expert dgrad, dGm
    NT_CASE_G(NT_SPEC(EPI_RELU, 1, 0, 0))            // expert projections / scale-attention hidden layer
    NT_CASE_G(NT_SPEC(EPI_MUL_DRELU, 0, 1, 1))       // gradient through the projection ReLU, accumulated
    default: hipLaunchKernelGGL((gemm_nt512_kernel<-1, true>), dim3(grid), dim3(512), 0, stream, p); return;
  }
#undef NT_CASE
#undef NT_CASE_G
}
