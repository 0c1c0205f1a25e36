// gemm_nt4w_kernel: the 256x256 NT GEMM tile on four waves, with its row-major epilogue helpers.  gemm_nt.hip sends it the plain and the
// grouped launches whose spec has a build here; the rest stay on gemm_nt512_kernel.
#include "gemm_nt.h"

// ---------------------------------------------------------------------------------------------
// gemm_nt4w: a 256x256 output tile run by FOUR waves (one per SIMD, 512 registers each) that own 128x128 of it: 256
// accumulator registers, two fragment sets of 16 x 16 bytes.  A 128x128 wave tile reads 16 KB of LDS per 64 MFMAs where
// the 128x64 tile of the eight-wave gemm_nt512 reads 12 KB per 32: LDS traffic per k = 32 falls from 96 KB + 32 KB of
// DMA writes (the whole 128 B/clk the LDS has during the 1024 clk the MFMAs take) to 64 KB + 32 KB.
// Stages are k = 64: 512 rows (256 A + 256 B) of 128 bytes, XOR-swizzled as in gemm_nt256, two buffers of 64 KB.  Every
// DMA instruction moves whole 128-byte lines (8 lanes per row); the k = 32 sub-stages of gemm_nt512 fetch half lines,
// twice the L1 tag work per byte, and that was what each DMA cost the issuing wave (measured: without DMA 1575, with
// 1219 TFLOP/s on random data).
// With one wave per SIMD nothing else fills the matrix pipe, and a wave issues one instruction per four clocks - three
// besides the MFMA per 16-clk MFMA slot - so every wave interleaves by hand.  Iteration s (stage s in buffer s & 1,
// set X = its k-half 0 fragments on entry), 128 MFMAs:
//   MFMA   0.. 15 : 16 reads of k-half 1 -> set Y (one per MFMA)
//   MFMA  21      : lgkmcnt(0), barrier 1 - every wave has everything it needs from buffer s & 1
//   MFMA  23.. 98 : the 16 DMA pieces of stage s+2 -> buffer s & 1 (one per 5 MFMAs); then the scalar bookkeeping
//   MFMA 101      : counted vmcnt for stage s+1 (issued one iteration ago), barrier 2
//   MFMA 102..117 : 16 reads of stage s+1's k-half 0 -> set X;  lgkmcnt(0) after MFMA 125
// The epilogue of a tile's last stage follows MFMA 127 (its stores are counted into the next vmcnt wait).
// ---------------------------------------------------------------------------------------------
// gemm_nt4w epilogue for the builds that READ a tile - C = acc (+ bias) + residual, or C = acc x aux (the stored GELU') - on tiles
// inside the matrix.  nt_epilogue loads that operand in the accumulator layout (16 rows x 32 bytes per instruction) block by block,
// each block's loads BEHIND the previous block's stores: vmcnt returns in issue order and hipcc waits with vmcnt(0) once loads and stores
// are mixed, so every block paid a store acknowledgement plus a load latency (30k clocks per tile against 8k for the plain epilogue).
// Here the fp32 accumulators of 32 rows x 64 columns go through the wave's 8-KB LDS region (16-byte slots XOR-swizzled by row & 15,
// conflict-free both ways) and come back row-major; the operand is loaded in that shape too - whole 128-byte lines, 16 bytes per lane -
// by inline-asm loads one half block AHEAD (16 registers per set) and consumed behind a COUNTED wait that leaves the stores and the next
// set's loads in flight.  Same arithmetic in the same order as nt_epilogue (one rounding): bit-identical results.
template <bool MUL>
__device__ __forceinline__ void nt4w_rows_load(const GemmNTArgs& p, u32x4e_t (&r)[4], int h, int mb, int nb, int rl, int c8) {
  const bf16_t* src = MUL ? (const bf16_t*)p.aux : p.residual;
  const long long ld = MUL ? p.ldaux : p.ldr;
  const int tmh = (h & 3) * 2, tnq = (h >> 2) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16_t* a = src + (long long)(mb + tmh * 16 + i * 8 + rl) * ld + nb + tnq * 16 + c8 * 8;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r[i]) : "v"(a));
  }
}
// half block H (rows (H & 3) * 32 .., columns (H >> 2) * 64 .. of the wave tile): accumulators (+ bias) -> LDS -> row-major, operand set r
// behind a wait that leaves WAIT younger vector-memory operations in flight, combine, store.  No closure over acc: the accumulator array
// has to stay in registers through every inlined copy.
template <int SPEC, int H, int WAIT>
__device__ __forceinline__ void nt4w_rows_half(const GemmNTArgs& p, f32x4_t (&acc)[8][8], const float4 (&b4)[8], u32x4e_t (&r)[4], int mb,
                                               int nb, int frag_row, int pg, int rl, int c8, unsigned lx) {
  constexpr bool MUL = (SPEC & 7) == EPI_MUL_AUX;
  constexpr int tmh = (H & 3) * 2, tnq = (H >> 2) * 4;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int row_l = t * 16 + frag_row, slot = tn * 4 + pg;
      const unsigned a = lx + row_l * 256 + ((slot ^ (row_l & 15)) << 4);
      // acc + b in VGPRs ("v"): an accumulator register as a direct asm operand - "v" or "a" - makes the allocator copy and spill
      // accumulator tuples; without a bias b is an opaque zero
      const float4 b = b4[tnq + tn];
      const f32x4_t v = {acc[tmh + t][tnq + tn][0] + b.x, acc[tmh + t][tnq + tn][1] + b.y, acc[tmh + t][tnq + tn][2] + b.z, acc[tmh + t][tnq + tn][3] + b.w};
      asm volatile("ds_write_b128 %0, %1" :: "v"(a), "v"(v) : "memory");
    }
  f32x4_t lo[4], hi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row_l = i * 8 + rl;
    const unsigned a0 = lx + row_l * 256 + (((2 * c8) ^ (row_l & 15)) << 4), a1 = lx + row_l * 256 + (((2 * c8 + 1) ^ (row_l & 15)) << 4);
    asm volatile("ds_read_b128 %0, %1" : "=v"(lo[i]) : "v"(a0));
    asm volatile("ds_read_b128 %0, %1" : "=v"(hi[i]) : "v"(a1));
  }
  // the waits carry every register the loads and LDS reads write as in/out operands: no use (not even a copy) can be scheduled above them
#define NT4R_PINS "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]), "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3])
  constexpr bool OPERAND = MUL || ((SPEC & 16) != 0);       // else: nothing is read (bias + GELU + GELU')
  constexpr bool GELU = (SPEC & 7) == EPI_GELU_DAUX;
  // (with an operand every use of lo / hi is an operation with an r value, i.e. behind the wait already; pinning lo / hi there as well costs
  // the bias + residual build seven spilled registers)
  if constexpr (!OPERAND) asm volatile("s_waitcnt lgkmcnt(0)" : NT4R_PINS :: "memory");
  else if constexpr (WAIT == 8) asm volatile("s_waitcnt vmcnt(8)\n\ts_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) :: "memory");
  else asm volatile("s_waitcnt vmcnt(4)\n\ts_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) :: "memory");
#undef NT4R_PINS
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float f[8] = {lo[i][0], lo[i][1], lo[i][2], lo[i][3], hi[i][0], hi[i][1], hi[i][2], hi[i][3]};
    float o[8], dg[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (GELU) {
        f32x2_t g_, d_;
        gelu_and_grad2((f32x2_t){f[2 * k], f[2 * k + 1]}, g_, d_);
        o[2 * k] = g_[0]; o[2 * k + 1] = g_[1]; dg[2 * k] = d_[0]; dg[2 * k + 1] = d_[1];
      } else {
        const float z0 = __uint_as_float(r[i][k] << 16), z1 = __uint_as_float(r[i][k] & 0xffff0000u);
        o[2 * k] = MUL ? f[2 * k] * z0 : f[2 * k] + z0;
        o[2 * k + 1] = MUL ? f[2 * k + 1] * z1 : f[2 * k + 1] + z1;
      }
    }
    const u32x4e_t pk = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7])};
    __builtin_nontemporal_store(pk, (u32x4e_t*)((bf16_t*)p.C + (long long)(mb + tmh * 16 + i * 8 + rl) * p.ldc + nb + tnq * 16 + c8 * 8));
    if constexpr (GELU) {
      const u32x4e_t pd = {pack2bf(dg[0], dg[1]), pack2bf(dg[2], dg[3]), pack2bf(dg[4], dg[5]), pack2bf(dg[6], dg[7])};
      __builtin_nontemporal_store(pd, (u32x4e_t*)(p.aux + (long long)(mb + tmh * 16 + i * 8 + rl) * p.ldaux + nb + tnq * 16 + c8 * 8));
    }
  }
}
template <int SPEC>
__device__ __forceinline__ int nt4w_epilogue_rows(const GemmNTArgs& p, f32x4_t (&acc)[8][8], int mb, int nb, int frag_row, int frag_q,
                                                  unsigned lx) {
  constexpr bool MUL = (SPEC & 7) == EPI_MUL_AUX;
  // the LDS addresses below depend on the lane only: left to itself the compiler computes all of them once, outside the tile loop, and
  // carries ~40 registers through the k-loop (first build: 281 spilled registers).  An opaque copy of the lane id keeps them here.
  asm volatile("" : "+v"(frag_row), "+v"(frag_q));
  const int lane = frag_q * 16 + frag_row, rl = lane >> 3, c8 = lane & 7;
  const int pg = ((frag_q & 1) << 1) | (frag_q >> 1);
  float4 b4[8];
  float zero = 0.f;
  asm volatile("" : "+v"(zero));
#pragma unroll
  for (int tn = 0; tn < 8; ++tn) b4[tn] = (SPEC & 8) ? *(const float4*)(p.bias + nb + tn * 16 + pg * 4) : make_float4(zero, zero, zero, zero);
  u32x4e_t ra[4], rb[4];
  constexpr bool OPERAND = MUL || ((SPEC & 16) != 0);
#define NT4R_LOAD(R, H) do { if constexpr (OPERAND) nt4w_rows_load<MUL>(p, R, H, mb, nb, rl, c8); } while (0)
#define NT4R_HALF(R, H, W) nt4w_rows_half<SPEC, H, W>(p, acc, b4, R, mb, nb, frag_row, pg, rl, c8, lx)
  NT4R_LOAD(ra, 0);
  NT4R_LOAD(rb, 1); NT4R_HALF(ra, 0, 4);
  NT4R_LOAD(ra, 2); NT4R_HALF(rb, 1, 8);
  NT4R_LOAD(rb, 3); NT4R_HALF(ra, 2, 8);
  NT4R_LOAD(ra, 4); NT4R_HALF(rb, 3, 8);
  NT4R_LOAD(rb, 5); NT4R_HALF(ra, 4, 8);
  NT4R_LOAD(ra, 6); NT4R_HALF(rb, 5, 8);
  NT4R_LOAD(rb, 7); NT4R_HALF(ra, 6, 8);
  NT4R_HALF(rb, 7, 4);
#undef NT4R_LOAD
#undef NT4R_HALF
  return ((SPEC & 7) == EPI_GELU_DAUX) ? 64 : 32;
}

#define DS_READ128(dst, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm))
#define STAGE4 (512 * 128)
#ifndef NT4_DSTEP
#define NT4_DSTEP 5      // MFMAs per DMA piece (2: -4 %, 3: -2 % against 5; the TA path wants them spread out)
#endif
#ifndef NT4_RS
#define NT4_RS 1         // MFMAs per fragment read in the first phase
#endif
#define NT4_B1 (16 * NT4_RS + 5)    // MFMA after which barrier 1 sits
#ifndef NT4_B2
#define NT4_B2 101                  // MFMA after which the vmcnt wait + barrier 2 sit
#endif
#ifndef NT4_RS3
#define NT4_RS3 1                   // MFMAs per fragment read in the last phase
#endif
static_assert(NT4_B1 + 2 + 15 * NT4_DSTEP + 2 < NT4_B2, "the DMA pieces must be out before the vmcnt wait");
static_assert(NT4_B2 + 16 * NT4_RS3 < 125, "the last fragment reads need time to land");
__device__ __forceinline__ void wait_vmcnt_4w(int n) {
  if (n == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if (n >= 63) asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
  else if (n >= 48) asm volatile("s_waitcnt vmcnt(48)" ::: "memory");
  else if (n >= 32) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
  else if (n >= 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
  else if (n >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// GROUPED: tiles come from the device-side table p.tiles (group, m0, m_end, -) of 256-row tiles, B / bias are per group,
// A rows are gathered through p.a_rowmap and C rows scattered through p.c_rowmap (expert GEMMs, dGm) - as in gemm_nt512.
template <int SPEC, bool GROUPED = false>
__global__ __launch_bounds__(256) void gemm_nt4w_kernel(GemmNTArgs p_in) {
  GemmNTArgs p = p_in;
  if (!GROUPED && p.m_dev) { p.M = min(*p.m_dev, p.M); p.max_tiles_m = (p.M + 255) / 256; }
#ifdef NT4_SKIP
  constexpr int dbg4 = NT4_SKIP;      // compile-time ablation (tools/nt_timing.hip -DNT_EXPERIMENT -DNT4_SKIP=bits): 1 reads, 8 DMA, 16 barriers
#else
  constexpr int dbg4 = 0;
#endif
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
  // the plain builds with bf16 output store through a wave-private 8-KB LDS region behind the ring (nt_epilogue LDSX)
#ifdef NT4_NO_XLDS
  constexpr bool XLDS = false;            // A/B builds (tools): the accumulator-layout stores
#else
  constexpr bool XLDS = !GROUPED && SPEC >= 0 && !(SPEC & 64);
#endif
  // builds whose epilogue READS a tile (residual add, x stored GELU') or writes two (GELU + GELU'): nt4w_epilogue_rows on tiles inside the
  // matrix; the next tile's first fragments are then read AFTER the epilogue, which needs their 64 registers
  constexpr bool OPER = XLDS && (((SPEC & 16) != 0 && (SPEC & 7) == EPI_NONE) || (SPEC & 7) == EPI_MUL_AUX || ((SPEC & 7) == EPI_GELU_DAUX && (SPEC & 32) != 0));
  __shared__ __attribute__((aligned(128))) char smem[2 * STAGE4 + (XLDS ? 32768 : 0)];      // 128: the k-half switch is an XOR of the byte address
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: LDS-DMA bases stay scalar
  const int wm = wid & 1, wn = wid >> 1;
  const int frag_row = lane & 15, frag_q = lane >> 4;
  const int G = gridDim.x;
  const int my = xcd_remap(blockIdx.x, G);
  const int total = GROUPED ? *p.tile_count * p.n_tiles_n : p.max_tiles_m * p.n_tiles_n;
  const int nk = p.K / 64;                        // stages per tile
  constexpr int SM = 4, SN = 8;
  struct Tile { int m0, n0, m_end, group; };
  auto decode = [&](int id) -> Tile {             // tile order of gemm_nt512 (row tiles last to first)
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
    t.m0 = (p.max_tiles_m - 1 - tile_m) * 256; t.n0 = tile_n * 256;
    return t;
  };
  // DMA piece i (0..15) moves 32 rows: thread t fills LDS slot q = i * 256 + t (16 bytes) = row q >> 3, position q & 7,
  // which holds the row's 16-byte chunk (q & 7) ^ (row & 7).  Per-lane sources are 32-bit byte offsets from the tile's
  // A / B base (one tile's rows span 256 * ld * 2 bytes < 4 GB, checked on the host).
  unsigned src[16];
  const char* baseA = (const char*)p.A;
  const char* baseB = (const char*)p.B;
  const unsigned r0 = tid >> 3, c16 = ((tid & 7) ^ (r0 & 7)) * 16;   // i * 32 leaves row & 7 alone: one chunk index for all pieces
  auto setup = [&](const Tile& t) {
    const bool gather = GROUPED && p.a_rowmap;                                 // gathered rows: offsets from A itself (whole A < 4 GB, host check)
    baseA = (const char*)(p.A + (gather ? 0ll : (long long)t.m0 * p.lda));
    baseB = (const char*)(p.B + (GROUPED ? (long long)t.group * p.strideB : 0ll) + (long long)t.n0 * p.ldb);
    const unsigned limA = t.m_end - 1 - t.m0, limB = p.N - 1 - t.n0;          // last valid row of the tile (rows past it re-read it)
    const unsigned ldaB = p.lda * 2, ldbB = p.ldb * 2;                         // < 2^24 (host check): 24-bit multiplies
    unsigned r0v = r0;
    if constexpr (OPER) asm volatile("" : "+v"(r0v));      // i * 32 + r0 recomputed here: hoisted out of the tile loop they were spilled
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned ra = min(i * 32 + r0v, limA);
      if (gather) src[i] = (unsigned)p.a_rowmap[t.m0 + ra] * ldaB + c16;
      else src[i] = __umul24(ra, ldaB) + c16;
      src[8 + i] = __umul24(min(i * 32 + r0v, limB), ldbB) + c16;
    }
  };
  f32x4_t acc[8][8];
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  };
  const int sig = ((((frag_row >> 2) & 1) << 1 | (frag_row >> 3)) << 2) | (frag_row & 3);   // sigma(frag_row), see nt_epilogue
  const unsigned lds0 = (unsigned)(size_t)smem;   // LDS byte address of buffer 0
  // fragment addresses in buffer 0 for k-half 0; k-half 1 is the same address ^ 64, buffer 1 is + STAGE4
  const unsigned offA = lds0 + (wm * 128 + frag_row) * 128 + ((frag_q ^ (frag_row & 7)) << 4);
  const unsigned offB = lds0 + (256 + wn * 128 + sig) * 128 + ((frag_q ^ (sig & 7)) << 4);

  if (my >= total) return;
  const int my_tiles = (total - my + G - 1) / G;
  Tile ct = decode(my);
  setup(ct);
  // the tile / k position the DMA is at (two stages ahead of the MFMAs); past the last tile the addresses stay where
  // they are (valid memory, the data is never used).  gA / gB / ldsW: scalar bases of the stage being issued, advanced
  // in an idle stretch of the iteration, never next to a DMA.
  int lid = my, lk = 0, wb = 0;
  const char* gA = baseA;
  const char* gB = baseB;
  unsigned ldsW = lds0 + wid * 1024;
  auto advance = [&]() __attribute__((always_inline)) {
    wb ^= 1;
    if (++lk == nk) {
      lk = 0; lid += G;
      if (lid < total) { const Tile lt = decode(lid); setup(lt); }
    }
    gA = baseA + lk * 128; gB = baseB + lk * 128;
    ldsW = lds0 + wb * STAGE4 + wid * 1024;
  };
  auto piece = [&](int i) __attribute__((always_inline)) {
    __builtin_amdgcn_global_load_lds(GLB_PTR((i < 8 ? gA : gB) + src[i]), (__attribute__((address_space(3))) void*)(size_t)(ldsW + i * 4096), 16, 0, 0);
  };
  int s_prev = 0;                                 // C / aux stores issued by the previous iteration's epilogue
  NT_T(long long t_wait = 0, t_bar = 0, t_comp = 0, t_epi = 0; const long long t_begin = nt_clk();)
  int rbuf = 0;                                   // buffer of the stage being computed
  bf16x8_t fa0[8], fb0[8], fa1[8], fb1[8];
  auto iteration = [&](bool last) __attribute__((always_inline)) {
    const unsigned aA1 = (offA + rbuf * STAGE4) ^ 64u, aB1 = (offB + rbuf * STAGE4) ^ 64u;          // this stage, k-half 1
    const unsigned aA0 = offA + (rbuf ^ 1) * STAGE4, aB0 = offB + (rbuf ^ 1) * STAGE4;              // next stage, k-half 0
    auto one = [&](auto qc) __attribute__((always_inline)) {
      constexpr int q = decltype(qc)::value, h = q >> 6, tm = (q >> 3) & 7, tn = q & 7;
      if constexpr (h == 0) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb0[tn], fa0[tm], acc[tm][tn], 0, 0, 0);
      else acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb1[tn], fa1[tm], acc[tm][tn], 0, 0, 0);
      if constexpr (q < 16 * NT4_RS && (q % NT4_RS) == NT4_RS - 1) {   // k-half 1 of this stage -> set Y
        constexpr int g = q / NT4_RS;
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!(dbg4 & 1)) { if constexpr (g < 8) DS_READ128(fa1[g], aA1, g * 2048); else DS_READ128(fb1[g - 8], aB1, (g - 8) * 2048); }
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (q == NT4_B1) {
        NT_T(const long long c0 = nt_clk();)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (!(dbg4 & 16)) __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
        NT_T(t_bar += nt_clk() - c0;)
      }
      if constexpr (q >= NT4_B1 + 2 && q < NT4_B1 + 2 + 16 * NT4_DSTEP && (q - NT4_B1 - 2) % NT4_DSTEP == 0) {      // stage s+2 -> the buffer just released
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!(dbg4 & 8)) piece((q - NT4_B1 - 2) / NT4_DSTEP);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (q == NT4_B1 + 2 + 15 * NT4_DSTEP + 2) advance();
      if constexpr (q == NT4_B2) {
        NT_T(const long long c0 = nt_clk();)
        __builtin_amdgcn_sched_barrier(0);
        wait_vmcnt_4w(__builtin_amdgcn_readfirstlane(s_prev + 16));
        NT_T(const long long c1 = nt_clk(); t_wait += c1 - c0;)
        if constexpr (!(dbg4 & 16)) __builtin_amdgcn_s_barrier();
        NT_T(t_bar += nt_clk() - c1;)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
      }
      if constexpr (q > NT4_B2 && q <= NT4_B2 + 16 * NT4_RS3 && ((q - NT4_B2 - 1) % NT4_RS3) == 0) {        // next stage's k-half 0 -> set X (its MFMAs are done)
        constexpr int g = (q - NT4_B2 - 1) / NT4_RS3;
        __builtin_amdgcn_sched_barrier(0);
        if (!(OPER && last)) {
          if constexpr (!(dbg4 & 1)) { if constexpr (g < 8) DS_READ128(fa0[g], aA0, g * 2048); else DS_READ128(fb0[g - 8], aB0, (g - 8) * 2048); }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (q == 125) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    NT_T(const long long i0 = nt_clk();)
    static_for<128>(one);
    NT_T(t_comp += nt_clk() - i0;)
    rbuf ^= 1;
    s_prev = 0;
    if (last) {
      int n = 0;
      NT_T(const long long e0 = nt_clk();)
      if constexpr (!(dbg4 & 4)) {
      const unsigned lx = lds0 + 2 * STAGE4 + wid * 8192;
      if (OPER && ct.m0 + 256 <= ct.m_end && ct.n0 + 256 <= p.N) {
        if constexpr (OPER) n += nt4w_epilogue_rows<SPEC>(p, acc, ct.m0 + wm * 128, ct.n0 + wn * 128, frag_row, frag_q, lx);
      } else {
      n += nt_epilogue<false, 0, 8, 0, 8, XLDS>(p, acc, ct.m0 + wm * 128, ct.m_end, ct.n0 + wn * 128, ct.group, frag_row, frag_q, nullptr, lx);
      n += nt_epilogue<false, 0, 8, 4, 8, XLDS>(p, acc, ct.m0 + wm * 128, ct.m_end, ct.n0 + wn * 128 + 64, ct.group, frag_row, frag_q, nullptr, lx);
      n += nt_epilogue<false, 4, 8, 0, 8, XLDS>(p, acc, ct.m0 + wm * 128 + 64, ct.m_end, ct.n0 + wn * 128, ct.group, frag_row, frag_q, nullptr, lx);
      n += nt_epilogue<false, 4, 8, 4, 8, XLDS>(p, acc, ct.m0 + wm * 128 + 64, ct.m_end, ct.n0 + wn * 128 + 64, ct.group, frag_row, frag_q, nullptr, lx);
      }
      }
      s_prev = __builtin_amdgcn_readfirstlane(n);
      zero_acc();
      if constexpr (OPER) {                        // the fragment reads this iteration skipped (rbuf already points at the next stage)
        const unsigned nA0 = offA + rbuf * STAGE4, nB0 = offB + rbuf * STAGE4;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 8; ++t) DS_READ128(fa0[t], nA0, t * 2048);
#pragma unroll
        for (int t = 0; t < 8; ++t) DS_READ128(fb0[t], nB0, t * 2048);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
      NT_T(t_epi += nt_clk() - e0;)
    }
  };

  zero_acc();
  for (int v = 0; v < 2; ++v) {                   // stages 0 and 1 (the host guarantees K >= 128)
#pragma unroll
    for (int i = 0; i < 16; ++i) piece(i);
    advance();
  }
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  __builtin_amdgcn_s_barrier();                   // stage 0 landed for every wave
  asm volatile("" ::: "memory");
#pragma unroll
  for (int t = 0; t < 8; ++t) DS_READ128(fa0[t], offA, t * 2048);
#pragma unroll
  for (int t = 0; t < 8; ++t) DS_READ128(fb0[t], offB, t * 2048);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  for (int ti = 0; ti < my_tiles; ++ti) {
    for (int k = 1; k < nk; ++k) iteration(false);
    iteration(true);
    if (ti + 1 < my_tiles) ct = decode(my + (ti + 1) * G);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA ran two stages past the end
  NT_T(if (lane == 0) { unsigned long long* g = g_nt_timing + wid * 8; atomicAdd(&g[0], (unsigned long long)(nt_clk() - t_begin));
         atomicAdd(&g[1], (unsigned long long)t_wait); atomicAdd(&g[2], (unsigned long long)t_bar); atomicAdd(&g[4], (unsigned long long)t_comp);
         atomicAdd(&g[5], (unsigned long long)t_epi); atomicAdd(&g[6], 1ull); })
}

bool nt4w_launch(const GemmNTArgs& p, int spec, bool grouped, int grid, hipStream_t stream) {
#define NT_CASE(s) case s: hipLaunchKernelGGL((gemm_nt4w_kernel<s, false>), dim3(grid), dim3(256), 0, stream, p); return true;
#define NT_CASE_G(s) case s: hipLaunchKernelGGL((gemm_nt4w_kernel<s, true>), dim3(grid), dim3(256), 0, stream, p); return true;
  if (!grouped) switch (spec) { NT_PLAIN_SPECS(NT_CASE) default: return false; }
  switch (spec) {
    NT_CASE_G(NT_SPEC(EPI_NONE, 0, 0, 0))
    NT_CASE_G(NT_SPEC(EPI_RELU, 1, 0, 0))
    NT_CASE_G(NT_SPEC(EPI_MUL_DRELU, 0, 1, 1))
    NT_CASE_G(NT_SPEC(EPI_NONE, 0, 1, 0))          // pyramid experts: dG += dH1 . W0 (the ReLU' follows the interpolation, swin.py:41-42)
  }
  return false;
#undef NT_CASE
#undef NT_CASE_G
}
