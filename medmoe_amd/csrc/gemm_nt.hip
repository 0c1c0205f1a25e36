// bf16 MFMA NT GEMM for gfx950 (MI355X): the host entry points, the choice of the kernel, and the two 128-row kernels.
//   gemm_nt : C[M,N]  = epi(alpha * A[M,K] . B[N,K]^T)        (forward + dgrad; weights are
//             stored [out,in] = the reference's nn.Linear layout, multi_head_attention.py:35-36,
//             mlp.py:55-64, swin.py:18-30,88-92)
// gemm_nt_kernel: 128x128 block tile, 4 waves (2x2, 64x64 each), K-step 64, operands staged HBM->LDS with
// global_load_lds_dwordx4 (16 B/lane, lane-linear LDS image, XOR swizzle applied on the SOURCE
// address and again on the LDS read), double-buffered, fp32 accumulation in MFMA:
// v_mfma_f32_16x16x32_bf16 with the operands swapped so a lane owns 4 consecutive
// output columns (8-byte bf16 stores).
#include "gemm_nt.h"
#include "options.h"

// Persistent over output tiles: a block walks tiles  t = round*grid + xcd_remap(block)  and runs ONE
// continuous double-buffered pipeline over (tile, k-step); the first k-tile of the next output tile is
// already in flight while the current tile's epilogue stores run, so the per-tile prologue/epilogue
// (~1/3 of a K=768 tile's lifetime) hides behind LDS-DMA traffic.
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(GemmNTArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 32768];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int frag_row = lane & 15, frag_q = lane >> 4, swz = lane & 7;
  const int G = gridDim.x;
  const int my = xcd_remap(blockIdx.x, G);
  if (!p.tiles && p.m_dev) { p.M = min(*p.m_dev, p.M); p.max_tiles_m = (p.M + BM - 1) / BM; }
  const int n_tiles_m = p.tiles ? min(*p.tile_count, p.max_tiles_m) : p.max_tiles_m;
  const int total = n_tiles_m * p.n_tiles_n;
  // K % 64 == 32 (Swin-T stage 1: 96 and 288 channels): the last k-step is half a stage - lanes that would fetch its upper four
  // 16-byte chunks re-fetch the lower four (valid memory, never multiplied) and the step runs one MFMA k-half instead of two
  const int nt = (p.K + BK - 1) / BK;
  const bool khalf = (p.K & 32) != 0;
  const int tail_adj = (khalf && (((lane & 7) ^ ((lane >> 3) & 7)) >= 4)) ? -32 : 0;

  struct Tile { int group, m0, m_end, n0; };
  auto decode = [&](int id) -> Tile {
    Tile t;
    const int tile_m = id / p.n_tiles_n, tile_n = id - tile_m * p.n_tiles_n;
    if (p.tiles) { const int4 q = p.tiles[tile_m]; t.group = q.x; t.m0 = q.y; t.m_end = q.z; }
    else { t.group = 0; t.m0 = tile_m * BM; t.m_end = p.M; }
    t.n0 = tile_n * BN;
    return t;
  };
  const bf16_t* asrc[4];
  const bf16_t* bsrc[4];
  auto setup = [&](const Tile& t) {
    const bf16_t* Bg = p.B + (long long)t.group * p.strideB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = i * 32 + wid * 8 + (lane >> 3);
      const int c = (lane & 7) ^ (row & 7);
      int ra = min(t.m0 + row, t.m_end - 1);
      if (p.a_rowmap) ra = p.a_rowmap[ra];
      asrc[i] = p.A + (long long)ra * p.lda + c * 8;
      const int rb = min(t.n0 + row, p.N - 1);
      bsrc[i] = Bg + (long long)rb * p.ldb + c * 8;
    }
  };
  auto stage = [&](int buf, int ks) {
    char* sA = smem + buf * 32768 + wid * 1024;
    char* sB = sA + 16384;
    const int k0 = ks * BK + ((ks == nt - 1) ? tail_adj : 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_global_load_lds(GLB_PTR(asrc[i] + k0), LDS_PTR(sA + i * 4096), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(GLB_PTR(bsrc[i] + k0), LDS_PTR(sB + i * 4096), 16, 0, 0);
    }
  };

  f32x4_t acc[4][4];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  };
  // B-matrix fragment rows go through sigma(i) = 4*perm(i>>2) + (i&3), perm = {0,2,1,3}: see nt_epilogue
  const int sig = ((((frag_row >> 2) & 1) << 1 | (frag_row >> 3)) << 2) | (frag_row & 3);
  auto compute = [&](int buf, int nks) {
    const char* sA = smem + buf * 32768 + (wm * 64 + frag_row) * 128;
    const char* sB = smem + buf * 32768 + 16384 + (wn * 64 + sig) * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks >= nks) break;
      const int coff = ((ks * 4 + frag_q) ^ swz) * 16;
      const int coffb = ((ks * 4 + frag_q) ^ (sig & 7)) * 16;
      bf16x8_t af[4], bf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        af[t] = *(const bf16x8_t*)(sA + t * 2048 + coff);
        bf[t] = *(const bf16x8_t*)(sB + t * 2048 + coffb);
      }
#pragma unroll
      for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[tn], af[tm], acc[tm][tn], 0, 0, 0);
    }
  };
  auto epilogue = [&](const Tile& t) -> int { return nt_epilogue<false>(p, acc, t.m0 + wm * 64, t.m_end, t.n0 + wn * 64, t.group, frag_row, frag_q, nullptr); };

  int id = my;
  if (id >= total) return;
  Tile cur_t = decode(id);
  setup(cur_t);
  zero_acc();
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int cur = 0;
  while (true) {
    const int nid = id + G;
    const bool has_next = nid < total;
    Tile next_t = cur_t;
    for (int ks = 0; ks < nt; ++ks) {
      if (ks + 1 < nt) {
        stage(cur ^ 1, ks + 1);
      } else if (has_next) {            // nothing is in flight here: row-map loads cost no DMA drain
        next_t = decode(nid);
        setup(next_t);
        stage(cur ^ 1, 0);
      }
      compute(cur, (khalf && ks == nt - 1) ? 1 : 2);
      if (ks == nt - 1) { epilogue(cur_t); zero_acc(); }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      cur ^= 1;
    }
    if (!has_next) break;
    id = nid; cur_t = next_t;
  }
}

// ---------------------------------------------------------------------------------------------
// gemm_nt_direct: short contractions that are not a multiple of the 64-wide k-step of the DMA kernels (K % 64 == 32, K <= 288: the 96 and
// 288 channels of Swin-T's first stage over 100 k token rows).  Such a product is a stream of A and C rows around a weight matrix of a few
// tens of KB: nothing to stage.  A wave owns a 64 x 64 block of C and takes BOTH operands' fragments straight from global memory (the
// weights stay in L2 / the vector L1; the six column blocks of one 64-row A panel are consecutive waves), runs K / 32 steps of 16 MFMAs with
// the next step's fragments in flight, and leaves through nt_epilogue - no LDS, no barrier, no tile pipeline to fill and drain every two
// k-steps (the 128 x 128 DMA kernel spent its time there: 1.75 TB/s at [100352, 384] x K = 96).
// ---------------------------------------------------------------------------------------------
template <int SPEC>
__global__ __launch_bounds__(256) void gemm_nt_direct_kernel(GemmNTArgs p_in) {
  GemmNTArgs p = p_in;
  if constexpr (SPEC >= 0) {          // as gemm_nt256_kernel: the epilogue flags are compile-time constants, only that path is emitted
    p.epi = SPEC & 7; p.out_f32 = 0; p.col_perm = 0; p.c_rowmap = nullptr; p.a_rowmap = nullptr; p.alpha = 1.f;
    if (!(SPEC & 8)) p.bias = nullptr;
    if (!(SPEC & 16)) p.residual = nullptr;
    if (!(SPEC & 32)) p.aux = nullptr;
    __builtin_assume((p.N & 7) == 0);
    if (SPEC & 8) __builtin_assume(p.bias != nullptr);
    if (SPEC & 16) __builtin_assume(p.residual != nullptr);
    if (SPEC & 32) __builtin_assume(p.aux != nullptr);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int frag_row = lane & 15, frag_q = lane >> 4;
  const int nblk_n = (p.N + 63) >> 6, nblk_m = (p.M + 63) >> 6;
  const long long w = (long long)blockIdx.x * 4 + wid;
  if (w >= (long long)nblk_m * nblk_n) return;                      // whole waves leave: no barrier anywhere in this kernel
  const int mb = (int)(w / nblk_n), nb = (int)(w - (long long)mb * nblk_n);
  const int m0 = mb * 64, n0 = nb * 64;
  const int sig = ((((frag_row >> 2) & 1) << 1 | (frag_row >> 3)) << 2) | (frag_row & 3);   // sigma(frag_row), see nt_epilogue
  const bf16_t* ar[4];
  const bf16_t* br[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    ar[t] = p.A + (long long)min(m0 + t * 16 + frag_row, p.M - 1) * p.lda + frag_q * 8;
    br[t] = p.B + (long long)min(n0 + t * 16 + sig, p.N - 1) * p.ldb + frag_q * 8;
  }
  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int nks = p.K >> 5;
  bf16x8_t af[4], bf[4], an[4], bn[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) { af[t] = *(const bf16x8_t*)ar[t]; bf[t] = *(const bf16x8_t*)br[t]; }
  for (int ks = 0; ks < nks; ++ks) {
    if (ks + 1 < nks) {
#pragma unroll
      for (int t = 0; t < 4; ++t) { an[t] = *(const bf16x8_t*)(ar[t] + (ks + 1) * 32); bn[t] = *(const bf16x8_t*)(br[t] + (ks + 1) * 32); }
    }
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[tn], af[tm], acc[tm][tn], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) { af[t] = an[t]; bf[t] = bn[t]; }
  }
  nt_epilogue<false>(p, acc, m0, p.M, n0, 0, frag_row, frag_q, nullptr);
}

static void nt_direct_launch(const GemmNTArgs& p, int spec, hipStream_t stream) {
  const long long waves = (long long)((p.M + 63) / 64) * ((p.N + 63) / 64);
  const dim3 dgrid((unsigned)((waves + 3) / 4));
  switch (spec) {
#define NT_CASE(s) case s: hipLaunchKernelGGL(gemm_nt_direct_kernel<s>, dgrid, dim3(256), 0, stream, p); break;
    NT_CASE(NT_SPEC(EPI_NONE, 0, 0, 0))          // dgrads
    NT_CASE(NT_SPEC(EPI_NONE, 1, 0, 0))          // QKV, o_proj under stochastic depth
    NT_CASE(NT_SPEC(EPI_NONE, 1, 1, 0))          // o_proj / FC2 + residual
    NT_CASE(NT_SPEC(EPI_GELU_DAUX, 1, 0, 1))     // FC1 forward, keeps GELU'(z)
    NT_CASE(NT_SPEC(EPI_MUL_AUX, 0, 0, 1))       // FC2 dgrad x stored GELU'
#undef NT_CASE
    default: hipLaunchKernelGGL(gemm_nt_direct_kernel<-1>, dgrid, dim3(256), 0, stream, p); break;
  }
}

int g_use_nt256 = 1, g_use_nt512 = 1, g_use_nt4w = 1, g_use_nt_direct = 1, g_nt_max_grid = 256;      // options.h, keys 1, 2, 7, 17 and 5

// Which kernel the most recent medmoe_gemm_nt / _rows / _tiles256 call of this process launched: 0 gemm_nt_kernel (128x128), 1 gemm_nt256_kernel,
// 2 gemm_nt512_kernel, 3 gemm_nt512_kernel GROUPED, 4 gemm_nt4w_kernel, 5 gemm_nt4w_kernel GROUPED, 6 gemm_nt_direct_kernel.  Measurement and
// test aid only (bench.py labels its per-launch HIP-event timings with it, tests/test_gemm_nt_exact_gpu.py asserts the kernel each of its
// cases was written for); nothing in the product path reads it.
static int g_last_nt_kernel = -1;
extern "C" int medmoe_last_gemm_nt_kernel() { return g_last_nt_kernel; }

// Every entry point below: validate, nt_args, choose the kernel and its tiling (n_tiles_n, max_tiles_m), call the family's launch
// function, record the kernel, return mm_check_launch().  nt_args fills every field of GemmNTArgs: the tiling as 0 and m_dev as null, for the entry point to set.
static GemmNTArgs nt_args(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const float* bias,
                          const void* residual, int ldr, void* aux, int ldaux, const int* a_rowmap, const int* c_rowmap, const int* tiles,
                          const int* tile_count, long long strideB, long long strideBias, float alpha, int epi, int out_f32, int col_perm) {
  GemmNTArgs p;
  p.A = (const bf16_t*)A; p.B = (const bf16_t*)B; p.C = C;
  p.bias = bias; p.residual = (const bf16_t*)residual; p.aux = (bf16_t*)aux;
  p.a_rowmap = a_rowmap; p.c_rowmap = c_rowmap; p.tiles = (const int4*)tiles; p.tile_count = tile_count;
  p.strideB = strideB; p.strideBias = strideBias;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ldr = ldr; p.ldaux = ldaux;
  p.n_tiles_n = 0; p.max_tiles_m = 0;
  p.alpha = alpha; p.epi = epi; p.out_f32 = out_f32; p.col_perm = col_perm; p.m_dev = nullptr;
  return p;
}

// The specialised build of a launch (NT_SPEC, | 64 for an fp32 C), or -1 where only the generic build applies: N % 8, alpha != 1, an fp32 C in a
// family without fp32 builds.  A spec that a family's list does not hold takes the generic build too: the ReLU forms have builds only when grouped.
static int nt_spec(const GemmNTArgs& p, bool f32_builds) {
  if ((p.N & 7) != 0 || p.alpha != 1.f || (p.out_f32 && !f32_builds)) return -1;
  return NT_SPEC(p.epi, p.bias ? 1 : 0, p.residual ? 1 : 0, p.aux ? 1 : 0) | (p.out_f32 ? 64 : 0);
}

static int gemm_nt_impl(const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                        int M, int N, int K, const float* bias, const void* residual, int ldr,
                        void* aux, int ldaux, const int* a_rowmap, const int* c_rowmap,
                        const int* tiles, const int* tile_count, int max_tiles,
                        long long strideB, long long strideBias, float alpha, int epi,
                        int out_f32, int col_perm, const int* m_dev, hipStream_t stream) {
  if (!A || !B || !C) return MM_ERR_ARG;
  if (M <= 0 || N <= 0 || K <= 0 || (K % 32) != 0 || (N % 4) != 0) return MM_ERR_SHAPE;      // K % 64 == 32: the 128x128 kernel only
  if ((lda % 8) || (ldb % 8) || (ldc % 4) || (residual && (ldr % 4)) || (aux && (ldaux % 4))) return MM_ERR_SHAPE;
  if (epi < 0 || epi > EPI_MUL_AUX) return MM_ERR_ARG;
  if ((epi == EPI_MUL_DGELU || epi == EPI_MUL_DRELU || epi == EPI_MUL_AUX) && !aux) return MM_ERR_ARG;
  if (tiles && (!tile_count || max_tiles <= 0)) return MM_ERR_ARG;
  GemmNTArgs p = nt_args(A, lda, B, ldb, C, ldc, M, N, K, bias, residual, ldr, aux, ldaux, a_rowmap, c_rowmap, tiles, tile_count, strideB,
                         strideBias, alpha, epi, out_f32, col_perm);
  p.m_dev = m_dev; p.n_tiles_n = (N + BN - 1) / BN;
  const bool fits32 = (long long)M * lda * 2 < (1ll << 32) && (long long)N * ldb * 2 < (1ll << 32);   // 32-bit DMA offsets
  const bool plain = !tiles && !a_rowmap && !c_rowmap && !col_perm && M >= 4 * BM2 && g_use_nt256 && (K % BK) == 0;
  const bool big = plain && K >= 3 * BK && fits32;
  // 256x256 tiles: wide N always; N of two or three tiles when K is long enough to amortise the seam or the tile
  // count fills the chip evenly (measured: N=768 K=3072 858 -> ~1150 TF/s; N=768 K=768 slower at 591 tiles).  Offsets are
  // tile-relative there, so only one tile's rows (256 * ld * 2 bytes) have to fit 32 bits.
  const bool tile32 = 256ll * lda * 2 < (1ll << 32) && 256ll * ldb * 2 < (1ll << 32);
  const bool pitch24 = 2ll * lda < (1ll << 24) && 2ll * ldb < (1ll << 24);        // gemm_nt4w multiplies row x pitch in 24 bits
  // 256x256 or 256x128 tiles: the big tile (gemm_nt4w) runs ~1.35x faster per flop, the small one wastes less of
  // the last round of 256 workgroups.  Compare fill x speed.
  const long long t512 = (long long)((M + 255) / 256) * ((N + 255) / 256), t256 = (long long)((M + 255) / 256) * ((N + 127) / 128);
  const double fill512 = (double)t512 / (double)(((t512 + 255) / 256) * 256), fill256 = (double)t256 / (double)(((t256 + 255) / 256) * 256);
  if (plain && tile32 && g_use_nt512 && K >= 128 && N >= 512 && (!big || fill512 * 1.35 >= fill256)) {
    p.max_tiles_m = (M + 255) / 256;
    p.n_tiles_n = (N + 255) / 256;
    const int grid = min(p.max_tiles_m * p.n_tiles_n, g_nt_max_grid);     // 1 resident block per CU (128 KB LDS)
    const int spec = nt_spec(p, true);
    // four waves, 128x128 wave tiles (see gemm_nt4w_kernel): the same tiles, 5-15 % faster
    if (g_use_nt4w && spec >= 0 && pitch24 && nt4w_launch(p, spec, false, grid, stream)) g_last_nt_kernel = 4;
    else { nt512_launch(p, spec, false, grid, stream); g_last_nt_kernel = 2; }
    return mm_check_launch();
  }
  if (big) {
    p.max_tiles_m = (M + BM2 - 1) / BM2;
    const int grid = min(p.max_tiles_m * p.n_tiles_n, 256);     // 1 resident block per CU (144 KB LDS)
    nt256_launch(p, nt_spec(p, true), grid, stream);
    g_last_nt_kernel = 1;
    return mm_check_launch();
  }
  if (g_use_nt_direct && !tiles && !a_rowmap && !c_rowmap && !col_perm && !m_dev && (K & 63) == 32 && K <= 288 && M >= 4096) {
    nt_direct_launch(p, nt_spec(p, false), stream);
    g_last_nt_kernel = 6;
    return mm_check_launch();
  }
  p.max_tiles_m = tiles ? max_tiles : (M + BM - 1) / BM;
  const int grid = min(p.max_tiles_m * p.n_tiles_n, 2 * 256);   // 2 resident blocks per CU (64 KB LDS each)
  hipLaunchKernelGGL(gemm_nt_kernel, dim3(grid), dim3(256), 0, stream, p);
  g_last_nt_kernel = 0;
  return mm_check_launch();
}

extern "C" int medmoe_gemm_nt(const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                              int M, int N, int K, const float* bias, const void* residual, int ldr,
                              void* aux, int ldaux, const int* a_rowmap, const int* c_rowmap,
                              const int* tiles, const int* tile_count, int max_tiles,
                              long long strideB, long long strideBias, float alpha, int epi,
                              int out_f32, int col_perm, hipStream_t stream) {
  return gemm_nt_impl(A, lda, B, ldb, C, ldc, M, N, K, bias, residual, ldr, aux, ldaux, a_rowmap, c_rowmap, tiles, tile_count, max_tiles,
                      strideB, strideBias, alpha, epi, out_f32, col_perm, nullptr, stream);
}

// The same product on the first *m_dev rows only (m_dev: device int, 1 <= *m_dev <= M; M sizes the launch): the packed rows of a
// variable-length batch (the text tower's non-padding tokens) without a device-to-host copy of the count.  Plain operands only.
extern "C" int medmoe_gemm_nt_rows(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const float* bias,
                                   const void* residual, int ldr, void* aux, int ldaux, float alpha, int epi, int out_f32, const int* m_dev,
                                   hipStream_t stream) {
  if (!m_dev) return MM_ERR_ARG;
  return gemm_nt_impl(A, lda, B, ldb, C, ldc, M, N, K, bias, residual, ldr, aux, ldaux, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, alpha, epi,
                      out_f32, 0, m_dev, stream);
}

// Grouped / row-mapped GEMM on the 256x256 kernel: same arguments as medmoe_gemm_nt, but `tiles` holds 256-ROW tiles
// (medmoe_dispatch writes that table behind the 128-row one).  Shapes the kernel does not take return MM_ERR_SHAPE.
extern "C" int medmoe_gemm_nt_tiles256(const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                                       int M, int N, int K, const float* bias, const void* residual, int ldr,
                                       void* aux, int ldaux, const int* a_rowmap, const int* c_rowmap,
                                       const int* tiles, const int* tile_count, int max_tiles,
                                       long long strideB, long long strideBias, float alpha, int epi,
                                       int out_f32, int col_perm, hipStream_t stream) {
  if (!A || !B || !C || !tiles || !tile_count || max_tiles <= 0) return MM_ERR_ARG;
  if (M <= 0 || N <= 0 || K < 128 || (K % BK) != 0 || (N % 8) != 0 || col_perm || out_f32 || alpha != 1.f) return MM_ERR_SHAPE;
  if ((lda % 8) || (ldb % 8) || (ldc % 8) || (residual && (ldr % 8)) || (aux && (ldaux % 8))) return MM_ERR_SHAPE;
  if (epi < 0 || epi > EPI_MUL_AUX) return MM_ERR_ARG;
  if ((epi == EPI_MUL_DGELU || epi == EPI_MUL_DRELU || epi == EPI_MUL_AUX) && !aux) return MM_ERR_ARG;
  if (256ll * lda * 2 >= (1ll << 32) || (long long)N * ldb * 2 >= (1ll << 32)) return MM_ERR_SHAPE;
  if (a_rowmap && (long long)M * lda * 2 >= (1ll << 32)) return MM_ERR_SHAPE;      // gathered rows: offsets from A itself
  GemmNTArgs p = nt_args(A, lda, B, ldb, C, ldc, M, N, K, bias, residual, ldr, aux, ldaux, a_rowmap, c_rowmap, tiles, tile_count, strideB,
                         strideBias, 1.f, epi, 0, 0);
  p.n_tiles_n = (N + 255) / 256; p.max_tiles_m = max_tiles;
  const int grid = min(max_tiles * p.n_tiles_n, 256);
  const int spec = nt_spec(p, false);             // never -1: N % 8, alpha and fp32 C were refused above
  if (g_use_nt4w && 2ll * lda < (1ll << 24) && 2ll * ldb < (1ll << 24) && nt4w_launch(p, spec, true, grid, stream)) g_last_nt_kernel = 5;
  else { nt512_launch(p, spec, true, grid, stream); g_last_nt_kernel = 3; }
  return mm_check_launch();
}
