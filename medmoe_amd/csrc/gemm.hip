// bf16 MFMA weight-gradient (TN) GEMMs for gfx950 (MI355X): three kernel generations, the two kernels that sum staged partial tiles,
// and every medmoe_gemm_tn* entry point.  (The file keeps the name it had when it also held what is now gemm_nt*.hip and gemm_scores.hip.)
//   gemm_tn : dW[Nn,Kk] += G[M,Nn]^T . X[M,Kk]                 (wgrad, split over M, fp32 atomics)
// gemm_tn_kernel: the tile, staging and double buffer of gemm_nt_kernel (gemm_nt.hip); v_mfma_f32_32x32x16_bf16 fed by
// ds_read_b64_tr_b16 transposed LDS reads (the contraction index is the ROW of both operands);
// a 32x32 accumulator register is two 128-B row segments = the full-rate float-atomic shape.
#include "gemm_nt.h"
#include "options.h"
#include "det_plan.h"

// --------------------------------------------------------------------------------------------
// gemm_tn (wgrad):  dW[g][n][k] += sum_m G[m][n] * X[xmap(m)][k],  db[g][n] += sum_m G[m][n]
// --------------------------------------------------------------------------------------------
// Every field after ldw has the value of the plain form as its default: an entry point sets what its form needs (tn_args).
struct GemmTNArgs {
  const bf16_t* G; const bf16_t* X; float* dW; float* db = nullptr;
  const int* x_rowmap = nullptr; const int* g_rowmap = nullptr; const int* row_off = nullptr;
  long long strideW = 0; long long strideDb = 0;
  int M, Nn, Kk, ldg, ldx, ldw;
  int tiles_n = 0, tiles_k = 0, nsplit = 1, n_groups = 1;
  long long gcol_stride = 0, xcol_stride = 0;      // COLG build: group g reads the columns G + g * gcol_stride, X + g * xcol_stride (all M rows)
  long long g_chunk_stride = 0; int g_chunk_w = 0;  // COLG build, g_chunk_w > 0: G column c lives at (c / g_chunk_w) * g_chunk_stride + c % g_chunk_w
  const float* gscale = nullptr; long long gscale_gstride = 0; int gscale_ld = 0;   // SCALE build: G row m of group g is multiplied by gscale[g * gscale_gstride + m * gscale_ld]
  float* partial = nullptr;   // gemm_tn4w builds, non-null: every workgroup STORES its 256 x 256 fp32 tile at partial + id * 65536 (accumulator order) instead of adding it to dW atomically; tn_reduce_kernel / tn_reduce_det_kernel sum the row ranges
  float* db_partial = nullptr;   // with partial: the waves' column sums of G go to db_partial + id * 512 (plain stores) instead of atomics on db
};

template <bool MAPPED>
__global__ __launch_bounds__(256) void gemm_tn_kernel(GemmTNArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 32768];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wn = wid >> 1, wk = wid & 1;
  int id = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_k = id % p.tiles_k; id /= p.tiles_k;
  const int tile_n = id % p.tiles_n; id /= p.tiles_n;
  const int split = id % p.nsplit;
  const int group = id / p.nsplit;
  int r0 = 0, r1 = p.M;
  if (p.row_off) { r0 = p.row_off[group]; r1 = p.row_off[group + 1]; }
  const int chunk = (((r1 - r0 + p.nsplit - 1) / p.nsplit) + BK - 1) / BK * BK;
  const int ms = r0 + split * chunk;
  const int me = min(r1, ms + chunk);
  if (ms >= me) return;
  const int n0 = tile_n * 128, k0 = tile_k * 128;

  // staging (register-staged, cdna guide T14): each thread loads 16 B of 4 rows of both tiles into
  // registers BEFORE the MFMA phase and writes them to the other LDS buffer AFTER it, so the HBM
  // latency hides under the MFMAs (an LDS-DMA + transposed-read mix makes hipcc drain the DMA with
  // vmcnt(0) ahead of every ds_read_b64_tr_b16).  Tile = 64 rows x 128 cols (256-B rows);
  // chunk' = chunk ^ ((row&3)<<2) keeps the transposed reads conflict-free; OOB rows are zeros.
  const int srow = wid * 4 + (lane >> 4);
  const int schunk = lane & 15;
  const int lds_off = srow * 256 + ((schunk ^ ((srow & 3) << 2)) << 4);
  const bool g_col_ok = (n0 + schunk * 8) < p.Nn;
  const bool x_col_ok = (k0 + schunk * 8) < p.Kk;
  const bf16_t* gbase = p.G + (g_col_ok ? n0 + schunk * 8 : 0);     // always a valid address; masked below
  const bf16_t* xbase = p.X + (x_col_ok ? k0 + schunk * 8 : 0);
  int gidx[4], xidx[4];
  auto load_idx = [&](int mbase) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mbase + i * 16 + srow;
      const bool ok = m < me;
      const int mc = ok ? m : ms;
      if constexpr (MAPPED) {
        const int gi = p.g_rowmap ? p.g_rowmap[mc] : mc;
        const int xi = p.x_rowmap ? p.x_rowmap[mc] : mc;
        gidx[i] = ok ? gi : -1; xidx[i] = ok ? xi : -1;   // NOTE: physical row 0 must exist (it is read, then masked)
      } else {
        gidx[i] = ok ? m : -1; xidx[i] = gidx[i];
      }
    }
  };
  uint4 rg[4], rx[4];
  bool okg[4], okx[4];
  auto gload = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rg[i] = *(const uint4*)(gbase + (long long)max(gidx[i], 0) * p.ldg);
      rx[i] = *(const uint4*)(xbase + (long long)max(xidx[i], 0) * p.ldx);
      okg[i] = gidx[i] >= 0 && g_col_ok; okx[i] = xidx[i] >= 0 && x_col_ok;
    }
  };
  auto lds_write = [&](int buf) {
    char* sG = smem + buf * 32768 + lds_off;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // masking happens here (after the MFMA phase) so the loads stay in flight across it
      *(uint4*)(sG + i * 4096) = okg[i] ? rg[i] : make_uint4(0, 0, 0, 0);
      *(uint4*)(sG + 16384 + i * 4096) = okx[i] ? rx[i] : make_uint4(0, 0, 0, 0);
    }
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float colsum[2] = {0.f, 0.f};
  const bool do_db = (p.db != nullptr) && tile_k == 0 && wk == 0;

  // transposed-read addressing (cdna guide T10): in each 16-lane group lane 4q+p supplies
  // row q, columns 4p..4p+3 of a 4x16 block and receives column (lane&15).
  const int h = lane >> 5, gam = (lane >> 4) & 1, q = (lane & 15) >> 2, pp = lane & 3;
  const int tr_row = 8 * h + q;                        // + 16*ks (+4 for the second read)
  const int tr_colg = (wn * 64 + gam * 16 + 4 * pp);   // + tn*32   (G tile column, elements)
  const int tr_colx = (wk * 64 + gam * 16 + 4 * pp);

  auto tr_addr = [&](const char* base, int row, int col) -> const char* {
    const int c = col >> 3;
    return base + row * 256 + ((c ^ ((row & 3) << 2)) << 4) + ((col & 7) << 1);
  };

  auto compute = [&](int buf) {
    const char* sG = smem + buf * 32768;
    const char* sX = sG + 16384;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8_t gf[2], xf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int row = ks * 16 + tr_row;
        bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (__attribute__((address_space(3))) bf16x4_t*)tr_addr(sG, row, tr_colg + t * 32));
        bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (__attribute__((address_space(3))) bf16x4_t*)tr_addr(sG, row + 4, tr_colg + t * 32));
        gf[t] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (__attribute__((address_space(3))) bf16x4_t*)tr_addr(sX, row, tr_colx + t * 32));
        hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (__attribute__((address_space(3))) bf16x4_t*)tr_addr(sX, row + 4, tr_colx + t * 32));
        xf[t] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
      if (do_db) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int e = 0; e < 8; ++e) colsum[t] += (float)gf[t][e];
      }
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tk = 0; tk < 2; ++tk)
          acc[tn][tk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gf[tn], xf[tk], acc[tn][tk], 0, 0, 0);
    }
  };

  const int nt = (me - ms + BK - 1) / BK;
  load_idx(ms);
  gload();
  load_idx(ms + BK);
  lds_write(0);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    const bool more = t + 1 < nt;
    if (more) {
      gload();                              // stage t+1 -> registers (indices fetched one iteration ago)
      load_idx(ms + (t + 2) * BK);
    }
    compute(cur);
    if (more) lds_write(cur ^ 1);           // buffer cur^1 was last read before the previous barrier
    __syncthreads();
    cur ^= 1;
  }

  float* dW = p.dW + (long long)group * p.strideW;
  const int kcol = lane & 31;
#pragma unroll
  for (int tn = 0; tn < 2; ++tn)
#pragma unroll
    for (int tk = 0; tk < 2; ++tk) {
      const int k = k0 + wk * 64 + tk * 32 + kcol;
      if (k >= p.Kk) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wn * 64 + tn * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (n < p.Nn) atomicAdd(dW + (long long)n * p.ldw + k, acc[tn][tk][r]);
      }
    }
  if (do_db) {
    float* db = p.db + (long long)group * p.strideDb;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float v = colsum[t] + __shfl_xor(colsum[t], 32, 64);
      const int n = n0 + wn * 64 + t * 32 + kcol;
      if (h == 0 && n < p.Nn) atomicAdd(db + n, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// gemm_tn512: wgrad dW[Nn,Kk] += G[m0:m1, :]^T X[m0:m1, :] with a 256x256 output tile per workgroup, 8 waves
// (2x4 of 128x64), the gemm_nt512 structure: sub-steps of 32 token rows, ring of four 32 KB LDS sub-stages filled
// by LDS-DMA, ping-pong between the two waves of a SIMD.  Half the DMA bytes per flop of the 128x128 kernel.
//   * both operands are reduction-major in memory, so fragments come from ds_read_b64_tr_b16.  hipcc drains
//     every LDS-DMA with vmcnt(0) in front of the tr-read BUILTIN, so the reads are inline asm: the fragment
//     registers pass through the s_waitcnt asm as "+v" operands, which is what orders the MFMAs behind it.
//   * LDS image of a sub-stage: [G: 32 rows x 512 B][X: 32 rows x 512 B], 16-B chunk c of row r stored at
//     chunk c ^ ((r & 3) << 2) (the four rows one transposed read touches land in four different 64-B bank groups).
//   * the M range is split over gridDim so that ~256 workgroups exist; partial sums meet in fp32 atomics.
//   * db = column sums of G: v_dot2_f32_bf16 against ones on the fragments, the four waves that hold the same
//     G columns take turns (sub-step & 3 == wn), only in the k-tile-0 workgroups.
// Requires M % 32 == 0, Nn % 256 == 0, Kk % 256 == 0, no row maps / groups (the 128x128 kernel takes the rest).
// ---------------------------------------------------------------------------------------------
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef short s16x2_t __attribute__((ext_vector_type(2)));
#define TR_READ(dst, addr, imm) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm))

template <bool MAPPED>
__global__ __launch_bounds__(512, 2) void gemm_tn512_kernel(GemmTNArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * SUB3 + (MAPPED ? 32768 : 0)];     // ring (+ the row-map slice)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid & 1, wn = wid >> 1;          // wave tile: G columns wm*128.., X columns wn*64..
  // split-major ids: the tiles of one M range (same G / X rows) sit on one XCD
  int id = xcd_remap(blockIdx.x, gridDim.x);
  const int ntile = p.tiles_n * p.tiles_k;
  // groups vary fastest: unequal groups (an unbalanced router leaves some empty) still spread over every XCD
  const int group = id % p.n_groups; id /= p.n_groups;
  const int split = id / ntile; id -= split * ntile;
  const int tile_n = id / p.tiles_k, tile_k = id - tile_n * p.tiles_k;
  int r0 = 0, r1 = p.M;
  if (MAPPED && p.row_off) { r0 = p.row_off[group]; r1 = p.row_off[group + 1]; }
  const int chunk = (((r1 - r0 + 31) / 32 + p.nsplit - 1) / p.nsplit) * 32;
  const int ms = r0 + split * chunk, me = min(r1, ms + chunk);
  if (ms >= me) return;
  const int U = (me - ms + 31) / 32;              // sub-steps; the last one may hold fewer than 32 valid rows
  const int n0 = tile_n * 256, k0 = tile_k * 256;

  // DMA piece i of wave w fills LDS bytes [(i*8 + w) * 1024, +1024) of the sub-stage: two 512-B rows.
  // MAPPED: rows come through g_rowmap / x_rowmap, rows past the range are clamped
  // (their G rows are zeroed in LDS before the fragment reads), G columns past Nn are clamped (never written back).
  const int prow = (wid << 1) + (lane >> 5);                               // row of pieces 0 / 2; pieces 1 / 3: +16
  unsigned col_g, col_x;
  {
    const int lc0 = (lane & 31) ^ ((prow & 3) << 2);                       // (prow + 16) & 3 == prow & 3
    const int gcol = n0 + lc0 * 8;
    col_g = (unsigned)((MAPPED && gcol >= p.Nn) ? n0 : gcol) * 2u;
    col_x = (unsigned)(k0 + lc0 * 8) * 2u;
  }
  const unsigned ldg2 = (unsigned)p.ldg * 2u, ldx2 = (unsigned)p.ldx * 2u;
  // A row map (g_rowmap or x_rowmap, at most one) is staged through LDS: a ring of 8192 entries (256 sub-steps),
  // filled up front and refilled half a ring at a time every 128 sub-steps.  Loading it from global memory inside
  // the loop makes hipcc drain every LDS-DMA in flight (vmcnt(0)) in front of the first use, which collapses the
  // DMA ring to one stage (measured 113 TF/s); LDS reads are counted by lgkmcnt instead, and the refill's drain
  // happens once per 128 sub-steps.
  const int* rmap = MAPPED ? (p.g_rowmap ? p.g_rowmap : p.x_rowmap) : nullptr;
  int* lmap = (int*)(smem + 4 * SUB3);
  if (MAPPED && rmap) {
    for (int i = tid; i < min(me - ms, 8192); i += 512) lmap[i] = rmap[ms + i];
    __syncthreads();
  }
  int wb = 0, rb = 0, lk = 0;
  int d2 = 0, d1 = 0, d0 = 0;                     // pieces of the three newest sub-stages (no stores in the loop)
  auto issue = [&]() __attribute__((always_inline)) {
    d2 = d1; d1 = d0; d0 = 0;
    if (lk < U) {
      char* sb = smem + wb * SUB3 + wid * 1024;
      unsigned so[4];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ml = min(lk * 32 + prow + j * 16, me - ms - 1);       // row inside the range (clamped past the end)
        const int r = (MAPPED && rmap) ? lmap[ml & 8191] : 0;
        so[j] = (unsigned)((MAPPED && p.g_rowmap) ? r : ms + ml) * ldg2 + col_g;
        so[2 + j] = (unsigned)((MAPPED && p.x_rowmap) ? r : ms + ml) * ldx2 + col_x;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds(GLB_PTR((const char*)(i < 2 ? p.G : p.X) + so[i]), LDS_PTR(sb + i * 8192), 16, 0, 0);
      d0 = 4; ++lk;
      wb = (wb + 1) & 3;
    }
  };
  auto wait_third_newest = [&]() { wait_vmcnt_ring4(__builtin_amdgcn_readfirstlane(d1 + d0)); };

  f32x16_t acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float colsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool do_db = (p.db != nullptr) && tile_k == 0;

  // transposed-read addressing (cdna guide T10): in each 16-lane group lane 4q+p supplies row q, columns 4p..4p+3
  // of a 4x16 block and receives column (lane & 15)
  const int h = lane >> 5, gam = (lane >> 4) & 1, q = (lane & 15) >> 2, pp = lane & 3;
  unsigned ag[4], ax[2];                          // LDS byte address of (row 8h+q, this lane's columns) per 32-column tile
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) {
    const int c = wm * 16 + tn * 4 + gam * 2 + (pp >> 1);
    ag[tn] = (unsigned)(size_t)LDS_PTR(smem) + (8 * h + q) * 512 + ((c ^ (q << 2)) << 4) + ((pp & 1) << 3);
  }
#pragma unroll
  for (int tk = 0; tk < 2; ++tk) {
    const int c = wn * 8 + tk * 4 + gam * 2 + (pp >> 1);
    ax[tk] = (unsigned)(size_t)LDS_PTR(smem) + 16384 + (8 * h + q) * 512 + ((c ^ (q << 2)) << 4) + ((pp & 1) << 3);
  }
  u32x2_t gl[2][4], gh[2][4], xl[2][2], xh[2][2];  // [16-row k sub-step][tile]: rows 8h+q and 8h+q+4
  auto read_frags = [&](int buf) __attribute__((always_inline)) {
    const unsigned bo = buf * SUB3;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const unsigned a = ag[tn] + bo;
      TR_READ(gl[0][tn], a, 0); TR_READ(gh[0][tn], a, 2048); TR_READ(gl[1][tn], a, 8192); TR_READ(gh[1][tn], a, 10240);
    }
#pragma unroll
    for (int tk = 0; tk < 2; ++tk) {
      const unsigned a = ax[tk] + bo;
      TR_READ(xl[0][tk], a, 0); TR_READ(xh[0][tk], a, 2048); TR_READ(xl[1][tk], a, 8192); TR_READ(xh[1][tk], a, 10240);
    }
  };
  auto fence_frags = [&]() __attribute__((always_inline)) {      // data of every tr-read above has arrived
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(gl[0][0]), "+v"(gl[0][1]), "+v"(gl[0][2]), "+v"(gl[0][3]), "+v"(gh[0][0]), "+v"(gh[0][1]), "+v"(gh[0][2]), "+v"(gh[0][3]),
                   "+v"(gl[1][0]), "+v"(gl[1][1]), "+v"(gl[1][2]), "+v"(gl[1][3]), "+v"(gh[1][0]), "+v"(gh[1][1]), "+v"(gh[1][2]), "+v"(gh[1][3]),
                   "+v"(xl[0][0]), "+v"(xl[0][1]), "+v"(xh[0][0]), "+v"(xh[0][1]), "+v"(xl[1][0]), "+v"(xl[1][1]), "+v"(xh[1][0]), "+v"(xh[1][1])
                 :: "memory");
  };
  auto frag = [&](u32x2_t lo, u32x2_t hi) -> bf16x8_t {
    const uint4 v = make_uint4(lo[0], lo[1], hi[0], hi[1]);
    return __builtin_bit_cast(bf16x8_t, v);
  };
  auto compute = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn)
#pragma unroll
        for (int tk = 0; tk < 2; ++tk)
          acc[tn][tk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(gl[ks][tn], gh[ks][tn]), frag(xl[ks][tk], xh[ks][tk]), acc[tn][tk], 0, 0, 0);
  };
  auto add_colsum = [&]() __attribute__((always_inline)) {
    const s16x2_t ones = {(short)0x3F80, (short)0x3F80};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        const uint4 v = __builtin_bit_cast(uint4, frag(gl[ks][tn], gh[ks][tn]));
        float c = colsum[tn];
        c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(s16x2_t, v.x), ones, c, false);
        c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(s16x2_t, v.y), ones, c, false);
        c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(s16x2_t, v.z), ones, c, false);
        c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(s16x2_t, v.w), ones, c, false);
        colsum[tn] = c;
      }
  };

  const int grp = __builtin_amdgcn_readfirstlane(wid >> 2);
  auto seg_barrier = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
  };
  issue(); issue(); issue();
  wait_third_newest();
  __builtin_amdgcn_s_barrier();                   // sub-stage 0 landed for every wave
  asm volatile("" ::: "memory");
  int u_load = 0;
  const int tail = (me - ms) - (U - 1) * 32;       // valid rows of the last sub-step
  auto load_seg = [&]() __attribute__((always_inline)) {
    if (MAPPED && rmap && u_load >= 128 && (u_load & 127) == 0) {
      // sub-steps [u-128, u) are behind every cursor: their ring slots take the rows of sub-steps [u+128, u+256)
      for (int i = tid; i < 4096; i += 512) {
        const int r = (u_load + 128) * 32 + i;
        if (r < me - ms) lmap[r & 8191] = rmap[ms + r];
      }
    }
    if (MAPPED && u_load == U - 1 && tail < 32) {
      // rows past the range hold clamped copies of real rows: zero their G half (every wave zeroes all of them
      // itself, so its own reads below are ordered behind its own writes; zero G rows add nothing to dW or db)
      char* zb = smem + rb * SUB3;
      for (int z = tail * 32 + lane; z < 32 * 32; z += 64) *(uint4*)(zb + z * 16) = make_uint4(0, 0, 0, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    read_frags(rb);
    rb = (rb + 1) & 3;
    issue();
    fence_frags();
    if (do_db && (u_load & 3) == wn && u_load < U) add_colsum();
    ++u_load;
    if (grp == 1) wait_third_newest();
    seg_barrier();
  };
  if (grp == 1) seg_barrier();
  load_seg();
  for (int u = 0; u < U; ++u) {
    compute();
    if (grp == 0) { wait_third_newest(); seg_barrier(); }
    if (grp == 1) seg_barrier();
    load_seg();                                   // past the end: reads a stale buffer, issues nothing
  }
  if (grp == 0) seg_barrier();

  float* dW = p.dW + (MAPPED ? (long long)group * p.strideW : 0ll);
  const int kcol = lane & 31;
#pragma unroll
  for (int tn = 0; tn < 4; ++tn)
#pragma unroll
    for (int tk = 0; tk < 2; ++tk) {
      const int k = k0 + wn * 64 + tk * 32 + kcol;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wm * 128 + tn * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (!MAPPED || n < p.Nn) atomicAdd(dW + (long long)n * p.ldw + k, acc[tn][tk][r]);
      }
    }
  if (do_db) {
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const float v = colsum[tn] + __shfl_xor(colsum[tn], 32, 64);
      const int n = n0 + wm * 128 + tn * 32 + kcol;
      if (h == 0 && (!MAPPED || n < p.Nn)) atomicAdd(p.db + (MAPPED ? (long long)group * p.strideDb : 0ll) + n, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// gemm_tn4w: the plain wgrad (no row maps / groups) on the gemm_nt4w recipe: 256x256 fp32 output tile, FOUR waves (one per
// SIMD) owning 128x128 of it = 16 accumulators of v_mfma_f32_32x32x16_bf16 (256 registers), two fragment sets of 32
// transposed 8-byte reads.  LDS image and DMA as gemm_tn512 (32-row sub-stages of [G 32 x 512 B][X 32 x 512 B], ring of four;
// rows are whole 128-B lines already).  Sub-step u (32 MFMAs of 32 clk): the 32 ds_read_b64_tr_b16 of sub-step u+1 into the
// other fragment set (two per MFMA gap for the first 8 gaps, then one), the 8 DMA pieces of sub-stage u+4 into buffer
// u % 4 (one per 3 MFMAs), lgkmcnt(0) + vmcnt(16) + barrier after MFMA 27.  The DMA runs four sub-stages past the end of
// the range with clamped rows (nothing is computed from them).
// Requires M % 32 == 0, Nn % 256 == 0, Kk % 256 == 0.
// ---------------------------------------------------------------------------------------------
// MAPPED build: expert groups (row_off; ids with the group fastest), ONE gathered operand (row map staged through an 8192-entry LDS
// ring as in gemm_tn512), ragged ranges (rows past the end: G rows zeroed in LDS), Nn a multiple of 128.
// COLG build (plain rows only): n_groups COLUMN groups - group g multiplies the column blocks G[:, g*gcol_stride + (0..Nn)] and
// X[:, g*xcol_stride + (0..Kk)] over all M rows into dW + g*strideW (the per-image U_b^T A_b of the transposed local loss); Nn and Kk
// need not be multiples of 256 (columns past them are fetched from valid memory and never written back).
// Plain and COLG builds address rows through a 64-bit scalar base per sub-stage (per-lane offsets stay below 32 rows), so M * ld may
// exceed 4 GB (the transposed pair matrices: 45k rows of 426 KB).
// SCALE build (COLG only): dW_g += G_g^T diag(w_g) X_g - every G fragment is multiplied by its rows' weights (fp32 product, rounded to bf16
// as a separately stored w * G would be) between the transposed read and the MFMA: 16 VALU per fragment of eight, placed under the four
// MFMAs of the fragment before it.  The 32 weights of a sub-stage travel with it as one more (4-byte) DMA piece into a private 256-byte
// slot per wave and buffer.  With G == X (the Gram products of the local loss, dGm_b = A_b^T diag(d2) A_b) the second operand's DMA hits
// the lines the first one just fetched, and the U = d2 * A matrix is never stored.
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
#define W_READ(dst, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm))
template <bool MAPPED, bool COLG = false, bool SCALE = false>
__global__ __launch_bounds__(256) void gemm_tn4w_kernel(GemmTNArgs p) {
  static_assert(!(MAPPED && COLG), "column groups only in the plain build");
  static_assert(!SCALE || COLG, "row weights only in the column-group build");
  __shared__ __attribute__((aligned(128))) char smem[4 * SUB3 + (MAPPED ? 32768 : 0) + (SCALE ? 4096 : 0)];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid & 1, wn = wid >> 1;          // wave tile: G columns wm*128.., X columns wn*128..
  int id = xcd_remap(blockIdx.x, gridDim.x);      // split-major ids: the tiles of one M range (same G / X rows) sit on one XCD
  const int ntile = p.tiles_n * p.tiles_k;
  int group = 0, ms, me;
  if (MAPPED && p.row_off) {
    // ranges of p.nsplit ROWS each, enumerated over the groups on the device (the group sizes are only known here): every
    // workgroup gets the same amount of work however unequal the groups are; the tiles of one range are adjacent ids
    // (det_plan::tn_group_range: tn_reduce_det_kernel and the host check walk the same enumeration)
    const int tile = id % ntile;
    if (!det_plan::tn_group_range(p.row_off, p.n_groups, p.nsplit, id / ntile, group, ms, me)) return;
    id = tile;
  } else {
    if (COLG) { group = id / (ntile * p.nsplit); id -= group * ntile * p.nsplit; }
    const int split = id / ntile; id -= split * ntile;
    det_plan::tn_split_range(p.M, p.nsplit, split, ms, me);
  }
  const int tile_n = id / p.tiles_k, tile_k = id - tile_n * p.tiles_k;
  if (ms >= me) return;
  const int U = (me - ms + 31) / 32;              // sub-steps; MAPPED: the last one may hold fewer than 32 valid rows
  const int tail = (me - ms) - (U - 1) * 32;
  const int n0 = tile_n * 256, k0 = tile_k * 256;

  // DMA piece i (0..7) of wave w fills LDS bytes [(i * 4 + w) * 1024, +1024) of the sub-stage: two 512-B rows.
  const int prow = (wid << 1) + (lane >> 5);      // row of piece 0 inside its 32-row half; piece i: + 8 * (i & 3)
  const unsigned lds0 = (unsigned)(size_t)smem;
  unsigned col_g, col_x;
  {
    const int lc0 = (lane & 31) ^ ((prow & 3) << 2);
    const int gcol = n0 + lc0 * 8;
    col_g = (unsigned)(((MAPPED || COLG) && gcol >= p.Nn) ? n0 : gcol) * 2u;       // columns past Nn: fetched from valid memory, never written back
    if (COLG && p.g_chunk_w > 0) {
      // chunked columns (the image-major pair matrices: 208 columns per image, images g_chunk_stride apart): a 256-column tile spans at
      // most a few chunks; the first one's base is scalar (gbase below), the lane keeps its distance from it (< 2^32 bytes, host check)
      const int gc = (gcol >= p.Nn) ? n0 : gcol;
      const int c0 = n0 / p.g_chunk_w, cc = gc / p.g_chunk_w;
      col_g = (unsigned)((long long)(cc - c0) * p.g_chunk_stride + (gc - cc * p.g_chunk_w)) * 2u;
    }
    const int xcol = k0 + lc0 * 8;
    col_x = (unsigned)((COLG && xcol >= p.Kk) ? k0 : xcol) * 2u;
  }
  const int* rmap = MAPPED ? (p.g_rowmap ? p.g_rowmap : p.x_rowmap) : nullptr;
  int* lmap = (int*)(smem + 4 * SUB3);
  if (MAPPED && rmap) {
    for (int i = tid; i < min(me - ms, 8192); i += 256) lmap[i] = rmap[ms + i];
    __syncthreads();
  }
  const unsigned ldg2 = (unsigned)p.ldg * 2u, ldx2 = (unsigned)p.ldx * 2u;
  // per-lane byte offsets of the current sub-stage's piece 0 rows; pieces 1..3 add 8 rows each (scalar); the next
  // sub-stage adds 32 rows.  Rows are clamped to the range's last row (only past the end of the range).
  int lk = 0, wb = 0, rb = 0;
  unsigned sg[4], sx[4];
  // plain / COLG builds: whole sub-stages only (M % 32 == 0), per-lane offsets are those of the sub-stage's 32 rows and the sub-stage
  // itself is a scalar 64-bit base (clamped to the range's last sub-stage for the four the DMA runs ahead)
  const char* gbase = (const char*)p.G + (COLG ? (long long)group * p.gcol_stride * 2 : 0ll)
                      + ((COLG && p.g_chunk_w > 0) ? (long long)(n0 / p.g_chunk_w) * p.g_chunk_stride * 2 : 0ll);
  const char* xbase = (const char*)p.X + (COLG ? (long long)group * p.xcol_stride * 2 : 0ll);
  const char* gsub = gbase;
  const char* xsub = xbase;
  const char* wbase = SCALE ? (const char*)(p.gscale + (long long)group * p.gscale_gstride) : nullptr;
  const char* wsub = wbase;
  int wr0 = 0;
  const unsigned wl0 = lds0 + 4 * SUB3 + wid * 1024;              // SCALE: this wave's four 256-byte weight slots
  auto setup_rows = [&]() __attribute__((always_inline)) {
    if constexpr (!MAPPED) {
      // wave-uniform by construction; readfirstlane makes it provably scalar, so every DMA piece is `global_load_lds v_off, s[base]`
      // with the persistent per-lane offsets (a 64-bit VGPR address would be a TEMPORARY register pair: see keep_frags below)
      const long long r0 = ms + min(lk, (me - ms) / 32 - 1) * 32;
      auto uni = [](const char* q) -> const char* {
        const unsigned long long v = (unsigned long long)q;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return (const char*)(((unsigned long long)hi << 32) | lo);
      };
      gsub = uni(gbase + r0 * (long long)ldg2);
      xsub = uni(xbase + r0 * (long long)ldx2);
      if constexpr (SCALE) { wr0 = (int)r0; wsub = uni(wbase + r0 * (long long)p.gscale_ld * 4); }
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ml = min(lk * 32 + prow + 8 * j, me - ms - 1);         // row inside the range (clamped past the end)
      const unsigned rm = (MAPPED && rmap) ? (unsigned)lmap[ml & 8191] : 0u;
      sg[j] = ((MAPPED && p.g_rowmap) ? rm : (unsigned)(ms + ml)) * ldg2 + col_g;
      sx[j] = ((MAPPED && p.x_rowmap) ? rm : (unsigned)(ms + ml)) * ldx2 + col_x;
    }
  };
  if constexpr (!MAPPED) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { sg[j] = (unsigned)(prow + 8 * j) * ldg2 + col_g; sx[j] = (unsigned)(prow + 8 * j) * ldx2 + col_x; }
  }
  unsigned ldsW = lds0 + wid * 1024;
  auto advance = [&]() __attribute__((always_inline)) {
    ++lk; wb = (wb + 1) & 3;
    setup_rows();
    ldsW = lds0 + wb * SUB3 + wid * 1024;
  };
  auto piece = [&](int i) __attribute__((always_inline)) {
    __builtin_amdgcn_global_load_lds(GLB_PTR((i < 4 ? gsub : xsub) + (i < 4 ? sg[i & 3] : sx[i & 3])),
                                     (__attribute__((address_space(3))) void*)(size_t)(ldsW + i * 4096), 16, 0, 0);
  };
  // SCALE: the weights of rows wr0 .. wr0 + 63 (this sub-stage's 32 and, unused, the next 32; clamped to the last row) into slot wb
  auto wpiece = [&]() __attribute__((always_inline)) {
    if constexpr (SCALE) {
      const unsigned wo = (unsigned)min(lane, p.M - 1 - wr0) * (unsigned)p.gscale_ld * 4u;
      __builtin_amdgcn_global_load_lds(GLB_PTR(wsub + wo), (__attribute__((address_space(3))) void*)(size_t)(wl0 + wb * 256), 4, 0, 0);
    }
  };

  f32x16_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float colsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool do_db = (p.db != nullptr) && tile_k == 0;

  // transposed-read addressing as in gemm_tn512
  const int h = lane >> 5, gam = (lane >> 4) & 1, q = (lane & 15) >> 2, pp = lane & 3;
  unsigned aa[8];                                 // G tiles 0..3, X tiles 0..3
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cg = wm * 16 + t * 4 + gam * 2 + (pp >> 1), cx = wn * 16 + t * 4 + gam * 2 + (pp >> 1);
    aa[t] = lds0 + (8 * h + q) * 512 + ((cg ^ (q << 2)) << 4) + ((pp & 1) << 3);
    aa[4 + t] = lds0 + 16384 + (8 * h + q) * 512 + ((cx ^ (q << 2)) << 4) + ((pp & 1) << 3);
  }
  struct Frags { u32x2_t gl[2][4], gh[2][4], xl[2][4], xh[2][4]; };
  Frags f0, f1;
  // SCALE: ONE set of row weights wv[ks][rows +0 / +4] - the current set's until its last G fragment is scaled (MFMA 24), then the next
  // set's (read there, landed at the wait after MFMA 27, first used under MFMA 28)
  u32x4_t wv[2][2];
  const unsigned wa = wl0 + 32 * (lane >> 5);     // this lane's eight rows of a 16-row half start at row 8 h
  auto read_w = [&](int buf) __attribute__((always_inline)) {
    if constexpr (SCALE) {
      const unsigned a = wa + buf * 256;
      W_READ(wv[0][0], a, 0); W_READ(wv[0][1], a, 16); W_READ(wv[1][0], a, 64); W_READ(wv[1][1], a, 80);
    }
  };
  // G fragment number i = ks * 4 + tn of a set times its rows' weights
  auto scale_frag = [&](Frags& f, auto ic) __attribute__((always_inline)) {
    if constexpr (SCALE) {
      constexpr int i = decltype(ic)::value, ks = i >> 2, tn = i & 3;
      auto sc = [](unsigned v, unsigned w0, unsigned w1) -> unsigned {
        return pack2bf(__uint_as_float(v << 16) * __uint_as_float(w0), __uint_as_float(v & 0xffff0000u) * __uint_as_float(w1));
      };
      const u32x4_t wl = wv[ks][0], wh = wv[ks][1];
      f.gl[ks][tn][0] = sc(f.gl[ks][tn][0], wl[0], wl[1]); f.gl[ks][tn][1] = sc(f.gl[ks][tn][1], wl[2], wl[3]);
      f.gh[ks][tn][0] = sc(f.gh[ks][tn][0], wh[0], wh[1]); f.gh[ks][tn][1] = sc(f.gh[ks][tn][1], wh[2], wh[3]);
    }
  };
  // read number g (0..31) of a sub-stage: operand (G / X), tile t, 16-row half ks, rows +0 / +4
  auto read_one = [&](Frags& f, unsigned bo, auto gc) __attribute__((always_inline)) {
    constexpr int g = decltype(gc)::value, t = (g >> 2) & 3, ks = (g >> 1) & 1, hi = g & 1;
    constexpr int off = ks * 8192 + hi * 2048;
    const unsigned a = aa[(g < 16 ? 0 : 4) + t] + bo;
    if constexpr (g < 16) { if constexpr (hi) TR_READ(f.gh[ks][t], a, off); else TR_READ(f.gl[ks][t], a, off); }
    else { if constexpr (hi) TR_READ(f.xh[ks][t], a, off); else TR_READ(f.xl[ks][t], a, off); }
  };
  auto frag = [&](u32x2_t lo, u32x2_t hi) -> bf16x8_t {
    const uint4 v = make_uint4(lo[0], lo[1], hi[0], hi[1]);
    return __builtin_bit_cast(bf16x8_t, v);
  };
  auto add_colsum = [&](Frags& f) __attribute__((always_inline)) {
    const s16x2_t ones = {(short)0x3F80, (short)0x3F80};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        const uint4 v = __builtin_bit_cast(uint4, frag(f.gl[ks][tn], f.gh[ks][tn]));
        float c = colsum[tn];
        c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(s16x2_t, v.x), ones, c, false);
        c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(s16x2_t, v.y), ones, c, false);
        c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(s16x2_t, v.z), ones, c, false);
        c = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(s16x2_t, v.w), ones, c, false);
        colsum[tn] = c;
      }
  };
  int u_now = 0;
  // rows past the range hold clamped copies of real rows: zero their G half (every wave zeroes all of them itself, so its own
  // reads are ordered behind its own writes; zero G rows add nothing to dW or db)
  auto zero_tail = [&](int buf) __attribute__((always_inline)) {
    char* zb = smem + buf * SUB3;
    for (int z = tail * 32 + lane; z < 32 * 32; z += 64) *(uint4*)(zb + z * 16) = make_uint4(0, 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  auto substep = [&](Frags& c, Frags& n) __attribute__((always_inline)) {
    const unsigned bo = rb * SUB3;
    if (MAPPED && rmap && u_now >= 128 && (u_now & 127) == 0) {
      // sub-steps [u-128, u) are behind every cursor: their ring slots take the rows of sub-steps [u+128, u+256)
      for (int i = tid; i < 4096; i += 256) {
        const int r = (u_now + 128) * 32 + i;
        if (r < me - ms) lmap[r & 8191] = rmap[ms + r];
      }
    }
    if (MAPPED && u_now + 1 == U - 1 && tail < 32) zero_tail(rb);  // the sub-stage read during this sub-step is the ragged last one
    if (do_db && (u_now & 1) == wn) add_colsum(c);               // the two waves that hold the same G columns take turns
    auto one = [&](auto qc) __attribute__((always_inline)) {
      constexpr int qq = decltype(qc)::value, ks = qq >> 4, tn = (qq >> 2) & 3, tk = qq & 3;
      acc[tn][tk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(c.gl[ks][tn], c.gh[ks][tn]), frag(c.xl[ks][tk], c.xh[ks][tk]), acc[tn][tk], 0, 0, 0);
      if constexpr (qq < 24) {
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (qq < 8) { read_one(n, bo, std::integral_constant<int, 2 * qq>{}); read_one(n, bo, std::integral_constant<int, 2 * qq + 1>{}); }
        else read_one(n, bo, std::integral_constant<int, qq + 8>{});
        if constexpr (qq % 3 == 2) piece(qq / 3);
        if constexpr (SCALE && qq == 0) wpiece();
        if constexpr (SCALE && qq % 4 == 0) scale_frag(c, std::integral_constant<int, qq / 4 + 1>{});
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (SCALE && qq == 24) {
        __builtin_amdgcn_sched_barrier(0);
        scale_frag(c, std::integral_constant<int, 7>{});
        read_w(rb);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (SCALE && qq == 28) {           // the next set's reads have landed (wait after MFMA 27): its first fragment
        __builtin_amdgcn_sched_barrier(0);
        scale_frag(n, std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (qq == 25) { advance(); rb = (rb + 1) & 3; ++u_now; }
      if constexpr (qq == 27) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_waitcnt vmcnt(16)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
      }
    };
    static_for<32>(one);
  };

  setup_rows();
  for (int v = 0; v < 4; ++v) {                   // sub-stages 0..3
    wpiece();
#pragma unroll
    for (int i = 0; i < 8; ++i) piece(i);
    advance();
  }
  asm volatile("s_waitcnt vmcnt(24)" ::: "memory");   // (SCALE: nine pieces per sub-stage - the same counts wait for a little more)
  __builtin_amdgcn_s_barrier();                   // sub-stage 0 landed for every wave
  asm volatile("" ::: "memory");
  if (MAPPED && U == 1 && tail < 32) zero_tail(0);
  {
    auto rd = [&](auto gc) __attribute__((always_inline)) { read_one(f0, 0u, gc); };
    static_for<32>(rd);
    read_w(0);
  }
  rb = 1;
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_waitcnt vmcnt(16)" ::: "memory");
  __builtin_amdgcn_s_barrier();                   // every wave has read buffer 0; sub-stage 1 landed
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
  scale_frag(f0, std::integral_constant<int, 0>{});
  int u = 0;
  for (; u + 1 < U; u += 2) { substep(f0, f1); substep(f1, f0); }
  if (u < U) substep(f0, f1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA ran four sub-stages past the end
  // The last sub-step's transposed reads fetch a sub-stage nobody multiplies: to the compiler their destination registers are dead
  // from the asm statement on, but the LDS writes them when the data arrives.  Keep both fragment sets allocated up to here, so that no
  // temporary (an address pair of a DMA piece, say) is placed in a register with a read still in flight.
  auto keep_frags = [&](Frags& f) __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      asm volatile("" :: "v"(f.gl[ks][0]), "v"(f.gl[ks][1]), "v"(f.gl[ks][2]), "v"(f.gl[ks][3]), "v"(f.gh[ks][0]), "v"(f.gh[ks][1]), "v"(f.gh[ks][2]), "v"(f.gh[ks][3]));
      asm volatile("" :: "v"(f.xl[ks][0]), "v"(f.xl[ks][1]), "v"(f.xl[ks][2]), "v"(f.xl[ks][3]), "v"(f.xh[ks][0]), "v"(f.xh[ks][1]), "v"(f.xh[ks][2]), "v"(f.xh[ks][3]));
    }
  };
  if constexpr (SCALE) asm volatile("" :: "v"(wv[0][0]), "v"(wv[0][1]), "v"(wv[1][0]), "v"(wv[1][1]));
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  keep_frags(f0); keep_frags(f1);

  float* dW = p.dW + ((MAPPED || COLG) ? (long long)group * p.strideW : 0ll);
  const int kcol = lane & 31;
  const bool staged = p.partial != nullptr;
  // the slot of this workgroup's partial tile is its (remapped) id: split * ntile + tile in the plain build, range * ntile + tile in the
  // MAPPED one, (group * nsplit + split) * ntile + tile in the COLG one - recomputed here, not kept across the k-loop
  const int pid = staged ? xcd_remap(blockIdx.x, gridDim.x) : 0;
  if (staged) {
    // STAGED: 256 whole-wave 256-byte stores in accumulator order [wave][tn][tk][r][lane] - plain stores leave a CU five times faster than
    // the same bytes as fp32 atomics (which execute at the memory side, ~1.3 TB/s chip-wide: 64 MB per launch whatever the row count).
    // MAPPED / COLG: rows and columns past Nn / Kk are stored too (whatever they hold); the summing kernel never reads them back into dW.
    float* part = p.partial + ((long long)pid << 16) + (wid << 14) + lane;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn)
#pragma unroll
      for (int tk = 0; tk < 4; ++tk)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[((tn * 4 + tk) * 16 + r) * 64] = acc[tn][tk][r];
  } else {
#pragma unroll
  for (int tn = 0; tn < 4; ++tn)
#pragma unroll
    for (int tk = 0; tk < 4; ++tk) {
      const int k = k0 + wn * 128 + tk * 32 + kcol;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wm * 128 + tn * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if ((!(MAPPED || COLG) || n < p.Nn) && (!COLG || k < p.Kk)) atomicAdd(dW + (long long)n * p.ldw + k, acc[tn][tk][r]);
      }
    }
  }
  if (do_db) {
    const bool db_staged = staged && p.db_partial != nullptr;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const float v = colsum[tn] + __shfl_xor(colsum[tn], 32, 64);
      const int n = n0 + wm * 128 + tn * 32 + kcol;
      if (db_staged) {                // [slot][wave][tn][column]: the two waves that took turns on the same G columns keep separate sums
        if (h == 0) p.db_partial[((long long)pid << 9) + (wid << 7) + tn * 32 + kcol] = v;
      } else if (h == 0 && (!(MAPPED || COLG) || n < p.Nn)) atomicAdd(p.db + ((MAPPED || COLG) ? (long long)group * p.strideDb : 0ll) + n, v);
    }
  }
}

// Second half of the STAGED plain wgrad: dW tile += sum over the row ranges of the partial tiles gemm_tn4w_kernel stored (fixed order:
// the result does not depend on which workgroup finished first, unlike the atomic form).  64 blocks per 256 x 256 tile, a float4 per thread.
__global__ __launch_bounds__(256) void tn_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dW, int ldw, int ntile,
                                                        int tiles_k, int nvalid) {
  const int tile = blockIdx.x >> 6;
  const int e4 = (((blockIdx.x & 63) << 8) + threadIdx.x) << 2;
  float4 s = {0.f, 0.f, 0.f, 0.f};
  for (int sp = 0; sp < nvalid; ++sp) {
    const float4 v = *(const float4*)(partial + ((long long)(sp * ntile + tile) << 16) + e4);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const int lane = e4 & 63, r = (e4 >> 6) & 15, tk = (e4 >> 10) & 3, tn = (e4 >> 12) & 3, wid = e4 >> 14;
  const int wm = wid & 1, wn = wid >> 1, h = lane >> 5, kcol = lane & 31;
  const int tile_n = tile / tiles_k, tile_k = tile - tile_n * tiles_k;
  const int n = tile_n * 256 + wm * 128 + tn * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
  const int k = tile_k * 256 + wn * 128 + tk * 32 + kcol;
  float4* d = (float4*)(dW + (long long)n * ldw + k);
  float4 o = *d;
  o.x += s.x; o.y += s.y; o.z += s.z; o.w += s.w;
  *d = o;
}

// The summing kernel of every other staged launch (deterministic mode): dW[group] tile += the partial tiles of its slots, walked in slot
// order, and db[group] += the slots' column sums (wave wn = 0, then wn = 1 of each slot).  64 blocks per (group, 256 x 256 tile), a float4
// per thread; rows >= Nn and columns >= Kk of a tile are never written (Kk % 8 == 0: a float4 is inside or outside as a whole).
//   mode 0: slot = (group * nsplit + sp) * ntile + tile for sp < nvalid (plain / row-mapped ranges: group 0; COLG: column groups)
//   mode 1: the ranges of R rows enumerated from row_off exactly as gemm_tn4w_kernel<true> enumerates them - a group's ranges are adjacent
struct TnReduceArgs {
  const float* partial; const float* db_partial; float* dW; float* db; const int* row_off;
  long long strideW, strideDb;
  int ldw, Nn, Kk, tiles_n, tiles_k, mode, nsplit, nvalid, n_groups, R, vec;
};
__global__ __launch_bounds__(256) void tn_reduce_det_kernel(TnReduceArgs p) {
  const int ntile = p.tiles_n * p.tiles_k;
  const int gt = blockIdx.x >> 6;
  const int group = gt / ntile, tile = gt - group * ntile;
  int first, count;
  if (p.mode == 0) { first = group * p.nsplit; count = p.nvalid; }
  else det_plan::tn_group_ranges(p.row_off, group, p.R, first, count);
  const int e4 = (((blockIdx.x & 63) << 8) + threadIdx.x) << 2;
  float4 s = {0.f, 0.f, 0.f, 0.f};
  for (int sp = 0; sp < count; ++sp) {
    const float4 v = *(const float4*)(p.partial + ((long long)((first + sp) * ntile + tile) << 16) + e4);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const int lane = e4 & 63, r = (e4 >> 6) & 15, tk = (e4 >> 10) & 3, tn = (e4 >> 12) & 3, wid = e4 >> 14;
  const int wm = wid & 1, wn = wid >> 1, h = lane >> 5, kcol = lane & 31;
  const int tile_n = tile / p.tiles_k, tile_k = tile - tile_n * p.tiles_k;
  const int n = tile_n * 256 + wm * 128 + tn * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
  const int k = tile_k * 256 + wn * 128 + tk * 32 + kcol;
  if (count > 0 && n < p.Nn && k < p.Kk) {
    float* d = p.dW + (long long)group * p.strideW + (long long)n * p.ldw + k;
    if (p.vec) {
      float4 o = *(float4*)d;
      o.x += s.x; o.y += s.y; o.z += s.z; o.w += s.w;
      *(float4*)d = o;
    } else { d[0] += s.x; d[1] += s.y; d[2] += s.z; d[3] += s.w; }
  }
  if (p.db && tile_k == 0 && (blockIdx.x & 63) == 0 && count > 0) {
    const int c = threadIdx.x;                    // column of the tile: wave half wm = c >> 7, then [tn][kcol]
    const int nn = tile_n * 256 + c;
    float a = 0.f;
    for (int sp = 0; sp < count; ++sp) {
      const float* q = p.db_partial + ((long long)((first + sp) * ntile + tile) << 9) + ((c >> 7) << 7) + (c & 127);
      a += q[0];
      a += q[256];
    }
    if (nn < p.Nn) p.db[(long long)group * p.strideDb + nn] += a;
  }
}

int g_use_tn512 = 1, g_use_tn4w = 1, g_tn_rows = 1024, g_tn_min_rows = 2048, g_tn_rows4w = 0;      // options.h, keys 3, 8, 4, 9 and 10

// Which TN kernel the most recent launch of this process took (medmoe_last_gemm_tn_kernel): host-side state only, written at every launch
// site below and never by a refused call.  id = generation * 8 + build * 2 + staged:  generation 0 gemm_tn_kernel (128 x 128 tile),
// 1 gemm_tn512_kernel, 2 gemm_tn4w_kernel;  build 0 plain, 1 MAPPED, 2 COLG, 3 COLG + SCALE;  staged 1: the partial tiles went through a
// scratch and a summing kernel.  split: the launch's nsplit (row ranges per tile; the ROWS per range in the grouped four-wave form).
enum { TN_G128 = 0, TN_G512 = 1, TN_G4W = 2, TN_B_PLAIN = 0, TN_B_MAPPED = 1, TN_B_COLG = 2, TN_B_SCALE = 3 };
static int g_last_tn_kernel = -1, g_last_tn_split = 0;
static inline void tn_ran(int gen, int build, bool staged, int split) { g_last_tn_kernel = gen * 8 + build * 2 + (staged ? 1 : 0); g_last_tn_split = split; }
extern "C" int medmoe_last_gemm_tn_kernel(int* split) {
  if (split) *split = g_last_tn_split;
  return g_last_tn_kernel;
}

// Every entry point below: validate, tn_args, set what this form needs, launch, return mm_check_launch().
static GemmTNArgs tn_args(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, int M, int Nn, int Kk) {
  GemmTNArgs p;
  p.G = (const bf16_t*)G; p.X = (const bf16_t*)X; p.dW = dW;
  p.M = M; p.Nn = Nn; p.Kk = Kk; p.ldg = ldg; p.ldx = ldx; p.ldw = ldw;
  return p;
}

static bool tn_fit32(int M, int ldg, int ldx) { return (long long)M * ldg * 2 < (1ll << 32) && (long long)M * ldx * 2 < (1ll << 32); }   // 32-bit DMA offsets

// row ranges per 256 x 256 tile of the plain forms: ~256 workgroups, at least g_tn_min_rows rows (g_tn_min_rows / 32 sub-steps) each
static int tn_row_split(long long ntile, int M) { return (int)max(1ll, min(256ll / ntile, (long long)M / g_tn_min_rows)); }

static inline bool tn_vec_ok(const float* dW, int ldw, long long strideW) {
  return ((unsigned long long)dW & 15) == 0 && (ldw % 4) == 0 && (strideW % 4) == 0;
}

// gemm_tn_kernel takes every shape: one workgroup per (group, 128 x 128 tile, row range)
static void tn128_launch(GemmTNArgs& p, int nsplit, hipStream_t stream) {
  p.tiles_n = (p.Nn + 127) / 128; p.tiles_k = (p.Kk + 127) / 128; p.nsplit = nsplit;
  const int grid = p.tiles_n * p.tiles_k * nsplit * p.n_groups;
  if (p.x_rowmap || p.g_rowmap) hipLaunchKernelGGL(gemm_tn_kernel<true>, dim3(grid), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(gemm_tn_kernel<false>, dim3(grid), dim3(256), 0, stream, p);
  tn_ran(TN_G128, (p.x_rowmap || p.g_rowmap) ? TN_B_MAPPED : TN_B_PLAIN, false, nsplit);
}

extern "C" int medmoe_gemm_tn(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw,
                              float* db, int M, int Nn, int Kk, const int* x_rowmap,
                              const int* g_rowmap, const int* row_off, int n_groups, long long strideW,
                              long long strideDb, int nsplit, hipStream_t stream) {
  if (!G || !X || !dW) return MM_ERR_ARG;
  if (M <= 0 || Nn <= 0 || Kk <= 0 || (Nn % 8) || (Kk % 8) || (ldg % 8) || (ldx % 8)) return MM_ERR_SHAPE;
  if (n_groups < 1 || nsplit < 1) return MM_ERR_ARG;
  GemmTNArgs p = tn_args(G, ldg, X, ldx, dW, ldw, M, Nn, Kk);
  p.db = db; p.x_rowmap = x_rowmap; p.g_rowmap = g_rowmap; p.row_off = row_off; p.strideW = strideW; p.strideDb = strideDb;
  const bool fit32 = tn_fit32(M, ldg, ldx);
  if (g_use_tn512 && !x_rowmap && !g_rowmap && !row_off && n_groups == 1 && (M % 32) == 0 && (Nn % 256) == 0 && (Kk % 256) == 0 &&
      M >= 4096 && fit32) {
    p.tiles_n = Nn / 256; p.tiles_k = Kk / 256;
    const int ntile = p.tiles_n * p.tiles_k;
    p.nsplit = tn_row_split(ntile, M);
    if (p.nsplit > 1) ++g_mm_nondet;
    if (g_use_tn4w) hipLaunchKernelGGL(gemm_tn4w_kernel<false>, dim3(ntile * p.nsplit), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(gemm_tn512_kernel<false>, dim3(ntile * p.nsplit), dim3(512), 0, stream, p);
    tn_ran(g_use_tn4w ? TN_G4W : TN_G512, TN_B_PLAIN, false, p.nsplit);
    return mm_check_launch();
  }
  // grouped (row_off) and/or ONE row-mapped operand, ragged row counts, Nn a multiple of 128: the MAPPED build
  if (g_use_tn512 && !(x_rowmap && g_rowmap) && (Nn % 128) == 0 && (Kk % 256) == 0 && M / n_groups >= 4096 && fit32) {
    p.tiles_n = (Nn + 255) / 256; p.tiles_k = Kk / 256;
    const int ntile = p.tiles_n * p.tiles_k;
    // groups are unequal (router imbalance): ranges of ~g_tn_rows rows, several waves of workgroups, so that a large
    // group's work spreads over the chip (3 ranges per group measured slower than 50)
    p.n_groups = n_groups;
    ++g_mm_nondet;                                  // several row ranges add to one tile
    if (g_use_tn4w && row_off) {
      // equal ranges of R rows over all groups, enumerated on the device.  tools/tn_rows_sweep4w.py (768x768 tiles, 8 groups,
      // us per launch; balanced / 2-of-8 groups): M = 401408: R 1024 887 / 860, 2048 635 / 651, 4096 540 / 547, 8192 502 / 629,
      // 16384 473 / 787;  M = 50176: 2048 95 / 143, 4096 104 / 109, 8192 149 / 182.  Long ranges lose on unequal groups: their few
      // output tiles take every range's fp32 atomics at the same time.
      long long R = g_tn_rows4w > 0 ? (g_tn_rows4w + 31) / 32 * 32 : 4096;
      p.nsplit = (int)R;
      const int max_ranges = (int)(M / R) + n_groups;
      hipLaunchKernelGGL(gemm_tn4w_kernel<true>, dim3(ntile * max_ranges), dim3(256), 0, stream, p);
      tn_ran(TN_G4W, TN_B_MAPPED, false, p.nsplit);
      return mm_check_launch();
    }
    p.nsplit = max(1, M / n_groups / g_tn_rows);
    if (g_use_tn4w) hipLaunchKernelGGL(gemm_tn4w_kernel<true>, dim3(ntile * p.nsplit * n_groups), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(gemm_tn512_kernel<true>, dim3(ntile * p.nsplit * n_groups), dim3(512), 0, stream, p);
    tn_ran(g_use_tn4w ? TN_G4W : TN_G512, TN_B_MAPPED, false, p.nsplit);
    return mm_check_launch();
  }
  p.n_groups = n_groups;
  if (nsplit > 1) ++g_mm_nondet;                    // nsplit == 1: one workgroup per (group, tile), its atomics arrive in program order
  tn128_launch(p, nsplit, stream);
  return mm_check_launch();
}

// Plain wgrad dW[Nn, Kk] += G^T X (db += column sums of G) in the staged form when it applies - plain rows, Nn and Kk multiples of 256,
// M % 32 == 0 and >= 4096, `scratch` holding tiles x row ranges partial tiles of 65536 floats - else exactly medmoe_gemm_tn(nsplit 16).
// db leaves through the scratch as well (512 floats per partial tile behind the tiles, summed in range order) when the scratch has that
// room; without it db keeps its atomics.  The caller owns `scratch` and must not share it between launches that may run concurrently
// (one per stream).
extern "C" int medmoe_gemm_tn_staged(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, float* db, int M, int Nn, int Kk,
                                     float* scratch, long long scratch_floats, hipStream_t stream) {
  if (!G || !X || !dW) return MM_ERR_ARG;
  if (M <= 0 || Nn <= 0 || Kk <= 0 || (Nn % 8) || (Kk % 8) || (ldg % 8) || (ldx % 8)) return MM_ERR_SHAPE;
  if (scratch && g_use_tn512 && g_use_tn4w && (M % 32) == 0 && (Nn % 256) == 0 && (Kk % 256) == 0 && M >= 4096 && tn_fit32(M, ldg, ldx) &&
      (ldw % 4) == 0) {
    GemmTNArgs p = tn_args(G, ldg, X, ldx, dW, ldw, M, Nn, Kk);
    p.db = db;
    p.tiles_n = Nn / 256; p.tiles_k = Kk / 256;
    const int ntile = p.tiles_n * p.tiles_k;
    p.nsplit = tn_row_split(ntile, M);
    if (p.nsplit >= 2 && (long long)ntile * p.nsplit * 65536 <= scratch_floats) {
      p.partial = scratch;
      const int chunk = det_plan::tn_chunk(M, p.nsplit);
      const int nvalid = (M + chunk - 1) / chunk;
      const long long slots = (long long)ntile * p.nsplit;
      if (db && slots * (65536 + 512) <= scratch_floats) p.db_partial = scratch + slots * 65536;
      if (db && !p.db_partial) ++g_mm_nondet;       // db still meets in atomics
      hipLaunchKernelGGL(gemm_tn4w_kernel<false>, dim3(ntile * p.nsplit), dim3(256), 0, stream, p);
      if (p.db_partial) {
        TnReduceArgs q{scratch, p.db_partial, dW, db, nullptr, 0, 0, ldw, Nn, Kk, p.tiles_n, p.tiles_k, 0, p.nsplit, nvalid, 1, 0, 1};
        q.vec = tn_vec_ok(dW, ldw, 0);
        hipLaunchKernelGGL(tn_reduce_det_kernel, dim3(ntile * 64), dim3(256), 0, stream, q);
      } else {
        hipLaunchKernelGGL(tn_reduce_kernel, dim3(ntile * 64), dim3(256), 0, stream, scratch, dW, ldw, ntile, p.tiles_k, nvalid);
      }
      tn_ran(TN_G4W, TN_B_PLAIN, true, p.nsplit);
      return mm_check_launch();
    }
  }
  return medmoe_gemm_tn(G, ldg, X, ldx, dW, ldw, db, M, Nn, Kk, nullptr, nullptr, nullptr, 1, 0, 0, 16, stream);
}

// dW[g][Nn][Kk] += G_g^T X_g, G_g = G + g*gcol_stride, X_g = X + g*xcol_stride ([M][ld] views; column blocks of one matrix, separate
// matrices, or the same one for stride 0), over ALL M rows (fp32 atomics: zero dW first).  M % 32 == 0; one group's Nn x Kk block is tiled 256 x 256 (partial tiles masked).  With n_groups == 1 and strides 0
// this is the plain wgrad for operands whose M * ld exceeds 4 GB (the transposed local-loss matrices).
// g_chunk_w > 0: G's Nn columns are stored in chunks of g_chunk_w columns (a multiple of 8), chunk j at G + j * g_chunk_stride (the
// image-major pair matrices seen as ONE [M][B * HWp] operand: full 256-column tiles across images).
static int tn_cols_impl(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, int M, int Nn, int Kk,
                        int n_groups, long long gcol_stride, long long xcol_stride, long long strideW, int g_chunk_w,
                        long long g_chunk_stride, bool det, float* scratch, long long scratch_floats, hipStream_t stream) {
  if (!G || !X || !dW) return MM_ERR_ARG;
  if (M < 32 || (M % 32) || Nn <= 0 || Kk <= 0 || (Nn % 8) || (Kk % 8) || (ldg % 8) || (ldx % 8) || n_groups < 1) return MM_ERR_SHAPE;
  if ((gcol_stride % 8) || (xcol_stride % 8) || gcol_stride < 0 || xcol_stride < 0) return MM_ERR_SHAPE;
  if (32ll * ldg * 2 + 1024 >= (1ll << 32) || 32ll * ldx * 2 + 1024 >= (1ll << 32)) return MM_ERR_SHAPE;
  if ((g_chunk_w <= 0 && Nn > ldg) || Kk > ldx) return MM_ERR_SHAPE;      // a group's columns (and the clamped reads past them) stay inside its rows
  if (g_chunk_w > 0 && ((g_chunk_w % 8) || g_chunk_w > ldg || (g_chunk_stride % 8) || g_chunk_stride < 0 ||
                        (256 / g_chunk_w + 2) * g_chunk_stride * 2 + 32ll * ldg * 2 >= (1ll << 32))) return MM_ERR_SHAPE;
  GemmTNArgs p = tn_args(G, ldg, X, ldx, dW, ldw, M, Nn, Kk);
  p.strideW = strideW;
  p.tiles_n = (Nn + 255) / 256; p.tiles_k = (Kk + 255) / 256;
  p.n_groups = n_groups; p.gcol_stride = gcol_stride; p.xcol_stride = xcol_stride;
  p.g_chunk_w = g_chunk_w; p.g_chunk_stride = g_chunk_stride;
  const long long ntile = (long long)p.tiles_n * p.tiles_k * n_groups;
  p.nsplit = tn_row_split(ntile, M);
  if (det && p.nsplit > 1) {
    // STAGED: every (group, range, tile) stores its partial tile, tn_reduce_det_kernel walks a group's ranges in order
    if (!scratch || ntile * p.nsplit * 65536 > scratch_floats) return MM_ERR_ARG;
    p.partial = scratch;
    const int chunk = det_plan::tn_chunk(M, p.nsplit);
    hipLaunchKernelGGL((gemm_tn4w_kernel<false, true>), dim3((unsigned)(ntile * p.nsplit)), dim3(256), 0, stream, p);
    TnReduceArgs q{scratch, nullptr, dW, nullptr, nullptr, strideW, 0, ldw, Nn, Kk, p.tiles_n, p.tiles_k, 0, p.nsplit, (M + chunk - 1) / chunk,
                   n_groups, 0, tn_vec_ok(dW, ldw, strideW) ? 1 : 0};
    hipLaunchKernelGGL(tn_reduce_det_kernel, dim3((unsigned)(ntile * 64)), dim3(256), 0, stream, q);
    tn_ran(TN_G4W, TN_B_COLG, true, p.nsplit);
    return mm_check_launch();
  }
  if (p.nsplit > 1) ++g_mm_nondet;
  hipLaunchKernelGGL((gemm_tn4w_kernel<false, true>), dim3((unsigned)(ntile * p.nsplit)), dim3(256), 0, stream, p);
  tn_ran(TN_G4W, TN_B_COLG, false, p.nsplit);
  return mm_check_launch();
}

extern "C" int medmoe_gemm_tn_cols(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, int M, int Nn, int Kk,
                                   int n_groups, long long gcol_stride, long long xcol_stride, long long strideW, int g_chunk_w,
                                   long long g_chunk_stride, hipStream_t stream) {
  return tn_cols_impl(G, ldg, X, ldx, dW, ldw, M, Nn, Kk, n_groups, gcol_stride, xcol_stride, strideW, g_chunk_w, g_chunk_stride, false,
                      nullptr, 0, stream);
}

// medmoe_gemm_tn_cols without order-dependent sums: with more than one row range per tile the partial tiles go through `scratch`
// (medmoe_gemm_tn_cols_det_scratch floats; the caller's, one per stream) and are summed in range order.
extern "C" int medmoe_gemm_tn_cols_det(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, int M, int Nn, int Kk,
                                       int n_groups, long long gcol_stride, long long xcol_stride, long long strideW, int g_chunk_w,
                                       long long g_chunk_stride, float* scratch, long long scratch_floats, hipStream_t stream) {
  return tn_cols_impl(G, ldg, X, ldx, dW, ldw, M, Nn, Kk, n_groups, gcol_stride, xcol_stride, strideW, g_chunk_w, g_chunk_stride, true,
                      scratch, scratch_floats, stream);
}

extern "C" long long medmoe_gemm_tn_cols_det_scratch(int M, int Nn, int Kk, int n_groups) {
  return det_plan::cols_scratch_floats(M, Nn, Kk, n_groups, g_tn_min_rows);
}

// dW[g][Nn][Nn] += A_g^T diag(w_g) A_g: weighted Gram products of the column blocks A_g = A + g*col_stride of one [M][lda] bf16 matrix,
// w_g[m] = w[g * w_gstride + m * w_ld] fp32 (every weight of rows 0..M-1 finite: it multiplies even all-zero rows).  The product
// w * A is rounded to bf16 before it is multiplied, as a stored copy would be.  fp32 atomics: zero dW first.  M % 32 == 0, Nn % 8 == 0.
// (The dGm of the GLoRIA local loss, sum over words of d2 a a^T per image, without the U = d2 * A matrix - losses.py:698-736 backward.)
static int tn_gram_impl(const void* A, int lda, const float* w, long long w_gstride, int w_ld, float* dW, int ldw, int M,
                        int Nn, int n_groups, long long col_stride, long long strideW, bool det, hipStream_t stream) {
  if (!A || !w || !dW) return MM_ERR_ARG;
  if (M < 32 || (M % 32) || Nn <= 0 || (Nn % 8) || (lda % 8) || n_groups < 1 || Nn > lda || w_ld < 1 || w_gstride < 0) return MM_ERR_SHAPE;
  if ((col_stride % 8) || col_stride < 0 || 32ll * lda * 2 + 1024 >= (1ll << 32) || 64ll * w_ld * 4 >= (1ll << 32)) return MM_ERR_SHAPE;
  GemmTNArgs p = tn_args(A, lda, A, lda, dW, ldw, M, Nn, Nn);
  p.strideW = strideW;
  p.tiles_n = (Nn + 255) / 256; p.tiles_k = p.tiles_n;
  p.n_groups = n_groups; p.gcol_stride = col_stride; p.xcol_stride = col_stride;
  p.gscale = w; p.gscale_gstride = w_gstride; p.gscale_ld = w_ld;
  const long long ntile = (long long)p.tiles_n * p.tiles_k * n_groups;
  p.nsplit = det ? 1 : tn_row_split(ntile, M);   // det: ONE workgroup adds to an output tile
  if (p.nsplit > 1) ++g_mm_nondet;
  hipLaunchKernelGGL((gemm_tn4w_kernel<false, true, true>), dim3((unsigned)(ntile * p.nsplit)), dim3(256), 0, stream, p);
  tn_ran(TN_G4W, TN_B_SCALE, false, p.nsplit);
  return mm_check_launch();
}

extern "C" int medmoe_gemm_tn_gram(const void* A, int lda, const float* w, long long w_gstride, int w_ld, float* dW, int ldw, int M,
                                   int Nn, int n_groups, long long col_stride, long long strideW, hipStream_t stream) {
  return tn_gram_impl(A, lda, w, w_gstride, w_ld, dW, ldw, M, Nn, n_groups, col_stride, strideW, false, stream);
}

// medmoe_gemm_tn_gram with a single writer per output tile (no split over the rows): the atomics of a tile all come from one workgroup,
// in program order.  The per-image Gram gradients are B groups of one tile: the groups fill the chip.
extern "C" int medmoe_gemm_tn_gram_det(const void* A, int lda, const float* w, long long w_gstride, int w_ld, float* dW, int ldw, int M,
                                       int Nn, int n_groups, long long col_stride, long long strideW, hipStream_t stream) {
  return tn_gram_impl(A, lda, w, w_gstride, w_ld, dW, ldw, M, Nn, n_groups, col_stride, strideW, true, stream);
}

// medmoe_gemm_tn without order-dependent sums (deterministic mode).  Shapes of the four-wave kernel - plain or ONE row-mapped operand or
// router groups (row_off), Kk % 256 == 0, Nn % 128 == 0 (plain: % 256), at least 2048 rows per group - run STAGED: every (range, tile)
// stores its partial tile and its column sums of G into `scratch`, tn_reduce_det_kernel adds a tile's ranges in range order (the ranges
// of a group are enumerated from row_off on the device by both kernels).  Every other shape runs gemm_tn_kernel with ONE workgroup per
// (group, tile).  scratch: medmoe_gemm_tn_det_scratch floats, the caller's, never shared by launches that may overlap (one per stream);
// too small is an error, not a fall-back.
extern "C" int medmoe_gemm_tn_det(const void* G, int ldg, const void* X, int ldx, float* dW, int ldw, float* db, int M, int Nn, int Kk,
                                  const int* x_rowmap, const int* g_rowmap, const int* row_off, int n_groups, long long strideW,
                                  long long strideDb, float* scratch, long long scratch_floats, hipStream_t stream) {
  if (!G || !X || !dW) return MM_ERR_ARG;
  if (M <= 0 || Nn <= 0 || Kk <= 0 || (Nn % 8) || (Kk % 8) || (ldg % 8) || (ldx % 8)) return MM_ERR_SHAPE;
  if (n_groups < 1 || (n_groups > 1 && !row_off)) return MM_ERR_ARG;
  GemmTNArgs p = tn_args(G, ldg, X, ldx, dW, ldw, M, Nn, Kk);
  p.db = db; p.x_rowmap = x_rowmap; p.g_rowmap = g_rowmap; p.row_off = row_off; p.strideW = strideW; p.strideDb = strideDb; p.n_groups = n_groups;
  const det_plan::TnPlan pl = det_plan::tn_plan(M, Nn, Kk, x_rowmap != nullptr, g_rowmap != nullptr, row_off != nullptr, n_groups,
                                               tn_fit32(M, ldg, ldx), g_tn_min_rows, g_tn_rows4w);
  if (pl.kind == det_plan::TN_SMALL) {
    tn128_launch(p, 1, stream);
    return mm_check_launch();
  }
  if (!scratch || pl.scratch_floats > scratch_floats) return MM_ERR_ARG;
  p.tiles_n = pl.tiles_n; p.tiles_k = pl.tiles_k; p.nsplit = pl.nsplit;
  const int ntile = pl.tiles_n * pl.tiles_k;
  p.partial = scratch;
  if (db) p.db_partial = scratch + (long long)pl.slots * 65536;
  TnReduceArgs q{scratch, p.db_partial, dW, db, row_off, strideW, strideDb, ldw, Nn, Kk, pl.tiles_n, pl.tiles_k, 0, pl.nsplit, pl.nvalid,
                 n_groups, 0, tn_vec_ok(dW, ldw, strideW) ? 1 : 0};
  if (pl.kind == det_plan::TN_PLAIN) hipLaunchKernelGGL(gemm_tn4w_kernel<false>, dim3(pl.slots), dim3(256), 0, stream, p);
  else {
    if (pl.kind == det_plan::TN_GROUPS) { q.mode = 1; q.R = pl.nsplit; }     // nsplit: the ROWS per range in this form
    hipLaunchKernelGGL(gemm_tn4w_kernel<true>, dim3(pl.slots), dim3(256), 0, stream, p);
  }
  hipLaunchKernelGGL(tn_reduce_det_kernel, dim3((unsigned)(n_groups * ntile * 64)), dim3(256), 0, stream, q);
  tn_ran(TN_G4W, pl.kind == det_plan::TN_PLAIN ? TN_B_PLAIN : TN_B_MAPPED, true, pl.nsplit);
  return mm_check_launch();
}

extern "C" long long medmoe_gemm_tn_det_scratch(int M, int Nn, int Kk, int x_mapped, int g_mapped, int grouped, int n_groups) {
  return det_plan::tn_plan(M, Nn, Kk, x_mapped != 0, g_mapped != 0, grouped != 0, n_groups, true, g_tn_min_rows, g_tn_rows4w).scratch_floats;
}
