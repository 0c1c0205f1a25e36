// MXFP8 (OCP Microscaling, e4m3 elements + one E8M0 scale byte per block of 32) expert weights on the CDNA4 block-scaled MFMA
// v_mfma_scale_f32_16x16x128_f8f6f4 (twice the rate of the bf16 / unscaled fp8 MFMA).  DESIGN.md "MXFP8 expert weights".
//
// The format.  A block is 32 consecutive elements along the contraction dimension of the product that reads the tensor.  With
// amax = max |v| over the block:  s = amax * (1/448) in fp32;  e = biased exponent of s, plus one if any mantissa bit of s is
// set (the scale is rounded UP to a power of two, so no element exceeds 448 and the saturating hardware convert equals
// torch.float8_e4m3fn everywhere), clamped to [1, 254]; amax == 0 gives e = 127.  The scale byte is e, the elements are
// rne_e4m3(v * 2^(127 - e)): a multiplication by a power of two, exact, so a torch twin is bit-exact by construction.
//
//   medmoe_quant_rows_mx     bf16 rows (optionally gathered) -> e4m3 [M][K] + scale bytes [M][K/32]
//   medmoe_quant_weights_mx  fp32 [G][N][K] -> e4m3 [G][N][K] + scales [G][N][K/32] (blocks along K: forward) and, quantised AGAIN with
//                            blocks along N, e4m3 [G][K][N] + scales [G][K][N/32] (dgrad).  The second copy is not a byte transpose of the first.
//   medmoe_gemm_mx_grouped   grouped NT product on the 128-row tile table of medmoe_dispatch, 128x128 tile per workgroup, k-step 128,
//                            operands staged global -> LDS by global_load_lds (16 B per lane) in a two-slot ring; epilogues of
//                            medmoe_gemm_fp8_grouped; optional second output of the ReLU epilogue: the tile MX-quantised along N.
//
// Operand layout of the MFMA, found by probing on the MI355X and pinned by tests/test_mxfp8_gpu.py::test_gemm_mx_layout_pin: with
// g = l >> 4, lane l holds TWO runs of 16 k bytes of row / column l & 15: k = 16 g .. 16 g + 15 in operand registers 0-3 and
// k = 64 + 16 g .. 64 + 16 g + 15 in registers 4-7.  Byte 0 (op_sel 0) of its scale register is the scale of that row's 32-block
// g, k = 32 g .. 32 g + 31 - which is NOT the data the lane itself holds (block g lives in registers 0-3 (g < 2) or 4-7 of lanes
// 2 (g & 1) and 2 (g & 1) + 1).  C/D: the standard 16x16 map, D[i = 4 (l >> 4) + r][j = l & 15].
#include "common.h"

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;
#define MX_DS_READ128(dst, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(imm))

__device__ __forceinline__ uint32_t mx_cvt4_e4m3(float a, float b, float c, float d) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);      // bytes 0, 1 (round to nearest even, saturating)
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);       // bytes 2, 3
  return (uint32_t)w;
}
// E8M0 byte of a block: integer operations on the bits of s = amax / 448
__device__ __forceinline__ int mx_scale_byte(float amax) {
  if (!(amax > 0.f)) return 127;
  const uint32_t b = __float_as_uint(amax * (1.f / 448.f));
  const int e = (int)((b >> 23) & 0xffu) + ((b & 0x7fffffu) ? 1 : 0);
  return min(max(e, 1), 254);
}
// 2^(127 - e) as a float (e = 254: the subnormal 2^-127)
__device__ __forceinline__ float mx_inv_scale(int e) { return __uint_as_float(e < 254 ? (uint32_t)(254 - e) << 23 : 0x00400000u); }

// one wave per row, 8 elements per lane and pass: a 32-block is 4 neighbouring lanes.  K % 32 == 0.
__global__ __launch_bounds__(256) void quant_rows_mx_kernel(const bf16_t* __restrict__ x, int ldx, const int* __restrict__ rowmap,
                                                            uint8_t* __restrict__ q, uint8_t* __restrict__ s, int M, int K) {
  const int lane = threadIdx.x & 63;
  const int nb = K >> 5;
  for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += gridDim.x * 4) {
    const bf16_t* xr = x + (long long)(rowmap ? rowmap[row] : row) * ldx;
    for (int c0 = 0; c0 < K; c0 += 512) {                    // wave-uniform trip count: every lane takes part in the shuffles
      const int c = c0 + lane * 8;
      const bool in = c < K;                                 // K % 32 == 0: the 4 lanes of a block are in or out together
      const uint4 v = in ? *(const uint4*)(xr + c) : make_uint4(0u, 0u, 0u, 0u);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      float f[8];
      float amax = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f[2 * e] = __uint_as_float(w[e] << 16); f[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
        amax = fmaxf(amax, fmaxf(fabsf(f[2 * e]), fabsf(f[2 * e + 1])));
      }
      amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
      const int eb = mx_scale_byte(amax);
      const float inv = mx_inv_scale(eb);
      if (in) {
        uint2 o;
        o.x = mx_cvt4_e4m3(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
        o.y = mx_cvt4_e4m3(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
        *(uint2*)(q + (long long)row * K + c) = o;
        if ((lane & 3) == 0) s[(long long)row * nb + (c >> 5)] = (uint8_t)eb;
      }
    }
  }
}

extern "C" int medmoe_quant_rows_mx(const void* x, int ldx, const int* rowmap, void* q, void* s, int M, int K, hipStream_t stream) {
  if (!x || !q || !s) return MM_ERR_ARG;
  if (M <= 0 || K <= 0 || (K % 32) || (ldx % 8)) return MM_ERR_SHAPE;
  const int grid = min((M + 3) / 4, 256 * 16);
  hipLaunchKernelGGL(quant_rows_mx_kernel, dim3(grid), dim3(256), 0, stream, (const bf16_t*)x, ldx, rowmap, (uint8_t*)q, (uint8_t*)s, M, K);
  return mm_check_launch();
}

// one workgroup per 32 x 32 block (n, k) of one group: the block's 32 row scales (along k) and 32 column scales (along n)
__global__ __launch_bounds__(256) void quant_weights_mx_kernel(const float* __restrict__ w, uint8_t* __restrict__ q, uint8_t* __restrict__ sq,
                                                               uint8_t* __restrict__ qT, uint8_t* __restrict__ sT, int N, int K) {
  __shared__ float t[32][33];
  __shared__ int er[32], ec[32];
  const int tid = threadIdx.x;
  const int kb = blockIdx.x, nb = blockIdx.y, g = blockIdx.z;
  const int k0 = kb * 32, n0 = nb * 32;
  const int r = tid >> 3, c = (tid & 7) * 4;
  {
    const float4 v = *(const float4*)(w + ((long long)g * N + n0 + r) * K + k0 + c);
    t[r][c] = v.x; t[r][c + 1] = v.y; t[r][c + 2] = v.z; t[r][c + 3] = v.w;
  }
  __syncthreads();
  if (tid < 64) {
    const int i = tid & 31;
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(tid < 32 ? t[i][j] : t[j][i]));
    const int e = mx_scale_byte(amax);
    if (tid < 32) { er[i] = e; sq[((long long)g * N + n0 + i) * (K >> 5) + kb] = (uint8_t)e; }
    else { ec[i] = e; sT[((long long)g * K + k0 + i) * (N >> 5) + nb] = (uint8_t)e; }
  }
  __syncthreads();
  {
    const float inv = mx_inv_scale(er[r]);
    *(uint32_t*)(q + ((long long)g * N + n0 + r) * K + k0 + c) = mx_cvt4_e4m3(t[r][c] * inv, t[r][c + 1] * inv, t[r][c + 2] * inv, t[r][c + 3] * inv);
  }
  {
    const float inv = mx_inv_scale(ec[r]);                   // r = k within the block, c = first of 4 consecutive n
    *(uint32_t*)(qT + ((long long)g * K + k0 + r) * N + n0 + c) = mx_cvt4_e4m3(t[c][r] * inv, t[c + 1][r] * inv, t[c + 2][r] * inv, t[c + 3][r] * inv);
  }
}

extern "C" int medmoe_quant_weights_mx(const float* w, void* q, void* sq, void* qT, void* sT, int G, int N, int K, hipStream_t stream) {
  if (!w || !q || !sq || !qT || !sT) return MM_ERR_ARG;
  if (G <= 0 || N <= 0 || K <= 0 || (K % 32) || (N % 32) || G > 65535 || N / 32 > 65535) return MM_ERR_SHAPE;
  hipLaunchKernelGGL(quant_weights_mx_kernel, dim3(K / 32, N / 32, G), dim3(256), 0, stream, w, (uint8_t*)q, (uint8_t*)sq, (uint8_t*)qT,
                     (uint8_t*)sT, N, K);
  return mm_check_launch();
}

// ---------------------------------------------------------------------------------------------
// grouped MX GEMM on the 128-row tile table of medmoe_dispatch: tiles[t] = {group, m0, m_end, -}
// ---------------------------------------------------------------------------------------------
#define MX_BM 128
#define MX_BN 128
#define MX_BK 128                                  // one 16x16x128 MFMA per 16 x 16 tile and k-step; a row of a stage is 128 bytes
#define MX_STAGE ((MX_BM + MX_BN) * MX_BK)         // 32 KB: A rows, then B rows
#define MX_EPI_RELU 1                              // relu(acc + bias)
#define MX_EPI_MUL_DRELU 2                         // (acc + residual) * (aux > 0)

struct GemmMxArgs {
  const uint8_t* A; const uint8_t* sa; const uint8_t* B; const uint8_t* sb; const float* bias;
  bf16_t* C; const bf16_t* residual; const bf16_t* aux; uint8_t* Cq; uint8_t* Csq; const int* tiles; const int* tile_count;
  int N, K, ldc, epi;
  long long strideB, strideSb, strideBias;
};

__global__ __launch_bounds__(256) void gemm_mx_grouped_kernel(GemmMxArgs p) {
  // two ring slots of 32 KB: two workgroups per CU, so one's epilogue runs under the other's k loop
  __shared__ __attribute__((aligned(128))) char smem[2 * MX_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: LDS-DMA bases stay scalar
  const int fr = lane & 15, g = lane >> 4;
  const int wm = wid & 1, wn = wid >> 1;                       // 2 x 2 waves of 64 x 64
  const int tiles_n = (p.N + MX_BN - 1) / MX_BN;
  const int n_tiles = p.tile_count[0];
  const int id = blockIdx.x;
  const int ti = id / tiles_n, tn_ = id - ti * tiles_n;
  if (ti >= n_tiles) return;
  const int group = p.tiles[ti * 4], m0 = p.tiles[ti * 4 + 1], m_end = p.tiles[ti * 4 + 2];
  const int n0 = tn_ * MX_BN;
  const int nb = p.K >> 5;                                     // scale bytes per row
  const uint8_t* Bg = p.B + (long long)group * p.strideB;
  const uint8_t* sbg = p.sb + (long long)group * p.strideSb;

  // DMA: one wave-instruction writes 1 KB = 8 rows of 128 B, lane t -> row t >> 3, 16-byte slot t & 7, which holds the row's
  // chunk (t & 7) ^ (row & 7) (the XOR swizzle goes on the SOURCE address; the LDS image of a wave-instruction is lane-linear).
  // Piece j (0..3) of wave w covers rows (4 j + w) * 8 .. + 7 of an operand.  Rows past the group's end / past N: clamped copies.
  const int chunk = ((lane & 7) ^ (lane >> 3)) * 16;
  const uint8_t* srcA[4]; const uint8_t* srcB[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (4 * j + wid) * 8 + (lane >> 3);
    srcA[j] = p.A + (long long)min(m0 + row, m_end - 1) * p.K;
    srcB[j] = Bg + (long long)min(n0 + row, p.N - 1) * p.K;
  }
  auto issue = [&](int kt) __attribute__((always_inline)) {
    // K % 32 == 0: a 16-byte piece is inside K or past it, never across.  A piece past K (last k-step of a K that is no
    // multiple of 128) re-reads the row's first piece - valid memory; the fragments of those 32-blocks are zeroed after the read.
    const int ko = kt * MX_BK + chunk < p.K ? kt * MX_BK + chunk : 0;
    char* sl = smem + (kt & 1) * MX_STAGE + wid * 1024;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      __builtin_amdgcn_global_load_lds(GLB_PTR(srcA[j] + ko), LDS_PTR(sl + j * 4096), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(GLB_PTR(srcB[j] + ko), LDS_PTR(sl + MX_BM * MX_BK + j * 4096), 16, 0, 0);
    }
  };
  // the scale bytes this lane supplies: row wm * 64 + 16 t + fr of A, wn * 64 + 16 t + fr of B, 32-block 4 kt + g of the k-step
  const uint8_t* psa[4]; const uint8_t* psb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    psa[t] = p.sa + (long long)min(m0 + wm * 64 + t * 16 + fr, m_end - 1) * nb + g;
    psb[t] = sbg + (long long)min(n0 + wn * 64 + t * 16 + fr, p.N - 1) * nb + g;
  }
  int sa_n[4], sb_n[4];
  auto load_scales = [&](int kt) __attribute__((always_inline)) {
    const bool in = kt * 4 + g < nb;
#pragma unroll
    for (int t = 0; t < 4; ++t) { sa_n[t] = in ? psa[t][kt * 4] : 127; sb_n[t] = in ? psb[t][kt * 4] : 127; }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int nk = (p.K + MX_BK - 1) / MX_BK;
  // fragment of row 16 t + fr: bytes 16 g .. + 15 (chunk g) and 64 + 16 g .. + 15 (chunk 4 + g), at slots g ^ (fr & 7) and that ^ 4
  const int offA = (wm * 64 + fr) * 128 + ((g ^ (fr & 7)) << 4);
  const int offB = MX_BM * MX_BK + (wn * 64 + fr) * 128 + ((g ^ (fr & 7)) << 4);
  const unsigned lds0 = (unsigned)(size_t)smem;                // LDS byte address of ring slot 0
  issue(0);
  load_scales(0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of stage kt (and its scale bytes) have landed
    __builtin_amdgcn_s_barrier();                              // ... every wave's; and every wave is done reading the other slot
    asm volatile("" ::: "memory");
    int sa_c[4], sb_c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { sa_c[t] = sa_n[t]; sb_c[t] = sb_n[t]; }
    if (kt + 1 < nk) { issue(kt + 1); load_scales(kt + 1); }
    // fragment reads as inline ds_read_b128 (as gemm_nt4w): through plain LDS loads the compiler drains the DMA just issued
    // (vmcnt(0)) before the first read, which serialises the ring
    const unsigned sl = lds0 + (kt & 1) * MX_STAGE;
    i32x4_t a0[4], a1[4], b0[4], b1[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      MX_DS_READ128(a0[t], sl + offA, t * 2048); MX_DS_READ128(a1[t], sl + (offA ^ 64), t * 2048);
      MX_DS_READ128(b0[t], sl + offB, t * 2048); MX_DS_READ128(b1[t], sl + (offB ^ 64), t * 2048);
    }
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a0[0]), "+v"(a0[1]), "+v"(a0[2]), "+v"(a0[3]), "+v"(a1[0]), "+v"(a1[1]), "+v"(a1[2]), "+v"(a1[3]),
                   "+v"(b0[0]), "+v"(b0[1]), "+v"(b0[2]), "+v"(b0[3]), "+v"(b1[0]), "+v"(b1[1]), "+v"(b1[2]), "+v"(b1[3]));
    if (kt * 4 + 4 > nb) {                                     // last k-step of a K that is no multiple of 128: zero elements past K
      const bool z0 = kt * 4 + (g >> 1) >= nb, z1 = kt * 4 + 2 + (g >> 1) >= nb;      // the 32-blocks of the lane's two runs
      const i32x4_t zero = {0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a0[t] = z0 ? zero : a0[t]; b0[t] = z0 ? zero : b0[t];
        a1[t] = z1 ? zero : a1[t]; b1[t] = z1 ? zero : b1[t];
      }
    }
    i32x8_t af[4], bf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      af[t] = __builtin_shufflevector(a0[t], a1[t], 0, 1, 2, 3, 4, 5, 6, 7);
      bf[t] = __builtin_shufflevector(b0[t], b1[t], 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn)        // D[i = n][j = m]: lane holds row m = fr of the tile, columns n = 4g + r; formats 0 = e4m3
        acc[tm][tn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[tn], af[tm], acc[tm][tn], 0, 0, 0, sb_c[tn], 0, sa_c[tm]);
  }
  // epilogue
  const float* bg = p.bias ? p.bias + (long long)group * p.strideBias : nullptr;
#pragma unroll
  for (int tm = 0; tm < 4; ++tm) {
    const int m = m0 + wm * 64 + tm * 16 + fr;
    const bool mok = m < m_end;                                // the 4 lanes that share a row agree: the shuffles below stay inside them
    uint2 pk[4];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int n = n0 + wn * 64 + tn * 16 + g * 4;
      const bool ok = mok && n < p.N;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[tm][tn][r] + ((bg && ok) ? bg[n + r] : 0.f);
      const long long o = (long long)m * p.ldc + n;
      if (p.epi == MX_EPI_RELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      } else if (p.epi == MX_EPI_MUL_DRELU) {
        const uint2 rs = (p.residual && ok) ? *(const uint2*)(p.residual + o) : make_uint2(0u, 0u);
        const uint2 ax = ok ? *(const uint2*)(p.aux + o) : make_uint2(0u, 0u);
        const float res[4] = {__uint_as_float(rs.x << 16), __uint_as_float(rs.x & 0xffff0000u), __uint_as_float(rs.y << 16), __uint_as_float(rs.y & 0xffff0000u)};
        const float au[4] = {__uint_as_float(ax.x << 16), __uint_as_float(ax.x & 0xffff0000u), __uint_as_float(ax.y << 16), __uint_as_float(ax.y & 0xffff0000u)};
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = au[r] > 0.f ? v[r] + res[r] : 0.f;
      }
      pk[tn].x = pack2bf(v[0], v[1]); pk[tn].y = pack2bf(v[2], v[3]);
      if (ok) *(uint2*)(p.C + o) = pk[tn];
    }
    if (p.Cq) {
      // second output: the bf16-ROUNDED row MX-quantised along n (= medmoe_quant_rows_mx of C).  A 32-block of row m is the
      // tn pair (2h, 2h + 1) over the 4 lanes g = 0..3 of that row (lanes fr, fr + 16, fr + 32, fr + 48).
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float f[8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const uint2 w = pk[2 * h + u];
          f[4 * u] = __uint_as_float(w.x << 16); f[4 * u + 1] = __uint_as_float(w.x & 0xffff0000u);
          f[4 * u + 2] = __uint_as_float(w.y << 16); f[4 * u + 3] = __uint_as_float(w.y & 0xffff0000u);
        }
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
        amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
        const int eb = mx_scale_byte(amax);
        const float inv = mx_inv_scale(eb);
        const int nblk = n0 + wn * 64 + h * 32;
        if (mok && nblk < p.N) {                               // N % 32 == 0 (host check): a block is inside N or past it
          uint8_t* qr = p.Cq + (long long)m * p.N + nblk + g * 4;
          *(uint32_t*)qr = mx_cvt4_e4m3(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
          *(uint32_t*)(qr + 16) = mx_cvt4_e4m3(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
          if (g == 0) p.Csq[(long long)m * (p.N >> 5) + (nblk >> 5)] = (uint8_t)eb;
        }
      }
    }
  }
}

extern "C" int medmoe_gemm_mx_grouped(const void* Aq, const void* sa, const void* Bq, const void* sb, const float* bias, void* C, int ldc,
                                      const void* residual, const void* aux, void* Cq, void* Csq, const int* tiles, const int* tile_count,
                                      int max_tiles, int N, int K, long long strideB, long long strideSb, long long strideBias, int epi,
                                      hipStream_t stream) {
  if (!Aq || !sa || !Bq || !sb || !C || !tiles || !tile_count || max_tiles <= 0) return MM_ERR_ARG;
  if (N <= 0 || K <= 0 || (K % 32) || (N % 4) || (ldc % 4)) return MM_ERR_SHAPE;
  if (epi < 0 || epi > MX_EPI_MUL_DRELU || (epi == MX_EPI_MUL_DRELU && !aux)) return MM_ERR_ARG;
  if ((Cq != nullptr) != (Csq != nullptr) || (Cq && epi != MX_EPI_RELU)) return MM_ERR_ARG;
  if (Cq && (N % 32)) return MM_ERR_SHAPE;
  GemmMxArgs p;
  p.A = (const uint8_t*)Aq; p.sa = (const uint8_t*)sa; p.B = (const uint8_t*)Bq; p.sb = (const uint8_t*)sb; p.bias = bias; p.C = (bf16_t*)C;
  p.residual = (const bf16_t*)residual; p.aux = (const bf16_t*)aux; p.Cq = (uint8_t*)Cq; p.Csq = (uint8_t*)Csq; p.tiles = tiles;
  p.tile_count = tile_count; p.N = N; p.K = K; p.ldc = ldc; p.epi = epi; p.strideB = strideB; p.strideSb = strideSb; p.strideBias = strideBias;
  const int tiles_n = (N + MX_BN - 1) / MX_BN;
  hipLaunchKernelGGL(gemm_mx_grouped_kernel, dim3(max_tiles * tiles_n), dim3(256), 0, stream, p);
  return mm_check_launch();
}
