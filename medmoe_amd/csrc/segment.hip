// Semantic segmentation on the region features: a linear decoder with independent sigmoids per class, its bilinear upsample to
// the mask size, BCE + batch-Dice loss, the backward of all of it and the pixel counts of Dice / IoU.  Nothing of the shape [B][C][H][W] is
// stored in fp32: the full-resolution logit zf of a pixel is recomputed from the patch logits z wherever it is needed.  No fp32 atomic:
// every sum leaves as per-workgroup records (plain stores) that a second launch adds in index order, so two runs give the same bits and
// medmoe_nondet_launches() never moves.
//
//   medmoe_seg_head_fwd   seg_row_kernel: a wave holds 4 rows of the bf16 features in registers (16 bytes per lane and load), W [C][D] sits in
//                         LDS, one wave reduction per class; z fp32 [N][C]
//   medmoe_seg_loss       seg_stats_kernel: workgroup = (plane (b, c), tile of the plane); the plane's g x g patch logits sit in LDS, a thread
//                         takes 16 pixels of a mask row at a time (one 16-byte load where W % 16 == 0) and the workgroup stores ONE record
//                         (BCE sum, I, P, T | n_valid, TP, FP, FN);
//                         seg_finish_kernel: one workgroup adds the records per class in index order (double / int64), forms the loss and
//                         the per-class coefficients of d loss / d zf;
//                         seg_grad_kernel: the adjoint of the upsample in GATHER form - a wave owns a (patch, class), walks the patch's
//                         support (seg_plan.h: a contiguous pixel range per axis) in a fixed order, recomputes zf and d loss / d zf per pixel
//                         and stores dz[patch][c]
//   medmoe_seg_head_bwd   seg_dfeat_kernel: dfeat = dz W, WRITTEN as bf16; seg_wgrad_kernel + seg_wgrad_sum_kernel: dW = dz^T feat and db = sum dz
//                         as records per row range, added into the gradient buffers in range order (the form of DESIGN 3e / 3p)
//   medmoe_seg_predict    seg_predict_kernel: masks uint8 [B][C][H][W] = (zf > 0), optionally zf itself
#include "common.h"
#include "medmoe_hip.h"
#include "seg_plan.h"

namespace {

constexpr int MAXC = 8;                        // classes
constexpr int MAX_G = 64;                      // patches per axis: a plane of g x g patch logits is at most 16 KiB of LDS
constexpr int MAX_D = 2048;
constexpr int RW = 4;                          // rows a wave of the row pass holds at a time
constexpr int PX = 16;                         // pixels of a unit: one 16-byte mask load
constexpr int UNITS = 4;                       // units a thread of the stats / predict pass walks
constexpr int REC = 8;                         // 4-byte slots of a stats record: 4 floats, 4 ints
constexpr int FIN = 32;                        // floats of the finished coefficients: [0] BCE, [1 + 2c] / [2 + 2c] the Dice pair of class c
constexpr int MAX_RECORDS = 256;               // row ranges of the staged dW / db
constexpr int REC_PAD = 64;                    // floats behind a wgrad record's [C][D]: the C sums of dz

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void unpack8(uint4 v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// row pass: z[row][c] = <feat[row], W_c> + b_c.  J: 16-byte loads per lane and row (D <= 512 J); a lane owns the columns 512 j + 8 lane.
// ---------------------------------------------------------------------------------------------------------------------------------------------
template <int J>
__global__ __launch_bounds__(256) void seg_row_kernel(const bf16_t* __restrict__ feat, const float* __restrict__ W, const float* __restrict__ b,
                                                      float* __restrict__ z, int N, int D, int C) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid * 4; i < C * D; i += 1024) *(float4*)(wl + i) = *(const float4*)(W + i);
  __syncthreads();
  const float bias = lane < C ? b[lane] : 0.f;
  const int ngroups = (N + 4 * RW - 1) / (4 * RW);
  for (int gi = blockIdx.x; gi < ngroups; gi += gridDim.x) {
    const int r0 = gi * 4 * RW + wave * RW;
    uint4 xv[RW][J];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int j = 0; j < J; ++j) {
        // issued unconditionally from a clamped address: a row past N repeats row N - 1 and is dropped below, a column past D repeats
        // the row's first columns and meets a zero of W
        const int col = 512 * j + 8 * lane;
        xv[r][j] = *(const uint4*)(feat + (long long)min(r0 + r, N - 1) * D + (col < D ? col : 0));
      }
    float zr[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) zr[r] = bias;
    for (int c = 0; c < C; ++c) {
      float w[J][8];
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int col = 512 * j + 8 * lane;
        const float m = col < D ? 1.f : 0.f;
        const float4 w0 = *(const float4*)(wl + c * D + (col < D ? col : 0)), w1 = *(const float4*)(wl + c * D + (col < D ? col : 0) + 4);
        w[j][0] = w0.x * m; w[j][1] = w0.y * m; w[j][2] = w0.z * m; w[j][3] = w0.w * m;
        w[j][4] = w1.x * m; w[j][5] = w1.y * m; w[j][6] = w1.z * m; w[j][7] = w1.w * m;
      }
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
          float f[8];
          unpack8(xv[r][j], f);
#pragma unroll
          for (int k = 0; k < 8; ++k) p += f[k] * w[j][k];
        }
        p = wave_sum(p);
        if (lane == c) zr[r] += p;
      }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r)
      if (r0 + r < N && lane < C) z[(long long)(r0 + r) * C + lane] = zr[r];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// per-pixel pieces
// ---------------------------------------------------------------------------------------------------------------------------------------------
// the bilinear read of a plane of g x g patch logits in LDS, in the operation order of torch's upsample_bilinear2d
// and with contraction to fused multiply-adds switched off: the stats, gradient and predict kernels inline this, and the counts of one must
// agree with the masks of another by construction, not by the compiler contracting the expression alike three times
__device__ __forceinline__ float zf_at(const float* zl, int g, SegSrc sy, SegSrc sx) {
#pragma clang fp contract(off)
  const float a = zl[sy.i0 * g + sx.i0], b = zl[sy.i0 * g + sx.i1], c = zl[sy.i1 * g + sx.i0], d = zl[sy.i1 * g + sx.i1];
  const float w1x = sx.lam, w0x = 1.f - w1x, w1y = sy.lam, w0y = 1.f - w1y;
  return w0y * (w0x * a + w1x * b) + w1y * (w0x * c + w1x * d);
}

struct Sig {
  float sp, sn, sg, sgn;                       // softplus(z), softplus(-z), sigmoid(z), sigmoid(-z): the stable forms
};
__device__ __forceinline__ Sig sig_of(float zf) {
  const float e = expf(-fabsf(zf)), l1p = log1pf(e);
  const float hi = 1.f / (1.f + e), lo = e / (1.f + e);
  Sig s;
  s.sp = fmaxf(zf, 0.f) + l1p;
  s.sn = fmaxf(-zf, 0.f) + l1p;
  s.sg = zf >= 0.f ? hi : lo;
  s.sgn = zf >= 0.f ? lo : hi;
  return s;
}

__device__ __forceinline__ void stage_plane(float* zl, const float* __restrict__ z, long long b, int c, int P, int C) {
  for (int i = threadIdx.x; i < P; i += 256) zl[i] = z[(b * P + i) * C + c];
  __syncthreads();
}

// the unit u of a plane: 16 pixels of row y from x0 on, n of them inside the row
struct Unit {
  int y, x0, n;
};
__device__ __forceinline__ Unit unit_of(int u, int nchunk, int Wd) {
  Unit q;
  q.y = u / nchunk;
  q.x0 = (u - q.y * nchunk) * PX;
  q.n = min(PX, Wd - q.x0);
  return q;
}

// the unit's 16 mask bytes in four words, a byte past the row reading -1 (ignored)
__device__ __forceinline__ uint4 load_mask16(const signed char* __restrict__ row, Unit q, bool wide) {
  if (wide) return *(const uint4*)(row + q.x0);
  unsigned w[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
#pragma unroll
  for (int k = 0; k < PX; ++k)
    if (k < q.n) w[k >> 2] = (w[k >> 2] & ~(0xffu << (8 * (k & 3)))) | ((unsigned)(unsigned char)row[q.x0 + k] << (8 * (k & 3)));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// stats pass: record[blockIdx.x] = (BCE sum, I, P, T | n_valid, TP, FP, FN) over the tile's pixels of plane (b, c)
// ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_stats_kernel(const float* __restrict__ z, const signed char* __restrict__ masks,
                                                        const float* __restrict__ pos_weight, float* __restrict__ rec, int g, int H, int Wd,
                                                        int C, int tiles) {
  __shared__ float zl[MAX_G * MAX_G];
  __shared__ float redf[4][4];
  __shared__ int redi[4][4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long plane = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles, c = (int)(plane % C);
  stage_plane(zl, z, plane / C, c, g * g, C);
  const float pw = pos_weight ? pos_weight[c] : 1.f;
  const float sy_scale = seg_scale(g, H), sx_scale = seg_scale(g, Wd);
  const int nchunk = (Wd + PX - 1) / PX, nunits = H * nchunk;
  const bool wide = Wd % PX == 0;
  float bce = 0.f, si = 0.f, sp = 0.f, st = 0.f;
  int nv = 0, tp = 0, fp = 0, fn = 0;
  for (int k = 0; k < UNITS; ++k) {
    const int u = (tile * UNITS + k) * 256 + tid;
    if (u >= nunits) break;
    const Unit q = unit_of(u, nchunk, Wd);
    const uint4 mw = load_mask16(masks + (plane * H + q.y) * Wd, q, wide);
    const unsigned words[4] = {mw.x, mw.y, mw.z, mw.w};
    const SegSrc sy = seg_src(q.y, sy_scale, g);
#pragma unroll
    for (int p = 0; p < PX; ++p) {
      const int t = (int)(signed char)(words[p >> 2] >> (8 * (p & 3)));
      const float zf = zf_at(zl, g, sy, seg_src(q.x0 + p, sx_scale, g));
      const Sig s = sig_of(zf);
      const bool on = t >= 0, pos = t > 0, pred = zf > 0.f;
      const float tf = pos ? 1.f : 0.f;
      bce += on ? pw * tf * s.sn + (1.f - tf) * s.sp : 0.f;
      sp += on ? s.sg : 0.f;
      si += on && pos ? s.sg : 0.f;
      st += on ? tf : 0.f;
      nv += on;
      tp += on && pos && pred;
      fp += on && !pos && pred;
      fn += on && pos && !pred;
    }
  }
  bce = wave_sum(bce); si = wave_sum(si); sp = wave_sum(sp); st = wave_sum(st);
  nv = wave_sum_i(nv); tp = wave_sum_i(tp); fp = wave_sum_i(fp); fn = wave_sum_i(fn);
  if (lane == 0) {
    redf[wave][0] = bce; redf[wave][1] = si; redf[wave][2] = sp; redf[wave][3] = st;
    redi[wave][0] = nv; redi[wave][1] = tp; redi[wave][2] = fp; redi[wave][3] = fn;
  }
  __syncthreads();
  if (tid < 4) {                                               // slot tid of the record: the four waves in wave order
    float* out = rec + (long long)blockIdx.x * REC;
    out[tid] = ((redf[0][tid] + redf[1][tid]) + redf[2][tid]) + redf[3][tid];
    ((int*)out)[4 + tid] = redi[0][tid] + redi[1][tid] + redi[2][tid] + redi[3][tid];
  }
}

// One workgroup: per class the B x tiles records added in index order (thread t takes records t, t + 256, ..., then a fixed tree), the counts
// to counts[c][0..3] = (n_valid, TP, FP, FN), then thread 0 forms the loss and the coefficients of the gradient pass:
//   d loss / d zf = fin[0] ((1 - t) p - pw t (1 - p)) + (fin[1 + 2c] t + fin[2 + 2c]) p (1 - p)     for a valid pixel of class c
__global__ __launch_bounds__(256) void seg_finish_kernel(const float* __restrict__ rec, long long* __restrict__ counts, float* __restrict__ loss,
                                                         float* __restrict__ fin, int B, int C, int tiles, float w_bce, float w_dice, float eps,
                                                         float loss_scale) {
  __shared__ double sd[256][4];
  __shared__ long long sl[256][4];
  __shared__ double totd[MAXC][4];
  __shared__ long long totl[MAXC][4];
  const int tid = threadIdx.x;
  const long long per = (long long)B * tiles;
  for (int c = 0; c < C; ++c) {
    double a[4] = {0., 0., 0., 0.};
    long long n[4] = {0, 0, 0, 0};
    for (long long r = tid; r < per; r += 256) {
      const float* q = rec + (((r / tiles) * C + c) * tiles + r % tiles) * REC;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k] += (double)q[k];
        n[k] += ((const int*)q)[4 + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { sd[tid][k] = a[k]; sl[tid][k] = n[k]; }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o)
#pragma unroll
        for (int k = 0; k < 4; ++k) { sd[tid][k] += sd[tid + o][k]; sl[tid][k] += sl[tid + o][k]; }
      __syncthreads();
    }
    if (tid < 4) {
      totd[c][tid] = sd[0][tid];
      totl[c][tid] = sl[0][tid];
      counts[4 * c + tid] = sl[0][tid];
    }
    __syncthreads();
  }
  if (tid == 0) {
    long long K = 0;
    int cv = 0;
    double bce = 0.;
    for (int c = 0; c < C; ++c) {
      K += totl[c][0];
      cv += totl[c][0] > 0;
      bce += totd[c][0];
    }
    for (int i = 0; i < FIN; ++i) fin[i] = 0.f;
    double L = 0.;
    if (K > 0) {
      const double s = (double)loss_scale;
      double dice = 0.;
      for (int c = 0; c < C; ++c) {
        if (totl[c][0] == 0) continue;
        const double I = totd[c][1], U = totd[c][2] + totd[c][3] + (double)eps;
        if (!(U > 0.)) continue;                                // eps = 0 and every probability underflowed: the class adds nothing
        dice += (2. * I + (double)eps) / U;
        fin[1 + 2 * c] = (float)(-s * (double)w_dice / cv * 2. / U);
        fin[2 + 2 * c] = (float)(s * (double)w_dice / cv * (2. * I + (double)eps) / (U * U));
      }
      fin[0] = (float)(s * (double)w_bce / (double)K);
      L = s * ((double)w_bce * bce / (double)K + (double)w_dice * (1. - dice / cv));
    }
    loss[0] = (float)L;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// gradient pass, gather form: wave = (patch, plane); dz[b][patch][c] = sum over the patch's support of wy wx d loss / d zf
// ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_grad_kernel(const float* __restrict__ z, const signed char* __restrict__ masks,
                                                       const float* __restrict__ pos_weight, const float* __restrict__ fin,
                                                       float* __restrict__ dz, int g, int H, int Wd, int C, int groups) {
  __shared__ float zl[MAX_G * MAX_G];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long plane = blockIdx.x / groups;
  const int P = g * g, patch = (blockIdx.x % groups) * 4 + wave, c = (int)(plane % C);
  stage_plane(zl, z, plane / C, c, P, C);
  if (patch >= P) return;                                       // wave-uniform, after the only barrier
  const float pw = pos_weight ? pos_weight[c] : 1.f, kb = fin[0], ka = fin[1 + 2 * c], kc = fin[2 + 2 * c];
  const float sy_scale = seg_scale(g, H), sx_scale = seg_scale(g, Wd);
  const int i = patch / g, j = patch - i * g;
  int ylo, yhi, xlo, xhi;
  seg_support(i, g, H, &ylo, &yhi);
  seg_support(j, g, Wd, &xlo, &xhi);
  const int ws = xhi - xlo, npx = (yhi - ylo) * ws;
  const signed char* mp = masks + plane * H * Wd;
  float acc = 0.f;
  for (int k = lane; k < npx; k += 64) {                        // a lane's pixels in a fixed order, then the wave's lanes in a fixed tree
    const int dy = k / ws, yy = ylo + dy, xx = xlo + (k - dy * ws);
    const int t = (int)mp[(long long)yy * Wd + xx];
    const SegSrc sy = seg_src(yy, sy_scale, g), sx = seg_src(xx, sx_scale, g);
    const Sig s = sig_of(zf_at(zl, g, sy, sx));
    const float tf = t > 0 ? 1.f : 0.f;
    const float d = kb * ((1.f - tf) * s.sg - pw * tf * s.sgn) + (ka * tf + kc) * (s.sg * s.sgn);
    acc += t >= 0 ? seg_weight(sy, i) * seg_weight(sx, j) * d : 0.f;
  }
  acc = wave_sum(acc);
  if (lane == 0) dz[((plane / C) * P + patch) * C + c] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// predict: masks[b][c][y][x] = zf > 0 (and zf itself when asked for)
// ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_predict_kernel(const float* __restrict__ z, unsigned char* __restrict__ out, float* __restrict__ zf_out,
                                                          int g, int H, int Wd, int C, int tiles) {
  __shared__ float zl[MAX_G * MAX_G];
  const int tid = threadIdx.x;
  const long long plane = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  stage_plane(zl, z, plane / C, (int)(plane % C), g * g, C);
  const float sy_scale = seg_scale(g, H), sx_scale = seg_scale(g, Wd);
  const int nchunk = (Wd + PX - 1) / PX, nunits = H * nchunk;
  const bool wide = Wd % PX == 0;
  for (int k = 0; k < UNITS; ++k) {
    const int u = (tile * UNITS + k) * 256 + tid;
    if (u >= nunits) break;
    const Unit q = unit_of(u, nchunk, Wd);
    const SegSrc sy = seg_src(q.y, sy_scale, g);
    const long long base = (plane * H + q.y) * Wd + q.x0;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int p = 0; p < PX; ++p) {
      const float zf = zf_at(zl, g, sy, seg_src(q.x0 + p, sx_scale, g));
      w[p >> 2] |= (zf > 0.f ? 1u : 0u) << (8 * (p & 3));
      if (zf_out && p < q.n) zf_out[base + p] = zf;
    }
    if (wide) {
      *(uint4*)(out + base) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int p = 0; p < PX; ++p)
        if (p < q.n) out[base + p] = (unsigned char)(w[p >> 2] >> (8 * (p & 3)));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// backward of the head
// ---------------------------------------------------------------------------------------------------------------------------------------------
// dfeat[row][8 ch .. 8 ch + 7] = sum_c dz[row][c] W[c][..], written as bf16 (one 16-byte store per thread and element group)
__global__ __launch_bounds__(256) void seg_dfeat_kernel(const float* __restrict__ dz, const float* __restrict__ W, bf16_t* __restrict__ dfeat,
                                                        int N, int D, int C) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  for (int i = threadIdx.x * 4; i < C * D; i += 1024) *(float4*)(wl + i) = *(const float4*)(W + i);
  __syncthreads();
  const int nch = D / 8;
  const long long total = (long long)N * nch;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / nch;
    const int col = (int)(idx - row * nch) * 8;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) {
      const float d = dz[row * C + c];
      const float4 w0 = *(const float4*)(wl + c * D + col), w1 = *(const float4*)(wl + c * D + col + 4);
      a[0] += d * w0.x; a[1] += d * w0.y; a[2] += d * w0.z; a[3] += d * w0.w;
      a[4] += d * w1.x; a[5] += d * w1.y; a[6] += d * w1.z; a[7] += d * w1.w;
    }
    *(uint4*)(dfeat + row * D + col) = make_uint4(pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(a[4], a[5]), pack2bf(a[6], a[7]));
  }
}

// rec[s][c][col] = sum over the rows of range s of dz[row][c] feat[row][col], rec[s][C D + c] = sum of dz[row][c]: stored, one writer each.
// Workgroup (s, t): row range s, columns 512 t + 8 lane .. + 7; its four waves take rows lo + w, lo + w + 4, ... and meet in LDS in wave order.
__global__ __launch_bounds__(256) void seg_wgrad_kernel(const bf16_t* __restrict__ feat, const float* __restrict__ dz, float* __restrict__ rec, int N,
                                                        int D, int C, int rows_per, long long rec_stride) {
  constexpr int UR = 4;
  __shared__ __attribute__((aligned(16))) float red[MAXC][64 * 8];
  __shared__ float redb[64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int s = blockIdx.x, col = blockIdx.y * 512 + lane * 8;
  const bool colok = col < D;                                   // D % 64 == 0: a lane's 8 columns are all in or all out
  const int lo = s * rows_per, hi = min(N, lo + rows_per);      // lo < N by the launch shape
  float acc[MAXC][8];
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[c][k] = 0.f;
  float bsum = 0.f;
#pragma unroll 1
  for (int r = lo + wave; r < hi; r += 4 * UR) {
    uint4 xv[UR];
#pragma unroll
    for (int u = 0; u < UR; ++u) xv[u] = *(const uint4*)(feat + (long long)min(r + 4 * u, hi - 1) * D + (colok ? col : 0));
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      if (r + 4 * u < hi) {                                     // wave-uniform
        const float* dr = dz + (long long)(r + 4 * u) * C;
        bsum += lane < C ? dr[lane] : 0.f;
        float f[8];
        unpack8(xv[u], f);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) {
            const float d = dr[c];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[c][k] += d * f[k];
          }
      }
    }
  }
  for (int w = 1; w < 4; ++w) {                                 // ((wave 0 + wave 1) + wave 2) + wave 3
    if (wave == w) {
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        *(float4*)(&red[c][lane * 8]) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
        *(float4*)(&red[c][lane * 8 + 4]) = make_float4(acc[c][4], acc[c][5], acc[c][6], acc[c][7]);
      }
      redb[lane] = bsum;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[c][k] += red[c][lane * 8 + k];
      bsum += redb[lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* out = rec + (long long)s * rec_stride;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < C && colok) {
        *(float4*)(out + (long long)c * D + col) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
        *(float4*)(out + (long long)c * D + col + 4) = make_float4(acc[c][4], acc[c][5], acc[c][6], acc[c][7]);
      }
    if (blockIdx.y == 0 && lane < C) out[(long long)C * D + lane] = bsum;
  }
}

__global__ __launch_bounds__(256) void seg_wgrad_sum_kernel(const float* __restrict__ rec, int S, long long rec_stride, float* __restrict__ dW,
                                                            float* __restrict__ db, int CD, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= CD + C) return;
  float v = 0.f;
  for (int s = 0; s < S; s += 8) {                              // eight loads in flight, added in record order
    float t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = s + k < S ? rec[(long long)(s + k) * rec_stride + i] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += t[k];
  }
  if (i < CD) dW[i] += v; else db[i - CD] += v;
}

inline long long align4(long long n) { return (n + 3) / 4 * 4; }
inline bool head_shape_ok(long long N, int D, int C) {
  return N >= 1 && N <= (1ll << 30) && D >= 64 && D % 64 == 0 && D <= MAX_D && C >= 1 && C <= MAXC;
}
inline int tiles_of(int H, int Wd) {
  const long long nunits = (long long)H * ((Wd + PX - 1) / PX);
  return (int)((nunits + 256 * UNITS - 1) / (256 * UNITS));
}
// every limit of the map launches, the workgroup counts of all three grids (stats / predict: B C tiles, gradient: B C ceil(g g / 4)) among
// them: whatever this takes can be launched, so every refusal comes before the first launch
inline bool map_shape_ok(int B, int g, int H, int Wd, int C) {
  if (!(B >= 1 && g >= 1 && g <= MAX_G && H >= g && Wd >= g && C >= 1 && C <= MAXC && (long long)H * ((Wd + PX - 1) / PX) <= (1ll << 30) &&
        (long long)B * C * (long long)H * Wd <= (1ll << 40)))
    return false;
  return (long long)B * C * tiles_of(H, Wd) <= 0x7fffffffll && (long long)B * C * ((g * g + 3) / 4) <= 0x7fffffffll;
}
inline int rows_per_record(int N) { return max(64, (N + MAX_RECORDS - 1) / MAX_RECORDS); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" long long medmoe_seg_scratch(int B, int g, int H, int W, int D, int C) {
  if (!map_shape_ok(B, g, H, W, C) || !head_shape_ok((long long)B * g * g, D, C)) return 0;
  const int N = B * g * g;
  const long long loss_part = align4((long long)B * C * tiles_of(H, W) * REC) + FIN;
  const long long bwd_part = medmoe_seg_head_bwd_scratch(N, D, C);
  return loss_part > bwd_part ? loss_part : bwd_part;
}

extern "C" long long medmoe_seg_head_bwd_scratch(int N, int D, int C) {
  if (!head_shape_ok(N, D, C)) return 0;
  const int rp = rows_per_record(N), S = (N + rp - 1) / rp;
  return (long long)S * ((long long)C * D + REC_PAD);
}

extern "C" int medmoe_seg_head_fwd(const void* feat, const float* W, const float* b, float* z, int N, int D, int C, hipStream_t stream) {
  if (!feat || !W || !b || !z || !aligned16(feat) || !aligned16(W)) return MM_ERR_ARG;
  if (!head_shape_ok(N, D, C)) return MM_ERR_SHAPE;
  const int ngroups = (N + 4 * RW - 1) / (4 * RW);
  const dim3 grid(min(ngroups, 1024)), block(256);
  const size_t lds = (size_t)C * D * sizeof(float);
  const bf16_t* x = (const bf16_t*)feat;
  switch ((D + 511) / 512) {
    case 1: hipLaunchKernelGGL(seg_row_kernel<1>, grid, block, lds, stream, x, W, b, z, N, D, C); break;
    case 2: hipLaunchKernelGGL(seg_row_kernel<2>, grid, block, lds, stream, x, W, b, z, N, D, C); break;
    case 3: hipLaunchKernelGGL(seg_row_kernel<3>, grid, block, lds, stream, x, W, b, z, N, D, C); break;
    default: hipLaunchKernelGGL(seg_row_kernel<4>, grid, block, lds, stream, x, W, b, z, N, D, C); break;
  }
  return mm_check_launch();
}

extern "C" int medmoe_seg_loss(const float* z, const signed char* masks, const float* pos_weight, float w_bce, float w_dice, float dice_eps,
                               float loss_scale, float* dz, float* loss, long long* counts, float* scratch, long long scratch_floats, int B,
                               int g, int H, int W, int C, hipStream_t stream) {
  if (!z || !masks || !loss || !counts || !scratch || !aligned16(masks) || !aligned16(scratch)) return MM_ERR_ARG;
  if (!map_shape_ok(B, g, H, W, C)) return MM_ERR_SHAPE;
  if (!(dice_eps >= 0.f)) return MM_ERR_ARG;
  const int tiles = tiles_of(H, W);
  const long long nrec = (long long)B * C * tiles;
  if (scratch_floats < align4(nrec * REC) + FIN) return MM_ERR_ARG;
  float* rec = scratch;
  float* fin = scratch + align4(nrec * REC);
  hipLaunchKernelGGL(seg_stats_kernel, dim3((unsigned)nrec), dim3(256), 0, stream, z, masks, pos_weight, rec, g, H, W, C, tiles);
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(256), 0, stream, rec, counts, loss, fin, B, C, tiles, w_bce, w_dice, dice_eps, loss_scale);
  if (dz) {
    const int groups = (g * g + 3) / 4;
    const long long nwg = (long long)B * C * groups;
    hipLaunchKernelGGL(seg_grad_kernel, dim3((unsigned)nwg), dim3(256), 0, stream, z, masks, pos_weight, fin, dz, g, H, W, C, groups);
  }
  return mm_check_launch();
}

extern "C" int medmoe_seg_head_bwd(const float* dz, const void* feat, const float* W, void* dfeat, float* dW, float* db, float* scratch,
                                   long long scratch_floats, int N, int D, int C, hipStream_t stream) {
  if (!dz || !feat || !W || !dW || !db || !scratch || !aligned16(feat) || !aligned16(W) || !aligned16(scratch) || (dfeat && !aligned16(dfeat)))
    return MM_ERR_ARG;
  if (!head_shape_ok(N, D, C)) return MM_ERR_SHAPE;
  const int rp = rows_per_record(N), S = (N + rp - 1) / rp;
  const long long stride = (long long)C * D + REC_PAD;
  if (scratch_floats < medmoe_seg_head_bwd_scratch(N, D, C)) return MM_ERR_ARG;
  if (dfeat) {
    const long long total = (long long)N * (D / 8);
    hipLaunchKernelGGL(seg_dfeat_kernel, dim3((unsigned)min((total + 255) / 256, 4096ll)), dim3(256), (size_t)C * D * sizeof(float), stream, dz, W,
                       (bf16_t*)dfeat, N, D, C);
  }
  hipLaunchKernelGGL(seg_wgrad_kernel, dim3(S, (D + 511) / 512), dim3(256), 0, stream, (const bf16_t*)feat, dz, scratch, N, D, C, rp, stride);
  hipLaunchKernelGGL(seg_wgrad_sum_kernel, dim3((C * D + C + 255) / 256), dim3(256), 0, stream, scratch, S, stride, dW, db, C * D, C);
  return mm_check_launch();
}

extern "C" int medmoe_seg_predict(const float* z, unsigned char* masks, float* zf, int B, int g, int H, int W, int C, hipStream_t stream) {
  if (!z || !masks || !aligned16(masks)) return MM_ERR_ARG;
  if (!map_shape_ok(B, g, H, W, C)) return MM_ERR_SHAPE;
  const int tiles = tiles_of(H, W);
  const long long nwg = (long long)B * C * tiles;
  hipLaunchKernelGGL(seg_predict_kernel, dim3((unsigned)nwg), dim3(256), 0, stream, z, masks, zf, g, H, W, C, tiles);
  return mm_check_launch();
}
