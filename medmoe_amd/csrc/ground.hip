// Phrase grounding: a word span of a caption becomes a heat map over the image regions, the map is scored against boxes.
// Two entry points, one owner per output element and no read-modify-write of memory anywhere: two launches on the same inputs give the same bits and
// medmoe_nondet_launches() never moves.
//
//   medmoe_ground_maps   ground_maps_kernel<TPW, NTT>: one workgroup of 8 waves per entry (image b, caption i, words [lo, hi)).  A wave owns the
//                        16-region row tiles wid, wid + 8, ... (TPW of them) against all NTT 16-word tiles of the caption: the raw scores
//                        s_raw[t][p] = <ctx[b][p], words[i][t]> accumulate on v_mfma_f32_16x16x32_bf16 with both operands read straight from
//                        global memory (a region row is read by one wave only; the word rows come from the cache for the other seven).  Lane
//                        (fr, g) then holds word 16 tt + fr against the regions 16 tile + 4 g + r, so a reduction over the WORDS crosses the 16
//                        lanes of a DPP row and the wave's word tiles, and nothing of the shape [T][P] is ever stored.
//                          mode 0 (attention, losses.py:698-736): s = softmax over the words t < cap_len, a = softmax over the regions of
//                          temp1 s, h[p] = mean of a[t][p] over the span.  s lies in [0, 1], so exp(temp1 (s - 1)) needs no running maximum
//                          (temp1 <= 64); the per-word region sums Z_t are the one cross-wave exchange: partial sums in LDS [wave][T], one
//                          barrier, every wave adds them in wave order.
//                          mode 1 (cosine): h[p] = <ctx_p, u> / max(|ctx_p| |u|, eps), u = the sum of the span's word vectors; <ctx_p, u> is
//                          the sum of s_raw over the span, |ctx_p|^2 and |u|^2 are fp32 sums over the bf16 inputs.
//   medmoe_ground_score  ground_score_kernel: one workgroup per entry, the g x g map in LDS; hf[y][x], the bilinear upsample of seg_plan.h (the
//                        map of DESIGN 3t), is recomputed per pixel by ONE device function in both passes and for the optional store.  Pass 1:
//                        max, min and the first maximal pixel in row-major order; pass 2: hit, the union's area, the counts at the stored
//                        thresholds and the fp64 sums, every thread over its pixels in index order, lanes and waves added in a fixed order.
//
// The kernels trust their tables: medmoe_amd/ops.py validates every image, caption, span and box on the host before anything is uploaded.
#include "common.h"
#include "medmoe_hip.h"
#include "seg_plan.h"

namespace {

constexpr int GM_WAVES = 8;
constexpr int GM_MAX_G = 32, GM_MAX_T = 80, GM_MAX_D = 2048;
constexpr float GM_MAX_TEMP1 = 64.f;
constexpr int GS_THREADS = 256, GS_WAVES = GS_THREADS / 64;
constexpr int GS_MAX_NB = 8, GS_MAX_TH = 4;

template <int CTRL>
__device__ __forceinline__ float gr_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// over the 16 lanes of a DPP row, result in every lane (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror)
__device__ __forceinline__ float gr_row16_sum(float v) {
  v += gr_dpp<0xB1>(v); v += gr_dpp<0x4E>(v); v += gr_dpp<0x141>(v); v += gr_dpp<0x140>(v);
  return v;
}
__device__ __forceinline__ float gr_row16_max(float v) {
  v = fmaxf(v, gr_dpp<0xB1>(v)); v = fmaxf(v, gr_dpp<0x4E>(v)); v = fmaxf(v, gr_dpp<0x141>(v)); v = fmaxf(v, gr_dpp<0x140>(v));
  return v;
}
__device__ __forceinline__ float gr_grp4_sum(float v) {      // over the four 16-lane groups
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

struct GroundArgs {
  const bf16_t* ctx; const bf16_t* words; const int* cap_lens; const int* entries; float* h;
  int P, T, D, mode;
  float temp1, eps;
};

template <int TPW, int NTT>
__global__ __launch_bounds__(GM_WAVES * 64) void ground_maps_kernel(GroundArgs a) {
  __shared__ float zpart[GM_WAVES][NTT * 16];          // mode 0: the waves' partial region sums of every word
  __shared__ float cn2[TPW * GM_WAVES * 16];           // mode 1: |ctx_p|^2
  __shared__ float red[GM_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, g = lane >> 4;
  const int4 en = *(const int4*)(a.entries + 4 * (long long)blockIdx.x);
  const int b = en.x, i = en.y, lo = en.z, hi = en.w;
  const int P = a.P, T = a.T, D = a.D, ntiles = (P + 15) >> 4;
  const int cap = a.cap_lens[i];
  // operand rows: a word past T and a region past P repeat the last one (loaded, never used)
  const bf16_t* wp[NTT];
  bool tok[NTT], insp[NTT];
#pragma unroll
  for (int tt = 0; tt < NTT; ++tt) {
    const int t = 16 * tt + fr;
    wp[tt] = a.words + ((long long)i * T + min(t, T - 1)) * D + 8 * g;
    tok[tt] = t < cap;
    insp[tt] = t >= lo && t < hi;
  }
  const bf16_t* cp[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) cp[j] = a.ctx + ((long long)b * P + min(16 * (wid + GM_WAVES * j) + fr, P - 1)) * D + 8 * g;
  // ---- raw scores: acc[j][tt][r] = <region 16 tile_j + 4 g + r, word 16 tt + fr> ----
  f32x4_t acc[TPW][NTT];
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) acc[j][tt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int k = 0; k < D; k += 32) {
    bf16x8_t bw[NTT];
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) bw[tt] = *(const bf16x8_t*)(wp[tt] + k);
#pragma unroll
    for (int j = 0; j < TPW; ++j)
      if (wid + GM_WAVES * j < ntiles) {                                         // wave-uniform
        const bf16x8_t av = *(const bf16x8_t*)(cp[j] + k);
#pragma unroll
        for (int tt = 0; tt < NTT; ++tt) acc[j][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bw[tt], acc[j][tt], 0, 0, 0);
      }
  }
  float* hout = a.h + (long long)blockIdx.x * P;
  if (a.mode == 0) {
    // ---- word softmax per region (over the DPP row and the word tiles), then e = exp(temp1 (s - 1)) in place and its sums over the regions ----
    float zp[NTT];
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) zp[tt] = 0.f;
#pragma unroll
    for (int j = 0; j < TPW; ++j)
      if (wid + GM_WAVES * j < ntiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool pok = 16 * (wid + GM_WAVES * j) + 4 * g + r < P;
          float m = -3.0e38f;
#pragma unroll
          for (int tt = 0; tt < NTT; ++tt) m = tok[tt] ? fmaxf(m, acc[j][tt][r]) : m;
          m = gr_row16_max(m);
          float s = 0.f;
#pragma unroll
          for (int tt = 0; tt < NTT; ++tt) {
            const float ex = tok[tt] ? expf(acc[j][tt][r] - m) : 0.f;
            acc[j][tt][r] = ex;
            s += ex;
          }
          s = gr_row16_sum(s);
#pragma unroll
          for (int tt = 0; tt < NTT; ++tt) {
            const float ev = (tok[tt] && pok) ? expf(a.temp1 * (acc[j][tt][r] / s - 1.f)) : 0.f;
            acc[j][tt][r] = ev;
            zp[tt] += ev;
          }
        }
      }
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) {
      const float z = gr_grp4_sum(zp[tt]);
      if (g == 0) zpart[wid][16 * tt + fr] = z;
    }
    __syncthreads();
    float zinv[NTT];
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) {
      float z = 0.f;
#pragma unroll
      for (int w = 0; w < GM_WAVES; ++w) z += zpart[w][16 * tt + fr];
      zinv[tt] = insp[tt] ? 1.f / z : 0.f;
    }
    const float nspan = (float)(hi - lo);
#pragma unroll
    for (int j = 0; j < TPW; ++j)
      if (wid + GM_WAVES * j < ntiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = 0.f;
#pragma unroll
          for (int tt = 0; tt < NTT; ++tt) v += acc[j][tt][r] * zinv[tt];
          v = gr_row16_sum(v) / nspan;
          const int p = 16 * (wid + GM_WAVES * j) + 4 * g + r;
          if (fr == r && p < P) hout[p] = v;
        }
      }
  } else {
    // ---- |ctx_p|^2: lane (fr, g) squares its quarter of row fr of every tile of the wave ----
#pragma unroll
    for (int j = 0; j < TPW; ++j)
      if (wid + GM_WAVES * j < ntiles) {
        float ss = 0.f;
        for (int k = 0; k < D; k += 32) {
          const uint4 v = *(const uint4*)(cp[j] + k);
          const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float x0 = __uint_as_float(q[c] << 16), x1 = __uint_as_float(q[c] & 0xffff0000u);
            ss += x0 * x0;
            ss += x1 * x1;
          }
        }
        ss = gr_grp4_sum(ss);
        if (g == 0) cn2[16 * (wid + GM_WAVES * j) + fr] = ss;
      }
    // ---- |u|^2, u = the fp32 sum of the span's word vectors: a thread takes the columns tid, tid + 512, ... ----
    float us = 0.f;
    for (int d = tid; d < D; d += GM_WAVES * 64) {
      float u = 0.f;
      for (int t = lo; t < hi; ++t) u += bf2f(a.words[((long long)i * T + t) * D + d]);
      us += u * u;
    }
    us = wave_sum(us);
    if (lane == 0) red[wid] = us;
    __syncthreads();
    float u2 = 0.f;
#pragma unroll
    for (int w = 0; w < GM_WAVES; ++w) u2 += red[w];
    const float un = sqrtf(u2);
#pragma unroll
    for (int j = 0; j < TPW; ++j)
      if (wid + GM_WAVES * j < ntiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = 0.f;
#pragma unroll
          for (int tt = 0; tt < NTT; ++tt) v += insp[tt] ? acc[j][tt][r] : 0.f;
          v = gr_row16_sum(v);
          const int p = 16 * (wid + GM_WAVES * j) + 4 * g + r;
          if (fr == r && p < P) hout[p] = v / fmaxf(sqrtf(cn2[p]) * un, a.eps);
        }
      }
  }
}

template <int TPW>
void gm_launch(const GroundArgs& a, int ntt, int n, hipStream_t stream) {
  const dim3 grid(n), block(GM_WAVES * 64);
  switch (ntt) {
    case 1: hipLaunchKernelGGL((ground_maps_kernel<TPW, 1>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((ground_maps_kernel<TPW, 2>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((ground_maps_kernel<TPW, 3>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((ground_maps_kernel<TPW, 4>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((ground_maps_kernel<TPW, 5>), grid, block, 0, stream, a); break;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// score pass
// ---------------------------------------------------------------------------------------------------------------------------------------------
// the bilinear read of the g x g map in LDS, in the operation order of torch's upsample_bilinear2d with contraction to fused multiply-adds
// switched off (the expression of segment.hip's zf_at): the statistics of both passes and the stored map come from this one function
__device__ __forceinline__ float hf_at(const float* hl, int g, SegSrc sy, SegSrc sx) {
#pragma clang fp contract(off)
  const float a = hl[sy.i0 * g + sx.i0], b = hl[sy.i0 * g + sx.i1], c = hl[sy.i1 * g + sx.i0], d = hl[sy.i1 * g + sx.i1];
  const float w1x = sx.lam, w0x = 1.f - w1x, w1y = sy.lam, w0y = 1.f - w1y;
  return w0y * (w0x * a + w1x * b) + w1y * (w0x * c + w1x * d);
}

__device__ __forceinline__ float thr_of(float mn, float mx, float th) {
#pragma clang fp contract(off)
  return mn + th * (mx - mn);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(GS_THREADS) void ground_score_kernel(const float* __restrict__ h, const int* __restrict__ boxes,
                                                                  const float* __restrict__ theta, float* __restrict__ hf,
                                                                  float* __restrict__ rec_f, int* __restrict__ rec_i,
                                                                  double* __restrict__ rec_d, int g, int H, int Wd, int NB, int NTH) {
  __shared__ float hl[GM_MAX_G * GM_MAX_G];
  __shared__ int bx[GS_MAX_NB][4];
  __shared__ float rmax[GS_WAVES], rmin[GS_WAVES], thr_s[GS_MAX_TH];
  __shared__ int rarg[GS_WAVES];
  __shared__ double rd[GS_WAVES][4];
  __shared__ int ri[GS_WAVES][1 + 2 * GS_MAX_TH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long e = blockIdx.x;
  const int npix = H * Wd;
  for (int k = tid; k < g * g; k += GS_THREADS) hl[k] = h[e * g * g + k];
  if (tid < 4 * NB) bx[tid >> 2][tid & 3] = boxes[(e * NB) * 4 + tid];
  __syncthreads();
  const float sy_scale = seg_scale(g, H), sx_scale = seg_scale(g, Wd);
  auto in_union = [&](int y, int x) -> bool {
    bool in = false;
    for (int k = 0; k < NB; ++k) in = in || (x >= bx[k][0] && x < bx[k][2] && y >= bx[k][1] && y < bx[k][3]);
    return in;
  };
  // ---- pass 1: max, min, the first maximal pixel (a thread's pixels ascend, so `>` keeps its first; ties between threads go to the lower index) ----
  float mx = -INFINITY, mn = INFINITY;
  int am = 0x7fffffff;
  float* hfe = hf ? hf + e * npix : nullptr;
  for (int idx = tid; idx < npix; idx += GS_THREADS) {
    const int y = idx / Wd, x = idx - y * Wd;
    const float v = hf_at(hl, g, seg_src(y, sy_scale, g), seg_src(x, sx_scale, g));
    if (hfe) hfe[idx] = v;
    if (v > mx) { mx = v; am = idx; }
    mn = fminf(mn, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float omx = __shfl_xor(mx, o, 64), omn = __shfl_xor(mn, o, 64);
    const int oam = __shfl_xor(am, o, 64);
    if (omx > mx || (omx == mx && oam < am)) { mx = omx; am = oam; }
    mn = fminf(mn, omn);
  }
  if (lane == 0) { rmax[wave] = mx; rmin[wave] = mn; rarg[wave] = am; }
  __syncthreads();
  mx = rmax[0]; mn = rmin[0]; am = rarg[0];
#pragma unroll
  for (int w = 1; w < GS_WAVES; ++w) {
    if (rmax[w] > mx || (rmax[w] == mx && rarg[w] < am)) { mx = rmax[w]; am = rarg[w]; }
    mn = fminf(mn, rmin[w]);
  }
  if (am >= npix) am = 0;                                  // no pixel compared greater than -inf (a map of NaN): pixel 0
  if (tid < NTH) thr_s[tid] = thr_of(mn, mx, theta[tid]);
  __syncthreads();
  float thr[GS_MAX_TH];
#pragma unroll
  for (int k = 0; k < GS_MAX_TH; ++k) thr[k] = k < NTH ? thr_s[k] : INFINITY;
  // ---- pass 2: the union's area, the counts at the thresholds, the fp64 sums ----
  int area = 0, pred[GS_MAX_TH], inter[GS_MAX_TH];
#pragma unroll
  for (int k = 0; k < GS_MAX_TH; ++k) { pred[k] = 0; inter[k] = 0; }
  double s_in = 0.0, q_in = 0.0, s_all = 0.0, q_all = 0.0;
  for (int idx = tid; idx < npix; idx += GS_THREADS) {
    const int y = idx / Wd, x = idx - y * Wd;
    const float v = hf_at(hl, g, seg_src(y, sy_scale, g), seg_src(x, sx_scale, g));
    const bool in = in_union(y, x);
    const double dv = (double)v, d2 = dv * dv;
    area += in;
    s_all += dv; q_all += d2;
    s_in += in ? dv : 0.0; q_in += in ? d2 : 0.0;
#pragma unroll
    for (int k = 0; k < GS_MAX_TH; ++k) {
      const bool on = k < NTH && v >= thr[k];
      pred[k] += on;
      inter[k] += on && in;
    }
  }
  area = wave_sum_int(area);
  s_in = wave_sum_f64(s_in); q_in = wave_sum_f64(q_in); s_all = wave_sum_f64(s_all); q_all = wave_sum_f64(q_all);
#pragma unroll
  for (int k = 0; k < GS_MAX_TH; ++k) { pred[k] = wave_sum_int(pred[k]); inter[k] = wave_sum_int(inter[k]); }
  if (lane == 0) {
    rd[wave][0] = s_in; rd[wave][1] = q_in; rd[wave][2] = s_all; rd[wave][3] = q_all;
    ri[wave][0] = area;
#pragma unroll
    for (int k = 0; k < GS_MAX_TH; ++k) { ri[wave][1 + 2 * k] = inter[k]; ri[wave][2 + 2 * k] = pred[k]; }
  }
  __syncthreads();
  if (tid == 0) {
    float* rf = rec_f + e * (2 + NTH);
    int* rI = rec_i + e * (4 + 2 * NTH);
    rf[0] = mx; rf[1] = mn;
    for (int k = 0; k < NTH; ++k) rf[2 + k] = thr_s[k];
    const int ay = am / Wd, ax = am - ay * Wd;
    rI[0] = ay; rI[1] = ax; rI[2] = in_union(ay, ax) ? 1 : 0;
    for (int c = 0; c < 1 + 2 * NTH; ++c) {
      int t = 0;
      for (int w = 0; w < GS_WAVES; ++w) t += ri[w][c];
      rI[3 + c] = t;
    }
    for (int c = 0; c < 4; ++c) {
      double t = 0.0;
      for (int w = 0; w < GS_WAVES; ++w) t += rd[w][c];
      rec_d[e * 4 + c] = t;
    }
  }
}

}  // namespace

extern "C" int medmoe_ground_maps(const void* ctx, const void* words, const int* cap_lens, const int* entries, float* h, int n, int B, int Bc,
                                  int P, int T, int D, int mode, float temp1, float eps, hipStream_t stream) {
  if (n < 0 || (mode != 0 && mode != 1) || !(temp1 >= 0.f && temp1 <= GM_MAX_TEMP1) || !(eps >= 0.f)) return MM_ERR_ARG;
  int g = 1;
  while (g * g < P && g < GM_MAX_G) ++g;
  if (B <= 0 || Bc <= 0 || P <= 0 || g * g != P || T < 1 || T > GM_MAX_T || D < 64 || D > GM_MAX_D || (D % 64)) return MM_ERR_SHAPE;
  if (n == 0) return MM_OK;
  if (!ctx || !words || !cap_lens || !entries || !h) return MM_ERR_ARG;
  GroundArgs a;
  a.ctx = (const bf16_t*)ctx; a.words = (const bf16_t*)words; a.cap_lens = cap_lens; a.entries = entries; a.h = h;
  a.P = P; a.T = T; a.D = D; a.mode = mode; a.temp1 = temp1; a.eps = eps;
  const int ntiles = (P + 15) / 16, ntt = (T + 15) / 16;
  const int tpw = (ntiles + GM_WAVES - 1) / GM_WAVES;       // 1 .. 8
  if (tpw <= 1) gm_launch<1>(a, ntt, n, stream);
  else if (tpw <= 2) gm_launch<2>(a, ntt, n, stream);
  else if (tpw <= 4) gm_launch<4>(a, ntt, n, stream);
  else gm_launch<8>(a, ntt, n, stream);
  return mm_check_launch();
}

extern "C" int medmoe_ground_score(const float* h, const int* boxes, const float* theta, float* hf, float* rec_f, int* rec_i, double* rec_d,
                                   int n, int g, int H, int W, int NB, int NTH, hipStream_t stream) {
  if (n < 0) return MM_ERR_ARG;
  if (g < 1 || g > GM_MAX_G || H < g || W < g || (long long)H * W > (1ll << 30) || NB < 1 || NB > GS_MAX_NB || NTH < 0 || NTH > GS_MAX_TH)
    return MM_ERR_SHAPE;
  if (n == 0) return MM_OK;
  if (!h || !boxes || (NTH > 0 && !theta) || !rec_f || !rec_i || !rec_d) return MM_ERR_ARG;
  hipLaunchKernelGGL(ground_score_kernel, dim3(n), dim3(GS_THREADS), 0, stream, h, boxes, theta, hf, rec_f, rec_i, rec_d, g, H, W, NB, NTH);
  return mm_check_launch();
}
