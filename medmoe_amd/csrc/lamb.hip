// LAMB on the flat arenas (You et al., "Large Batch Optimization for Deep Learning"): Adam's moments, the weight decay as part
// of the update u, and one trust ratio |w| / |u| per SEGMENT (one parameter tensor) that scales the step.  Three launches per arena:
//   moments  reads p, g, m, v, writes m, v; forms u in registers and leaves, with plain stores, the partial sums of p^2 and u^2 per
//            (chunk of LAMB_CHUNK elements, segment met inside that chunk) as records in a scratch buffer          24 B / element
//   ratios   adds each segment's records in index order (one wave per segment) and writes r_s                      a few KB
//   apply    reads p, m, v, recomputes u with the SAME inline function (contraction pinned: the same bits), steps p, writes the bf16 copy
//            and, in the EMA forms, averages the new parameter while it is in registers                             18 B / element
// u is recomputed, not stored: 42 B per element against 46 with a stored u, and no third state buffer.  No floating-point atomics, no
// arrival counters: the record layout (lamb_plan.h) is a function of (n, segment table) only, every sum has a fixed order, and a step
// reads nothing from the host.
#include "common.h"
#include "lamb_plan.h"
#include "medmoe_hip.h"

using lamb_plan::LAMB_CHUNK;
using lamb_plan::LAMB_THREADS;
using lamb_plan::LAMB_VEC;
using lamb_plan::LAMB_RATIO_THREADS;

#define LAMB_LDS_SEGS 1024            // segment tables up to this size are staged in LDS; larger ones are searched where they lie

// the gradient operand: fp32, or the reduced bf16 buffer of a bf16 gradient exchange widened in registers, element order kept
__device__ __forceinline__ float4 lamb_grad4(const float* g, long long i) { return *(const float4*)(g + i * 4); }
__device__ __forceinline__ float4 lamb_grad4(const bf16_t* g, long long i) {
  const uint2 r = *(const uint2*)(g + i * 4);
  float4 v;
  v.x = __uint_as_float(r.x << 16); v.y = __uint_as_float(r.x & 0xffff0000u);
  v.z = __uint_as_float(r.y << 16); v.w = __uint_as_float(r.y & 0xffff0000u);
  return v;
}

// Adam's moments in adam_update's operation order (lerp form), on the scaled and clipped gradient.  The first moment is formed in double and
// rounded ONCE: m + (1 - b1) (g' - m) cancels where the new gradient opposes the old moment, and in fp32 the roundings of g', of the
// difference and of 1 - b1 then stay at the size of |g'| while m itself goes to zero - a relative error of a = m_hat / (sqrt(v_hat) + eps)
// of many units in the last place, which LAMB's step (a times a trust ratio that may be large) hands on to the parameter.  g coef is
// exact in double; three fp64 operations per element of a launch that waits for memory.  v is a sum of non-negative terms: fp32.
__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, float coef, float b2, double omb1, float omb2) {
  const float gr = g * coef;
  const double md = (double)m;
  m = (float)(md + omb1 * ((double)g * (double)coef - md));
  v = b2 * v + omb2 * gr * gr;
}

// u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd_s p.  Five separately rounded fp32 operations: contraction is switched off for the whole
// function, so that the moments launch and the apply launch - which inline it into different surroundings - produce the same bits.
__device__ __forceinline__ float lamb_u(float p, float m, float v, float wds, float bc1, float bc2_sqrt, float eps) {
#pragma clang fp contract(off)
  const float mh = m / bc1;
  const float den = sqrtf(v) / bc2_sqrt + eps;
  const float a = mh / den;
  const float d = wds * p;
  return a + d;
}

// the weight average of the EMA forms, exactly as the Adam launches form it (optim.hip ema_update): three separately rounded operations
__device__ __forceinline__ void lamb_ema_update(float& e, float p, float omd) {
#pragma clang fp contract(off)
  const float d = p - e;
  const float s = omd * d;
  e = e + s;
}

// first segment whose end lies behind element e0 (<= last whatever the table holds)
__device__ __forceinline__ int lamb_find(const long long* ends, int last, long long e0) {
  int r = 0, hi = last;
  while (r < hi) {
    const int mid = (r + hi) >> 1;
    if (ends[mid] > e0) hi = mid; else r = mid + 1;
  }
  return r;
}

__device__ __forceinline__ float lamb_clip_coef(const float* normsq, float max_norm, float grad_scale) {
  float coef = grad_scale;
  if (normsq && max_norm > 0.f) {
    const float nrm = sqrtf(*normsq) * grad_scale;
    coef *= fminf(1.f, max_norm / (nrm + 1e-6f));
  }
  return coef;
}

// ---------------------------------------------------------------------------------------------
// moments: one workgroup per chunk (grid-strided over the chunks: what a workgroup stores depends on the chunk alone).  A thread holds
// LAMB_VEC float4s of the chunk (float4 t + 256 k), keeps their p^2 and u^2 in registers, and for every segment the chunk meets the block
// sums the squares that lie in it: per thread in element order, the wave by the xor tree, the four waves as (w0 + w1) + (w2 + w3).
// ---------------------------------------------------------------------------------------------
template <bool LDS, typename GT>
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long long n, const long long* __restrict__ seg_end,
                                                           const float* __restrict__ seg_wd, const long long* __restrict__ rec_base,
                                                           int n_segs, float2* __restrict__ rec, long long max_rec, float b2, double omb1,
                                                           float omb2, float eps, float wd, float bc1, float bc2_sqrt,
                                                           const float* __restrict__ normsq, float max_norm, float grad_scale) {
  __shared__ long long s_end[LDS ? LAMB_LDS_SEGS : 1], s_base[LDS ? LAMB_LDS_SEGS : 1];
  __shared__ float s_wd[LDS ? LAMB_LDS_SEGS : 1];
  __shared__ float red[2][4];
  if (LDS) {
    for (int r = threadIdx.x; r < n_segs; r += LAMB_THREADS) { s_end[r] = seg_end[r]; s_base[r] = rec_base[r]; s_wd[r] = seg_wd[r]; }
    __syncthreads();
  }
  const long long* ends = LDS ? s_end : seg_end;
  const long long* base = LDS ? s_base : rec_base;
  const float* wdm = LDS ? s_wd : seg_wd;
  const float coef = lamb_clip_coef(normsq, max_norm, grad_scale);
  if (blockIdx.x == 0 && threadIdx.x == 0) ((float*)rec)[lamb_plan::coef_slot(n, n_segs)] = coef;   // what this step scaled the gradient by
  const int last = n_segs - 1;
  const long long n4 = n >> 2, nch = lamb_plan::n_chunks(n);
  for (long long c = blockIdx.x; c < nch; c += gridDim.x) {
    const long long c0 = c * LAMB_CHUNK, c1 = c0 + LAMB_CHUNK < n ? c0 + LAMB_CHUNK : n;
    float PS[LAMB_VEC * 4], US[LAMB_VEC * 4];
#pragma unroll
    for (int k = 0; k < LAMB_VEC; ++k) {
      const long long i = (c0 >> 2) + k * LAMB_THREADS + threadIdx.x;
      if (i < n4) {
        const float4 pp = *(const float4*)(p + i * 4);
        const float4 gg = lamb_grad4(g, i);
        float4 mm = *(float4*)(m + i * 4), vv = *(float4*)(v + i * 4);
        const float* P = (const float*)&pp; const float* G = (const float*)&gg; float* M = (float*)&mm; float* V = (float*)&vv;
        const long long e0 = i * 4;
        int r = lamb_find(ends, last, e0);
        long long end = ends[r];
        float wds = wd * wdm[r];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (e0 + e >= end && r < last) {                          // a boundary inside this float4 (segments may be one element long)
            do { ++r; end = ends[r]; } while (e0 + e >= end && r < last);
            wds = wd * wdm[r];
          }
          lamb_moments(G[e], M[e], V[e], coef, b2, omb1, omb2);
          const float u = lamb_u(P[e], M[e], V[e], wds, bc1, bc2_sqrt, eps);
          PS[k * 4 + e] = P[e] * P[e];
          US[k * 4 + e] = u * u;
        }
        *(float4*)(m + i * 4) = mm; *(float4*)(v + i * 4) = vv;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { PS[k * 4 + e] = 0.f; US[k * 4 + e] = 0.f; }
      }
    }
    // the segments this chunk meets: sf .. sl, the same for every thread of the block
    const int sf = lamb_find(ends, last, c0), sl = lamb_find(ends, last, c1 - 1);
    for (int s = sf; s <= sl; ++s) {
      const long long start = s ? ends[s - 1] : 0;
      const long long lo = start > c0 ? start : c0, hi = (ends[s] < c1 && s < last) ? ends[s] : c1;
      float ps = 0.f, us = 0.f;
#pragma unroll
      for (int k = 0; k < LAMB_VEC; ++k) {
        const long long e0 = c0 + ((long long)k * LAMB_THREADS + threadIdx.x) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool in = e0 + e >= lo && e0 + e < hi;
          ps += in ? PS[k * 4 + e] : 0.f;
          us += in ? US[k * 4 + e] : 0.f;
        }
      }
      ps = wave_sum(ps); us = wave_sum(us);
      if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ps; red[1][threadIdx.x >> 6] = us; }
      __syncthreads();
      if (threadIdx.x == 0 && hi > lo) {
        const long long idx = lamb_plan::record_index(base[s], start, c);
        if (idx >= 0 && idx < max_rec) rec[idx] = make_float2((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]),
                                                              (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------
// ratios: one wave per segment.  Lane t adds records t, t + 64, ... of the segment in that order, the lanes meet in the xor tree.
// out: [n_segs] trust ratios, then per segment (sum p^2, sum u^2) - kept for logging and for the tests.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void lamb_ratios_kernel(const float2* __restrict__ rec, long long max_rec, const long long* __restrict__ seg_end,
                                                         const float* __restrict__ seg_wd, const long long* __restrict__ rec_base, int n_segs,
                                                         float wd, int always_adapt, int trust_clip, float* __restrict__ out) {
  const int s = blockIdx.x;
  const long long start = s ? seg_end[s - 1] : 0, end = seg_end[s];
  const long long cnt = lamb_plan::seg_chunks(start, end), b = rec_base[s];
  float ps = 0.f, us = 0.f;
  for (long long r = threadIdx.x; r < cnt; r += LAMB_RATIO_THREADS) {
    const long long idx = b + r;
    if (idx >= 0 && idx < max_rec) { const float2 q = rec[idx]; ps += q.x; us += q.y; }
  }
  ps = wave_sum(ps); us = wave_sum(us);
  if (threadIdx.x == 0) {
    const float wn = sqrtf(ps), un = sqrtf(us), wds = wd * seg_wd[s];
    float r = 1.f;
    if (wn > 0.f && un > 0.f && (always_adapt || wds != 0.f)) r = wn / un;
    if (trust_clip) r = fminf(r, 1.f);
    out[s] = r;
    out[n_segs + 2 * s] = ps;
    out[n_segs + 2 * s + 1] = us;
  }
}

// ---------------------------------------------------------------------------------------------
// apply: p <- p - ((lr lr_mult_s) r_s) u, the bf16 copy, the average.  Element-wise, 16 bytes per lane; the segment of a float4's first
// element by bisection, followed per element inside the float4 (adam_groups_kernel's walk).
// ---------------------------------------------------------------------------------------------
template <bool LDS, bool EMA>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                         bf16_t* __restrict__ p16, long long n, const long long* __restrict__ seg_end,
                                                         const float* __restrict__ seg_lr, const float* __restrict__ seg_wd, int n_segs,
                                                         const float* __restrict__ ratios, float lr, float eps, float wd, float bc1,
                                                         float bc2_sqrt, float* __restrict__ ema, float omd) {
  __shared__ long long s_end[LDS ? LAMB_LDS_SEGS : 1];
  __shared__ float s_step[LDS ? LAMB_LDS_SEGS : 1], s_wd[LDS ? LAMB_LDS_SEGS : 1];
  if (LDS) {
    for (int r = threadIdx.x; r < n_segs; r += 256) { s_end[r] = seg_end[r]; s_step[r] = (lr * seg_lr[r]) * ratios[r]; s_wd[r] = wd * seg_wd[r]; }
    __syncthreads();
  }
  const long long* ends = LDS ? s_end : seg_end;
  const int last = n_segs - 1;
  const long long n4 = n >> 2;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 pp = *(float4*)(p + i * 4);
    const float4 mm = *(const float4*)(m + i * 4), vv = *(const float4*)(v + i * 4);
    float* P = (float*)&pp; const float* M = (const float*)&mm; const float* V = (const float*)&vv;
    float4 ee;
    if constexpr (EMA) ee = *(const float4*)(ema + i * 4);
    const long long e0 = i * 4;
    int r = lamb_find(ends, last, e0);
    long long end = ends[r];
    float step = LDS ? s_step[r] : (lr * seg_lr[r]) * ratios[r], wds = LDS ? s_wd[r] : wd * seg_wd[r];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e0 + e >= end && r < last) {
        do { ++r; end = ends[r]; } while (e0 + e >= end && r < last);
        step = LDS ? s_step[r] : (lr * seg_lr[r]) * ratios[r]; wds = LDS ? s_wd[r] : wd * seg_wd[r];
      }
      const float u = lamb_u(P[e], M[e], V[e], wds, bc1, bc2_sqrt, eps);
      P[e] = P[e] - step * u;
    }
    *(float4*)(p + i * 4) = pp;
    if (p16) { uint2 o; o.x = pack2bf(P[0], P[1]); o.y = pack2bf(P[2], P[3]); *(uint2*)(p16 + i * 4) = o; }
    if constexpr (EMA) {
      float* E = (float*)&ee;
#pragma unroll
      for (int e = 0; e < 4; ++e) lamb_ema_update(E[e], P[e], omd);
      *(float4*)(ema + i * 4) = ee;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
extern "C" long long medmoe_lamb_chunk(void) { return LAMB_CHUNK; }
extern "C" long long medmoe_lamb_threads(void) { return LAMB_THREADS; }
extern "C" long long medmoe_lamb_ratio_threads(void) { return LAMB_RATIO_THREADS; }
extern "C" long long medmoe_lamb_scratch_floats(long long n, long long n_segs) { return lamb_plan::scratch_floats(n, n_segs); }
// index (in floats) of the scratch slot the moments launch leaves its clip coefficient in
extern "C" long long medmoe_lamb_coef_slot(long long n, long long n_segs) { return lamb_plan::coef_slot(n, n_segs); }
// seg_end, rec_base: HOST arrays of n_segs entries; returns the number of records, -1 for a table that is not ascending or does not end at n
extern "C" long long medmoe_lamb_plan(const long long* seg_end, long long n_segs, long long n, long long* rec_base) {
  if (!seg_end || !rec_base) return -1;
  return lamb_plan::plan(seg_end, n_segs, n, rec_base);
}

template <typename GT>
static int lamb_moments_launch(const float* p, const GT* g, float* m, float* v, long long n, const long long* seg_end, const float* seg_wd,
                               const long long* rec_base, int n_segs, float* scratch, long long scratch_floats, double beta1, double beta2,
                               double eps, double weight_decay, int step, const float* grad_normsq, float max_norm, float grad_scale,
                               hipStream_t stream) {
  if (!p || !g || !m || !v || !seg_end || !seg_wd || !rec_base || !scratch || n <= 0 || n_segs < 1 || step < 1) return MM_ERR_ARG;
  if (sizeof(GT) == 2 && ((uintptr_t)g & 7)) return MM_ERR_ARG;   // 8-byte loads of the bf16 gradient
  if (((uintptr_t)p & 15) || ((uintptr_t)m & 15) || ((uintptr_t)v & 15) || ((uintptr_t)scratch & 7)) return MM_ERR_ARG;
  if (n % 4) return MM_ERR_SHAPE;                                 // flat buffers are padded to a multiple of 4 by the host
  if (scratch_floats < lamb_plan::scratch_floats(n, n_segs)) return MM_ERR_SHAPE;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  const int grid = (int)min(lamb_plan::n_chunks(n), (long long)256 * 8);
  auto kern = n_segs <= LAMB_LDS_SEGS ? lamb_moments_kernel<true, GT> : lamb_moments_kernel<false, GT>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(LAMB_THREADS), 0, stream, p, g, m, v, n, seg_end, seg_wd, rec_base, n_segs, (float2*)scratch,
                     lamb_plan::max_records(n, n_segs), (float)beta2, 1.0 - beta1, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)bc1,
                     (float)sqrt(bc2), grad_normsq, max_norm, grad_scale);
  return mm_check_launch();
}

extern "C" int medmoe_lamb_moments(const float* p, const float* g, float* m, float* v, long long n, const long long* seg_end,
                                   const float* seg_wd_mult, const long long* rec_base, int n_segs, float* scratch, long long scratch_floats,
                                   double beta1, double beta2, double eps, double weight_decay, int step, const float* grad_normsq,
                                   float max_norm, float grad_scale, hipStream_t stream) {
  return lamb_moments_launch<float>(p, g, m, v, n, seg_end, seg_wd_mult, rec_base, n_segs, scratch, scratch_floats, beta1, beta2, eps,
                                    weight_decay, step, grad_normsq, max_norm, grad_scale, stream);
}

extern "C" int medmoe_lamb_moments_g16(const float* p, const void* g_bf16, float* m, float* v, long long n, const long long* seg_end,
                                       const float* seg_wd_mult, const long long* rec_base, int n_segs, float* scratch,
                                       long long scratch_floats, double beta1, double beta2, double eps, double weight_decay, int step,
                                       const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream) {
  return lamb_moments_launch<bf16_t>(p, (const bf16_t*)g_bf16, m, v, n, seg_end, seg_wd_mult, rec_base, n_segs, scratch, scratch_floats, beta1,
                                     beta2, eps, weight_decay, step, grad_normsq, max_norm, grad_scale, stream);
}

extern "C" int medmoe_lamb_ratios(const float* scratch, long long scratch_floats, const long long* seg_end, const float* seg_wd_mult,
                                  const long long* rec_base, int n_segs, long long n, double weight_decay, int always_adapt, int trust_clip,
                                  float* ratios, hipStream_t stream) {
  if (!scratch || !seg_end || !seg_wd_mult || !rec_base || !ratios || n_segs < 1 || n <= 0) return MM_ERR_ARG;
  if (scratch_floats < lamb_plan::scratch_floats(n, n_segs)) return MM_ERR_SHAPE;
  hipLaunchKernelGGL(lamb_ratios_kernel, dim3(n_segs), dim3(LAMB_RATIO_THREADS), 0, stream, (const float2*)scratch, lamb_plan::max_records(n, n_segs), seg_end,
                     seg_wd_mult, rec_base, n_segs, (float)weight_decay, always_adapt ? 1 : 0, trust_clip ? 1 : 0, ratios);
  return mm_check_launch();
}

template <bool EMA>
static int lamb_apply_launch(float* p, const float* m, const float* v, void* p_bf16, long long n, const long long* seg_end, const float* seg_lr,
                             const float* seg_wd, int n_segs, const float* ratios, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int step, float* ema, float omd, hipStream_t stream) {
  if (!p || !m || !v || !seg_end || !seg_lr || !seg_wd || !ratios || n <= 0 || n_segs < 1 || step < 1) return MM_ERR_ARG;
  if (((uintptr_t)p & 15) || ((uintptr_t)m & 15) || ((uintptr_t)v & 15) || ((uintptr_t)p_bf16 & 7) || ((uintptr_t)ema & 15)) return MM_ERR_ARG;
  if (n % 4) return MM_ERR_SHAPE;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  const int grid = (int)min((n / 4 + 255) / 256, (long long)256 * 8);
  auto kern = n_segs <= LAMB_LDS_SEGS ? lamb_apply_kernel<true, EMA> : lamb_apply_kernel<false, EMA>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, p, m, v, (bf16_t*)p_bf16, n, seg_end, seg_lr, seg_wd, n_segs, ratios, (float)lr,
                     (float)eps, (float)weight_decay, (float)bc1, (float)sqrt(bc2), ema, omd);
  return mm_check_launch();
}

extern "C" int medmoe_lamb_apply(float* p, const float* m, const float* v, void* p_bf16, long long n, const long long* seg_end,
                                 const float* seg_lr_mult, const float* seg_wd_mult, int n_segs, const float* ratios, double lr, double beta1,
                                 double beta2, double eps, double weight_decay, int step, hipStream_t stream) {
  return lamb_apply_launch<false>(p, m, v, p_bf16, n, seg_end, seg_lr_mult, seg_wd_mult, n_segs, ratios, lr, beta1, beta2, eps, weight_decay,
                                  step, nullptr, 0.f, stream);
}

extern "C" int medmoe_lamb_apply_ema(float* p, const float* m, const float* v, void* p_bf16, long long n, const long long* seg_end,
                                     const float* seg_lr_mult, const float* seg_wd_mult, int n_segs, const float* ratios, double lr,
                                     double beta1, double beta2, double eps, double weight_decay, int step, float* ema,
                                     float one_minus_decay, hipStream_t stream) {
  if (!ema || !(one_minus_decay >= 0.f && one_minus_decay <= 1.f)) return MM_ERR_ARG;
  return lamb_apply_launch<true>(p, m, v, p_bf16, n, seg_end, seg_lr_mult, seg_wd_mult, n_segs, ratios, lr, beta1, beta2, eps, weight_decay,
                                 step, ema, one_minus_decay, stream);
}
