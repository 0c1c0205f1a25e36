// Optimizer-side kernels (HBM-bound): global grad-norm, clip + Adam on the flat fp32 master
// buffer (torch.optim.Adam semantics: L2 weight decay added to the gradient; reference settings
// configs/model/med-moe_pretraining.yaml:7-11, clip 0.25 configs/experiment/pretraining_medmoe.yaml:23),
// fused bf16 down-cast of the updated weights, batched bf16 transposes (dgrad reads W^T), casts.
#include "common.h"

// The gradient operand of the clip norm and of Adam is either the arena's fp32 gradient or, after a bf16 gradient exchange, the
// reduced bf16 buffer.  The kernels below are templates on its element type and differ in these loads alone: one float4 of gradients
// (16 bytes of fp32, or 8 bytes of bf16 widened, element order kept: lo half first) and the scalar form for a tail.  The fp32
// instantiations are the kernels as they were; a bf16 instantiation computes what the fp32 one computes on float(g_bf16), bit for bit.
__device__ __forceinline__ float4 bf16x4_to_float4(uint2 r) {
  float4 v;
  v.x = __uint_as_float(r.x << 16); v.y = __uint_as_float(r.x & 0xffff0000u);
  v.z = __uint_as_float(r.y << 16); v.w = __uint_as_float(r.y & 0xffff0000u);
  return v;
}
__device__ __forceinline__ float4 grad4(const float* g, long long i) { return *(const float4*)(g + i * 4); }
__device__ __forceinline__ float4 grad4(const bf16_t* g, long long i) { return bf16x4_to_float4(*(const uint2*)(g + i * 4)); }
__device__ __forceinline__ float grad1(const float* g, long long i) { return g[i]; }
__device__ __forceinline__ float grad1(const bf16_t* g, long long i) { return bf2f(g[i]); }

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long long n, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  const long long n4 = n >> 2;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 v = *(const float4*)(g + i * 4);
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (long long i = n4 * 4; i < n; ++i) s += g[i] * g[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

extern "C" int medmoe_sumsq(const float* g, long long n, float* out, hipStream_t stream) {
  if (!g || !out || n <= 0) return MM_ERR_ARG;
  const int grid = (int)min((n / 4 + 255) / 256 + 1, (long long)2048);
  if (grid > 1) ++g_mm_nondet;
  hipLaunchKernelGGL(sumsq_kernel, dim3(grid), dim3(256), 0, stream, g, n, out);
  return mm_check_launch();
}

// Deterministic sum of squares: out[0] = sum g^2 with a FIXED summation order (per-block partials to scratch, the last
// block to arrive adds them in index order).  The atomicAdd form above depends on block arrival order in its last
// bits; with data parallelism every rank would clip with a slightly different coefficient and the replicas' weights
// would drift apart step by step (found with tools/two_rank_gpu.py: reduced gradients bit-identical, weights not).
// scratch: >= 2049 floats, scratch[2048] (an arrival counter) must be 0 on entry and is 0 again on exit.
template <typename GT>
__global__ __launch_bounds__(256) void sumsq_det_kernel(const GT* __restrict__ g, long long n, float* __restrict__ out,
                                                       float* __restrict__ scratch) {
  __shared__ float red[4];
  __shared__ int last;
  float s = 0.f;
  const long long n4 = n >> 2;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 v = grad4(g, i);
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (long long i = n4 * 4; i < n; ++i) s += grad1(g, i) * grad1(g, i);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    scratch[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    __threadfence();
    const unsigned t = atomicAdd((unsigned*)(scratch + 2048), 1u);
    last = (t == gridDim.x - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  float a = 0.f;
  if (threadIdx.x < 64) {
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 64) a += __builtin_nontemporal_load(scratch + i);
    a = wave_sum(a);
    if (threadIdx.x == 0) { out[0] = a; *(unsigned*)(scratch + 2048) = 0u; }
  }
}

extern "C" int medmoe_sumsq_det(const float* g, long long n, float* out, float* scratch, hipStream_t stream) {
  if (!g || !out || !scratch || n <= 0) return MM_ERR_ARG;
  const int grid = (int)min((n / 4 + 255) / 256 + 1, (long long)2048);
  hipLaunchKernelGGL(sumsq_det_kernel<float>, dim3(grid), dim3(256), 0, stream, g, n, out, scratch);
  return mm_check_launch();
}

// clip coefficient = min(1, max_norm / (sqrt(normsq) + 1e-6))  (torch.nn.utils.clip_grad_norm_).
// Update in torch.optim.Adam's operation order (exp_avg.lerp_, exp_avg_sq.mul_().addcmul_(), sqrt / sqrt(bc2) + eps,
// addcdiv_ with step size lr / bc1); the scalars 1-b1, 1-b2, sqrt(bc2), lr/bc1 are formed in double on the host, as torch
// forms them in Python floats (1 - 0.999f in fp32 is off by 1.3e-5 relative: the second moment would inherit that).
// One element of the update, shared by adam_kernel and adam_groups_kernel so that both compile the same expressions (operation order and
// the contraction the compiler applies to them): `wd` is the L2 decay added to the gradient, 0 for the decoupled form.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float coef, float wd, float b2, float omb1, float omb2,
                                            float eps, float step_size, float bc2_sqrt) {
  const float gr = g * coef + wd * p;
  m = m + omb1 * (gr - m);
  v = b2 * v + omb2 * gr * gr;
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p -= step_size * (m / denom);
}

// Weight EMA inside the Adam launch.  The EMA = true instantiations of the two kernels below take two more arguments, `float* ema`
// (fp32, the arena's layout) and `float omd` (1 - decay of this update, formed on the host), and average the parameter they have just
// updated while it is in registers: E <- fadd_rn(E, fmul_rn(omd, fsub_rn(P, E))).  Three separately rounded fp32 operations: the contraction
// HIP applies by default is switched off for this one expression (the __f*_rn intrinsics are plain operators that it would still fuse), so
// torch's e + omd * (p - e) in fp32 reproduces it bit for bit.  The average is moved as whole float4s next to p, m, v: 8 B/param on top of
// the launch's 34.  The EMA = false instantiations have no such arguments and are the kernels as they were.
__device__ __forceinline__ void ema_update(float& e, float p, float omd) {
#pragma clang fp contract(off)
  const float d = p - e;
  const float s = omd * d;
  e = e + s;
}
__device__ __forceinline__ float* ema_ptr() { return nullptr; }
__device__ __forceinline__ float* ema_ptr(float* ema, float) { return ema; }
__device__ __forceinline__ float ema_omd() { return 0.f; }
__device__ __forceinline__ float ema_omd(float*, float omd) { return omd; }

template <typename GT, bool EMA = false, typename... EA>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, bf16_t* __restrict__ p16, long long n,
                                                   float b2, float omb1, float omb2, float eps, float wd, float step_size,
                                                   float bc2_sqrt, const float* __restrict__ normsq, float max_norm,
                                                   float grad_scale, EA... ema_args) {
  static_assert(sizeof...(EA) == (EMA ? 2 : 0), "EMA = true: (float* ema, float omd) behind grad_scale; EMA = false: nothing");
  float* __restrict__ const ema = ema_ptr(ema_args...);
  const float omd = ema_omd(ema_args...);
  float coef = grad_scale;
  if (normsq && max_norm > 0.f) {
    const float nrm = sqrtf(*normsq) * grad_scale;
    coef *= fminf(1.f, max_norm / (nrm + 1e-6f));
  }
  const long long n4 = n >> 2;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 pp = *(float4*)(p + i * 4);
    const float4 gg = grad4(g, i);
    float4 mm = *(float4*)(m + i * 4), vv = *(float4*)(v + i * 4);
    float* P = (float*)&pp; const float* G = (const float*)&gg; float* M = (float*)&mm; float* V = (float*)&vv;
    float4 ee;
    if constexpr (EMA) ee = *(const float4*)(ema + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) adam_update(P[e], G[e], M[e], V[e], coef, wd, b2, omb1, omb2, eps, step_size, bc2_sqrt);
    *(float4*)(p + i * 4) = pp; *(float4*)(m + i * 4) = mm; *(float4*)(v + i * 4) = vv;
    if (p16) { uint2 o; o.x = pack2bf(P[0], P[1]); o.y = pack2bf(P[2], P[3]); *(uint2*)(p16 + i * 4) = o; }
    if constexpr (EMA) {
      float* E = (float*)&ee;
#pragma unroll
      for (int e = 0; e < 4; ++e) ema_update(E[e], P[e], omd);
      *(float4*)(ema + i * 4) = ee;
    }
  }
}

// Host side of the plain step, shared by the fp32 / bf16 gradient and the EMA forms: `ea` is empty, or (ema, one_minus_decay).
template <typename GT, bool EMA, typename... EA>
static int adam_launch(float* p, const GT* g, float* m, float* v, void* p_bf16, long long n, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int step, const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream, EA... ea) {
  if (!p || !g || !m || !v || n <= 0 || step < 1) return MM_ERR_ARG;
  if (sizeof(GT) == 2 && ((uintptr_t)g & 7)) return MM_ERR_ARG;  // 8-byte loads of the bf16 gradient
  if (n % 4) return MM_ERR_SHAPE;   // flat buffers are padded to a multiple of 4 by the host
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  const int grid = (int)min((n / 4 + 255) / 256, (long long)256 * 8);
  hipLaunchKernelGGL((adam_kernel<GT, EMA, EA...>), dim3(grid), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, n, (float)beta2,
                     (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)(lr / bc1),
                     (float)sqrt(bc2), grad_normsq, max_norm, grad_scale, ea...);
  return mm_check_launch();
}

// The average's arguments: a buffer, and 1 - decay in [0, 1] (0 leaves the average as it is).
static bool ema_args_ok(const float* ema, float one_minus_decay) { return ema && one_minus_decay >= 0.f && one_minus_decay <= 1.f; }

extern "C" int medmoe_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, double lr,
                                double beta1, double beta2, double eps, double weight_decay, int step,
                                const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream) {
  return adam_launch<float, false>(p, g, m, v, p_bf16, n, lr, beta1, beta2, eps, weight_decay, step, grad_normsq, max_norm, grad_scale, stream);
}

extern "C" int medmoe_adam_step_ema(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, double lr,
                                    double beta1, double beta2, double eps, double weight_decay, int step,
                                    const float* grad_normsq, float max_norm, float grad_scale, float* ema, float one_minus_decay,
                                    hipStream_t stream) {
  if (!ema_args_ok(ema, one_minus_decay)) return MM_ERR_ARG;
  return adam_launch<float, true>(p, g, m, v, p_bf16, n, lr, beta1, beta2, eps, weight_decay, step, grad_normsq, max_norm, grad_scale, stream,
                                  ema, one_minus_decay);
}

// ---------------------------------------------------------------------------------------------
// The same step with parameter groups.  The arena is cut into `n_runs` contiguous runs (run r = elements [run_end[r-1], run_end[r]),
// run_end ascending, run_end[n_runs-1] == n); run r steps with step_size * lr_mult[r] and decays with wd * wd_mult[r].  decoupled = 0:
// adam_kernel's update (L2 decay added to the gradient); decoupled = 1: torch.optim.AdamW's single-tensor order, p *= 1 - lr_r * wd_r
// (formed in double and rounded once, as torch forms the Python float it hands to mul_), then Adam on the undecayed gradient.
// The table is static between regroupings and lives on the device; a workgroup stages it in LDS (up to ADAM_LDS_RUNS runs, larger tables
// are searched where they are: a few KB that stay in the caches) and every lane finds the run of its float4's first element by bisection.
// A run boundary may fall on any element (the members of an arena group are stored back to back), so the run is followed per element
// inside the float4; the four arrays are still moved 16 bytes per lane.  No atomics: the result is a function of the inputs only.
// ---------------------------------------------------------------------------------------------
#define ADAM_LDS_RUNS 1024

template <bool LDS, typename GT, bool EMA = false, typename... EA>
__global__ __launch_bounds__(256) void adam_groups_kernel(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, bf16_t* __restrict__ p16, long long n,
                                                          const long long* __restrict__ run_end, const float* __restrict__ run_lr,
                                                          const float* __restrict__ run_wd, int n_runs, float b2, float omb1, float omb2,
                                                          float eps, float wd, float step_size, float bc2_sqrt, double lr_d, double wd_d,
                                                          int decoupled, const float* __restrict__ normsq, float max_norm,
                                                          float grad_scale, EA... ema_args) {
  static_assert(sizeof...(EA) == (EMA ? 2 : 0), "EMA = true: (float* ema, float omd) behind grad_scale; EMA = false: nothing");
  float* __restrict__ const ema = ema_ptr(ema_args...);
  const float omd = ema_omd(ema_args...);
  __shared__ long long s_end[LDS ? ADAM_LDS_RUNS : 1];
  __shared__ float s_lr[LDS ? ADAM_LDS_RUNS : 1], s_wd[LDS ? ADAM_LDS_RUNS : 1];
  if (LDS) {
    for (int r = threadIdx.x; r < n_runs; r += 256) { s_end[r] = run_end[r]; s_lr[r] = run_lr[r]; s_wd[r] = run_wd[r]; }
    __syncthreads();
  }
  const long long* ends = LDS ? s_end : run_end;
  const float* lrm = LDS ? s_lr : run_lr;
  const float* wdm = LDS ? s_wd : run_wd;
  float coef = grad_scale;
  if (normsq && max_norm > 0.f) {
    const float nrm = sqrtf(*normsq) * grad_scale;
    coef *= fminf(1.f, max_norm / (nrm + 1e-6f));
  }
  const int last = n_runs - 1;
  const long long n4 = n >> 2;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 pp = *(float4*)(p + i * 4);
    const float4 gg = grad4(g, i);
    float4 mm = *(float4*)(m + i * 4), vv = *(float4*)(v + i * 4);
    float* P = (float*)&pp; const float* G = (const float*)&gg; float* M = (float*)&mm; float* V = (float*)&vv;
    float4 ee;
    if constexpr (EMA) ee = *(const float4*)(ema + i * 4);
    const long long e0 = i * 4;
    int r = 0, hi = last;                                         // first run whose end lies behind e0 (r <= last whatever the table holds)
    while (r < hi) {
      const int mid = (r + hi) >> 1;
      if (ends[mid] > e0) hi = mid; else r = mid + 1;
    }
    long long end = ends[r];
    float ss = step_size * lrm[r], wdr = wd * wdm[r], keep = 1.f;
    if (decoupled) { keep = (float)(1.0 - (lr_d * (double)lrm[r]) * (wd_d * (double)wdm[r])); wdr = 0.f; }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e0 + e >= end && r < last) {                            // a boundary inside this float4: move on (runs may be one element long)
        do { ++r; end = ends[r]; } while (e0 + e >= end && r < last);
        ss = step_size * lrm[r]; wdr = wd * wdm[r];
        if (decoupled) { keep = (float)(1.0 - (lr_d * (double)lrm[r]) * (wd_d * (double)wdm[r])); wdr = 0.f; }
      }
      if (decoupled) P[e] *= keep;
      adam_update(P[e], G[e], M[e], V[e], coef, wdr, b2, omb1, omb2, eps, ss, bc2_sqrt);
    }
    *(float4*)(p + i * 4) = pp; *(float4*)(m + i * 4) = mm; *(float4*)(v + i * 4) = vv;
    if (p16) { uint2 o; o.x = pack2bf(P[0], P[1]); o.y = pack2bf(P[2], P[3]); *(uint2*)(p16 + i * 4) = o; }
    if constexpr (EMA) {
      float* E = (float*)&ee;
#pragma unroll
      for (int e = 0; e < 4; ++e) ema_update(E[e], P[e], omd);
      *(float4*)(ema + i * 4) = ee;
    }
  }
}

template <typename GT, bool EMA, typename... EA>
static int adam_groups_launch(float* p, const GT* g, float* m, float* v, void* p_bf16, long long n, const long long* run_end,
                              const float* run_lr_mult, const float* run_wd_mult, int n_runs, double lr, double beta1, double beta2, double eps,
                              double weight_decay, int decoupled, int step, const float* grad_normsq, float max_norm, float grad_scale,
                              hipStream_t stream, EA... ea) {
  if (!p || !g || !m || !v || !run_end || !run_lr_mult || !run_wd_mult || n <= 0 || n_runs < 1 || step < 1) return MM_ERR_ARG;
  if (sizeof(GT) == 2 && ((uintptr_t)g & 7)) return MM_ERR_ARG;  // 8-byte loads of the bf16 gradient
  if (n % 4) return MM_ERR_SHAPE;   // flat buffers are padded to a multiple of 4 by the host
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  const int grid = (int)min((n / 4 + 255) / 256, (long long)256 * 8);
  auto kern = n_runs <= ADAM_LDS_RUNS ? adam_groups_kernel<true, GT, EMA, EA...> : adam_groups_kernel<false, GT, EMA, EA...>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, n, run_end, run_lr_mult, run_wd_mult, n_runs,
                     (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)(lr / bc1),
                     (float)sqrt(bc2), lr, weight_decay, decoupled ? 1 : 0, grad_normsq, max_norm, grad_scale, ea...);
  return mm_check_launch();
}

extern "C" int medmoe_adam_groups_step(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, const long long* run_end,
                                       const float* run_lr_mult, const float* run_wd_mult, int n_runs, double lr, double beta1,
                                       double beta2, double eps, double weight_decay, int decoupled, int step, const float* grad_normsq,
                                       float max_norm, float grad_scale, hipStream_t stream) {
  return adam_groups_launch<float, false>(p, g, m, v, p_bf16, n, run_end, run_lr_mult, run_wd_mult, n_runs, lr, beta1, beta2, eps, weight_decay,
                                          decoupled, step, grad_normsq, max_norm, grad_scale, stream);
}

extern "C" int medmoe_adam_groups_step_ema(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, const long long* run_end,
                                           const float* run_lr_mult, const float* run_wd_mult, int n_runs, double lr, double beta1,
                                           double beta2, double eps, double weight_decay, int decoupled, int step, const float* grad_normsq,
                                           float max_norm, float grad_scale, float* ema, float one_minus_decay, hipStream_t stream) {
  if (!ema_args_ok(ema, one_minus_decay)) return MM_ERR_ARG;
  return adam_groups_launch<float, true>(p, g, m, v, p_bf16, n, run_end, run_lr_mult, run_wd_mult, n_runs, lr, beta1, beta2, eps, weight_decay,
                                         decoupled, step, grad_normsq, max_norm, grad_scale, stream, ema, one_minus_decay);
}

// ---------------------------------------------------------------------------------------------
// bf16 gradient exchange: the rank-local fp32 gradient is scaled by 1 / world and rounded to bf16 on the chip (grad_pack), the
// bf16 buffer is all-reduced, and the clip norm and Adam read the reduced bf16 gradient where it lies - no pass widens it back to fp32.
// No atomics besides sumsq's arrival counter, nothing read from the host: every result is a function of the inputs only.
// ---------------------------------------------------------------------------------------------
// out[i] = bf16_rne(g[i] * scale), the product formed in fp32 (as DDP's bf16_compress_hook divides before it rounds).  8 elements per lane
// and iteration: two 16-byte loads, one 16-byte store; 6 B of HBM traffic per element.
__global__ __launch_bounds__(256) void grad_pack_bf16_kernel(const float* __restrict__ g, bf16_t* __restrict__ out, long long n, float scale) {
  const long long n8 = n >> 3;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    const float4 a = *(const float4*)(g + i * 8), b = *(const float4*)(g + i * 8 + 4);
    uint4 o;
    o.x = pack2bf(a.x * scale, a.y * scale); o.y = pack2bf(a.z * scale, a.w * scale);
    o.z = pack2bf(b.x * scale, b.y * scale); o.w = pack2bf(b.z * scale, b.w * scale);
    *(uint4*)(out + i * 8) = o;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (long long i = n8 * 8; i < n; ++i) out[i] = f2bf(g[i] * scale);
}

extern "C" int medmoe_grad_pack_bf16(const float* g, void* out_bf16, long long n, float scale, hipStream_t stream) {
  if (!g || !out_bf16 || n <= 0) return MM_ERR_ARG;
  if (((uintptr_t)g & 15) || ((uintptr_t)out_bf16 & 15)) return MM_ERR_ARG;   // bucket offsets are multiples of 8 elements of a 16-byte aligned arena
  const int grid = (int)min((n / 8 + 255) / 256 + 1, (long long)256 * 8);
  hipLaunchKernelGGL(grad_pack_bf16_kernel, dim3(grid), dim3(256), 0, stream, g, (bf16_t*)out_bf16, n, scale);
  return mm_check_launch();
}

// sumsq_det_kernel's bf16 instantiation: the same grid, the same elements per thread in the same order, the same expressions and the same
// partial-sum tree, so the result is bit-identical to medmoe_sumsq_det on the fp32 up-cast of the buffer (tests pin it with torch.equal).
extern "C" int medmoe_sumsq_det_bf16(const void* g_bf16, long long n, float* out, float* scratch, hipStream_t stream) {
  if (!g_bf16 || !out || !scratch || n <= 0) return MM_ERR_ARG;
  if ((uintptr_t)g_bf16 & 7) return MM_ERR_ARG;                   // 8-byte loads
  const int grid = (int)min((n / 4 + 255) / 256 + 1, (long long)2048);
  hipLaunchKernelGGL(sumsq_det_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)g_bf16, n, out, scratch);
  return mm_check_launch();
}

// adam_kernel / adam_groups_kernel instantiated on the bf16 gradient (8 bytes per float4 of parameters: 32 B/param instead of 34, and no
// 6 B/param widening pass before them).  One loop body and one adam_update for both element types: the step is bit-identical to the
// fp32-gradient step on float(g_bf16).
extern "C" int medmoe_adam_step_g16(float* p, const void* g_bf16, float* m, float* v, void* p_bf16, long long n, double lr,
                                    double beta1, double beta2, double eps, double weight_decay, int step,
                                    const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream) {
  return adam_launch<bf16_t, false>(p, (const bf16_t*)g_bf16, m, v, p_bf16, n, lr, beta1, beta2, eps, weight_decay, step, grad_normsq, max_norm,
                                    grad_scale, stream);
}

extern "C" int medmoe_adam_step_ema_g16(float* p, const void* g_bf16, float* m, float* v, void* p_bf16, long long n, double lr,
                                        double beta1, double beta2, double eps, double weight_decay, int step,
                                        const float* grad_normsq, float max_norm, float grad_scale, float* ema, float one_minus_decay,
                                        hipStream_t stream) {
  if (!ema_args_ok(ema, one_minus_decay)) return MM_ERR_ARG;
  return adam_launch<bf16_t, true>(p, (const bf16_t*)g_bf16, m, v, p_bf16, n, lr, beta1, beta2, eps, weight_decay, step, grad_normsq, max_norm,
                                   grad_scale, stream, ema, one_minus_decay);
}

extern "C" int medmoe_adam_groups_step_g16(float* p, const void* g_bf16, float* m, float* v, void* p_bf16, long long n,
                                           const long long* run_end, const float* run_lr_mult, const float* run_wd_mult, int n_runs,
                                           double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, int step,
                                           const float* grad_normsq, float max_norm, float grad_scale, hipStream_t stream) {
  return adam_groups_launch<bf16_t, false>(p, (const bf16_t*)g_bf16, m, v, p_bf16, n, run_end, run_lr_mult, run_wd_mult, n_runs, lr, beta1, beta2,
                                           eps, weight_decay, decoupled, step, grad_normsq, max_norm, grad_scale, stream);
}

extern "C" int medmoe_adam_groups_step_ema_g16(float* p, const void* g_bf16, float* m, float* v, void* p_bf16, long long n,
                                               const long long* run_end, const float* run_lr_mult, const float* run_wd_mult, int n_runs,
                                               double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                                               int step, const float* grad_normsq, float max_norm, float grad_scale, float* ema,
                                               float one_minus_decay, hipStream_t stream) {
  if (!ema_args_ok(ema, one_minus_decay)) return MM_ERR_ARG;
  return adam_groups_launch<bf16_t, true>(p, (const bf16_t*)g_bf16, m, v, p_bf16, n, run_end, run_lr_mult, run_wd_mult, n_runs, lr, beta1, beta2,
                                          eps, weight_decay, decoupled, step, grad_normsq, max_norm, grad_scale, stream, ema, one_minus_decay);
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ s, bf16_t* __restrict__ d, long long n) {
  const long long n4 = n >> 2;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 v = *(const float4*)(s + i * 4);
    uint2 o; o.x = pack2bf(v.x, v.y); o.y = pack2bf(v.z, v.w);
    *(uint2*)(d + i * 4) = o;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (long long i = n4 * 4; i < n; ++i) d[i] = f2bf(s[i]);
}

extern "C" int medmoe_cast_bf16(const float* src, void* dst, long long n, hipStream_t stream) {
  if (!src || !dst || n <= 0) return MM_ERR_ARG;
  const int grid = (int)min((n / 4 + 255) / 256 + 1, (long long)256 * 8);
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid), dim3(256), 0, stream, src, (bf16_t*)dst, n);
  return mm_check_launch();
}

// batched 2-D transposes: table[i] = {src_off, dst_off, rows, cols} (element offsets into the flat
// bf16 buffers); dst[c][r] = src[r][c].  grid = (n_entries, max 64x64 tiles per entry).
__global__ __launch_bounds__(256) void transpose_many_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                             const long long* __restrict__ table) {
  // 64 x 64 tile through LDS.  Both global sides move 16 bytes per lane (8 consecutive bf16 of a source row in, 8 consecutive bf16 of a
  // destination row out) whenever the tile is whole and the pitches are multiples of 8; the 2-byte path covers the ragged edges.
  __shared__ bf16_t tile[64][72];
  const long long so = table[blockIdx.x * 4 + 0], doff = table[blockIdx.x * 4 + 1];
  const int rows = (int)table[blockIdx.x * 4 + 2], cols = (int)table[blockIdx.x * 4 + 3];
  const int tc = (cols + 63) / 64, tr = (rows + 63) / 64;
  if ((int)blockIdx.y >= tc * tr) return;
  const int r0 = (blockIdx.y / tc) * 64, c0 = (blockIdx.y % tc) * 64;
  const bool whole = r0 + 64 <= rows && c0 + 64 <= cols && !(rows & 7) && !(cols & 7) && !(so & 7) && !(doff & 7);
  if (whole) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ch = t + i * 256, r = ch >> 3, c8 = (ch & 7) * 8;
      *(uint4*)&tile[r][c8] = *(const uint4*)(src + so + (long long)(r0 + r) * cols + c0 + c8);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ch = t + i * 256, c = ch >> 3, r8 = (ch & 7) * 8;       // destination row c0 + c, its columns r0 + r8 .. + 7
      bf16_t v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = tile[r8 + q][c];
      *(uint4*)(dst + doff + (long long)(c0 + c) * rows + r0 + r8) = *(const uint4*)v;
    }
    return;
  }
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4)
    if (r0 + r < rows && c0 + tx < cols) tile[r][tx] = src[so + (long long)(r0 + r) * cols + c0 + tx];
  __syncthreads();
  for (int c = ty; c < 64; c += 4)
    if (c0 + c < cols && r0 + tx < rows) dst[doff + (long long)(c0 + c) * rows + r0 + tx] = tile[tx][c];
}

extern "C" int medmoe_transpose_many(const void* src, void* dst, const long long* table, int n_entries,
                                     int max_tiles, hipStream_t stream) {
  if (!src || !dst || !table || n_entries <= 0 || max_tiles <= 0) return MM_ERR_ARG;
  hipLaunchKernelGGL(transpose_many_kernel, dim3(n_entries, max_tiles), dim3(256), 0, stream, (const bf16_t*)src,
                     (bf16_t*)dst, table);
  return mm_check_launch();
}

// ---------------------------------------------------------------------------------------------
// Stream ordering helper for hosts that schedule two streams by hand (the weight-gradient GEMMs of a backward run on a second stream
// underneath the dgrad chain): `to` waits for everything enqueued on `from` so far.  One hipEventRecord + hipStreamWaitEvent on an event
// from a small ring (a wait captures the event's state when it is enqueued, so re-recording a ring slot later does not disturb it) - the
// same two calls torch.cuda.Event.record / Stream.wait_event make, without ~20 us of Python per fork at a hundred forks per step.
// ---------------------------------------------------------------------------------------------
extern "C" int medmoe_stream_fork(hipStream_t from, hipStream_t to) {
  static hipEvent_t ring[32];
  static int dev_of[32];
  static bool made[32];
  static unsigned next = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return MM_ERR_LAUNCH;
  const unsigned slot = next++ & 31u;
  if (made[slot] && dev_of[slot] != dev) { (void)hipEventDestroy(ring[slot]); made[slot] = false; }
  if (!made[slot]) {
    if (hipEventCreateWithFlags(&ring[slot], hipEventDisableTiming) != hipSuccess) return MM_ERR_LAUNCH;
    made[slot] = true; dev_of[slot] = dev;
  }
  if (hipEventRecord(ring[slot], from) != hipSuccess) return MM_ERR_LAUNCH;
  if (hipStreamWaitEvent(to, ring[slot], 0) != hipSuccess) return MM_ERR_LAUNCH;
  return MM_OK;
}
