// Fused flat-bucket SGD (Nesterov momentum) and the GradScaler device-side kernels.
//
// Replaces `optim.SGD(params, lr, weight_decay, momentum=0.9, nesterov=True).step()`
// (reference src/ddp/trainer.py:92-98, 158/165) and the AMP helpers behind
// `GradScaler.step/update` (main.py:25, trainer.py:157-159). torch.optim.SGD, dampening 0:
//     d = g + wd*p ; buf = mu*buf + d   (first step: buf = d) ; d = d + mu*buf ; p -= lr*d
// The first-step special case needs no flag: buffers start at zero and mu*0 + d == d exactly.
// GradScaler semantics (torch._amp_update_scale_): a step whose gradients hold inf/NaN is
// skipped entirely; scale *= backoff on overflow, *= growth after `interval` clean steps.
// The step also refreshes the bf16 shadow of every parameter (the GEMM operand layout).
#include "flat.h"
#include "kernels.h"

namespace dtc {

__global__ void __launch_bounds__(256) sgd_nesterov_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, u16* __restrict__ pb, int64_t n4,
                                                          float lr, float wd, float mu,
                                                          const float* __restrict__ inv_scale,
                                                          const int* __restrict__ found_inf) {
  if (found_inf && *found_inf) return;  // GradScaler: skip the whole step
  const float is = inv_scale ? *inv_scale : 1.f;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 pv = *(const f32x4*)(p + i * 4);
    const f32x4 gv = *(const f32x4*)(g + i * 4);
    f32x4 mv = *(const f32x4*)(m + i * 4);
    momentum_step<true>(pv, mv, gv * is + pv * wd, mu, lr);
    *(f32x4*)(p + i * 4) = pv;
    *(f32x4*)(m + i * 4) = mv;
    store_bf16x4(pb + i * 4, pv);
  }
}

int sgd_nesterov(float* p, const float* g, float* mom, u16* p_bf16, int64_t n, float lr, float wd, float mu,
                 const float* inv_scale, const int* found_inf, hipStream_t st) {
  DTC_CHECK_ARG(p && g && mom && p_bf16 && mult4(n), "sgd_nesterov: bad args (n=%lld)", (long long)n);
  DTC_CHECK_ARG(aligned(p, 16) && aligned(g, 16) && aligned(mom, 16) && aligned(p_bf16, 8),
                "sgd_nesterov: p, g and momentum must be 16-byte aligned, p_bf16 8-byte aligned");
  const int64_t n4 = n / 4;
  const int blocks = flat_blocks(n4, 256, 2048);
  DTC_KLAUNCH(sgd_nesterov_kernel, dim3(blocks), dim3(256), 0, st, p, g, mom, p_bf16, n4, lr, wd, mu, inv_scale,
                     found_inf);
  DTC_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- Adam / AdamW
// torch.optim.Adam / AdamW (amsgrad=False, maximize=False), per element and in torch's own operation order
// (_single_tensor_adam):
//     g' = g * gmul ;  Adam: g' += wd*p ;  AdamW: p *= 1 - lr*wd
//     m += (g' - m)*(1-b1) ;  v = b2*v + (1-b2)*g'*g'
//     p -= (lr/bc1) * (m / (sqrt(v)/sqrt(bc2) + eps)),   bc1 = 1 - b1^t, bc2 = 1 - b2^t
// The step count t lives in a small device record (AdamState): a GradScaler-skipped step must not advance it,
// and the host cannot know about a skip without a synchronisation. A one-thread "tick" launch ahead of the
// update advances t (unless *found_inf) and writes the two factors that depend on it, computed in double
// as torch's Python scalars are; the update launch only reads the record, so no block can see it half
// written (stream order separates the two launches). Two launches per step, no host synchronisation.
struct AdamState {
  int step;         // completed (non-skipped) steps
  float step_size;  // lr / bc1
  float bc2_sqrt;   // sqrt(bc2)
  int reserved;
};
static_assert(sizeof(AdamState) == 4 * DTC_ADAM_STATE_WORDS, "AdamState is DTC_ADAM_STATE_WORDS 32-bit words");

// b^t by squaring, in double: at most 62 multiplications (1 - b^t within 2e-14 of pow()'s, invisible once
// the factors are rounded to float), a fraction of the time of two library pow() calls in a one-thread kernel
__device__ __forceinline__ double pow_int(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

__global__ void adam_tick_kernel(AdamState* __restrict__ s, double lr, double b1, double b2,
                                 const int* __restrict__ found_inf) {
  if (found_inf && *found_inf) return;
  const int t = s->step + 1;
  s->step = t;
  s->step_size = (float)(lr / (1.0 - pow_int(b1, t)));
  s->bc2_sqrt = (float)sqrt(1.0 - pow_int(b2, t));
}

// omb1 = 1-b1, omb2 = 1-b2, decay = 1 - lr*wd are formed in double by the launcher: 1.f - 0.999f is
// 0.00100004673, 4.7e-5 off, an order of magnitude more than the whole update's fp32 error.
template <bool DECOUPLED>
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   u16* __restrict__ pb, int64_t n4,
                                                   const AdamState* __restrict__ state, float omb1, float b2,
                                                   float omb2, float eps, float wd, float decay,
                                                   const float* __restrict__ inv_scale,
                                                   const int* __restrict__ found_inf) {
  if (found_inf && *found_inf) return;  // GradScaler: skip the whole step (the tick skipped it too)
  const float is = inv_scale ? *inv_scale : 1.f;
  const float step_size = state->step_size, bc2_sqrt = state->bc2_sqrt;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 pv = *(const f32x4*)(p + i * 4);
    f32x4 gv = *(const f32x4*)(g + i * 4) * is;
    f32x4 mv = *(const f32x4*)(m + i * 4);
    f32x4 vv = *(const f32x4*)(v + i * 4);
    if (DECOUPLED) pv = pv * decay;
    else gv = gv + pv * wd;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // the roundings of torch's CPU kernels: lerp_ is one fused multiply-add, addcmul_ another on mul_'s result
      mv[k] = fmaf(gv[k] - mv[k], omb1, mv[k]);
      vv[k] = fmaf(omb2 * gv[k], gv[k], vv[k] * b2);
      pv[k] -= step_size * (mv[k] / (sqrtf(vv[k]) / bc2_sqrt + eps));
    }
    *(f32x4*)(p + i * 4) = pv;
    *(f32x4*)(m + i * 4) = mv;
    *(f32x4*)(v + i * 4) = vv;
    store_bf16x4(pb + i * 4, pv);
  }
}

int adam_flat(float* p, const float* g, float* m, float* v, u16* p_bf16, int64_t n, void* state, double lr,
              double beta1, double beta2, double eps, double wd, int decoupled, const float* inv_scale,
              const int* found_inf, hipStream_t st) {
  DTC_CHECK_ARG(p && g && m && v && p_bf16 && state, "adam_flat: null pointer");
  DTC_CHECK_ARG(mult4(n), "adam_flat: n = %lld must be a positive multiple of 4", (long long)n);
  DTC_CHECK_ARG(aligned(p, 16) && aligned(g, 16) && aligned(m, 16) && aligned(v, 16) && aligned(p_bf16, 8) &&
                    aligned(state, 16),
                "adam_flat: p, g, m, v and state must be 16-byte aligned, p_bf16 8-byte aligned");
  DTC_CHECK_ARG(eps > 0.0, "adam_flat: eps = %g must be positive", eps);
  DTC_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
                "adam_flat: betas (%g, %g) must lie in [0, 1)", beta1, beta2);
  DTC_CHECK_ARG(lr >= 0.0 && wd >= 0.0, "adam_flat: lr = %g and weight_decay = %g must not be negative", lr, wd);
  const int64_t n4 = n / 4;
  const int blocks = flat_blocks(n4, 256, 2048);
  DTC_KLAUNCH(adam_tick_kernel, dim3(1), dim3(1), 0, st, (AdamState*)state, lr, beta1, beta2, found_inf);
  const float omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
  const float decay = (float)(1.0 - lr * wd);
  if (decoupled)
    DTC_KLAUNCH(adam_kernel<true>, dim3(blocks), dim3(256), 0, st, p, g, m, v, p_bf16, n4, (const AdamState*)state,
                omb1, b2, omb2, (float)eps, (float)wd, decay, inv_scale, found_inf);
  else
    DTC_KLAUNCH(adam_kernel<false>, dim3(blocks), dim3(256), 0, st, p, g, m, v, p_bf16, n4, (const AdamState*)state,
                omb1, b2, omb2, (float)eps, (float)wd, decay, inv_scale, found_inf);
  DTC_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- global gradient norm + clip coefficient
// torch.nn.utils.clip_grad_norm_(norm_type=2) over the flat gradient buffer, with the GradScaler factor
// folded in: total_norm = inv_scale * sqrt(sum g^2), grad_mult = inv_scale * min(1, max_norm / (total_norm
// + 1e-6)). The optimizer kernels take grad_mult where they would take inv_scale, so the clip costs one
// read pass and no write pass. Squares are accumulated in double (loss-scaled gradients overflow and
// underflow fp32 squares) and in a fixed order -- per thread in index order, the workgroup by
// block_sum_ordered (flat.h), one workspace slot per block, the slots in index order -- with no
// floating-point atomics: the result is bit-identical from run to run.
constexpr int GN_THREADS = 1024;  // one workgroup per CU fills it (16 waves), and keeps the slot count small
constexpr int GN_MAX_BLOCKS = 256;
static int grad_norm_blocks(int64_t n) { return flat_blocks(n / 4, GN_THREADS, GN_MAX_BLOCKS); }
size_t grad_norm_workspace_bytes(int64_t n) { return n > 0 ? (size_t)grad_norm_blocks(n) * sizeof(double) : 0; }

__global__ void __launch_bounds__(GN_THREADS) grad_sumsq_kernel(const float* __restrict__ g, int64_t n4,
                                                                double* __restrict__ slots) {
  const int64_t stride = (int64_t)gridDim.x * GN_THREADS;
  const f32x4* __restrict__ g4 = (const f32x4*)g;
  double acc[1] = {0.0};
  int64_t i = blockIdx.x * (int64_t)GN_THREADS + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {  // four loads in flight per thread per trip
    const f32x4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
    acc[0] = sumsq4(sumsq4(sumsq4(sumsq4(acc[0], a), b), c), d);
  }
  for (; i < n4; i += stride) acc[0] = sumsq4(acc[0], g4[i]);
  block_sum_ordered<GN_THREADS>(acc);
  if (threadIdx.x == 0) slots[blockIdx.x] = acc[0];
}

__global__ void __launch_bounds__(64) grad_norm_finalize_kernel(const double* __restrict__ slots, int nslots,
                                                                const float* __restrict__ inv_scale,
                                                                double max_norm, float* __restrict__ total_norm,
                                                                float* __restrict__ grad_mult) {
  __shared__ double sh[GN_MAX_BLOCKS];
#pragma unroll
  for (int k = threadIdx.x; k < GN_MAX_BLOCKS; k += 64) sh[k] = k < nslots ? slots[k] : 0.0;  // one memory latency
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;  // index order; the unused slots add + 0.0, which changes no bit of a sum of squares
#pragma unroll 16
  for (int k = 0; k < GN_MAX_BLOCKS; ++k) s += sh[k];
  const double is = inv_scale ? (double)*inv_scale : 1.0;
  const double tn = is * sqrt(s);
  const double c = max_norm / (tn + 1e-6);
  const double coef = c > 1.0 ? 1.0 : c;  // clamp(max=1) that keeps a NaN a NaN, as torch's does
  *total_norm = (float)tn;
  *grad_mult = (float)(is * coef);
}

int grad_norm_clip(const float* g, int64_t n, const float* inv_scale, double max_norm, void* workspace,
                   float* total_norm, float* grad_mult, hipStream_t st) {
  DTC_CHECK_ARG(g && workspace && total_norm && grad_mult, "grad_norm_clip: null pointer");
  DTC_CHECK_ARG(mult4(n), "grad_norm_clip: n = %lld must be a positive multiple of 4", (long long)n);
  DTC_CHECK_ARG(aligned(g, 16) && aligned(workspace, 8),
                "grad_norm_clip: g must be 16-byte aligned, the workspace 8-byte aligned");
  DTC_CHECK_ARG(max_norm > 0.0, "grad_norm_clip: max_norm = %g must be positive", max_norm);
  const int blocks = grad_norm_blocks(n);
  DTC_KLAUNCH(grad_sumsq_kernel, dim3(blocks), dim3(GN_THREADS), 0, st, g, n / 4, (double*)workspace);
  DTC_KLAUNCH(grad_norm_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, blocks, inv_scale,
              max_norm, total_norm, grad_mult);
  DTC_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- element-wise operations (flat_map_kernel, flat.h)
struct CastBf16 {
  const float* s;
  u16* d;
  __device__ void operator()(int64_t i) const { d[i] = f2bf(s[i]); }
};
int cast_f32_bf16(const float* src, u16* dst, int64_t n, hipStream_t st) {
  DTC_CHECK_ARG(src && dst && n > 0, "cast_f32_bf16: bad args");
  return launch_map(n, 2048, st, CastBf16{src, dst});
}

struct Zero8 {
  uint2* p;
  __device__ void operator()(int64_t i) const { p[i] = uint2{0u, 0u}; }
};
// A kernel, not hipMemsetAsync: inside a captured graph a memset node is a separate (fill) dispatch
int zero_bytes(void* p, size_t bytes, hipStream_t st) {
  DTC_CHECK_ARG(p && bytes % 8 == 0 && aligned(p, 8), "zero_bytes: 8-byte aligned ranges only");
  if (bytes == 0) return 0;
  return launch_map((int64_t)(bytes / 8), 1024, st, Zero8{(uint2*)p});
}

// The executor's forward prologue: the caller's input copied into the executor's own buffer (the
// captured forward graph reads a fixed address) and the BN slots zeroed, in one launch.
__global__ void copy_zero_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n16,
                                 uint2* __restrict__ z, int64_t n8) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n8; i += stride) z[i] = uint2{0u, 0u};
}

int copy_and_zero(const void* src, void* dst, size_t bytes, void* zp, size_t zbytes, hipStream_t st) {
  DTC_CHECK_ARG(src && dst && zp && bytes % 16 == 0 && zbytes % 8 == 0 && aligned(src, 16) && aligned(dst, 16) &&
                    aligned(zp, 8),
                "copy_and_zero: 16-byte aligned copy, 8-byte aligned zero range");
  const int64_t n16 = (int64_t)(bytes / 16), n8 = (int64_t)(zbytes / 8);
  DTC_KLAUNCH(copy_zero_kernel, dim3(flat_blocks(std::max(n16, n8), 256, 1024)), dim3(256), 0, st, (const uint4*)src,
              (uint4*)dst, n16, (uint2*)zp, n8);
  DTC_LAUNCH_CHECK();
  return 0;
}

template <typename T>
struct Scale {
  T* x;
  T f;
  __device__ void operator()(int64_t i) const { x[i] *= f; }
};
// bf16 words: x = bf16_rne(widen(x) * f), one fp32 multiply (__fmul_rn) and one rounding per element
struct ScaleBf16 {
  u16* x;
  float f;
  __device__ void operator()(int64_t i) const { x[i] = f2bf(__fmul_rn(bf2f(x[i]), f)); }
};
int scale_f32(float* x, int64_t n, float f, hipStream_t st) {
  DTC_CHECK_ARG(x && n > 0, "scale_f32: bad args");
  return launch_map(n, 2048, st, Scale<float>{x, f});
}
int scale_bf16(u16* x, int64_t n, float f, hipStream_t st) {
  DTC_CHECK_ARG(x && n > 0, "scale_bf16: bad args");
  return launch_map(n, 2048, st, ScaleBf16{x, f});
}
int scale_f64(double* x, int64_t n, double f, hipStream_t st) {
  DTC_CHECK_ARG(x && n > 0, "scale_f64: bad args");
  return launch_map(n, 2048, st, Scale<double>{x, f});
}
int scale_i64(int64_t* x, int64_t n, int64_t f, hipStream_t st) {
  DTC_CHECK_ARG(x && n > 0, "scale_i64: bad args");
  return launch_map(n, 2048, st, Scale<int64_t>{x, f});
}

struct AmpScale {
  const float *x, *scale;
  float* out;
  __device__ void operator()(int64_t i) const { out[i] = x[i] * *scale; }
};
int amp_scale(const float* x, const float* scale, float* out, int64_t n, hipStream_t st) {
  DTC_CHECK_ARG(x && scale && out && n > 0, "amp_scale: bad args");
  return launch_map(n, 1024, st, AmpScale{x, scale, out});
}

struct AddF32 {
  f32x4* d;
  const f32x4* s;
  __device__ void operator()(int64_t i) const {
    f32x4 a = d[i];
    a += s[i];
    d[i] = a;
  }
};
int add_f32(float* dst, const float* src, int64_t n, hipStream_t st) {
  DTC_CHECK_ARG(dst && src && mult4(n) && aligned(dst, 16) && aligned(src, 16),
                "add_f32: bad args (n %% 4 and 16-byte alignment required)");
  return launch_map(n / 4, 2048, st, AddF32{(f32x4*)dst, (const f32x4*)src});
}

// In-process thread-group communicator (comm.cpp): out_r[i] = sum_q in_q[i] for every rank r, the
// ranks' buffers summed in rank order (fixed; for two ranks the fp32 sum itself), read before written
// per element so the all-reduce is in place in every rank's buffer.
template <typename T>
struct GroupSum {
  GroupPtrs g;
  int w;
  __device__ void operator()(int64_t i) const {
    T s = ((const T*)g.p[0])[i];
    for (int r = 1; r < w; ++r) s += ((const T*)g.p[r])[i];
    for (int r = 0; r < w; ++r) ((T*)g.p[r])[i] = s;
  }
};
// bf16 buffers: every rank's word <- bf16_rne(((widen(c_0) + widen(c_1)) + ...) + widen(c_{w-1})), fp32 adds in
// rank order (__fadd_rn), rounded once; read before written per element, as above
struct GroupSumBf16 {
  GroupPtrs g;
  int w;
  __device__ void operator()(int64_t i) const {
    float s = bf2f(((const u16*)g.p[0])[i]);
    for (int r = 1; r < w; ++r) s = __fadd_rn(s, bf2f(((const u16*)g.p[r])[i]));
    const u16 o = f2bf(s);
    for (int r = 0; r < w; ++r) ((u16*)g.p[r])[i] = o;
  }
};
int group_sum(const GroupPtrs& g, int w, int64_t n, int dtype, hipStream_t st) {
  DTC_CHECK_ARG(w >= 1 && w <= DTC_GROUP_MAX && n > 0 && dtype >= 0 && dtype <= 3, "group_sum: bad args");
  if (dtype == 0) return launch_map(n, 2048, st, GroupSum<float>{g, w});
  if (dtype == 1) return launch_map(n, 2048, st, GroupSumBf16{g, w});
  if (dtype == 2) return launch_map(n, 2048, st, GroupSum<int64_t>{g, w});
  return launch_map(n, 2048, st, GroupSum<double>{g, w});
}

__global__ void amp_check_finite_kernel(const float* __restrict__ g, int64_t n, int* __restrict__ found) {
  bool bad = false;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    bad |= !isfinite(g[i]);
  if (__any(bad) && (threadIdx.x & 63) == 0) *found = 1;
}

// 16-B aligned gradients (the flat buffer): float4 loads, four in flight per thread per trip
__global__ void amp_check_finite4_kernel(const float* __restrict__ g, int64_t n, int* __restrict__ found) {
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
  const f32x4* __restrict__ g4 = (const f32x4*)g;
  bool bad = false;
  int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const f32x4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
#pragma unroll
    for (int k = 0; k < 4; ++k)  // branch-free: the four tests OR-ed as integers
      bad |= (int)!isfinite(a[k]) | (int)!isfinite(b[k]) | (int)!isfinite(c[k]) | (int)!isfinite(d[k]);
  }
  for (; i < n4; i += stride) {
    const f32x4 a = g4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) bad |= !isfinite(a[k]);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) bad |= !isfinite(g[(n4 << 2) + threadIdx.x]);
  if (__any(bad) && (threadIdx.x & 63) == 0) *found = 1;
}

int amp_check_finite(const float* g, int64_t n, int* found_inf, hipStream_t st) {
  DTC_CHECK_ARG(g && found_inf && n > 0, "amp_check_finite: bad args");
  if (aligned(g, 16))
    DTC_KLAUNCH(amp_check_finite4_kernel, dim3(flat_blocks(n / 4, 256, 1024)), dim3(256), 0, st, g, n, found_inf);
  else
    DTC_KLAUNCH(amp_check_finite_kernel, dim3(flat_blocks(n, 256, 2048)), dim3(256), 0, st, g, n, found_inf);
  DTC_LAUNCH_CHECK();
  return 0;
}

__global__ void amp_update_scale_kernel(float* scale, float* inv_scale, int* tracker, int* found, float growth,
                                        float backoff, int interval) {
  float s = *scale;  // the three state words loaded together (one memory latency), then the update
  const int f = *found, tr = *tracker;
  if (f) {
    s *= backoff;
    *tracker = 0;
  } else {
    const int k = tr + 1;
    if (k >= interval) {
      const float ns = s * growth;
      if (isfinite(ns)) s = ns;
      *tracker = 0;
    } else {
      *tracker = k;
    }
  }
  *scale = s;
  if (inv_scale) *inv_scale = 1.f / s;
  *found = 0;
}

int amp_update_scale(float* scale, float* inv_scale, int* growth_tracker, int* found_inf, float growth, float backoff,
                     int interval, hipStream_t st) {
  DTC_CHECK_ARG(scale && growth_tracker && found_inf && interval > 0, "amp_update_scale: bad args");
  DTC_KLAUNCH(amp_update_scale_kernel, dim3(1), dim3(1), 0, st, scale, inv_scale, growth_tracker, found_inf,
                     growth, backoff, interval);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
