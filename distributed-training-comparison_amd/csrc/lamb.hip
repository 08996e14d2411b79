// Fused LAMB on the flat parameter buffer: layer-wise trust ratios on the Adam moments.
//
// LAMB (You et al. 2020, "Large Batch Optimization for Deep Learning") is to Adam what LARS (lars.hip) is to SGD:
// the step of every parameter tensor is scaled by ||p|| / ||u||, u being the Adam direction formed from the moments
// as this step updates them. Per step, with mult = *inv_scale (GradScaler's 1/scale or a pending clip_grad_norm_
// multiplier; NULL: 1) and t the count of non-skipped steps including this one, for every element of segment s:
//     g' = g * mult
//     m  = m + (g' - m) * (1 - b1)                                  (one fused multiply-add, as adam_kernel's)
//     v  = b2 * v + (1 - b2) * g' * g'
//     r  = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps)                  bc1 = 1 - b1^t, bc2 = 1 - b2^t; without
//                                                                   bias_correction bc1 = bc2 = 1
//     u  = r + wd_s * p                                             wd_s = wd on ADAPT segments, 0 elsewhere
// and per segment, sums and sqrt in double:
//     wn = sqrt(sum p^2), un = sqrt(sum u^2)
//     ADAPT:     ratio = (wn > 0 && un > 0) ? wn / un : 1, with max_trust > 0 min(ratio, max_trust), rounded once to
//                fp32
//     otherwise: ratio = 1        (BatchNorm weight / bias, linear.bias: a bias-corrected Adam step without decay)
//     p -= lr * ratio * u ;  p_bf16 = bf16(p)
// The norm of u needs the updated moments, so the norm pass is the moment update. Four launches, no host
// synchronisation, no floating-point atomics:
//   1. lamb_tick_kernel: one thread advances t in the device record (unless *found_inf) and writes 1 / bc1 and
//      sqrt(bc2), formed in double;
//   2. lamb_moments_kernel: one workgroup per SEG_CHUNK-element chunk of one segment (the plan's work map) loads p, g,
//      m, v -- every load of the chunk issued before the first arithmetic -- writes m and v back, forms u in registers
//      and sums p^2 and u^2 in double in seg_sumsq_kernel's fixed order into the chunk's own slot
//      (16 bytes read + 8 written per element);
//   3. lamb_ratio_kernel: one wave per segment folds its slots in index order and writes (wn, un, ratio);
//   4. lamb_apply_kernel: over the same map reads p, m, v, forms u again through the same lamb_direction() and applies
//      the step and the bf16 shadow (12 bytes read + 6 written per element).
// u is not stored: the gradient buffer keeps showing the gradients, and a scratch buffer would cost 8 more bytes per
// element than forming u twice. lamb_direction() is written with explicit fmaf and without contraction, so the u
// whose norm is taken is bit for bit the u that is applied. Every result is bit-identical from run to run; elements
// between the segments are neither read nor written; a step with *found_inf != 0 changes nothing, t included.
#include "kernels.h"
#include "seg.h"

namespace dtc {

// Pass 2 holds four streams in registers. At seg_sumsq_kernel's depth (256 threads x 8 f32x4 per stream) that is
// 128 data VGPRs per thread, 145 in all: 3 waves per SIMD. 512 threads x 4 f32x4 keep the chunk and the sixteen
// 16-byte loads in flight per thread at 73 VGPRs, 6 waves per SIMD: the same three chunks resident per CU with
// twice the waves to cover the divisions and the double sums (measured 1.7 % faster per step: DESIGN.md 7s).
constexpr int LAMB_THREADS = 512;
constexpr int LAMB_VEC = 4;
static_assert((int64_t)LAMB_THREADS * LAMB_VEC * 4 == SEG_CHUNK, "one workgroup loads one whole chunk");

struct LambState {
  int step;        // completed (non-skipped) steps
  float inv_bc1;   // 1 / bc1
  float bc2_sqrt;  // sqrt(bc2)
  int reserved;
};
static_assert(sizeof(LambState) == 4 * DTC_LAMB_STATE_WORDS, "LambState is DTC_LAMB_STATE_WORDS 32-bit words");

// what both streaming passes need beside the buffers; omb1 = 1 - b1 and omb2 = 1 - b2 are formed in double by the
// launcher (adam_kernel's note: 1.f - 0.999f is 4.7e-5 off)
struct LambCoef {
  float omb1, b2, omb2, eps, wd;
};

__global__ void lamb_tick_kernel(LambState* __restrict__ s, double b1, double b2, int bias_correction,
                                 const int* __restrict__ found_inf) {
  if (found_inf && *found_inf) return;
  const int t = s->step + 1;
  s->step = t;
  s->inv_bc1 = bias_correction ? (float)(1.0 / (1.0 - pow_int(b1, t))) : 1.f;
  s->bc2_sqrt = bias_correction ? (float)sqrt(1.0 - pow_int(b2, t)) : 1.f;
}

// The element formulas. Contraction is off inside them and every fused operation is an explicit fmaf: the compiler
// has no freedom to round u differently in the two kernels that form it.
__device__ __forceinline__ void lamb_moments(float g, float mult, float& m, float& v, const LambCoef& c) {
#pragma clang fp contract(off)
  const float gs = g * mult;
  m = fmaf(gs - m, c.omb1, m);
  v = fmaf(c.omb2 * gs, gs, v * c.b2);
}
__device__ __forceinline__ float lamb_direction(float p, float m, float v, float wds, float inv_bc1, float bc2_sqrt,
                                                float eps) {
#pragma clang fp contract(off)
  const float den = sqrtf(v) / bc2_sqrt + eps;
  const float r = (m * inv_bc1) / den;
  return fmaf(wds, p, r);
}

__global__ void __launch_bounds__(LAMB_THREADS) lamb_moments_kernel(
    const SegDev* __restrict__ segs, const SegChunk* __restrict__ map, const float* __restrict__ p,
    const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, const LambState* __restrict__ state,
    LambCoef co, const float* __restrict__ inv_scale, const int* __restrict__ found_inf, SegSums* __restrict__ slots) {
  if (found_inf && *found_inf) return;  // GradScaler: skip the whole step (the tick skipped it too)
  const ChunkSpan c = chunk_span(segs, map);
  const float is = inv_scale ? *inv_scale : 1.f;
  const float inv_bc1 = state->inv_bc1, bc2_sqrt = state->bc2_sqrt;
  const float wds = (c.flags & 1) ? co.wd : 0.f;
  const int n4 = c.len >> 2, t = threadIdx.x;
  const f32x4* __restrict__ p4 = (const f32x4*)(p + c.base);
  const f32x4* __restrict__ g4 = (const f32x4*)(g + c.base);
  f32x4* __restrict__ m4 = (f32x4*)(m + c.base);
  f32x4* __restrict__ v4 = (f32x4*)(v + c.base);
  // a row past the chunk's end computes on zeros: m = v = u = 0, + 0.0 to both sums, and nothing is stored
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 pv[LAMB_VEC], gv[LAMB_VEC], mv[LAMB_VEC], vv[LAMB_VEC];
#pragma unroll
  for (int k = 0; k < LAMB_VEC; ++k) {
    const int i = t + k * LAMB_THREADS;
    pv[k] = i < n4 ? p4[i] : zero;
    gv[k] = i < n4 ? g4[i] : zero;
    mv[k] = i < n4 ? m4[i] : zero;
    vv[k] = i < n4 ? v4[i] : zero;
  }
  __builtin_amdgcn_sched_barrier(0);  // sixteen loads in flight before the first of them is waited for
  double s[2] = {0.0, 0.0};           // sum p^2, sum u^2
#pragma unroll
  for (int k = 0; k < LAMB_VEC; ++k) {
    const int i = t + k * LAMB_THREADS;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float me = mv[k][j], ve = vv[k][j];
      lamb_moments(gv[k][j], is, me, ve, co);
      const double a = (double)pv[k][j];
      const double u = (double)lamb_direction(pv[k][j], me, ve, wds, inv_bc1, bc2_sqrt, co.eps);
      s[0] += a * a;
      s[1] += u * u;
      mv[k][j] = me;
      vv[k][j] = ve;
    }
    if (i < n4) {
      m4[i] = mv[k];
      v4[i] = vv[k];
    }
  }
  if (t < (c.len & 3)) {  // numel % 4 elements at the end of a segment
    const int64_t i = c.base + 4 * n4 + t;
    const float pe = p[i];
    float me = m[i], ve = v[i];
    lamb_moments(g[i], is, me, ve, co);
    const double a = (double)pe, u = (double)lamb_direction(pe, me, ve, wds, inv_bc1, bc2_sqrt, co.eps);
    s[0] += a * a;
    s[1] += u * u;
    m[i] = me;
    v[i] = ve;
  }
  block_sum_ordered<LAMB_THREADS>(s);
  if (t == 0) slots[blockIdx.x] = SegSums{s[0], s[1]};
}

__global__ void __launch_bounds__(64) lamb_ratio_kernel(const SegDev* __restrict__ segs,
                                                        const SegSums* __restrict__ slots, double max_trust,
                                                        const int* __restrict__ found_inf,
                                                        SegResult* __restrict__ res, float* __restrict__ seg_out) {
  if (found_inf && *found_inf) return;  // pass 2 wrote no slots: the last step's results stay
  const SegDev s = segs[blockIdx.x];
  DTC_SEG_FOLD_SLOTS(s, slots, sp, su)
  if (threadIdx.x != 0) return;
  const double wn = sqrt(sp), un = sqrt(su);
  double ratio = 1.0;
  if ((s.flags & 1) && wn > 0.0 && un > 0.0) {
    ratio = wn / un;
    if (max_trust > 0.0 && ratio > max_trust) ratio = max_trust;
  }
  const SegResult r = {(float)wn, (float)un, (float)ratio, 0.f};
  res[blockIdx.x] = r;
  if (seg_out) {
    seg_out[3 * blockIdx.x + 0] = r.wn;
    seg_out[3 * blockIdx.x + 1] = r.gn;
    seg_out[3 * blockIdx.x + 2] = r.ratio;
  }
}

__global__ void __launch_bounds__(SEG_THREADS) lamb_apply_kernel(
    const SegDev* __restrict__ segs, const SegChunk* __restrict__ map, const SegResult* __restrict__ res,
    float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v, u16* __restrict__ pb,
    const LambState* __restrict__ state, LambCoef co, float lr, const int* __restrict__ found_inf) {
  if (found_inf && *found_inf) return;  // GradScaler: skip the whole step
  const ChunkSpan c = chunk_span(segs, map);
  const float inv_bc1 = state->inv_bc1, bc2_sqrt = state->bc2_sqrt;
  const bool adapt = (c.flags & 1) != 0;
  const float wds = adapt ? co.wd : 0.f;
  const float nstep = -(lr * (adapt ? res[c.seg].ratio : 1.f));  // p = fma(-lr * ratio, u, p)
  const int n4 = c.len >> 2, t = threadIdx.x;
  float* __restrict__ pc = p + c.base;
  const float* __restrict__ mc = m + c.base;
  const float* __restrict__ vc = v + c.base;
  u16* __restrict__ pbc = pb + c.base;
#pragma unroll 4
  for (int i = t; i < n4; i += SEG_THREADS) {
    f32x4 pv = *(const f32x4*)(pc + i * 4);
    const f32x4 mv = *(const f32x4*)(mc + i * 4);
    const f32x4 vv = *(const f32x4*)(vc + i * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      pv[j] = fmaf(nstep, lamb_direction(pv[j], mv[j], vv[j], wds, inv_bc1, bc2_sqrt, co.eps), pv[j]);
    *(f32x4*)(pc + i * 4) = pv;
    store_bf16x4(pbc + i * 4, pv);
  }
  if (t < (c.len & 3)) {  // numel % 4 elements at the end of a segment
    const int i = 4 * n4 + t;
    const float pv = fmaf(nstep, lamb_direction(pc[i], mc[i], vc[i], wds, inv_bc1, bc2_sqrt, co.eps), pc[i]);
    pc[i] = pv;
    pbc[i] = f2bf(pv);
  }
}

int lamb_flat(SegPlan* plan, float* p, const float* g, float* m, float* v, u16* p_bf16, void* state, double lr,
              double beta1, double beta2, double eps, double wd, int bias_correction, double max_trust,
              const float* inv_scale, const int* found_inf, float* seg_out, hipStream_t st) {
  DTC_CHECK_ARG(plan && p && g && m && v && p_bf16 && state, "lamb_flat: null pointer");
  DTC_CHECK_ARG(aligned(p, 16) && aligned(g, 16) && aligned(m, 16) && aligned(v, 16) && aligned(p_bf16, 8) &&
                    aligned(state, 16),
                "lamb_flat: p, g, exp_avg, exp_avg_sq and state must be 16-byte aligned, p_bf16 8-byte aligned");
  DTC_CHECK_ARG(eps > 0.0, "lamb_flat: eps = %g must be positive", eps);
  DTC_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
                "lamb_flat: betas (%g, %g) must lie in [0, 1)", beta1, beta2);
  DTC_CHECK_ARG(lr >= 0.0 && wd >= 0.0, "lamb_flat: lr = %g and weight_decay = %g must not be negative", lr, wd);
  DTC_CHECK_ARG(max_trust >= 0.0, "lamb_flat: max_trust = %g must not be negative (0: no clamp)", max_trust);
  DTC_CHECK_ARG(plan->dev, "lamb_flat: the plan is not bound to device memory (dtc_segplan_bind)");
  const LambCoef co = {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)wd};
  const dim3 grid((unsigned)plan->map.size());
  DTC_KLAUNCH(lamb_tick_kernel, dim3(1), dim3(1), 0, st, (LambState*)state, beta1, beta2, bias_correction, found_inf);
  DTC_KLAUNCH(lamb_moments_kernel, grid, dim3(LAMB_THREADS), 0, st, plan->d_segs(), plan->d_map(), (const float*)p, g,
              m, v, (const LambState*)state, co, inv_scale, found_inf, plan->d_slots());
  DTC_KLAUNCH(lamb_ratio_kernel, dim3((unsigned)plan->segs.size()), dim3(64), 0, st, plan->d_segs(),
              (const SegSums*)plan->d_slots(), max_trust, found_inf, plan->d_res(), seg_out);
  DTC_KLAUNCH(lamb_apply_kernel, grid, dim3(SEG_THREADS), 0, st, plan->d_segs(), plan->d_map(),
              (const SegResult*)plan->d_res(), p, (const float*)m, (const float*)v, p_bf16, (const LambState*)state,
              co, (float)lr, found_inf);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
