// Exponential moving average of the weights over flat buffers (timm ModelEma / torchvision's --model-ema /
// tf.train.ExponentialMovingAverage): per element of every range
//     ema += (src - ema) * w          (one fused multiply-add, torch's lerp_)
//     ema_bf16 = bf16(ema)            (where the range has a bf16 copy: the GEMM operand layout of the EMA)
// with w = 1 - decay, or under warm-up w = 1 - min(decay, (1 + t) / (10 + t)) for the t-th update.
// The update count t lives in a small device record (EmaState), as Adam's step count does (optim.hip): a
// GradScaler-skipped step is not an update, and the host cannot know about a skip without a synchronisation.
// A one-thread "tick" launch ahead of the update advances t (unless *found_inf) and writes w, formed in double
// and rounded once; the update launch only reads the record (stream order separates the two launches). Up to
// DTC_EMA_MAX_RANGES ranges (the parameters and the BatchNorm running statistics of a model) share ONE update
// launch: the range table travels by value and the blocks are dealt out in proportion to the lengths. HBM-bound:
// 4 (ema read) + 4 (src) + 4 (ema write) + 2 (bf16) = 14 B per element. No atomics, no host synchronisation;
// every element is written by exactly one thread, so the result is bit-identical from run to run.
#include "flat.h"
#include "kernels.h"

namespace dtc {

struct EmaState {
  int t;    // updates applied (skipped steps do not count)
  float w;  // the weight of the last update: 1 - decay_t
  int reserved[2];
};
static_assert(sizeof(EmaState) == 4 * DTC_EMA_STATE_WORDS, "EmaState is DTC_EMA_STATE_WORDS 32-bit words");

__global__ void ema_tick_kernel(EmaState* __restrict__ s, double decay, int warmup,
                                const int* __restrict__ found_inf) {
  if (found_inf && *found_inf) return;
  const int t = s->t + 1;
  s->t = t;
  double d = decay;
  if (warmup) {
    const double ramp = (1.0 + (double)t) / (10.0 + (double)t);
    d = ramp < d ? ramp : d;
  }
  s->w = (float)(1.0 - d);
}

// the range table of one launch, passed by value: range r owns blocks [first[r], first[r + 1])
struct EmaTable {
  float* ema[DTC_EMA_MAX_RANGES];
  const float* src[DTC_EMA_MAX_RANGES];
  u16* bf[DTC_EMA_MAX_RANGES];
  int64_t n4[DTC_EMA_MAX_RANGES];
  int first[DTC_EMA_MAX_RANGES + 1];
  int nranges;
};

__global__ void __launch_bounds__(256) ema_update_kernel(const EmaTable tab, const EmaState* __restrict__ state,
                                                         const int* __restrict__ found_inf) {
  if (found_inf && *found_inf) return;  // a skipped optimizer step is not an update (the tick skipped it too)
  const float w = state->w;
  int r = 0;
#pragma unroll
  for (int k = 1; k < DTC_EMA_MAX_RANGES; ++k)
    if (k < tab.nranges && (int)blockIdx.x >= tab.first[k]) r = k;
  float* __restrict__ e = tab.ema[r];
  const float* __restrict__ s = tab.src[r];
  u16* __restrict__ eb = tab.bf[r];
  const int64_t n4 = tab.n4[r];
  const int64_t stride = (int64_t)(tab.first[r + 1] - tab.first[r]) * 256;
  for (int64_t i = ((int)blockIdx.x - tab.first[r]) * (int64_t)256 + threadIdx.x; i < n4; i += stride) {
    f32x4 ev = *(const f32x4*)(e + i * 4);
    const f32x4 sv = *(const f32x4*)(s + i * 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) ev[k] = fmaf(sv[k] - ev[k], w, ev[k]);
    *(f32x4*)(e + i * 4) = ev;
    if (eb) store_bf16x4(eb + i * 4, ev);  // uniform over the block
  }
}

int ema_update(const EmaRange* ranges, int nranges, void* state, double decay, int warmup, const int* found_inf,
               hipStream_t st) {
  DTC_CHECK_ARG(ranges && state, "ema_update: null pointer (ranges or state)");
  DTC_CHECK_ARG(nranges >= 1 && nranges <= DTC_EMA_MAX_RANGES, "ema_update: nranges = %d outside [1, %d]", nranges,
                DTC_EMA_MAX_RANGES);
  DTC_CHECK_ARG(aligned(state, 16), "ema_update: state must be 16-byte aligned");
  DTC_CHECK_ARG(decay >= 0.0 && decay < 1.0, "ema_update: decay = %g must lie in [0, 1)", decay);
  EmaTable tab = {};
  tab.nranges = nranges;
  int64_t total4 = 0, want = 0;  // float4 elements; blocks of one float4 per thread
  for (int r = 0; r < nranges; ++r) {
    const EmaRange& q = ranges[r];
    DTC_CHECK_ARG(q.ema && q.src, "ema_update: range %d: null pointer (ema or src)", r);
    DTC_CHECK_ARG(mult4(q.n), "ema_update: range %d: n = %lld must be a positive multiple of 4", r,
                  (long long)q.n);
    DTC_CHECK_ARG(aligned(q.ema, 16) && aligned(q.src, 16) && aligned(q.ema_bf16, 8),
                  "ema_update: range %d: ema and src must be 16-byte aligned, ema_bf16 8-byte aligned", r);
    DTC_CHECK_ARG(!ranges_overlap(q.ema, q.n * 4, q.src, q.n * 4), "ema_update: range %d: ema and src overlap", r);
    for (int o = 0; o < r; ++o)
      DTC_CHECK_ARG(!ranges_overlap(q.ema, q.n * 4, ranges[o].ema, ranges[o].n * 4),
                    "ema_update: the ema of ranges %d and %d overlap", o, r);
    tab.ema[r] = q.ema;
    tab.src[r] = q.src;
    tab.bf[r] = q.ema_bf16;
    tab.n4[r] = q.n / 4;
    total4 += tab.n4[r];
    want += flat_blocks(tab.n4[r], 256, INT32_MAX);
  }
  // blocks in proportion to the lengths, at least one per range and never more than a range has float4 rows of 256
  const int64_t budget = std::min<int64_t>(2048, want);
  tab.first[0] = 0;
  for (int r = 0; r < nranges; ++r) {
    const int64_t full = flat_blocks(tab.n4[r], 256, INT32_MAX);
    const int64_t share = (int64_t)((double)budget * (double)tab.n4[r] / (double)total4);
    tab.first[r + 1] = tab.first[r] + (int)std::max<int64_t>(1, std::min<int64_t>(full, share));
  }
  DTC_KLAUNCH(ema_tick_kernel, dim3(1), dim3(1), 0, st, (EmaState*)state, decay, warmup != 0 ? 1 : 0, found_inf);
  DTC_KLAUNCH(ema_update_kernel, dim3(tab.first[nranges]), dim3(256), 0, st, tab, (const EmaState*)state, found_inf);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
