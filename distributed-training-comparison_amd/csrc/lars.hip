// Per-tensor (segmented) reductions over the flat parameter / gradient buffers, and fused LARS on top of them.
//
// LARS (You, Gitman, Ginsburg 2017, "Large Batch Training of Convolutional Networks") is SGD with momentum whose
// step of every parameter tensor is scaled by a trust ratio formed from the norms of that tensor and of its
// gradient. The other kernels of optim.hip see the flat buffer as one anonymous vector; here a segment plan tells
// the device where each tensor lies. Per step, with mult = *inv_scale (GradScaler's 1/scale or a pending
// clip_grad_norm_ multiplier; NULL: 1), for every segment s:
//     wn = sqrt(sum p^2), gn = |mult| * sqrt(sum g^2)                                   (sums and sqrt in double)
//     ADAPT:     ratio = (wn > 0 && gn > 0) ? trust_coef * wn / (gn + wd * wn + eps) : 1, and with trust_clip
//                (LARC's "clip" mode) ratio = min(ratio / lr, 1) where both norms are positive;
//                ratio rounded once to fp32;  d = (g * mult + wd * p) * ratio
//     otherwise: ratio = 1 and no weight decay;  d = g * mult            (BatchNorm weight / bias, linear.bias)
//     buf = mu * buf + d ;  u = nesterov ? d + mu * buf : buf ;  p -= lr * u ;  p_bf16 = bf16(p)
// Three launches, no host synchronisation, no floating-point atomics:
//   1. seg_sumsq_kernel: one workgroup per SEG_CHUNK-element chunk of one segment (the host-built work map), both
//      sums of squares in double in grad_sumsq_kernel's fixed order -- per thread in index order, the workgroup by
//      the same block_sum_ordered (flat.h) -- into the chunk's own slot;
//   2. seg_ratio_kernel: one wave per segment folds its slots in index order and writes norms and ratio;
//   3. lars_update_kernel: one workgroup per chunk over the same map applies the update and the bf16 shadow.
// Every result is bit-identical from run to run. Elements between the segments (the flat buffer's 64-element
// alignment padding) are neither read nor written.
#include <new>
#include <vector>
#include "flat.h"
#include "kernels.h"

namespace dtc {

constexpr int SEG_THREADS = 256;
constexpr int SEG_VEC = 8;  // f32x4 per thread and buffer: sixteen 16-byte loads in flight in the norm pass
constexpr int64_t SEG_CHUNK = (int64_t)SEG_THREADS * SEG_VEC * 4;  // 8192 elements
constexpr int SEG_MAX = 4096;
constexpr int64_t SEG_MAX_CHUNKS = 1 << 24;
constexpr int SEG_KNOWN_FLAGS = 1;  // bit 0: ADAPT

struct SegDev {  // one segment as the kernels read it (32 bytes)
  int64_t offset, numel;
  int32_t flags, first_chunk, nchunks, reserved;
};
struct SegChunk {  // work map: workgroup -> (segment, chunk of it)
  int32_t seg, chunk;
};
struct SegSums {  // one partial slot
  double p, g;
};
struct SegResult {  // per segment: ||p||, |mult| * ||g||, ratio
  float wn, gn, ratio, reserved;
};

struct SegPlan {
  std::vector<SegDev> segs;
  std::vector<SegChunk> map;
  size_t off_map = 0, off_slots = 0, off_res = 0, bytes = 0;
  void* dev = nullptr;  // caller-owned, set by bind
  const SegDev* d_segs() const { return (const SegDev*)dev; }
  const SegChunk* d_map() const { return (const SegChunk*)((char*)dev + off_map); }
  SegSums* d_slots() const { return (SegSums*)((char*)dev + off_slots); }
  SegResult* d_res() const { return (SegResult*)((char*)dev + off_res); }
};

static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

int64_t segplan_chunk_elems() { return SEG_CHUNK; }

int segplan_create(SegPlan** out, const SegDesc* segs, int nseg) {
  DTC_CHECK_ARG(out, "segplan_create: null output pointer");
  *out = nullptr;
  DTC_CHECK_ARG(segs, "segplan_create: null segment table");
  DTC_CHECK_ARG(nseg >= 1 && nseg <= SEG_MAX, "segplan_create: nseg = %d must lie in [1, %d]", nseg, SEG_MAX);
  int64_t end = 0, chunks = 0;
  for (int i = 0; i < nseg; ++i) {
    const SegDesc& s = segs[i];
    DTC_CHECK_ARG(s.numel >= 1, "segplan_create: segment %d: numel = %lld must be positive", i, (long long)s.numel);
    DTC_CHECK_ARG(s.offset >= 0 && s.offset % 4 == 0,
                  "segplan_create: segment %d: offset = %lld must be a non-negative multiple of 4", i,
                  (long long)s.offset);
    DTC_CHECK_ARG(s.numel <= INT64_MAX - s.offset, "segplan_create: segment %d: offset + numel overflows", i);
    DTC_CHECK_ARG(s.offset >= end,
                  "segplan_create: segment %d (offset %lld) is not sorted after / overlaps its predecessor (end %lld)",
                  i, (long long)s.offset, (long long)end);
    DTC_CHECK_ARG(s.reserved == 0, "segplan_create: segment %d: reserved = %d must be 0", i, (int)s.reserved);
    DTC_CHECK_ARG((s.flags & ~SEG_KNOWN_FLAGS) == 0, "segplan_create: segment %d: unknown flag bits 0x%x", i,
                  (unsigned)(s.flags & ~SEG_KNOWN_FLAGS));
    end = s.offset + s.numel;
    chunks += (s.numel - 1) / SEG_CHUNK + 1;
    DTC_CHECK_ARG(chunks <= SEG_MAX_CHUNKS, "segplan_create: more than %lld chunks of %lld elements",
                  (long long)SEG_MAX_CHUNKS, (long long)SEG_CHUNK);
  }
  SegPlan* pl = new (std::nothrow) SegPlan;
  DTC_CHECK_ARG(pl, "segplan_create: out of host memory");
  pl->segs.reserve(nseg);
  pl->map.reserve((size_t)chunks);
  for (int i = 0; i < nseg; ++i) {
    const int nch = (int)((segs[i].numel - 1) / SEG_CHUNK + 1);
    pl->segs.push_back(SegDev{segs[i].offset, segs[i].numel, segs[i].flags, (int32_t)pl->map.size(), nch, 0});
    for (int c = 0; c < nch; ++c) pl->map.push_back(SegChunk{i, c});
  }
  pl->off_map = up16(pl->segs.size() * sizeof(SegDev));
  pl->off_slots = up16(pl->off_map + pl->map.size() * sizeof(SegChunk));
  pl->off_res = up16(pl->off_slots + pl->map.size() * sizeof(SegSums));
  pl->bytes = up16(pl->off_res + pl->segs.size() * sizeof(SegResult));
  *out = pl;
  return 0;
}

int segplan_destroy(SegPlan* plan) {
  delete plan;
  return 0;
}

int segplan_num_segments(const SegPlan* plan) { return plan ? (int)plan->segs.size() : 0; }
size_t segplan_device_bytes(const SegPlan* plan) { return plan ? plan->bytes : 0; }

int segplan_bind(SegPlan* plan, void* dev, size_t bytes, hipStream_t st) {
  DTC_CHECK_ARG(plan && dev, "segplan_bind: null pointer");
  DTC_CHECK_ARG(aligned(dev, 16), "segplan_bind: the device region must be 16-byte aligned");
  DTC_CHECK_ARG(bytes >= plan->bytes, "segplan_bind: %zu bytes given, the plan needs %zu", bytes, plan->bytes);
  plan->dev = nullptr;
  DTC_HIP(hipMemcpyAsync(dev, plan->segs.data(), plan->segs.size() * sizeof(SegDev), hipMemcpyHostToDevice, st));
  DTC_HIP(hipMemcpyAsync((char*)dev + plan->off_map, plan->map.data(), plan->map.size() * sizeof(SegChunk),
                         hipMemcpyHostToDevice, st));
  plan->dev = dev;
  return 0;
}

// ---------------------------------------------------------------- kernels
// this workgroup's chunk: first element and length (the last chunk of a segment is the short one)
struct ChunkSpan {
  int64_t base;
  int len, flags, seg;
};
__device__ __forceinline__ ChunkSpan chunk_span(const SegDev* __restrict__ segs, const SegChunk* __restrict__ map) {
  const SegChunk m = map[blockIdx.x];
  const SegDev s = segs[m.seg];
  const int64_t start = (int64_t)m.chunk * SEG_CHUNK;
  const int64_t left = s.numel - start;
  return ChunkSpan{s.offset + start, (int)(left < SEG_CHUNK ? left : SEG_CHUNK), s.flags, m.seg};
}

__global__ void __launch_bounds__(SEG_THREADS) seg_sumsq_kernel(const SegDev* __restrict__ segs,
                                                                const SegChunk* __restrict__ map,
                                                                const float* __restrict__ p,
                                                                const float* __restrict__ g,
                                                                SegSums* __restrict__ slots) {
  const ChunkSpan c = chunk_span(segs, map);
  const int n4 = c.len >> 2, t = threadIdx.x;
  const f32x4* __restrict__ p4 = (const f32x4*)(p + c.base);
  const f32x4* __restrict__ g4 = (const f32x4*)(g + c.base);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};  // + 0.0 * 0.0 changes no bit of a sum of squares
  f32x4 pv[SEG_VEC], gv[SEG_VEC];
#pragma unroll
  for (int k = 0; k < SEG_VEC; ++k) {
    const int i = t + k * SEG_THREADS;
    pv[k] = i < n4 ? p4[i] : zero;
    gv[k] = i < n4 ? g4[i] : zero;
  }
  double s[2] = {0.0, 0.0};  // sum p^2, sum g^2
#pragma unroll
  for (int k = 0; k < SEG_VEC; ++k) {
    s[0] = sumsq4(s[0], pv[k]);
    s[1] = sumsq4(s[1], gv[k]);
  }
  if (t < (c.len & 3)) {  // numel % 4 elements at the end of a segment
    const double a = (double)p[c.base + 4 * n4 + t], b = (double)g[c.base + 4 * n4 + t];
    s[0] += a * a;
    s[1] += b * b;
  }
  block_sum_ordered<SEG_THREADS>(s);
  if (t == 0) slots[blockIdx.x] = SegSums{s[0], s[1]};
}

struct RatioArgs {
  double lr, wd, trust_coef, eps;
  int trust_clip;
};

__global__ void __launch_bounds__(64) seg_ratio_kernel(const SegDev* __restrict__ segs,
                                                       const SegSums* __restrict__ slots, RatioArgs a,
                                                       const float* __restrict__ inv_scale,
                                                       SegResult* __restrict__ res, float* __restrict__ seg_out) {
  const SegDev s = segs[blockIdx.x];
  const double mult = inv_scale ? (double)*inv_scale : 1.0;  // loaded beside the record, not behind the fold
  constexpr int TILE = 512;  // slots per memory latency (ResNet-18's largest tensor has 288), summed in index order
  __shared__ SegSums sh[TILE];
  double sp = 0.0, sg = 0.0;
  for (int base = 0; base < s.nchunks; base += TILE) {
#pragma unroll
    for (int j = 0; j < TILE / 64; ++j) {
      const int k = base + j * 64 + threadIdx.x;
      if (k < s.nchunks) sh[j * 64 + threadIdx.x] = slots[s.first_chunk + k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = s.nchunks - base < TILE ? s.nchunks - base : TILE;
#pragma unroll 8
      for (int j = 0; j < m; ++j) {
        sp += sh[j].p;
        sg += sh[j].g;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double wn = sqrt(sp), gn = fabs(mult) * sqrt(sg);
  double ratio = 1.0;
  if ((s.flags & 1) && wn > 0.0 && gn > 0.0) {
    ratio = a.trust_coef * wn / (gn + a.wd * wn + a.eps);
    if (a.trust_clip) {
      const double r = ratio / a.lr;
      ratio = r < 1.0 ? r : 1.0;
    }
  }
  const SegResult r = {(float)wn, (float)gn, (float)ratio, 0.f};
  res[blockIdx.x] = r;
  if (seg_out) {
    seg_out[3 * blockIdx.x + 0] = r.wn;
    seg_out[3 * blockIdx.x + 1] = r.gn;
    seg_out[3 * blockIdx.x + 2] = r.ratio;
  }
}

template <bool NESTEROV>
__global__ void __launch_bounds__(SEG_THREADS) lars_update_kernel(const SegDev* __restrict__ segs,
                                                                  const SegChunk* __restrict__ map,
                                                                  const SegResult* __restrict__ res,
                                                                  float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, u16* __restrict__ pb, float lr,
                                                                  float wd, float mu,
                                                                  const float* __restrict__ inv_scale,
                                                                  const int* __restrict__ found_inf) {
  if (found_inf && *found_inf) return;  // GradScaler: skip the whole step
  const ChunkSpan c = chunk_span(segs, map);
  const float is = inv_scale ? *inv_scale : 1.f;
  const bool adapt = (c.flags & 1) != 0;
  const float ratio = adapt ? res[c.seg].ratio : 1.f;
  const float wds = adapt ? wd : 0.f;
  const int n4 = c.len >> 2, t = threadIdx.x;
  float* __restrict__ pc = p + c.base;
  const float* __restrict__ gc = g + c.base;
  float* __restrict__ mc = m + c.base;
  u16* __restrict__ pbc = pb + c.base;
#pragma unroll 4
  for (int i = t; i < n4; i += SEG_THREADS) {
    f32x4 pv = *(const f32x4*)(pc + i * 4);
    const f32x4 gv = *(const f32x4*)(gc + i * 4);
    f32x4 mv = *(const f32x4*)(mc + i * 4);
    momentum_step<NESTEROV>(pv, mv, (gv * is + pv * wds) * ratio, mu, lr);
    *(f32x4*)(pc + i * 4) = pv;
    *(f32x4*)(mc + i * 4) = mv;
    store_bf16x4(pbc + i * 4, pv);
  }
  if (t < (c.len & 3)) {  // numel % 4 elements at the end of a segment
    const int i = 4 * n4 + t;
    float pv = pc[i], mv = mc[i];
    momentum_step<NESTEROV>(pv, mv, (gc[i] * is + pv * wds) * ratio, mu, lr);
    pc[i] = pv;
    mc[i] = mv;
    pbc[i] = f2bf(pv);
  }
}

// ---------------------------------------------------------------- launchers
static int launch_norms(const SegPlan* pl, const float* p, const float* g, const RatioArgs& ra, const float* gmul,
                        float* seg_out, hipStream_t st) {
  DTC_KLAUNCH(seg_sumsq_kernel, dim3((unsigned)pl->map.size()), dim3(SEG_THREADS), 0, st, pl->d_segs(), pl->d_map(), p,
              g, pl->d_slots());
  DTC_KLAUNCH(seg_ratio_kernel, dim3((unsigned)pl->segs.size()), dim3(64), 0, st, pl->d_segs(),
              (const SegSums*)pl->d_slots(), ra, gmul, pl->d_res(), seg_out);
  return 0;
}

int seg_norms(SegPlan* plan, const float* p, const float* g, const float* gmul, float* seg_out, hipStream_t st) {
  DTC_CHECK_ARG(plan && p && g, "seg_norms: null pointer");
  DTC_CHECK_ARG(aligned(p, 16) && aligned(g, 16), "seg_norms: p and g must be 16-byte aligned");
  DTC_CHECK_ARG(plan->dev, "seg_norms: the plan is not bound to device memory (dtc_segplan_bind)");
  launch_norms(plan, p, g, RatioArgs{1.0, 0.0, 1.0, 0.0, 0}, gmul, seg_out, st);  // ratio = ||p|| / (|mult| ||g||)
  DTC_LAUNCH_CHECK();
  return 0;
}

int lars_flat(SegPlan* plan, float* p, const float* g, float* mom, u16* p_bf16, double lr, double wd, double mu,
              int nesterov, double trust_coef, double eps, int trust_clip, const float* inv_scale,
              const int* found_inf, float* seg_out, hipStream_t st) {
  DTC_CHECK_ARG(lr >= 0.0 && wd >= 0.0, "lars_flat: lr = %g and weight_decay = %g must not be negative", lr, wd);
  DTC_CHECK_ARG(mu >= 0.0 && mu < 1.0, "lars_flat: momentum = %g must lie in [0, 1)", mu);
  DTC_CHECK_ARG(trust_coef > 0.0, "lars_flat: trust_coef = %g must be positive", trust_coef);
  DTC_CHECK_ARG(eps >= 0.0, "lars_flat: eps = %g must not be negative", eps);
  DTC_CHECK_ARG(!trust_clip || lr > 0.0, "lars_flat: trust_clip divides the ratio by lr = %g, which must be positive",
                lr);
  DTC_CHECK_ARG(plan && p && g && mom && p_bf16, "lars_flat: null pointer");
  DTC_CHECK_ARG(aligned(p, 16) && aligned(g, 16) && aligned(mom, 16) && aligned(p_bf16, 8),
                "lars_flat: p, g and momentum_buf must be 16-byte aligned, p_bf16 8-byte aligned");
  DTC_CHECK_ARG(plan->dev, "lars_flat: the plan is not bound to device memory (dtc_segplan_bind)");
  launch_norms(plan, p, g, RatioArgs{lr, wd, trust_coef, eps, trust_clip}, inv_scale, seg_out, st);
  const dim3 grid((unsigned)plan->map.size());
  if (nesterov)
    DTC_KLAUNCH(lars_update_kernel<true>, grid, dim3(SEG_THREADS), 0, st, plan->d_segs(), plan->d_map(),
                (const SegResult*)plan->d_res(), p, g, mom, p_bf16, (float)lr, (float)wd, (float)mu, inv_scale,
                found_inf);
  else
    DTC_KLAUNCH(lars_update_kernel<false>, grid, dim3(SEG_THREADS), 0, st, plan->d_segs(), plan->d_map(),
                (const SegResult*)plan->d_res(), p, g, mom, p_bf16, (float)lr, (float)wd, (float)mu, inv_scale,
                found_inf);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
