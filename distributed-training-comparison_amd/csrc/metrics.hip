// Evaluation metrics of one batch in one launch: the mean cross-entropy and the top-1 / top-k hit counts
// that `validate` / `test` (reference src/ddp/trainer.py:170-215: `criterion(pred, label).item()` and
// `accuracy(pred, label, topk=(1, 5))`, utils.py:18-31) compute per batch, written as one 16-byte record
// into device memory. No host synchronisation, no atomics: every reduction has a fixed order.
//
//   loss : exactly xent_fwd's value (head.hip): row_lse16 per row, xent_mean_kernel's summation order
//          (256 strided accumulators, wave_sum, four partials, / n) -- bit-identical.
//   rank : of the label's logit within its row,
//            rank = #{ j != y : !(z[j] <= z[y]) } + #{ j < y : z[j] == z[y] }
//          i.e. strictly greater logits first, ties to the lower index, a NaN logit above everything (a NaN
//          label logit ranks last but for itself: ncls - 1). top1 / topk count the rows with rank < 1 /
//          rank < k; a row whose label is out of range counts for neither (and makes the loss NaN, as in
//          xent_fwd). torch.topk leaves the order of ties unspecified; on tie-free rows the two agree.
#include "common.h"
#include "kernels.h"
#include "../../include/dtc.h"

namespace dtc {

constexpr int EM_MAX_ROWS = 4096;

// lane li's share of the rank of row z (the values j = li, li + 16, ...); y in range
__device__ __forceinline__ int rank_part(float v, float zy, int j, int y) {
  return j == y ? 0 : ((!(v <= zy) ? 1 : 0) + ((j < y && v == zy) ? 1 : 0));
}

__global__ void __launch_bounds__(1024) eval_metrics_kernel(const float* __restrict__ logits,
                                                           const int64_t* __restrict__ labels, int N, int ncls,
                                                           int topk, dtc_eval_record* __restrict__ rec) {
  __shared__ float sterm[EM_MAX_ROWS];    // lse - logit[label] per row (xent_mean_kernel's term)
  __shared__ uint8_t hits[EM_MAX_ROWS];   // bit 0: rank < 1, bit 1: rank < topk
  __shared__ float part[4];
  __shared__ int hpart[2][4];
  const int t = threadIdx.x, li = t & 15, lane = t & 63;
  if (ncls <= 128) {
    // As xent_fwd_fused_kernel: sixteen lanes per row, each thread first issues ALL the loads of four rows
    // (lane li: z[li + 16 k], and the label), then reduces -- one memory latency per four rounds of 64 rows.
    // The folds match row_lse16 (same per-lane order, same DPP tree); the label's logit comes from the lane
    // holding it, and the rank is counted from the same registers.
    constexpr int RR = 4, KV = 8;
    for (int b0 = t >> 4; b0 < N; b0 += 64 * RR) {
      float v[RR][KV];
      int64_t y[RR];
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        const int b = b0 + 64 * r, bb = b < N ? b : 0;
        const float* z = logits + (int64_t)bb * ncls;
#pragma unroll
        for (int k = 0; k < KV; ++k) v[r][k] = li + 16 * k < ncls ? z[li + 16 * k] : 0.f;
        y[r] = labels[bb];
      }
#pragma unroll
      for (int r = 0; r < RR; ++r) {
        const int b = b0 + 64 * r;
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < KV; ++k)
          if (li + 16 * k < ncls) m = fmaxf(m, v[r][k]);
        m = row16_max(m);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < KV; ++k)
          if (li + 16 * k < ncls) sum += expf(v[r][k] - m);
        sum = row16_sum(sum);
        const float l = m + logf(sum);
        const bool ok = y[r] >= 0 && y[r] < ncls;
        const int yl = ok ? (int)y[r] : 0;
        float cand = 0.f;
#pragma unroll
        for (int k = 0; k < KV; ++k) cand = (yl >> 4) == k ? v[r][k] : cand;
        const float zy = __shfl(cand, (lane & ~15) | (yl & 15));
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < KV; ++k)
          if (li + 16 * k < ncls) cnt += rank_part(v[r][k], zy, li + 16 * k, yl);
        cnt = row16_sum_i(cnt);
        if (li == 0 && b < N) {
          sterm[b] = ok ? (l - zy) : NAN;
          hits[b] = ok ? (uint8_t)((cnt < 1 ? 1 : 0) | (cnt < topk ? 2 : 0)) : (uint8_t)0;
        }
      }
    }
  } else {
    for (int b = t >> 4; b < N; b += 64) {  // 64 rows per round, sixteen lanes each (whole rows retire together)
      const float* z = logits + (int64_t)b * ncls;
      const float l = row_lse16(z, ncls, li);
      const int64_t y = labels[b];
      const bool ok = y >= 0 && y < ncls;
      const int yl = ok ? (int)y : 0;
      const float zy = z[yl];
      int cnt = 0;
#pragma unroll 8
      for (int j = li; j < ncls; j += 16) cnt += rank_part(z[j], zy, j, yl);
      cnt = row16_sum_i(cnt);
      if (li == 0) {
        sterm[b] = ok ? (l - zy) : NAN;
        hits[b] = ok ? (uint8_t)((cnt < 1 ? 1 : 0) | (cnt < topk ? 2 : 0)) : (uint8_t)0;
      }
    }
  }
  __syncthreads();
  if (t < 256) {  // the mean exactly as xent_mean_kernel sums it; the hit flags in the same fixed order
    float acc = 0.f;
    int h1 = 0, hk = 0;
    for (int b = t; b < N; b += 256) {
      acc += sterm[b];
      const int f = hits[b];
      h1 += f & 1;
      hk += f >> 1;
    }
    acc = wave_sum(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      h1 += __shfl_xor(h1, o, 64);
      hk += __shfl_xor(hk, o, 64);
    }
    if ((t & 63) == 0) {
      part[t >> 6] = acc;
      hpart[0][t >> 6] = h1;
      hpart[1][t >> 6] = hk;
    }
  }
  __syncthreads();
  if (t == 0) {
    rec->loss = (part[0] + part[1] + part[2] + part[3]) / (float)N;
    rec->n = N;
    rec->top1 = hpart[0][0] + hpart[0][1] + hpart[0][2] + hpart[0][3];
    rec->topk = hpart[1][0] + hpart[1][1] + hpart[1][2] + hpart[1][3];
  }
}

int eval_metrics(const float* logits, const int64_t* labels, int N, int ncls, int topk, dtc_eval_record* rec,
                 hipStream_t st) {
  DTC_CHECK_ARG(logits && labels && rec, "eval_metrics: null pointer");
  DTC_CHECK_ARG(N >= 1 && N <= EM_MAX_ROWS, "eval_metrics: n = %d outside [1, %d]", N, EM_MAX_ROWS);
  DTC_CHECK_ARG(ncls >= 1 && topk >= 1 && topk <= ncls, "eval_metrics: topk = %d outside [1, ncls = %d]", topk, ncls);
  DTC_KLAUNCH(eval_metrics_kernel, dim3(1), dim3(1024), 0, st, logits, labels, N, ncls, topk, rec);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
