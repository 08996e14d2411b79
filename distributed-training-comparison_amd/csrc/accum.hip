// Gradient accumulation over fp32 ranges of the flat gradient buffer (torch's `.grad +=` across the micro-batches
// of one optimizer step; DistributedDataParallel.no_sync()). The backward kernels WRITE their gradients, so the
// sum over a window of micro-batches is kept in a second buffer `acc` of the same layout, one launch per range:
//     DTC_ACCUM_STORE   acc = g          (first micro-batch of a window)        4 + 4     =  8 B per element
//     DTC_ACCUM_ADD     acc = acc + g    (every further one inside the window)  4 + 4 + 4 = 12 B per element
//     DTC_ACCUM_FINISH  g   = g + acc    (the micro-batch that ends the window) 4 + 4 + 4 = 12 B per element
// Each result is exactly one IEEE fp32 add per element (__fadd_rn: no FMA to contract into, nothing reassociated),
// so it is bit-defined, and an inf or NaN of any micro-batch reaches the final g: the finiteness check over g
// after FINISH still decides a skipped step. HBM-bound. A workgroup takes chunks of ACCUM_CHUNK4 float4 rows
// (ACCUM_UNROLL per thread, ACCUM_THREADS apart); in a full chunk every thread issues all its 16-byte loads of
// both operands before the first add, a ragged last chunk guards each row. The grid is sized to the range, capped
// at ACCUM_MAX_BLOCKS (four workgroups per CU), and strides over the chunks. No atomics, vector stores only; every
// element is written by exactly one thread, so the result is bit-identical from run to run. The kernel keeps its own
// loop rather than flat.h's stream_chunks: on that, STORE measured 2% slower (profiles/flat_refactor_ab.json).
#include "../../include/dtc.h"
#include "flat.h"
#include "kernels.h"

namespace dtc {

constexpr int ACCUM_THREADS = DTC_ACCUM_THREADS, ACCUM_UNROLL = DTC_ACCUM_UNROLL;
constexpr int ACCUM_CHUNK4 = ACCUM_THREADS * ACCUM_UNROLL;  // float4 rows per workgroup trip
constexpr int ACCUM_MAX_BLOCKS = DTC_ACCUM_MAX_BLOCKS;

// dst = a + b per element, rows i of float4; MODE picks which operand is the destination
template <int MODE>
__global__ void __launch_bounds__(ACCUM_THREADS) grad_accum_kernel(float* __restrict__ acc, float* __restrict__ g,
                                                                   int64_t n4) {
  f32x4* __restrict__ a4 = (f32x4*)acc;
  f32x4* __restrict__ g4 = (f32x4*)g;
  const int64_t chunks = (n4 + ACCUM_CHUNK4 - 1) / ACCUM_CHUNK4;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t i0 = c * ACCUM_CHUNK4 + threadIdx.x;
    f32x4 gv[ACCUM_UNROLL], av[ACCUM_UNROLL];
    if ((c + 1) * ACCUM_CHUNK4 <= n4) {  // uniform over the workgroup: a full chunk, no per-row guard
#pragma unroll
      for (int k = 0; k < ACCUM_UNROLL; ++k) gv[k] = g4[i0 + k * ACCUM_THREADS];
      if (MODE != DTC_ACCUM_STORE) {
#pragma unroll
        for (int k = 0; k < ACCUM_UNROLL; ++k) av[k] = a4[i0 + k * ACCUM_THREADS];
      }
#pragma unroll
      for (int k = 0; k < ACCUM_UNROLL; ++k) {
        f32x4 r = gv[k];
        if (MODE == DTC_ACCUM_ADD) {
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = __fadd_rn(av[k][e], gv[k][e]);
        } else if (MODE == DTC_ACCUM_FINISH) {
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = __fadd_rn(gv[k][e], av[k][e]);
        }
        (MODE == DTC_ACCUM_FINISH ? g4 : a4)[i0 + k * ACCUM_THREADS] = r;
      }
    } else {  // the ragged last chunk
#pragma unroll
      for (int k = 0; k < ACCUM_UNROLL; ++k) {
        const int64_t i = i0 + k * ACCUM_THREADS;
        if (i < n4) {
          gv[k] = g4[i];
          if (MODE != DTC_ACCUM_STORE) av[k] = a4[i];
        }
      }
#pragma unroll
      for (int k = 0; k < ACCUM_UNROLL; ++k) {
        const int64_t i = i0 + k * ACCUM_THREADS;
        if (i < n4) {
          f32x4 r = gv[k];
          if (MODE == DTC_ACCUM_ADD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = __fadd_rn(av[k][e], gv[k][e]);
          } else if (MODE == DTC_ACCUM_FINISH) {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = __fadd_rn(gv[k][e], av[k][e]);
          }
          (MODE == DTC_ACCUM_FINISH ? g4 : a4)[i] = r;
        }
      }
    }
  }
}

int grad_accum(float* acc, float* g, int64_t n, int mode, hipStream_t st) {
  DTC_CHECK_ARG(acc && g, "grad_accum: null pointer (acc or g)");
  DTC_CHECK_ARG(mult4(n), "grad_accum: n = %lld must be a positive multiple of 4", (long long)n);
  DTC_CHECK_ARG(aligned(acc, 16) && aligned(g, 16), "grad_accum: acc and g must be 16-byte aligned");
  DTC_CHECK_ARG(mode >= DTC_ACCUM_STORE && mode <= DTC_ACCUM_FINISH, "grad_accum: mode = %d outside [1, 3]", mode);
  DTC_CHECK_ARG(!ranges_overlap(acc, n * 4, g, n * 4), "grad_accum: acc and g overlap");
  const int64_t n4 = n / 4;
  const dim3 grid(flat_blocks(n4, ACCUM_CHUNK4, ACCUM_MAX_BLOCKS));
  if (mode == DTC_ACCUM_STORE)
    DTC_KLAUNCH(grad_accum_kernel<DTC_ACCUM_STORE>, grid, dim3(ACCUM_THREADS), 0, st, acc, g, n4);
  else if (mode == DTC_ACCUM_ADD)
    DTC_KLAUNCH(grad_accum_kernel<DTC_ACCUM_ADD>, grid, dim3(ACCUM_THREADS), 0, st, acc, g, n4);
  else
    DTC_KLAUNCH(grad_accum_kernel<DTC_ACCUM_FINISH>, grid, dim3(ACCUM_THREADS), 0, st, acc, g, n4);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
