// bf16 gradient compression for the bucketed all-reduce (torch's ddp_comm_hooks.default_hooks.bf16_compress_hook):
// a bucket's fp32 gradients are rounded into a bf16 staging buffer, the collective moves half the bytes, and the
// reduced bf16 words are widened back into the fp32 gradient buffer, one launch each per range:
//     compress     c = bf16_rne(g)  or  c = bf16_rne(g + acc)   4 (+ 4) B read, 2 B written per element
//     decompress   g = widen(c)     (bits << 16, exact)         2 B read, 4 B written per element
// The rounding is f2bf's / pack_bf2's (common.h): round to nearest even, a NaN stays a NaN, a finite value at or
// above the bf16 overflow threshold becomes +-inf. With `acc` the sum is exactly one IEEE fp32 add (__fadd_rn: no
// FMA to contract into, nothing reassociated) and then one rounding, so the result is bit-identical to
// DTC_ACCUM_FINISH followed by the plain compress at 10 instead of 18 bytes per element. HBM-bound.
// The fp32 side is 16-byte aligned; the bf16 side is only 8-byte aligned (bucket offsets are multiples of 4
// elements). Compress stores 16 bytes of bf16 per thread: its body works in rows of 8 elements from the first
// 16-byte boundary of `c`, two 16-byte fp32 loads against one 16-byte bf16 store per row. What is left in front of
// that boundary (`head`) and behind the last whole row (`tail`) is 0 or 4 elements each, done with one 8-byte store
// by one thread of workgroup 0. Decompress works in rows of 4 (an 8-byte load, a 16-byte store; see there). The
// compress body is stream_chunks (flat.h), COMPRESS_UNROLL rows of 8 per thread; its workgroup-uniform base and
// 32-bit row index keep the fused form's 16 float4 of loads within the register budget without scratch. Decompress
// keeps its own copy of that loop: on stream_chunks it measured 2% slower (profiles/flat_refactor_ab.json). The
// grids are sized to the range, capped at COMPRESS_MAX_BLOCKS (four workgroups per CU).
// No atomics, vector stores only; every element is written by exactly one thread.
#include "../../include/dtc.h"
#include "flat.h"
#include "kernels.h"

namespace dtc {

constexpr int COMPRESS_THREADS = DTC_COMPRESS_THREADS, COMPRESS_UNROLL = DTC_COMPRESS_UNROLL;
constexpr int COMPRESS_MAX_BLOCKS = DTC_COMPRESS_MAX_BLOCKS;
// four workgroups of four waves per CU = four waves per SIMD: the register budget that keeps the whole capped grid
// resident (the fused compress holds 16 float4 of loads per thread)
constexpr int COMPRESS_WAVES_PER_EU = 4;

template <bool ACC>
__device__ __forceinline__ uint2 compress4(const f32x4& g, const f32x4& a) {
  f32x4 s = g;
  if (ACC) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = __fadd_rn(g[e], a[e]);
  }
  return pack_bf16x4(s);
}
__device__ __forceinline__ f32x4 widen4(uint32_t lo, uint32_t hi) {
  return f32x4{bf_lo(lo), bf_hi(lo), bf_lo(hi), bf_hi(hi)};
}

// g, acc: the first element of the body (16-byte aligned); c: likewise; n8 rows. The `head` elements in front of
// them and the `tail` elements behind the body are 0 or 4.
template <bool ACC>
__global__ void __launch_bounds__(COMPRESS_THREADS, COMPRESS_WAVES_PER_EU)
    grad_compress_kernel(const float* __restrict__ g, const float* __restrict__ acc, u16* __restrict__ c, int64_t n8,
                         int head, int tail) {
  const f32x4* __restrict__ g4 = (const f32x4*)g;
  const f32x4* __restrict__ a4 = (const f32x4*)acc;
  uint4* __restrict__ c8 = (uint4*)c;
  if (blockIdx.x == 0 && threadIdx.x < 2) {  // thread 0: the head row of 4, thread 1: the tail row of 4
    if (threadIdx.x == 0 ? head != 0 : tail != 0) {
      const int64_t r = threadIdx.x == 0 ? -1 : 2 * n8;  // the float4 row relative to the body
      const f32x4 gv = g4[r];
      f32x4 av = gv;
      if (ACC) av = a4[r];
      *(uint2*)(c + r * 4) = compress4<ACC>(gv, av);
    }
  }
  f32x4 gv[COMPRESS_UNROLL][2], av[COMPRESS_UNROLL][2];
  stream_chunks<COMPRESS_THREADS, COMPRESS_UNROLL>(
      n8,
      [&](int k, int64_t base, uint32_t i) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          gv[k][h] = (g4 + 2 * base)[2 * i + h];
          if (ACC) av[k][h] = (a4 + 2 * base)[2 * i + h];
        }
      },
      [&](int k, int64_t base, uint32_t i) {
        const uint2 lo = compress4<ACC>(gv[k][0], ACC ? av[k][0] : gv[k][0]);
        const uint2 hi = compress4<ACC>(gv[k][1], ACC ? av[k][1] : gv[k][1]);
        (c8 + base)[i] = uint4{lo.x, lo.y, hi.x, hi.y};
      });
}

// Widening has no 16-byte constraint on the bf16 side worth a head and a tail: a thread takes rows of 4 elements, one
// 8-byte load against one 16-byte store, both contiguous across the wave (a row of 8 per thread would store two
// float4 32 bytes apart per lane: measured 0.82 of the accumulate kernel's rate, this shape 0.93). The
// stores are 2/3 of the traffic. COMPRESS_UNROLL * 2 rows per thread keep a trip at the compress kernels' size.
constexpr int DECOMPRESS_UNROLL = 2 * COMPRESS_UNROLL;
constexpr int DECOMPRESS_CHUNK4 = COMPRESS_THREADS * DECOMPRESS_UNROLL;  // rows of 4 elements per workgroup trip
__global__ void __launch_bounds__(COMPRESS_THREADS, COMPRESS_WAVES_PER_EU)
    grad_decompress_kernel(const u16* __restrict__ c, float* __restrict__ g, int64_t n4) {
  const uint2* __restrict__ c4 = (const uint2*)c;
  f32x4* __restrict__ g4 = (f32x4*)g;
  const int64_t chunks = (n4 + DECOMPRESS_CHUNK4 - 1) / DECOMPRESS_CHUNK4;
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const uint2* __restrict__ cb = c4 + ch * DECOMPRESS_CHUNK4;
    f32x4* __restrict__ gb = g4 + ch * DECOMPRESS_CHUNK4;
    const uint32_t rows = (uint32_t)std::min<int64_t>(DECOMPRESS_CHUNK4, n4 - ch * DECOMPRESS_CHUNK4);
    uint2 cv[DECOMPRESS_UNROLL];
    if (rows == DECOMPRESS_CHUNK4) {  // uniform over the workgroup: a full chunk, no per-row guard
#pragma unroll
      for (int k = 0; k < DECOMPRESS_UNROLL; ++k) cv[k] = cb[threadIdx.x + k * COMPRESS_THREADS];
#pragma unroll
      for (int k = 0; k < DECOMPRESS_UNROLL; ++k) gb[threadIdx.x + k * COMPRESS_THREADS] = widen4(cv[k].x, cv[k].y);
    } else {  // the ragged last chunk
#pragma unroll
      for (int k = 0; k < DECOMPRESS_UNROLL; ++k) {
        const uint32_t i = threadIdx.x + k * COMPRESS_THREADS;
        if (i < rows) cv[k] = cb[i];
      }
#pragma unroll
      for (int k = 0; k < DECOMPRESS_UNROLL; ++k) {
        const uint32_t i = threadIdx.x + k * COMPRESS_THREADS;
        if (i < rows) gb[i] = widen4(cv[k].x, cv[k].y);
      }
    }
  }
}

// the split of n elements at `c` into head (to the first 16-byte boundary of c), n8 rows of 8 and tail
struct CompressSplit {
  int head, tail;
  int64_t n8;
  dim3 grid;
};
static CompressSplit compress_split(const u16* c, int64_t n) {
  CompressSplit s;
  s.head = aligned(c, 16) ? 0 : 4;
  s.n8 = (n - s.head) / 8;
  s.tail = (int)(n - s.head - s.n8 * 8);
  s.grid = dim3(flat_blocks(s.n8, COMPRESS_THREADS * COMPRESS_UNROLL, COMPRESS_MAX_BLOCKS));
  return s;
}

static int compress_args_ok(const char* fn, const float* g, const float* acc, const u16* c, int64_t n) {
  DTC_CHECK_ARG(g && c, "%s: null pointer (g or c)", fn);
  DTC_CHECK_ARG(mult4(n), "%s: n = %lld must be a positive multiple of 4", fn, (long long)n);
  DTC_CHECK_ARG(aligned(g, 16) && aligned(acc, 16), "%s: g and acc must be 16-byte aligned", fn);
  DTC_CHECK_ARG(aligned(c, 8), "%s: c must be 8-byte aligned", fn);
  DTC_CHECK_ARG(!ranges_overlap(c, n * 2, g, n * 4), "%s: c and g overlap", fn);
  DTC_CHECK_ARG(!acc || !ranges_overlap(c, n * 2, acc, n * 4), "%s: c and acc overlap", fn);
  return 0;
}

int grad_compress_bf16(const float* g, const float* acc, u16* c, int64_t n, hipStream_t st) {
  DTC_TRY(compress_args_ok("grad_compress_bf16", g, acc, c, n));
  const CompressSplit s = compress_split(c, n);
  if (acc)
    DTC_KLAUNCH(grad_compress_kernel<true>, s.grid, dim3(COMPRESS_THREADS), 0, st, g + s.head, acc + s.head, c + s.head,
                s.n8, s.head, s.tail);
  else
    DTC_KLAUNCH(grad_compress_kernel<false>, s.grid, dim3(COMPRESS_THREADS), 0, st, g + s.head, acc, c + s.head, s.n8,
                s.head, s.tail);
  DTC_LAUNCH_CHECK();
  return 0;
}

int grad_decompress_bf16(const u16* c, float* g, int64_t n, hipStream_t st) {
  DTC_TRY(compress_args_ok("grad_decompress_bf16", g, nullptr, c, n));
  const int64_t n4 = n / 4;
  const dim3 grid(flat_blocks(n4, DECOMPRESS_CHUNK4, COMPRESS_MAX_BLOCKS));
  DTC_KLAUNCH(grad_decompress_kernel, grid, dim3(COMPRESS_THREADS), 0, st, c, g, n4);
  DTC_LAUNCH_CHECK();
  return 0;
}

}  // namespace dtc
