// Shared pieces of the streaming kernels over the flat fp32 buffers (optim.hip, lars.hip, ema.hip, accum.hip,
// compress.hip). Internal: not part of the C ABI. A new optimizer or compression dtype is a functor on these, not
// another copy of the loops.
#pragma once
#include <algorithm>
#include "common.h"

namespace dtc {

// ---------------------------------------------------------------- host: grids and argument checks
// workgroups for `rows` rows at `per_block` rows each, at least one and at most `cap`
inline int flat_blocks(int64_t rows, int per_block, int cap) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(cap, (rows + per_block - 1) / per_block));
}
inline bool aligned(const void* p, size_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }  // bytes: a power of 2
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
inline bool mult4(int64_t n) { return n > 0 && (n % 4) == 0; }  // "a positive multiple of 4"

// ---------------------------------------------------------------- the chunked streaming loop
// A workgroup of THREADS takes chunks of THREADS * UNROLL rows and strides over them by the grid; a thread's UNROLL
// rows lie THREADS apart. load(k, base, i) and store(k, base, i) are called for the thread's k-th row, row i of the
// chunk that starts at row `base`: `base` is workgroup-uniform (scalar registers) and `i` a 32-bit index, so a load
// needs one address register. In a full chunk every load is issued before the first store's arithmetic, unguarded;
// the ragged last chunk guards each row. Every row is visited by exactly one thread. A scheduling barrier separates
// the two phases of a full chunk: without it the scheduler starts the fused compress's adds after 11 of its 16 loads.
template <int THREADS, int UNROLL, typename Load, typename Store>
__device__ __forceinline__ void stream_chunks(int64_t rows, Load&& load, Store&& store) {
  constexpr int CHUNK = THREADS * UNROLL;
  const int64_t chunks = (rows + CHUNK - 1) / CHUNK;
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t base = ch * CHUNK;
    const uint32_t left = (uint32_t)std::min<int64_t>(CHUNK, rows - base);
    if (left == CHUNK) {  // uniform over the workgroup
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) load(k, base, threadIdx.x + k * THREADS);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < UNROLL; ++k) store(k, base, threadIdx.x + k * THREADS);
    } else {
#pragma unroll
      for (int k = 0; k < UNROLL; ++k)
        if (threadIdx.x + k * THREADS < left) load(k, base, threadIdx.x + k * THREADS);
#pragma unroll
      for (int k = 0; k < UNROLL; ++k)
        if (threadIdx.x + k * THREADS < left) store(k, base, threadIdx.x + k * THREADS);
    }
  }
}

// ---------------------------------------------------------------- the plain grid-stride loop
// f(i) for every i < n, 256 threads per workgroup; an element-wise operation is a functor struct
template <typename F>
__global__ void __launch_bounds__(256) flat_map_kernel(int64_t n, F f) {
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) f(i);
}
template <typename F>
int launch_map(int64_t n, int max_blocks, hipStream_t st, F f) {
  DTC_KLAUNCH(flat_map_kernel<F>, dim3(flat_blocks(n, 256, max_blocks)), dim3(256), 0, st, n, f);
  DTC_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- fixed-order double-precision sums
__device__ __forceinline__ double sumsq4(double acc, const f32x4& a) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double d = (double)a[k];
    acc += d * d;
  }
  return acc;
}
// N per-thread sums over a workgroup of THREADS: a butterfly over the wave (a + b == b + a: every lane gets the same
// bits), lane 0 of each wave to LDS, thread 0 adds the waves in index order. The totals are valid in thread 0 only.
// No floating-point atomics: bit-identical from run to run.
template <int THREADS, int N>
__device__ __forceinline__ void block_sum_ordered(double (&v)[N]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] += __shfl_xor(v[j], o, 64);
  }
  __shared__ double wsum[THREADS / 64][N];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) wsum[threadIdx.x >> 6][j] = v[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) {
#pragma unroll
      for (int j = 0; j < N; ++j) v[j] += wsum[w][j];
    }
  }
}

// ---------------------------------------------------------------- bf16 shadow of four fp32 values (8 bytes)
__device__ __forceinline__ uint2 pack_bf16x4(const f32x4& v) {
  return uint2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
}
__device__ __forceinline__ void store_bf16x4(u16* p, const f32x4& v) { *(uint2*)p = pack_bf16x4(v); }

// ---------------------------------------------------------------- SGD momentum step on d (T: f32x4 or float)
//     buf = mu * buf + d ;  u = nesterov ? d + mu * buf : buf ;  p -= lr * u
template <bool NESTEROV, typename T>
__device__ __forceinline__ void momentum_step(T& p, T& m, const T& d, float mu, float lr) {
  m = m * mu + d;
  const T u = NESTEROV ? d + m * mu : m;
  p = p - u * lr;
}

}  // namespace dtc
