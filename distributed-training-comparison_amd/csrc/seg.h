// The segment plan as the per-tensor kernels see it (lars.hip, lamb.hip): the device tables, the work map that gives
// one workgroup one SEG_CHUNK-element chunk of one segment, the partial slots and their fold in index order.
// Internal: not part of the C ABI. The plan's host side (segplan_create / bind) is lars.hip's.
#pragma once
#include <vector>
#include "flat.h"

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
struct SegSums {  // one partial slot: sum p^2 and the second sum of squares (LARS: g, LAMB: the direction u)
  double p, g;
};
struct SegResult {  // per segment: ||p||, the second norm (LARS: |mult| * ||g||, LAMB: ||u||), ratio
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

// One wave (64 threads) folds the slots of segment `s` (a SegDev) in index order: declares the doubles `sp`, `sg` and
// adds the slots' .p and .g into them, 512 slots staged in LDS per memory latency (ResNet-18's largest tensor has
// 288), added by thread 0; the sums are valid in thread 0 only. A macro, once per kernel: a function, even a
// force-inlined one, is simplified on its own before it is inlined, and the code of seg_ratio_kernel, which this was
// lifted from, then comes out with other branches; the text expanded in place compiles to the same bytes.
#define DTC_SEG_FOLD_SLOTS(s, slots, sp, sg)                                           \
  constexpr int TILE = 512;                                                            \
  __shared__ SegSums sh[TILE];                                                         \
  double sp = 0.0, sg = 0.0;                                                           \
  for (int base = 0; base < s.nchunks; base += TILE) {                                 \
    _Pragma("unroll") for (int j = 0; j < TILE / 64; ++j) {                            \
      const int k = base + j * 64 + threadIdx.x;                                       \
      if (k < s.nchunks) sh[j * 64 + threadIdx.x] = slots[s.first_chunk + k];          \
    }                                                                                  \
    __syncthreads();                                                                   \
    if (threadIdx.x == 0) {                                                            \
      const int m = s.nchunks - base < TILE ? s.nchunks - base : TILE;                 \
      _Pragma("unroll 8") for (int j = 0; j < m; ++j) {                                \
        sp += sh[j].p;                                                                 \
        sg += sh[j].g;                                                                 \
      }                                                                                \
    }                                                                                  \
    __syncthreads();                                                                   \
  }

}  // namespace dtc
