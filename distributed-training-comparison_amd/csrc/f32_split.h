// What the split-bf16 fp32 convs (conv_f32x*.hip) share: the in-kernel operand split (device), and the weight
// gradients' split-K arithmetic (host).
#pragma once
#include <algorithm>

#include "common.h"
#include "tile_common.h"

namespace dtc {

// ---- host: the split-K of conv_f32x_wgrad.hip and conv_f32x_s2_wgrad.hip over `nsteps` reduction steps
// Splits that fill the chip's 256 CUs with (tiles x splits) workgroups, at least four steps each: a split's prologue
// (its first loads and split, not overlapped) and its slab are paid once per workgroup
inline int f32x_wgrad_splits(int tiles, int nsteps) {
  return std::min(std::max(1, 256 / tiles), std::max(1, nsteps / 4));
}
// `splits` equal shares of nsteps, none empty: the splits that run
inline int f32x_wgrad_splits_run(int nsteps, int splits) {
  const int per = (nsteps + splits - 1) / splits;
  return (nsteps + per - 1) / per;
}
// The splits that run with `slab_bytes` on hand, one split's slab being `one` bytes: the slab bounds them, and one
// split needs none. SIZE_MAX: the splits the kernel wants
inline int f32x_wgrad_splits_on_hand(int tiles, int nsteps, size_t one, size_t slab_bytes) {
  const size_t fit = std::min<size_t>(f32x_wgrad_splits(tiles, nsteps), slab_bytes / one);
  return f32x_wgrad_splits_run(nsteps, std::max(1, (int)fit));
}

// Eight fp32 values -> three packed bf16 planes (v_cvt_pk_bf16_f32: round to nearest even). The lean form the conv
// kernel uses: a finite value that rounds to bf16 infinity (|a| >= 2^128 - 2^119) and an infinity give NaN planes.
__device__ __forceinline__ void split8(const float (&v)[8], uint4& q0, uint4& q1, uint4& q2) {
  uint32_t w0[4], w1[4], w2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w0[k] = pack_bf2(v[2 * k], v[2 * k + 1]);
    float ra = v[2 * k] - bf_lo(w0[k]), rb = v[2 * k + 1] - bf_hi(w0[k]);
    w1[k] = pack_bf2(ra, rb);
    ra -= bf_lo(w1[k]);
    rb -= bf_hi(w1[k]);
    w2[k] = pack_bf2(ra, rb);
  }
  q0 = uint4{w0[0], w0[1], w0[2], w0[3]};
  q1 = uint4{w1[0], w1[1], w1[2], w1[3]};
  q2 = uint4{w2[0], w2[1], w2[2], w2[3]};
}

// Eight fp32 (32 B) at byte offset o of a buffer descriptor, as two 16-B loads (an offset outside it: zeros)
__device__ __forceinline__ void f32x_load16(const __amdgpu_buffer_rsrc_t& r, uint32_t o, f32x4 (&d)[2]) {
  d[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, 0));
  d[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o + 16u, 0, 0));
}
// Eight held fp32 -> split8 -> one 16-B store into each of the three plane images, plane_bytes apart
__device__ __forceinline__ void f32x_split_write(const f32x4 (&v2)[2], char* dst, int plane_bytes) {
  const float v[8] = {v2[0][0], v2[0][1], v2[0][2], v2[0][3], v2[1][0], v2[1][1], v2[1][2], v2[1][3]};
  uint4 q0, q1, q2;
  split8(v, q0, q1, q2);
  *(uint4*)dst = q0;
  *(uint4*)(dst + plane_bytes) = q1;
  *(uint4*)(dst + 2 * plane_bytes) = q2;
}
// The trswz swizzle of LDS row r as an 8-B unit XOR
__device__ __forceinline__ int f32x_uswz(int r) { return (((r >> 1) & 1) << 2) | (((r >> 3) & 1) << 3); }
// One bf16 fragment of a tr image from its two ds_read_b64_tr_b16 at byte offsets o0, o1 of sb
__device__ __forceinline__ bf16x8 f32x_tr8(const char* sb, uint32_t o0, uint32_t o1) {
  typedef __attribute__((address_space(3))) bf16x4_t lds_v4;
  const bf16x4_t t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(sb + o0));
  const bf16x4_t t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(sb + o1));
  return __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
}

}  // namespace dtc
