// The in-kernel operand split of the split-bf16 fp32 convs (conv_f32x.hip, conv_f32x_wgrad.hip): device code only.
#pragma once
#include "common.h"

namespace dtc {

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

}  // namespace dtc
