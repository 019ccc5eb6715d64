// The RoPE rotation of 8 pairs, shared by rope_kernel (elementwise.hip) and the fused decode
// kernels (decode_step.hip), which promise rope_kernel's bits.
#pragma once
#include "common.h"

// a[j], b[j]: elements i + j and i + D/2 + j of one head; csr: the 8 (cos, sin) float2 entries of the
// position, read as 4 float4 (16-B aligned). sign = +1 rotates forward, -1 is the adjoint.
// The contraction is spelled out, so every caller rounds alike whatever surrounds the call: the
// sine product is rounded on its own and the cosine product is fused into the sum.
__device__ __forceinline__ void rope_rotate8(const float* a, const float* b, const float4* __restrict__ csr,
                                             const float sign, float* oa, float* ob) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 q = csr[j];  // (cos_j0, sin_j0, cos_j1, sin_j1)
    const float c0 = q.x, s0 = sign * q.y, c1 = q.z, s1 = sign * q.w;
    oa[2 * j] = __builtin_fmaf(c0, a[2 * j], -(s0 * b[2 * j]));
    ob[2 * j] = __builtin_fmaf(c0, b[2 * j], s0 * a[2 * j]);
    oa[2 * j + 1] = __builtin_fmaf(c1, a[2 * j + 1], -(s1 * b[2 * j + 1]));
    ob[2 * j + 1] = __builtin_fmaf(c1, b[2 * j + 1], s1 * a[2 * j + 1]);
  }
}
