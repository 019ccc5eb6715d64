// MXFP4 (OCP e2m1 nibbles, E8M0 block scales) to bf16 in registers: shared by the dense W4A16 linear
// (linear_w4.hip) and the grouped W4A16 expert FFN (moe_w4.hip). Anonymous namespace: each translation unit
// gets its own copy.
#pragma once
#include "common.h"

namespace {

// 4 bytes = 8 e2m1 nibbles (k ascending: low nibble first) times `scale` (a power of two) -> 8 bf16, exact
__device__ __forceinline__ u32x4 w4_cvt8(unsigned w, float scale) {
  u32x4 r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
  return r;
}

// the float 2^(e - 127) of an E8M0 byte (2 <= e <= 252: normal)
__device__ __forceinline__ float e8m0(unsigned e) { return __uint_as_float(e << 23); }

}  // namespace
