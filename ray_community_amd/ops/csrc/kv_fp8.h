// FP8 paged KV cache: what its kernels share (attention_decode_fp8.hip: quantising append and
// decode; attention_extend.hip: the fp8 stage of the extend kernel). The format is described at the
// top of attention_decode_fp8.hip.
#pragma once
#include "common.h"

typedef unsigned char fp8_t;  // raw OCP e4m3 bits (= torch.float8_e4m3fn)
typedef float f32x2 __attribute__((ext_vector_type(2)));

// 8 e4m3 bytes -> f32 (v_cvt_pk_f32_fp8: exact)
__device__ __forceinline__ void unpack8_fp8(const uint2 v, float* f) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, true);
  f[0] = a[0], f[1] = a[1], f[2] = b[0], f[3] = b[1];
  f[4] = c[0], f[5] = c[1], f[6] = d[0], f[7] = d[1];
}
