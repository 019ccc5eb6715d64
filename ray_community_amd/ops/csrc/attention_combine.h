// The split-KV merge shared by the paged decode (attention_decode.hip) and the paged extend
// (attention_extend.hip) kernels. Anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }

// out[row] = sum_s exp2(m_s - m) O_s / sum_s exp2(m_s - m) l_s over the splits in index order.
// Empty splits (m = -inf, l = 0) are skipped, not multiplied by zero; a row whose splits are all
// empty (context_len 0) writes zeros. One thread per 8 output columns.
__global__ __launch_bounds__(256) void attn_decode_combine_kernel(const float* __restrict__ part_o,
                                                                  const float* __restrict__ part_ml,
                                                                  bf16_t* __restrict__ out, long rows, int num_splits,
                                                                  int D) {
  const int lpt = D / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = idx / lpt;
  const int c = (int)(idx % lpt);
  if (row >= rows) return;
  const float* ml = part_ml + row * num_splits * 2;
  float mt = neg_inf();
  for (int s = 0; s < num_splits; ++s) mt = fmaxf(mt, ml[2 * s]);
  float lt = 0.f, acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int s = 0; s < num_splits; ++s) {
    const float ms = ml[2 * s];
    if (ms == neg_inf()) continue;
    const float a = __builtin_amdgcn_exp2f(ms - mt);
    lt += a * ml[2 * s + 1];
    const float* po = part_o + (row * num_splits + s) * D + c * 8;
    const f32x4 x = *reinterpret_cast<const f32x4*>(po), y = *reinterpret_cast<const f32x4*>(po + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] += a * x[j];
      acc[4 + j] += a * y[j];
    }
  }
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] *= inv;
  *reinterpret_cast<u32x4*>(out + row * D + c * 8) = pack8(acc);
}

// rows = output rows of D columns ((sequence or token) x query head); part_o fp32
// [rows, num_splits, D], part_ml fp32 [rows, num_splits, 2] = (m, l), out bf16 [rows, D].
inline int launch_split_combine(const float* part_o, const float* part_ml, bf16_t* out, long rows, int num_splits, int D,
                                hipStream_t stream) {
  const long n = rows * (D / 8);
  if (n <= 0) return 0;
  if ((n + 255) / 256 >= (1L << 31)) return -2;
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part_o,
                     part_ml, out, rows, num_splits, D);
  return (int)hipGetLastError();
}

}  // namespace
