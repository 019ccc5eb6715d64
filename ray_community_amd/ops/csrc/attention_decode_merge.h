// The epilogue of the paged decode kernels as a function (attention_decode_fp8.hip calls it): every
// (lane group, wave) of a 4-wave workgroup arrives with its own running (m, l, O) of a base-2 online
// softmax over the tokens it streamed; they are merged by cross-lane butterflies, then across the
// waves through LDS, and written as the normalised bf16 row (num_splits == 1) or as this split's
// fp32 partial for attn_decode_combine_kernel. attn_decode_paged_kernel (attention_decode.hip)
// keeps the same statements inline: calling this function from it changed its register allocation
// and instruction order, and the bf16 kernel's code is to stay as measured.
#pragma once
#include "attention_combine.h"
#include "attention_common.h"

namespace {

constexpr int kDecWaves = 4;

// exp2(a - m) with m == -inf (nothing seen yet) mapped to a zero reference: exp2(-inf - 0) = 0,
// never exp2(-inf + inf) = NaN
__device__ __forceinline__ float safe_ref(float m) { return m == neg_inf() ? 0.f : m; }

// Lane map of the callers: D / 8 lanes per token (8 columns each, sub = lane % (D / 8)), the
// 64 / (D / 8) lane groups of a wave on different tokens; wave = the caller's wave-uniform
// threadIdx.x / 64.
template <int D, int G>
__device__ __forceinline__ void decode_merge_store(float (&m)[G], float (&l)[G], float (&o)[G][8], int wave, int split,
                                                   int hk, int b, int Hk, int num_splits, bf16_t* __restrict__ out,
                                                   float* __restrict__ part_o, float* __restrict__ part_ml) {
  constexpr int LPT = D / 8;
  __shared__ float sm_o[kDecWaves][G][D];
  __shared__ float sm_m[kDecWaves][G], sm_l[kDecWaves][G];
  const int tid = threadIdx.x, lane = tid & 63;
  const int sub = lane % LPT, grp = lane / LPT;
  const int Hq = Hk * G;

  // merge the lane groups of the wave (butterfly: both partners compute the same sums)
#pragma unroll
  for (int off = LPT; off < 64; off <<= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float mn = fmaxf(m[g], __shfl_xor(m[g], off, 64));
      const float a = fast_exp2(m[g] - safe_ref(mn));
      const float ls = l[g] * a;
      l[g] = ls + __shfl_xor(ls, off, 64);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = o[g][j] * a;
        o[g][j] = x + __shfl_xor(x, off, 64);
      }
      m[g] = mn;
    }
  }
  if (grp == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sm_o[wave][g][sub * 8 + j] = o[g][j];
      if (sub == 0) {
        sm_m[wave][g] = m[g];
        sm_l[wave][g] = l[g];
      }
    }
  }
  __syncthreads();

  // merge the 4 waves in wave order; thread -> (query row g, 8 columns c)
  if (tid < G * LPT) {
    const int g = tid / LPT, c = tid % LPT;
    float mt = neg_inf();
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) mt = fmaxf(mt, sm_m[w][g]);
    const float mr = safe_ref(mt);
    float lt = 0.f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) {
      const float a = fast_exp2(sm_m[w][g] - mr);
      lt += a * sm_l[w][g];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += a * sm_o[w][g][c * 8 + j];
    }
    const int hq = hk * G + g;
    if (num_splits == 1) {
      const float inv = lt > 0.f ? 1.f / lt : 0.f;  // context_len 0: zeros
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] *= inv;
      *reinterpret_cast<u32x4*>(out + ((long)b * Hq + hq) * D + c * 8) = pack8(acc);
    } else {
      const long row = ((long)b * Hq + hq) * num_splits + split;
      float* po = part_o + row * D + c * 8;
      *reinterpret_cast<f32x4*>(po) = f32x4{acc[0], acc[1], acc[2], acc[3]};
      *reinterpret_cast<f32x4*>(po + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
      if (c == 0) *reinterpret_cast<float2*>(part_ml + row * 2) = float2{mt, lt};  // empty split: (-inf, 0)
    }
  }
}

}  // namespace
