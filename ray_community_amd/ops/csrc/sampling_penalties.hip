// What a request asks of a generation step besides a token, for gfx950, next to sampling.hip and
// with its row reader, keys and radix select (sampling_common.h). One workgroup of 1024 threads
// per row of the [B, V] logits in both kernels; a row's result is a bitwise function of that row's
// inputs alone (integer atomics only, no floating-point sum whose order could vary).
//
// penalize_logits_kernel: repetition / presence / frequency penalties over the row's token history
//   (tokens[start:end], of which tokens[prompt_end:end] were produced), written as fp32 [B, V].
//   The vocabulary does not fit in LDS as counters, so the counters are an int32 [B, V] global
//   workspace that is zero on entry and on exit:
//     1. the row streams to the output (16-byte loads and stores where aligned);
//     2. every produced token adds 1 to its counter, every prompt token ORs the top bit in;
//     3. after a fence and a barrier every history position exchanges its counter with 0: the one
//        thread that gets a non-zero value owns the token, computes its logit and stores it.
//   Work is O(V + history), the ids are never sorted or searched, and ids outside [0, V) are
//   skipped before they index anything. Every product and difference is one IEEE fp32 operation
//   (compiled with contraction off: no fma), in the order of reference.penalize_logits_ref.
//
// token_logprobs_kernel: log-softmax of the row at one chosen token and at the top_n <= 20 largest
//   logits (equal logits by ascending index). The maximum as in the sampler, the sum of
//   exp(x - max) in the sampler's 2^-40 fixed point (an integer sum: reproducible), its logarithm
//   in double by one thread, the top_n-th key by the radix select in count mode; the entries above
//   that key are collected through LDS in any order, its ties in index order by a block scan per
//   tile, and the <= 20 entries ranked by (key descending, index ascending).
//
// Semantics: ops.penalize_logits / ops.token_logprobs and their references in ops/reference.py.
#include "sampling_common.h"

namespace {

constexpr int kMaxTop = 20;
constexpr unsigned kPromptBit = 0x80000000u;

// The kPer elements at virtual index v .. v+kPer-1 as fp32, with load_keys' rules: one 16-byte
// load if all of them are inside the row, element by element otherwise.
template <typename T>
__device__ __forceinline__ void load_vals(const char* a0, long lo, long hi, long v, float* x, unsigned& valid) {
  constexpr int P = Elem<T>::kPer;
  const T* p = reinterpret_cast<const T*>(a0) + v;
  if (v >= lo && v + P <= hi) {
    const u32x4 raw = *reinterpret_cast<const u32x4*>(p);
    if constexpr (P == 8) {
      unpack8(raw, x);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = __uint_as_float(raw[i]);
    }
    valid = (1u << P) - 1;
  } else {
    valid = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      x[j] = 0.f;
      if (v + j >= lo && v + j < hi) {
        x[j] = Elem<T>::to_f(p[j]);
        valid |= 1u << j;
      }
    }
  }
}

template <typename T>
__device__ __forceinline__ Row make_row(const T* row, int V) {
  Row R;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(row);
  R.a0 = reinterpret_cast<const char*>(addr & ~(uintptr_t)15);
  R.lo = (long)((addr & 15) / sizeof(T));
  R.hi = R.lo + V;
  R.ntiles = (int)((R.hi + kThreads * Elem<T>::kPer - 1) / (kThreads * Elem<T>::kPer));
  return R;
}

// One IEEE fp32 product / difference each, never contracted into an fma with a neighbour (the
// __fmul_rn / __fsub_rn of the HIP headers are plain operators, which -ffp-contract=fast may fuse).
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename T>
__global__ __launch_bounds__(kThreads) void penalize_logits_kernel(const T* __restrict__ logits, long long row_stride,
                                                                   const int* __restrict__ tokens,
                                                                   const int* __restrict__ ranges,
                                                                   const float* __restrict__ params,
                                                                   unsigned* __restrict__ counts,
                                                                   float* __restrict__ out, int V, int T_len) {
  constexpr int P = Elem<T>::kPer;
  constexpr int kTile = kThreads * P;
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  const T* src = logits + row * row_stride;
  const Row R = make_row<T>(src, V);
  float* dst = out + row * (long)V;
  unsigned* cnt = counts + row * (long)V;

  // 1. the fp32 image of the row; element e = v - lo goes to dst + e, 16-byte aligned for every
  // whole group iff it is for v = 0
  const bool vec = ((reinterpret_cast<uintptr_t>(dst) - (uintptr_t)R.lo * 4) & 15) == 0;
  for (int t = 0; t < R.ntiles; ++t) {
    float x[P];
    unsigned valid;
    const long v = (long)t * kTile + (long)tid * P;
    load_vals<T>(R.a0, R.lo, R.hi, v, x, valid);
    float* d = dst + (v - R.lo);
    if (vec && valid == (1u << P) - 1) {
#pragma unroll
      for (int i = 0; i < P / 4; ++i) {
        f32x4 o = {x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]};
        *reinterpret_cast<f32x4*>(d + 4 * i) = o;
      }
    } else {
#pragma unroll
      for (int j = 0; j < P; ++j)
        if ((valid >> j) & 1) d[j] = x[j];
    }
  }

  const float rep = params[row * 4], inv_rep = params[row * 4 + 1], freq = params[row * 4 + 2],
              pres = params[row * 4 + 3];
  if (rep == 1.f && freq == 0.f && pres == 0.f) return;  // neutral: the copy, whatever the history
  const int start = clampi(ranges[row * 3], 0, T_len);
  const int prompt_end = clampi(ranges[row * 3 + 1], start, T_len);
  const int end = clampi(ranges[row * 3 + 2], prompt_end, T_len);

  // 2. counts of the produced tokens, the top bit for the prompt's
  for (int p = start + tid; p < end; p += kThreads) {
    const int id = tokens[p];
    if (id >= 0 && id < V) {
      if (p >= prompt_end) {
        atomicAdd(&cnt[id], 1u);
      } else {
        atomicOr(&cnt[id], kPromptBit);
      }
    }
  }
  __threadfence();
  __syncthreads();  // every counter is final, and every store of phase 1 is behind us

  // 3. one owner per distinct token; the counters go back to zero
  for (int p = start + tid; p < end; p += kThreads) {
    const int id = tokens[p];
    if (id >= 0 && id < V) {
      const unsigned got = atomicExch(&cnt[id], 0u);
      if (got) {
        const unsigned c = got & ~kPromptBit;
        const float x = Elem<T>::to_f(src[id]);
        float y = x > 0.f ? mul_rn(x, inv_rep) : mul_rn(x, rep);
        y = sub_rn(y, mul_rn(freq, (float)c));
        if (c) y = sub_rn(y, pres);
        dst[id] = y;
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void token_logprobs_kernel(const T* __restrict__ logits, long long row_stride,
                                                                  const long long* __restrict__ tokens,
                                                                  float* __restrict__ lp,
                                                                  long long* __restrict__ top_ids,
                                                                  float* __restrict__ top_lp, int V, int top_n) {
  constexpr int P = Elem<T>::kPer;
  constexpr int kTile = kThreads * P;
  constexpr unsigned kKeyMask = P == 8 ? 0xffff0000u : 0xffffffffu;  // the bits the radix select tells apart
  __shared__ u64 hist[kBins * kRep];
  __shared__ u64 bins[kBins];
  __shared__ u64 red[kWaves];
  __shared__ u64 sel[2];
  __shared__ u64 cand[kMaxTop];
  __shared__ unsigned wtot[kWaves];
  __shared__ unsigned nabove;
  __shared__ double log_sum;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long row = blockIdx.x;
  const T* src = logits + row * row_stride;
  const Row R = make_row<T>(src, V);

  // the maximum, as in sample_logits_kernel
  u64 best = 0;
  for (int t = 0; t < R.ntiles; ++t) {
    unsigned key[P], valid;
    const long v = (long)t * kTile + (long)tid * P;
    load_keys<T>(R.a0, R.lo, R.hi, v, key, valid);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const u64 pk = ((u64)key[j] << 32) | (u64)(0xffffffffu - (unsigned)(v + j - R.lo));
      if (((valid >> j) & 1) && pk > best) best = pk;
    }
  }
  best = wave_max_u64(best);
  if (lane == 0) red[wid] = best;
  __syncthreads();
  best = 0;
  for (int i = 0; i < kWaves; ++i) best = red[i] > best ? red[i] : best;
  const float m = key_value((unsigned)(best >> 32));
  __syncthreads();  // every read of red[] above is over

  // S = sum exp(x - m) in 2^-40 fixed point, log S in double
  u64 s = 0;
  for (int t = 0; t < R.ntiles; ++t) {
    unsigned key[P], valid;
    load_keys<T>(R.a0, R.lo, R.hi, (long)t * kTile + (long)tid * P, key, valid);
#pragma unroll
    for (int j = 0; j < P; ++j)
      if ((valid >> j) & 1) s += fixed(expf(key_value(key[j]) - m));
  }
  s = wave_sum_u64(s);
  if (lane == 0) red[wid] = s;
  __syncthreads();
  if (tid == 0) {
    u64 total = 0;
    for (int i = 0; i < kWaves; ++i) total += red[i];
    log_sum = log((double)total * 9.094947017729282e-13);  // 2^-40
    nabove = 0;
  }
  __syncthreads();
  const double ls = log_sum;
  auto logprob = [&](float x) { return (float)((double)(x - m) - ls); };

  if (tid == 0) {
    const long long tok = tokens[row];
    lp[row] = (tok >= 0 && tok < V) ? logprob(Elem<T>::to_f(src[tok])) : __uint_as_float(0x7fc00000u);
  }
  const int n = top_n < V ? top_n : V;
  for (int i = n + tid; i < top_n; i += kThreads) {
    top_ids[row * top_n + i] = -1;
    top_lp[row * top_n + i] = __uint_as_float(0xff800000u);
  }
  if (n == 0) return;

  // the key of the n-th largest logit; in count mode the select leaves in sel[1] how many of that
  // key's elements are among the n
  const unsigned thr = radix_select<T>(R, false, (u64)n, 0.f, 0u, m, 1.f, hist, bins, sel) & kKeyMask;
  const unsigned need_ties = (unsigned)sel[1] < (unsigned)n ? (unsigned)sel[1] : (unsigned)n;
  const unsigned first_tie = (unsigned)n - need_ties;
  unsigned taken = 0;
  for (int t = 0; t < R.ntiles; ++t) {
    unsigned key[P], valid, c = 0;
    const long v = (long)t * kTile + (long)tid * P;
    load_keys<T>(R.a0, R.lo, R.hi, v, key, valid);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if ((valid >> j) & 1) {
        const unsigned kk = key[j] & kKeyMask;
        if (kk > thr) {
          const unsigned slot = atomicAdd(&nabove, 1u);
          if (slot < first_tie) cand[slot] = ((u64)key[j] << 32) | (u64)(0xffffffffu - (unsigned)(v + j - R.lo));
        } else if (kk == thr) {
          ++c;
        }
      }
    }
    if (taken < need_ties) {  // the same for every thread: ties in index order by a block scan
      unsigned incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
      }
      if (lane == 63) wtot[wid] = incl;
      __syncthreads();
      unsigned r = taken + incl - c, total = 0;
      for (int i = 0; i < kWaves; ++i) {
        if (i < wid) r += wtot[i];
        total += wtot[i];
      }
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (((valid >> j) & 1) && (key[j] & kKeyMask) == thr) {
          if (r < need_ties) cand[first_tie + r] = ((u64)key[j] << 32) | (u64)(0xffffffffu - (unsigned)(v + j - R.lo));
          ++r;
        }
      }
      taken += total;
      __syncthreads();  // wtot[] is free again
    }
  }
  __syncthreads();
  if (tid < n) {
    const u64 mine = cand[tid];
    int rank = 0;
    for (int i = 0; i < n; ++i) rank += cand[i] > mine;
    top_ids[row * top_n + rank] = (long long)(0xffffffffu - (unsigned)mine);
    top_lp[row * top_n + rank] = logprob(key_value((unsigned)(mine >> 32)));
  }
}

}  // namespace

// logits: [B, V] bf16 (is_bf16 != 0) or fp32, unit inner stride, row_stride in elements.
// tokens: int32 [T]; ranges: int32 [B, 3] = (start, prompt_end, end) into tokens;
// params: fp32 [B, 4] = (repetition, 1 / repetition, frequency, presence);
// counts: int32 [B, V], zero on entry and on exit; out: fp32 [B, V] contiguous.
RCA_API int rca_penalize_logits(const void* logits, long long row_stride, int is_bf16, const void* tokens,
                                const void* ranges, const void* params, void* counts, void* out, int B, int V, int T,
                                hipStream_t st) {
  if (B < 0 || B > 65535 || V < 1 || V > kMaxV || T < 0) return 1;
  if (B == 0) return 0;
  if (!logits || !ranges || !params || !counts || !out || (T > 0 && !tokens)) return 2;
  if (is_bf16) {
    hipLaunchKernelGGL(penalize_logits_kernel<bf16_t>, dim3(B), dim3(kThreads), 0, st, (const bf16_t*)logits, row_stride,
                       (const int*)tokens, (const int*)ranges, (const float*)params, (unsigned*)counts, (float*)out, V,
                       T);
  } else {
    hipLaunchKernelGGL(penalize_logits_kernel<float>, dim3(B), dim3(kThreads), 0, st, (const float*)logits, row_stride,
                       (const int*)tokens, (const int*)ranges, (const float*)params, (unsigned*)counts, (float*)out, V,
                       T);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// tokens: int64 [B] (an id outside [0, V) gives NaN); lp: fp32 [B]; top_ids: int64 [B, top_n];
// top_lp: fp32 [B, top_n]; 0 <= top_n <= 20 (both may be null at 0).
RCA_API int rca_token_logprobs(const void* logits, long long row_stride, int is_bf16, const void* tokens, void* lp,
                               void* top_ids, void* top_lp, int B, int V, int top_n, hipStream_t st) {
  if (B < 0 || B > 65535 || V < 1 || V > kMaxV || top_n < 0 || top_n > kMaxTop) return 1;
  if (B == 0) return 0;
  if (!logits || !tokens || !lp || (top_n > 0 && (!top_ids || !top_lp))) return 2;
  if (is_bf16) {
    hipLaunchKernelGGL(token_logprobs_kernel<bf16_t>, dim3(B), dim3(kThreads), 0, st, (const bf16_t*)logits, row_stride,
                       (const long long*)tokens, (float*)lp, (long long*)top_ids, (float*)top_lp, V, top_n);
  } else {
    hipLaunchKernelGGL(token_logprobs_kernel<float>, dim3(B), dim3(kThreads), 0, st, (const float*)logits, row_stride,
                       (const long long*)tokens, (float*)lp, (long long*)top_ids, (float*)top_lp, V, top_n);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
