// What the sampling kernels of gfx950 share (sampling.hip, sampling_penalties.hip): the
// order-preserving integer keys of the logits, the 16-byte row reader with its ragged head and
// tail, the 2^-40 fixed-point weights and the radix select over a row. One workgroup of 1024
// threads per row throughout; see sampling.hip for the scheme.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kBins = 256;
constexpr int kRep = 8;               // histogram replicas (lane & 7): fewer same-address adds
constexpr int kMaxV = 1 << 20;
constexpr int kMaxTiles = kMaxV / (kThreads * 4) + 2;
constexpr float kFix = 1099511627776.f;  // 2^40: w <= 1 and V <= 2^20, so a row's mass < 2^61
constexpr u64 kNone = ~0ull;

template <typename T>
struct Elem;
template <>
struct Elem<bf16_t> {
  static constexpr int kPer = 8;     // elements per 16-byte load
  static constexpr int kDigits = 2;  // 8-bit radix passes that tell all keys apart
  static __device__ __forceinline__ float to_f(bf16_t v) { return bf2f(v); }
};
template <>
struct Elem<float> {
  static constexpr int kPer = 4;
  static constexpr int kDigits = 4;
  static __device__ __forceinline__ float to_f(float v) { return v; }
};

// Unsigned key with the order of the float (-0 counts as +0, as in a float comparison).
__device__ __forceinline__ unsigned order_key(float x) {
  unsigned b = __float_as_uint(x);
  if ((b & 0x7fffffffu) == 0) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// exp((x - max) / temperature) in fp32, and its 2^-40 fixed-point image (NaN -> 0).
__device__ __forceinline__ float weight(unsigned key, float m, float temp) { return expf((key_value(key) - m) / temp); }

__device__ __forceinline__ u64 fixed(float w) { return w > 0.f ? (u64)(fminf(w, 1.f) * kFix) : 0ull; }

// Keys of the kPer elements at virtual index v .. v+kPer-1 of a row whose elements sit at
// virtual indices [lo, hi) from the 16-byte aligned address a0; bit j of `valid` says whether
// element j is inside the row.
template <typename T>
__device__ __forceinline__ void load_keys(const char* a0, long lo, long hi, long v, unsigned* key, unsigned& valid) {
  constexpr int P = Elem<T>::kPer;
  const T* p = reinterpret_cast<const T*>(a0) + v;
  if (v >= lo && v + P <= hi) {
    const u32x4 raw = *reinterpret_cast<const u32x4*>(p);
    if constexpr (P == 8) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        key[2 * i] = order_key(__uint_as_float(raw[i] << 16));
        key[2 * i + 1] = order_key(__uint_as_float(raw[i] & 0xffff0000u));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) key[i] = order_key(__uint_as_float(raw[i]));
    }
    valid = (1u << P) - 1;
  } else {
    valid = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      key[j] = 0;
      if (v + j >= lo && v + j < hi) {
        key[j] = order_key(Elem<T>::to_f(p[j]));
        valid |= 1u << j;
      }
    }
  }
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const u64 t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct Row {
  const char* a0;  // 16-byte aligned address at or before the row
  long lo, hi;     // the row's elements, as virtual indices from a0
  int ntiles;
};

// Radix select over the row's keys >= floor_key. Count mode (mass == false): the key of the
// need0-th largest element. Mass mode: the smallest key whose elements still have less than
// top_p of the total mass strictly above them. Returns floor_key if nothing crosses (keep all).
// All threads of the block call it and get the same value.
template <typename T>
__device__ unsigned radix_select(const Row& R, bool mass, u64 need0, float top_p, unsigned floor_key, float m,
                                 float temp, u64* hist, u64* bins, u64* sel) {
  constexpr int P = Elem<T>::kPer;
  const int tid = threadIdx.x;
  unsigned prefix = 0, pmask = 0;
  u64 need = need0;
  for (int d = 0; d < Elem<T>::kDigits; ++d) {
    const int shift = 24 - 8 * d;
    for (int i = tid; i < kBins * kRep; i += kThreads) hist[i] = 0;
    if (tid == 0) sel[0] = kNone;
    __syncthreads();
    for (int t = 0; t < R.ntiles; ++t) {
      unsigned key[P], valid;
      load_keys<T>(R.a0, R.lo, R.hi, (long)t * (kThreads * P) + (long)tid * P, key, valid);
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (((valid >> j) & 1) && key[j] >= floor_key && (key[j] & pmask) == prefix) {
          const u64 a = mass ? fixed(weight(key[j], m, temp)) : 1ull;
          if (a) atomicAdd(&hist[((key[j] >> shift) & 255u) * kRep + (tid & (kRep - 1))], a);
        }
      }
    }
    __syncthreads();
    u64 own = 0;
    if (tid < kBins) {
#pragma unroll
      for (int r = 0; r < kRep; ++r) own += hist[tid * kRep + r];
      bins[tid] = own;
    }
    __syncthreads();
    if (tid < kBins) {
      u64 above = 0, total = 0;
      for (int j = 0; j < kBins; ++j) {
        const u64 b = bins[j];
        total += b;
        if (j > tid) above += b;
      }
      if (mass && d == 0) need = (u64)ceil((double)top_p * (double)total);
      if (above < need && need <= above + own) {  // at most one bin
        sel[0] = (u64)tid;
        sel[1] = need - above;
      }
    }
    __syncthreads();
    const u64 s = sel[0];
    need = sel[1];
    __syncthreads();
    if (s == kNone) return floor_key;
    prefix |= (unsigned)s << shift;
    pmask |= 255u << shift;
  }
  return prefix > floor_key ? prefix : floor_key;
}

}  // namespace
