// What the bf16 (moe.hip) and the MXFP4 (moe_w4.hip) expert FFNs share: the tile constants, the grouping
// kernel, the combine kernel and the workspace layout. Anonymous namespace: each translation unit gets its
// own copy.
#pragma once
#include "common.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int kTilePairs = 16;        // pairs per tile: the MFMA's columns
constexpr int kBN = 64;               // weight rows per block: 4 waves x one 16-wide MFMA tile
constexpr int kMaxSplits = 8;
constexpr int kTargetBlocks = 512;    // two blocks per CU from one tile
constexpr int kMaxE = 64;             // router: an expert's logit lives in its lane
constexpr int kMaxK = 8;
constexpr int kAlignThreads = 1024;

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ------------------------------------------------------------------------------------------ grouping
// wave w owns the experts w, w + NW, ...; a scan of ids takes 64 pairs a step, in ascending pair order.
// Each expert costs two scans of all P ids and no other block runs beside this one: the time grows with
// P E / NW. That is small change at decode sizes; at the thousands of rows of a captured prefill it has not
// been measured (profiles/moe.md).
__global__ __launch_bounds__(kAlignThreads) void moe_align_kernel(const int* __restrict__ ids,
                                                                  int* __restrict__ tile_expert,
                                                                  int* __restrict__ tile_pairs, int P, int E,
                                                                  int n_tiles_max) {
  constexpr int kWaves = kAlignThreads / 64;
  __shared__ int count[kMaxE], first[kMaxE + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;

  for (int e = wave; e < E; e += kWaves) {
    int c = 0;
    for (int p0 = 0; p0 < P; p0 += 64) {
      const int p = p0 + lane;
      c += __popcll(__ballot(p < P && ids[p] == e));
    }
    if (lane == 0) count[e] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int at = 0;
    for (int e = 0; e < E; ++e) {
      first[e] = at;
      at += (count[e] + kTilePairs - 1) / kTilePairs;
    }
    first[E] = at;  // <= n_tiles_max
  }
  __syncthreads();

  for (int e = wave; e < E; e += kWaves) {
    int* out = tile_pairs + (size_t)first[e] * kTilePairs;
    int c = 0;
    for (int p0 = 0; p0 < P; p0 += 64) {
      const int p = p0 + lane;
      const bool mine = p < P && ids[p] == e;
      const unsigned long long b = __ballot(mine);
      if (mine) out[c + __popcll(b & below)] = p;
      c += __popcll(b);
    }
    const int tiles = first[e + 1] - first[e];
    for (int i = c + lane; i < tiles * kTilePairs; i += 64) out[i] = -1;
    for (int i = lane; i < tiles; i += 64) tile_expert[first[e] + i] = e;
  }
  const int used = first[E];
  for (int i = used + tid; i < n_tiles_max; i += kAlignThreads) tile_expert[i] = -1;
  for (long long i = (long long)used * kTilePairs + tid; i < (long long)n_tiles_max * kTilePairs; i += kAlignThreads)
    tile_pairs[i] = -1;
}

// y[t][h..h+3] = bf16(sum_j weights[t][j] * (part[0] + part[1] + ... in range order)[t k + j])
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ part, const int* __restrict__ ids,
                                                          const float* __restrict__ wts, bf16_t* __restrict__ y,
                                                          long long ldy, int T, int k, int H, int E, int splits) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, quads = H / 4;
  if (idx >= (long long)T * quads) return;
  const int t = (int)(idx / quads), h = (int)(idx % quads) * 4;
  const size_t zstride = (size_t)T * k * H;
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < k; ++j) {
    const int pr = t * k + j, e = ids[pr];
    if (e < 0 || e >= E) continue;  // never grouped: nothing was computed for this pair
    const float* p = part + (size_t)pr * H + h;
    f32x4 a = *reinterpret_cast<const f32x4*>(p);
    for (int z = 1; z < splits; ++z) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(p + z * zstride);
      a[0] += b[0], a[1] += b[1], a[2] += b[2], a[3] += b[3];
    }
    const float wj = wts[pr];
    o[0] += wj * a[0], o[1] += wj * a[1], o[2] += wj * a[2], o[3] += wj * a[3];
  }
  uint2 v;
  v.x = (unsigned)f2bf(o[0]) | ((unsigned)f2bf(o[1]) << 16);
  v.y = (unsigned)f2bf(o[2]) | ((unsigned)f2bf(o[3]) << 16);
  *reinterpret_cast<uint2*>(y + (size_t)t * ldy + h) = v;
}

// E and k as the router gives them: one contract for every entry
bool moe_topk_ok(int E, int k) { return E >= 2 && E <= kMaxE && k >= 1 && k <= kMaxK && k <= E; }

// T against the grids, once H and I are within an entry's own contract
bool moe_rows_ok(int T, int H, int k) {
  return T >= 1 && (long long)T * k <= 0x7fffffffLL / kTilePairs && ((long long)T * (H / 4) + 255) / 256 <= 0x7fffffffLL;
}

long long align16(long long n) { return (n + 15) / 16 * 16; }

int moe_tiles_max(int P, int E) { return (E < P ? E : P) + P / kTilePairs; }

// workspace layout: tile_expert | tile_pairs | act | part, each 16-byte aligned
struct MoeWs {
  long long expert, pairs, act, part, total;
};

MoeWs moe_ws(int T, int H, int I, int E, int k, int splits) {
  const long long P = (long long)T * k, nt = moe_tiles_max((int)P, E);
  MoeWs w;
  w.expert = 0;
  w.pairs = align16(nt * 4);
  w.act = w.pairs + align16(nt * kTilePairs * 4);
  w.part = w.act + align16(P * I * 2);
  w.total = w.part + (long long)splits * P * H * 4;
  return w;
}

}  // namespace
