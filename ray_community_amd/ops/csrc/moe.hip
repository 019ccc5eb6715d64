// Sparse mixture-of-experts FFN for inference (Mixtral): a top-k router and the grouped expert SwiGLU MLP,
// y[t] = sum_j weights[t][j] * W_d[e] . bf16(silu(W_g[e] . x[t]) * (W_u[e] . x[t])), e = ids[t][j].
//
// Operands (ops/reference.py, moe_route_ref / moe_ffn_ref): x [T][H] and y [T][H] bf16 with row strides;
// w_router [E][H], w_gate_up [E][2I][H] (gate rows, then up rows) and w_down [E][H][I] bf16, contiguous;
// ids [T][k] int32 and weights [T][k] fp32. Pair p = t * k + j is row t taken through expert ids[t][j].
//
// Routing. moe_route_kernel: one wave per token; the lanes split H in 16-byte pieces, every expert's
// logit is summed over the wave in a fixed butterfly and lane 0 picks the k largest (equal logits: the
// lower expert first) and takes their softmax.
//
// Grouping on the device. moe_align_kernel: ONE workgroup turns ids into tile_expert [n_tiles_max] and
// tile_pairs [n_tiles_max][16]: tiles of up to 16 pairs of one expert, experts ascending, an expert's
// pairs ascending, -1 as padding and for the unused tiles. n_tiles_max = min(E, T k) + T k / 16 bounds
// sum_e ceil(count_e / 16), so the host sizes every later grid without reading the counts; a block whose
// tile is unused returns at once. An id outside [0, E) matches no expert and is in no tile. Ballots and
// prefix counts, no atomics: every word of both arrays is written exactly once.
//
// Two tile GEMMs (moe_tile_gemm), as lora.hip's shrink: the expert's weight rows are the MFMA row operand,
// streamed from global as in linear_w8.hip (per 128-deep chunk lane (n = lane & 15, g = lane >> 4) loads
// the 64 bytes W[n][k0 + 32 g ..] and feeds 4 v_mfma_f32_16x16x32_bf16; the next 256-deep stage's weight
// registers are in flight while the current MFMAs run); the tile's source rows are gathered by pair into
// LDS in 256-deep stages, two buffers, and are the column operand.
//   moe_gate_up_kernel  grid (tile, I / 64): wave w owns 16 gate rows and the matching 16 up rows, two
//                       accumulators; act[p] = bf16(silu(g) * u), one rounding, pair-major [T k][I].
//   moe_down_kernel     grid (tile, H / 64, splits): fp32 partials part [splits][T k][H].
// moe_combine_kernel: y[t] = bf16(sum_j weights[t][j] * (part[0] + part[1] + ...)[t k + j]), ranges in
// ascending order, then j ascending; a pair with an id outside [0, E) is skipped (its rows of act and part
// were never written).
//
// splits depends on (H, I) ONLY, every range is summed in ascending chunks, the partials are added in
// range order and nothing is atomic: an output row is a function of its own x row, its ids and weights and
// the expert weights, whatever T is and in whichever tile and position its pairs sit (an MFMA column
// depends on its own column operand only), and results are bitwise reproducible. Padding rows of a tile
// are zeros in LDS and are not stored.
#include "common.h"
#include "moe_common.h"  // the tile constants, lds_barrier, moe_align_kernel, moe_combine_kernel, the workspace layout

namespace {

constexpr int kKT = 256;              // k per LDS stage
constexpr int kRowB = kKT * 2 + 16;   // LDS bytes per source row: +16 so the 16 m-lanes of a read start 4 banks apart
constexpr int kBufB = kTilePairs * kRowB;
constexpr int kMinSplitBlocks = 4;    // a K range is at least 4 x 128 deep

// ------------------------------------------------------------------------------------------- router
__global__ __launch_bounds__(256) void moe_route_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                        const bf16_t* __restrict__ w, int* __restrict__ ids,
                                                        float* __restrict__ wts, int T, int H, int E, int k) {
  __shared__ float logit[4][kMaxE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 4 + wave;
  const int pieces = H / 8;
  if (t < T) {
    const bf16_t* xr = x + (size_t)t * ldx;
    for (int e = 0; e < E; ++e) {
      const bf16_t* wr = w + (size_t)e * H;
      float s = 0.f;
      for (int p = lane; p < pieces; p += 64) {
        float xf[8], wf[8];
        unpack8(*reinterpret_cast<const u32x4*>(xr + p * 8), xf);
        unpack8(*reinterpret_cast<const u32x4*>(wr + p * 8), wf);
#pragma unroll
        for (int i = 0; i < 8; ++i) s = fmaf(xf[i], wf[i], s);
      }
      s = wave_sum(s);  // xor butterfly: the same order, and the same bits, in every lane
      if (lane == e) logit[wave][e] = s;
    }
  }
  lds_barrier();
  if (t >= T || lane != 0) return;
  const float* lg = logit[wave];
  unsigned long long taken = 0ull;
  int pick[kMaxK];
  float val[kMaxK];
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) {  // constant bounds: pick and val stay in registers
    int best = -1;
    float bv = 0.f;
    if (j < k) {
      for (int e = 0; e < E; ++e) {  // ascending e and a strict >: of equal logits the lower expert wins
        if ((taken >> e) & 1ull) continue;
        const float v = lg[e];
        if (best < 0 || v > bv) best = e, bv = v;
      }
      taken |= 1ull << best;
    }
    pick[j] = best;
    val[j] = bv;
  }
  const float top = val[0];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) {
    val[j] = j < k ? expf(val[j] - top) : 0.f;
    sum += val[j];
  }
#pragma unroll
  for (int j = 0; j < kMaxK; ++j) {
    if (j < k) {
      ids[(size_t)t * k + j] = pick[j];
      wts[(size_t)t * k + j] = val[j] / sum;
    }
  }
}

// --------------------------------------------------------------------------------------- tile GEMMs
// acc[s] += W_s[16 rows of this wave][kbeg .. kend) . src[16 pairs of the tile][kbeg .. kend)^T for NS row
// sets. wrow[s]: this lane's weight row, + 32 g. The source row of pair p is src + (p / div) * ld.
template <int NS>
__device__ __forceinline__ void moe_tile_gemm(const bf16_t* __restrict__ src, long long ld, int div, int P,
                                              const int* __restrict__ pairs, const bf16_t* const (&wrow)[NS], int kbeg,
                                              int kend, f32x4 (&acc)[NS], char* lds) {
  constexpr int kPieces = kTilePairs * (kKT / 8) / 256;  // 16-byte pieces of a source tile per thread
  const int tid = threadIdx.x, lane = tid & 63;
  const int ln = lane & 15, g = lane >> 4;

  // the source rows this thread stages: a padding (or out of range) pair is zeros
  const bf16_t* xsrc[kPieces];
#pragma unroll
  for (int i = 0; i < kPieces; ++i) {
    const int p = tid + 256 * i, pr = pairs[p >> 5];
    xsrc[i] = (pr >= 0 && pr < P) ? src + (size_t)(pr / div) * ld + (p & 31) * 8 : nullptr;
  }
  u32x4 xr[kPieces], wn[NS][2][4];
  auto load_x = [&](int k) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int col = ((tid + 256 * i) & 31) * 8;
      xr[i] = u32x4{0u, 0u, 0u, 0u};
      if (xsrc[i] != nullptr && k + col < kend) xr[i] = *reinterpret_cast<const u32x4*>(xsrc[i] + k);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int p = tid + 256 * i;
      *reinterpret_cast<u32x4*>(lds + buf * kBufB + (p >> 5) * kRowB + (p & 31) * 16) = xr[i];
    }
  };
  auto load_w = [&](int k) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          wn[s][c][j] = u32x4{0u, 0u, 0u, 0u};
          if (k + c * 128 < kend) wn[s][c][j] = *reinterpret_cast<const u32x4*>(wrow[s] + k + c * 128 + 8 * j);
        }
  };

  if (kbeg < kend) {
    load_x(kbeg);
    load_w(kbeg);
    store_x(0);
    lds_barrier();
  }
  int buf = 0;
  for (int k = kbeg; k < kend; k += kKT, buf ^= 1) {
    u32x4 wc[NS][2][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) wc[s][c][j] = wn[s][c][j];
    const bool more = k + kKT < kend;
    if (more) {
      load_x(k + kKT);
      load_w(k + kKT);
    }
    const char* xb = lds + buf * kBufB + ln * kRowB + g * 64;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (k + c * 128 < kend) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bf16x8_t xf = *reinterpret_cast<const bf16x8_t*>(xb + c * 256 + j * 16);
#pragma unroll
          for (int s = 0; s < NS; ++s)
            acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wc[s][c][j]), xf, acc[s], 0, 0, 0);
        }
      }
    }
    if (more) store_x(buf ^ 1);
    lds_barrier();
  }
}

__global__ __launch_bounds__(256) void moe_gate_up_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                          const bf16_t* __restrict__ Wgu,
                                                          const int* __restrict__ tile_expert,
                                                          const int* __restrict__ tile_pairs, bf16_t* __restrict__ act,
                                                          int P, int k, int H, int I, int E) {
  __shared__ __attribute__((aligned(16))) char lds[2 * kBufB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ln = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int e = tile_expert[tile];
  if (e < 0 || e >= E) return;  // the whole block: never index the weights with a bad expert
  const int i0 = blockIdx.y * kBN + wave * 16;  // I % 64 == 0: every wave has a whole tile
  const bf16_t* gate = Wgu + ((size_t)e * 2 * I + i0 + ln) * H + g * 32;
  const bf16_t* const wrow[2] = {gate, gate + (size_t)I * H};
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  moe_tile_gemm<2>(x, ldx, k, P, tile_pairs + (size_t)tile * kTilePairs, wrow, 0, H, acc, lds);

  // lane holds gate and up [i = i0 + 4 g + r][pair = ln], r = 0..3
  const int pr = tile_pairs[(size_t)tile * kTilePairs + ln];
  if (pr < 0 || pr >= P) return;
  float a[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = acc[0][r] / (1.f + expf(-acc[0][r])) * acc[1][r];
  uint2 o;
  o.x = (unsigned)f2bf(a[0]) | ((unsigned)f2bf(a[1]) << 16);
  o.y = (unsigned)f2bf(a[2]) | ((unsigned)f2bf(a[3]) << 16);
  *reinterpret_cast<uint2*>(act + (size_t)pr * I + i0 + 4 * g) = o;
}

__global__ __launch_bounds__(256) void moe_down_kernel(const bf16_t* __restrict__ act, const bf16_t* __restrict__ Wd,
                                                       const int* __restrict__ tile_expert,
                                                       const int* __restrict__ tile_pairs, float* __restrict__ part,
                                                       int P, int H, int I, int E, int per) {
  __shared__ __attribute__((aligned(16))) char lds[2 * kBufB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ln = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int e = tile_expert[tile];
  if (e < 0 || e >= E) return;
  const int h0 = blockIdx.y * kBN + wave * 16;  // H % 64 == 0
  const int kblocks = I / 128;
  const int kb0 = min((int)blockIdx.z * per, kblocks), kb1 = min(kb0 + per, kblocks);
  const bf16_t* const wrow[1] = {Wd + ((size_t)e * H + h0 + ln) * I + g * 32};
  f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
  moe_tile_gemm<1>(act, I, 1, P, tile_pairs + (size_t)tile * kTilePairs, wrow, kb0 * 128, kb1 * 128, acc, lds);

  // lane holds D[h = h0 + 4 g + r][pair = ln]; an empty range stores zeros
  const int pr = tile_pairs[(size_t)tile * kTilePairs + ln];
  if (pr < 0 || pr >= P) return;
  *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.z * P + pr) * H + h0 + 4 * g) = acc[0];
}

int moe_splits(int H, int I) {
  const int blocks = H / kBN, kblocks = I / 128;
  int ks = 1;
  while (ks < kMaxSplits && blocks * ks < kTargetBlocks && ks * 2 * kMinSplitBlocks <= kblocks) ks *= 2;
  return ks;
}

bool moe_dims_ok(int H, int I) {
  return H > 0 && I > 0 && H % 128 == 0 && I % 128 == 0 && I / kBN <= 65535 && H / kBN <= 65535;
}

bool moe_shape_ok(int T, int H, int I, int E, int k) { return moe_dims_ok(H, I) && moe_topk_ok(E, k) && moe_rows_ok(T, H, k); }

}  // namespace

// K ranges rca_moe_ffn's down projection uses (a function of H and I only); 0: outside the contract
RCA_API int rca_moe_down_splits(int H, int I) { return moe_dims_ok(H, I) ? moe_splits(H, I) : 0; }

// bytes of rca_moe_ffn's workspace; 0: outside the contract
RCA_API long long rca_moe_ffn_workspace(int T, int H, int I, int E, int k) {
  return moe_shape_ok(T, H, I, E, k) ? moe_ws(T, H, I, E, k, moe_splits(H, I)).total : 0;
}

// ids[t][0..k) (int32) = the k largest of x[t] . w_router[e] (fp32 sums) in descending order, equal logits
// by ascending e; weights[t][0..k) (fp32) = their softmax. x [T][H] bf16 with row stride ldx, w_router
// [E][H] bf16 contiguous.
// -1: shape outside the contract (H % 128, 2 <= E <= 64, 1 <= k <= min(E, 8), T >= 1); -2: alignment /
// stride; -4: launch.
RCA_API int rca_moe_route(const void* x, long long ldx, const void* w_router, void* ids, void* weights, int T, int H,
                          int E, int k, hipStream_t st) {
  if (T < 1 || H <= 0 || H % 128 || !moe_topk_ok(E, k)) return -1;
  if (ldx & 7 || ldx < H || ((uintptr_t)x | (uintptr_t)w_router) & 15) return -2;
  if (!ids || !weights || ((uintptr_t)ids | (uintptr_t)weights) & 3) return -2;
  moe_route_kernel<<<(T + 3) / 4, 256, 0, st>>>((const bf16_t*)x, ldx, (const bf16_t*)w_router, (int*)ids, (float*)weights,
                                               T, H, E, k);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

// y[t][:] (bf16, row stride ldy) = sum_j weights[t][j] * W_d[e] . bf16(silu(W_g[e] . x[t]) * (W_u[e] . x[t])),
// e = ids[t][j]; a pair whose id is outside [0, E) adds nothing. x [T][H] bf16 with row stride ldx,
// w_gate_up [E][2I][H] and w_down [E][H][I] bf16 contiguous, ids [T][k] int32, weights [T][k] fp32.
// ws: rca_moe_ffn_workspace(T, H, I, E, k) bytes. Four launches: align, gate_up, down, combine.
// -1: shape outside the contract (H % 128, I % 128, T >= 1, 2 <= E <= 64, 1 <= k <= min(E, 8)); -2: alignment /
// stride; -3: workspace; -4: launch. Nothing is launched on a refusal.
RCA_API int rca_moe_ffn(const void* x, long long ldx, void* y, long long ldy, const void* ids, const void* weights,
                        const void* w_gate_up, const void* w_down, void* ws, long long ws_bytes, int T, int H, int I,
                        int E, int k, hipStream_t st) {
  if (!moe_shape_ok(T, H, I, E, k)) return -1;
  if ((ldx | ldy) & 7 || ldx < H || ldy < H) return -2;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w_gate_up | (uintptr_t)w_down) & 15) return -2;
  if (!ids || !weights || ((uintptr_t)ids | (uintptr_t)weights) & 3) return -2;
  const int P = T * k, nt = moe_tiles_max(P, E), splits = moe_splits(H, I);
  const MoeWs w = moe_ws(T, H, I, E, k, splits);
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < w.total) return -3;
  const int kblocks = I / 128, per = (kblocks + splits - 1) / splits;
  char* base = (char*)ws;
  int* te = (int*)(base + w.expert);
  int* tp = (int*)(base + w.pairs);
  bf16_t* act = (bf16_t*)(base + w.act);
  float* part = (float*)(base + w.part);
  moe_align_kernel<<<1, kAlignThreads, 0, st>>>((const int*)ids, te, tp, P, E, nt);
  moe_gate_up_kernel<<<dim3(nt, I / kBN), 256, 0, st>>>((const bf16_t*)x, ldx, (const bf16_t*)w_gate_up, te, tp, act, P, k,
                                                       H, I, E);
  moe_down_kernel<<<dim3(nt, H / kBN, splits), 256, 0, st>>>(act, (const bf16_t*)w_down, te, tp, part, P, H, I, E, per);
  const long long quads = (long long)T * (H / 4);
  moe_combine_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, st>>>(part, (const int*)ids, (const float*)weights,
                                                                    (bf16_t*)y, ldy, T, k, H, E, splits);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}
