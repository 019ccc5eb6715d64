// The grouped expert SwiGLU FFN of moe.hip over MXFP4 expert weights (W4A16):
// y[t] = sum_j weights[t][j] * deq(W_d)[e] . bf16(silu(deq(W_g)[e] . x[t]) * (deq(W_u)[e] . x[t])), e = ids[t][j].
//
// Operands (ops/reference.py, moe_ffn_w4_ref): x, y, ids and weights as in moe.hip. Each expert matrix is
// quantised row by row as a linear's weight is (linear_w4.hip): q_gate_up [E][2I][H/2] and q_down [E][H][I/2]
// hold two e2m1 nibbles a byte, the low nibble the even k; s_gate_up [E][2I][H/32] and s_down [E][H][I/32] one
// E8M0 byte per 32 consecutive k of a row, any value in [2, 252]. A nibble times its block scale is a normal
// bf16 number or zero, so the kernels multiply by exactly known weights.
//
// Grouping, the workspace, the tiles of up to 16 pairs of one expert and the combine are moe.hip's
// (moe_common.h): moe_align_kernel, then the two tile GEMMs below, then moe_combine_kernel. Nothing is read on
// the host.
//
// The tile GEMM (moe_w4_tile_gemm). A block is 4 waves; wave w owns 16 weight rows, the MFMA's row operand,
// and the tile's 16 pairs are the column operand. The weights stream from global as in linear_w4.hip: per
// 256-deep chunk (one 128-byte line of a weight row and 8 scale bytes) lane (n = lane & 15, g = lane >> 4)
// issues two 16-byte loads, bytes 16 (4 h + g) .. + 15 of the line for h = 0, 1, and one 8-byte load of the
// chunk's scale bytes, of which it uses bytes g and 4 + g. A 16-byte load is the 32 k of MX block 4 h + g: one
// scale. Each of its four dwords goes through v_cvt_scalef32_pk_bf16_fp4 with the block scale (the float whose
// bits are e << 23) as the scale operand and is one bf16x8 row fragment of v_mfma_f32_16x16x32_bf16; the
// column fragment of that MFMA is src[pair][k0 + 32 (4 h + g) + 8 j ..], the same k's. Nothing is scaled after
// the MFMA. An LDS stage is 512 k (two chunks) of the tile's source rows, gathered by pair, in two buffers:
// the next stage's q, e and source rows are in flight while the 16 NS MFMAs and 64 NS conversions of the
// current one run. A lane holds 64 NS bytes of weight in flight, half of the bf16 kernel's.
//   moe_w4_gate_up_kernel  grid (tile, I / 64): wave w owns 16 gate rows and the matching 16 up rows, two
//                          accumulators; act[p] = bf16(silu(g) * u), one rounding, pair-major [T k][I].
//   moe_w4_down_kernel     grid (tile, H / 64, splits): K ranges of whole 256-deep chunks, fp32 partials
//                          part [splits][T k][H].
//
// splits depends on (H, I) ONLY (linear_w4.hip's rule), every range is summed in ascending chunks, the
// partials are added in range order and nothing is atomic: an output row is a bitwise function of its own x
// row, its ids and weights and the expert bytes, in any batch and any tile position. Padding rows of a tile
// are zeros in LDS and are not stored. An id outside [0, E) is in no tile: it adds nothing and no weight or
// scale is read for it.
#include "common.h"
#include "moe_common.h"  // the tile constants, lds_barrier, moe_align_kernel, moe_combine_kernel, the workspace layout
#include "w4_cvt.h"      // w4_cvt8, e8m0

namespace {

constexpr int kCK = 256;              // k per chunk: 128 weight bytes and 8 scale bytes of a row
constexpr int kKT = 2 * kCK;          // k per LDS stage
constexpr int kRowB = kKT * 2 + 16;   // LDS bytes per source row: +16 so the 16 m-lanes of a read start 4 banks apart
constexpr int kBufB = kTilePairs * kRowB;
constexpr int kMinSplitChunks = 4;    // a K range is at least 4 x 256 deep

// acc[s] += deq(q_s, e_s)[16 rows of this wave][kbeg .. kend) . src[16 pairs of the tile][kbeg .. kend)^T for NS
// row sets. qrow[s]: this lane's row of nibble pairs, + 16 g; erow[s]: its row of scale bytes. kbeg and kend
// are multiples of 256. The source row of pair p is src + (p / div) * ld.
template <int NS>
__device__ __forceinline__ void moe_w4_tile_gemm(const bf16_t* __restrict__ src, long long ld, int div, int P,
                                                 const int* __restrict__ pairs, const unsigned char* const (&qrow)[NS],
                                                 const unsigned char* const (&erow)[NS], int kbeg, int kend,
                                                 f32x4 (&acc)[NS], char* lds) {
  constexpr int kPieces = kTilePairs * (kKT / 8) / 256;  // 16-byte pieces of a source stage per thread
  const int tid = threadIdx.x, lane = tid & 63;
  const int ln = lane & 15, g = lane >> 4;

  // the source rows this thread stages: a padding (or out of range) pair is zeros
  const bf16_t* xsrc[kPieces];
#pragma unroll
  for (int i = 0; i < kPieces; ++i) {
    const int p = tid + 256 * i, pr = pairs[p >> 6];
    xsrc[i] = (pr >= 0 && pr < P) ? src + (size_t)(pr / div) * ld + (p & 63) * 8 : nullptr;
  }
  u32x4 xr[kPieces], wn[NS][2][2];
  uint2 en[NS][2];
  auto load_x = [&](int k) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int col = ((tid + 256 * i) & 63) * 8;
      xr[i] = u32x4{0u, 0u, 0u, 0u};
      if (xsrc[i] != nullptr && k + col < kend) xr[i] = *reinterpret_cast<const u32x4*>(xsrc[i] + k);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int p = tid + 256 * i;
      *reinterpret_cast<u32x4*>(lds + buf * kBufB + (p >> 6) * kRowB + (p & 63) * 16) = xr[i];
    }
  };
  auto load_w = [&](int k) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bool in = k + c * kCK < kend;
        en[s][c] = make_uint2(0u, 0u);
        if (in) en[s][c] = *reinterpret_cast<const uint2*>(erow[s] + (k + c * kCK) / 32);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          wn[s][c][h] = u32x4{0u, 0u, 0u, 0u};
          if (in) wn[s][c][h] = *reinterpret_cast<const u32x4*>(qrow[s] + (k + c * kCK) / 2 + h * 64);
        }
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
    u32x4 wc[NS][2][2];
    float sc[NS][2][2];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        sc[s][c][0] = e8m0((en[s][c].x >> (8 * g)) & 0xffu);
        sc[s][c][1] = e8m0((en[s][c].y >> (8 * g)) & 0xffu);
#pragma unroll
        for (int h = 0; h < 2; ++h) wc[s][c][h] = wn[s][c][h];
      }
    const bool more = k + kKT < kend;
    if (more) {
      load_x(k + kKT);
      load_w(k + kKT);
    }
    const char* xb = lds + buf * kBufB + ln * kRowB + g * 64;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (k + c * kCK < kend) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bf16x8_t xf = *reinterpret_cast<const bf16x8_t*>(xb + c * 512 + h * 256 + j * 16);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
              const bf16x8_t wf = __builtin_bit_cast(bf16x8_t, w4_cvt8(wc[s][c][h][j], sc[s][c][h]));
              acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[s], 0, 0, 0);
            }
          }
        }
      }
    }
    if (more) store_x(buf ^ 1);
    lds_barrier();
  }
}

__global__ __launch_bounds__(256) void moe_w4_gate_up_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                             const unsigned char* __restrict__ Qgu,
                                                             const unsigned char* __restrict__ Sgu,
                                                             const int* __restrict__ tile_expert,
                                                             const int* __restrict__ tile_pairs,
                                                             bf16_t* __restrict__ act, int P, int k, int H, int I, int E) {
  __shared__ __attribute__((aligned(16))) char lds[2 * kBufB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ln = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int e = tile_expert[tile];
  if (e < 0 || e >= E) return;  // the whole block: never index the weights with a bad expert
  const int i0 = blockIdx.y * kBN + wave * 16;  // I % 64 == 0: every wave has a whole tile
  const size_t row = (size_t)e * 2 * I + i0 + ln;  // the gate row; the up row is I further
  const unsigned char* const qrow[2] = {Qgu + row * (H / 2) + g * 16, Qgu + (row + I) * (H / 2) + g * 16};
  const unsigned char* const erow[2] = {Sgu + row * (H / 32), Sgu + (row + I) * (H / 32)};
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  moe_w4_tile_gemm<2>(x, ldx, k, P, tile_pairs + (size_t)tile * kTilePairs, qrow, erow, 0, H, acc, lds);

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

__global__ __launch_bounds__(256) void moe_w4_down_kernel(const bf16_t* __restrict__ act,
                                                          const unsigned char* __restrict__ Qd,
                                                          const unsigned char* __restrict__ Sd,
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
  const int chunks = I / kCK;
  const int c0 = min((int)blockIdx.z * per, chunks), c1 = min(c0 + per, chunks);
  const size_t row = (size_t)e * H + h0 + ln;
  const unsigned char* const qrow[1] = {Qd + row * (I / 2) + g * 16};
  const unsigned char* const erow[1] = {Sd + row * (I / 32)};
  f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
  moe_w4_tile_gemm<1>(act, I, 1, P, tile_pairs + (size_t)tile * kTilePairs, qrow, erow, c0 * kCK, c1 * kCK, acc, lds);

  // lane holds D[h = h0 + 4 g + r][pair = ln]; an empty range stores zeros
  const int pr = tile_pairs[(size_t)tile * kTilePairs + ln];
  if (pr < 0 || pr >= P) return;
  *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.z * P + pr) * H + h0 + 4 * g) = acc[0];
}

int moe_w4_splits(int H, int I) {
  const int blocks = H / kBN, chunks = I / kCK;
  int ks = 1;
  while (ks < kMaxSplits && blocks * ks < kTargetBlocks && ks * 2 * kMinSplitChunks <= chunks) ks *= 2;
  return ks;
}

bool moe_w4_dims_ok(int H, int I) {
  return H > 0 && I > 0 && H % kCK == 0 && I % kCK == 0 && I / kBN <= 65535 && H / kBN <= 65535;
}

bool moe_w4_shape_ok(int T, int H, int I, int E, int k) {
  return moe_w4_dims_ok(H, I) && moe_topk_ok(E, k) && moe_rows_ok(T, H, k);
}

}  // namespace

// K ranges rca_moe_ffn_w4's down projection uses (a function of H and I only); 0: outside the contract
RCA_API int rca_moe_w4_down_splits(int H, int I) { return moe_w4_dims_ok(H, I) ? moe_w4_splits(H, I) : 0; }

// bytes of rca_moe_ffn_w4's workspace; 0: outside the contract
RCA_API long long rca_moe_ffn_w4_workspace(int T, int H, int I, int E, int k) {
  return moe_w4_shape_ok(T, H, I, E, k) ? moe_ws(T, H, I, E, k, moe_w4_splits(H, I)).total : 0;
}

// y[t][:] (bf16, row stride ldy) = sum_j weights[t][j] * deq(q_down, s_down)[e] . bf16(silu(W_g[e] . x[t]) *
// (W_u[e] . x[t])), W_g | W_u = deq(q_gate_up, s_gate_up)[e], e = ids[t][j]; a pair whose id is outside [0, E)
// adds nothing. x [T][H] bf16 with row stride ldx; q_gate_up [E][2I][H/2], s_gate_up [E][2I][H/32], q_down
// [E][H][I/2] and s_down [E][H][I/32] uint8, contiguous; ids [T][k] int32, weights [T][k] fp32.
// ws: rca_moe_ffn_w4_workspace(T, H, I, E, k) bytes. Four launches: align, gate_up, down, combine.
// -1: shape outside the contract (H % 256, I % 256, T >= 1, 2 <= E <= 64, 1 <= k <= min(E, 8)); -2: alignment /
// stride (16-byte bases, 8-byte scale bases); -3: workspace; -4: launch. Nothing is launched on a refusal.
RCA_API int rca_moe_ffn_w4(const void* x, long long ldx, void* y, long long ldy, const void* ids, const void* weights,
                           const void* q_gate_up, const void* s_gate_up, const void* q_down, const void* s_down, void* ws,
                           long long ws_bytes, int T, int H, int I, int E, int k, hipStream_t st) {
  if (!moe_w4_shape_ok(T, H, I, E, k)) return -1;
  if ((ldx | ldy) & 7 || ldx < H || ldy < H) return -2;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)q_gate_up | (uintptr_t)q_down) & 15) return -2;
  if (!s_gate_up || !s_down || ((uintptr_t)s_gate_up | (uintptr_t)s_down) & 7) return -2;
  if (!ids || !weights || ((uintptr_t)ids | (uintptr_t)weights) & 3) return -2;
  const int P = T * k, nt = moe_tiles_max(P, E), splits = moe_w4_splits(H, I);
  const MoeWs w = moe_ws(T, H, I, E, k, splits);
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < w.total) return -3;
  const int chunks = I / kCK, per = (chunks + splits - 1) / splits;
  char* base = (char*)ws;
  int* te = (int*)(base + w.expert);
  int* tp = (int*)(base + w.pairs);
  bf16_t* act = (bf16_t*)(base + w.act);
  float* part = (float*)(base + w.part);
  moe_align_kernel<<<1, kAlignThreads, 0, st>>>((const int*)ids, te, tp, P, E, nt);
  moe_w4_gate_up_kernel<<<dim3(nt, I / kBN), 256, 0, st>>>((const bf16_t*)x, ldx, (const unsigned char*)q_gate_up,
                                                          (const unsigned char*)s_gate_up, te, tp, act, P, k, H, I, E);
  moe_w4_down_kernel<<<dim3(nt, H / kBN, splits), 256, 0, st>>>(act, (const unsigned char*)q_down,
                                                               (const unsigned char*)s_down, te, tp, part, P, H, I, E, per);
  const long long quads = (long long)T * (H / 4);
  moe_combine_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, st>>>(part, (const int*)ids, (const float*)weights,
                                                                    (bf16_t*)y, ldy, T, k, H, E, splits);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}
