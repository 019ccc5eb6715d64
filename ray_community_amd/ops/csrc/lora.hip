// Multi-LoRA for inference linears: y[m] += scale[a] * B[a] . bf16(A[a] . x[m]) with a = the adapter slot
// of row m, for a batch whose rows name different adapters (or none).
//
// Operands (ops/reference.py, lora_add_ref): x [M][K] and y [M][N] bf16 with row strides; the bank
// A [S][R][K], B [S][N][R] bf16 and scale [S] fp32 (alpha / rank, applied to the fp32 accumulator, so it
// costs no rounding). R is the bank's slot capacity; an adapter of lower rank leaves the rest zero.
//
// Routing. The host groups the rows that name a slot into tiles of up to 16 rows of one slot, in any row
// order: tile_slot [n_tiles] and tile_rows [n_tiles][16], -1 as padding. Rows without an adapter are in no
// tile and are never read or written.
//
// Two launches. lora_shrink_kernel: one workgroup per (tile, K range), wave w owns the 16-row tiles
// w, w + NW, ... of A[slot] (the MFMA row operand, streamed from global as in linear_w8.hip: per 128-deep
// chunk lane (n = lane & 15, g = lane >> 4) loads the 64 bytes A[n][k0 + 32 g ..] and feeds 4
// v_mfma_f32_16x16x32_bf16); the tile's x rows are gathered into LDS in 256-deep K tiles, two buffers, and
// are the column operand. It writes fp32 partials [splits][n_tiles * 16][R]. lora_expand_add_kernel: one
// workgroup per (tile, 64 output columns); it adds its tile's partials in ascending range order, rounds
// them to bf16 into LDS (t never exists in HBM as bf16), runs the MFMAs over R with B[slot] as the row
// operand and stores bf16(float(y) + scale[slot] * acc) to the tile's real rows.
//
// splits depends on (K, R) ONLY, every range is summed in ascending chunks, the partials are added in range
// order and nothing is atomic: an output row is a function of its own x row and its slot's A, B and scale,
// whatever M is and in whichever tile and position the row sits (an MFMA column depends on its own column
// operand only), and results are bitwise reproducible. Padding rows of a tile are zeros in LDS and are
// not stored.
#include "common.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int kTileRows = 16;         // x rows per tile: the MFMA's columns
constexpr int kBN = 64;               // output columns per expand block: 4 waves x one 16-wide MFMA tile
constexpr int kKT = 256;              // k per LDS stage
constexpr int kRowB = kKT * 2 + 16;   // LDS bytes per x row: +16 so the 16 m-lanes of a read start 4 banks apart
constexpr int kMaxR = 256;
constexpr int kMinSplitBlocks = 4;    // a K range is at least 4 x 128 deep

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// NW waves: R / 16 row tiles of A[slot] dealt round-robin, at most 4 a wave
template <int NW>
__global__ __launch_bounds__(64 * NW) void lora_shrink_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                              const bf16_t* __restrict__ A,
                                                              const int* __restrict__ tile_slot,
                                                              const int* __restrict__ tile_rows,
                                                              float* __restrict__ part, int n_tiles, int M, int K, int R,
                                                              int S, int per) {
  constexpr int kThreads = 64 * NW;
  constexpr int kPieces = kTileRows * (kKT / 8) / kThreads;  // 16-byte pieces of an x tile per thread
  constexpr int kBufB = kTileRows * kRowB;
  __shared__ __attribute__((aligned(16))) char lds[2 * kBufB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int slot = tile_slot[tile];
  if (slot < 0 || slot >= S) return;  // the whole block: never index the bank with a bad slot
  const int kblocks = K / 128, rtiles = R / 16;
  const int kb0 = min((int)blockIdx.y * per, kblocks), kb1 = min(kb0 + per, kblocks);
  const int kbeg = kb0 * 128, kend = kb1 * 128;

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the x rows this thread stages: a padding (or out of range) row is zeros
  const bf16_t* xsrc[kPieces];
#pragma unroll
  for (int i = 0; i < kPieces; ++i) {
    const int p = tid + kThreads * i, row = tile_rows[tile * kTileRows + (p >> 5)];
    xsrc[i] = (row >= 0 && row < M) ? x + (size_t)row * ldx + (p & 31) * 8 : nullptr;
  }
  u32x4 xr[kPieces];
  auto load_x = [&](int k) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int col = ((tid + kThreads * i) & 31) * 8;
      xr[i] = u32x4{0u, 0u, 0u, 0u};
      if (xsrc[i] != nullptr && k + col < kend) xr[i] = *reinterpret_cast<const u32x4*>(xsrc[i] + k);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int p = tid + kThreads * i;
      *reinterpret_cast<u32x4*>(lds + buf * kBufB + (p >> 5) * kRowB + (p & 31) * 16) = xr[i];
    }
  };

  const bf16_t* arow = A + ((size_t)slot * R + ln) * K + g * 32;

  if (kbeg < kend) {
    load_x(kbeg);
    store_x(0);
    lds_barrier();
  }
  int buf = 0;
  for (int k = kbeg; k < kend; k += kKT, buf ^= 1) {
    const bool more = k + kKT < kend;
    if (more) load_x(k + kKT);
    const char* xb = lds + buf * kBufB + ln * kRowB + g * 64;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (k + c * 128 < kend) {
        bf16x8_t xf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xf[j] = *reinterpret_cast<const bf16x8_t*>(xb + c * 256 + j * 16);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int rt = wave + NW * t;
          if (rt < rtiles) {
            const bf16_t* ap = arow + (size_t)rt * 16 * K + k + c * 128;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(ap + 8 * j);
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, xf[j], acc[t], 0, 0, 0);
            }
          }
        }
      }
    }
    if (more) store_x(buf ^ 1);
    lds_barrier();
  }

  // lane holds D[r = 16 rt + 4 g + i][m = ln], i = 0..3; padding rows are stored too (zeros)
  float* prow = part + (((size_t)blockIdx.y * n_tiles + tile) * kTileRows + ln) * R + 4 * g;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int rt = wave + NW * t;
    if (rt < rtiles) *reinterpret_cast<f32x4*>(prow + rt * 16) = acc[t];
  }
}

__global__ __launch_bounds__(256) void lora_expand_add_kernel(const float* __restrict__ part, const bf16_t* __restrict__ B,
                                                              const float* __restrict__ scale,
                                                              const int* __restrict__ tile_slot,
                                                              const int* __restrict__ tile_rows, bf16_t* __restrict__ y,
                                                              long long ldy, int n_tiles, int M, int N, int R, int S,
                                                              int splits) {
  __shared__ __attribute__((aligned(16))) char lds[kTileRows * (kMaxR * 2 + 16)];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int slot = tile_slot[tile];
  if (slot < 0 || slot >= S) return;
  const int rowb = R * 2 + 16, quads = R / 4;

  // t[m][r..r+3] = bf16(part[0] + part[1] + ... in range order)
  const size_t zstride = (size_t)n_tiles * kTileRows * R;
  for (int q = tid; q < kTileRows * quads; q += 256) {
    const int m = q / quads, r = (q % quads) * 4;
    const float* p = part + ((size_t)tile * kTileRows + m) * R + r;
    f32x4 a = *reinterpret_cast<const f32x4*>(p);
    for (int z = 1; z < splits; ++z) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(p + z * zstride);
      a[0] += b[0], a[1] += b[1], a[2] += b[2], a[3] += b[3];
    }
    uint2 o;
    o.x = (unsigned)f2bf(a[0]) | ((unsigned)f2bf(a[1]) << 16);
    o.y = (unsigned)f2bf(a[2]) | ((unsigned)f2bf(a[3]) << 16);
    *reinterpret_cast<uint2*>(lds + m * rowb + r * 2) = o;
  }
  lds_barrier();

  const int n0 = blockIdx.y * kBN + wave * 16;
  if (n0 >= N) return;  // N % 16 == 0: a wave has a whole tile or none
  const bf16_t* brow = B + ((size_t)slot * N + n0 + ln) * R + 8 * g;
  const char* tb = lds + ln * rowb + g * 16;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < R; r0 += 32) {
    u32x4 bv = u32x4{0u, 0u, 0u, 0u}, tv = u32x4{0u, 0u, 0u, 0u};
    if (r0 + 8 * g < R) {  // R % 32 == 16: the last MFMA's upper half is zeros
      bv = *reinterpret_cast<const u32x4*>(brow + r0);
      tv = *reinterpret_cast<const u32x4*>(tb + r0 * 2);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bv), __builtin_bit_cast(bf16x8_t, tv), acc,
                                                  0, 0, 0);
  }

  // lane holds D[n = n0 + 4 g + i][m = ln]
  const int row = tile_rows[tile * kTileRows + ln];
  if (row < 0 || row >= M) return;
  const float sc = scale[slot];
  uint2* yp = reinterpret_cast<uint2*>(y + (size_t)row * ldy + n0 + 4 * g);
  const uint2 y0 = *yp;
  uint2 o;
  o.x = (unsigned)f2bf(bf2f((bf16_t)(y0.x & 0xffffu)) + sc * acc[0]) |
        ((unsigned)f2bf(bf2f((bf16_t)(y0.x >> 16)) + sc * acc[1]) << 16);
  o.y = (unsigned)f2bf(bf2f((bf16_t)(y0.y & 0xffffu)) + sc * acc[2]) |
        ((unsigned)f2bf(bf2f((bf16_t)(y0.y >> 16)) + sc * acc[3]) << 16);
  *yp = o;
}

int lora_splits(int K, int R) {
  // fewer row tiles of A per workgroup (small R) leave room for more K ranges
  const int kblocks = K / 128, most = R <= 64 ? 16 : 8;
  int ks = 1;
  while (ks < most && ks * 2 * kMinSplitBlocks <= kblocks) ks *= 2;
  return ks;
}

bool lora_shape_ok(int N, int K, int R) {
  return N > 0 && K > 0 && N % 16 == 0 && K % 128 == 0 && R % 16 == 0 && R >= 16 && R <= kMaxR;
}

}  // namespace

// K ranges rca_lora_add uses for a bank of capacity R over K inputs (a function of K and R only); 0:
// outside the contract
RCA_API int rca_lora_splits(int K, int R) { return lora_shape_ok(16, K, R) ? lora_splits(K, R) : 0; }

// y[m][:] (bf16, row stride ldy) += scale[s] * B[s] . bf16(A[s] . x[m][:]) for the rows m listed in the
// tiles, s = tile_slot[tile]. A [S][R][K], B [S][N][R] bf16 contiguous, scale [S] fp32, tile_slot
// [n_tiles] and tile_rows [n_tiles][16] int32 (-1: padding; a row is in at most one tile).
// ws: rca_lora_splits(K, R) * n_tiles * 16 * R floats.
// -1: shape outside the contract (K % 128, N % 16, R % 16, 16 <= R <= 256, M, S >= 1); -2: alignment /
// stride; -3: workspace; -4: launch. Nothing is launched on a refusal, nor with n_tiles == 0 (returns 0).
RCA_API int rca_lora_add(const void* x, long long ldx, void* y, long long ldy, const void* A, const void* B,
                         const void* scale, const void* tile_slot, const void* tile_rows, int n_tiles, void* ws,
                         long long ws_bytes, int M, int N, int K, int R, int S, hipStream_t st) {
  if (!lora_shape_ok(N, K, R) || M < 1 || S < 1 || n_tiles < 0 || (N + kBN - 1) / kBN > 65535) return -1;
  if ((ldx | ldy) & 7 || ldx < K || ldy < N) return -2;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)A | (uintptr_t)B) & 15) return -2;
  if (((uintptr_t)scale | (uintptr_t)tile_slot | (uintptr_t)tile_rows) & 3) return -2;
  if (!scale || !tile_slot || !tile_rows) return -2;
  if (n_tiles == 0) return 0;
  const int splits = lora_splits(K, R), kblocks = K / 128, per = (kblocks + splits - 1) / splits;
  if (!ws || ((uintptr_t)ws & 15) || ws_bytes < (long long)splits * n_tiles * kTileRows * R * 4) return -3;
  const bf16_t* xp = (const bf16_t*)x;
  const bf16_t* ap = (const bf16_t*)A;
  const int* ts = (const int*)tile_slot;
  const int* tr = (const int*)tile_rows;
  float* pp = (float*)ws;
  const dim3 sgrid(n_tiles, splits);
  if (R >= 64)
    lora_shrink_kernel<4><<<sgrid, 256, 0, st>>>(xp, ldx, ap, ts, tr, pp, n_tiles, M, K, R, S, per);
  else if (R >= 32)
    lora_shrink_kernel<2><<<sgrid, 128, 0, st>>>(xp, ldx, ap, ts, tr, pp, n_tiles, M, K, R, S, per);
  else
    lora_shrink_kernel<1><<<sgrid, 64, 0, st>>>(xp, ldx, ap, ts, tr, pp, n_tiles, M, K, R, S, per);
  lora_expand_add_kernel<<<dim3(n_tiles, (N + kBN - 1) / kBN), 256, 0, st>>>(pp, (const bf16_t*)B, (const float*)scale, ts,
                                                                            tr, (bf16_t*)y, ldy, n_tiles, M, N, R, S,
                                                                            splits);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}
