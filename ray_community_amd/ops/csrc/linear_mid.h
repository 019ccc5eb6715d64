// Quantised-weight linears between the skinny tile and prefill (33 .. a few hundred rows): the main loop
// shared by the MXFP4 (linear_w4.hip) and fp8 (linear_w8.hip) mid-M kernels, templated on the producer P
// of the weight fragment. Anonymous namespace: each translation unit gets its own copy.
//
// Why a second kernel. The skinny kernels give a block 32 rows of x and send further rows to blockIdx.y,
// so at M rows the weight is streamed and converted ceil(M / 32) times, and every MFMA reads its own
// 16-byte x fragment from LDS. Here the weight is streamed and converted ONCE per block for up to 128
// rows, and an x fragment feeds two MFMAs.
//
// Work split. A block is 4 waves and covers 128 output columns and MT 16-row tiles of x (MT = 4 for
// M <= 64, else 8; blockIdx.y takes further 64- / 128-row slabs, blockIdx.z the K ranges). Wave w owns
// the NT = 2 column tiles nb + 32 w + 16 i; N % 16 == 0 only, so a tile may sit at or past N: nothing is
// loaded for it (its fragments are zeros) and nothing stored. Per 32 k of a stage a wave converts NT
// weight fragments (each feeds MT MFMAs) and reads MT x fragments from LDS (each feeds NT MFMAs).
//   accumulators: NT * MT * 4 = 32 (MT = 4) or 64 (MT = 8) fp32 registers a lane;
//   LDS: 1 KB a wave per x fragment over NT MFMAs = 512 bytes per MFMA (the skinny kernels: 1 KB).
//
// x goes through LDS exactly as in the skinny kernels: a stage is 256 k, the row pitch 512 + 16 bytes
// (the 16 m-lanes of a fragment read start 4 banks apart), two buffers, the stage after the current one
// on its way (global -> registers while the MFMAs run -> LDS before the barrier). 128 rows x 528 bytes x 2
// buffers = 135 168 bytes of the 160 KB (one block a CU); MT = 4 takes half (two blocks a CU). The weight
// bytes of the next stage are in registers meanwhile (64 bytes a lane and column tile, as the skinny
// kernels have).
//
// Arithmetic: the skinny kernels' to the bit. W is the row operand and x the column operand of
// v_mfma_f32_16x16x32_bf16; a chunk (P::kCK k: one 128-byte line of a weight row) is P::kCK / 32 MFMAs,
// MFMA s of chunk c over the k-set {k0 + 32 (4 (s >> 2) + g) + 8 (s & 3) ..+7 : g = 0..3}, in ascending
// (c, s) per accumulator; K ranges are whole chunks, `per` of them per blockIdx.z, by the skinny kernel's
// split rule; fp32 partials go to the same workspace layout for the same combine kernel. A column of the
// MFMA result depends on its own column operand only, rows of x past M are zeros in LDS and are not
// stored: an output row is a function of its own x row and W, whichever of the two kernels ran.
//
// P provides: kCK; kRowScale (the fp32 accumulator is multiplied by s[n] before the one rounding);
// Row (a lane's pointers into its weight row) and row(n, K, g); Raw (a lane's bytes of one chunk) and
// load(Raw&, Row, k, in) (zeros when !in: no load is issued); frag(Raw, s, g) (MFMA s's row operand);
// out_scale(n) (s[n .. n + 3], kRowScale only).
#pragma once
#include "common.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int kMidNT = 2;                   // 16-column tiles per wave
constexpr int kMidBN = 4 * kMidNT * 16;     // output columns per block
constexpr int kMidKT = 256;                 // k per LDS stage
constexpr int kMidRowB = kMidKT * 2 + 16;   // LDS bytes per x row (the skinny kernels' pitch)

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <class P, int MT, bool SPLIT>
__global__ __launch_bounds__(256) void linear_mid_kernel(const bf16_t* __restrict__ x, long long ldx, const P p,
                                                         bf16_t* __restrict__ y, long long ldy,
                                                         float* __restrict__ part, int M, int N, int K, int per) {
  constexpr int kRows = MT * 16;               // x rows per block
  constexpr int kPieces = kRows * (kMidKT / 8) / 256;  // 16-byte pieces of an x stage per thread
  constexpr int kBufB = kRows * kMidRowB;
  constexpr int kCPS = kMidKT / P::kCK;        // chunks per stage
  constexpr int kMF = P::kCK / 32;             // MFMAs per chunk and accumulator
  extern __shared__ __attribute__((aligned(16))) char lds[];  // 2 * kBufB

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, g = lane >> 4;
  const int nb = blockIdx.x * kMidBN + wave * (16 * kMidNT);
  const int m0 = blockIdx.y * kRows;
  const int chunks = K / P::kCK;
  const int c0 = min((int)blockIdx.z * per, chunks), c1 = min(c0 + per, chunks);
  const int kbeg = c0 * P::kCK, kend = c1 * P::kCK;

  bool act[kMidNT];  // N % 16 == 0: a tile is whole or absent (the wave still stages x)
  typename P::Row wrow[kMidNT];
#pragma unroll
  for (int i = 0; i < kMidNT; ++i) {
    act[i] = nb + 16 * i < N;
    wrow[i] = p.row(act[i] ? nb + 16 * i + ln : 0, K, g);
  }

  f32x4 acc[kMidNT][MT];
#pragma unroll
  for (int i = 0; i < kMidNT; ++i)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 xr[kPieces];
  typename P::Raw wn[kMidNT][kCPS];

  auto load_x = [&](int k) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int q = tid + 256 * i, row = q >> 5, col = (q & 31) * 8;
      xr[i] = u32x4{0u, 0u, 0u, 0u};
      if (m0 + row < M && k + col < kend)
        xr[i] = *reinterpret_cast<const u32x4*>(x + (size_t)(m0 + row) * ldx + k + col);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int q = tid + 256 * i, row = q >> 5, col = q & 31;
      *reinterpret_cast<u32x4*>(lds + buf * kBufB + row * kMidRowB + col * 16) = xr[i];
    }
  };
  auto load_w = [&](int k) {
#pragma unroll
    for (int i = 0; i < kMidNT; ++i)
#pragma unroll
      for (int c = 0; c < kCPS; ++c) P::load(wn[i][c], wrow[i], k + c * P::kCK, act[i] && k + c * P::kCK < kend);
  };

  if (kbeg < kend) {
    load_x(kbeg);
    load_w(kbeg);
    store_x(0);
    lds_barrier();
  }
  int buf = 0;
  for (int k = kbeg; k < kend; k += kMidKT, buf ^= 1) {
    typename P::Raw wc[kMidNT][kCPS];
#pragma unroll
    for (int i = 0; i < kMidNT; ++i)
#pragma unroll
      for (int c = 0; c < kCPS; ++c) wc[i][c] = wn[i][c];
    const bool more = k + kMidKT < kend;
    if (more) {
      load_x(k + kMidKT);
      load_w(k + kMidKT);
    }
    if (act[0]) {
      const char* xb = lds + buf * kBufB + ln * kMidRowB + g * 64;
#pragma unroll
      for (int c = 0; c < kCPS; ++c) {
        if (k + c * P::kCK < kend) {
#pragma unroll
          for (int s = 0; s < kMF; ++s) {
            bf16x8_t wf[kMidNT];
#pragma unroll
            for (int i = 0; i < kMidNT; ++i) wf[i] = P::frag(wc[i][c], s, g);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
              const bf16x8_t xf = *reinterpret_cast<const bf16x8_t*>(xb + t * 16 * kMidRowB + c * P::kCK * 2 +
                                                                     (s >> 2) * 256 + (s & 3) * 16);
#pragma unroll
              for (int i = 0; i < kMidNT; ++i)
                acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf, acc[i][t], 0, 0, 0);
            }
          }
        }
      }
    }
    if (more) store_x(buf ^ 1);
    lds_barrier();
  }

  // lane holds D[n = nb + 16 i + 4 g + r][m = m0 + 16 t + ln], r = 0..3
#pragma unroll
  for (int i = 0; i < kMidNT; ++i) {
    if (!act[i]) continue;
    const int n = nb + 16 * i + 4 * g;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = m0 + 16 * t + ln;
      if (m >= M) continue;
      if constexpr (SPLIT) {
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.z * M + m) * N + n) = acc[i][t];
      } else {
        f32x4 v = acc[i][t];
        if constexpr (P::kRowScale) {
          const f32x4 sc = p.out_scale(n);
          v[0] = v[0] * sc[0], v[1] = v[1] * sc[1], v[2] = v[2] * sc[2], v[3] = v[3] * sc[3];
        }
        uint2 o;
        o.x = (unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16);
        o.y = (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16);
        *reinterpret_cast<uint2*>(y + (size_t)m * ldy + n) = o;
      }
    }
  }
}

template <class P, int MT, bool SPLIT>
bool linear_mid_launch_one(dim3 grid, const bf16_t* x, long long ldx, const P& p, bf16_t* y, long long ldy, float* part,
                           int M, int N, int K, int per, hipStream_t st) {
  constexpr int kLdsB = 2 * MT * 16 * kMidRowB;  // above the 64 KB a kernel gets unasked
  static const bool attr = hipFuncSetAttribute((const void*)linear_mid_kernel<P, MT, SPLIT>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, kLdsB) == hipSuccess;
  if (!attr) return false;
  linear_mid_kernel<P, MT, SPLIT><<<grid, 256, kLdsB, st>>>(x, ldx, p, y, ldy, part, M, N, K, per);
  return true;
}

// rows per block of the launch below: 64 up to 64 rows of x, else 128
inline int linear_mid_rows(int M) { return M <= 64 ? 64 : 128; }

// The main kernel over (column blocks, row slabs, K ranges); with splits > 1 the caller's combine kernel
// follows. false: the LDS size could not be set.
template <class P>
bool linear_mid_launch(const bf16_t* x, long long ldx, const P& p, bf16_t* y, long long ldy, float* part, int M, int N,
                       int K, int splits, int per, hipStream_t st) {
  const int rows = linear_mid_rows(M);
  const dim3 grid((N + kMidBN - 1) / kMidBN, (M + rows - 1) / rows, splits);
  if (rows == 64)
    return splits > 1 ? linear_mid_launch_one<P, 4, true>(grid, x, ldx, p, y, ldy, part, M, N, K, per, st)
                      : linear_mid_launch_one<P, 4, false>(grid, x, ldx, p, y, ldy, part, M, N, K, per, st);
  return splits > 1 ? linear_mid_launch_one<P, 8, true>(grid, x, ldx, p, y, ldy, part, M, N, K, per, st)
                    : linear_mid_launch_one<P, 8, false>(grid, x, ldx, p, y, ldy, part, M, N, K, per, st);
}

}  // namespace
