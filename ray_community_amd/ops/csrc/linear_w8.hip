// FP8 weights for inference linears (W8A16): y[M][N] = x[M][K] . (Wq[N][K] * s[N])^T for skinny M, and
// the dequantiser that feeds the large-M path.
//
// Format (ops/reference.py, quantize_weight_fp8_ref): Wq holds OCP e4m3 bytes, k-major ([N][K] as
// nn.Linear.weight), s one fp32 power of two per output row, so byte * scale is exact in bf16 and the
// scale can be applied to the fp32 accumulator without a rounding. x stays bf16.
//
// Arithmetic: e4m3 -> f32 (v_cvt_pk_f32_fp8, exact) -> bf16 (exact: 3 mantissa bits), fp32 accumulation
// on v_mfma_f32_16x16x32_bf16 with W as the row operand and x as the column operand, acc * s[n], one
// bf16 rounding.
//
// Work split. A block is 4 waves; wave w owns the 16 output columns n0 + 16 w .. + 15 over the block's
// K range and up to 32 rows of x (MT = 1 or 2 MFMA column tiles), so Wq is streamed once for M <= 32;
// further rows go to blockIdx.y and stream it again. x is staged through LDS in 256-deep K tiles, two
// buffers, shared by the 4 waves; the tile after the current one is in flight (x in registers on its
// way to LDS, Wq in registers) while the MFMAs of the current one run. Per 128-deep chunk a lane
// (n = lane & 15, g = lane >> 4) loads the 32 bytes Wq[n][k0 + 32 g ..] with two 16-byte loads (a wave
// covers 16 rows x one 128-byte line) and feeds 4 MFMAs with 8 bytes each; the x fragment of MFMA j is
// x[m][k0 + 32 g + 8 j ..], the same k's, so the order of k inside a chunk is the lanes' business only.
//
// Split K. Narrow N (o, down) gives too few blocks, so K is cut into `splits` ranges of whole 128-deep
// blocks, at least 512 deep, over blockIdx.z. splits depends on (N, K) ONLY, every range is summed in
// ascending k, and the fp32 partials are added in ascending range order by a second kernel (no
// atomics): an output row is a function of its own x row and W, whatever M is and wherever the row
// sits in the batch. Rows of a 16-row MFMA tile beyond M are zeros in LDS and are not stored; a column
// of the MFMA result depends on its own column operand only.
#include "kv_fp8.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int kBN = 64;               // output columns per block: 4 waves x one 16-wide MFMA tile
constexpr int kKT = 256;              // k per LDS stage
constexpr int kRowB = kKT * 2 + 16;   // LDS bytes per x row: +16 so the 16 m-lanes of a read start 4 banks apart
constexpr int kMinSplitBlocks = 4;    // a K range is at least 4 x 128 deep
constexpr int kMaxSplits = 8;
constexpr int kTargetBlocks = 512;    // two blocks per CU

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// 8 e4m3 bytes -> the bf16 MFMA fragment (exact)
__device__ __forceinline__ bf16x8_t w8_frag(unsigned lo, unsigned hi) {
  float f[8];
  unpack8_fp8(make_uint2(lo, hi), f);
  return __builtin_bit_cast(bf16x8_t, pack8(f));
}

template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void linear_w8a16_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                           const fp8_t* __restrict__ W, const float* __restrict__ s,
                                                           bf16_t* __restrict__ y, long long ldy,
                                                           float* __restrict__ part, int M, int N, int K, int per) {
  constexpr int kRows = MT * 16;               // x rows per block
  constexpr int kPieces = kRows * (kKT / 8) / 256;  // 16-byte pieces of an x tile per thread
  constexpr int kBufB = kRows * kRowB;
  __shared__ __attribute__((aligned(16))) char lds[2 * kBufB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kBN + wave * 16;
  const int m0 = blockIdx.y * kRows;
  const bool active = n0 < N;  // N % 16 == 0: a wave has a whole tile or none (it still stages x)
  const int kblocks = K / 128;
  const int kb0 = min((int)blockIdx.z * per, kblocks), kb1 = min(kb0 + per, kblocks);
  const int kbeg = kb0 * 128, kend = kb1 * 128;

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 xr[kPieces], wn[2][2];
  const fp8_t* wrow = W + (size_t)(active ? n0 + ln : 0) * K + g * 32;

  auto load_x = [&](int k) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int p = tid + 256 * i, row = p >> 5, col = (p & 31) * 8;
      xr[i] = u32x4{0u, 0u, 0u, 0u};
      if (m0 + row < M && k + col < kend)
        xr[i] = *reinterpret_cast<const u32x4*>(x + (size_t)(m0 + row) * ldx + k + col);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int p = tid + 256 * i, row = p >> 5, col = p & 31;
      *reinterpret_cast<u32x4*>(lds + buf * kBufB + row * kRowB + col * 16) = xr[i];
    }
  };
  auto load_w = [&](int k) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        wn[c][h] = u32x4{0u, 0u, 0u, 0u};
        if (active && k + c * 128 < kend)
          wn[c][h] = *reinterpret_cast<const u32x4*>(wrow + k + c * 128 + h * 16);
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
    u32x4 wc[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h) wc[c][h] = wn[c][h];
    const bool more = k + kKT < kend;
    if (more) {
      load_x(k + kKT);
      load_w(k + kKT);
    }
    if (active) {
      const char* xb = lds + buf * kBufB + ln * kRowB + g * 64;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (k + c * 128 < kend) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u32x4 wv = wc[c][j >> 1];
            const bf16x8_t wf = (j & 1) ? w8_frag(wv[2], wv[3]) : w8_frag(wv[0], wv[1]);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
              const bf16x8_t xf = *reinterpret_cast<const bf16x8_t*>(xb + t * 16 * kRowB + c * 256 + j * 16);
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[t], 0, 0, 0);
            }
          }
        }
      }
    }
    if (more) store_x(buf ^ 1);
    lds_barrier();
  }

  if (!active) return;
  // lane holds D[n = n0 + 4 g + r][m = m0 + 16 t + ln], r = 0..3
  const int n = n0 + 4 * g;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m0 + 16 * t + ln;
    if (m >= M) continue;
    if constexpr (SPLIT) {
      *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.z * M + m) * N + n) = acc[t];
    } else {
      const f32x4 sc = *reinterpret_cast<const f32x4*>(s + n);
      uint2 o;
      o.x = (unsigned)f2bf(acc[t][0] * sc[0]) | ((unsigned)f2bf(acc[t][1] * sc[1]) << 16);
      o.y = (unsigned)f2bf(acc[t][2] * sc[2]) | ((unsigned)f2bf(acc[t][3] * sc[3]) << 16);
      *reinterpret_cast<uint2*>(y + (size_t)m * ldy + n) = o;
    }
  }
}

// y[m][n..n+3] = bf16((part[0] + part[1] + ... in range order) * s[n])
__global__ __launch_bounds__(256) void linear_w8_combine_kernel(const float* __restrict__ part, const float* __restrict__ s,
                                                                bf16_t* __restrict__ y, long long ldy, int M, int N,
                                                                int splits) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, quads = N / 4;
  if (idx >= (long long)M * quads) return;
  const int m = (int)(idx / quads), n = (int)(idx % quads) * 4;
  f32x4 a = *reinterpret_cast<const f32x4*>(part + (size_t)m * N + n);
  for (int z = 1; z < splits; ++z) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(part + ((size_t)z * M + m) * N + n);
    a[0] += b[0], a[1] += b[1], a[2] += b[2], a[3] += b[3];
  }
  const f32x4 sc = *reinterpret_cast<const f32x4*>(s + n);
  uint2 o;
  o.x = (unsigned)f2bf(a[0] * sc[0]) | ((unsigned)f2bf(a[1] * sc[1]) << 16);
  o.y = (unsigned)f2bf(a[2] * sc[2]) | ((unsigned)f2bf(a[3] * sc[3]) << 16);
  *reinterpret_cast<uint2*>(y + (size_t)m * ldy + n) = o;
}

// out[n][k..k+15] = bf16(Wq[n][k..] * s[n]): 16 bytes in, 32 bytes out per thread
__global__ __launch_bounds__(256) void dequant_w8_kernel(const fp8_t* __restrict__ W, const float* __restrict__ s,
                                                         bf16_t* __restrict__ out, long long pieces, int kp) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= pieces) return;
  const float sc = s[idx / kp];
  const u32x4 v = *reinterpret_cast<const u32x4*>(W + idx * 16);
  float f[16];
  unpack8_fp8(make_uint2(v[0], v[1]), f);
  unpack8_fp8(make_uint2(v[2], v[3]), f + 8);
#pragma unroll
  for (int i = 0; i < 16; ++i) f[i] *= sc;
  u32x4* o = reinterpret_cast<u32x4*>(out + idx * 16);
  o[0] = pack8(f);
  o[1] = pack8(f + 8);
}

int w8_splits(int N, int K) {
  const int blocks = (N + kBN - 1) / kBN, kblocks = K / 128;
  int ks = 1;
  while (ks < kMaxSplits && blocks * ks < kTargetBlocks && ks * 2 * kMinSplitBlocks <= kblocks) ks *= 2;
  return ks;
}

bool w8_shape_ok(int N, int K) { return N > 0 && K > 0 && N % 16 == 0 && K % 128 == 0; }

}  // namespace

// K ranges rca_linear_w8a16 uses for an [N][K] weight (a function of N and K only); 0: outside the contract
RCA_API int rca_linear_w8_splits(int N, int K) { return w8_shape_ok(N, K) ? w8_splits(N, K) : 0; }

// y[M][N] (bf16, row stride ldy) = x[M][K] (bf16, row stride ldx) . (wq[N][K] e4m3 * scale[N])^T.
// ws: splits * M * N floats when rca_linear_w8_splits(N, K) > 1 (unused otherwise).
// -1: shape outside the contract (K % 128, N % 16, M >= 1); -2: alignment / stride; -3: workspace.
RCA_API int rca_linear_w8a16(const void* x, const void* wq, const void* scale, void* y, void* ws, long long ws_bytes,
                             int M, int N, int K, long long ldx, long long ldy, hipStream_t st) {
  if (!w8_shape_ok(N, K) || M < 1 || (M + 31) / 32 > 65535) return -1;
  if ((ldx | ldy) & 7 || ldx < K || ldy < N) return -2;
  if (((uintptr_t)x | (uintptr_t)wq | (uintptr_t)scale | (uintptr_t)y) & 15) return -2;
  const int splits = w8_splits(N, K), kblocks = K / 128, per = (kblocks + splits - 1) / splits;
  if (splits > 1 && (!ws || ((uintptr_t)ws & 15) || ws_bytes < (long long)splits * M * N * 4)) return -3;
  const bool one = M <= 16;
  const dim3 grid((N + kBN - 1) / kBN, one ? 1 : (M + 31) / 32, splits);
  const bf16_t* xp = (const bf16_t*)x;
  const fp8_t* wp = (const fp8_t*)wq;
  const float* sp = (const float*)scale;
  bf16_t* yp = (bf16_t*)y;
  float* pp = (float*)ws;
  if (splits > 1) {
    if (one)
      linear_w8a16_kernel<1, true><<<grid, 256, 0, st>>>(xp, ldx, wp, sp, yp, ldy, pp, M, N, K, per);
    else
      linear_w8a16_kernel<2, true><<<grid, 256, 0, st>>>(xp, ldx, wp, sp, yp, ldy, pp, M, N, K, per);
    const long long quads = (long long)M * (N / 4);
    linear_w8_combine_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, st>>>(pp, sp, yp, ldy, M, N, splits);
  } else if (one) {
    linear_w8a16_kernel<1, false><<<grid, 256, 0, st>>>(xp, ldx, wp, sp, yp, ldy, pp, M, N, K, per);
  } else {
    linear_w8a16_kernel<2, false><<<grid, 256, 0, st>>>(xp, ldx, wp, sp, yp, ldy, pp, M, N, K, per);
  }
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

// out[N][K] (bf16, contiguous) = wq[N][K] e4m3 * scale[N]: exact
RCA_API int rca_dequant_w8(const void* wq, const void* scale, void* out, int N, int K, hipStream_t st) {
  if (N <= 0 || K <= 0 || K % 16) return -1;
  if (((uintptr_t)wq | (uintptr_t)out) & 15 || ((uintptr_t)scale & 3)) return -2;
  const long long pieces = (long long)N * (K / 16);
  if ((pieces + 255) / 256 > 0x7fffffffLL) return -1;
  dequant_w8_kernel<<<(unsigned)((pieces + 255) / 256), 256, 0, st>>>((const fp8_t*)wq, (const float*)scale, (bf16_t*)out,
                                                                     pieces, K / 16);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}
