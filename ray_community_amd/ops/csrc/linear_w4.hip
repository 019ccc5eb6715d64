// MXFP4 weights for inference linears (W4A16): y[M][N] = x[M][K] . deq(q, e)[N][K]^T for skinny M, and
// the dequantiser that feeds the large-M path.
//
// Format (ops/reference.py, quantize_weight_mxfp4_ref): q[N][K/2] holds two OCP e2m1 nibbles a byte, the
// low nibble the even k, k-major as nn.Linear.weight; e[N][K/32] one E8M0 byte per 32 consecutive k of a
// row, the block scale 2^(e - 127) with 2 <= e <= 252. A nibble (+-{0, .5, 1, 1.5, 2, 3, 4, 6}) times
// the scale is a normal bf16 number or zero, so the kernel multiplies by exactly known weights. x stays
// bf16.
//
// Arithmetic: v_cvt_scalef32_pk_bf16_fp4 turns one byte (two nibbles) into two bf16 with the block scale
// applied, exactly; the scale operand is the float whose bits are e << 23. Four of them make the bf16x8
// row operand of v_mfma_f32_16x16x32_bf16 (W the row operand, x the column operand), fp32
// accumulation, one bf16 rounding. Nothing is scaled after the MFMA.
//
// Work split. A block is 4 waves; wave w owns the 16 output columns n0 + 16 w .. + 15 over the block's
// K range and up to 32 rows of x (MT = 1 or 2 MFMA column tiles), so q is streamed once for M <= 32;
// further rows go to blockIdx.y and stream it again. One LDS stage is 512 k: two 256-deep chunks, each
// one 128-byte line of a weight row and 8 scale bytes. Per chunk a lane (n = lane & 15, g = lane >> 4)
// issues two 16-byte loads, bytes 16 (4 h + g) .. + 15 of the line for h = 0, 1 (a wave covers 16 rows x
// the whole line), and one 8-byte load of the chunk's scale bytes, of which it uses bytes g and 4 + g.
// A 16-byte load is the 32 k of MX block 4 h + g: one scale for all of it. Its four dwords feed four
// MFMAs; the x fragment of MFMA j is x[m][k0 + 32 (4 h + g) + 8 j ..], the same k's, so the order of k
// inside a chunk is the lanes' business only. A stage is twice as deep as the fp8 kernel's so that a
// lane has the same 64 bytes of weight in flight: x (through registers on its way to LDS, two buffers,
// shared by the 4 waves), q and e of the stage after the current one are loading while the 16 MT MFMAs
// and 64 conversions of the current one run.
//
// Split K. Narrow N (o, down) gives too few blocks, so K is cut into `splits` ranges of whole 256-deep
// chunks, at least 1024 deep (two stages: one to overlap with), over blockIdx.z. splits depends on
// (N, K) ONLY, every range is summed in ascending k, and the fp32 partials are added in ascending range
// order by a second kernel (no atomics): an output row is a function of its own x row and W, whatever
// M is and wherever the row sits in the batch. Rows of a 16-row MFMA tile beyond M are zeros in LDS and
// are not stored; a column of the MFMA result depends on its own column operand only.
//
// Mid M (33 .. ops.M_MID_W4 rows): linear_mid.h's loop with the producer below, the same K ranges, the same
// k-set and order per MFMA and the same combine kernel, so its output equals this kernel's bit for bit.
#include "common.h"
#include "linear_mid.h"  // bf16x8_t, lds_barrier, linear_mid_launch
#include "w4_cvt.h"      // w4_cvt8, e8m0

namespace {

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

constexpr int kBN = 64;               // output columns per block: 4 waves x one 16-wide MFMA tile
constexpr int kCK = 256;              // k per chunk: 128 weight bytes and 8 scale bytes of a row
constexpr int kKT = 2 * kCK;          // k per LDS stage
constexpr int kRowB = kKT * 2 + 16;   // LDS bytes per x row: +16 so the 16 m-lanes of a read start 4 banks apart
constexpr int kMinSplitChunks = 4;    // a K range is at least 4 x 256 deep
constexpr int kMaxSplits = 8;
constexpr int kTargetBlocks = 512;    // two blocks per CU

template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void linear_w4a16_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                           const unsigned char* __restrict__ W,
                                                           const unsigned char* __restrict__ E,
                                                           bf16_t* __restrict__ y, long long ldy,
                                                           float* __restrict__ part, int M, int N, int K, int per) {
  constexpr int kRows = MT * 16;                    // x rows per block
  constexpr int kPieces = kRows * (kKT / 8) / 256;  // 16-byte pieces of an x stage per thread
  constexpr int kBufB = kRows * kRowB;
  __shared__ __attribute__((aligned(16))) char lds[2 * kBufB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kBN + wave * 16;
  const int m0 = blockIdx.y * kRows;
  const bool active = n0 < N;  // N % 16 == 0: a wave has a whole tile or none (it still stages x)
  const int chunks = K / kCK;
  const int c0 = min((int)blockIdx.z * per, chunks), c1 = min(c0 + per, chunks);
  const int kbeg = c0 * kCK, kend = c1 * kCK;

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 xr[kPieces], wn[2][2];
  uint2 en[2];
  const size_t nrow = active ? n0 + ln : 0;
  const unsigned char* wrow = W + nrow * (size_t)(K / 2) + g * 16;
  const unsigned char* erow = E + nrow * (size_t)(K / 32);

  auto load_x = [&](int k) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int p = tid + 256 * i, row = p >> 6, col = (p & 63) * 8;
      xr[i] = u32x4{0u, 0u, 0u, 0u};
      if (m0 + row < M && k + col < kend)
        xr[i] = *reinterpret_cast<const u32x4*>(x + (size_t)(m0 + row) * ldx + k + col);
    }
  };
  auto store_x = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      const int p = tid + 256 * i, row = p >> 6, col = p & 63;
      *reinterpret_cast<u32x4*>(lds + buf * kBufB + row * kRowB + col * 16) = xr[i];
    }
  };
  auto load_w = [&](int k) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const bool in = active && k + c * kCK < kend;
      en[c] = make_uint2(0u, 0u);
      if (in) en[c] = *reinterpret_cast<const uint2*>(erow + (k + c * kCK) / 32);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        wn[c][h] = u32x4{0u, 0u, 0u, 0u};
        if (in) wn[c][h] = *reinterpret_cast<const u32x4*>(wrow + (k + c * kCK) / 2 + h * 64);
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
    u32x4 wc[2][2];
    float sc[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      sc[c][0] = e8m0((en[c].x >> (8 * g)) & 0xffu);
      sc[c][1] = e8m0((en[c].y >> (8 * g)) & 0xffu);
#pragma unroll
      for (int h = 0; h < 2; ++h) wc[c][h] = wn[c][h];
    }
    const bool more = k + kKT < kend;
    if (more) {
      load_x(k + kKT);
      load_w(k + kKT);
    }
    if (active) {
      const char* xb = lds + buf * kBufB + ln * kRowB + g * 64;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (k + c * kCK < kend) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const bf16x8_t wf = __builtin_bit_cast(bf16x8_t, w4_cvt8(wc[c][h][j], sc[c][h]));
#pragma unroll
              for (int t = 0; t < MT; ++t) {
                const bf16x8_t xf =
                    *reinterpret_cast<const bf16x8_t*>(xb + t * 16 * kRowB + c * 512 + h * 256 + j * 16);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[t], 0, 0, 0);
              }
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
      uint2 o;
      o.x = (unsigned)f2bf(acc[t][0]) | ((unsigned)f2bf(acc[t][1]) << 16);
      o.y = (unsigned)f2bf(acc[t][2]) | ((unsigned)f2bf(acc[t][3]) << 16);
      *reinterpret_cast<uint2*>(y + (size_t)m * ldy + n) = o;
    }
  }
}

// linear_mid.h's weight producer: a chunk is one 128-byte line of a weight row and its 8 scale bytes. Lane
// (n, g) holds bytes 16 (4 h + g) ..+15 of the line for h = 0, 1 (MX block 4 h + g: one scale, byte 4 h + g)
// and MFMA s = 4 h + j takes dword j of load h: the skinny kernel's fragments.
struct W4Producer {
  static constexpr int kCK = 256;  // the skinny kernel's chunk
  static constexpr bool kRowScale = false;
  const unsigned char* W;
  const unsigned char* E;
  struct Row {
    const unsigned char *w, *e;
  };
  struct Raw {
    u32x4 w[2];
    uint2 e;
  };
  __device__ __forceinline__ Row row(size_t n, int K, int g) const {
    return Row{W + n * (size_t)(K / 2) + g * 16, E + n * (size_t)(K / 32)};
  }
  static __device__ __forceinline__ void load(Raw& r, const Row& row, int k, bool in) {
    r.e = make_uint2(0u, 0u);
    r.w[0] = r.w[1] = u32x4{0u, 0u, 0u, 0u};
    if (in) {
      r.e = *reinterpret_cast<const uint2*>(row.e + k / 32);
      r.w[0] = *reinterpret_cast<const u32x4*>(row.w + k / 2);
      r.w[1] = *reinterpret_cast<const u32x4*>(row.w + k / 2 + 64);
    }
  }
  static __device__ __forceinline__ bf16x8_t frag(const Raw& r, int s, int g) {
    const float sc = e8m0((((s >> 2) ? r.e.y : r.e.x) >> (8 * g)) & 0xffu);
    return __builtin_bit_cast(bf16x8_t, w4_cvt8(r.w[s >> 2][s & 3], sc));
  }
};

// y[m][n..n+3] = bf16(part[0] + part[1] + ... in range order)
__global__ __launch_bounds__(256) void linear_w4_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ y,
                                                                long long ldy, int M, int N, int splits) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, quads = N / 4;
  if (idx >= (long long)M * quads) return;
  const int m = (int)(idx / quads), n = (int)(idx % quads) * 4;
  f32x4 a = *reinterpret_cast<const f32x4*>(part + (size_t)m * N + n);
  for (int z = 1; z < splits; ++z) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(part + ((size_t)z * M + m) * N + n);
    a[0] += b[0], a[1] += b[1], a[2] += b[2], a[3] += b[3];
  }
  uint2 o;
  o.x = (unsigned)f2bf(a[0]) | ((unsigned)f2bf(a[1]) << 16);
  o.y = (unsigned)f2bf(a[2]) | ((unsigned)f2bf(a[3]) << 16);
  *reinterpret_cast<uint2*>(y + (size_t)m * ldy + n) = o;
}

// out[32 i .. 32 i + 31] = bf16(nibbles of q[16 i .. 16 i + 15] * 2^(e[i] - 127)): one MX block, 16 bytes
// in and 64 bytes out per thread ([N][K/2], [N][K/32] and [N][K] are all contiguous: block i is block i)
__global__ __launch_bounds__(256) void dequant_w4_kernel(const unsigned char* __restrict__ W,
                                                         const unsigned char* __restrict__ E,
                                                         bf16_t* __restrict__ out, long long blocks) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= blocks) return;
  const float sc = e8m0(E[idx]);
  const u32x4 v = *reinterpret_cast<const u32x4*>(W + idx * 16);
  u32x4* o = reinterpret_cast<u32x4*>(out + idx * 32);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = w4_cvt8(v[j], sc);
}

int w4_splits(int N, int K) {
  const int blocks = (N + kBN - 1) / kBN, chunks = K / kCK;
  int ks = 1;
  while (ks < kMaxSplits && blocks * ks < kTargetBlocks && ks * 2 * kMinSplitChunks <= chunks) ks *= 2;
  return ks;
}

bool w4_shape_ok(int N, int K) { return N > 0 && K > 0 && N % 16 == 0 && K % kCK == 0; }

// the argument checks of both linear entries (0: take the call) and the K ranges: `per` chunks in each of `splits`
int w4_check(const void* x, const void* wq, const void* scale, const void* y, const void* ws, long long ws_bytes, int M,
             int N, int K, long long ldx, long long ldy, int& splits, int& per) {
  if (!w4_shape_ok(N, K) || M < 1 || (M + 31) / 32 > 65535) return -1;
  if ((ldx | ldy) & 7 || ldx < K || ldy < N) return -2;
  if (((uintptr_t)x | (uintptr_t)wq | (uintptr_t)scale | (uintptr_t)y) & 15) return -2;
  splits = w4_splits(N, K);
  per = (K / kCK + splits - 1) / splits;
  if (splits > 1 && (!ws || ((uintptr_t)ws & 15) || ws_bytes < (long long)splits * M * N * 4)) return -3;
  return 0;
}

}  // namespace

// K ranges rca_linear_w4a16 uses for an [N][K] weight (a function of N and K only); 0: outside the contract
RCA_API int rca_linear_w4_splits(int N, int K) { return w4_shape_ok(N, K) ? w4_splits(N, K) : 0; }

// y[M][N] (bf16, row stride ldy) = x[M][K] (bf16, row stride ldx) . deq(wq[N][K/2] e2m1 pairs, scale[N][K/32] E8M0)^T.
// ws: splits * M * N floats when rca_linear_w4_splits(N, K) > 1 (unused otherwise).
// -1: shape outside the contract (K % 256, N % 16, M >= 1); -2: alignment / stride; -3: workspace; -4: launch.
RCA_API int rca_linear_w4a16(const void* x, const void* wq, const void* scale, void* y, void* ws, long long ws_bytes,
                             int M, int N, int K, long long ldx, long long ldy, hipStream_t st) {
  int splits, per;
  if (const int rc = w4_check(x, wq, scale, y, ws, ws_bytes, M, N, K, ldx, ldy, splits, per)) return rc;
  const bool one = M <= 16;
  const dim3 grid((N + kBN - 1) / kBN, one ? 1 : (M + 31) / 32, splits);
  const bf16_t* xp = (const bf16_t*)x;
  const unsigned char* wp = (const unsigned char*)wq;
  const unsigned char* ep = (const unsigned char*)scale;
  bf16_t* yp = (bf16_t*)y;
  float* pp = (float*)ws;
  if (splits > 1) {
    if (one)
      linear_w4a16_kernel<1, true><<<grid, 256, 0, st>>>(xp, ldx, wp, ep, yp, ldy, pp, M, N, K, per);
    else
      linear_w4a16_kernel<2, true><<<grid, 256, 0, st>>>(xp, ldx, wp, ep, yp, ldy, pp, M, N, K, per);
    const long long quads = (long long)M * (N / 4);
    linear_w4_combine_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, st>>>(pp, yp, ldy, M, N, splits);
  } else if (one) {
    linear_w4a16_kernel<1, false><<<grid, 256, 0, st>>>(xp, ldx, wp, ep, yp, ldy, pp, M, N, K, per);
  } else {
    linear_w4a16_kernel<2, false><<<grid, 256, 0, st>>>(xp, ldx, wp, ep, yp, ldy, pp, M, N, K, per);
  }
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

// rca_linear_w4a16 for the rows above its tile (arguments, return codes and workspace rule are its own; any
// M >= 1 is taken): the weight is streamed and converted once per 128 rows of x (linear_mid.h). Bit for bit
// rca_linear_w4a16's output.
RCA_API int rca_linear_w4a16_mid(const void* x, const void* wq, const void* scale, void* y, void* ws,
                                 long long ws_bytes, int M, int N, int K, long long ldx, long long ldy, hipStream_t st) {
  int splits, per;
  if (const int rc = w4_check(x, wq, scale, y, ws, ws_bytes, M, N, K, ldx, ldy, splits, per)) return rc;
  const W4Producer p{(const unsigned char*)wq, (const unsigned char*)scale};
  if (!linear_mid_launch((const bf16_t*)x, ldx, p, (bf16_t*)y, ldy, (float*)ws, M, N, K, splits, per, st)) return -4;
  if (splits > 1) {
    const long long quads = (long long)M * (N / 4);
    linear_w4_combine_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, st>>>((float*)ws, (bf16_t*)y, ldy, M, N, splits);
  }
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

// out[N][K] (bf16, contiguous) = deq(wq[N][K/2], scale[N][K/32]): exact
RCA_API int rca_dequant_w4(const void* wq, const void* scale, void* out, int N, int K, hipStream_t st) {
  if (N <= 0 || K <= 0 || K % 32) return -1;
  if (((uintptr_t)wq | (uintptr_t)out) & 15) return -2;
  const long long blocks = (long long)N * (K / 32);
  if ((blocks + 255) / 256 > 0x7fffffffLL) return -1;
  dequant_w4_kernel<<<(unsigned)((blocks + 255) / 256), 256, 0, st>>>((const unsigned char*)wq,
                                                                     (const unsigned char*)scale, (bf16_t*)out, blocks);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}
