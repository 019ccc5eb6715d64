// Batched token sampling for gfx950: one launch takes the [B, V] logits of a generation step
// with per-row temperature / top_k / top_p / min_p / (seed, step) and writes B token ids.
//
// One workgroup of 1024 threads per row. Nothing is sorted: scaling by a positive temperature
// preserves order, so the top_k and top_p thresholds are found by a radix select (8 bits a pass,
// 2 passes for bf16, 4 for fp32) over order-preserving integer keys of the raw logits, with
// 256-bin LDS histograms of counts (top_k) or of probability mass (top_p). Mass is accumulated
// in 2^-40 fixed point with 64-bit integer LDS adds: an integer sum does not depend on the order
// of arrival, so every threshold, the total and the final inverse-CDF draw are bitwise functions
// of the row alone (no floating-point atomics anywhere). The draw is a prefix scan in index
// order over the one 1024 x 16 B tile that holds the target.
//
// The row is re-read from memory by every pass (it stays in L2: 128,256 bf16 = 250 KiB); all
// full 16-byte groups are read with one vector load per lane, the ragged head and tail of a row
// that is not 16-byte aligned element by element, so nothing outside [row, row + V) is touched.
//
// Semantics: see ops.sample_logits / ops.reference.sample_logits_ref.
#include "sampling_common.h"

namespace {

// Philox4x32-10, word 0, as a uniform strictly inside (0, 1). Its 25 significant bits are one more
// than fp32 holds (the top half of the range would round, up to 1.0), so it stays in double.
__device__ __forceinline__ double philox_uniform(unsigned seed_lo, unsigned seed_hi, unsigned step_lo, unsigned step_hi) {
  unsigned c0 = step_lo, c1 = step_hi, c2 = 0, c3 = 0, k0 = seed_lo, k1 = seed_hi;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return ((double)(c0 >> 8) + 0.5) * 5.9604644775390625e-08;  // 2^-24
}

template <typename T>
__global__ __launch_bounds__(kThreads) void sample_logits_kernel(const T* __restrict__ logits, long long row_stride,
                                                                 const int* __restrict__ params,
                                                                 const float* __restrict__ uniforms,
                                                                 long long* __restrict__ out, int V) {
  constexpr int P = Elem<T>::kPer;
  constexpr int kTile = kThreads * P;
  __shared__ u64 hist[kBins * kRep];
  __shared__ u64 bins[kBins];
  __shared__ u64 tiles[kMaxTiles];
  __shared__ u64 red[kWaves];
  __shared__ u64 sel[2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long row = blockIdx.x;

  Row R;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(logits + row * row_stride);
  R.a0 = reinterpret_cast<const char*>(addr & ~(uintptr_t)15);
  R.lo = (long)((addr & 15) / sizeof(T));
  R.hi = R.lo + V;
  R.ntiles = (int)((R.hi + kTile - 1) / kTile);

  const int* prm = params + row * 8;
  const float temp = __int_as_float(prm[0]);
  const int top_k = prm[1];
  const float top_p = __int_as_float(prm[2]);
  const float min_p = __int_as_float(prm[3]);

  // the maximum and the lowest index attaining it, as one 64-bit max of (key, ~index)
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
  const unsigned max_key = (unsigned)(best >> 32);
  long arg_max = (long)(0xffffffffu - (unsigned)best);
  arg_max = arg_max < V ? arg_max : V - 1;
  if (!(temp > 0.f)) {  // greedy
    if (tid == 0) out[row] = arg_max;
    return;
  }
  const float m = key_value(max_key);

  unsigned floor_key = 0;
  if (top_k > 0 && top_k < V) floor_key = radix_select<T>(R, false, (u64)top_k, 0.f, 0u, m, temp, hist, bins, sel);
  if (top_p < 1.f) floor_key = radix_select<T>(R, true, 0ull, top_p, floor_key, m, temp, hist, bins, sel);

  // kept mass per tile of 1024 x 16 B, then the tile that holds the target, then a scan of it
  for (int i = tid; i < R.ntiles; i += kThreads) tiles[i] = 0;
  __syncthreads();
  for (int t = 0; t < R.ntiles; ++t) {
    unsigned key[P], valid;
    load_keys<T>(R.a0, R.lo, R.hi, (long)t * kTile + (long)tid * P, key, valid);
    u64 s = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (((valid >> j) & 1) && key[j] >= floor_key) {
        const float w = weight(key[j], m, temp);
        if (w >= min_p) s += fixed(w);
      }
    }
    s = wave_sum_u64(s);
    if (lane == 0 && s) atomicAdd(&tiles[t], s);
  }
  __syncthreads();
  u64 total = 0;
  for (int t = 0; t < R.ntiles; ++t) total += tiles[t];
  if (total == 0) {  // out of contract (NaN, no finite logit): still an index inside the row
    if (tid == 0) out[row] = arg_max;
    return;
  }
  const double u = uniforms ? (double)uniforms[row]
                            : philox_uniform((unsigned)prm[4], (unsigned)prm[5], (unsigned)prm[6], (unsigned)prm[7]);
  // the first kept index whose inclusive running sum exceeds u * total, i.e. reaches need
  const double target = u * (double)total;
  u64 need = target >= 0.0 ? (u64)target : 0ull;
  need = (need < total ? need : total - 1) + 1;
  int ts = 0;
  for (; ts < R.ntiles - 1; ++ts) {
    if (tiles[ts] >= need) break;
    need -= tiles[ts];
  }
  unsigned key[P], valid;
  const long v = (long)ts * kTile + (long)tid * P;
  load_keys<T>(R.a0, R.lo, R.hi, v, key, valid);
  u64 wq[P], local = 0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    wq[j] = 0;
    if (((valid >> j) & 1) && key[j] >= floor_key) {
      const float w = weight(key[j], m, temp);
      if (w >= min_p) wq[j] = fixed(w);
    }
    local += wq[j];
  }
  u64 incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();  // every read of red[] above is over
  if (lane == 63) red[wid] = incl;
  __syncthreads();
  u64 before = incl - local;
  for (int i = 0; i < wid; ++i) before += red[i];
  if (before < need && need <= before + local) {  // exactly one thread
    long tok = arg_max;
    u64 run = before;
    bool found = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      run += wq[j];
      if (!found && run >= need) {
        found = true;
        tok = v + j - R.lo;
      }
    }
    out[row] = tok;
  }
}

}  // namespace

// logits: [B, V] bf16 (is_bf16 != 0) or fp32, unit inner stride, row_stride in elements.
// params: int32 [B, 8] = {temperature bits, top_k, top_p bits, min_p bits, seed lo, seed hi, step lo, step hi}.
// uniforms: nullable fp32 [B], replaces the Philox value. out: int64 [B].
RCA_API int rca_sample_logits(const void* logits, long long row_stride, int is_bf16, const void* params,
                              const void* uniforms, void* out, int B, int V, hipStream_t st) {
  if (B < 0 || B > 65535 || V < 1 || V > kMaxV) return 1;
  if (B == 0) return 0;
  if (!logits || !params || !out) return 2;
  if (is_bf16) {
    hipLaunchKernelGGL(sample_logits_kernel<bf16_t>, dim3(B), dim3(kThreads), 0, st, (const bf16_t*)logits, row_stride,
                       (const int*)params, (const float*)uniforms, (long long*)out, V);
  } else {
    hipLaunchKernelGGL(sample_logits_kernel<float>, dim3(B), dim3(kThreads), 0, st, (const float*)logits, row_stride,
                       (const int*)params, (const float*)uniforms, (long long*)out, V);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
