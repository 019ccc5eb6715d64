// Single-token (decode) attention over a paged bf16 KV cache, and the cache append, for gfx950.
//
// Cache layout per layer: k_cache, v_cache = bf16 [num_blocks, page_size, Hk, D]; a token's slot is
// block * page_size + offset, so its K (or V) heads are the Hk*D contiguous elements at slot*Hk*D.
//
// Decode is a memory-bound KV stream (no MFMA): one 4-wave workgroup handles all G = Hq/Hk query
// rows of one kv head over a contiguous range of pages (one split), so every K/V byte is read from
// HBM once for the whole GQA group. K/V go global -> VGPR with 16-byte loads (D/8 lanes per token,
// 64/(D/8) tokens per wave-instruction, 16 tokens in flight per wave); scores and PV run on the
// VALU in fp32 with a base-2 online softmax. Every (lane group, wave) keeps its own running
// (m, l, O); they are merged by cross-lane butterflies, then across the 4 waves through LDS.
// num_splits == 1 normalises and writes bf16 directly; otherwise fp32 partial O and (m, l) go to a
// workspace that attn_decode_combine_kernel (attention_combine.h) merges in split order
// (deterministic, no atomics).
//
// Masking is by loop bounds and by not loading: a token at position >= context_lens[b] is never
// read (its lanes get zero K/V and a -inf score), and block_table[b, j] is read only for
// j < ceil(context_lens[b] / page_size), so NaN/Inf garbage in dead slots cannot reach the output.
//
// The entry points at the end, rca_kv_cache_append and rca_attn_decode_paged, serve both cache
// kinds: the e4m3 kernels and their launchers are in attention_decode_fp8.hip (paged_kv.h).
#include "attention_combine.h"
#include "attention_common.h"
#include "paged_kv.h"

namespace {

constexpr int kDecWaves = 4;

// exp2(a - m) with m == -inf (nothing seen yet) mapped to a zero reference: exp2(-inf - 0) = 0,
// never exp2(-inf + inf) = NaN
__device__ __forceinline__ float safe_ref(float m) { return m == neg_inf() ? 0.f : m; }

template <int D, int G>
__global__ __launch_bounds__(256, (G == 8 ? 1 : 2)) void attn_decode_paged_kernel(
    const bf16_t* __restrict__ q, long q_stride, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const int* __restrict__ block_table, const int* __restrict__ context_lens, int max_blocks, int num_blocks,
    int page_size, int Hk, float scale_log2, int num_splits, bf16_t* __restrict__ out, float* __restrict__ part_o,
    float* __restrict__ part_ml) {
  constexpr int LPT = D / 8;     // lanes per token (16 B of the row each)
  constexpr int TPW = 64 / LPT;  // tokens per wave-wide load
  constexpr int STEP = 16;               // tokens per wave step
  constexpr int U = STEP / TPW;          // loads in flight per lane and operand
  __shared__ float sm_o[kDecWaves][G][D];
  __shared__ float sm_m[kDecWaves][G], sm_l[kDecWaves][G];

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = lane % LPT, grp = lane / LPT;
  const int Hq = Hk * G;

  long ctx_l = context_lens[b];
  const long cap = (long)max_blocks * page_size;  // never index past the block table's row
  const int ctx = (int)(ctx_l < 0 ? 0 : (ctx_l > cap ? cap : ctx_l));
  const int npages = (ctx + page_size - 1) / page_size;
  const int pps = (npages + num_splits - 1) / num_splits;
  const int p0 = split * pps;
  const int p1 = min(p0 + pps, npages);

  float qf[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const u32x4 raw = *reinterpret_cast<const u32x4*>(q + (long)b * q_stride + (long)(hk * G + g) * D + sub * 8);
    unpack8(raw, qf[g]);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[g][j] *= scale_log2;
  }

  float m[G], l[G], o[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = neg_inf();
    l[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[g][j] = 0.f;
  }

  const long tok_stride = (long)Hk * D;  // elements between consecutive slots
  const int* bt = block_table + (long)b * max_blocks;

  // one STEP-token step: FULL = every token of the step is live (no per-lane tests)
  auto step = [&](const bf16_t* kp, const bf16_t* vp, int live, auto full_tag) {
    constexpr bool FULL = decltype(full_tag)::value;
    u32x4 kr[U], vr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = u * TPW + grp;
      if (FULL || t < live) {
        kr[u] = *reinterpret_cast<const u32x4*>(kp + t * tok_stride);
        vr[u] = *reinterpret_cast<const u32x4*>(vp + t * tok_stride);
      } else {
        kr[u] = u32x4{0u, 0u, 0u, 0u};
        vr[u] = u32x4{0u, 0u, 0u, 0u};
      }
    }
    float s[U][G];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      unpack8(kr[u], kf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += qf[g][j] * kf[j];
        s[u][g] = a;
      }
    }
#pragma unroll
    for (int off = 1; off < LPT; off <<= 1)
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g) s[u][g] += __shfl_xor(s[u][g], off, 64);
    if (!FULL) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (u * TPW + grp >= live) {
#pragma unroll
          for (int g = 0; g < G; ++g) s[u][g] = neg_inf();
        }
    }
    float p[U][G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u][g]);
      const float mr = safe_ref(mn);
      const float alpha = fast_exp2(m[g] - mr);
      float ls = l[g] * alpha;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        p[u][g] = fast_exp2(s[u][g] - mr);
        ls += p[u][g];
      }
      l[g] = ls;
      m[g] = mn;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[g][j] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[8];
      unpack8(vr[u], vf);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 8; ++j) o[g][j] += p[u][g] * vf[j];
    }
  };

#pragma unroll 1
  for (int pg = p0 + wave; pg < p1; pg += kDecWaves) {
    const int blk = bt[pg];
    if ((unsigned)blk >= (unsigned)num_blocks) continue;  // not a block of this cache: nothing to read
    const long base = (long)blk * page_size * tok_stride + (long)hk * D + sub * 8;
    const int live_pg = min(page_size, ctx - pg * page_size);  // >= 1: pg < npages
#pragma unroll 1
    for (int t0 = 0; t0 < live_pg; t0 += STEP) {
      const bf16_t* kp = kc + base + t0 * tok_stride;
      const bf16_t* vp = vc + base + t0 * tok_stride;
      if (live_pg - t0 >= STEP) {
        step(kp, vp, STEP, std::true_type{});
      } else {
        step(kp, vp, live_pg - t0, std::false_type{});
      }
    }
  }

  // merge the TPW lane groups of the wave (butterfly: both partners compute the same sums)
#pragma unroll
  for (int off = LPT; off < 64; off <<= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float mn = fmaxf(m[g], __shfl_xor(m[g], off, 64));
      const float a = fast_exp2(m[g] - safe_ref(mn));
      const float ls = l[g] * a;
      l[g] = ls + __shfl_xor(ls, off, 64);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = o[g][j] * a;
        o[g][j] = x + __shfl_xor(x, off, 64);
      }
      m[g] = mn;
    }
  }
  if (grp == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sm_o[wave][g][sub * 8 + j] = o[g][j];
      if (sub == 0) {
        sm_m[wave][g] = m[g];
        sm_l[wave][g] = l[g];
      }
    }
  }
  __syncthreads();

  // merge the 4 waves in wave order; thread -> (query row g, 8 columns c)
  if (tid < G * LPT) {
    const int g = tid / LPT, c = tid % LPT;
    float mt = neg_inf();
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) mt = fmaxf(mt, sm_m[w][g]);
    const float mr = safe_ref(mt);
    float lt = 0.f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) {
      const float a = fast_exp2(sm_m[w][g] - mr);
      lt += a * sm_l[w][g];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += a * sm_o[w][g][c * 8 + j];
    }
    const int hq = hk * G + g;
    if (num_splits == 1) {
      const float inv = lt > 0.f ? 1.f / lt : 0.f;  // context_len 0: zeros
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] *= inv;
      *reinterpret_cast<u32x4*>(out + ((long)b * Hq + hq) * D + c * 8) = pack8(acc);
    } else {
      const long row = ((long)b * Hq + hq) * num_splits + split;
      float* po = part_o + row * D + c * 8;
      *reinterpret_cast<f32x4*>(po) = f32x4{acc[0], acc[1], acc[2], acc[3]};
      *reinterpret_cast<f32x4*>(po + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
      if (c == 0) *reinterpret_cast<float2*>(part_ml + row * 2) = float2{mt, lt};  // empty split: (-inf, 0)
    }
  }
}

// One thread per 16-byte chunk of a token's K|V heads (qkv columns [Hq*D, (Hq+2Hk)*D)).
__global__ __launch_bounds__(256) void kv_cache_append_kernel(const bf16_t* __restrict__ qkv, long row_stride,
                                                              const int* __restrict__ slot_mapping,
                                                              bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, long T,
                                                              int kv_chunks, int q_cols, long num_slots) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long t = idx / (2 * kv_chunks);
  if (t >= T) return;
  const int c = (int)(idx % (2 * kv_chunks));
  const long slot = slot_mapping[t];
  if (slot < 0 || slot >= num_slots) return;  // -1: padding token, writes nothing
  const u32x4 x = *reinterpret_cast<const u32x4*>(qkv + t * row_stride + q_cols + (long)c * 8);
  const bool is_v = c >= kv_chunks;
  bf16_t* dst = (is_v ? vc : kc) + slot * ((long)kv_chunks * 8) + (long)(is_v ? c - kv_chunks : c) * 8;
  *reinterpret_cast<u32x4*>(dst) = x;
}

}  // namespace

// Default split count of the paged decode. Heuristic:
//   * the grid is num_splits * Hk * B workgroups; aim for >= 512 of them (two per CU on the 256 CUs,
//     so one workgroup's load latency hides behind the other's math);
//   * a split streams at least 4 pages and at least 256 tokens (one workgroup round is 64 tokens:
//     below a few rounds the partial-result write and the combine pass cost more than they spread);
//   * at most 16 splits (the combine reads num_splits partials per output row).
RCA_API int rca_attn_decode_num_splits(int B, int Hk, int max_context, int page_size) {
  if (B <= 0 || Hk <= 0 || max_context <= 0 || page_size <= 0) return 1;
  const long base = (long)B * Hk;
  const long want = (512 + base - 1) / base;
  const long pages = ((long)max_context + page_size - 1) / page_size;
  const long min_pages = 4 > (256 + page_size - 1) / page_size ? 4 : (256 + page_size - 1) / page_size;
  const long by_work = pages / min_pages;
  long n = want < by_work ? want : by_work;
  if (n > 16) n = 16;
  if (n < 1) n = 1;
  return (int)n;
}

int launch_kv_append_bf16(const void* qkv, long long row_stride, const int* slot_mapping, void* k_cache, void* v_cache,
                          void*, void*, long long T, int Hq, int Hk, int D, long long num_slots, unsigned blocks,
                          hipStream_t stream) {
  hipLaunchKernelGGL(kv_cache_append_kernel, dim3(blocks), dim3(256), 0, stream, (const bf16_t*)qkv, (long)row_stride,
                     slot_mapping, (bf16_t*)k_cache, (bf16_t*)v_cache, (long)T, Hk * D / 8, Hq * D, (long)num_slots);
  return (int)hipGetLastError();
}

int launch_attn_decode_bf16(const void* q, long long q_stride, const void* k_cache, const void* v_cache, const void*,
                            const void*, const int* block_table, const int* context_lens, void* out, void* part_o,
                            void* part_ml, int B, int Hq, int Hk, int D, int page_size, int max_blocks, int num_blocks,
                            float scale, int num_splits, hipStream_t stream) {
  const int rc = paged_kv::dispatch_dg(D, Hq / Hk, [&](auto d, auto g) {
    hipLaunchKernelGGL((attn_decode_paged_kernel<d.value, g.value>), dim3(num_splits, Hk, B), dim3(256), 0, stream,
                       (const bf16_t*)q, (long)q_stride, (const bf16_t*)k_cache, (const bf16_t*)v_cache, block_table,
                       context_lens, max_blocks, num_blocks, page_size, Hk, scale * paged_kv::kLog2e, num_splits,
                       (bf16_t*)out, (float*)part_o, (float*)part_ml);
    return (int)hipGetLastError();
  });
  if (rc != 0 || num_splits == 1) return rc;
  return launch_split_combine((const float*)part_o, (const float*)part_ml, (bf16_t*)out, (long)B * Hq, num_splits, D,
                              stream);
}

// qkv: [T, >= (Hq+2Hk)*D] bf16 with row stride `row_stride` elements (a multiple of 8; K heads at
// column Hq*D, V heads after them), 16-B aligned; slot_mapping: int32 [T], -1 = skip; caches and
// scales: either kind (paged_kv.h), num_slots = num_blocks * page_size. D is any multiple of 8; the
// e4m3 cache needs D / 8 to be a power of two <= 64 (the lanes that reduce a head row's amax).
RCA_API int rca_kv_cache_append(const void* qkv, long long row_stride, const int* slot_mapping, void* k_cache,
                                void* v_cache, void* k_scale, void* v_scale, long long T, int Hq, int Hk, int D,
                                long long num_slots, hipStream_t stream) {
  if (T == 0 || num_slots == 0) return 0;  // no token, or no slot a token could go to (a cache of no blocks)
  if (T < 0 || !paged_kv::heads_ok(Hq, Hk) || D <= 0 || (D & 7) || num_slots < 0) return -1;
  if (!paged_kv::rows_ok(row_stride, (long long)(Hq + 2 * Hk) * D)) return -1;
  const int lpt = D / 8;
  if ((k_scale || v_scale) && ((lpt & (lpt - 1)) || lpt > 64)) return -1;
  const long long blocks = (T * 2 * Hk * lpt + 255) / 256;
  if (blocks >= (1LL << 31)) return -2;
  if (!paged_kv::all_set(qkv, slot_mapping) || !paged_kv::aligned(16, qkv)) return -3;
  if (!paged_kv::caches_ok(k_cache, v_cache, k_scale, v_scale)) return -3;
  return (k_scale ? launch_kv_append_fp8 : launch_kv_append_bf16)(qkv, row_stride, slot_mapping, k_cache, v_cache,
                                                                  k_scale, v_scale, T, Hq, Hk, D, num_slots,
                                                                  (unsigned)blocks, stream);
}

// q: logical [B, Hq, D] bf16 at q + b*q_stride + h*D (q_stride in elements: Hq*D for a contiguous q,
// (Hq+2Hk)*D to read it in place from the fused qkv row). block_table: int32 [B, max_blocks];
// context_lens: int32 [B]; caches and scales: either kind (paged_kv.h). out: bf16 [B, Hq*D].
// num_splits > 1 needs part_o (fp32 [B, Hq, num_splits, D]) and part_ml (fp32 [B, Hq, num_splits, 2]
// = (m, l)). D is 64 or 128, Hq / Hk one of 1, 2, 4, 8, page_size a multiple of 16.
RCA_API int rca_attn_decode_paged(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                                  const void* k_scale, const void* v_scale, const int* block_table,
                                  const int* context_lens, void* out, void* part_o, void* part_ml, int B, int Hq,
                                  int Hk, int D, int page_size, int max_blocks, int num_blocks, float scale,
                                  int num_splits, hipStream_t stream) {
  if (B == 0) return 0;
  if (!paged_kv::attn_shape_ok(B, Hq, Hk, D, q_stride, page_size, max_blocks, num_blocks, num_splits)) return -1;
  if (!paged_kv::grid_ok(B, Hk)) return -2;
  if (!paged_kv::caches_ok(k_cache, v_cache, k_scale, v_scale)) return -3;
  if (!paged_kv::attn_ptrs_ok(q, out, block_table, context_lens, part_o, part_ml, num_splits)) return -3;
  return (k_scale ? launch_attn_decode_fp8 : launch_attn_decode_bf16)(
      q, q_stride, k_cache, v_cache, k_scale, v_scale, block_table, context_lens, out, part_o, part_ml, B, Hq, Hk, D,
      page_size, max_blocks, num_blocks, scale, num_splits, stream);
}
