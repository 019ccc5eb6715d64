// FP8 paged KV cache for gfx950: the quantising cache append and the single-token (decode)
// attention over it. The bf16 counterparts are in attention_decode.hip, and so are the entry points
// of both kinds, rca_kv_cache_append and rca_attn_decode_paged, which reach the launchers at the end
// of this file when they are given scales (paged_kv.h).
//
// Cache layout per layer: k_cache, v_cache = OCP e4m3 bytes [num_blocks, page_size, Hk, D] with the
// slot arithmetic of the bf16 cache (slot = block * page_size + offset), plus k_scale, v_scale =
// fp32 [num_blocks, page_size, Hk]: one scale per (token, kv head), at slot * Hk + hk. A scale is
// the smallest power of two s with max|x| / s <= 448 over the head row, clamped to [2^-126, 2^127],
// 1 for an all-zero row; the stored element is RNE-to-e4m3 of x / s. The quotient is exact in fp32
// and never exceeds 448, so the conversion never saturates, and byte * scale is exact in bf16 and
// fp32: the attention kernels compute on exactly known values.
//
// Append: D / 8 lanes per head row, 16 B (8 bf16) in and 8 B out per lane. The row's amax is
// reduced over those lanes with shuffles, the exponent comes from the fp32 bits, the elements are
// multiplied by the exact reciprocal and packed with v_cvt_pk_fp8_f32. One lane per row stores the
// scale. No LDS. A token with slot -1, or outside [0, num_slots), writes nothing.
//
// Decode: attn_decode_paged_kernel's design (one 4-wave workgroup per (split, kv head, sequence),
// D / 8 lanes per token, fp32 VALU scores and PV, base-2 online softmax per (lane group, wave),
// the same grid, split policy, workspace layout and combine kernel), with 8-byte K/V loads. A wave
// step covers NG groups of 16 consecutive tokens (NG = 2: 32 tokens, the bf16 kernel's bytes in
// flight; NG = 1: its 16 tokens at half the bytes); page_size % 16 == 0 puts each group inside one
// page, so a step may span two pages (page 16) at one wave-uniform block_table lookup per group.
// The score is (q . k8) * k_scale, the scale applied after the lane reduction; v_scale multiplies p
// for the PV accumulation only, never l.
//
// Masking is by loop bounds and by not loading, as in the bf16 kernel: a token at position >=
// context_lens[b] is never read, neither its bytes nor its scales (its lanes get zero K/V, zero
// scales and a -inf score); block_table[b, j] is read only for j < ceil(context_lens[b] /
// page_size); an entry outside [0, num_blocks) is not a block of this cache and its tokens are
// skipped. So NaN garbage in dead slots, bytes or scales, cannot reach the output. A K/V address is
// (blk * page_size + off + t) * Hk * D + hk * D + c with 0 <= blk < num_blocks checked, off + t <
// page_size (off a multiple of 16 below page_size, t < 16) and c < D; the scale address is
// (blk * page_size + off + t) * Hk + hk under the same bounds.
#include "attention_decode_merge.h"
#include "kv_fp8.h"
#include "paged_kv.h"

namespace {

template <int D, int G, int NG>
__global__ __launch_bounds__(256, (G == 8 ? 1 : 2)) void attn_decode_paged_fp8_kernel(
    const bf16_t* __restrict__ q, long q_stride, const fp8_t* __restrict__ kc, const fp8_t* __restrict__ vc,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const int* __restrict__ block_table,
    const int* __restrict__ context_lens, int max_blocks, int num_blocks, int page_size, int Hk, float scale_log2,
    int num_splits, bf16_t* __restrict__ out, float* __restrict__ part_o, float* __restrict__ part_ml) {
  constexpr int LPT = D / 8;     // lanes per token (8 B of the row each)
  constexpr int TPW = 64 / LPT;  // tokens per wave-wide load
  constexpr int UG = 16 / TPW;   // loads per lane, operand and 16-token group
  constexpr int U = NG * UG;     // loads in flight per lane and operand

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = lane % LPT, grp = lane / LPT;

  long ctx_l = context_lens[b];
  const long cap = (long)max_blocks * page_size;  // never index past the block table's row
  const int ctx = (int)(ctx_l < 0 ? 0 : (ctx_l > cap ? cap : ctx_l));
  const int npages = (ctx + page_size - 1) / page_size;
  const int pps = (npages + num_splits - 1) / num_splits;
  const int p0 = min(split * pps, npages);
  const int p1 = min(p0 + pps, npages);
  // this split's tokens [tok0, tok1) as 16-token groups; tok0 is a multiple of page_size
  const int tok0 = p0 * page_size, tok1 = min(p1 * page_size, ctx);
  const int ngrp = (tok1 - tok0 + 15) >> 4;
  const int pshift = (page_size & (page_size - 1)) == 0 ? __builtin_ctz(page_size) : -1;

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

  const long tok_stride = (long)Hk * D;  // bytes between consecutive slots
  const int* bt = block_table + (long)b * max_blocks;
  const long lane_kv = (long)grp * tok_stride + (long)hk * D + sub * 8;  // this lane inside a group
  const long lane_sc = (long)grp * Hk + hk;

  // one step of NG 16-token groups: group n starts at slot slot0[n] and has live[n] live tokens
  // (0: nothing to read); FULL = every token of the step is live (no per-lane tests)
  auto step = [&](const long (&slot0)[NG], const int (&live)[NG], auto full_tag) {
    constexpr bool FULL = decltype(full_tag)::value;
    uint2 kr[U], vr[U];
    float ks[U], vs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int n = u / UG, t = (u % UG) * TPW;  // token t + grp of group n
      if (FULL || t + grp < live[n]) {
        const long kv = (slot0[n] + t) * tok_stride + lane_kv, sc = (slot0[n] + t) * Hk + lane_sc;
        kr[u] = *reinterpret_cast<const uint2*>(kc + kv);
        vr[u] = *reinterpret_cast<const uint2*>(vc + kv);
        ks[u] = ksc[sc];
        vs[u] = vsc[sc];
      } else {
        kr[u] = uint2{0u, 0u};
        vr[u] = uint2{0u, 0u};
        ks[u] = 0.f;
        vs[u] = 0.f;
      }
    }
    float s[U][G];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      unpack8_fp8(kr[u], kf);
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
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool dead = !FULL && (u % UG) * TPW + grp >= live[u / UG];
#pragma unroll
      for (int g = 0; g < G; ++g) s[u][g] = dead ? neg_inf() : s[u][g] * ks[u];
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
      unpack8_fp8(vr[u], vf);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pv = p[u][g] * vs[u];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[g][j] += pv * vf[j];
      }
    }
  };

#pragma unroll 1
  for (int g0 = wave * NG; g0 < ngrp; g0 += kDecWaves * NG) {
    long slot0[NG];
    int live[NG];
    bool full = true;
#pragma unroll
    for (int n = 0; n < NG; ++n) {
      const int key0 = tok0 + 16 * (g0 + n);
      int lv = min(16, tok1 - key0);  // <= 0: past this split's tokens
      long s0 = 0;
      if (lv > 0) {
        const int pg = pshift >= 0 ? key0 >> pshift : key0 / page_size;  // < p1 <= npages
        const int blk = bt[pg];
        if ((unsigned)blk < (unsigned)num_blocks) s0 = (long)blk * page_size + (key0 - pg * page_size);
        else lv = 0;  // not a block of this cache: nothing to read
      }
      slot0[n] = s0;
      live[n] = max(lv, 0);
      full = full && lv == 16;
    }
    if (full) step(slot0, live, std::true_type{});
    else step(slot0, live, std::false_type{});
  }

  decode_merge_store<D, G>(m, l, o, wave, split, hk, b, Hk, num_splits, out, part_o, part_ml);
}

// Quantising append. Thread -> one 8-element chunk of a token's K|V heads (qkv columns
// [Hq*D, (Hq+2Hk)*D)); the LPT = D / 8 threads of a head row are consecutive lanes of one wave
// (LPT divides 64), share t and slot, and so leave or stay together.
template <int LPT>
__global__ __launch_bounds__(256) void kv_cache_append_fp8_kernel(const bf16_t* __restrict__ qkv, long row_stride,
                                                                  const int* __restrict__ slot_mapping,
                                                                  fp8_t* __restrict__ kc, fp8_t* __restrict__ vc,
                                                                  float* __restrict__ ksc, float* __restrict__ vsc,
                                                                  long T, int Hk, int q_cols, long num_slots) {
  const int kv_chunks = Hk * LPT;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long t = idx / (2 * kv_chunks);
  if (t >= T) return;
  const int c = (int)(idx % (2 * kv_chunks));
  const long slot = slot_mapping[t];
  if (slot < 0 || slot >= num_slots) return;  // -1: padding token, writes nothing
  float x[8];
  unpack8(*reinterpret_cast<const u32x4*>(qkv + t * row_stride + q_cols + (long)c * 8), x);
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(x[j]));
#pragma unroll
  for (int off = 1; off < LPT; off <<= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  // amax = (1 + M / 2^23) * 2^(E - 127); 448 = 1.75 * 2^8: the smallest power of two s with
  // amax / s <= 448 is 2^(E - 127 - 8), one more when the mantissa exceeds 1.75's. Biased exponent
  // clamped to [1, 254] (a subnormal or tiny amax: 2^-126); amax == 0: 1.
  const unsigned bits = __float_as_uint(amax);
  int eb = (int)(bits >> 23) - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  eb = bits == 0u ? 127 : min(max(eb, 1), 254);
  const float inv = __uint_as_float((unsigned)(254 - eb) << 23);  // exact 1 / s: eb <= 248, so >= 2^-121
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv, x[3] * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] * inv, x[5] * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] * inv, x[7] * inv, hi, true);
  const bool is_v = c >= kv_chunks;
  const int ck = is_v ? c - kv_chunks : c;  // chunk inside the token's K (or V) heads: head ck / LPT
  *reinterpret_cast<uint2*>((is_v ? vc : kc) + slot * ((long)kv_chunks * 8) + (long)ck * 8) =
      uint2{(unsigned)lo, (unsigned)hi};
  if (ck % LPT == 0) (is_v ? vsc : ksc)[slot * Hk + ck / LPT] = __uint_as_float((unsigned)eb << 23);
}

int g_dec_fp8_groups = 2;  // 16-token groups per wave step: rca_attn_decode_fp8_set_step

}  // namespace

// Tokens per wave step of the fp8 decode kernel: 32 (default) or 16. A measurement knob
// (scripts/decode_bench.py --fp8-step; profiles/kv_cache_fp8.md has the comparison).
RCA_API int rca_attn_decode_fp8_set_step(int tokens) {
  if (tokens != 16 && tokens != 32) return -1;
  g_dec_fp8_groups = tokens / 16;
  return 0;
}

// rca_kv_cache_append (attention_decode.hip) over the e4m3 cache. D / 8 is a power of two <= 64.
int launch_kv_append_fp8(const void* qkv, long long row_stride, const int* slot_mapping, void* k_cache, void* v_cache,
                         void* k_scale, void* v_scale, long long T, int Hq, int Hk, int D, long long num_slots,
                         unsigned blocks, hipStream_t stream) {
  auto launch = [&](auto lpt) {
    hipLaunchKernelGGL(kv_cache_append_fp8_kernel<lpt.value>, dim3(blocks), dim3(256), 0, stream, (const bf16_t*)qkv,
                       (long)row_stride, slot_mapping, (fp8_t*)k_cache, (fp8_t*)v_cache, (float*)k_scale,
                       (float*)v_scale, (long)T, Hk, Hq * D, (long)num_slots);
    return (int)hipGetLastError();
  };
  using namespace paged_kv;
  switch (D / 8) {
    case 1: return launch(int_c<1>{});
    case 2: return launch(int_c<2>{});
    case 4: return launch(int_c<4>{});
    case 8: return launch(int_c<8>{});
    case 16: return launch(int_c<16>{});
    case 32: return launch(int_c<32>{});
    case 64: return launch(int_c<64>{});
  }
  return -1;
}

// rca_attn_decode_paged (attention_decode.hip) over the e4m3 cache.
int launch_attn_decode_fp8(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                           const void* k_scale, const void* v_scale, const int* block_table, const int* context_lens,
                           void* out, void* part_o, void* part_ml, int B, int Hq, int Hk, int D, int page_size,
                           int max_blocks, int num_blocks, float scale, int num_splits, hipStream_t stream) {
  auto launch = [&](auto ng) {
    return paged_kv::dispatch_dg(D, Hq / Hk, [&](auto d, auto g) {
      // G = 8: 32 tokens of s and p for 8 rows do not fit the VGPRs
      constexpr int NG = g.value == 8 ? 1 : ng.value;
      hipLaunchKernelGGL((attn_decode_paged_fp8_kernel<d.value, g.value, NG>), dim3(num_splits, Hk, B), dim3(256), 0,
                         stream, (const bf16_t*)q, (long)q_stride, (const fp8_t*)k_cache, (const fp8_t*)v_cache,
                         (const float*)k_scale, (const float*)v_scale, block_table, context_lens, max_blocks,
                         num_blocks, page_size, Hk, scale * paged_kv::kLog2e, num_splits, (bf16_t*)out,
                         (float*)part_o, (float*)part_ml);
      return (int)hipGetLastError();
    });
  };
  const int rc = g_dec_fp8_groups == 2 ? launch(paged_kv::int_c<2>{}) : launch(paged_kv::int_c<1>{});
  if (rc != 0 || num_splits == 1) return rc;
  return launch_split_combine((const float*)part_o, (const float*)part_ml, (bf16_t*)out, (long)B * Hq, num_splits, D,
                              stream);
}
