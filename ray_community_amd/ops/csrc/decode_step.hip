// The decode step's RoPE and KV-cache append in one launch, with position and slot derived on the
// device: rope_kernel (elementwise.hip) followed by kv_cache_append_kernel (attention_decode.hip) or
// kv_cache_append_fp8_kernel (attention_decode_fp8.hip), bit for bit, for one new token per
// sequence. Nothing the host computes per step goes in except block_table and context_lens, which a
// captured decode graph keeps in static buffers (models/decode_graph.py).
//
// Row b of the fused qkv [B, (Hq+2Hk)*D] holds the token that brings sequence b to n =
// context_lens[b] tokens: its position is n - 1 and its slot block_table[b, (n-1) / page] * page +
// (n-1) % page. A row is inactive, left untouched and writing nothing, when n <= 0, when n exceeds
// max_blocks * page (the block table's row, as attn_decode_paged_kernel's `cap`) or max_pos (the
// RoPE table), or when the table entry is no block of this cache.
//
// One thread per 16 elements of a head: chunk c..c+7 and its rotation partner D/2+c..D/2+c+7, 16 B
// each. A q head is rotated and stored back; a K head is rotated, stored back and written to the
// cache from the same registers (rounded to bf16 first: the cache gets what the qkv row holds); a V
// head is copied. The D / 16 threads of a head are consecutive lanes of one wave, share the row and
// so leave or stay together: the fp8 variant reduces the head row's amax over them with shuffles
// and then quantises as kv_cache_append_fp8_kernel does (the power-of-two scale rule and
// v_cvt_pk_fp8_f32 on the exact quotient). No LDS, no atomics.
#include "kv_fp8.h"
#include "paged_kv.h"
#include "rope_rotate.h"

namespace {

template <int D, bool FP8>
__global__ __launch_bounds__(256) void rope_kv_append_decode_kernel(
    bf16_t* __restrict__ qkv, long row_stride, const float2* __restrict__ cs, int max_pos,
    const int* __restrict__ block_table, const int* __restrict__ context_lens, int max_blocks, int page_size,
    int num_blocks, void* __restrict__ k_cache, void* __restrict__ v_cache, float* __restrict__ ksc,
    float* __restrict__ vsc, int B, int Hq, int Hk) {
  constexpr int HALF = D / 2, PH = D / 16;  // PH: threads per head
  const int per_row = (Hq + 2 * Hk) * PH;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)B * (unsigned)per_row) return;  // the host keeps B * per_row below 2^31
  const int b = (int)(i / (unsigned)per_row);
  const int r = (int)(i - (unsigned)b * (unsigned)per_row);
  const int h = r / PH;
  const int c = (r - h * PH) << 3;

  const long n = context_lens[b];
  const long cap = (long)max_blocks * page_size;  // never index past the block table's row
  if (n <= 0 || n > cap || n > max_pos) return;
  const int p = (int)n - 1;
  const int pg = p / page_size;  // < max_blocks
  const int blk = block_table[(long)b * max_blocks + pg];
  if ((unsigned)blk >= (unsigned)num_blocks) return;  // not a block of this cache
  const long slot = (long)blk * page_size + (p - pg * page_size);

  bf16_t* base = qkv + (long)b * row_stride + (long)h * D;
  u32x4* lo = reinterpret_cast<u32x4*>(base + c);
  u32x4* hi = reinterpret_cast<u32x4*>(base + HALF + c);
  u32x4 xl = *lo, xh = *hi;
  if (h < Hq + Hk) {
    float a[8], bb[8], oa[8], ob[8];
    unpack8(xl, a);
    unpack8(xh, bb);
    rope_rotate8(a, bb, reinterpret_cast<const float4*>(cs + (long)p * HALF + c), 1.f, oa, ob);
    xl = pack8(oa);
    xh = pack8(ob);
    *lo = xl;
    *hi = xh;
    if (h < Hq) return;
  }
  const bool is_v = h >= Hq + Hk;
  const int hk = h - Hq - (is_v ? Hk : 0);
  const long at = (slot * Hk + hk) * D + c;  // element (= fp8 byte) index of chunk c in the cache
  if constexpr (!FP8) {
    bf16_t* dst = reinterpret_cast<bf16_t*>(is_v ? v_cache : k_cache) + at;
    *reinterpret_cast<u32x4*>(dst) = xl;
    *reinterpret_cast<u32x4*>(dst + HALF) = xh;
  } else {
    float x[16];
    unpack8(xl, x);
    unpack8(xh, x + 8);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) amax = fmaxf(amax, fabsf(x[j]));
#pragma unroll
    for (int off = 1; off < PH; off <<= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    // kv_cache_append_fp8_kernel's rule: the smallest power of two s with amax / s <= 448, biased
    // exponent clamped to [1, 254]; amax == 0: 1
    const unsigned bits = __float_as_uint(amax);
    int eb = (int)(bits >> 23) - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    eb = bits == 0u ? 127 : min(max(eb, 1), 254);
    const float inv = __uint_as_float((unsigned)(254 - eb) << 23);  // exact 1 / s
    int w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j] * inv, x[4 * j + 1] * inv, w[j], false);
      w[j] = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * j + 2] * inv, x[4 * j + 3] * inv, w[j], true);
    }
    fp8_t* dst = reinterpret_cast<fp8_t*>(is_v ? v_cache : k_cache) + at;
    *reinterpret_cast<uint2*>(dst) = uint2{(unsigned)w[0], (unsigned)w[1]};
    *reinterpret_cast<uint2*>(dst + HALF) = uint2{(unsigned)w[2], (unsigned)w[3]};
    if (c == 0) (is_v ? vsc : ksc)[slot * Hk + hk] = __uint_as_float((unsigned)eb << 23);
  }
}

}  // namespace

// qkv: [B, >= (Hq+2Hk)*D] bf16 with row stride `row_stride` elements (a multiple of 8), 16-B aligned;
// cs: [max_pos, D/2] float2 (cos, sin), 16-B aligned; block_table: int32 [B, max_blocks];
// context_lens: int32 [B], each sequence's length including this token; caches and scales: either
// kind (paged_kv.h). D is 64 or 128.
RCA_API int rca_rope_kv_append_decode(void* qkv, long long row_stride, const void* cs, int max_pos,
                                      const int* block_table, const int* context_lens, int max_blocks, void* k_cache,
                                      void* v_cache, void* k_scale, void* v_scale, int B, int Hq, int Hk, int D,
                                      int page_size, int num_blocks, hipStream_t stream) {
  if (B == 0) return 0;
  if (B < 0 || !paged_kv::heads_ok(Hq, Hk) || (D != 64 && D != 128) || max_pos <= 0) return -1;
  if (!paged_kv::rows_ok(row_stride, (long long)(Hq + 2 * Hk) * D)) return -1;
  if (!paged_kv::pages_ok(page_size, max_blocks, num_blocks)) return -1;
  const long long n = (long long)B * (Hq + 2 * Hk) * (D / 16);
  if (n >= (1LL << 31)) return -2;
  if (!paged_kv::all_set(qkv, cs, block_table, context_lens) || !paged_kv::aligned(16, qkv, cs)) return -3;
  if (!paged_kv::caches_ok(k_cache, v_cache, k_scale, v_scale)) return -3;
  auto launch = [&](auto fp8, auto d) {
    hipLaunchKernelGGL((rope_kv_append_decode_kernel<d.value, fp8.value>), dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, stream, (bf16_t*)qkv, (long)row_stride, (const float2*)cs, max_pos, block_table,
                       context_lens, max_blocks, page_size, num_blocks, k_cache, v_cache, (float*)k_scale,
                       (float*)v_scale, B, Hq, Hk);
    return (int)hipGetLastError();
  };
  // bf16 before fp8 and 64 before 128: the kernels are emitted in the order they are named here
  using paged_kv::int_c;
  if (!k_scale) return D == 64 ? launch(std::false_type{}, int_c<64>{}) : launch(std::false_type{}, int_c<128>{});
  return D == 64 ? launch(std::true_type{}, int_c<64>{}) : launch(std::true_type{}, int_c<128>{});
}
