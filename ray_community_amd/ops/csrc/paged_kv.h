// Host side of the paged KV ops (cache append, fused RoPE + append, paged decode and extend
// attention): the argument checks their entry points share, the (D, G) dispatch, and the launchers
// an entry point reaches in the other cache kind's translation unit. No device code.
//
// The cache kind is what the scale pointers say: both null is the bf16 cache ([num_blocks,
// page_size, Hk, D] bf16, 16-B aligned), both set the e4m3 cache (the same layout in bytes, 8-B
// aligned, with fp32 scales [num_blocks, page_size, Hk]); one of the two is an error.
//
// Return codes of every entry point: 0 launched (or nothing to do), -1 bad shape, -2 exceeds a
// grid or index limit, -3 pointer or alignment, otherwise the hipError_t of the launch. An entry
// point checks in that order, its own rules next to the shared ones, and launches nothing unless
// all hold. The "nothing to do" exits (no row, no token, a cache of no slots) come before every
// check and return 0 whatever the other arguments are.
#pragma once
#include "common.h"

namespace paged_kv {

template <typename... P>
bool all_set(P... p) {
  return (... && (p != nullptr));
}

template <typename... P>
bool aligned(uintptr_t bytes, P... p) {  // null counts as aligned
  return ((... | (uintptr_t)p) & (bytes - 1)) == 0;
}

// -1 unless: GQA heads
inline bool heads_ok(int Hq, int Hk) { return Hq > 0 && Hk > 0 && Hq % Hk == 0; }

// -1 unless: a 16-token group of a kernel's key loop never straddles a page
inline bool pages_ok(int page_size, int max_blocks, int num_blocks) {
  return page_size > 0 && !(page_size & 15) && max_blocks > 0 && num_blocks > 0;
}

// -1 unless: rows of `width` bf16 elements read from a 2-D tensor by 16-B chunks
inline bool rows_ok(long long row_stride, long long width) { return row_stride >= width && !(row_stride & 7); }

// -1 unless: what the paged attention kernels are instantiated for
inline bool attn_shape_ok(int B, int Hq, int Hk, int D, long long q_stride, int page_size, int max_blocks,
                          int num_blocks, int num_splits) {
  return B >= 0 && heads_ok(Hq, Hk) && (D == 64 || D == 128) && pages_ok(page_size, max_blocks, num_blocks) &&
         rows_ok(q_stride, (long long)Hq * D) && num_splits >= 1;
}

// -2 unless: B and Hk are grid dimensions y and z
inline bool grid_ok(int B, int Hk) { return B <= 65535 && Hk <= 65535; }

// -3 unless: both caches, aligned for their kind, and the scales given together
inline bool caches_ok(const void* k_cache, const void* v_cache, const void* k_scale, const void* v_scale) {
  return all_set(k_cache, v_cache) && !k_scale == !v_scale && aligned(k_scale ? 8 : 16, k_cache, v_cache) &&
         aligned(4, k_scale, v_scale);
}

// -3 unless: the attention ops' other pointers; the split workspaces only when they are used
inline bool attn_ptrs_ok(const void* q, const void* out, const int* block_table, const int* context_lens,
                         const void* part_o, const void* part_ml, int num_splits) {
  return all_set(q, out, block_table, context_lens) && aligned(16, q, out) &&
         (num_splits == 1 || (all_set(part_o, part_ml) && aligned(16, part_o, part_ml)));
}

constexpr float kLog2e = 1.44269504088896340736f;  // the kernels' softmax is base 2

// Host dispatch: run-time D in {64, 128} and G in {1, 2, 4, 8} -> compile-time ones. f receives
// std::integral_constant values (use ``d.value`` / ``g.value`` as template arguments) and returns
// int; -1 for a G no kernel is instantiated for. The caller has checked D.
template <int N>
using int_c = std::integral_constant<int, N>;

template <typename F>
int dispatch_dg(int D, int G, F&& f) {
  auto with_d = [&](auto d) {
    switch (G) {
      case 1: return f(d, int_c<1>{});
      case 2: return f(d, int_c<2>{});
      case 4: return f(d, int_c<4>{});
      case 8: return f(d, int_c<8>{});
    }
    return -1;
  };
  return D == 128 ? with_d(int_c<128>{}) : with_d(int_c<64>{});
}

}  // namespace paged_kv

// One launcher per op and cache kind, defined next to its kernels (attention_decode.hip and
// attention_extend.hip: bf16; the _fp8 files: e4m3) and called by the op's entry point with checked
// arguments. The two kinds of an op share a signature, so the entry point picks a function and
// writes the arguments once; the bf16 launchers ignore the scales.
#define RCA_LOCAL __attribute__((visibility("hidden")))

using kv_append_launcher = int(const void* qkv, long long row_stride, const int* slot_mapping, void* k_cache,
                               void* v_cache, void* k_scale, void* v_scale, long long T, int Hq, int Hk, int D,
                               long long num_slots, unsigned blocks, hipStream_t stream);
RCA_LOCAL kv_append_launcher launch_kv_append_bf16, launch_kv_append_fp8;

// the kernel over num_splits splits, then the merge of the partials when num_splits > 1
using attn_decode_launcher = int(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                                 const void* k_scale, const void* v_scale, const int* block_table,
                                 const int* context_lens, void* out, void* part_o, void* part_ml, int B, int Hq,
                                 int Hk, int D, int page_size, int max_blocks, int num_blocks, float scale,
                                 int num_splits, hipStream_t stream);
RCA_LOCAL attn_decode_launcher launch_attn_decode_bf16, launch_attn_decode_fp8;

// the same for the extend; `tiles` is the grid's x dimension, T is read only when num_splits > 1
using attn_extend_launcher = int(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                                 const void* k_scale, const void* v_scale, const int* block_table,
                                 const int* context_lens, const int* cu_q_lens, void* out, void* part_o,
                                 void* part_ml, int B, long long T, int max_q_len, int Hq, int Hk, int D,
                                 int page_size, int max_blocks, int num_blocks, float scale, int num_splits,
                                 unsigned tiles, hipStream_t stream);
RCA_LOCAL attn_extend_launcher launch_attn_extend_bf16, launch_attn_extend_fp8;
