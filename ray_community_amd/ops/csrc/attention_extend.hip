// Extend attention for gfx950: causal attention of a ragged batch of query chunks over a paged
// bf16 KV cache, each chunk sitting at the END of its sequence's context (chunked prefill, a
// continued turn, draft tokens to verify). The prefill-side counterpart of
// attn_decode_paged_kernel (attention_decode.hip); compute-bound, so it runs on
// v_mfma_f32_32x32x16_bf16 like attn_fwd_kernel (attention.hip), whose tile body it follows.
//
// Cache layout as in attention_decode.hip: k_cache, v_cache = bf16 [num_blocks, page_size, Hk, D].
// Sequence b owns query rows cu_q_lens[b] .. cu_q_lens[b+1]-1 of the packed q ([T, Hq*D], or the
// fused qkv row through q_stride); context_lens[b] counts its cached tokens INCLUDING these n_b new
// ones (their K/V were appended before the call), so query i sits at position
// p = context_lens[b] - n_b + i and attends keys 0..p.
//
// One workgroup = 4 waves = 128 "rows" of one kv head of one sequence, a row being a
// (query token, group head) pair: row r -> token r / G, head hk*G + r % G. Packing the GQA group
// into the row dimension fills the MFMA rows of a short chunk (16 tokens at G = 8 are a full
// tile) and stages every K/V byte once per group; the causal position depends on r / G only.
// Swapped product S^T = K.Q^T puts one row on each lane (row max/sum lane-local + one cross-half
// shuffle) and makes the S^T accumulator the B operand of O^T += V^T.P^T; V^T fragments come from
// ds_read_b64_tr_b16. Q lives in VGPRs; K/V tiles of 64 keys are register-staged (global loads
// before the tile's MFMAs, LDS writes after them) into a 2-deep ring of Img<D> images. A tile is
// four 16-key groups; page_size % 16 == 0 puts each group inside one page, so staging costs one
// wave-uniform block_table lookup per group and a 64-key tile may straddle pages (page 48).
// Base-2 online softmax with the forward's deferred, wave-uniform rescale.
//
// Masking is by loop bounds, by not loading, and by select:
//  * the key loop of a row tile ends at the tile's largest position + 1, and a wave skips the
//    tiles past its own largest position;
//  * a key at position >= context_lens[b] is never loaded: its LDS rows (K and V) are written as
//    zeros (0 * NaN inside an MFMA would be NaN), and every such key is > p for every row;
//  * block_table[b, j] is read only for j < ceil(context_lens[b] / page_size);
//  * a table entry outside [0, num_blocks) is "not a block of this cache", as in the decode
//    kernel: its keys are not read and take no part in the softmax (scores selected to -inf);
//  * inside a tile, key > p is a select to -inf, and a row that has seen nothing yet (m = -inf)
//    subtracts a zero reference, so exp2(-inf + inf) never happens. Rows past n_b*G load q as
//    zeros, sit at position -1 (everything masked: they never vote for a rescale) and are never
//    stored.
// Why no global read leaves the buffers: a K/V address is (blk * page_size + off + j) * Hk * D +
// hk * D + c with 0 <= blk < num_blocks checked, off + j < page_size (off is a multiple of 16,
// j < 16) and c < D; the table index is < ceil(ctx / page_size) <= max_blocks because ctx is
// clamped to max_blocks * page_size; q rows are cu_q_lens[b] + tok with tok < n_b <= max_q_len
// (cu_q_lens itself is the caller's contract: non-decreasing, cu_q_lens[B] <= T).
//
// Split-KV (SPLIT = true; a few rows over a long context, e.g. draft tokens to verify): the grid's
// x dimension is row tile * num_splits + split, and workgroup (row tile, split, hk, b) runs only
// key tiles [split * tps, min((split + 1) * tps, ntile)) of its row tile, ntile being that row
// tile's own causal bound and tps = ceil(ntile / num_splits). The range is a sub-range of
// [0, ntile), and every rule above is stated per key tile (what is loaded, which table entry is
// read, which scores are selected away), so each holds unchanged inside a split and the proof that
// no global read leaves the buffers needs no new case: a split only visits fewer of the same
// tiles. The first tile of the range is staged where the unsplit kernel stages tile 0, and the ring
// buffer of a tile is its index relative to the range's start. Instead of the normalised bf16 row a
// split stores, per (token, query head), the unnormalised fp32 O row and (m, l) into the decode
// path's workspace layout (part_o fp32 [T, Hq, num_splits, D], part_ml fp32 [T, Hq, num_splits, 2]);
// m is the base-2 scaled reference that O and l were accumulated against, which with the deferred
// rescale may lie up to THR below the true maximum: the merge is exact for any consistent triple.
// A split with no visible key for a row (an empty tile range, a row whose position lies before
// the split's first key, a wave that skipped all its tiles) has m = -inf, l = 0 and stores only
// that pair: attn_decode_combine_kernel (attention_combine.h) skips such a split without reading its
// O row. Rows past n_b*G are not stored at all, as in the unsplit kernel. The workspace addresses
// are the out address's (q0 + tok, hq) with the split index inside, so they stay inside
// [T, Hq, num_splits, *] under the same cu_q_lens contract.
//
// The entry point at the end, rca_attn_extend_paged, serves both cache kinds: the e4m3 kernel and
// its launcher are in attention_extend_fp8.hip (paged_kv.h).
#include "attention_combine.h"
#include "attention_common.h"
#include "paged_kv.h"

namespace {

template <int D, int G, bool SPLIT>
__global__ __launch_bounds__(kThreads, 2) void attn_extend_paged_kernel(
    const bf16_t* __restrict__ q, long q_stride, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
    const int* __restrict__ block_table, const int* __restrict__ context_lens, const int* __restrict__ cu_q_lens,
    bf16_t* __restrict__ out, int max_q_len, int Hk, int page, int max_blocks, int num_blocks, float scale2,
    float* __restrict__ part_o, float* __restrict__ part_ml, int num_splits) {
  constexpr int BQ = 128, BK = 64, NKS = D / 16, NDB = D / 32, TILE = BK * D * 2, G8 = Img<D>::G8;
  constexpr int NCH = D / 8, N = BK * NCH / kThreads, RPI = kThreads / NCH;  // staging: Stage<D, BK>'s split
  constexpr float THR = 8.f;
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE];

  const int b = blockIdx.z, hk = blockIdx.y;
  const int split = SPLIT ? (int)(blockIdx.x % (unsigned)num_splits) : 0;
  const int r0 = (SPLIT ? (int)(blockIdx.x / (unsigned)num_splits) : (int)blockIdx.x) * BQ;
  const int q0 = cu_q_lens[b];
  int nq = cu_q_lens[b + 1] - q0;
  nq = nq < 0 ? 0 : (nq > max_q_len ? max_q_len : nq);
  const int rows = nq * G;
  if (r0 >= rows) return;  // whole workgroup: tiles past this sequence's rows

  const long ctx_l = context_lens[b];
  const long cap = (long)max_blocks * page;  // never index past the block table's row
  const int ctx = (int)(ctx_l < 0 ? 0 : (ctx_l > cap ? cap : ctx_l));
  const int prior = ctx - nq;  // position of the chunk's first token (< 0: rows before 0 see nothing)

  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rw0 = r0 + 32 * w, row = rw0 + l32;
  const bool valid = row < rows;
  const int tok = row / G, hq = hk * G + row % G;
  const int pos = valid ? prior + tok : -1;
  // wave-uniform: any of the 32 rows live, largest position of the live rows
  const bool w_live = rw0 < rows;
  const int pmax_w = prior + min(rw0 + 31, rows - 1) / G;
  const int kend = prior + min(r0 + BQ - 1, rows - 1) / G + 1;  // the tile's largest position + 1
  const int ntile = kend > 0 ? (kend + BK - 1) / BK : 0;
  // this workgroup's key tiles [it0, it1): all of them, or its split's share (possibly none)
  const int tps = SPLIT ? (ntile + num_splits - 1) / num_splits : ntile;
  const int it0 = SPLIT ? min(split * tps, ntile) : 0;
  const int it1 = SPLIT ? min(it0 + tps, ntile) : ntile;

  const int rb0 = Img<D>::row_base(l32, h, 0), rb1 = Img<D>::row_base(l32, h, 1);
  const int tb0 = Img<D>::tr_base(lane, 0), tb1 = Img<D>::tr_base(lane, 1);

  bf16x8_t qf[NKS];
  if (valid) {
    const bf16_t* Qr = q + (long)(q0 + tok) * q_stride + (long)hq * D;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = gload8(Qr + 16 * ks + 8 * h);
  } else {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = __builtin_bit_cast(bf16x8_t, u32x4{0u, 0u, 0u, 0u});
  }
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) settle(qf[ks]);

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = zero16();
  float m = -INFINITY, lsum = 0.f;

  // staging thread -> (row, chunk) of Stage<D, BK>: conflict-free ds_write_b128 into the image
  constexpr int LG = NCH == 16 ? 2 : 1;  // log2(NCH / 4)
  const int sch = (tid & 3) | (((tid >> 3) & ((NCH >> 2) - 1)) << 2);
  const int srow = ((tid >> 2) & 1) | ((tid >> (3 + LG)) << 1);  // 0 .. RPI-1; srow >> 4 is wave-uniform
  const int loff = Img<D>::off(srow, sch);
  const long tok_stride = (long)Hk * D;  // elements between consecutive slots
  const int voff = (int)((srow & 15) * tok_stride * 2) + sch * 16;  // bytes, inside one 16-slot group
  const int sgrp = __builtin_amdgcn_readfirstlane(srow >> 4);  // D = 64: which of an iteration's two groups
  const int* bt = block_table + (long)b * max_blocks;
  u32x4 kr[N], vr[N];
  int dead_cur = 0, dead_nxt = 0;  // bit g: 16-key group g of the tile has an out-of-range table entry

  auto stage_load = [&](int kb) {
    int base[4], dead = 0;  // first slot of each 16-key group, -1 = nothing to read
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int key0 = kb + 16 * g4;
      int sb = -1;
      if (key0 < ctx) {
        const int pg = key0 / page;
        const int blk = bt[pg];
        if ((unsigned)blk < (unsigned)num_blocks) sb = blk * page + (key0 - pg * page);
        else dead |= 1 << g4;
      }
      base[g4] = sb;
    }
    dead_nxt = dead;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      // one buffer descriptor per 16-key group (wave-uniform: sgrp is): it spans the group's live
      // slots only, so a lane on a dead slot, or on a group with nothing to read (0 records),
      // gets zeros from the bounds check without touching memory
      const int gi = RPI == 16 ? i : 2 * i + sgrp;
      const int sb = __builtin_amdgcn_readfirstlane(RPI == 16 ? base[i] : (sgrp ? base[2 * i + 1] : base[2 * i]));
      const int live = min(16, ctx - (kb + 16 * gi));
      const bool any = sb >= 0 && live > 0;
      const long a = any ? (long)sb * tok_stride + (long)hk * D : 0;
      const int nrec = any ? (int)(((live - 1) * tok_stride + D) * 2) : 0;
      const auto rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(kc + a), (short)0, nrec, 0x00020000);
      const auto rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(vc + a), (short)0, nrec, 0x00020000);
      kr[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, voff, 0, 0));
      vr[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rv, voff, 0, 0));
    }
  };
  auto stage_store = [&](char* dst) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      *reinterpret_cast<u32x4*>(dst + loff + i * (RPI / 8) * G8) = kr[i];
      *reinterpret_cast<u32x4*>(dst + TILE + loff + i * (RPI / 8) * G8) = vr[i];
    }
  };

  if (it0 < it1) {
    stage_load(it0 * BK);
    dead_cur = dead_nxt;
    stage_store(smem);
  }
  __syncthreads();

  auto tile = [&](auto bufc, int it) {
    constexpr int buf = decltype(bufc)::value;
    const char* Ks = smem + buf * 2 * TILE;
    const char* Vs = Ks + TILE;
    const int kb = it * BK;
    const bool more = it + 1 < it1;
    if (more) stage_load(kb + BK);
    if (w_live && kb <= pmax_w) {
      auto qk = [&](int t) {
        bf16x8_t fr[NKS];
#pragma unroll
        for (int kk = 0; kk < NKS; ++kk) fr[kk] = lds_b128(Ks + ((kk & 1) ? rb1 : rb0) + 4 * G8 * t + 512 * (kk >> 1));
        f32x16 sx = zero16();
#pragma unroll
        for (int kk = 0; kk < NKS; ++kk) sx = mfma32(fr[kk], qf[kk], sx);
        // register r holds key kb + 32 t + 4 h + (r & 3) + 8 (r >> 2), of 16-key group 2 t + (r >> 3):
        // visible iff that offset is <= lim (a dead group: never)
        const int lim = pos - kb - 32 * t - 4 * h;
        const int lim0 = (dead_cur >> (2 * t)) & 1 ? -1 : lim, lim1 = (dead_cur >> (2 * t + 1)) & 1 ? -1 : lim;
#pragma unroll
        for (int r = 0; r < 16; ++r) sx[r] = (r & 3) + 8 * (r >> 2) > (r < 8 ? lim0 : lim1) ? -INFINITY : sx[r];
        return sx;
      };
      // deferred, wave-uniform rescale; a row with nothing visible (padded, or masked so far) has
      // mts = m = -inf and does not vote
      auto rescale = [&](float mt_raw) {
        const float mts = mt_raw * scale2;
        if (__builtin_amdgcn_ballot_w64(mts > m + THR) != 0) {
          const float mn = fmaxf(m, mts);
          const float a = mn == -INFINITY ? 1.f : fast_exp2(m - mn);
#pragma unroll
          for (int i = 0; i < NDB; ++i) o[i] *= a;
          lsum *= a;
          m = mn;
        }
      };
      auto softmax = [&](f32x16& sx, bf16x8_t& p0, bf16x8_t& p1) {
        const float nm = m == -INFINITY ? 0.f : -m;  // zero reference: exp2(-inf - 0) = 0
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          sx[r] = fast_exp2(fmaf(sx[r], scale2, nm));
          sx[r + 1] = fast_exp2(fmaf(sx[r + 1], scale2, nm));
          a0 += sx[r];
          a1 += sx[r + 1];
        }
        lsum += a0 + a1;
        p0 = acc_to_bf16(sx, 0);
        p1 = acc_to_bf16(sx, 1);
      };
      auto pv = [&](int t, bf16x8_t p0, bf16x8_t p1) {
        bf16x8_t fr[2 * NDB];
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
          for (int db = 0; db < NDB; ++db) {
            const int ts = 2 * t + st;
            fr[st * NDB + db] =
                lds_tr8(Vs + tb0 + G8 * (2 * ts) + 512 * db, Vs + tb1 + G8 * (2 * ts + 1) + 512 * db);
          }
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] = mfma32(fr[db], p0, o[db]);
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] = mfma32(fr[NDB + db], p1, o[db]);
      };
      // Every tile takes the masked body. A second, unmasked instantiation for the tiles below the
      // wave's smallest position (the forward's split) made hipcc spill ~70 VGPRs at D = 128 under
      // the 2-workgroups-per-CU register budget; the selects cost 32 VALU ops per tile and wave.
      {
        f32x16 s0 = qk(0);
        rescale(xhalf_max(max16(s0, -INFINITY)));
        f32x16 s1 = qk(1);
        bf16x8_t p00, p01;
        softmax(s0, p00, p01);
        const float mt1 = xhalf_max(max16(s1, -INFINITY));
        pv(0, p00, p01);
        rescale(mt1);
        bf16x8_t p10, p11;
        softmax(s1, p10, p11);
        pv(1, p10, p11);
      }
    }
    if (more) {
      stage_store(smem + (buf ^ 1) * 2 * TILE);
      dead_cur = dead_nxt;
    }
    __syncthreads();
  };
  for (int it = it0; it < it1; it += 2) {
    tile(IC<0>{}, it);
    if (it + 1 < it1) tile(IC<1>{}, it + 1);
  }

  const float lt = xhalf_sum(lsum);
  if (!valid) return;
  if constexpr (SPLIT) {
    // m is the same in both halves of a row (every rescale takes the cross-half maximum)
    const long prow = ((long)(q0 + tok) * ((long)Hk * G) + hq) * num_splits + split;
    if (h == 0) *reinterpret_cast<float2*>(part_ml + prow * 2) = float2{m, lt};  // nothing seen: (-inf, 0)
    if (m == -INFINITY) return;  // the combine skips this split without reading its O row
    float* Pr = part_o + prow * D;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4*>(Pr + 32 * db + 8 * g + 4 * h) =
            f32x4{o[db][4 * g], o[db][4 * g + 1], o[db][4 * g + 2], o[db][4 * g + 3]};
    }
    return;
  }
  const float inv = lt > 0.f ? 1.f / lt : 0.f;  // nothing visible (position < 0): zeros
  bf16_t* Or = out + (long)(q0 + tok) * ((long)Hk * G * D) + (long)hq * D;
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      store4(Or + 32 * db + 8 * g + 4 * h, o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv,
             o[db][4 * g + 3] * inv);
    }
  }
}

// Explicit instantiations for every (D, G) the launcher selects (see attention.hip: hipcc has
// dropped the host stub of a kernel template instantiated only through its launcher).
#define RCA_EXT_INST1(DD, GG, SS)                                                                                   \
  template __global__ void attn_extend_paged_kernel<DD, GG, SS>(                                                    \
      const bf16_t* __restrict__, long, const bf16_t* __restrict__, const bf16_t* __restrict__,                     \
      const int* __restrict__, const int* __restrict__, const int* __restrict__, bf16_t* __restrict__, int, int, int, \
      int, int, float, float* __restrict__, float* __restrict__, int);
#define RCA_EXT_INST(DD, GG) RCA_EXT_INST1(DD, GG, false) RCA_EXT_INST1(DD, GG, true)
RCA_EXT_INST(64, 1)
RCA_EXT_INST(64, 2)
RCA_EXT_INST(64, 4)
RCA_EXT_INST(64, 8)
RCA_EXT_INST(128, 1)
RCA_EXT_INST(128, 2)
RCA_EXT_INST(128, 4)
RCA_EXT_INST(128, 8)
#undef RCA_EXT_INST
#undef RCA_EXT_INST1

}  // namespace

// Default split count of the paged extend. The unsplit grid is row_tiles * Hk * B workgroups
// (row_tiles = ceil(max_q_len * G / 128)), each walking its row tile's key tiles (64 keys) serially.
// Heuristic:
//   * aim for >= kExtWant workgroups;
//   * a split walks at least kExtMinTiles key tiles (below that the partial-result write and the
//     combine pass cost more than they spread);
//   * at most 16 splits (the combine reads num_splits partials per output row);
//   * 1 when the unsplit grid already reaches kExtWant workgroups (chunked prefill of a batch).
// page_size takes no part: key tiles are 64 keys whatever the page. Measured values and the sweep
// behind them: profiles/speculative_decoding.md.
RCA_API int rca_attn_extend_num_splits(int B, int Hk, int max_q_len, int G, int max_context, int page_size) {
  constexpr long kExtWant = 512, kExtMinTiles = 4;
  (void)page_size;
  if (B <= 0 || Hk <= 0 || max_q_len <= 0 || G <= 0 || max_context <= 0) return 1;
  const long base = (((long)max_q_len * G + 127) / 128) * Hk * B;
  const long want = (kExtWant + base - 1) / base;
  const long by_work = (((long)max_context + 63) / 64) / kExtMinTiles;
  long n = want < by_work ? want : by_work;
  if (n > 16) n = 16;
  if (n < 1) n = 1;
  return (int)n;
}

int launch_attn_extend_bf16(const void* q, long long q_stride, const void* k_cache, const void* v_cache, const void*,
                            const void*, const int* block_table, const int* context_lens, const int* cu_q_lens,
                            void* out, void* part_o, void* part_ml, int B, long long T, int max_q_len, int Hq, int Hk,
                            int D, int page_size, int max_blocks, int num_blocks, float scale, int num_splits,
                            unsigned tiles, hipStream_t stream) {
  const int rc = with_bool(num_splits > 1, [&](auto split) {
    return paged_kv::dispatch_dg(D, Hq / Hk, [&](auto d, auto g) {
      hipLaunchKernelGGL((attn_extend_paged_kernel<d.value, g.value, split.value>), dim3(tiles, Hk, B),
                         dim3(kThreads), 0, stream, (const bf16_t*)q, (long)q_stride, (const bf16_t*)k_cache,
                         (const bf16_t*)v_cache, block_table, context_lens, cu_q_lens, (bf16_t*)out, max_q_len, Hk,
                         page_size, max_blocks, num_blocks, scale * paged_kv::kLog2e, (float*)part_o, (float*)part_ml,
                         num_splits);
      return (int)hipGetLastError();
    });
  });
  if (rc != 0 || num_splits == 1 || T == 0) return rc;
  return launch_split_combine((const float*)part_o, (const float*)part_ml, (bf16_t*)out, (long)T * Hq, num_splits, D,
                              stream);
}

// q: packed query rows, row t at q + t*q_stride (+ h*D per head; q_stride in elements: Hq*D for a
// contiguous q, (Hq+2Hk)*D to read it in place from the fused qkv row). cu_q_lens: int32 [B+1],
// non-decreasing, cu_q_lens[B] <= T = rows of q and out; max_q_len >= every chunk length (host side:
// it sizes the grid). context_lens counts each sequence's cached tokens including its chunk. Caches
// and scales: either kind (paged_kv.h). out: bf16 [T, Hq*D]. scale must be > 0.
//
// num_splits == 1 is the unsplit launch: no workspace, T unread, rows of out that no sequence owns
// not written. num_splits > 1 runs that many splits of every row tile's keys, merged in split order
// (deterministic, no atomics); it needs part_o (fp32 [T, Hq, num_splits, D]) and part_ml (fp32
// [T, Hq, num_splits, 2] = (m, l)), and then rows of out that no sequence owns are written with
// whatever the workspace held.
RCA_API int rca_attn_extend_paged(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                                  const void* k_scale, const void* v_scale, const int* block_table,
                                  const int* context_lens, const int* cu_q_lens, void* out, void* part_o,
                                  void* part_ml, int B, long long T, int max_q_len, int Hq, int Hk, int D,
                                  int page_size, int max_blocks, int num_blocks, float scale, int num_splits,
                                  hipStream_t stream) {
  if (B == 0 || max_q_len == 0) return 0;
  if (!paged_kv::attn_shape_ok(B, Hq, Hk, D, q_stride, page_size, max_blocks, num_blocks, num_splits)) return -1;
  if (max_q_len < 0 || !(scale > 0.f) || (num_splits > 1 && T < 0)) return -1;
  const long long tiles = ((long long)max_q_len * (Hq / Hk) + 127) / 128 * num_splits;
  if (!paged_kv::grid_ok(B, Hk) || tiles >= (1LL << 31)) return -2;
  if ((long long)num_blocks * page_size >= (1LL << 31)) return -2;  // the kernels' slot index is an int
  if (!paged_kv::caches_ok(k_cache, v_cache, k_scale, v_scale) || !cu_q_lens) return -3;
  if (!paged_kv::attn_ptrs_ok(q, out, block_table, context_lens, part_o, part_ml, num_splits)) return -3;
  return (k_scale ? launch_attn_extend_fp8 : launch_attn_extend_bf16)(
      q, q_stride, k_cache, v_cache, k_scale, v_scale, block_table, context_lens, cu_q_lens, out, part_o, part_ml, B, T,
      max_q_len, Hq, Hk, D, page_size, max_blocks, num_blocks, scale, num_splits, (unsigned)tiles, stream);
}
