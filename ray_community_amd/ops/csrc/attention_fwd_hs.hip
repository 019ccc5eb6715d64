// Hand-scheduled flash-attention forward for gfx950 (D = 128; RCA_ATTN_FWD=hs).
//
// Geometry as attention_fwd_wide.hip: 4 waves x 64 query rows (two 32-row groups g) = 256 rows per
// workgroup, one wave per SIMD; Q^T fragments (64) and the O^T accumulators (128) live in the
// accumulator file, K/V tiles of 64 keys arrive by LDS-DMA (DmaStage image of attention_common.h).
// What differs is the schedule. The work of a 32-key half-tile u is QK(u) (16 MFMAs: S^T of both
// groups), a row max, the softmax exponentials, and PV(u) (16 MFMAs); the kernel runs it as a
// software pipeline of 16-MFMA phases in which every MFMA gap carries a fixed share of the OTHER
// half-tile's VALU / LDS work (MI355X_MICROARCH.md: one wave per SIMD hides about five single-issue
// instructions, one of them an 8-cycle transcendental, per 32-cycle MFMA gap):
//   A_u: QK(u)     || exp2 of S(u-1) (2 per gap), P(u-1) conversion, V(u-1) transposed reads
//   B_u: PV(u-1)   || row sums of P(u-1), row max of S(u) (+ causal mask), K(u+1) reads, then the
//                     deferred-rescale decision for u (applied after PV(u-1), THR = 8 as the
//                     32-row kernel)
// MFMAs are volatile inline asm separated by scheduling fences, so the compiler keeps the slot
// order; the MFMA -> VALU and VALU -> MFMA hazards that the asm hides from the hazard recognizer
// are covered by data-tied s_nop gaps at the phase boundaries (the same scheme as the hand-
// scheduled dK/dV kernel, attention_dkdv.hip).
// LDS: a 4-deep ring of K|V tiles (128 KB); tile j+3's DMA is spread over tile j's last three
// phases (after its barrier, buffer (j-1) mod 4 is free), so each tile has about two tiles of
// flight time and one barrier per tile (a 5-deep ring, 160 KB, measured the same).
// Measured (profiles/attn_fwd_hs_r4.md): 0.273-0.275 ms at the 8B shape, level with the 32-row
// kernel (0.271-0.292) -- opt-in. Waves whose causal rows end early keep joining the
// barriers and issuing their DMA share (the pipeline drains one tile after a wave's last).
#include "attention_common.h"
#include "attention_host.h"

#include <utility>

namespace {

__device__ __forceinline__ void hf_fence() { __builtin_amdgcn_sched_barrier(0); }
template <typename F, int... I>
__device__ __forceinline__ void hf_for_(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void hf_for(F&& f) {
  hf_for_(f, std::make_integer_sequence<int, N>{});
}
template <int OFF>
__device__ __forceinline__ bf16x8_t hf_rd(unsigned base) {
  static_assert(OFF < 65536, "ds offset field is 16 bits");
  s16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(base), "n"(OFF));
  return __builtin_bit_cast(bf16x8_t, v);
}
template <int OFF0, int OFF1>
__device__ __forceinline__ bf16x8_t hf_rdtr(unsigned b0, unsigned b1) {
  static_assert(OFF0 < 65536 && OFF1 < 65536, "ds offset field is 16 bits");
  s16x4 a, b;
  asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%4\n\tds_read_b64_tr_b16 %1, %3 offset:%5"
               : "=&v"(a), "=&v"(b)
               : "v"(b0), "v"(b1), "n"(OFF0), "n"(OFF1));
  s16x8 r = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8_t, r);
}
__device__ __forceinline__ void hf_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// one v_max3_f32 (no canonicalising v_max pair: the operands are past a hazard gap)
__device__ __forceinline__ float hf_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// S^T chain: K fragment (VGPRs) x Q^T fragment (accumulator registers); the first MFMA of a
// chain takes C = 0 instead of a zeroed register block
#define HF_MF0(acc, a, b) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "a"(b))
#define HF_MFK(acc, a, b) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(b))
// O^T += V^T P^T with O^T in accumulator registers
#define HF_MFA(acc, a, b) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b))
// >= 18 wait states between an XDL write and a VALU read of the result (and the reverse)
#define HF_GAP "s_nop 7\n\ts_nop 7\n\ts_nop 4"
// every lambda below is inlined: an outlined phase would pass the S / fragment arrays through scratch
#define HF_AI __attribute__((always_inline))

template <bool CAUSAL>
__global__ __launch_bounds__(kThreads, 1) void attn_fwd_hs_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    bf16_t* __restrict__ O, float* __restrict__ LSE, int B, int S, int Hq, int Hk, long sq, long sk, long sv,
    long so, float scale2, float THR) {
  constexpr int D = 128, BQ = 256, BK = 64, NKS = 8, NDB = 4, TILE = BK * D * 2, BUF = 2 * TILE, G8 = Img<D>::G8;
  __shared__ __attribute__((aligned(16))) char smem[4 * BUF];

  const int nqb = S / BQ, G = Hq / Hk;
  int bhk, item;
  xcd_group_map(blockIdx.x, B * Hk, G * nqb, bhk, item);
  const int qr = item / G, b = bhk / Hk, hk = bhk % Hk, hq = hk * G + item % G, bh = b * Hq + hq;
  const int qb = CAUSAL ? nqb - 1 - qr : qr;  // longest causal rows first
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the tile loops stay scalar
  const int q0 = qb * BQ, qw0 = q0 + 64 * w;  // group g rows: qw0 + 32 g + l32
  // per-lane LDS bases of buffer 0 (bases(j) adds the buffer offset)
  const unsigned sb = (unsigned)(__UINTPTR_TYPE__)smem;
  const unsigned uk0 = sb + Img<D>::row_base(l32, h, 0), uk1 = sb + Img<D>::row_base(l32, h, 1);
  const unsigned ut0 = sb + Img<D>::tr_base(lane, 0), ut1 = sb + Img<D>::tr_base(lane, 1);

  bf16x8_t qf[2][NKS];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const bf16_t* Qr = Q + ((long)b * S + qw0 + 32 * g + l32) * sq + (long)hq * D;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[g][ks] = gload8(Qr + 16 * ks + 8 * h);
  }
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) asm volatile("" : "+a"(qf[g][ks]));  // resident in accumulator registers

  f32x16 o[2][NDB];
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int i = 0; i < NDB; ++i) o[g][i] = zero16();
  asm volatile(HF_GAP : "+a"(o[0][0]), "+a"(o[0][1]), "+a"(o[0][2]), "+a"(o[0][3]), "+a"(o[1][0]), "+a"(o[1][1]),
               "+a"(o[1][2]), "+a"(o[1][3]));
  float m[2] = {-INFINITY, -INFINITY}, ls0[2] = {0.f, 0.f}, ls1[2] = {0.f, 0.f}, mx[2];
  bool dflag = false;  // tile 0 is this wave's diagonal tile

  const int ntile = CAUSAL ? (q0 + BQ) / BK : S / BK;       // this workgroup's K/V tiles
  const int ntw = CAUSAL ? qw0 / BK + 1 : ntile;            // this wave's (its last is diagonal)
  DmaStage<D, BK> kst, vst;
  kst.init(K + (long)b * S * sk + (long)hk * D, sk, S, tid);
  vst.init(V + (long)b * S * sv + (long)hk * D, sv, S, tid);
  // piece p (0-3 K, 4-7 V) of tile j3 into buffer j3 mod 4 (past the end the source row is
  // clamped: the last tile is re-fetched into a free buffer, so every wave issues 8 pieces per
  // tile and the vmcnt counts stay constant)
  auto dma_piece = [&](auto pc, int j3) HF_AI {
    constexpr int p = decltype(pc)::value;
    const int t = min(j3, ntile - 1);
    char* dst = smem + (j3 & 3) * BUF;
    if constexpr (p < 4) kst.issue_one(p, t * BK, sk, dst);
    else vst.issue_one(p - 4, t * BK, sv, dst + TILE);
  };

  f32x16 sa[2], sbv[2];  // S^T of even / odd half-tiles
  bf16x8_t kf[NKS], vf[2][NDB], pp[2][2];

  // per-lane read bases of buffer j mod 4 (immediates address inside a 32-KB buffer)
  struct Bases {
    unsigned k0, k1, t0, t1;
  };
  auto bases = [&](int j) HF_AI {
    const unsigned off = (unsigned)(j & 3) * BUF;
    return Bases{uk0 + off, uk1 + off, ut0 + off, ut1 + off};
  };
  // K fragment kk of half t; V^T fragment (st, db) of half t
  auto kread = [&](const Bases& bs, auto kkc, auto tc) HF_AI {
    constexpr int kk = decltype(kkc)::value, t = decltype(tc)::value;
    return hf_rd<4 * G8 * t + 512 * (kk >> 1)>((kk & 1) ? bs.k1 : bs.k0);
  };
  auto vread = [&](const Bases& bs, auto stc, auto dbc, auto tc) HF_AI {
    constexpr int st = decltype(stc)::value, db = decltype(dbc)::value;
    constexpr int ts = 2 * decltype(tc)::value + st;
    return hf_rdtr<TILE + G8 * (2 * ts) + 512 * db, TILE + G8 * (2 * ts + 1) + 512 * db>(bs.t0, bs.t1);
  };

  // A phase: QK of the current half (CUR) into sc || softmax exponentials + P conversion + V^T
  // reads (buffer vb, half TP) of the previous half (PREV, on sp) || DMA pieces P0 .. P0+NP-1
  auto phaseA = [&](auto curc, auto prevc, const Bases& vb, auto tpc, auto p0c, auto npc, f32x16(&sc)[2],
                    f32x16(&sp)[2], int dtile) HF_AI {
    constexpr bool CUR = decltype(curc)::value, PREV = decltype(prevc)::value;
    constexpr int P0 = decltype(p0c)::value, NP = decltype(npc)::value;
    const float nm0 = -m[0], nm1 = -m[1];
    hf_for<16>([&](auto ic) HF_AI {
      constexpr int i = decltype(ic)::value;
      hf_fence();
      if constexpr (CUR) {
        constexpr int kk = i >> 1, g = i & 1;
        if constexpr (kk == 0) HF_MF0(sc[g], kf[0], qf[g][0]);
        else HF_MFK(sc[g], kf[kk], qf[g][kk]);
      }
      hf_fence();
      if constexpr (PREV) {
        constexpr int gp = i >> 3, r = 2 * (i & 7);
        const float nm = gp ? nm1 : nm0;
        sp[gp][r] = fast_exp2(fmaf(sp[gp][r], scale2, nm));
        sp[gp][r + 1] = fast_exp2(fmaf(sp[gp][r + 1], scale2, nm));
        if constexpr (i == 4) pp[0][0] = acc_to_bf16(sp[0], 0);
        if constexpr (i == 12) pp[1][0] = acc_to_bf16(sp[1], 0);
        if constexpr (i < 8) vf[i >> 2][i & 3] = vread(vb, IC<(i >> 2)>{}, IC<(i & 3)>{}, tpc);
      }
      if constexpr (NP > 0 && i == 9) dma_piece(IC<P0>{}, dtile);
      if constexpr (NP > 1 && i == 13) dma_piece(IC<P0 + 1>{}, dtile);
    });
    hf_fence();
    hf_lgkm0();
    hf_fence();
    asm volatile(HF_GAP : "+v"(sc[0]), "+v"(sc[1]), "+v"(pp[0][0]), "+v"(pp[1][0]));
    hf_fence();
  };

  // B phase: PV of the previous half (PREV; P from sp) || row sums of sp, row max of sc (half T
  // of a diagonal tile: masked) and K reads of the next half (buffer kb, half TN) || DMA pieces;
  // then the rescale decision for the current half (CUR)
  auto phaseB = [&](auto curc, auto prevc, auto diagc, auto tc, const Bases& kb, auto tnc, auto p0c, auto npc,
                    f32x16(&sc)[2], f32x16(&sp)[2], int dtile) HF_AI {
    constexpr bool CUR = decltype(curc)::value, PREV = decltype(prevc)::value;
    constexpr int DIAG = decltype(diagc)::value;  // 0 none, 1 diagonal tile, 2 diagonal iff dflag
    constexpr int T = decltype(tc)::value, P0 = decltype(p0c)::value, NP = decltype(npc)::value;
    // key - row offset of element r in the diagonal tile: 32(T-g) + crow(r) + c4 (never > 0 off it)
    const int c4 = (DIAG == 2 && !dflag) ? -4096 : 4 * h - l32;
    hf_for<16>([&](auto ic) HF_AI {
      constexpr int i = decltype(ic)::value;
      hf_fence();
      if constexpr (PREV) {
        constexpr int st = i >> 3, g = (i >> 2) & 1, db = i & 3;
        HF_MFA(o[g][db], vf[st][db], pp[g][st]);
      }
      hf_fence();
      if constexpr (PREV) {
        if constexpr (i == 0) pp[0][1] = acc_to_bf16(sp[0], 1);
        if constexpr (i == 1) pp[1][1] = acc_to_bf16(sp[1], 1);
        constexpr int g = i >> 3, r = 2 * (i & 7);
        // compiler-visible adds: an inline-asm v_add_f32 here (to keep them out of v_pk_add_f32
        // pairs) gave wrong row sums on hardware (profiles/attn_fwd_hs_r4.md)
        ls0[g] += sp[g][r];
        ls1[g] += sp[g][r + 1];
      }
      if constexpr (CUR) {
        constexpr int g = i >> 3, k = i & 7, r = 2 * k;
        if constexpr (DIAG == 2) {
          constexpr int cr0 = 32 * (T - g) + (r & 3) + 8 * (r >> 2), cr1 = 32 * (T - g) + ((r + 1) & 3) + 8 * ((r + 1) >> 2);
          if constexpr (!(T == 0 && g == 1)) {
            sc[g][r] = cr0 + c4 > 0 ? -INFINITY : sc[g][r];
            sc[g][r + 1] = cr1 + c4 > 0 ? -INFINITY : sc[g][r + 1];
          }
        } else if constexpr (DIAG == 1) {
          constexpr int cr0 = 32 * (T - g) + (r & 3) + 8 * (r >> 2), cr1 = 32 * (T - g) + ((r + 1) & 3) + 8 * ((r + 1) >> 2);
          if constexpr (T == 1 && g == 0) {
            sc[g][r] = -INFINITY;
            sc[g][r + 1] = -INFINITY;
          } else if constexpr (!(T == 0 && g == 1)) {
            sc[g][r] = cr0 + c4 > 0 ? -INFINITY : sc[g][r];
            sc[g][r + 1] = cr1 + c4 > 0 ? -INFINITY : sc[g][r + 1];
          }
        }
        if constexpr (k == 0) mx[g] = hf_max3(sc[g][0], sc[g][1], sc[g][1]);
        else mx[g] = hf_max3(mx[g], sc[g][r], sc[g][r + 1]);
        if constexpr (i >= 2 && i < 2 + NKS) kf[i - 2] = kread(kb, IC<i - 2>{}, tnc);
      }
      if constexpr (NP > 0 && i == 10) dma_piece(IC<P0>{}, dtile);
      if constexpr (NP > 1 && i == 12) dma_piece(IC<P0 + 1>{}, dtile);
      if constexpr (NP > 2 && i == 14) dma_piece(IC<P0 + 2>{}, dtile);
    });
    hf_fence();
    hf_lgkm0();
    hf_fence();
    if constexpr (CUR) {
      const float mt0 = xhalf_max(mx[0]) * scale2, mt1 = xhalf_max(mx[1]) * scale2;
      if (__builtin_amdgcn_ballot_w64(mt0 > m[0] + THR || mt1 > m[1] + THR) != 0) {
        // after PV(prev): every P already exponentiated against the old max is in O and l
        asm volatile(HF_GAP : "+a"(o[0][0]), "+a"(o[0][1]), "+a"(o[0][2]), "+a"(o[0][3]), "+a"(o[1][0]),
                     "+a"(o[1][1]), "+a"(o[1][2]), "+a"(o[1][3]));
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const float mn = fmaxf(m[g], g ? mt1 : mt0);
          const float a = mn == -INFINITY ? 1.f : fast_exp2(m[g] - mn);
#pragma unroll
          for (int i = 0; i < NDB; ++i) {
            o[g][i] *= a;
            hf_fence();  // one accumulator block at a time through the VGPRs
          }
          ls0[g] *= a;
          ls1[g] *= a;
          m[g] = mn;
        }
        asm volatile(HF_GAP : "+a"(o[0][0]), "+a"(o[0][1]), "+a"(o[0][2]), "+a"(o[0][3]), "+a"(o[1][0]),
                     "+a"(o[1][1]), "+a"(o[1][2]), "+a"(o[1][3]));
      }
    }
    hf_fence();
  };

  auto sync_tile = [&]() HF_AI {  // tile j+1 landed for every wave; every wave is past tile j-1's reads
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __syncthreads();
  };
  using F = std::false_type;
  using Tr = std::true_type;
  // K/V tile j: A_2j, barrier, B_2j, A_2j+1, B_2j+1; tile j+3's DMA (into the buffer tile j-1
  // vacated at the barrier) spread over the last three phases
  auto active = [&](auto diagc, auto firstc, int j) HF_AI {
    constexpr bool FIRST = decltype(firstc)::value;
    using NF = std::integral_constant<bool, !FIRST>;
    const Bases cur = bases(j);
    phaseA(Tr{}, NF{}, bases(j - 1), IC<1>{}, IC<0>{}, IC<0>{}, sa, sbv, 0);
    sync_tile();
    phaseB(Tr{}, NF{}, diagc, IC<0>{}, cur, IC<1>{}, IC<0>{}, IC<3>{}, sa, sbv, j + 3);
    phaseA(Tr{}, Tr{}, cur, IC<0>{}, IC<3>{}, IC<2>{}, sbv, sa, j + 3);
    phaseB(Tr{}, Tr{}, diagc, IC<1>{}, bases(j + 1), IC<0>{}, IC<5>{}, IC<3>{}, sbv, sa, j + 3);
  };
  auto drain = [&](int j) HF_AI {  // the wave's last half-tile: softmax + PV only
    phaseA(F{}, Tr{}, bases(j - 1), IC<1>{}, IC<0>{}, IC<0>{}, sa, sbv, 0);
    sync_tile();
    phaseB(F{}, Tr{}, IC<0>{}, IC<0>{}, bases(j), IC<0>{}, IC<0>{}, IC<3>{}, sa, sbv, j + 3);
    hf_for<5>([&](auto pc) HF_AI { dma_piece(IC<3 + decltype(pc)::value>{}, j + 3); });
  };
  auto idle = [&](int j) HF_AI {
    sync_tile();
    hf_for<8>([&](auto pc) HF_AI { dma_piece(pc, j + 3); });
  };

  // prologue: tiles 0-2 in flight, tile 0 landed, K of half 0 in registers
  hf_for<8>([&](auto pc) HF_AI { dma_piece(pc, 0); });
  hf_for<8>([&](auto pc) HF_AI { dma_piece(pc, 1); });
  hf_for<8>([&](auto pc) HF_AI { dma_piece(pc, 2); });
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  __syncthreads();
  {
    const Bases b0 = bases(0);
    hf_for<NKS>([&](auto kkc) HF_AI { kf[decltype(kkc)::value] = kread(b0, kkc, IC<0>{}); });
  }
  hf_lgkm0();
  hf_fence();
  // tiles 0 .. ntw-1 active (the last one diagonal when causal), ntw drains, the rest idle: every
  // wave passes ntile + 1 barriers
  // tile 0 is the diagonal one only for the first 64 rows: one copy with a run-time mask (two
  // copies behind a branch made the register allocator split every live range at the join)
  dflag = CAUSAL && ntw == 1;
  active(IC<2>{}, Tr{}, 0);
  int j = 1;
  for (; j < ntw - 1; ++j) active(IC<0>{}, F{}, j);
  if (j == ntw - 1) active(IC<(CAUSAL ? 1 : 0)>{}, F{}, j++);
  drain(j++);
  for (; j <= ntile; ++j) idle(j);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA may land after the workgroup ends

  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int db = 0; db < NDB; ++db) asm volatile("" : "+a"(o[g][db]));
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int qrow = qw0 + 32 * g + l32;
    const float lt = xhalf_sum(ls0[g] + ls1[g]);
    const float inv = 1.f / lt;
    bf16_t* Or = O + ((long)b * S + qrow) * so + (long)hq * D;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        store4(Or + 32 * db + 8 * gg + 4 * h, o[g][db][4 * gg] * inv, o[g][db][4 * gg + 1] * inv,
               o[g][db][4 * gg + 2] * inv, o[g][db][4 * gg + 3] * inv);
      }
    }
    if (h == 0) LSE[(long)bh * S + qrow] = m[g] + __log2f(lt);
  }
}
#undef HF_MF0
#undef HF_MFK
#undef HF_MFA
#undef HF_GAP
#undef HF_AI

template __global__ void attn_fwd_hs_kernel<true>(const bf16_t* __restrict__, const bf16_t* __restrict__,
                                                  const bf16_t* __restrict__, bf16_t* __restrict__, float* __restrict__,
                                                  int, int, int, int, long, long, long, long, float, float);
template __global__ void attn_fwd_hs_kernel<false>(const bf16_t* __restrict__, const bf16_t* __restrict__,
                                                   const bf16_t* __restrict__, bf16_t* __restrict__, float* __restrict__,
                                                   int, int, int, int, long, long, long, long, float, float);

}  // namespace

void rca_attn_launch_fwd_hs(const AttnFwd& a, float thr) {
  with_bool(a.causal, [&](auto c) {
    hipLaunchKernelGGL((attn_fwd_hs_kernel<decltype(c)::value>), dim3(a.B * a.Hq * (a.S / 256)), dim3(kThreads), 0,
                       a.st, a.q, a.k, a.v, a.o, a.lse, a.B, a.S, a.Hq, a.Hk, a.sq, a.sk, a.sv, a.so, a.scale2, thr);
  });
}
