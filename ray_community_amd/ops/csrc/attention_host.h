// Host side of the flash-attention kernels: the argument structs of one forward / backward call
// and the only declarations of the launchers that cross translation units. Kernel selection lives
// in attention.hip (Policy, launch_fwd, launch_bwd); a launcher declared here launches exactly the
// kernel it names, with the template arguments it is given.
#pragma once
#include "common.h"

struct AttnFwd {
  const bf16_t *q, *k, *v;
  bf16_t* o;
  float* lse;
  int B, S, Hq, Hk, D;
  long sq, sk, sv, so;  // token strides (elements)
  float scale, scale2;  // softmax scale; scale * log2(e)
  bool causal;
  hipStream_t st;
};

struct AttnBwd {
  const bf16_t *q, *k, *v, *o, *dout;
  const float* lse;
  float* delta;
  bf16_t *dq, *dk, *dv;
  int B, S, Hq, Hk, D;
  long sq, sk, sv, so, sdo, sdq, sdk, sdv;
  float scale, scale2;
  bool causal;
  hipStream_t st;
  bf16_t* ws;  // dS workspace of rca_attn_ds_ws_bytes, or nullptr: dQ recomputes S, P and dP
  long tiles;  // 32 x 32 dS tiles per (batch, query head)
};

// f(std::integral_constant<int, D>{}) for the two head sizes
template <typename F>
auto with_dim(int D, F&& f) {
  return D == 128 ? f(std::integral_constant<int, 128>{}) : f(std::integral_constant<int, 64>{});
}

// 64 query rows per wave, D = 128 and S % 256 == 0: compiler-scheduled (attention_fwd_wide.hip) and
// hand-scheduled with the deferred-rescale threshold thr in log2 units (attention_fwd_hs.hip)
void rca_attn_launch_fwd_wide(const AttnFwd& a);
void rca_attn_launch_fwd_hs(const AttnFwd& a, float thr);

// dK/dV (attention_dkdv.hip). _ds: the hand-scheduled kernel that also stores the dS tiles to a.ws,
// with s_nop operand nops (1 or 3) ahead of its asm MFMAs; _hs: hand-scheduled, K/V by LDS-DMA or
// register-staged; both D = 128. Plain: compiler-scheduled, nh (1 or 2) 32-row query slices in flight.
void rca_attn_launch_dkdv_ds(const AttnBwd& a, int nops);
void rca_attn_launch_dkdv_hs(const AttnBwd& a, bool dma);
void rca_attn_launch_dkdv(const AttnBwd& a, int nh);

// recompute-free dQ (attention_dq.hip): workspace bytes for a shape (0: none), delta = rowsum(dO * O),
// and dQ from the dS tiles with qw (1 or 2; 2 needs S % 256 == 0) query blocks per wave
long rca_attn_ds_ws_bytes(int B, int S, int Hq, int D, bool causal);
void rca_attn_launch_delta(const AttnBwd& a);
void rca_attn_launch_dq_ds(const AttnBwd& a, int qw);
