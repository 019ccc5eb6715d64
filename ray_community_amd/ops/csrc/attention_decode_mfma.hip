// Single-token (decode) attention over a paged KV cache on the matrix unit, for wide GQA groups
// (G = Hq / Hk <= 16; exposed for G = 8 and 16), bf16 and e4m3 caches, gfx950.
//
// attn_decode_paged_kernel (attention_decode.hip) keeps G x 8 fp32 accumulators per lane and spends
// 2 * D * G VALU FMAs per key: VALU-bound at G = 8, impossible at G = 16. Here the G query heads of
// one kv head are the 16 columns of v_mfma_f32_16x16x32_bf16 (heads >= G: q loaded as zeros, never
// stored), so a key costs the wave a few MFMAs whatever G is and decode is a K/V stream again.
//
// Grid, splits, workspaces and the merge across splits are the VALU kernel's: grid (num_splits, Hk,
// B), 4 waves per workgroup, split s owns pages [s * pps, (s + 1) * pps) of the sequence's own
// ceil(ctx / page) pages, part_o fp32 [B, Hq, num_splits, D] and part_ml fp32 [B, Hq, num_splits, 2]
// merged by attn_decode_combine_kernel in split order. No atomics. A split's tokens are cut into
// steps of 32 consecutive keys; wave w takes steps w, w + 4, ... (with page 32 exactly the VALU
// kernel's page-per-wave deal; with other pages a step may straddle two pages, so the block table is
// read per 16-key tile: page % 16 == 0 keeps a tile inside one page).
//
// One step of one wave (lane = 16 c + r):
//   scores  S^T[key][head] = K Q^T as two 16-key x 16-head tiles of D / 32 MFMAs each. K is the row
//           operand, loaded global -> VGPR by 16-byte loads straight into the fragment: lane (r, c)
//           holds elements 32 ks + 8 c .. + 7 of key r (no LDS on the K side). Q is the column
//           operand, D / 32 fragments per lane loaded once (lane % 16 = head). The fp32 scores are
//           multiplied by scale * log2(e); q itself is not touched.
//   softmax In the accumulator layout a lane holds keys 4 c .. 4 c + 3 of both tiles for head r: the
//           step's maximum is lane-local over 8 values plus two shuffles (xor 16, xor 32); base-2
//           online softmax, a zero reference while nothing has been seen (safe_ref). The running sum
//           stays a per-lane partial until the epilogue.
//   PV      O^T[d][head] += V^T P. The two probability tiles rounded to bf16 ARE the column operand
//           of a 32-key MFMA whose k slot 8 c + 4 t + i is defined to be key 16 t + 4 c + i: P never
//           moves. V^T is the row operand under the same slot order; V needs the transpose, so the
//           step's 32 x D V rows go VGPR -> LDS (row-major, pitch 2 D + 32 bytes: the 8 rows a
//           half-wave reads start 32 B apart in the bank window) and come back through
//           ds_read_b64_tr_b16, two reads per 16-row d tile.
//   The next step's K and V loads are issued after the score MFMAs have consumed K and the LDS store
//   has consumed V, into the same registers, and are in flight during softmax and PV and while the
//   other waves of the SIMD run.
//
// Changed from the first sketch of this design (per-wave V staging "double-buffered"): one LDS buffer
// per wave. A wave's LDS instructions execute in order, the buffer is private to the wave, and the
// next step's V waits in registers, not in LDS, so a second buffer would never be written earlier
// than the first can be; it would only halve the workgroups an LDS budget admits.
//
// Tail and masking, the VALU kernel's rules: a key at position >= ctx is not loaded; its K fragment
// and its LDS V row are zeros, never garbage (0 x NaN inside an MFMA is NaN), and its score is
// selected to -inf. block_table[b, j] is read only for j < ceil(ctx / page); an entry outside
// [0, num_blocks) contributes nothing and reads nothing; ctx is clamped to max_blocks * page. A K/V
// address is (blk * page + off + r) * Hk * D + hk * D + c with 0 <= blk < num_blocks checked,
// off + r < page (off a multiple of 16 below page, r < live <= 16) and c < D; a scale address is
// (blk * page + off + r) * Hk + hk under the same bounds.
//
// e4m3 cache (FP8): bytes -> f32 (v_cvt_pk_f32_fp8, exact) x the (token, kv head) power-of-two scale
// -> bf16 (exact), then as above: K into the fragment, V into the LDS image. The result is the
// attention over the dequantised cache.
//
// Epilogue: the 4 waves merge in wave order through LDS as in the VALU kernel; num_splits == 1
// normalises (l == 0: zeros) and rounds to bf16 once, otherwise fp32 O and (m, l) go to the
// workspace, (-inf, 0) for an empty split. A row's bits depend on its own q, its own sequence and
// num_splits only.
#include "attention_decode_merge.h"
#include "kv_fp8.h"
#include "paged_kv.h"

namespace {

__device__ __forceinline__ bf16x8_t zero_frag() { return __builtin_bit_cast(bf16x8_t, u32x4{0u, 0u, 0u, 0u}); }

// 8 cache elements as loaded -> the bf16 MFMA fragment
__device__ __forceinline__ bf16x8_t kv_frag(u32x4 raw, float) { return __builtin_bit_cast(bf16x8_t, raw); }
__device__ __forceinline__ bf16x8_t kv_frag(uint2 raw, float s) {
  float f[8];
  unpack8_fp8(raw, f);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] *= s;
  return __builtin_bit_cast(bf16x8_t, pack8(f));
}

template <int D, bool FP8>
__global__ __launch_bounds__(256, 2) void attn_decode_mfma_kernel(
    const bf16_t* __restrict__ q, long q_stride, const void* __restrict__ k_cache, const void* __restrict__ v_cache,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const int* __restrict__ block_table,
    const int* __restrict__ context_lens, int max_blocks, int num_blocks, int page_size, int Hk, int G,
    float scale_log2, int num_splits, bf16_t* __restrict__ out, float* __restrict__ part_o,
    float* __restrict__ part_ml) {
  using elem_t = std::conditional_t<FP8, fp8_t, bf16_t>;
  using raw_t = std::conditional_t<FP8, uint2, u32x4>;  // 8 elements of a cache row
  constexpr int NKS = D / 32;       // MFMAs per score tile
  constexpr int NDT = D / 16;       // 16-row tiles of O^T
  constexpr int LPT = D / 8;        // lanes per V row
  constexpr int TPW = 64 / LPT;     // V rows per wave-wide load
  constexpr int U = 32 / TPW;       // V loads per lane and step
  constexpr int PITCH = D * 2 + 32;  // bytes per V row in LDS
  constexpr int VBUF = 32 * PITCH;   // one wave's staging buffer; later its [16][D] fp32 partial O
  static_assert(16 * D * 4 <= VBUF && 16 % TPW == 0, "the partial O reuses the wave's staging buffer");
  __shared__ __attribute__((aligned(16))) char smem[kDecWaves * VBUF];
  __shared__ float sm_m[kDecWaves][16], sm_l[kDecWaves][16];

  const elem_t* __restrict__ kc = static_cast<const elem_t*>(k_cache);
  const elem_t* __restrict__ vc = static_cast<const elem_t*>(v_cache);
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, c = lane >> 4;        // MFMA lane map
  const int sub = lane % LPT, grp = lane / LPT;  // V staging lane map
  const int Hq = Hk * G;

  const long ctx_l = context_lens[b];
  const long cap = (long)max_blocks * page_size;  // never index past the block table's row
  const int ctx = (int)(ctx_l < 0 ? 0 : (ctx_l > cap ? cap : ctx_l));
  const int npages = (ctx + page_size - 1) / page_size;
  const int pps = (npages + num_splits - 1) / num_splits;
  const int p0 = min(split * pps, npages);
  const int p1 = min(p0 + pps, npages);
  // this split's tokens [tok0, tok1) as steps of 32; tok0 is a multiple of page_size, hence of 16
  const int tok0 = p0 * page_size, tok1 = min(p1 * page_size, ctx);
  const int nstep = (tok1 - tok0 + 31) >> 5;

  bf16x8_t qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
    qf[ks] = r < G ? gload8(q + (long)b * q_stride + (long)(hk * G + r) * D + 32 * ks + 8 * c) : zero_frag();

  f32x4 o[NDT];
#pragma unroll
  for (int i = 0; i < NDT; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = neg_inf(), l = 0.f;  // l: this lane's keys only, summed over the 4 lane groups at the end

  const long tok_stride = (long)Hk * D;  // elements between consecutive slots
  const int* bt = block_table + (long)b * max_blocks;
  char* vs_w = smem + wave * VBUF;
  const int trb = (4 * c + (r >> 2)) * PITCH + 8 * (r & 3);  // transposed read: row 4c + r/4, columns 4 (r%4) ..

  long slot0[2];  // first slot of each 16-key tile of the step in registers
  int live[2];    // its live keys, 0: nothing to read
  raw_t kr[2][NKS], vr[U];
  float ksr[2], vsr[U];

  auto lookup = [&](int st) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key0 = tok0 + 32 * st + 16 * t;
      int lv = min(16, tok1 - key0);  // <= 0: past this split's tokens
      long s0 = 0;
      if (lv > 0) {
        const int pg = key0 / page_size;  // < p1 <= npages
        const int blk = bt[pg];
        if ((unsigned)blk < (unsigned)num_blocks) s0 = (long)blk * page_size + (key0 - pg * page_size);
        else lv = 0;  // not a block of this cache: nothing to read
      }
      slot0[t] = s0;
      live[t] = max(lv, 0);
    }
  };
  auto load = [&]() {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bool on = r < live[t];
      const long slot = slot0[t] + r;
      const elem_t* kp = kc + slot * tok_stride + (long)hk * D + 8 * c;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) kr[t][ks] = on ? *reinterpret_cast<const raw_t*>(kp + 32 * ks) : raw_t{};
      if constexpr (FP8) ksr[t] = on ? ksc[slot * Hk + hk] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = (u * TPW) >> 4, rr = ((u * TPW) & 15) + grp;  // row 16 t + rr of the step
      const bool on = rr < live[t];
      const long slot = slot0[t] + rr;
      vr[u] = on ? *reinterpret_cast<const raw_t*>(vc + slot * tok_stride + (long)hk * D + 8 * sub) : raw_t{};
      if constexpr (FP8) vsr[u] = on ? vsc[slot * Hk + hk] : 0.f;
    }
  };

  if (wave < nstep) {
    lookup(wave);
    load();
  }
#pragma unroll 1
  for (int st = wave; st < nstep; st += kDecWaves) {
    // V rows -> LDS (dead rows as zeros), K -> score MFMAs; both free their registers for the prefetch
#pragma unroll
    for (int u = 0; u < U; ++u)
      *reinterpret_cast<u32x4*>(vs_w + (u * TPW + grp) * PITCH + sub * 16) =
          __builtin_bit_cast(u32x4, kv_frag(vr[u], FP8 ? vsr[u] : 0.f));
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kv_frag(kr[t][ks], FP8 ? ksr[t] : 0.f), qf[ks], s[t], 0, 0, 0);
    }
    const int lv[2] = {live[0], live[1]};
    if (st + kDecWaves < nstep) {
      lookup(st + kDecWaves);
      load();
    }

    // lane (r, c): head r, keys 4 c + i of tile t in s[t][i]
    float mx = m;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[t][i] = 4 * c + i < lv[t] ? s[t][i] * scale_log2 : neg_inf();
        mx = fmaxf(mx, s[t][i]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mr = safe_ref(mx);
    const float alpha = fast_exp2(m - mr);
    m = mx;
    float ps = 0.f;
    bf16x8_t pf;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = fast_exp2(s[t][i] - mr);
        ps += p;
        pf[4 * t + i] = (__bf16)p;
      }
    l = l * alpha + ps;
#pragma unroll
    for (int db = 0; db < NDT; ++db) {
      o[db] *= alpha;
      const bf16x8_t vf = lds_tr8(vs_w + trb + 32 * db, vs_w + trb + 16 * PITCH + 32 * db);
      o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[db], 0, 0, 0);
    }
  }

  // this wave's (m, l, O) -> LDS: O as [head][D] fp32 over the wave's own staging buffer (its LDS
  // instructions execute in order, and no other wave touches it before the barrier)
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  float* so = reinterpret_cast<float*>(vs_w);
#pragma unroll
  for (int db = 0; db < NDT; ++db) *reinterpret_cast<f32x4*>(so + r * D + 16 * db + 4 * c) = o[db];
  if (c == 0) {
    sm_m[wave][r] = m;
    sm_l[wave][r] = l;
  }
  __syncthreads();

  // merge the 4 waves in wave order; thread -> (query head g, 8 columns cc)
  if (tid < G * LPT) {
    const int g = tid / LPT, cc = tid % LPT;
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
      const float* po = reinterpret_cast<const float*>(smem + w * VBUF) + g * D + cc * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += a * po[j];
    }
    const int hq = hk * G + g;
    if (num_splits == 1) {
      const float inv = lt > 0.f ? 1.f / lt : 0.f;  // context_len 0: zeros
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] *= inv;
      *reinterpret_cast<u32x4*>(out + ((long)b * Hq + hq) * D + cc * 8) = pack8(acc);
    } else {
      const long row = ((long)b * Hq + hq) * num_splits + split;
      float* po = part_o + row * D + cc * 8;
      *reinterpret_cast<f32x4*>(po) = f32x4{acc[0], acc[1], acc[2], acc[3]};
      *reinterpret_cast<f32x4*>(po + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
      if (cc == 0) *reinterpret_cast<float2*>(part_ml + row * 2) = float2{mt, lt};  // empty split: (-inf, 0)
    }
  }
}

// Explicit instantiations for every (D, FP8) the launcher selects (see attention.hip: hipcc has
// dropped the host stub of a kernel template instantiated only through its launcher).
#define RCA_DEC_MFMA_INST(DD, FF)                                                                                    \
  template __global__ void attn_decode_mfma_kernel<DD, FF>(                                                          \
      const bf16_t* __restrict__, long, const void* __restrict__, const void* __restrict__, const float* __restrict__, \
      const float* __restrict__, const int* __restrict__, const int* __restrict__, int, int, int, int, int, float,   \
      int, bf16_t* __restrict__, float* __restrict__, float* __restrict__);
RCA_DEC_MFMA_INST(64, false)
RCA_DEC_MFMA_INST(64, true)
RCA_DEC_MFMA_INST(128, false)
RCA_DEC_MFMA_INST(128, true)
#undef RCA_DEC_MFMA_INST

}  // namespace

// The MFMA decode over either cache kind (the scales say which), G = Hq / Hk <= 16 checked by the
// callers: rca_attn_decode_paged_mfma below, and rca_attn_decode_paged (attention_decode.hip) for
// G = 16.
int launch_attn_decode_mfma(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                            const void* k_scale, const void* v_scale, const int* block_table, const int* context_lens,
                            void* out, void* part_o, void* part_ml, int B, int Hq, int Hk, int D, int page_size,
                            int max_blocks, int num_blocks, float scale, int num_splits, hipStream_t stream) {
  auto go = [&](auto d, auto fp8) {
    hipLaunchKernelGGL((attn_decode_mfma_kernel<d.value, fp8.value>), dim3(num_splits, Hk, B), dim3(256), 0, stream,
                       (const bf16_t*)q, (long)q_stride, k_cache, v_cache, (const float*)k_scale,
                       (const float*)v_scale, block_table, context_lens, max_blocks, num_blocks, page_size, Hk, Hq / Hk,
                       scale * paged_kv::kLog2e, num_splits, (bf16_t*)out, (float*)part_o, (float*)part_ml);
    return (int)hipGetLastError();
  };
  const int rc = with_bool(k_scale != nullptr, [&](auto fp8) {
    return D == 128 ? go(paged_kv::int_c<128>{}, fp8) : go(paged_kv::int_c<64>{}, fp8);
  });
  if (rc != 0 || num_splits == 1) return rc;
  return launch_split_combine((const float*)part_o, (const float*)part_ml, (bf16_t*)out, (long)B * Hq, num_splits, D,
                              stream);
}

// rca_attn_decode_paged's arguments, checks and return codes (attention_decode.hip), on the MFMA
// kernel: Hq / Hk is 8 or 16, anything else is a bad shape (-1).
RCA_API int rca_attn_decode_paged_mfma(const void* q, long long q_stride, const void* k_cache, const void* v_cache,
                                       const void* k_scale, const void* v_scale, const int* block_table,
                                       const int* context_lens, void* out, void* part_o, void* part_ml, int B, int Hq,
                                       int Hk, int D, int page_size, int max_blocks, int num_blocks, float scale,
                                       int num_splits, hipStream_t stream) {
  if (B == 0) return 0;
  if (!paged_kv::attn_shape_ok(B, Hq, Hk, D, q_stride, page_size, max_blocks, num_blocks, num_splits)) return -1;
  if (Hq / Hk != 8 && Hq / Hk != 16) return -1;
  if (!paged_kv::grid_ok(B, Hk)) return -2;
  if (!paged_kv::caches_ok(k_cache, v_cache, k_scale, v_scale)) return -3;
  if (!paged_kv::attn_ptrs_ok(q, out, block_table, context_lens, part_o, part_ml, num_splits)) return -3;
  return launch_attn_decode_mfma(q, q_stride, k_cache, v_cache, k_scale, v_scale, block_table, context_lens, out,
                                 part_o, part_ml, B, Hq, Hk, D, page_size, max_blocks, num_blocks, scale, num_splits,
                                 stream);
}
