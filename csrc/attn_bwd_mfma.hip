// Flash-attention backward on CDNA4 matrix cores (v_mfma_f32_32x32x16_{bf16,f16}).
//
// Replaces autograd through the reference's materialised attention (GPT2.py:38-46,
// Llama3.py:131-155) — no [B,H,T,T] tensor, P recomputed from the forward's LSE.
//
// Two atomic-free kernels (dQ is bitwise deterministic):
//  * dK/dV kernel — one workgroup = 4 waves = 128 keys of ONE query head h (kv head
//    g = h / (H/G)).  Key on the MFMA lane: S = Q K^T and dP = dO V^T put the key in the
//    accumulator column, so dV^T += dO^T P and dK^T += Q^T dS take P / dS straight from the
//    accumulator registers as their B operand; dK^T / dV^T for the wave's 32 keys stay in
//    registers for the whole sweep over 32-query steps (one barrier per step).  Per-head
//    partials are plain-stored in fp32 and summed over the H/G heads of each kv group by a
//    tiny reduction (GQA without atomics; MHA writes bf16 directly).
//  * dQ kernel — forward-shaped: one workgroup = 128 queries of one head, the query on the
//    lane (S^T = K Q^T, dP^T = V dO^T), dQ^T += K^T dS^T accumulated in registers over the
//    key tiles, written once.  Costs two extra MFMA products vs. a fused kernel but removes
//    the ~300 MB/layer of fp32 dQ atomics that floored the fused version.
// Softmax constants are lane-local: p = exp2(s*c - lse2), ds = p*(dp - delta)*scale;
// delta = rowsum(dO * O) is computed by the dQ kernel (which holds dO in registers anyway
// and runs first) and handed to the dK/dV kernel through a [B,H,T] fp32 buffer.  Q/dO (dK/dV
// kernel) and K/V (dQ kernel) tiles arrive by global_load_lds DMA, double-buffered, stored as
// row images for MFMA row reads and transposed images for hardware-transposed reads
// (ds_read_b64_tr_b16), or one dual image for both (layouts: attn_tiles.h).  Causal: only tiles
// at/below the diagonal; heaviest first.
#include <float.h>
#include <stdlib.h>
#include <type_traits>

#include "api.h"
#include "attn_tiles.h"
#include "mma.h"

namespace bllm {

constexpr int BWD_BKV = 128;  // keys per workgroup
constexpr int BWD_BQ = 32;    // queries per step

// LDS bytes of one ring slot of the dK/dV kernel: Q rows, Q^T image, dO rows, dO^T image,
// and a per-wave copy of the step's lse/delta (so each wave's stats DMA is its own)
template <int HD, bool DUAL = false, bool MASK = false> constexpr int dkdv_buf_bytes() {
  return (DUAL ? 2 : 4) * BWD_BQ * HD * 2 + 4 * 256 + (MASK ? 4 * 256 : 0);
}

// Inverse RoPE in a backward epilogue (rotate_half form, reference common_components.py:6-35):
// the lane holds elements d..d+3 (d = dc + 8 gq + 4 hh) of the first half in lo and the same
// elements of the second half (d + HD/2) in hi, so each rotation pair is lane-local:
//   g1' = g1 c + g2 s,  g2' = g2 c - g1 s   (c, s = cos/sin [T, HD/2] fp32 at position pos).
// Replaces a separate rope pass over dQ / dK (read + write of [N, (H + G) hd]).  ``row`` is the
// head's first element.
template <typename T, int HD>
__device__ __forceinline__ void rope_bwd_store(const f32x16& lo, const f32x16& hi, float scale, int hh, int pos,
                                               int dc, const float* __restrict__ rcos,
                                               const float* __restrict__ rsin, T* row) {
  constexpr int HALF = HD / 2;
  const float* cp = rcos + (long)pos * HALF + dc + 4 * hh;
  const float* sp = rsin + (long)pos * HALF + dc + 4 * hh;
  uint32_t w1[4][2], w2[4][2];  // packed (d, d+1), (d+2, d+3) of group gq, both halves
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const float4 c = *reinterpret_cast<const float4*>(cp + 8 * gq);
    const float4 sn = *reinterpret_cast<const float4*>(sp + 8 * gq);
    const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {sn.x, sn.y, sn.z, sn.w};
    float o1[4], o2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float g1 = lo[4 * gq + j] * scale, g2 = hi[4 * gq + j] * scale;
      o1[j] = g1 * cc[j] + g2 * ss[j];
      o2[j] = g2 * cc[j] - g1 * ss[j];
    }
    w1[gq][0] = pack2<T>(o1[0], o1[1]);
    w1[gq][1] = pack2<T>(o1[2], o1[3]);
    w2[gq][0] = pack2<T>(o2[0], o2[1]);
    w2[gq][1] = pack2<T>(o2[2], o2[3]);
  }
  // 16-B stores (T21, as attn_fwd_mfma_k's epilogue): lanes l and l+32 hold the same row
#pragma unroll
  for (int gq = 0; gq < 4; gq += 2) {
    store16_pair<T>(row + dc + 8 * gq + 8 * hh, w1[gq], w1[gq + 1]);
    store16_pair<T>(row + HALF + dc + 8 * gq + 8 * hh, w2[gq], w2[gq + 1]);
  }
}

// dQ kernel tile constants (attn_bwd_kernels.h)
constexpr int DQ_BQ = 128;
template <int HD, int BK, bool MASK = false> constexpr int dq_buf_bytes() {
  return 3 * BK * HD * 2 + (MASK ? 4 * 256 : 0);
}

#define BLLM_ATTN_VARLEN 0
#include "attn_bwd_kernels.h"
#undef BLLM_ATTN_VARLEN
#define BLLM_ATTN_VARLEN 1
#include "attn_bwd_kernels.h"
#undef BLLM_ATTN_VARLEN

// GQA heads of a kv head fused into one dK/dV workgroup (no per-head fp32 partials, no
// reduction pass) when the fused grid still has >= 4 workgroups per CU (Llama-3-8B B=24
// 1.51 -> 1.12 ms); below that the per-head grid wins (B=4: 256 fused workgroups, 0.25 ms unfused
// vs 0.35 fused).  Dropped variants (3-slot ring at one workgroup per CU, 64-key dQ tiles) are
// in profiles/r2_kernel_experiments.md.
static bool fuse_gqa_heads(int B, int T_, int H, int G) {
  if (H == G) return false;
  const long nkb = (T_ + BWD_BKV - 1) / BWD_BKV;
  return nkb * G * (long)B >= 1024;
}

bool attn_bwd_kv_partials(int B, int T_, int H, int G) { return H != G && !fuse_gqa_heads(B, T_, H, G); }

// launch helpers: one instantiation per (ring, occupancy, fused heads, dual images) and per
// dropout form (none / counter hash / forward keep mask)
struct BwdArgs {
  const void *qkv, *o, *dout;
  const float* lse;
  float *delta, *dkv_part;
  void* dqkv;
  int T_, H, G, B;
  bool causal;
  uint32_t thr;
  float ik;
  uint64_t seed, offset;
  const uint32_t* kmask;
  const float *rcos, *rsin;
  hipStream_t s;
  int xmap_q, xmap_kv;  // attn_wg_order modes of the dQ / dK-dV grids
};
template <typename TT, int HDD, bool DROP, int BK, int NB, int OC, bool MASK>
static void launch_dq1(const BwdArgs& a, dim3 grid) {
  constexpr int lds = NB * dq_buf_bytes<HDD, BK, MASK>();
  hipLaunchKernelGGL((attn_bwd_dq_k<TT, HDD, DROP, BK, NB, OC, MASK>), grid, dim3(256), lds, a.s, (const TT*)a.qkv, (const TT*)a.o, (const TT*)a.dout, a.lse, a.delta, (TT*)a.dqkv, a.T_, a.H,
                     a.G, a.B, a.causal, a.thr, a.ik, a.seed, a.offset, a.kmask, a.rcos, a.rsin, a.xmap_q);
}
template <typename TT, int HDD, int BK, int NB, int OC>
static void launch_dq(const BwdArgs& a, bool drop, dim3 grid) {
  if (drop && a.kmask) launch_dq1<TT, HDD, true, BK, NB, OC, true>(a, grid);
  else if (drop) launch_dq1<TT, HDD, true, BK, NB, OC, false>(a, grid);
  else launch_dq1<TT, HDD, false, BK, NB, OC, false>(a, grid);
}
template <typename TT, int HDD, bool DROP, int NB, int OC, bool FG, bool DU, bool MASK, bool VL>
static void launch_kv1(const BwdArgs& a, dim3 grid) {
  constexpr int lds = NB * dkdv_buf_bytes<HDD, DU, MASK>() + (VL ? BWD_BKV * HDD * 2 : 0);
  hipLaunchKernelGGL((attn_bwd_mfma_k<TT, HDD, DROP, NB, OC, FG, DU, MASK, VL>), grid, dim3(256), lds, a.s, (const TT*)a.qkv, (const TT*)a.dout, a.lse, a.delta,
                     (TT*)a.dqkv, a.dkv_part, a.T_, a.H, a.G, a.B, a.causal, a.thr, a.ik, a.seed, a.offset, a.kmask,
                     a.rcos, a.rsin, a.xmap_kv);
}
template <typename TT, int HDD, int NB, int OC, bool FG, bool DU, bool VL = false>
static void launch_kv(const BwdArgs& a, bool drop, dim3 grid) {
  if (drop && a.kmask) launch_kv1<TT, HDD, true, NB, OC, FG, DU, true, VL>(a, grid);
  else if (drop) launch_kv1<TT, HDD, true, NB, OC, FG, DU, false, VL>(a, grid);
  else launch_kv1<TT, HDD, false, NB, OC, FG, DU, false, VL>(a, grid);
}
// dQ: 32-key tiles, 3-slot ring, 2 workgroups per CU.  dK/dV: hd 128 -> one dual-use LDS image
// per Q / dO tile, V fragments in LDS, 2-slot ring (Llama-3-8B B=24 1.158 -> 1.009 ms); hd 64 ->
// dual images only with the forward's dropout keep mask (GPT2-774M B=24 0.430 -> 0.420 ms; they
// lose without dropout or with fused GQA heads: 0.367 -> 0.376, Llama-3.2-1B 0.575 -> 0.602 ms,
// profiles/r2_attn_hd64_dual.md), 4-slot ring; else separate row / transposed images, 2-slot ring
template <typename TT, int HDD>
static void launch_bwd(const BwdArgs& a, bool drop, bool fuseg, dim3 grid_q, dim3 grid_kv) {
  launch_dq<TT, HDD, 32, 3, 2>(a, drop, grid_q);
  if constexpr (HDD == 128) {
    if (fuseg) launch_kv<TT, HDD, 2, 2, true, true, true>(a, drop, grid_kv);
    else launch_kv<TT, HDD, 2, 2, false, true, true>(a, drop, grid_kv);
  } else {
    // keep-mask dual-image variant at a launch bound of 3 workgroups per CU (168 VGPRs, 3 waves
    // per SIMD instead of 2 at 170): GPT2-774M B=64 backward 1.260 -> 1.195 ms, B=24 0.448 ->
    // 0.417 (profiles/r6/attn/occ_ab.jsonl)
    if (drop && a.kmask && !fuseg) launch_kv<TT, HDD, 4, 3, false, true>(a, drop, grid_kv);
    else if (fuseg) launch_kv<TT, HDD, 2, 2, true, false>(a, drop, grid_kv);
    else launch_kv<TT, HDD, 2, 2, false, false>(a, drop, grid_kv);
  }
}

void attn_bwd_mfma(DType dt, const void* qkv, const void* o, const float* lse, const void* dout, void* dqkv,
                   float* delta, float* dkv_part, int B, int T_, int H, int G, int hd, bool causal, float p,
                   uint64_t seed, uint64_t offset, const uint32_t* keep_mask, const float* rcos, const float* rsin,
                   hipStream_t s) {
  const int nkb = (T_ + BWD_BKV - 1) / BWD_BKV;
  const bool fuseg = fuse_gqa_heads(B, T_, H, G);
  dim3 grid_kv(nkb * (fuseg ? G : H) * B), grid_q(((T_ + DQ_BQ - 1) / DQ_BQ) * H * B);
  const bool drop = p > 0.f;
  const int xq = attn_xcd_order_ok(B * H, H / G) ? 1 : 0;
  const int xkv = attn_xcd_order_ok((fuseg ? G : H) * B, 1) ? 1 : 0;
  const BwdArgs a{qkv, o, dout, lse, delta, dkv_part, dqkv, T_, H, G, B, causal, drop_threshold16(p),
                  drop_inv_keep(p), seed, offset, drop ? keep_mask : nullptr, rcos, rsin, s, xq, xkv};
  if (dt == DType::BF16) {
    if (hd == 128) launch_bwd<bf16_t, 128>(a, drop, fuseg, grid_q, grid_kv);
    else launch_bwd<bf16_t, 64>(a, drop, fuseg, grid_q, grid_kv);
  } else {
    if (hd == 128) launch_bwd<f16_t, 128>(a, drop, fuseg, grid_q, grid_kv);
    else launch_bwd<f16_t, 64>(a, drop, fuseg, grid_q, grid_kv);
  }
  if (H != G && !fuseg) {
    const long BT = (long)B * T_;
    const long groups = BT * 2L * G * hd / 4;
    const int fg = (int)((groups + 255) / 256 < 4096 ? (groups + 255) / 256 : 4096);
    BLLM_DISPATCH(dt, TT, {
      hipLaunchKernelGGL(attn_bwd_kv_reduce_k<TT>, dim3(fg), dim3(256), 0, s, dkv_part, (TT*)dqkv, BT, H, G, hd, T_,
                         rcos, rsin);
    });
  }
}

// ---- variable-length launch (causal, no dropout): the tilings launch_bwd picks without dropout;
// a.T_ carries max_len, which only sizes the grids
template <typename TT, int HDD, int NB, int OC, bool FG, bool DU, bool VL>
static void launch_kv_varlen(const BwdArgs& a, const int* cu, dim3 grid) {
  constexpr int lds = NB * dkdv_buf_bytes<HDD, DU, false>() + (VL ? BWD_BKV * HDD * 2 : 0);
  hipLaunchKernelGGL((attn_bwd_mfma_varlen_k<TT, HDD, false, NB, OC, FG, DU, false, VL>), grid, dim3(256), lds, a.s,
                     (const TT*)a.qkv, (const TT*)a.dout, a.lse, a.delta, (TT*)a.dqkv, a.dkv_part, a.T_, a.H, a.G, a.B,
                     true, a.thr, a.ik, a.seed, a.offset, a.kmask, a.rcos, a.rsin, a.xmap_kv, cu);
}
template <typename TT, int HDD>
static void launch_bwd_varlen(const BwdArgs& a, const int* cu, bool fuseg, dim3 grid_q, dim3 grid_kv) {
  constexpr int lds_q = 3 * dq_buf_bytes<HDD, 32, false>();
  hipLaunchKernelGGL((attn_bwd_dq_varlen_k<TT, HDD, false, 32, 3, 2, false>), grid_q, dim3(256), lds_q, a.s,
                     (const TT*)a.qkv, (const TT*)a.o, (const TT*)a.dout, a.lse, a.delta, (TT*)a.dqkv, a.T_, a.H, a.G,
                     a.B, true, a.thr, a.ik, a.seed, a.offset, a.kmask, a.rcos, a.rsin, a.xmap_q, cu);
  if constexpr (HDD == 128) {
    if (fuseg) launch_kv_varlen<TT, HDD, 2, 2, true, true, true>(a, cu, grid_kv);
    else launch_kv_varlen<TT, HDD, 2, 2, false, true, true>(a, cu, grid_kv);
  } else {
    if (fuseg) launch_kv_varlen<TT, HDD, 2, 2, true, false, false>(a, cu, grid_kv);
    else launch_kv_varlen<TT, HDD, 2, 2, false, false, false>(a, cu, grid_kv);
  }
}

// cu: device int32 [B + 1] row offsets (cu[B] = N); pos_ids: device int32 [N], each row's index
// inside its sequence (the GQA reduction's inverse RoPE reads it); delta: [H * N] floats;
// dkv_part: 2 * N * H * hd floats when attn_bwd_kv_partials(B, max_len, H, G), else unused
void attn_bwd_mfma_varlen(DType dt, const void* qkv, const void* o, const float* lse, const void* dout, void* dqkv,
                          float* delta, float* dkv_part, const int* cu, const int* pos_ids, long N, int B, int max_len,
                          int H, int G, int hd, const float* rcos, const float* rsin, hipStream_t s) {
  const int nkb = (max_len + BWD_BKV - 1) / BWD_BKV, nqb = (max_len + DQ_BQ - 1) / DQ_BQ;
  if (nkb == 0 || B == 0) return;
  const bool fuseg = fuse_gqa_heads(B, max_len, H, G);
  dim3 grid_kv(nkb * (fuseg ? G : H) * B), grid_q(nqb * H * B);
  const int xq = attn_xcd_order_ok(B * H, H / G) ? 1 : 0;
  const int xkv = attn_xcd_order_ok((fuseg ? G : H) * B, 1) ? 1 : 0;
  const BwdArgs a{qkv, o, dout, lse, delta, dkv_part, dqkv, max_len, H, G, B, true, 0u, 1.f, 0, 0, nullptr, rcos, rsin,
                  s, xq, xkv};
  if (dt == DType::BF16) {
    if (hd == 128) launch_bwd_varlen<bf16_t, 128>(a, cu, fuseg, grid_q, grid_kv);
    else launch_bwd_varlen<bf16_t, 64>(a, cu, fuseg, grid_q, grid_kv);
  } else {
    if (hd == 128) launch_bwd_varlen<f16_t, 128>(a, cu, fuseg, grid_q, grid_kv);
    else launch_bwd_varlen<f16_t, 64>(a, cu, fuseg, grid_q, grid_kv);
  }
  if (H != G && !fuseg) {
    const long groups = N * 2L * G * hd / 4;
    if (groups == 0) return;
    const int fg = (int)((groups + 255) / 256 < 4096 ? (groups + 255) / 256 : 4096);
    BLLM_DISPATCH(dt, TT, {
      hipLaunchKernelGGL(attn_bwd_kv_reduce_varlen_k<TT>, dim3(fg), dim3(256), 0, s, dkv_part, (TT*)dqkv, N, H, G, hd,
                         pos_ids, rcos, rsin);
    });
  }
}

}  // namespace bllm
