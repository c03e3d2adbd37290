// Flash-attention forward on CDNA4 matrix cores (v_mfma_f32_32x32x16_{bf16,f16}).
//
// Replaces the reference's materialised attention (GPT2.py:38-46, Llama3.py:131-155:
// scores [B,H,T,T] -> masked_fill -> softmax -> @V, plus K/V repeat_interleave for GQA).
//
// Formulation ("swapped" operands, so every per-query quantity is lane-local):
//   S^T[key][q] = K · Q^T        A = K tile from LDS (row reads), B = Q fragment in VGPRs
//   O^T[d][q]  += V^T · P^T       A = V^T via ds_read_b64_tr_b16 (hardware transpose),
//                                 B = P taken straight from the S accumulator registers
// With 32x32x16 MFMA the accumulator column is the lane (lane & 31 = query) and its rows
// are keys, so the online-softmax max/sum for a query are a per-lane reduction over its
// 32 registers plus ONE cross-half exchange (lane ^ 32); the rescale of O^T by alpha is
// per lane.  The accumulator registers 8s..8s+7 are reused as the PV B-operand of k-step s
// (element j of lane half h = key 16s + 8(j>>2) + 4h + (j&3)); the V^T operand is read
// with the matching key permutation: two transposed reads of 4 keys each.
//
// Workgroup = 4 waves; each wave owns one 32-query block (128 queries per workgroup; two blocks
// per wave, which halves the LDS reads per FLOP, measured slower on every shape:
// profiles/r3/attn_fwd_qb2.md -- the per-query arrays below keep a block index for that layout).
// K/V tiles of 64 keys, register DMA (global_load_lds) of tile t+1 under the MFMAs of tile t,
// double-buffered LDS.  GQA reads kv head h / (H/G)
// directly; causal tiles above the diagonal are skipped; q-blocks are launched
// heaviest-first.  LDS images are XOR-swizzled (attn_tiles.h): K is a row image (conflict-free
// ds_read_b128 row reads), V a transposed image (conflict-free transposed reads).
// Attention-probability dropout (GPT-2) uses the stateless counter hash of common.h.
#include <float.h>
#include <stdlib.h>

#include <type_traits>
#include "api.h"
#include "attn_tiles.h"
#include "mma.h"

namespace bllm {

constexpr float kRescaleThr = 8.f;  // deferred online-softmax rescale threshold (log2 units)
constexpr int FWD_BQ = 128;  // queries per workgroup per q-block of each wave (x QB)
constexpr int FWD_NBUF = 2;  // LDS ring slots: the DMA of tile t+1 lands under the MFMAs of tile t
// keys per tile (FWD_BK) and workgroups per CU are template parameters

#define BLLM_ATTN_VARLEN 0
#include "attn_fwd_kernel.h"
#undef BLLM_ATTN_VARLEN
#define BLLM_ATTN_VARLEN 1
#include "attn_fwd_kernel.h"
#undef BLLM_ATTN_VARLEN

bool attn_mfma_head_dim(int hd) { return hd == 64 || hd == 128; }

// forward tiling: 64-key tiles, 2 workgroups per CU; for hd 64 on grids of >= 2048
// workgroups 32-key tiles with up to 3 workgroups per CU (GPT2-774M B=24 with dropout 0.179 ->
// 0.163 ms: the hash work wants the third co-resident workgroup; round 6, after the XCD order:
// Llama-3.2-1B B=24 without dropout 658 -> 686 TF/s, GPT-2 without dropout unchanged,
// profiles/r6/attn/smalltiles/).  Dropped: 32-key tiles with a 3-slot ring, two 32-query blocks
// per wave (slower on every shape, profiles/r3/attn_fwd_qb2.md).
static bool fwd_small_tiles(int hd, long nwg) { return hd == 64 && nwg >= 2048; }

void attn_fwd_mfma(DType dt, const void* qkv, void* o, float* lse, int B, int T_, int H, int G, int hd, bool causal,
                   float p, uint64_t seed, uint64_t offset, uint32_t* keep_mask, hipStream_t s) {
  const uint32_t thr = drop_threshold16(p);
  const float ik = drop_inv_keep(p);
  const bool small = fwd_small_tiles(hd, (long)((T_ + FWD_BQ - 1) / FWD_BQ) * H * B);
  // XCD-aware workgroup order when the (batch, kv head) groups split evenly over the 8 XCDs
  const int xmap = attn_xcd_order_ok(B * H, H / G) ? 1 : 0;
#define LAUNCH_V(TT, HDD, BK, OC)                                                                      \
  do {                                                                                                        \
    const int lds = FWD_NBUF * 2 * BK * HDD * 2;                                                                    \
    const dim3 grid(((T_ + FWD_BQ - 1) / FWD_BQ) * H * B), block(256);                                        \
    if (p > 0.f)                                                                                              \
      hipLaunchKernelGGL((attn_fwd_mfma_k<TT, HDD, true, BK, OC>), grid, block, lds, s,          \
                         (const TT*)qkv, (TT*)o, lse, T_, H, G, B, causal, thr, ik, seed, offset, keep_mask, xmap); \
    else                                                                                                      \
      hipLaunchKernelGGL((attn_fwd_mfma_k<TT, HDD, false, BK, OC>), grid, block, lds, s,         \
                         (const TT*)qkv, (TT*)o, lse, T_, H, G, B, causal, thr, ik, seed, offset, nullptr, xmap); \
  } while (0)
#define LAUNCH(TT, HDD)                                                                                       \
  do {                                                                                                        \
    if (small) LAUNCH_V(TT, HDD, 32, 3);                                                                   \
    else LAUNCH_V(TT, HDD, 64, 2);                                                                         \
  } while (0)
  if (dt == DType::BF16) {
    if (hd == 128) LAUNCH(bf16_t, 128); else LAUNCH(bf16_t, 64);
  } else {
    if (hd == 128) LAUNCH(f16_t, 128); else LAUNCH(f16_t, 64);
  }
#undef LAUNCH
#undef LAUNCH_V
}

// Variable-length forward (causal, no dropout): cu = device int32 [B + 1] row offsets, max_len >=
// every length (it only sizes the grid); the tilings of the uniform launch above
void attn_fwd_mfma_varlen(DType dt, const void* qkv, void* o, float* lse, const int* cu, int B, int max_len, int H,
                          int G, int hd, hipStream_t s) {
  const int nqb = (max_len + FWD_BQ - 1) / FWD_BQ;
  if (nqb == 0 || B == 0) return;
  const bool small = fwd_small_tiles(hd, (long)nqb * H * B);
  const int xmap = attn_xcd_order_ok(B * H, H / G) ? 1 : 0;
#define LAUNCH_V(TT, HDD, BK, OC)                                                                              \
  do {                                                                                                         \
    const int lds = FWD_NBUF * 2 * BK * HDD * 2;                                                               \
    hipLaunchKernelGGL((attn_fwd_mfma_varlen_k<TT, HDD, false, BK, OC>), dim3(nqb * H * B), dim3(256), lds, s, \
                       (const TT*)qkv, (TT*)o, lse, max_len, H, G, B, true, 0u, 1.f, (uint64_t)0, (uint64_t)0, \
                       (uint32_t*)nullptr, xmap, cu);                                                          \
  } while (0)
#define LAUNCH(TT, HDD)                  \
  do {                                   \
    if (small) LAUNCH_V(TT, HDD, 32, 3); \
    else LAUNCH_V(TT, HDD, 64, 2);       \
  } while (0)
  if (dt == DType::BF16) {
    if (hd == 128) LAUNCH(bf16_t, 128); else LAUNCH(bf16_t, 64);
  } else {
    if (hd == 128) LAUNCH(f16_t, 128); else LAUNCH(f16_t, 64);
  }
#undef LAUNCH
#undef LAUNCH_V
}

}  // namespace bllm
