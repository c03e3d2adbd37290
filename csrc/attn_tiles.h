// LDS images of a [rows][HD] 16-bit tile used by the MFMA attention kernels (attn_mfma.hip,
// attn_bwd_mfma.hip), HD = 64 or 128, rows of HD * 2 bytes.
//
// A tile arrives by LDS-DMA (global_load_lds_dwordx4): every wave instruction writes 1 KiB of
// LDS lane-linearly, so lane P of the tile's piece sequence lands at byte 16 P = physical 16-B
// chunk pc = P % (HD / 8) of row r = P / (HD / 8).  The DMA cannot scatter; the swizzle is
// applied to the per-lane SOURCE address instead (a permutation of the 16-B chunks inside one
// row, so the loads stay coalesced): the lane fetches the logical chunk that belongs at its
// physical slot (*_SRC16 / *_src16 below), and the linear DMA image IS the swizzled layout.  The MFMA
// consumer then reads logical (row, column) at the byte offset the *_off functions give.  Both
// sides are derived from the same swizzle term here; a producer and a consumer that disagree
// would compute silently wrong numbers.
//
//   row image         16-B chunk c16 of row r at chunk c16 ^ swz16(r): the 16 rows (HD 128) or
//                     the 8 same-parity rows (HD 64) of a ds_read_b128 lane group hit distinct
//                     bank quads -- conflict-free fragment row reads (S / dP operands).
//   transposed image  64-B chunk c64 (32 columns) of row r at c64 ^ swz64(r), 16-B chunks inside
//                     it in place: conflict-free ds_read_b64_tr_b16 (mma.h tr_read8) of the
//                     O^T / dQ^T / dK^T / dV^T operands.
//   dual image        ONE image serving both kinds of read: chunk ch of row r at ch ^ dual_swz(r).
//                     HD 128 (256-B rows): f = ((r&3)<<2) | ((r>>2)&3) (cdna_hip_programming.md
//                     T10 (b)).  HD 64 (128-B rows): f = (((r>>1)&1)<<2) | ((r>>2)&3) -- over the
//                     8 same-parity rows of every b128 lane group f is a permutation of 0..7 (row
//                     reads conflict-free), and rows r, r+2 of an aligned 4-row block differ in
//                     bit 2 (the 4-chunk block a transposed half-wave read touches), so a 32-lane
//                     transposed read hits 32 distinct bank pairs.  Depends on r & 15 only.
//
// The two XOR terms and the producer-side chunk formulas are macros, and the DMA-issue code uses
// them as such: hipcc simplifies a function body before it inlines it, and a swizzle term behind
// a call no longer folds with the caller's row arithmetic (r = P / chunks-per-row, or a
// wave-uniform row base plus the lane's row) the way the in-place expression does -- the kernels'
// ISA changed.  They are type-generic: the forward's full-tile DMA issue does this arithmetic in
// uint32_t on purpose (unsigned shifts, fewer VALU), everything else in int.
#pragma once
#include "common.h"

// swizzle term of row r: 16-B-chunk XOR of the row image, 64-B-chunk XOR of the transposed image
#define BLLM_SWZ16(HD, r) ((HD) == 128 ? ((r) & 15) : (((r) >> 1) & 7))
#define BLLM_SWZ64(HD, r) ((HD) == 128 ? ((r) & 3) : (((r) >> 1) & 1))
// producer side: the logical 16-B chunk of row r that the DMA lane of physical chunk pc fetches
#define BLLM_ROW_IMG_SRC16(HD, r, pc) ((pc) ^ BLLM_SWZ16(HD, r))
#define BLLM_TR_IMG_SRC16(HD, r, pc) ((((pc) >> 2) ^ BLLM_SWZ64(HD, r)) * 4 + ((pc) & 3))

namespace bllm {

template <int HD, typename I> __device__ __forceinline__ I swz16(I r) {
  static_assert(HD == 64 || HD == 128, "head dim");
  return BLLM_SWZ16(HD, r);
}
template <int HD, typename I> __device__ __forceinline__ I swz64(I r) {
  static_assert(HD == 64 || HD == 128, "head dim");
  return BLLM_SWZ64(HD, r);
}
template <int HD> __device__ __forceinline__ int dual_swz(int r) {
  if constexpr (HD == 128) return ((r & 3) << 2) | ((r >> 2) & 3);
  else return (((r >> 1) & 1) << 2) | ((r >> 2) & 3);
}

// consumer side: byte offset of 16-B chunk c16 of row r (row, dual image) / of element col of
// row r (transposed image)
template <int HD> __device__ __forceinline__ int row_img_off(int r, int c16) {
  return r * (HD * 2) + ((c16 ^ swz16<HD>(r)) << 4);
}
template <int HD> __device__ __forceinline__ int tr_img_off(int r, int col) {
  const int c64 = col >> 5, w = (col & 31) << 1;
  return r * (HD * 2) + ((c64 ^ swz64<HD>(r)) << 6) + w;
}
template <int HD> __device__ __forceinline__ int dual_img_off(int r, int ch) {
  return r * (HD * 2) + ((ch ^ dual_swz<HD>(r)) << 4);
}
// producer side of the dual image (its term sits behind a call in every kernel)
template <int HD> __device__ __forceinline__ int dual_img_src16(int r, int pc) { return pc ^ dual_swz<HD>(r); }

}  // namespace bllm
