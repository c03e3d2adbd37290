// Matrix-core primitives shared by every MFMA kernel of csrc/: the vector typedefs, the bf16 /
// fp16 MFMA trait, the float -> 16-bit pair pack, the transposed LDS fragment read and the
// lane-pair 16-B store.  (gemm4.h's g4::MfA is the AGPR-tied inline-asm MFMA of the 4-wave GEMMs,
// a different thing; attn_f32.hip keeps its own fp32 32x32x2 wrapper.)
#pragma once
#include <type_traits>

#include "common.h"

namespace bllm {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) s16x8 lds_s16x8;

// v_mfma_f32_{32x32x16,16x16x32}_{bf16,f16}, picked by the accumulator type: f32x16 -> 32x32x16,
// f32x4 -> 16x16x32.  Fragments are the native 8-element vector v8, or raw s16x8 bits (what the
// transposed LDS reads and 16-B global loads of the GEMM-style kernels deliver).
template <typename T> struct Mma {
  static constexpr bool BF = std::is_same<T, bf16_t>::value;
  static_assert(BF || std::is_same<T, f16_t>::value, "bf16 / fp16 only");
  typedef typename std::conditional<BF, bf16x8, f16x8>::type v8;
  static __device__ __forceinline__ f32x16 mma(v8 a, v8 b, f32x16 c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4 mma(v8 a, v8 b, f32x4 c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  template <typename Acc> static __device__ __forceinline__ Acc mma(s16x8 a, s16x8 b, Acc c) {
    return mma(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c);
  }
};

// two floats -> packed pair (one v_cvt_pk_bf16_f32 for bf16)
template <typename T> __device__ __forceinline__ uint32_t pack2(float a, float b) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef T t2 __attribute__((ext_vector_type(2)));
  const t2 v = __builtin_convertvector((f2{a, b}), t2);
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  return u;
}

// One 8-element MFMA fragment from two hardware-transposed LDS reads (ds_read_b64_tr_b16: a
// 16-lane group gets 4 rows x 16 columns delivered column-major = 4 k-values of one column per
// lane): the lane's 4 k-values at base + off_lo, then the 4 at base + off_hi.  V8 = s16x8 or the
// native vector.
template <typename V8> __device__ __forceinline__ V8 tr_read8(const char* base, int off_lo, int off_hi) {
  const s16x4 r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off_lo));
  const s16x4 r2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off_hi));
  // whole-register concatenation (an element-wise short[8] build made hipcc emit a v_bfi per
  // fragment and wait for the read right there)
  return __builtin_bit_cast(V8, __builtin_shufflevector(r1, r2, 0, 1, 2, 3, 4, 5, 6, 7));
}

// The same fragment out of a row-major [k][col] tile with rows of `stride` bytes: lane (g, q, p) =
// (lane >> 4, (lane & 15) >> 2, lane & 3) reads k-rows 8g + q and 8g + q + 4 at the 4 columns
// from byte col_byte + 8p, i.e. the 8 k-values 8g .. 8g+7 of column lane & 15 of the 16-column
// block at col_byte.
template <typename V8>
__device__ __forceinline__ V8 tr_tile8(const char* tile, int stride, int col_byte, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  return tr_read8<V8>(tile + (8 * g + q) * stride + col_byte + 8 * p, 0, 4 * stride);
}

// Row-per-lane-pair 16-B store (cdna_hip_programming.md T21).  A lane of a 32x32 accumulator
// holds, per group gq of 8 columns, the 4 columns 4 hh + 0..3 (hh = lane >> 5).  Given the packed
// columns of groups gq (a) and gq + 1 (b), one v_permlane32_swap per dword leaves group gq's 8
// contiguous columns in the lower lane half and gq + 1's in the upper: half the store instructions
// of the dwordx2 form, same bytes.  Every lane must take part in pair16 (cross-lane), lanes l and
// l + 32 must hold the same row, and the result is stored at row + 8 gq + 8 hh.
__device__ __forceinline__ uint4 pair16(const uint32_t (&a)[2], const uint32_t (&b)[2]) {
  const auto rx = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);
  const auto ry = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
  return uint4{rx[0], ry[0], rx[1], ry[1]};
}
template <typename T>
__device__ __forceinline__ void store16_pair(T* dst, const uint32_t (&a)[2], const uint32_t (&b)[2]) {
  *reinterpret_cast<uint4*>(dst) = pair16(a, b);
}

}  // namespace bllm
