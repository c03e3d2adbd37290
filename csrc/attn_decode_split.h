// Shared by the split-KV decode kernels (attn_decode_split.hip, attn_decode_fp8.hip): the chunk
// geometry, which fixes the workspace layout that both partial passes write and the one combine
// kernel reads, and the packed 16-bit dot product of the score pass.
#pragma once
#include "common.h"

namespace bllm {

constexpr int SPL_THREADS = 256;
constexpr int SPL_CHUNK = 256;  // keys per workgroup of the partial pass

// two 16-bit elements (one dword of a row) times two of q, added to c in fp32
template <typename T>
__device__ __forceinline__ float spl_dot2(uint32_t a, uint32_t b, float c);
template <>
__device__ __forceinline__ float spl_dot2<bf16_t>(uint32_t a, uint32_t b, float c) {
  typedef __attribute__((ext_vector_type(2))) __bf16 v2;
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(v2, a), __builtin_bit_cast(v2, b), c, false);
}
template <>
__device__ __forceinline__ float spl_dot2<f16_t>(uint32_t a, uint32_t b, float c) {
  typedef __attribute__((ext_vector_type(2))) _Float16 v2;
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(v2, a), __builtin_bit_cast(v2, b), c, false);
}

}  // namespace bllm
