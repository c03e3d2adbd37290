// FP8-weight projection for the decode step, gfx950: y[M, N] = x[M, K] . dequant(pack)^T (+ bias)
// (+ residual) at one token per row (M = B <= 32 is the design point; any M >= 1 is correct).
//
// Format (ops/reference.py:kv_quantize_rows applied to the rows of W [N, K] is the contract): row n
// is K e4m3fn bytes q[n] and one fp32 scale s[n]; the weight is float(q[n][k]) * s[n].  Every e4m3
// value is exact in bf16 and fp16 (v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1, as
// attn_decode_fp8.hip), so x . q is exact in fp32 products; the roundings are the fp32 sums, one
// multiply by s[n] on the finished dot product, the fp32 adds of bias and residual, and the store.
//
// Pack layout (ops.w8_pack): N is padded to 16-row tiles (zero bytes), K is whole 64-wide blocks.
// Tile t, block kb is 1 KiB at ((t * K / 64 + kb) * 64 + lane) * 16: lane = 16 g + r holds the 16
// bytes q[16 t + r][64 kb + 16 g .. + 15], i.e. the A fragments of two v_mfma_f32_16x16x32 steps
// (bytes 0..7, then 8..15, in k slots 8 g + j).  A wave's 16-byte load is that KiB, contiguous, and
// the blocks of a tile follow each other.  The B operand is x^T with the same k permutation: lane
// (g, c) takes x[m0 + c][64 kb + 16 g ..] (two 16-byte loads, straight from global memory: x is
// at most 32 x K and stays in the caches).  Column m of an MFMA depends on x row m alone, so a
// row of y is the same bits for any M and any contents of the other rows.
//
// One launch: workgroup = RT consecutive tiles x one group of 32 x rows, K split in contiguous
// slices over the 8 waves, weights streamed to VGPRs (U blocks of every tile in flight per wave,
// no LDS), the waves' partial accumulators summed through LDS in wave order.  Nothing passes
// between workgroups.  RT and U depend on N alone (linear_w8_tiles).  x rows at or past M are read
// as row M - 1 and tiles past the last as the last (in bounds, no branch around a load) and are
// not stored.
#include "api.h"
#include "mma.h"

namespace bllm {

constexpr int W8_TN = 16;     // rows of a pack tile
constexpr int W8_KG = 64;     // k per 1-KiB block of a tile
constexpr int W8_WAVES = 8;   // waves per workgroup = K slices

int linear_w8_row_tile() { return W8_TN; }
int linear_w8_k_granule() { return W8_KG; }
// pack tiles per workgroup: 64-row workgroups once they alone cover the chip's 256 CUs
static int linear_w8_tiles(int N) { return N >= 256 * 4 * W8_TN ? 4 : 1; }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 8 e4m3 bytes (two dwords) -> one 8-element MFMA fragment of T
template <typename T> __device__ __forceinline__ s16x8 w8_frag(uint32_t lo, uint32_t hi) {
  u32x4 r;
  if constexpr (std::is_same<T, bf16_t>::value) {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
  } else {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true));
  }
  return __builtin_bit_cast(s16x8, r);
}

// U blocks from kb of every tile: all loads first, then the conversions and MFMAs.  H2: the group
// has x rows in its second 16 (uniform per workgroup).
template <typename T, int RT, int U, bool H2>
__device__ __forceinline__ void w8_blocks(const uint4* const (&wt)[RT], const T* x0, const T* x1, int kb,
                                          f32x4 (&acc)[RT][2]) {
  uint4 a[U][RT];
  s16x8 b[U][2][2];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < RT; ++t) a[u][t] = wt[t][(long)(kb + u) * 64];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long o = (long)(kb + u) * W8_KG;
    b[u][0][0] = *reinterpret_cast<const s16x8*>(x0 + o);
    b[u][0][1] = *reinterpret_cast<const s16x8*>(x0 + o + 8);
    if constexpr (H2) {
      b[u][1][0] = *reinterpret_cast<const s16x8*>(x1 + o);
      b[u][1][1] = *reinterpret_cast<const s16x8*>(x1 + o + 8);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const s16x8 a0 = w8_frag<T>(a[u][t].x, a[u][t].y), a1 = w8_frag<T>(a[u][t].z, a[u][t].w);
      acc[t][0] = Mma<T>::mma(a0, b[u][0][0], acc[t][0]);
      acc[t][0] = Mma<T>::mma(a1, b[u][0][1], acc[t][0]);
      if constexpr (H2) {
        acc[t][1] = Mma<T>::mma(a0, b[u][1][0], acc[t][1]);
        acc[t][1] = Mma<T>::mma(a1, b[u][1][1], acc[t][1]);
      }
    }
}

template <typename T, int RT, int U, bool H2>
__device__ __forceinline__ void w8_stream(const uint4* const (&wt)[RT], const T* x0, const T* x1, int kb, int kb1,
                                          f32x4 (&acc)[RT][2]) {
  for (; kb + U <= kb1; kb += U) w8_blocks<T, RT, U, H2>(wt, x0, x1, kb, acc);
  for (; kb < kb1; ++kb) w8_blocks<T, RT, 1, H2>(wt, x0, x1, kb, acc);
}

template <typename T, int RT, int U>
__global__ __launch_bounds__(W8_WAVES * 64) void linear_w8_k(const T* __restrict__ x, const uint4* __restrict__ wp,
                                                             const float* __restrict__ scale,
                                                             const T* __restrict__ bias, const T* __restrict__ res,
                                                             T* __restrict__ y, int M, int N, int K) {
  __shared__ __align__(16) float s_red[W8_WAVES][RT][2][64][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int nkb = K / W8_KG, ntile = (N + W8_TN - 1) / W8_TN;
  const int t0 = blockIdx.x * RT, m0 = blockIdx.y * 32;
  const bool h2 = m0 + 16 < M;

  const int per = (nkb + W8_WAVES - 1) / W8_WAVES;   // this wave's slice of the blocks
  const int kb0 = min(w * per, nkb), kb1 = min(kb0 + per, nkb);
  const T* x0 = x + (long)min(m0 + c, M - 1) * K + 16 * g;
  const T* x1 = x + (long)min(m0 + 16 + c, M - 1) * K + 16 * g;
  const uint4* wt[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) wt[t] = wp + (long)min(t0 + t, ntile - 1) * nkb * 64 + lane;

  f32x4 acc[RT][2];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (h2) w8_stream<T, RT, U, true>(wt, x0, x1, kb0, kb1, acc);
  else w8_stream<T, RT, U, false>(wt, x0, x1, kb0, kb1, acc);

#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      *reinterpret_cast<float4*>(s_red[w][t][h][lane]) = make_float4(acc[t][h][0], acc[t][h][1], acc[t][h][2], acc[t][h][3]);
  __syncthreads();

  // thread = (tile t, half h, accumulator lane l): rows n .. n + 3 of y row m, waves summed in order
  for (int i = tid; i < RT * 2 * 64; i += W8_WAVES * 64) {
    const int t = i >> 7, h = (i >> 6) & 1, l = i & 63;
    const int m = m0 + 16 * h + (l & 15), n = (t0 + t) * W8_TN + 4 * (l >> 4);
    if (m >= M || n >= N) continue;
    float4 v = *reinterpret_cast<const float4*>(s_red[0][t][h][l]);
#pragma unroll
    for (int ww = 1; ww < W8_WAVES; ++ww) {
      const float4 p = *reinterpret_cast<const float4*>(s_red[ww][t][h][l]);
      v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    const float o[4] = {v.x, v.y, v.z, v.w};
    T* yr = y + (long)m * N + n;
    const T* rr = res ? res + (long)m * N + n : nullptr;
    if ((N & 3) == 0) {   // n + 3 < N and 8-byte aligned rows: one load / store for the four
      VecN<T, 4> r4, out;
      if (rr) r4 = ldv<T, 4>(rr);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float f = o[e] * scale[n + e];
        if (bias) f += to_f(bias[n + e]);
        if (rr) f += to_f(r4.v[e]);
        out.v[e] = from_f<T>(f);
      }
      stv<T, 4>(yr, out);
    } else {
      for (int e = 0; e < 4 && n + e < N; ++e) {
        float f = o[e] * scale[n + e];
        if (bias) f += to_f(bias[n + e]);
        if (rr) f += to_f(rr[e]);
        yr[e] = from_f<T>(f);
      }
    }
  }
}

bool linear_w8_supported(int M, int N, int K) { return M >= 1 && N >= 1 && K >= W8_KG && K % W8_KG == 0; }

template <typename T>
static void w8_launch(const void* x, const void* wp, const float* scale, const void* bias, const void* res, void* y,
                      int M, int N, int K, hipStream_t s) {
  const int ntile = (N + W8_TN - 1) / W8_TN, RT = linear_w8_tiles(N);
  const dim3 grid((ntile + RT - 1) / RT, (M + 31) / 32), block(W8_WAVES * 64);
#define L_(RTT, UU) hipLaunchKernelGGL((linear_w8_k<T, RTT, UU>), grid, block, 0, s, (const T*)x, (const uint4*)wp, \
                                       scale, (const T*)bias, (const T*)res, (T*)y, M, N, K)
  if (RT == 4) L_(4, 2); else L_(1, 4);
#undef L_
}

void linear_w8(DType dt, const void* x, const void* wp, const float* scale, const void* bias, const void* res,
               void* y, int M, int N, int K, hipStream_t s) {
  if (dt == DType::BF16) w8_launch<bf16_t>(x, wp, scale, bias, res, y, M, N, K, s);
  else w8_launch<f16_t>(x, wp, scale, bias, res, y, M, N, K, s);
}

}  // namespace bllm
