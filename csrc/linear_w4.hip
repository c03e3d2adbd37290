// MXFP4-weight projection for the decode step, gfx950: y[M, N] = x[M, K] . dequant(pack)^T (+ bias)
// (+ residual) at one token per row (M = B <= 32 is the design point; any M >= 1 is correct).  The
// sibling of linear_w8.hip, and the same shape: only the bytes and their conversion differ.
//
// Format (ops/reference.py:mx4_quantize_rows applied to the rows of W [N, K] is the contract): a
// row is cut into blocks of 32 consecutive k; a block is 32 e2m1 codes (sign + 3 bits, magnitudes
// {0, .5, 1, 1.5, 2, 3, 4, 6}), two to a byte with element 2 i in the low nibble, and one E8M0
// byte b = e + 127; the weight is magnitude * 2^e.  v_cvt_scalef32_pk_{bf16,f16}_fp4 turns one
// byte into two 16-bit values times a power-of-two scale; float(b << 23) is that scale bit for bit
// (b is in [1, 254]).  magnitude * 2^e is exact in bf16 (and in fp16 while 2^-13 <= 2^e <= 2^13),
// so x . w is exact in fp32 products; the roundings are the fp32 sums, the fp32 adds of bias and
// residual, and the store.
//
// Pack layout (ops.w4_pack): N is padded to 16-row tiles (zero codes, scale byte 127), K is whole
// 128-wide blocks.  Tile t, block kb is 1 KiB of codes at ((t * K / 128 + kb) * 64 + lane) * 16:
// lane = 16 g + r holds the 16 bytes of row 16 t + r, k = 128 kb + 32 g .. + 31, which is exactly
// one MX block, so a lane needs one scale per 16-byte load: byte (t * K / 128 + kb) * 64 + lane of
// the scale array.  Dword j of the 16 bytes is the A fragment of the j-th of four
// v_mfma_f32_16x16x32 steps (k slots 8 g + i <- k = 128 kb + 32 g + 8 j + i).  The B operand is x^T
// with the same k permutation: lane (g, c) takes x[m0 + c][128 kb + 32 g ..] (four 16-byte loads,
// straight from global memory: x is at most 32 x K and stays in the caches).  Column m of an MFMA
// depends on x row m alone, so a row of y is the same bits for any M and any contents of the other
// rows.
//
// One launch: workgroup = RT consecutive tiles x one group of 32 x rows, K split in contiguous
// slices over the 8 waves, weights streamed to VGPRs (U blocks of every tile in flight per wave,
// no LDS), the waves' partial accumulators summed through LDS in wave order.  Nothing passes
// between workgroups.  RT and U depend on N alone (linear_w4_tiles).  x rows at or past M are read
// as row M - 1 and tiles past the last as the last (in bounds, no branch around a load) and are
// not stored.
#include "api.h"
#include "mma.h"

namespace bllm {

constexpr int W4_TN = 16;     // rows of a pack tile
constexpr int W4_KG = 128;    // k per 1-KiB block of a tile
constexpr int W4_WAVES = 8;   // waves per workgroup = K slices

int linear_w4_row_tile() { return W4_TN; }
int linear_w4_k_granule() { return W4_KG; }
// pack tiles per workgroup: 64-row workgroups once they alone cover the chip's 256 CUs
static int linear_w4_tiles(int N) { return N >= 256 * 4 * W4_TN ? 4 : 1; }

typedef uint32_t w4_u32x4 __attribute__((ext_vector_type(4)));

// 8 e2m1 codes (one dword) times the block scale -> one 8-element MFMA fragment of T
template <typename T> __device__ __forceinline__ s16x8 w4_frag(uint32_t c, float sc) {
  w4_u32x4 r;
  if constexpr (std::is_same<T, bf16_t>::value) {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 0));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 1));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 2));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 3));
  } else {
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 0));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 1));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 2));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, sc, 3));
  }
  return __builtin_bit_cast(s16x8, r);
}

// U blocks from kb of every tile: all loads first, then the conversions and MFMAs.  H2: the group
// has x rows in its second 16 (uniform per workgroup).
template <typename T, int RT, int U, bool H2>
__device__ __forceinline__ void w4_blocks(const uint4* const (&wt)[RT], const uint8_t* const (&st)[RT], const T* x0,
                                          const T* x1, int kb, f32x4 (&acc)[RT][2]) {
  uint4 a[U][RT];
  uint32_t e[U][RT];
  s16x8 b[U][2][4];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      a[u][t] = wt[t][(long)(kb + u) * 64];
      e[u][t] = st[t][(long)(kb + u) * 64];
    }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long o = (long)(kb + u) * W4_KG;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b[u][0][j] = *reinterpret_cast<const s16x8*>(x0 + o + 8 * j);
      if constexpr (H2) b[u][1][j] = *reinterpret_cast<const s16x8*>(x1 + o + 8 * j);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const float sc = __builtin_bit_cast(float, e[u][t] << 23);
      const uint32_t d[4] = {a[u][t].x, a[u][t].y, a[u][t].z, a[u][t].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const s16x8 aj = w4_frag<T>(d[j], sc);
        acc[t][0] = Mma<T>::mma(aj, b[u][0][j], acc[t][0]);
        if constexpr (H2) acc[t][1] = Mma<T>::mma(aj, b[u][1][j], acc[t][1]);
      }
    }
}

template <typename T, int RT, int U, bool H2>
__device__ __forceinline__ void w4_stream(const uint4* const (&wt)[RT], const uint8_t* const (&st)[RT], const T* x0,
                                          const T* x1, int kb, int kb1, f32x4 (&acc)[RT][2]) {
  for (; kb + U <= kb1; kb += U) w4_blocks<T, RT, U, H2>(wt, st, x0, x1, kb, acc);
  for (; kb < kb1; ++kb) w4_blocks<T, RT, 1, H2>(wt, st, x0, x1, kb, acc);
}

template <typename T, int RT, int U>
__global__ __launch_bounds__(W4_WAVES * 64) void linear_w4_k(const T* __restrict__ x, const uint4* __restrict__ wp,
                                                             const uint8_t* __restrict__ sp,
                                                             const T* __restrict__ bias, const T* __restrict__ res,
                                                             T* __restrict__ y, int M, int N, int K) {
  __shared__ __align__(16) float s_red[W4_WAVES][RT][2][64][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int nkb = K / W4_KG, ntile = (N + W4_TN - 1) / W4_TN;
  const int t0 = blockIdx.x * RT, m0 = blockIdx.y * 32;
  const bool h2 = m0 + 16 < M;

  const int per = (nkb + W4_WAVES - 1) / W4_WAVES;   // this wave's slice of the blocks
  const int kb0 = min(w * per, nkb), kb1 = min(kb0 + per, nkb);
  const T* x0 = x + (long)min(m0 + c, M - 1) * K + 32 * g;
  const T* x1 = x + (long)min(m0 + 16 + c, M - 1) * K + 32 * g;
  const uint4* wt[RT];
  const uint8_t* st[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const long o = (long)min(t0 + t, ntile - 1) * nkb * 64 + lane;
    wt[t] = wp + o;
    st[t] = sp + o;
  }

  f32x4 acc[RT][2];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (h2) w4_stream<T, RT, U, true>(wt, st, x0, x1, kb0, kb1, acc);
  else w4_stream<T, RT, U, false>(wt, st, x0, x1, kb0, kb1, acc);

#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      *reinterpret_cast<float4*>(s_red[w][t][h][lane]) = make_float4(acc[t][h][0], acc[t][h][1], acc[t][h][2], acc[t][h][3]);
  __syncthreads();

  // thread = (tile t, half h, accumulator lane l): rows n .. n + 3 of y row m, waves summed in order
  for (int i = tid; i < RT * 2 * 64; i += W4_WAVES * 64) {
    const int t = i >> 7, h = (i >> 6) & 1, l = i & 63;
    const int m = m0 + 16 * h + (l & 15), n = (t0 + t) * W4_TN + 4 * (l >> 4);
    if (m >= M || n >= N) continue;
    float4 v = *reinterpret_cast<const float4*>(s_red[0][t][h][l]);
#pragma unroll
    for (int ww = 1; ww < W4_WAVES; ++ww) {
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
        float f = o[e];
        if (bias) f += to_f(bias[n + e]);
        if (rr) f += to_f(r4.v[e]);
        out.v[e] = from_f<T>(f);
      }
      stv<T, 4>(yr, out);
    } else {
      for (int e = 0; e < 4 && n + e < N; ++e) {
        float f = o[e];
        if (bias) f += to_f(bias[n + e]);
        if (rr) f += to_f(rr[e]);
        yr[e] = from_f<T>(f);
      }
    }
  }
}

bool linear_w4_supported(int M, int N, int K) { return M >= 1 && N >= 1 && K >= W4_KG && K % W4_KG == 0; }

template <typename T>
static void w4_launch(const void* x, const void* wp, const void* sp, const void* bias, const void* res, void* y,
                      int M, int N, int K, hipStream_t s) {
  const int ntile = (N + W4_TN - 1) / W4_TN, RT = linear_w4_tiles(N);
  const dim3 grid((ntile + RT - 1) / RT, (M + 31) / 32), block(W4_WAVES * 64);
#define L_(RTT, UU) hipLaunchKernelGGL((linear_w4_k<T, RTT, UU>), grid, block, 0, s, (const T*)x, (const uint4*)wp, \
                                       (const uint8_t*)sp, (const T*)bias, (const T*)res, (T*)y, M, N, K)
  if (RT == 4) L_(4, 2); else L_(1, 4);
#undef L_
}

void linear_w4(DType dt, const void* x, const void* wp, const void* sp, const void* bias, const void* res, void* y,
               int M, int N, int K, hipStream_t s) {
  if (dt == DType::BF16) w4_launch<bf16_t>(x, wp, sp, bias, res, y, M, N, K, s);
  else w4_launch<f16_t>(x, wp, sp, bias, res, y, M, N, K, s);
}

}  // namespace bllm
