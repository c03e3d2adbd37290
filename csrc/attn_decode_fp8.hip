// FP8 (OCP e4m3fn) KV cache, gfx950: the quantised prefill fill and the per-row append + decode step.
//
// Format (ops/reference.py:kv_quantize_rows is the contract): a head row x of hd elements, read as
// fp32, is stored as hd bytes and one fp32 scale: a = max |x|, s = a / 448 (s = 1 when a = 0),
// byte_i = e4m3fn_rne(x_i / s), both divisions IEEE fp32; dequantised value = float(byte_i) * s.
// Caches K8 / V8 [B, G, Tmax, hd] bytes, Ks / Vs [B, G, Tmax] fp32.  The kernels write exactly the
// oracle's bytes and scale bits.
//
//   fill     one launch over the packed prefill rows, as kv_cache_fill_varlen: hd / 8 lanes per
//            (row, k-or-v head), 16-B load and 8-B store per lane, the row maximum by shuffles
//            inside the lane group.
//   decode   the split-KV step of attn_decode_split.hip on the quantised cache: 256-key chunks,
//            one workgroup per (chunk, kv group or sub-group, row), all loads up front, one key per
//            thread for the scores, the same fp32 partials and the same combine kernel
//            (attn_decode_split_combine_rows).  A thread converts its K row to packed 16-bit pairs
//            once (v_cvt_scalef32_pk_{bf16,f16}_fp8: every e4m3 value is exact in both) and dots it
//            with every head's q; Ks[key] is one multiply on the finished dot product.  Vs[key] is
//            folded into the probability of the key before the P.V pass, which converts the V
//            bytes to fp32 once per key for all heads.  No row is dequantised as a whole.
//            The appended token: the workgroups of the chunk that holds pos[b] quantise the new
//            k / v from the qkv row into LDS and use them from there (that row of the cache is
//            never read in the launch); the one with sub-group 0 also stores them to the cache.
#include "api.h"
#include "attn_decode_split.h"

namespace bllm {

BLLM_DEBUG_WORD(attn_decode_fp8)

constexpr float kFp8Max = 448.f;

// s = a / 448, or 1 for an all-zero row (IEEE division: once per row)
__device__ __forceinline__ float f8_scale(float a) { return a > 0.f ? a / kFp8Max : 1.f; }

// two quotients -> two e4m3 bytes in the low half
__device__ __forceinline__ uint32_t f8_pack2(float x0, float x1, float s) {
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x0 / s, x1 / s, 0, false) & 0xFFFFu;
}

// bytes (2 sel, 2 sel + 1) of w -> a packed pair of T
template <typename T, bool HI>
__device__ __forceinline__ uint32_t f8_pair(uint32_t w);
template <>
__device__ __forceinline__ uint32_t f8_pair<bf16_t, false>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
}
template <>
__device__ __forceinline__ uint32_t f8_pair<bf16_t, true>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
}
template <>
__device__ __forceinline__ uint32_t f8_pair<f16_t, false>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false));
}
template <>
__device__ __forceinline__ uint32_t f8_pair<f16_t, true>(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true));
}

// ------------------------------------------------------------------ fill
// thread = (packed row n, k-or-v head j, 16-B piece c of its hd elements); C = HD / 8 lanes share a
// head row (C divides 64, so a row never straddles a wave and its lanes leave together)
// Two forms share one body (kv_fill_fp8_body.h).  FILL_ROWS: the slot-mapped form, as
// kv_cache_fill_varlen_rows_k (sequence b of B -> cache row rows[b] of CB); without it the kernel
// as it always was.
template <typename T, int HD>
__global__ __launch_bounds__(256) void kv_cache_fill_varlen_fp8_k(const T* __restrict__ qkv,
                                                                  const int* __restrict__ cu, uint8_t* __restrict__ k8,
                                                                  float* __restrict__ ks, uint8_t* __restrict__ v8,
                                                                  float* __restrict__ vs, long N, int B, int H, int G,
                                                                  int Tmax) {
#define FILL_ROWS 0
#include "kv_fill_fp8_body.h"
#undef FILL_ROWS
}

template <typename T, int HD>
__global__ __launch_bounds__(256) void kv_cache_fill_varlen_fp8_rows_k(
    const T* __restrict__ qkv, const int* __restrict__ cu, uint8_t* __restrict__ k8, float* __restrict__ ks,
    uint8_t* __restrict__ v8, float* __restrict__ vs, long N, int B, int H, int G, int Tmax,
    const int* __restrict__ rows, int CB) {
#define FILL_ROWS 1
#include "kv_fill_fp8_body.h"
#undef FILL_ROWS
}

void kv_cache_fill_varlen_fp8(DType dt, const void* qkv, const int* cu, void* k8, float* ks, void* v8, float* vs,
                              long N, int B, int H, int G, int hd, int Tmax, hipStream_t s, const int* rows, int CB) {
  const long total = N * 2L * G * (hd / 8);
  if (total == 0) return;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define L_(TT, HDD)                                                                                                \
  do {                                                                                                             \
    if (rows)                                                                                                      \
      hipLaunchKernelGGL((kv_cache_fill_varlen_fp8_rows_k<TT, HDD>), grid, block, 0, s, (const TT*)qkv, cu,       \
                         (uint8_t*)k8, ks, (uint8_t*)v8, vs, N, B, H, G, Tmax, rows, CB);                          \
    else                                                                                                           \
      hipLaunchKernelGGL((kv_cache_fill_varlen_fp8_k<TT, HDD>), grid, block, 0, s, (const TT*)qkv, cu,            \
                         (uint8_t*)k8, ks, (uint8_t*)v8, vs, N, B, H, G, Tmax);                                    \
  } while (0)
  if (dt == DType::BF16) {
    if (hd == 128) L_(bf16_t, 128); else L_(bf16_t, 64);
  } else {
    if (hd == 128) L_(f16_t, 128); else L_(f16_t, 64);
  }
#undef L_
}

// ------------------------------------------------------------------ append + decode, partial pass
// RT query heads of one kv group per workgroup (H/G = RT * SUB, blockIdx.y = g * SUB + sub).
// po [B, H, NCH, HD] unnormalised outputs, pml [B, H, NCH, 2] (max, exp-sum): the layout of
// attn_decode_split.hip, merged by its combine kernel.
template <typename T, int HD, int RT>
__global__ __launch_bounds__(SPL_THREADS) void attn_decode_fp8_partial_k(
    const T* __restrict__ qkv, uint8_t* __restrict__ k8, float* __restrict__ ks, uint8_t* __restrict__ v8,
    float* __restrict__ vs, float* __restrict__ po, float* __restrict__ pml, int H, int G, int Tmax, int NCH,
    float scale, const int* __restrict__ pos, long qs) {
  constexpr int VEC = 8;                       // q elements per 16-B load; V bytes per 8-B load
  constexpr int NC = HD / VEC;                 // pieces per q row / per V row
  constexpr int KC = HD / 16;                  // 16-B pieces of a K row
  constexpr int KG = SPL_THREADS / NC;         // lane groups of the output pass
  constexpr int KPL = SPL_CHUNK / KG;          // keys per lane group
  constexpr int RP = RT < 4 ? RT : 4;          // heads per LDS reduction round
  constexpr int NW = SPL_THREADS / 64;
  static_assert(SPL_CHUNK == SPL_THREADS && RT % RP == 0 && HD / 2 <= 64, "one key per thread in the score pass");
  __shared__ __align__(16) uint4 s_q[RT][NC];            // the heads' q rows, as loaded
  __shared__ __align__(16) float s_p[SPL_CHUNK][RT];     // probabilities times the key's V scale
  __shared__ __align__(16) float s_part[RP][KG][HD];
  __shared__ float s_m[NW][RT];
  __shared__ float s_l[NW][RT];
  __shared__ __align__(16) uint8_t s_n8[2][HD];          // the appended k and v rows, quantised
  __shared__ float s_ns[2];                              // and their scales

  const int chunk = blockIdx.x, b = blockIdx.z;
  const int R = H / G, SUB = R / RT;
  const int g = blockIdx.y / SUB, sub = blockIdx.y % SUB;
  const int h0 = g * R + sub * RT;
  const int tid = threadIdx.x, ci = tid % NC, j = tid / NC, lane = tid & 63, w = tid >> 6;
  int p = pos[b];
  BLLM_DASSERT(p >= 0 && p < Tmax, DBG_DECODE_POS);
  p = p < 0 ? 0 : (p >= Tmax ? Tmax - 1 : p);
  const int L = p + 1;
  const int k0 = chunk * SPL_CHUNK;
  if (k0 >= L) return;
  const bool last = k0 + SPL_CHUNK >= L;        // this chunk holds the appended key p (uniform)

  const long rb = ((long)b * G + g) * (long)Tmax;   // first cache row of (b, g)
  const uint8_t* kb = k8 + rb * HD;
  const uint8_t* vb = v8 + rb * HD;
  if (tid < RT * NC) {
    const int r = tid / NC;
    s_q[r][ci] = *reinterpret_cast<const uint4*>(qkv + (long)b * qs + (long)(h0 + r) * HD + ci * VEC);
  }

  // All loads first.  Score pass: thread = key k0 + tid, its whole K row and both of its scales.
  // Output pass: thread = (piece ci, lane group j), the V pieces of keys k0 + i * KG + j.  Keys
  // at or beyond L - 1 are never loaded: the appended one comes from LDS below.
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  uint4 kr[KC];
  uint2 vv[KPL];
  const int key = k0 + tid;
  float ksc = 0.f, vsc = 0.f;
#pragma unroll
  for (int i = 0; i < KC; ++i) kr[i] = zero;
  if (key < p) {
#pragma unroll
    for (int i = 0; i < KC; ++i) kr[i] = *reinterpret_cast<const uint4*>(kb + (long)key * HD + i * 16);
    ksc = ks[rb + key];
    vsc = vs[rb + key];
  }
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    const int k = k0 + i * KG + j;
    vv[i] = make_uint2(0u, 0u);
    if (k < p) vv[i] = *reinterpret_cast<const uint2*>(vb + (long)k * HD + ci * VEC);
  }
  if (last && w < 2) {  // wave 0 quantises the new k, wave 1 the new v: two elements per lane
    const T* src = qkv + (long)b * qs + (long)(H + (w == 0 ? 0 : G) + g) * HD;
    float x0 = 0.f, x1 = 0.f;
    if (lane < HD / 2) {
      x0 = to_f(src[2 * lane]);
      x1 = to_f(src[2 * lane + 1]);
    }
    const float a = wave_max(fmaxf(fabsf(x0), fabsf(x1)));
    const float s = f8_scale(a);
    if (lane < HD / 2) reinterpret_cast<uint16_t*>(&s_n8[w][0])[lane] = (uint16_t)f8_pack2(x0, x1, s);
    if (lane == 0) s_ns[w] = s;
  }
  __syncthreads();
  if (last) {
    if (key == p) {
#pragma unroll
      for (int i = 0; i < KC; ++i) kr[i] = *reinterpret_cast<const uint4*>(&s_n8[0][i * 16]);
      ksc = s_ns[0];
      vsc = s_ns[1];
    }
#pragma unroll
    for (int i = 0; i < KPL; ++i)
      if (k0 + i * KG + j == p) vv[i] = *reinterpret_cast<const uint2*>(&s_n8[1][ci * VEC]);
    if (sub == 0) {  // one workgroup per (row, kv group) stores the appended row and its scales
      if (tid < 2 * KC) {
        const int kv = tid / KC, c = tid % KC;
        *reinterpret_cast<uint4*>((kv == 0 ? k8 : v8) + (rb + p) * HD + c * 16) =
            *reinterpret_cast<const uint4*>(&s_n8[kv][c * 16]);
      } else if (tid < 2 * KC + 2) {
        const int kv = tid - 2 * KC;
        (kv == 0 ? ks : vs)[rb + p] = s_ns[kv];
      }
    }
  }

  // the K row as packed pairs of T, converted once for all heads
  uint32_t kp[HD / 2];
#pragma unroll
  for (int i = 0; i < KC; ++i) {
    const uint32_t d[4] = {kr[i].x, kr[i].y, kr[i].z, kr[i].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      kp[i * 8 + e * 2] = f8_pair<T, false>(d[e]);
      kp[i * 8 + e * 2 + 1] = f8_pair<T, true>(d[e]);
    }
  }
  // scores (log2 domain) of this thread's key against every head
  const float c = scale * kLog2e * ksc;
  float s[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const uint4 qv = s_q[r][i];
      t = spl_dot2<T>(kp[i * 4], qv.x, t);
      t = spl_dot2<T>(kp[i * 4 + 1], qv.y, t);
      t = spl_dot2<T>(kp[i * 4 + 2], qv.z, t);
      t = spl_dot2<T>(kp[i * 4 + 3], qv.w, t);
    }
    s[r] = key < L ? t * c : -INFINITY;
    const float mw = wave_max(s[r]);
    if (lane == 0) s_m[w][r] = mw;
  }
  __syncthreads();
  // probabilities against the chunk's max, and their sums; the V scale rides on the probability
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    float M = s_m[0][r];
#pragma unroll
    for (int i = 1; i < NW; ++i) M = fmaxf(M, s_m[i][r]);
    const float pr = __builtin_amdgcn_exp2f(s[r] - (M == -INFINITY ? 0.f : M));
    s_p[tid][r] = pr * vsc;
    const float lw = wave_sum(pr);
    if (lane == 0) s_l[w][r] = lw;
  }
  __syncthreads();

  // out[r][d] = sum_k (p[k][r] Vs[k]) V8[k][d] over this lane group's keys
  float acc[RT][VEC];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[r][e] = 0.f;
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    typedef __attribute__((ext_vector_type(2))) float v2f;
    const v2f f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vv[i].x, false);
    const v2f f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vv[i].x, true);
    const v2f f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vv[i].y, false);
    const v2f f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vv[i].y, true);
    const float vf[VEC] = {f0[0], f0[1], f1[0], f1[1], f2[0], f2[1], f3[0], f3[1]};
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const float pv = s_p[i * KG + j][r];
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[r][e] += pv * vf[e];
    }
  }
  // lane groups summed through LDS in ascending order, RP heads per round
#pragma unroll
  for (int r0 = 0; r0 < RT; r0 += RP) {
    if (r0 > 0) __syncthreads();
#pragma unroll
    for (int r = 0; r < RP; ++r) {
      float4* dst = reinterpret_cast<float4*>(&s_part[r][j][ci * VEC]);
      dst[0] = make_float4(acc[r0 + r][0], acc[r0 + r][1], acc[r0 + r][2], acc[r0 + r][3]);
      dst[1] = make_float4(acc[r0 + r][4], acc[r0 + r][5], acc[r0 + r][6], acc[r0 + r][7]);
    }
    __syncthreads();
    for (int idx = tid; idx < RP * HD; idx += SPL_THREADS) {
      const int r = idx / HD, d = idx % HD;
      float o = 0.f;
#pragma unroll 8
      for (int g2 = 0; g2 < KG; ++g2) o += s_part[r][g2][d];
      const long slot = ((long)b * H + h0 + r0 + r) * NCH + chunk;
      po[slot * HD + d] = o;
      if (d == 0) {
        float M = s_m[0][r0 + r], ls = s_l[0][r0 + r];
#pragma unroll
        for (int i = 1; i < NW; ++i) {
          M = fmaxf(M, s_m[i][r0 + r]);
          ls += s_l[i][r0 + r];
        }
        pml[slot * 2] = M;
        pml[slot * 2 + 1] = ls;
      }
    }
  }
}

// query heads of a kv group per workgroup: as attn_decode_split.hip (attn_decode_split_grid_ok)
static int f8_heads(int R) { return R % 8 == 0 ? 8 : R % 4 == 0 ? 4 : R % 2 == 0 ? 2 : 1; }

template <typename T, int HD>
static void f8_launch(const T* qkv, uint8_t* k8, float* ks, uint8_t* v8, float* vs, float* ws, const int* pos, int B,
                      int H, int G, int Tmax, hipStream_t s) {
  const float scale = 1.f / sqrtf((float)HD);
  const int NCH = (int)(((long)Tmax + SPL_CHUNK - 1) / SPL_CHUNK);  // attn_decode_split_workspace's chunk count
  float* po = ws;
  float* pml = ws + (long)B * H * NCH * HD;
  const long qs = (long)(H + 2 * G) * HD;
  const int R = H / G, RT = f8_heads(R);
  dim3 grid(NCH, G * (R / RT), B), block(SPL_THREADS);
#define P_(RTT) hipLaunchKernelGGL((attn_decode_fp8_partial_k<T, HD, RTT>), grid, block, 0, s, qkv, k8, ks, v8, vs, \
                                   po, pml, H, G, Tmax, NCH, scale, pos, qs)
  switch (RT) {
    case 8: P_(8); break;
    case 4: P_(4); break;
    case 2: P_(2); break;
    default: P_(1); break;
  }
#undef P_
}

void attn_decode_append_rows_fp8(DType dt, const void* qkv, void* k8, float* ks, void* v8, float* vs, void* out,
                                 float* ws, const int* pos, int B, int H, int G, int hd, int Tmax, hipStream_t s) {
#define L_(TT, HDD) f8_launch<TT, HDD>((const TT*)qkv, (uint8_t*)k8, ks, (uint8_t*)v8, vs, ws, pos, B, H, G, Tmax, s)
  if (dt == DType::BF16) {
    if (hd == 128) L_(bf16_t, 128); else L_(bf16_t, 64);
  } else {
    if (hd == 128) L_(f16_t, 128); else L_(f16_t, 64);
  }
#undef L_
  attn_decode_split_combine_rows(dt, ws, out, pos, B, H, hd, Tmax, s);
}

}  // namespace bllm
