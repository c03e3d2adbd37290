// Split-KV single-query attention against a KV cache of any length (long-context decode), gfx950.
//
// attn_decode.hip keeps every score of a (row, head) in LDS (at most 8,192 keys) and runs one
// workgroup per (row, query head): at a long cache that is few workgroups, and every query head of
// a kv group re-reads the group's K/V rows.  Here the keys are cut into chunks of SPL_CHUNK and the
// work into two launches, with no atomics and no hand-off between workgroups inside a launch:
//
//   partial  grid (key chunk, kv group, batch row), 256 threads.  The workgroup reads its chunk of
//            the group's K and V rows once, for all H/G query heads of the group, straight to
//            VGPRs and all loads up front.  Scores: one key per thread, its K row dotted with
//            every head's q (q in LDS, packed 16-bit dot products into fp32); the chunk's max and
//            the probabilities against it go through LDS.  Outputs: a lane owns one 16-B piece
//            of V rows (HD/8 lanes per key, so a wave load is 1 KiB contiguous) for every head;
//            the lane groups are summed through LDS in a fixed order.  Per (row, head, chunk):
//            max (log2 domain), exp-sum, unnormalised fp32 output.
//   combine  grid (batch row x query head).  Merges the partials of chunks 0 .. ceil(L/chunk) - 1
//            (never a slot that this step did not write): the max over them, then the weighted
//            sums over contiguous ascending chunk ranges, the ranges added in ascending order.
//
// The chunk size and count come from Tmax on the host; the position is read from device memory
// (graph replay), and a workgroup whose chunk starts at or beyond L leaves before any other load
// or store.  Forms as in attn_decode.hip: plain (q [B, H, hd], host L) and APPEND (q / new k /
// new v from the token's packed qkv row, position *pos shared or pos[b] per row; chunk 0's first
// workgroup of each (row, kv group) writes the new k / v to cache row pos, which nothing in
// either launch reads: key L - 1 is taken from the qkv row).  fp32 accumulation throughout; the
// result does not depend on workgroup scheduling.
#include "api.h"
#include "attn_decode_split.h"

namespace bllm {

BLLM_DEBUG_WORD(attn_decode_split)

// the length this launch attends over: host L, or position + 1 (kept inside the cache)
template <bool APPEND>
__device__ __forceinline__ int spl_len(int L, const int* __restrict__ pos, int pos_stride, int b, int Tmax) {
  if constexpr (APPEND) {
    int p = pos[(long)b * pos_stride];
    BLLM_DASSERT(p >= 0 && p < Tmax, DBG_DECODE_POS);
    p = p < 0 ? 0 : (p >= Tmax ? Tmax - 1 : p);
    return p + 1;
  } else {
    return L < Tmax ? L : Tmax;
  }
}

// RT query heads of one kv group per workgroup (H/G = RT * SUB, blockIdx.y = g * SUB + sub).
// po [B, H, NCH, HD] unnormalised outputs, pml [B, H, NCH, 2] (max, exp-sum).
template <typename T, int HD, int RT, bool APPEND>
__global__ __launch_bounds__(SPL_THREADS) void attn_decode_split_partial_k(
    const T* __restrict__ q, T* __restrict__ kc, T* __restrict__ vc, float* __restrict__ po,
    float* __restrict__ pml, int H, int G, int Tmax, int NCH, int Lhost, float scale, const int* __restrict__ pos,
    int pos_stride, long qs) {
  constexpr int VEC = 8;                       // elements per 16-B load
  constexpr int NC = HD / VEC;                 // 16-B pieces per row
  constexpr int KG = SPL_THREADS / NC;         // lane groups of the output pass
  constexpr int KPL = SPL_CHUNK / KG;          // keys per lane group
  constexpr int RP = RT < 4 ? RT : 4;          // heads per LDS reduction round
  constexpr int NW = SPL_THREADS / 64;
  static_assert(SPL_CHUNK == SPL_THREADS && RT % RP == 0, "one key per thread in the score pass");
  __shared__ __align__(16) uint4 s_q[RT][NC];            // the heads' q rows, as loaded
  __shared__ __align__(16) float s_p[SPL_CHUNK][RT];     // scores, then probabilities
  __shared__ __align__(16) float s_part[RP][KG][HD];
  __shared__ float s_m[NW][RT];
  __shared__ float s_l[NW][RT];

  const int chunk = blockIdx.x, b = blockIdx.z;
  const int R = H / G, SUB = R / RT;
  const int g = blockIdx.y / SUB, sub = blockIdx.y % SUB;
  const int h0 = g * R + sub * RT;
  const int tid = threadIdx.x, ci = tid % NC, j = tid / NC, lane = tid & 63, w = tid >> 6;
  const int L = spl_len<APPEND>(Lhost, pos, pos_stride, b, Tmax);
  const int k0 = chunk * SPL_CHUNK;
  if (k0 >= L) return;

  T* kb = kc + ((long)b * G + g) * (long)Tmax * HD;
  T* vb = vc + ((long)b * G + g) * (long)Tmax * HD;
  const T* knew = nullptr;
  const T* vnew = nullptr;
  if constexpr (APPEND) {
    knew = q + (long)b * qs + (long)(H + g) * HD;
    vnew = q + (long)b * qs + (long)(H + G + g) * HD;
    if (chunk == 0 && sub == 0 && tid < 2 * NC) {  // one workgroup per (row, kv group) appends k and v
      if (tid < NC) st16(kb + (long)(L - 1) * HD + ci * VEC, ld16(knew + ci * VEC));
      else st16(vb + (long)(L - 1) * HD + ci * VEC, ld16(vnew + ci * VEC));
    }
  }
  if (tid < RT * NC) {
    const int r = tid / NC;
    const T* qr = APPEND ? q + (long)b * qs + (long)(h0 + r) * HD : q + ((long)b * H + h0 + r) * HD;
    s_q[r][ci] = *reinterpret_cast<const uint4*>(qr + ci * VEC);
  }

  // All loads first.  Score pass: thread = key k0 + tid, its whole K row.  Output pass: thread =
  // (piece ci, lane group j), the V pieces of keys k0 + i * KG + j (a wave load is 1 KiB
  // contiguous).  Keys at or beyond L are never loaded; the appended key comes from the qkv row.
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  uint4 kr[NC], vv[KPL];
  const int key = k0 + tid;
  {
    const T* krow = (APPEND && key == L - 1) ? knew : kb + (long)key * HD;
#pragma unroll
    for (int i = 0; i < NC; ++i) kr[i] = zero;
    if (key < L) {
#pragma unroll
      for (int i = 0; i < NC; ++i) kr[i] = *reinterpret_cast<const uint4*>(krow + i * VEC);
    }
  }
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    const int k = k0 + i * KG + j;
    vv[i] = zero;
    if (k < L) vv[i] = *reinterpret_cast<const uint4*>(((APPEND && k == L - 1) ? vnew : vb + (long)k * HD) + ci * VEC);
  }
  __syncthreads();

  // scores (log2 domain) of this thread's key against every head
  const float c = scale * kLog2e;
  float s[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const uint4 qv = s_q[r][i];
      t = spl_dot2<T>(kr[i].x, qv.x, t);
      t = spl_dot2<T>(kr[i].y, qv.y, t);
      t = spl_dot2<T>(kr[i].z, qv.z, t);
      t = spl_dot2<T>(kr[i].w, qv.w, t);
    }
    s[r] = key < L ? t * c : -INFINITY;
    const float mw = wave_max(s[r]);
    if (lane == 0) s_m[w][r] = mw;
  }
  __syncthreads();
  // probabilities against the chunk's max, and their sums
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    float M = s_m[0][r];
#pragma unroll
    for (int i = 1; i < NW; ++i) M = fmaxf(M, s_m[i][r]);
    const float p = __builtin_amdgcn_exp2f(s[r] - (M == -INFINITY ? 0.f : M));
    s_p[tid][r] = p;
    const float lw = wave_sum(p);
    if (lane == 0) s_l[w][r] = lw;
  }
  __syncthreads();

  // out[r][d] = sum_k p[k][r] V[k][d] over this lane group's keys
  float acc[RT][VEC];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[r][e] = 0.f;
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    const Vec16<T> v = __builtin_bit_cast(Vec16<T>, vv[i]);
    float vf[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) vf[e] = to_f(v.v[e]);
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const float p = s_p[i * KG + j][r];
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[r][e] += p * vf[e];
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

// One workgroup per (row, head): thread = (4 output columns, chunk range).
template <typename T, int HD, bool APPEND>
__global__ __launch_bounds__(SPL_THREADS) void attn_decode_split_combine_k(
    const float* __restrict__ po, const float* __restrict__ pml, T* __restrict__ out, int H, int Tmax, int NCH,
    int Lhost, const int* __restrict__ pos, int pos_stride) {
  constexpr int D4 = HD / 4;             // float4 columns
  constexpr int NR = SPL_THREADS / D4;   // chunk ranges
  constexpr int NW = SPL_THREADS / 64;
  __shared__ float s_red[NW];
  __shared__ __align__(16) float s_acc[NR][HD];
  __shared__ float s_ls[NR];
  const int bh = blockIdx.x, b = bh / H, tid = threadIdx.x;
  const int L = spl_len<APPEND>(Lhost, pos, pos_stride, b, Tmax);
  int n = (L + SPL_CHUNK - 1) / SPL_CHUNK;  // chunks the partial pass wrote for this row
  n = n < NCH ? n : NCH;
  const float* ml = pml + (long)bh * NCH * 2;
  const float* o = po + (long)bh * NCH * HD;

  float mx = -INFINITY;
  for (int ch = tid; ch < n; ch += SPL_THREADS) mx = fmaxf(mx, ml[2 * ch]);
  mx = wave_max(mx);
  if ((tid & 63) == 0) s_red[tid >> 6] = mx;
  __syncthreads();
  mx = s_red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) mx = fmaxf(mx, s_red[i]);
  const float M = mx == -INFINITY ? 0.f : mx;

  const int d4 = tid % D4, rg = tid / D4;
  const int per = (n + NR - 1) / NR;
  const int c0 = rg * per, c1 = c0 + per < n ? c0 + per : n;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, ls = 0.f;
#pragma unroll 4
  for (int ch = c0; ch < c1; ++ch) {
    const float2 x = *reinterpret_cast<const float2*>(ml + 2 * ch);
    const float4 v = *reinterpret_cast<const float4*>(o + (long)ch * HD + d4 * 4);
    const float wt = exp2f(x.x - M);
    ls += wt * x.y;
    a0 += wt * v.x;
    a1 += wt * v.y;
    a2 += wt * v.z;
    a3 += wt * v.w;
  }
  *reinterpret_cast<float4*>(&s_acc[rg][d4 * 4]) = make_float4(a0, a1, a2, a3);
  if (d4 == 0) s_ls[rg] = ls;
  __syncthreads();
  for (int d = tid; d < HD; d += SPL_THREADS) {
    float ov = 0.f, lv = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      ov += s_acc[r][d];
      lv += s_ls[r];
    }
    out[(long)bh * HD + d] = from_f<T>(ov / lv);
  }
}

int attn_decode_split_chunk() { return SPL_CHUNK; }
int attn_decode_split_chunks(int Tmax) { return (int)(((long)Tmax + SPL_CHUNK - 1) / SPL_CHUNK); }
long attn_decode_split_workspace(int B, int H, int hd, int Tmax) {
  return (long)B * H * attn_decode_split_chunks(Tmax) * (hd + 2);
}

// query heads of a kv group per workgroup: the largest of 8, 4, 2, 1 that divides H / G
static int spl_heads(int R) { return R % 8 == 0 ? 8 : R % 4 == 0 ? 4 : R % 2 == 0 ? 2 : 1; }

bool attn_decode_split_grid_ok(int B, int H, int G) {
  const int R = H / G;
  return B <= 65535 && (long)G * (R / spl_heads(R)) <= 65535;
}

template <typename T, int HD, bool APPEND>
static void spl_launch(const T* q, T* kc, T* vc, T* out, float* ws, const int* pos, int pos_stride, int B, int H,
                       int G, int Tmax, int L, hipStream_t s) {
  const float scale = 1.f / sqrtf((float)HD);
  const int NCH = attn_decode_split_chunks(Tmax);
  float* po = ws;
  float* pml = ws + (long)B * H * NCH * HD;
  const long qs = APPEND ? (long)(H + 2 * G) * HD : 0L;
  const int R = H / G, RT = spl_heads(R);
  dim3 grid(NCH, G * (R / RT), B), block(SPL_THREADS);
#define P_(RTT) hipLaunchKernelGGL((attn_decode_split_partial_k<T, HD, RTT, APPEND>), grid, block, 0, s, q, kc, vc, \
                                   po, pml, H, G, Tmax, NCH, L, scale, pos, pos_stride, qs)
  switch (RT) {
    case 8: P_(8); break;
    case 4: P_(4); break;
    case 2: P_(2); break;
    default: P_(1); break;
  }
#undef P_
  hipLaunchKernelGGL((attn_decode_split_combine_k<T, HD, APPEND>), dim3(B * H), block, 0, s, po, pml, out, H, Tmax,
                     NCH, L, pos, pos_stride);
}

template <bool APPEND>
static void spl_dispatch(DType dt, const void* q, void* kc, void* vc, void* out, float* ws, const int* pos,
                         int pos_stride, int B, int H, int G, int hd, int Tmax, int L, hipStream_t s) {
#define L_(TT, HDD) spl_launch<TT, HDD, APPEND>((const TT*)q, (TT*)kc, (TT*)vc, (TT*)out, ws, pos, pos_stride, B, H, \
                                                G, Tmax, L, s)
  if (dt == DType::BF16) {
    if (hd == 128) L_(bf16_t, 128); else L_(bf16_t, 64);
  } else {
    if (hd == 128) L_(f16_t, 128); else L_(f16_t, 64);
  }
#undef L_
}

void attn_decode_split(DType dt, const void* q, const void* kc, const void* vc, void* out, float* ws, int B, int H,
                       int G, int hd, int Tmax, int L, hipStream_t s) {
  spl_dispatch<false>(dt, q, const_cast<void*>(kc), const_cast<void*>(vc), out, ws, nullptr, 0, B, H, G, hd, Tmax, L,
                      s);
}

void attn_decode_append_split(DType dt, const void* qkv, void* kc, void* vc, void* out, float* ws, const int* pos,
                              int pos_stride, int B, int H, int G, int hd, int Tmax, hipStream_t s) {
  spl_dispatch<true>(dt, qkv, kc, vc, out, ws, pos, pos_stride, B, H, G, hd, Tmax, 0, s);
}

// The merge alone, per-row positions: for a partial pass that lives in another file and writes the
// same workspace layout (attn_decode_fp8.hip).  Two template levels, as spl_dispatch / spl_launch:
// the kernels are then instantiated after those of the two entry points above, which keeps the
// order of the kernels in the code object (tools/isa_diff.py compares it as a text).
template <typename T, int HD>
static void spl_combine_launch(const float* ws, T* out, const int* pos, int B, int H, int Tmax, hipStream_t s) {
  const int NCH = attn_decode_split_chunks(Tmax);
  hipLaunchKernelGGL((attn_decode_split_combine_k<T, HD, true>), dim3(B * H), dim3(SPL_THREADS), 0, s, ws,
                     ws + (long)B * H * NCH * HD, out, H, Tmax, NCH, 0, pos, 1);
}

template <bool ROWS>
static void spl_combine_dispatch(DType dt, const float* ws, void* out, const int* pos, int B, int H, int hd, int Tmax,
                                 hipStream_t s) {
  static_assert(ROWS, "a position per row");
  if (dt == DType::BF16) {
    if (hd == 128) spl_combine_launch<bf16_t, 128>(ws, (bf16_t*)out, pos, B, H, Tmax, s);
    else spl_combine_launch<bf16_t, 64>(ws, (bf16_t*)out, pos, B, H, Tmax, s);
  } else {
    if (hd == 128) spl_combine_launch<f16_t, 128>(ws, (f16_t*)out, pos, B, H, Tmax, s);
    else spl_combine_launch<f16_t, 64>(ws, (f16_t*)out, pos, B, H, Tmax, s);
  }
}

void attn_decode_split_combine_rows(DType dt, const float* ws, void* out, const int* pos, int B, int H, int hd,
                                    int Tmax, hipStream_t s) {
  spl_combine_dispatch<true>(dt, ws, out, pos, B, H, hd, Tmax, s);
}

}  // namespace bllm
