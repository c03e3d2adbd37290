// Attention of Q new tokens per row over a KV cache (the verify step of speculative decoding),
// gfx950.  Row b brings Q tokens at positions pos[b] .. pos[b] + Q - 1 (packed qkv rows b Q + j,
// RoPE applied); their K / V go into cache rows pos[b] + j and query j attends over keys
// 0 .. pos[b] + j: by definition what Q consecutive attn_decode_append_rows calls give.
//
// Split-KV at every length, on the workspace layout of attn_decode_split.h with the B Q
// (row, token) pairs as the workspace's rows, so the merge is attn_decode_split.hip's combine
// kernel, unchanged, given the int32 [B Q] vector pos[b] + j:
//
//   partial  grid (key chunk, kv group, batch row), 256 threads = 4 waves of 64 keys.  The
//            workgroup reads its chunk of the group's K and V rows once for all Q H/G query
//            vectors of the group (at most 32: one MFMA tile of queries).  S^T = K Q^T on
//            v_mfma_f32_32x32x16: the K fragments are 16-B global loads of the key rows, the Q
//            fragments 16-B loads of the qkv rows (both straight to VGPRs, all loads up front).
//            The chunk's max per query goes through LDS, the probabilities are packed from the
//            accumulators (as attn_fwd_kernel.h does), and O^T += V^T P^T reads V^T with
//            transposed LDS reads from the transposed image of attn_tiles.h (a wave stages its
//            own 32 keys at a time, 16-B pieces, swizzle on the source chunk).  The four waves'
//            outputs are summed through LDS in ascending wave order.  Per (row, token, head,
//            chunk): max (log2 domain), exp-sum, unnormalised fp32 output.
//   combine  attn_decode_split_combine_rows over B Q rows.
//
// Keys pos[b] .. pos[b] + Q - 1 are taken from the qkv rows, never from the cache: chunk 0's
// workgroup of each (row, kv group) writes them to the cache, and nothing in either launch reads
// what the launch writes there.  Keys at or beyond pos[b] + Q are never loaded (their fragments
// are zero), so what the cache holds there does not matter.  A workgroup whose chunk starts
// beyond every query's last key leaves before any other load or store; an active one writes the
// slots of exactly the queries whose last key is at or beyond the chunk's first, which are the
// slots the combine reads.  No atomics, fp32 accumulation, fixed summation order; row b's output
// and cache rows depend on row b alone.
#include "api.h"
#include "attn_decode_split.h"
#include "attn_tiles.h"
#include "mma.h"

namespace bllm {

BLLM_DEBUG_WORD(attn_extend)

constexpr int EXT_NQ = 32;    // query vectors per workgroup: one 32-column MFMA tile
constexpr int EXT_MAX_Q = 8;

template <typename T, int HD>
__global__ __launch_bounds__(SPL_THREADS) void attn_extend_partial_k(
    const T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc, float* __restrict__ po,
    float* __restrict__ pml, const int* __restrict__ pos, int Q, int H, int G, int Tmax, int NCH, float c) {
  typedef typename Mma<T>::v8 v8;
  constexpr int KK = HD / 16;                  // k-steps of the QK^T product
  constexpr int DT = HD / 32;                  // 32-row tiles of O^T
  constexpr int CH = HD / 8;                   // 16-B chunks per row
  constexpr int ROWB = HD * 2;
  constexpr int NW = SPL_THREADS / 64;
  constexpr int WK = SPL_CHUNK / NW;           // keys per wave
  constexpr int NKT = WK / 32;                 // 32-key MFMA tiles per wave
  constexpr int VLD = 32 * CH / 64;            // 16-B pieces per lane of one 32-key V tile
  constexpr int VTILE = 32 * ROWB;             // bytes of a wave's staged V tile
  constexpr int OWAVE = DT * 4 * 64 * 16;      // bytes of a wave's output accumulators
  constexpr int SBUF = NW * VTILE > (NW - 1) * OWAVE ? NW * VTILE : (NW - 1) * OWAVE;
  static_assert(SPL_CHUNK == 256 && NKT == 2, "four waves of two 32-key tiles");
  __shared__ __align__(16) char s_buf[SBUF];   // V tiles, then the waves' outputs
  __shared__ float s_m[NW][EXT_NQ];
  __shared__ float s_l[NW][EXT_NQ];

  const int chunk = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int p = pos[b];
  BLLM_DASSERT(p >= 0 && p + Q <= Tmax, DBG_DECODE_POS);
  p = p < 0 ? 0 : (p > Tmax - Q ? Tmax - Q : p);
  const int Lmax = p + Q;                      // keys of the last query
  const int k0 = chunk * SPL_CHUNK;
  if (k0 >= Lmax) return;

  const int R = H / G, NQ = Q * R;
  const long qs = (long)(H + 2 * G) * HD;
  const T* rows = qkv + (long)b * Q * qs;      // the row's Q packed tokens
  T* kb = kc + ((long)b * G + g) * (long)Tmax * HD;
  T* vb = vc + ((long)b * G + g) * (long)Tmax * HD;
  const long koff = (long)(H + g) * HD, voff_g = (long)(H + G + g) * HD;

  // the Q new k / v rows -> cache rows p .. p + Q - 1 (one workgroup per (row, kv group))
  if (chunk == 0) {
    for (int i = tid; i < Q * 2 * CH; i += SPL_THREADS) {
      const int j = i / (2 * CH), rem = i % (2 * CH), ci = rem % CH;
      if (rem < CH) st16(kb + (long)(p + j) * HD + ci * 8, ld16(rows + j * qs + koff + ci * 8));
      else st16(vb + (long)(p + j) * HD + ci * 8, ld16(rows + j * qs + voff_g + ci * 8));
    }
  }

  // ---- all loads first.  Key k: cache row k below p, the qkv row of token k - p from p on,
  //      nothing (zero) from Lmax on.
  const int kw0 = k0 + w * WK;                 // this wave's first key
  const int qn = l32, qj = qn / R, qr = qn % R;  // this lane's query vector: token qj, head g R + qr
  const bool qok = qn < NQ;
  v8 qf[KK];
  {
    const T* qrow = rows + (long)(qok ? qj : 0) * qs + (long)(g * R + (qok ? qr : 0)) * HD + hh * 8;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      qf[kk] = v8{};
      if (qok) qf[kk] = *reinterpret_cast<const v8*>(qrow + kk * 16);
    }
  }
  v8 kf[NKT][KK];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    const int key = kw0 + kt * 32 + l32;
    const T* krow = (key >= p ? rows + (long)(key < Lmax ? key - p : 0) * qs + koff : kb + (long)key * HD) + hh * 8;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      kf[kt][kk] = v8{};
      if (key < Lmax) kf[kt][kk] = *reinterpret_cast<const v8*>(krow + kk * 16);
    }
  }
  // V piece i of tile kt: P = i 64 + lane lands at byte 16 P of the wave's tile = physical chunk
  // P % CH of row P / CH; the lane fetches the logical chunk that belongs there
  uint4 vr[NKT][VLD];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int i = 0; i < VLD; ++i) {
      const int P = i * 64 + lane, r = P / CH, pc = P % CH;
      const int key = kw0 + kt * 32 + r;
      const int c16 = BLLM_TR_IMG_SRC16(HD, r, pc);
      const T* vrow = key >= p ? rows + (long)(key < Lmax ? key - p : 0) * qs + voff_g : vb + (long)key * HD;
      vr[kt][i] = make_uint4(0u, 0u, 0u, 0u);
      if (key < Lmax) vr[kt][i] = *reinterpret_cast<const uint4*>(vrow + c16 * 8);
    }

  // ---- S^T = K Q^T: lane (l32, hh) holds query l32, keys (r & 3) + 8 (r >> 2) + 4 hh of the tile
  f32x16 s[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    s[kt] = f32x16{};
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) s[kt] = Mma<T>::mma(kf[kt][kk], qf[kk], s[kt]);
  }
  // mask: query (token qj) sees keys 0 .. p + qj; a padding column sees nothing
  const int lim = (qok ? p + qj : -1) - (kw0 + 4 * hh);
  float mx = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = kt * 32 + (r & 3) + 8 * (r >> 2) > lim ? -INFINITY : s[kt][r] * c;
      s[kt][r] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if (hh == 0) s_m[w][l32] = mx;
  __syncthreads();
  // probabilities against the chunk's max, and the wave's sum
  float M = s_m[0][l32];
#pragma unroll
  for (int i = 1; i < NW; ++i) M = fmaxf(M, s_m[i][l32]);
  const float Ms = M == -INFINITY ? 0.f : M;
  float ls = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pv = __builtin_amdgcn_exp2f(s[kt][r] - Ms);
      s[kt][r] = pv;
      ls += pv;
    }
  ls += __shfl_xor(ls, 32, 64);
  if (hh == 0) s_l[w][l32] = ls;

  // ---- O^T += V^T P^T over the wave's keys: P fragments packed from the accumulators, V^T by
  //      transposed reads of the wave's staged tile
  const int gi = lane & 15, gl = (lane >> 4) & 1, qrow = gi >> 2, pcol = gi & 3;
  int voff[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) voff[dt] = tr_img_off<HD>(4 * hh + qrow, dt * 32 + gl * 16 + pcol * 4);
  char* vtile = s_buf + w * VTILE;
  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x16{};
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    if (kt > 0) __syncthreads();               // the previous tile's reads are done
#pragma unroll
    for (int i = 0; i < VLD; ++i) *reinterpret_cast<uint4*>(vtile + (i * 64 + lane) * 16) = vr[kt][i];
    __syncthreads();
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      uint32_t uu[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) uu[e] = pack2<T>(s[kt][8 * s2 + 2 * e], s[kt][8 * s2 + 2 * e + 1]);
      v8 pf;
      __builtin_memcpy(&pf, uu, 16);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int off = voff[dt] + s2 * 16 * ROWB;
        o[dt] = Mma<T>::mma(tr_read8<v8>(vtile, off, off + 8 * ROWB), pf, o[dt]);
      }
    }
  }

  // ---- the waves' outputs summed in ascending wave order: waves 1 .. 3 through LDS (lane-linear
  //      16-B pieces, read back by the same lane of wave 0)
  __syncthreads();                             // every V tile read is done: s_buf changes hands
  if (w > 0) {
    float4* dst = reinterpret_cast<float4*>(s_buf + (w - 1) * OWAVE);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq)
        dst[(dt * 4 + rq) * 64 + lane] =
            make_float4(o[dt][4 * rq], o[dt][4 * rq + 1], o[dt][4 * rq + 2], o[dt][4 * rq + 3]);
  }
  __syncthreads();
  if (w > 0) return;
  // this query's slot exists iff its last key is at or beyond the chunk's first
  if (!qok || k0 > p + qj) return;
  const long slot = (((long)b * Q + qj) * H + g * R + qr) * NCH + chunk;
  float* orow = po + slot * HD;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      float4 a = make_float4(o[dt][4 * rq], o[dt][4 * rq + 1], o[dt][4 * rq + 2], o[dt][4 * rq + 3]);
#pragma unroll
      for (int ww = 1; ww < NW; ++ww) {
        const float4 x = reinterpret_cast<const float4*>(s_buf + (ww - 1) * OWAVE)[(dt * 4 + rq) * 64 + lane];
        a.x += x.x;
        a.y += x.y;
        a.z += x.z;
        a.w += x.w;
      }
      // accumulator rows (r & 3) + 8 (r >> 2) + 4 hh of tile dt = output columns d
      *reinterpret_cast<float4*>(orow + dt * 32 + 8 * rq + 4 * hh) = a;
    }
  if (hh == 0) {
    float lt = s_l[0][l32];
#pragma unroll
    for (int i = 1; i < NW; ++i) lt += s_l[i][l32];
    pml[slot * 2] = M;
    pml[slot * 2 + 1] = lt;
  }
}

bool attn_extend_supported(int Q, int H, int G) {
  return Q >= 2 && Q <= EXT_MAX_Q && G > 0 && H > 0 && H % G == 0 && (long)Q * (H / G) <= EXT_NQ;
}
bool attn_extend_grid_ok(int B, int G) { return B <= 65535 && G <= 65535; }
long attn_extend_workspace(int B, int Q, int H, int hd, int Tmax) {
  return attn_decode_split_workspace(B * Q, H, hd, Tmax);
}

template <typename T, int HD>
static void ext_launch(const T* qkv, T* kc, T* vc, float* ws, const int* pos, int B, int Q, int H, int G, int Tmax,
                       hipStream_t s) {
  const int NCH = (int)(((long)Tmax + SPL_CHUNK - 1) / SPL_CHUNK);   // the workspace's chunks per (row, head)
  float* po = ws;
  float* pml = ws + (long)B * Q * H * NCH * HD;
  const float c = kLog2e / sqrtf((float)HD);
  hipLaunchKernelGGL((attn_extend_partial_k<T, HD>), dim3(NCH, G, B), dim3(SPL_THREADS), 0, s, qkv, kc, vc, po, pml,
                     pos, Q, H, G, Tmax, NCH, c);
}

void attn_extend_rows(DType dt, const void* qkv, void* kc, void* vc, void* out, float* ws, const int* pos,
                      const int* pos_rows, int B, int Q, int H, int G, int hd, int Tmax, hipStream_t s) {
#define L_(TT, HDD) ext_launch<TT, HDD>((const TT*)qkv, (TT*)kc, (TT*)vc, ws, pos, B, Q, H, G, Tmax, s)
  if (dt == DType::BF16) {
    if (hd == 128) L_(bf16_t, 128); else L_(bf16_t, 64);
  } else {
    if (hd == 128) L_(f16_t, 128); else L_(f16_t, 64);
  }
#undef L_
  attn_decode_split_combine_rows(dt, ws, out, pos_rows, B * Q, H, hd, Tmax, s);
}

}  // namespace bllm
