// Single-query attention against a KV cache (autoregressive decode), gfx950.
//
// Replaces the reference's generation path (generate.py:37-42), which re-runs the full model
// over the whole context for every new token (no KV cache; Llama3.py:131-155 materialises the
// [B,H,T,T] scores each time).  Here K/V of past positions live in a cache laid out
// [B, G, Tmax, hd] (one contiguous 2*hd-byte row per key, GQA-native: the H/G query heads of a
// kv group read the same rows), and each new token costs one pass over the cache.
//
// One workgroup per (batch, query head), 256 threads:
//   1. scores: every thread owns keys k = tid, tid+256, ...; it streams its key's row (16-B
//      loads) and dots it with q held in registers (fp32);  scores -> LDS;
//   2. softmax: block max / sum over the scores (exp2 with folded log2e);
//   3. out[d] = sum_k p_k V[k][d]: thread = (d-chunk of 8, key phase), rows read coalesced,
//      partial sums combined through LDS in a fixed order.
// Memory-bound (reads each cached row once per query head); fp32 accumulation throughout.
#include "api.h"

namespace bllm {

BLLM_DEBUG_WORD(attn_decode)

constexpr int DEC_THREADS = 256;
constexpr int DEC_MAXL = 8192;  // LDS score buffer (32 KiB)

// Three forms share one body (attn_decode_body.h):
// plain: q [B, H, hd] against the first L cached positions.
// APPEND (graph-replayed decode, the position known only on the device): q, the new key and
// the new value come from the packed qkv row of the token (row stride qs); L = *pos + 1 and key
// L - 1 is read from that row, while the first query head of each kv group also writes it into
// the caches at row *pos (no block of this launch reads cache row *pos, so no ordering needed).
// rows (attn_decode_rows_k, decode of a ragged batch): APPEND with one position per batch row;
// row b appends at cache row pos[b] and attends over its own pos[b] + 1 keys.
template <typename T, int HD, bool APPEND>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_k(const T* __restrict__ q, T* __restrict__ kc,
                                                             T* __restrict__ vc, T* __restrict__ out,
                                                             int H, int G, int Tmax, int L, float scale,
                                                             const int* __restrict__ pos, long qs) {
#define DEC_POS(b) (*pos)
#include "attn_decode_body.h"
#undef DEC_POS
}

template <typename T, int HD>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_rows_k(const T* __restrict__ q, T* __restrict__ kc,
                                                                  T* __restrict__ vc, T* __restrict__ out,
                                                                  int H, int G, int Tmax, float scale,
                                                                  const int* __restrict__ pos, long qs) {
  constexpr bool APPEND = true;
  int L = 0;
#define DEC_POS(b) (pos[b])
#include "attn_decode_body.h"
#undef DEC_POS
}

// Prefill of the caches from a packed variable-length batch: cache row (b, g, t) <- the k and v
// of packed row cu[b] + t.  One thread per 16-B chunk of one (row, k-or-v head); the row's
// sequence is found by bisection of cu (B + 1 entries, read through the scalar cache).  C =
// chunks per head row, qsc = chunks per qkv row.  Any element type: the copy is bitwise.
// Two forms share one body (kv_fill_body.h), as the decode kernels above do.  FILL_ROWS (slot-mapped
// fill, admission into a live cache): the batch has B sequences and sequence b goes to cache row
// rows[b] of a cache with CB rows, B <= CB; the host wrapper has checked the rows distinct and in
// range, so no two threads store to one address.  Without it: row b, the kernel as it always was.
__global__ __launch_bounds__(256) void kv_cache_fill_varlen_k(const uint4* __restrict__ qkv,
                                                              const int* __restrict__ cu, uint4* __restrict__ kc,
                                                              uint4* __restrict__ vc, long N, int B, int H, int G,
                                                              int Tmax, int C, long qsc) {
#define FILL_ROWS 0
#include "kv_fill_body.h"
#undef FILL_ROWS
}

__global__ __launch_bounds__(256) void kv_cache_fill_varlen_rows_k(const uint4* __restrict__ qkv,
                                                                   const int* __restrict__ cu, uint4* __restrict__ kc,
                                                                   uint4* __restrict__ vc, long N, int B, int H, int G,
                                                                   int Tmax, int C, long qsc,
                                                                   const int* __restrict__ rows, int CB) {
#define FILL_ROWS 1
#include "kv_fill_body.h"
#undef FILL_ROWS
}

int attn_decode_max_len() { return DEC_MAXL; }

void attn_decode(DType dt, const void* q, const void* kc, const void* vc, void* out, int B, int H, int G, int hd,
                 int Tmax, int L, hipStream_t s) {
  const float scale = 1.f / sqrtf((float)hd);
  dim3 grid(B * H), block(DEC_THREADS);
#define L_(TT, HDD) hipLaunchKernelGGL((attn_decode_k<TT, HDD, false>), grid, block, 0, s, (const TT*)q, (TT*)kc, \
                                       (TT*)vc, (TT*)out, H, G, Tmax, L, scale, nullptr, 0L)
  if (dt == DType::BF16) {
    if (hd == 128) L_(bf16_t, 128); else L_(bf16_t, 64);
  } else {
    if (hd == 128) L_(f16_t, 128); else L_(f16_t, 64);
  }
#undef L_
}

void attn_decode_append(DType dt, const void* qkv, void* kc, void* vc, void* out, const int* pos, int B, int H,
                        int G, int hd, int Tmax, hipStream_t s) {
  const float scale = 1.f / sqrtf((float)hd);
  const long qs = (long)(H + 2 * G) * hd;
  dim3 grid(B * H), block(DEC_THREADS);
#define L_(TT, HDD) hipLaunchKernelGGL((attn_decode_k<TT, HDD, true>), grid, block, 0, s, (const TT*)qkv, (TT*)kc, \
                                       (TT*)vc, (TT*)out, H, G, Tmax, 0, scale, pos, qs)
  if (dt == DType::BF16) {
    if (hd == 128) L_(bf16_t, 128); else L_(bf16_t, 64);
  } else {
    if (hd == 128) L_(f16_t, 128); else L_(f16_t, 64);
  }
#undef L_
}

void attn_decode_append_rows(DType dt, const void* qkv, void* kc, void* vc, void* out, const int* pos, int B, int H,
                             int G, int hd, int Tmax, hipStream_t s) {
  const float scale = 1.f / sqrtf((float)hd);
  const long qs = (long)(H + 2 * G) * hd;
  dim3 grid(B * H), block(DEC_THREADS);
#define L_(TT, HDD) hipLaunchKernelGGL((attn_decode_rows_k<TT, HDD>), grid, block, 0, s, (const TT*)qkv, (TT*)kc, \
                                       (TT*)vc, (TT*)out, H, G, Tmax, scale, pos, qs)
  if (dt == DType::BF16) {
    if (hd == 128) L_(bf16_t, 128); else L_(bf16_t, 64);
  } else {
    if (hd == 128) L_(f16_t, 128); else L_(f16_t, 64);
  }
#undef L_
}

void kv_cache_fill_varlen(const void* qkv, const int* cu, void* kc, void* vc, long N, int B, int H, int G, int Tmax,
                          int row_bytes, hipStream_t s, const int* rows, int CB) {
  const int C = row_bytes / 16;
  const long total = N * 2L * G * C;
  if (total == 0) return;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (rows)
    hipLaunchKernelGGL(kv_cache_fill_varlen_rows_k, grid, dim3(256), 0, s, (const uint4*)qkv, cu, (uint4*)kc,
                       (uint4*)vc, N, B, H, G, Tmax, C, (long)(H + 2 * G) * C, rows, CB);
  else
    hipLaunchKernelGGL(kv_cache_fill_varlen_k, grid, dim3(256), 0, s, (const uint4*)qkv, cu, (uint4*)kc, (uint4*)vc,
                       N, B, H, G, Tmax, C, (long)(H + 2 * G) * C);
}

}  // namespace bllm
