// Body of kv_cache_fill_varlen_k / kv_cache_fill_varlen_rows_k (attn_decode.hip), included once per
// kernel with FILL_ROWS 0 / 1.  In scope: qkv, cu, kc, vc, N, B, H, G, Tmax, C, qsc and, with
// FILL_ROWS, rows (int32 [B]: the cache row of each sequence) and CB (rows of the cache).
{
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long per_row = 2L * G * C;
  if (i >= N * per_row) return;
  const long n = i / per_row;
  const int j = (int)((i % per_row) / C), c = (int)(i % C);  // j: k heads 0..G-1, then v heads
  if (n < cu[0] || n >= cu[B]) return;                        // rows outside every sequence
  int lo = 0, hi = B;                                         // cu[lo] <= n < cu[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= n) lo = mid; else hi = mid;
  }
  const int t = (int)(n - cu[lo]);
  BLLM_DASSERT(t < Tmax, DBG_DECODE_POS);
  if (t >= Tmax) return;
#if FILL_ROWS
  lo = rows[lo];                                              // from here on: the cache row
  BLLM_DASSERT(lo >= 0 && lo < CB, DBG_DECODE_POS);
  if (lo < 0 || lo >= CB) return;
#endif
  const int g = j < G ? j : j - G;
  uint4* dst = (j < G ? kc : vc) + (((long)lo * G + g) * Tmax + t) * C + c;
  *dst = qkv[n * qsc + (long)(H + j) * C + c];
}
