// Body of kv_cache_fill_varlen_fp8_k / kv_cache_fill_varlen_fp8_rows_k (attn_decode_fp8.hip),
// included once per kernel with FILL_ROWS 0 / 1.  In scope: T, HD, qkv, cu, k8, ks, v8, vs, N, B, H,
// G, Tmax and, with FILL_ROWS, rows (int32 [B]) and CB (rows of the cache).  An out-of-range row
// leaves ahead of the shuffles like t >= Tmax does: the C lanes of a head row share lo, so they
// leave together.
{
  constexpr int C = HD / 8;
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
  const Vec16<T> x = ld16(qkv + n * (long)(H + 2 * G) * HD + (long)(H + j) * HD + c * 8);
  float f[8], a = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f[e] = to_f(x.v[e]);
    a = fmaxf(a, fabsf(f[e]));
  }
#pragma unroll
  for (int o = C / 2; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
  const float s = f8_scale(a);
  uint2 w;
  w.x = f8_pack2(f[0], f[1], s) | (f8_pack2(f[2], f[3], s) << 16);
  w.y = f8_pack2(f[4], f[5], s) | (f8_pack2(f[6], f[7], s) << 16);
  const int g = j < G ? j : j - G;
  const long row = ((long)lo * G + g) * Tmax + t;
  *reinterpret_cast<uint2*>((j < G ? k8 : v8) + row * HD + c * 8) = w;
  if (c == 0) (j < G ? ks : vs)[row] = s;
}
