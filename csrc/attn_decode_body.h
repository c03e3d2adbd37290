// Body of the decode kernels of attn_decode.hip, included once per kernel definition (no include
// guard on purpose).  The including kernel provides: template parameters T, HD and a constant
// APPEND; parameters q, kc, vc, out, H, G, Tmax, L (written here when APPEND), scale, pos, qs;
// and DEC_POS(b), the cache position of batch row b (read only when APPEND).  The text is shared,
// not a device function: with the body in a force-inlined function the compiler scheduled the
// existing attn_decode_k instantiations differently (tools/isa_diff.py), and a further template
// parameter would rename them; included like this their gfx950 code is what it was.
  constexpr int VEC = 8;               // elements per 16-B load
  constexpr int NC = HD / VEC;         // 16-B chunks per row
  constexpr int KPH = DEC_THREADS / NC;  // key phases in the output pass
  __shared__ float sc[DEC_MAXL];
  __shared__ float red[DEC_THREADS / 64];
  __shared__ float part[KPH][HD];
  const int bh = blockIdx.x, h = bh % H, b = bh / H;
  const int g = h / (H / G);
  const int tid = threadIdx.x;
  const T* qr = APPEND ? q + (long)b * qs + (long)h * HD : q + ((long)b * H + h) * HD;
  T* kb = kc + ((long)b * G + g) * (long)Tmax * HD;
  T* vb = vc + ((long)b * G + g) * (long)Tmax * HD;
  const T* knew = nullptr;
  const T* vnew = nullptr;
  if constexpr (APPEND) {
    int p = DEC_POS(b);
    BLLM_DASSERT(p >= 0 && p < Tmax && p < DEC_MAXL, DBG_DECODE_POS);
#ifdef BLLM_KERNEL_DEBUG
    p = p < 0 ? 0 : (p >= Tmax ? Tmax - 1 : p);
    p = p >= DEC_MAXL ? DEC_MAXL - 1 : p;
#endif
    L = p + 1;
    knew = q + (long)b * qs + (long)(H + g) * HD;
    vnew = q + (long)b * qs + (long)(H + G + g) * HD;
    if (h % (H / G) == 0 && tid < 2 * (HD / 8)) {  // one block per kv group appends k and v
      const int c = tid % (HD / 8);
      if (tid < HD / 8) st16(kb + (long)p * HD + c * 8, ld16(knew + c * 8));
      else st16(vb + (long)p * HD + c * 8, ld16(vnew + c * 8));
    }
  }
  const float c = scale * kLog2e;

  float qf[HD];
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const Vec16<T> v = ld16(qr + i * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j) qf[i * VEC + j] = to_f(v.v[j]);
  }
  // 1. scores (log2 domain)
  float mx = -INFINITY;
  for (int k = tid; k < L; k += DEC_THREADS) {
    const T* kr = (APPEND && k == L - 1) ? knew : kb + (long)k * HD;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const Vec16<T> v = ld16(kr + i * VEC);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s += qf[i * VEC + j] * to_f(v.v[j]);
    }
    s *= c;
    sc[k] = s;
    mx = fmaxf(mx, s);
  }
  // 2. softmax statistics
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int i = 1; i < DEC_THREADS / 64; ++i) mx = fmaxf(mx, red[i]);
  __syncthreads();
  float sum = 0.f;
  for (int k = tid; k < L; k += DEC_THREADS) {
    const float p = exp2f(sc[k] - mx);
    sc[k] = p;
    sum += p;
  }
  sum = wave_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  sum = 0.f;
#pragma unroll
  for (int i = 0; i < DEC_THREADS / 64; ++i) sum += red[i];
  const float inv = 1.f / sum;
  // 3. weighted V sum: thread = (chunk ci, key phase kp)
  const int ci = tid % NC, kp = tid / NC;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  for (int k = kp; k < L; k += KPH) {
    const Vec16<T> v = ld16(((APPEND && k == L - 1) ? vnew : vb + (long)k * HD) + ci * VEC);
    const float p = sc[k];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] += p * to_f(v.v[j]);
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) part[kp][ci * VEC + j] = acc[j];
  __syncthreads();
  for (int d = tid; d < HD; d += DEC_THREADS) {
    float o = 0.f;
#pragma unroll
    for (int p2 = 0; p2 < KPH; ++p2) o += part[p2][d];
    out[((long)b * H + h) * HD + d] = from_f<T>(o * inv);
  }
