// Token sampler: one row of logits -> one token, with temperature, top-k and top-p (nucleus)
// filters and a counter-based random stream per row (common.h sample_uniform).  The contract is
// ops/reference.py:sample_rows; what matters here:
//
//  * one workgroup of 1,024 threads per row, so a row's token depends on nothing but its own
//    logits, stream id and counter;
//  * no sort.  Both filters are VALUE thresholds, found by radix select over order-preserving
//    integer keys of the logits, 8 bits per pass from the top (two passes for bf16 / fp16, four
//    for fp32): a 256-bin LDS histogram of counts (top-k: the k-th largest value, ties kept) or
//    of softmax masses (top-p: the largest value whose upward mass reaches top_p of the kept
//    mass), then the bin that crosses the target is refined.  A row of 128,256 bf16 logits is
//    256 KB and stays in L2 between the passes;
//  * masses are 2^-40 fixed point in 64-bit integers (weights are <= 1 and a row has < 2^17 of
//    them, so the sums fit and lose < 2^-23 of the total): integer LDS atomics give the same
//    histogram in any order, so the result is deterministic.  There is no floating-point atomic;
//  * the draw is Gumbel-max over the kept set, argmax of l / T - log(-log u), with libm's logf
//    (1 ulp; the fast __logf loses relative accuracy for u near 1, where the winners are) and an
//    IEEE division; the lowest index wins an exact tie (64-bit (key, ~index) max reduction);
//  * rows start at b * V elements, so only element alignment is assumed: 16-byte loads over the
//    aligned middle of a row, element loads for its head and tail;
//  * NaN logits count as -inf and +inf as the largest finite value; the token is clamped into
//    [0, V) whatever the values are (it feeds the embedding kernel);
//  * the step's state lives on the device so that it replays from a graph: the token goes to
//    next_idx[b], out[b, ctr[b]] and (== eos_id) finished[b], then ctr[b] advances.  Only row
//    b's workgroup touches ctr[b]; the column written is clamped into out.
#include "api.h"

#include <float.h>
#include <math.h>

namespace bllm {

BLLM_DEBUG_WORD(sample)

namespace {

constexpr int NT = 1024;
constexpr int BINS = 256;
// copies of every bin, picked by lane: the logits of a row share a few exponents, so a wave's
// 64 atomics would otherwise pile onto a handful of addresses.  Bin-major layout: the copies
// of one bin lie in different banks.
constexpr int COPIES = 8;

typedef unsigned long long u64;

struct Smem {
  u64 hist[BINS * COPIES];
  u64 binsum[BINS];
  u64 red[NT / 64];
  u64 sel[2];   // the bin that crosses the target, and the target inside it
};

template <typename T> struct KeyBits {
  static constexpr int KB = 8 * sizeof(T);
  static constexpr uint32_t SIGN = 1u << (KB - 1);
  static constexpr uint32_t MASK = KB == 32 ? 0xFFFFFFFFu : 0xFFFFu;
};
template <typename T> __device__ __forceinline__ uint32_t raw_bits(T v) {
  if constexpr (sizeof(T) == 2) return __builtin_bit_cast(uint16_t, v);
  else return __builtin_bit_cast(uint32_t, v);
}
template <typename T> __device__ __forceinline__ T from_bits(uint32_t b) {
  if constexpr (sizeof(T) == 2) return __builtin_bit_cast(T, (uint16_t)b);
  else return __builtin_bit_cast(T, b);
}
// integer key of a logit, ascending with its value: equal values (-0 and +0 too) get equal keys,
// NaN the key of -inf
template <typename T> __device__ __forceinline__ uint32_t logit_key(T v, float x) {
  typedef KeyBits<T> K;
  uint32_t b = raw_bits(v);
  if (x != x) b = raw_bits(from_f<T>(-INFINITY));
  if (x == 0.f) b = 0;
  return (b & K::SIGN) ? (~b & K::MASK) : (b | K::SIGN);
}
template <typename T> __device__ __forceinline__ float key_value(uint32_t k) {
  typedef KeyBits<T> K;
  const uint32_t b = (k & K::SIGN) ? (k & ~K::SIGN) : (~k & K::MASK);
  return to_f(from_bits<T>(b));
}
__device__ __forceinline__ float sanitize(float x) { return x != x ? -INFINITY : fminf(x, FLT_MAX); }

// fp32 -> uint32 ascending with the value (no NaN reaches it), paired with the index so that one
// 64-bit max picks the largest key and, among equal keys, the lowest index
__device__ __forceinline__ u64 pack_key(float key, int i) {
  const uint32_t b = __float_as_uint(key + 0.0f);   // -0 -> +0
  const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((u64)o << 32) | (0xFFFFFFFFu - (uint32_t)i);
}
__device__ __forceinline__ float packed_value(u64 p) {
  const uint32_t o = (uint32_t)(p >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ u64 umax(u64 a, u64 b) { return a > b ? a : b; }

__device__ __forceinline__ u64 block_max(u64 v, u64* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = umax(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  u64 t = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) t = umax(t, red[i]);
  return t;
}

// f(i, row[i]) for every i in [0, V), the workgroup's threads sharing the row
template <typename T, typename F>
__device__ __forceinline__ void for_row(const T* row, int V, F f) {
  constexpr int N = 16 / sizeof(T);
  const int tid = threadIdx.x;
  int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) / sizeof(T));   // elements before the first 16-B boundary
  if (head > V) head = V;
  if (tid < head) f(tid, row[tid]);
  const int nvec = (V - head) / N;
  const T* body = row + head;
  for (int v = tid; v < nvec; v += NT) {
    const Vec16<T> x = ld16(body + (long)v * N);
#pragma unroll
    for (int j = 0; j < N; ++j) f(head + v * N + j, x.v[j]);
  }
  const int t0 = head + nvec * N;   // fewer than N <= 8 elements are left
  if (t0 + tid < V) f(t0 + tid, row[t0 + tid]);
}

// Radix select from the top over the keys >= floor_key.  MASS false: the key of the target-th
// largest element (1 <= target <= their number).  MASS true: the largest key whose upward mass
// sum{w : key' >= key} reaches top_p of the whole mass, w = exp((l - mx) / temp) in 2^-40 fixed
// point (mx is the row maximum and belongs to the set, so the mass is at least 2^40).
template <typename T, bool MASS>
__device__ uint32_t radix_select(const T* row, int V, u64 target, uint32_t floor_key, float mx, float temp,
                                 double top_p, Smem& sm) {
  constexpr int KB = KeyBits<T>::KB;
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  for (int shift = KB - 8; shift >= 0; shift -= 8) {
    const bool first = shift == KB - 8;
    __syncthreads();   // the previous pass has read sel and binsum
    for (int j = tid; j < BINS * COPIES; j += NT) sm.hist[j] = 0;
    if (tid == 0) {
      sm.sel[0] = 0;
      sm.sel[1] = 1;
    }
    __syncthreads();
    const uint32_t hi = first ? 0u : prefix >> ((shift + 8) & 31);
    for_row(row, V, [&](int, T v) {
      const float x = to_f(v);
      const uint32_t k = logit_key<T>(v, x);
      bool in = first || (k >> ((shift + 8) & 31)) == hi;
      if (MASS) in = in && k >= floor_key;
      if (in) {
        u64 add = 1;
        if (MASS) add = (u64)(expf((sanitize(x) - mx) / temp) * 1099511627776.f);
        if (add) atomicAdd(&sm.hist[((k >> shift) & 255u) * COPIES + (tid & (COPIES - 1))], add);
      }
    });
    __syncthreads();
    if (tid < BINS) {
      u64 s = 0;
#pragma unroll
      for (int c = 0; c < COPIES; ++c) s += sm.hist[tid * COPIES + c];
      sm.binsum[tid] = s;
    }
    __syncthreads();
    if (tid < BINS) {
      u64 above = 0, total = 0;
      for (int j = 0; j < BINS; ++j) {
        const u64 v = sm.binsum[j];
        total += v;
        if (j > tid) above += v;
      }
      u64 t = target;
      if (MASS && first) {
        t = (u64)ceil(top_p * (double)total);
        t = t < 1 ? 1 : (t > total ? total : t);
      }
      if (above < t && t <= above + sm.binsum[tid]) {   // true for exactly one bin
        sm.sel[0] = (u64)tid;
        sm.sel[1] = t - above;
      }
    }
    __syncthreads();
    prefix |= (uint32_t)sm.sel[0] << shift;
    target = sm.sel[1];
  }
  return prefix;
}

template <typename T>
__global__ __launch_bounds__(NT) void sample_rows_kernel(const T* __restrict__ logits, const int64_t* __restrict__ stream,
                                                         int* ctr, uint64_t seed, float temp, int top_k, double top_p,
                                                         long eos_id, int64_t* next_idx, int64_t* out, long out_ld,
                                                         int out_cols, unsigned char* finished, float* thr,
                                                         int64_t* tokens, int V) {
  __shared__ Smem sm;
  const int b = blockIdx.x;
  const T* row = logits + (long)b * V;
  const int c = ctr[b];

  // the row maximum and its lowest index: the greedy token, and the softmax shift
  u64 best = 0;
  for_row(row, V, [&](int i, T v) { best = umax(best, pack_key(sanitize(to_f(v)), i)); });
  best = block_max(best, sm.red);
  const float mx = packed_value(best);

  float kept_min = -INFINITY;
  if (temp > 0.f) {
    uint32_t tkey = 0;
    const bool use_k = top_k > 0 && top_k < V, use_p = top_p < 1.0;
    if (mx > -INFINITY) {   // a row of -inf / NaN only has nothing to filter
      if (use_k) tkey = radix_select<T, false>(row, V, (u64)top_k, 0u, mx, temp, top_p, sm);
      if (use_p) tkey = radix_select<T, true>(row, V, 0, tkey, mx, temp, top_p, sm);
      if (use_k || use_p) kept_min = key_value<T>(tkey);
    }
    const SampleKeys rk = sample_row_keys(seed, (uint64_t)stream[b], (uint32_t)c);
    best = 0;
    for_row(row, V, [&](int i, T v) {
      const float x = to_f(v);
      if (logit_key<T>(v, x) >= tkey) {
        const float key = sanitize(x) / temp - logf(-logf(sample_uniform(rk, (uint32_t)i)));
        if (key == key) best = umax(best, pack_key(key, i));
      }
    });
    best = block_max(best, sm.red);
  }
  if (threadIdx.x == 0) {
    uint32_t tok = 0xFFFFFFFFu - (uint32_t)best;
    if (tok > (uint32_t)(V - 1)) tok = (uint32_t)(V - 1);   // nothing comparable in the row
    tokens[b] = (int64_t)tok;
    if (next_idx) next_idx[b] = (int64_t)tok;
    if (out) {
      BLLM_DASSERT(c >= 0 && c < out_cols, DBG_SAMPLE_CTR);
      const int col = c < 0 ? 0 : (c >= out_cols ? out_cols - 1 : c);
      out[(long)b * out_ld + col] = (int64_t)tok;
    }
    if (finished && eos_id >= 0 && (long)tok == eos_id) finished[b] = 1;
    if (thr && temp > 0.f) thr[b] = kept_min;
    ctr[b] = c + 1;   // every thread read ctr[b] before the barriers above
  }
}

}  // namespace

void sample_rows(DType dt, const void* logits, const int64_t* stream, int* ctr, uint64_t seed, float temperature,
                 int top_k, double top_p, long eos_id, int64_t* next_idx, int64_t* out, long out_ld, int out_cols,
                 unsigned char* finished, float* thr, int64_t* tokens, int B, int V, hipStream_t s) {
  BLLM_DISPATCH(dt, T,
                hipLaunchKernelGGL(sample_rows_kernel<T>, dim3(B), dim3(NT), 0, s, (const T*)logits, stream, ctr, seed,
                                   temperature, top_k, top_p, eos_id, next_idx, out, out_ld, out_cols, finished, thr,
                                   tokens, V));
}

}  // namespace bllm
