// Speculative decoding bookkeeping on the device (prompt lookup): accept the drafts that the
// verify step confirmed, then draft the next step's tokens.  The contract, in plain Python, is
// ops/reference.py:spec_advance; integers only, so kernel and oracle agree exactly.
//
// One workgroup per row, one launch.  Thread 0 does the accept part (at most 8 tokens): how many
// leading drafts equal what the sampler chose, the tokens that are emitted (cut at the answer's
// length and at the first eos), their copy into the answer and into the row's corpus, and the
// row's position, counter, step count and finished flag.  After a barrier all threads scan the
// corpus for the latest earlier occurrence of its trailing n-gram (each thread keeps the largest
// start it matched, then a max over the workgroup) and the first Q threads write the next input
// tokens: the last emitted token, then the continuation of the match, repeated with its period.
// Only row b's workgroup touches row b's state.
#include "api.h"

namespace bllm {

BLLM_DEBUG_WORD(spec)

namespace {

constexpr int SPEC_NT = 256;
constexpr int SPEC_MAX_Q = 8;
constexpr int SPEC_MAX_NGRAM = 4;

__global__ __launch_bounds__(SPEC_NT) void spec_advance_k(
    int64_t* __restrict__ idx, const int64_t* __restrict__ samp, int* __restrict__ hist, const int* __restrict__ h0,
    int* __restrict__ pos, int* __restrict__ ctr, int* __restrict__ nsteps, unsigned char* __restrict__ finished,
    int64_t* __restrict__ out, long out_stride, int Q, int Lh, int newn, long eos_id, int ngram, int accept) {
  __shared__ int s_pos;
  __shared__ int s_best[SPEC_NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x, K = Q - 1;
  int* hrow = hist + (long)b * Lh;
  int64_t* irow = idx + (long)b * Q;
  const int hb = h0[b];

  if (tid == 0) {
    int p = pos[b];
    if (accept && !finished[b]) {
      const int64_t* srow = samp + (long)b * Q;
      int c = ctr[b];
      BLLM_DASSERT(c >= 0 && c < newn && hb >= 0 && p >= 0 && hb + p + 1 + Q <= Lh, DBG_SPEC_STATE);
      c = c < 0 ? 0 : c;
      int a = 0;
      while (a < K && irow[a + 1] == srow[a]) ++a;
      int e = a + 1 < newn - c ? a + 1 : newn - c;
      bool fin = false;
      if (eos_id >= 0) {
        for (int j = 0; j < e; ++j)
          if (srow[j] == (int64_t)eos_id) {
            e = j + 1;
            fin = true;
            break;
          }
      }
      for (int j = 0; j < e; ++j) {
        out[(long)b * out_stride + c + j] = srow[j];
        const int hp = hb + p + 1 + j;
        if (hp >= 0 && hp < Lh) hrow[hp] = (int)srow[j];
      }
      if (e > 0) {
        p += e;
        c += e;
        pos[b] = p;
        ctr[b] = c;
      }
      nsteps[b] += 1;
      if (fin || c >= newn) finished[b] = 1;
    }
    s_pos = p;
  }
  __syncthreads();   // the corpus row as thread 0 left it

  // ---- draft: the latest i in [0, n - ngram - 1] with c[i : i + ngram] == c[n - ngram : n]
  int n = hb + s_pos + 1;
  BLLM_DASSERT(n >= 1 && n <= Lh, DBG_SPEC_STATE);
  n = n < 1 ? 1 : (n > Lh ? Lh : n);
  int best = -1;
  if (n > ngram) {
    int tail[SPEC_MAX_NGRAM];
#pragma unroll
    for (int t = 0; t < SPEC_MAX_NGRAM; ++t) tail[t] = t < ngram ? hrow[n - ngram + t] : 0;
    for (int i = tid; i <= n - ngram - 1; i += SPEC_NT) {
      bool m = true;
#pragma unroll
      for (int t = 0; t < SPEC_MAX_NGRAM; ++t)
        if (t < ngram) m = m && hrow[i + t] == tail[t];
      if (m) best = i;   // ascending i per thread: the last match is the largest
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int x = __shfl_xor(best, o, 64);
    best = x > best ? x : best;
  }
  if ((tid & 63) == 0) s_best[tid >> 6] = best;
  __syncthreads();
  best = s_best[0];
#pragma unroll
  for (int i = 1; i < SPEC_NT / 64; ++i) best = s_best[i] > best ? s_best[i] : best;

  if (tid < Q) {
    int tok = hrow[n - 1];
    if (tid > 0 && best >= 0) {
      const int per = n - best - ngram;   // >= 1
      tok = hrow[best + ngram + (tid - 1) % per];
    }
    irow[tid] = tok;
  }
}

}  // namespace

bool spec_advance_supported(int Q, int ngram) {
  return Q >= 1 && Q <= SPEC_MAX_Q && ngram >= 1 && ngram <= SPEC_MAX_NGRAM;
}

void spec_advance(int64_t* idx, const int64_t* samp, int* hist, const int* h0, int* pos, int* ctr, int* nsteps,
                  unsigned char* finished, int64_t* out, long out_stride, int B, int Q, int Lh, int newn,
                  long eos_id, int ngram, bool accept, hipStream_t s) {
  hipLaunchKernelGGL(spec_advance_k, dim3(B), dim3(SPEC_NT), 0, s, idx, samp, hist, h0, pos, ctr, nsteps, finished,
                     out, out_stride, Q, Lh, newn, eos_id, ngram, accept ? 1 : 0);
}

}  // namespace bllm
