// The flash-attention forward kernel, written once and compiled twice by
// attn_mfma.hip: BLLM_ATTN_VARLEN 0 gives the
// uniform kernel (B sequences of T_ rows each, sequence b at row b T_), BLLM_ATTN_VARLEN 1 the
// *_varlen_k sibling: sequence b is rows [cu[b], cu[b+1]) of the packed tensors (cu int32
// [B + 1], cu[B] = N rows in all) and has T_ = cu[b+1] - cu[b] rows, read once per workgroup
// and wave-uniform; Tmax only sizes the grid, and a workgroup whose first query (key, in dK/dV)
// lies beyond its sequence leaves before its first barrier, DMA or store (T_ = 0 is legal).
// lse / delta are then [H * N] floats at H cu[b] + h T_ + q -- the uniform formula when all
// lengths are equal.  Every other line is shared, so the sequence-tail clamps keep each address
// inside rows [cu[b], cu[b+1]).  The macros below are the only difference; the uniform
// expansion is token for token the kernel as it was before the variable-length form existed.
// No include guard: included once per form.
#if BLLM_ATTN_VARLEN
#define BLLM_SEQ_KERNEL(name) name##_varlen_k
#define BLLM_SEQ_T Tmax
#define BLLM_SEQ_CU , const int* __restrict__ cu
#define BLLM_SEQ_ROW0 row0
#define BLLM_SEQ_STAT0(hq) ((long)H * row0 + (long)(hq) * T_)
#define BLLM_SEQ_NROWS ((long)cu[B_])
// blk0 = the workgroup's first query / key inside its sequence
#define BLLM_SEQ_ENTER(blk0)                                                                    \
  const int row0_ = __builtin_amdgcn_readfirstlane(cu[b]);                                      \
  const int T_ = __builtin_amdgcn_readfirstlane(cu[b + 1]) - row0_;                             \
  const long row0 = row0_;                                                                      \
  if ((blk0) >= T_) return; /* workgroup-uniform; nothing issued, waited on or stored yet */
#else
#define BLLM_SEQ_KERNEL(name) name##_k
#define BLLM_SEQ_T T_
#define BLLM_SEQ_CU
#define BLLM_SEQ_ROW0 ((long)b * T_)
#define BLLM_SEQ_STAT0(hq) (((long)b * H + (hq)) * T_)
#define BLLM_SEQ_NROWS ((long)B_ * T_)
#define BLLM_SEQ_ENTER(blk0)
#endif

// Per 64-key tile and wave: 32 MFMAs, 16 b128 + 32 tr_b64 LDS reads at loop-invariant
// per-lane offsets, 2x(LD) saddr DMA issues with precomputed per-lane source offsets, and
// ~130 VALU of online softmax (scale folded into the exp2 FMA; the O rescale is skipped when
// no lane's running max moved, which is the common case after the first tiles).  The LDS
// fragment reads run one MFMA step ahead (QK^T: both 32-key sub-tiles' next K fragments before
// this step's pair of MFMAs, pinned by sched_barrier; PV: the next V^T fragment before each
// MFMA): hipcc's own schedule waited on every read right before its MFMA (round 6, headline
// forward +1.5 % same process, profiles/r6/attn/).
template <typename T, int HD, bool DROP, int FWD_BK, int OCC>
__global__ __launch_bounds__(256, OCC) void BLLM_SEQ_KERNEL(attn_fwd_mfma)(const T* __restrict__ qkv, T* __restrict__ out,
                                                          float* __restrict__ lse, int BLLM_SEQ_T, int H, int G, int B_,
                                                          bool causal, uint32_t thr, float inv_keep, uint64_t seed,
                                                          uint64_t doff, uint32_t* __restrict__ kmask, int xmap BLLM_SEQ_CU) {
  typedef typename Mma<T>::v8 v8;
  constexpr int KK = HD / 16;               // k-steps of the QK^T product
  constexpr int DT = HD / 32;               // 32-row tiles of O^T
  constexpr int CH = HD / 8;                // 16-B chunks per K/V row
  constexpr int ROWB = HD * 2;
  constexpr int TILE_B = FWD_BK * ROWB;     // bytes per K (or V) tile
  constexpr int LD = FWD_BK * CH / 256;     // 1-KiB pieces per wave per tile (K and V each)
  constexpr int NKT = FWD_BK / 32;          // 32-key MFMA tiles per step
  // 32-query blocks per wave.  A constant 1 (file header), yet the block index and its one-trip
  // loops stay: hipcc's code for this kernel depends on them (without the loops of the Q / O
  // set-up and of the epilogue it allocates registers and orders blocks differently), and so
  // does the one-trip loop of the ring prologue below
  constexpr int QB = 1;
  constexpr int WQ = 32 * QB;               // queries per wave
  constexpr int BQ = FWD_BQ * QB;           // queries per workgroup
  constexpr int NBUF = FWD_NBUF;

  extern __shared__ __attribute__((aligned(16))) char smem[];

  // heaviest (latest, for causal) q-blocks first over the whole grid; the q-blocks of one
  // (b, h) and (xmap 1) the query heads of one kv head run on one XCD / L2 (common.h)
  const int nqb = (BLLM_SEQ_T + BQ - 1) / BQ;
  const int lin = blockIdx.x, nbh = H * B_;
  int qbi, bh;
  attn_wg_order(lin, nbh, H / G, xmap, qbi, bh);
  const int h = bh % H, b = bh / H;
  const int qb = causal ? nqb - 1 - qbi : qbi;
  BLLM_SEQ_ENTER(qb * BQ)
  const int g = h / (H / G);
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l32 = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gi = lane & 15, gl = (lane >> 4) & 1, qrow = gi >> 2, pcol = gi & 3;
  const long rs = (long)(H + 2 * G) * HD;
  const T* qbase = qkv + BLLM_SEQ_ROW0 * rs + (long)h * HD;
  const T* kbase = qkv + BLLM_SEQ_ROW0 * rs + (long)(H + g) * HD;
  const T* vbase = qkv + BLLM_SEQ_ROW0 * rs + (long)(H + G + g) * HD;
  const int q0 = qb * BQ;
  const int wq_lo = q0 + w * WQ, wq_hi = wq_lo + WQ - 1;  // this wave's query range
  int qi[QB];                                             // this lane's query in each q-block
#pragma unroll
  for (int u = 0; u < QB; ++u) qi[u] = wq_lo + 32 * u + l32;
  const float c = rsqrtf((float)HD) * kLog2e;
  DropSlab ds;
  uint64_t dslab = 0;
  bool dpair = false;
  if constexpr (DROP) {
    dslab = doff + (uint64_t)(b * H + h) * T_ * T_;
    ds.init(seed, dslab);
    dpair = ((doff | (uint64_t)T_) & 1) == 0;
  }

  // ---- Q fragments (B operand): Q[qi][16kk + 8hh + 0..7]
  v8 qf[QB][KK];
#pragma unroll
  for (int u = 0; u < QB; ++u)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      if (qi[u] < T_) qf[u][kk] = *reinterpret_cast<const v8*>(qbase + (long)qi[u] * rs + kk * 16 + hh * 8);
      else qf[u][kk] = v8{};
    }
#pragma unroll
  for (int u = 0; u < QB; ++u)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) asm volatile("" ::"v"(qf[u][kk]));  // retire before the loop

  f32x16 o[QB][DT];
#pragma unroll
  for (int u = 0; u < QB; ++u)
#pragma unroll
    for (int i = 0; i < DT; ++i) o[u][i] = f32x16{};
  float m[QB], l[QB];
#pragma unroll
  for (int u = 0; u < QB; ++u) m[u] = -1e30f, l[u] = 0.f;

  // ---- loop-invariant per-lane offsets
  int koff[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) koff[kk] = row_img_off<HD>(l32, kk * 2 + hh);
  int voff[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) voff[dt] = tr_img_off<HD>(4 * hh + qrow, dt * 32 + gl * 16 + pcol * 4);
  // DMA piece i of this lane: row P / CH, physical 16-B chunk P % CH (P = (w LD + i) 64 + lane);
  // the source chunk carries the image's XOR swizzle.  Recomputed at every issue from an opaque
  // copy of the lane id (kept in VGPRs across the loop they were spilled at hd 128, and each
  // scratch reload's vmcnt(0) serialised the DMA pieces); the full-tile path below splits P into
  // a wave-uniform row (SGPR base) and the lane's row / chunk with unsigned shifts (23 VALU per
  // 8 pieces instead of 61), this general form serves the sequence-tail tile.
  const uint32_t rs2 = (uint32_t)rs * 2u;  // row stride in bytes (< 2^24 for every shape)
  auto piece = [&](int i, int ln, int& r, int& kc16, int& vc16) {
    const int P = (w * LD + i) * 64 + ln;
    r = P / CH;
    const int pc = P % CH;
    kc16 = BLLM_ROW_IMG_SRC16(HD, r, pc);
    vc16 = BLLM_TR_IMG_SRC16(HD, r, pc);
  };
  const uint32_t smem_u = lds_u32(smem);
  // K / V bases in SGPRs once (the per-piece row offsets are then scalar arithmetic)
  const char* ksb = (const char*)sgpr_ptr(kbase);
  const char* vsb = (const char*)sgpr_ptr(vbase);

  const int kend = causal ? min(T_, q0 + BQ) : T_;
  const int ntiles = (kend + FWD_BK - 1) / FWD_BK;
  const int nact = wq_lo >= T_ ? 0 : (causal ? min(ntiles, min(wq_hi, T_ - 1) / FWD_BK + 1) : ntiles);

  // K/V tiles land in LDS by direct DMA (1 KiB per wave instruction, lane-linear destination);
  // the XOR swizzle is applied to the per-lane SOURCE offset, so the linear DMA image IS the
  // swizzled layout.
  auto issue = [&](int t, int buf) {
    const int k0 = t * FWD_BK;
    const uint32_t base = smem_u + buf * 2 * TILE_B;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    if (k0 + FWD_BK <= T_) {
      // piece i of lane ln: row rb_i + lr (rb_i = (w LD + i) 64 / CH, wave-uniform, folded into the
      // SGPR base), chunk pc = ln % CH; unsigned shifts, and the V chunk does not depend on i
      const uint32_t lr = (uint32_t)ln / CH, pc = (uint32_t)ln % CH;
      const uint32_t lro = lr * rs2;
#pragma unroll
      for (int i = 0; i < LD; ++i) {
        const int rb = (w * LD + i) * (64 / CH);
        const uint32_t r = (uint32_t)rb + lr;
        const uint32_t kc16 = BLLM_ROW_IMG_SRC16(HD, r, pc), vc16 = BLLM_TR_IMG_SRC16(HD, r, pc);
        const void* ks = ksb + (long)(k0 + rb) * rs2;
        const void* vs = vsb + (long)(k0 + rb) * rs2;
        const uint32_t pd = (w * LD + i) * 1024;
        glds16s(ks, lro + kc16 * 16u, base + pd);
        glds16s(vs, lro + vc16 * 16u, base + TILE_B + pd);
      }
    } else {  // sequence tail: clamp rows (masked / multiplied by P = 0 later)
      char* kb = smem + buf * 2 * TILE_B;
#pragma unroll
      for (int i = 0; i < LD; ++i) {
        int r, kc16, vc16;
        piece(i, ln, r, kc16, vc16);
        const int pd = (w * LD + i) * 1024;
        const int key = min(k0 + r, T_ - 1);
        glds16(kbase + (long)key * rs + kc16 * 8, kb + pd);
        glds16(vbase + (long)key * rs + vc16 * 8, kb + TILE_B + pd);
      }
    }
  };
  // the whole ring is drained at every step: with two slots nothing else is in flight
  auto ring_wait = [&]() {
    wait_vm0();
    __builtin_amdgcn_s_barrier();
  };
#pragma unroll
  for (int j = 0; j < NBUF - 1; ++j)
    if (j < ntiles) issue(j, j);
  wait_vm0();
  __builtin_amdgcn_s_barrier();
  int t = 0, buf = 0;
  // dropout keep-mask words of the last computed tile (kmask != nullptr): stored at the top of
  // the next iteration, BEFORE that iteration's DMA issue -- vector memory completes in order,
  // so the ring's counted waits are not lengthened by the stores
  uint32_t kw_pend[QB][NKT];
  int kw_n = 0, kw_t = 0;
  const long kw_row = (long)((T_ + 31) / 32) * T_;  // words per (b, h)
  auto flush_mask = [&]() {
    if constexpr (DROP) {
      if (kmask != nullptr && hh == 0) {
#pragma unroll
        for (int u = 0; u < QB; ++u) {
          if (qi[u] >= T_) continue;
          uint32_t* mrow = kmask + (long)(b * H + h) * kw_row + qi[u];
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt)
            if (kt < kw_n) mrow[(long)(kw_t * NKT + kt) * T_] = kw_pend[u][kt];
        }
      }
      kw_n = 0;
    }
  };
  // One K/V tile.  NV = 32-key sub-tiles this wave can see (< NKT only on causal-diagonal or
  // tail tiles: even waves' diagonal tile has its upper half above every query), EDGE = some
  // visible key is masked.  Instantiated per (NV, EDGE) so each path is straight-line code.
  auto body = [&](auto nv_c, auto edge_c, int k0, const char* kb, const char* vb) {
    constexpr int NV = decltype(nv_c)::value;
    constexpr bool EDGE = decltype(edge_c)::value;
    // ---- S^T = K Q^T for the visible 32-key sub-tiles; each K fragment feeds QB MFMAs
    f32x16 s[QB][NV];
    {
      // the NV sub-tiles' chains interleaved, K fragments of step kk+1 read before the MFMAs of
      // step kk: NV reads in flight under every MFMA pair instead of read -> wait -> MFMA
      v8 cur[NV];
#pragma unroll
      for (int kt = 0; kt < NV; ++kt) {
        cur[kt] = *reinterpret_cast<const v8*>(kb + kt * 32 * ROWB + koff[0]);
#pragma unroll
        for (int u = 0; u < QB; ++u) s[u][kt] = f32x16{};
      }
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        v8 nxt[NV];
        if (kk + 1 < KK) {
#pragma unroll
          for (int kt = 0; kt < NV; ++kt) nxt[kt] = *reinterpret_cast<const v8*>(kb + kt * 32 * ROWB + koff[kk + 1]);
        }
        // keep the next step's reads ahead of this step's MFMAs (the scheduler otherwise sinks
        // them to just before their use and every MFMA pair waits on a fresh LDS read)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kt = 0; kt < NV; ++kt)
#pragma unroll
          for (int u = 0; u < QB; ++u) s[u][kt] = Mma<T>::mma(cur[kt], qf[u][kk], s[u][kt]);
        __builtin_amdgcn_sched_barrier(0);
        if (kk + 1 < KK) {
#pragma unroll
          for (int kt = 0; kt < NV; ++kt) cur[kt] = nxt[kt];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < QB; ++u) {
      // ---- mask: key k0 + 4hh + off is visible iff off <= lim (one compare + select each)
      if constexpr (EDGE) {
        const int lim = (causal ? min(qi[u], T_ - 1) : T_ - 1) - (k0 + 4 * hh);
#pragma unroll
        for (int kt = 0; kt < NV; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (kt * 32 + (r & 3) + 8 * (r >> 2) > lim) s[u][kt][r] = -INFINITY;
      }
      // ---- online softmax
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < NV; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[u][kt][r]);
      {  // other half's max: one v_permlane32_swap (no LDS round trip / lgkmcnt wait)
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(mx, fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]))) * c;
      }
      // deferred rescale: only when some lane's max grew by more than kRescaleThr (log2 units);
      // until then P is exponentiated against the stale max and stays below 2^kRescaleThr
      // (fp32 O / l accumulators; bf16 P keeps its relative precision), and the epilogue's
      // lse = m + log2(l) is exact for whatever m the sums were taken against
      if (__builtin_amdgcn_ballot_w64(mx > m[u] + kRescaleThr)) {
        const float mn = fmaxf(m[u], mx);
        const float alpha = __builtin_amdgcn_exp2f(m[u] - mn);
        l[u] *= alpha;
#pragma unroll
        for (int i = 0; i < DT; ++i) o[u][i] *= alpha;
        m[u] = mn;
      }
      float ls = 0.f;
      {  // four partial sums: no 32-deep dependent add chain
        float l4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < NV; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float pv = __builtin_amdgcn_exp2f(fmaf(s[u][kt][r], c, -m[u]));
            l4[r & 3] += pv;
            s[u][kt][r] = pv;
          }
        ls = (l4[0] + l4[1]) + (l4[2] + l4[3]);
      }
      l[u] += ls;
      if constexpr (DROP) {
        // keys (r, r+1) with r even are adjacent: one hash serves both when the row base is even.
        // The keep bits also go to the backward's mask (bit (r&3) + 8(r>>2) + 4hh of the word of
        // this query and 32-key sub-tile; the two lane halves' bits are merged by one swap).
        // Element e0 + o (o = (r&3) + 8(r>>2) <= 27) of this sub-tile row is hashed as pair
        // pb + off: the 64-bit base and both candidate window seeds are formed once per sub-tile,
        // each pair then costs a 32-bit add, a carry select and one mix32 (same values as
        // DropSlab::pair_hash: the low word wraps at most once, into the next window).
        const uint64_t rowbase = dslab + (uint64_t)qi[u] * T_;
#pragma unroll
        for (int kt = 0; kt < NV; ++kt) {
          uint32_t kbits = 0;
          const uint64_t e0 = rowbase + (uint64_t)(k0 + kt * 32 + 4 * hh);
          const uint32_t plo = (uint32_t)(e0 >> 1), phi = (uint32_t)(e0 >> 33);
          const uint32_t smA = phi == ds.hi0 ? ds.sm0 : ds.sm1;
          const uint32_t smB = phi + 1u == ds.hi0 ? ds.sm0 : ds.sm1;
          auto hash_at = [&](uint32_t off) {
            const uint32_t lo = plo + off;
            return mix32(lo ^ (lo < plo ? smB : smA));
          };
          if (dpair) {  // e0 even: keys (r, r+1) share pair pb + o/2
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
              const uint32_t hv = hash_at((uint32_t)(((r & 3) + 8 * (r >> 2)) >> 1));
              const bool k0b = (hv & 0xFFFFu) >= thr, k1b = (hv >> 16) >= thr;
              s[u][kt][r] = k0b ? s[u][kt][r] : 0.f;
              s[u][kt][r + 1] = k1b ? s[u][kt][r + 1] : 0.f;
              kbits |= ((uint32_t)k0b << ((r & 3) + 8 * (r >> 2))) |
                       ((uint32_t)k1b << (((r + 1) & 3) + 8 * (r >> 2)));
            }
          } else {  // odd T or offset: element e0 + o is half (o+par)&1 of pair pb + (o+par)/2
            const int par = (int)(e0 & 1);
            uint32_t hv[4][3];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
              for (int j = 0; j < 3; ++j) hv[g][j] = hash_at((uint32_t)(4 * g + j));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int cr = r & 3;  // compile-time hash indices; par picks between them
              const uint32_t h = par ? hv[r >> 2][(cr + 1) >> 1] : hv[r >> 2][cr >> 1];
              const bool hi = par ? ((cr + 1) & 1) : (cr & 1);
              const bool kb_ = (hi ? (h >> 16) : (h & 0xFFFFu)) >= thr;
              s[u][kt][r] = kb_ ? s[u][kt][r] : 0.f;
              kbits |= (uint32_t)kb_ << ((r & 3) + 8 * (r >> 2));
            }
          }
          if (kmask != nullptr) {
            const uint32_t mine = kbits << (4 * hh);
            const auto sw = __builtin_amdgcn_permlane32_swap(mine, mine, false, false);
            kw_pend[u][kt] = mine | sw[0] | sw[1];
          }
        }
        kw_n = NV;
      }
    }
    // ---- O^T += V^T P^T: P fragments packed from the accumulators, V^T by transposed reads
    //      (each V^T fragment feeds QB MFMAs)
    auto vread = [&](int kt, int s2, int dt) {
      const int off = voff[dt] + (kt * 32 + s2 * 16) * ROWB;
      return tr_read8<v8>(vb, off, off + 8 * ROWB);
    };
    {
      // one flat sequence of (kt, s2, dt) MFMAs with the next V^T fragment read before each one
      constexpr int NPV = NV * 2 * DT;
      v8 vcur = vread(0, 0, 0);
      v8 pf[QB];
#pragma unroll
      for (int i = 0; i < NPV; ++i) {
        const int kt = i / (2 * DT), s2 = (i / DT) & 1, dt = i % DT;
        v8 vnxt;
        if (i + 1 < NPV) vnxt = vread((i + 1) / (2 * DT), ((i + 1) / DT) & 1, (i + 1) % DT);
        if (dt == 0) {
#pragma unroll
          for (int u = 0; u < QB; ++u) {
            uint32_t uu[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) uu[j] = pack2<T>(s[u][kt][8 * s2 + 2 * j], s[u][kt][8 * s2 + 2 * j + 1]);
            __builtin_memcpy(&pf[u], uu, 16);
          }
        }
#pragma unroll
        for (int u = 0; u < QB; ++u) o[u][dt] = Mma<T>::mma(vcur, pf[u], o[u][dt]);
        if (i + 1 < NPV) vcur = vnxt;
      }
    }
  };
  using Ic1 = std::integral_constant<int, 1>;
  using IcN = std::integral_constant<int, NKT>;
  using Yes = std::true_type;
  using No = std::false_type;
  // Interior tiles (no masked key for any of the wave's queries: below the causal diagonal,
  // inside the sequence) form a prefix of the wave's tiles; they run in a loop of their own with
  // the one unmasked body, so the O accumulators never meet the edge variants' registers on the
  // hot path (a shared loop made hipcc copy them between variants every tile).
  const int n_int = wq_hi >= T_ ? 0 : min(min(nact, T_ / FWD_BK), causal ? (wq_lo + 1) / FWD_BK : nact);
  for (; t < n_int; ++t) {
    flush_mask();  // keep bits of tile t - 1
    if (t + NBUF - 1 < ntiles) issue(t + NBUF - 1, buf == 0 ? NBUF - 1 : buf - 1);
    kw_t = t;
    const char* kb = smem + buf * 2 * TILE_B;
    body(IcN{}, No{}, t * FWD_BK, kb, kb + TILE_B);
    ring_wait();  // the DMA of tile t+1 has landed (asm-issued, so drained by hand)
    buf = buf == NBUF - 1 ? 0 : buf + 1;
  }
  // causal diagonal / sequence tail tiles
  for (; t < nact; ++t) {
    flush_mask();
    if (t + NBUF - 1 < ntiles) issue(t + NBUF - 1, buf == 0 ? NBUF - 1 : buf - 1);
    const int k0 = t * FWD_BK;
    kw_t = t;
    const char* kb = smem + buf * 2 * TILE_B;
    const int kvis = min(causal ? wq_hi : T_ - 1, T_ - 1) - k0;  // >= 0 for an active tile
    if (NKT == 1 || kvis >= 32) body(IcN{}, Yes{}, k0, kb, kb + TILE_B);
    else body(Ic1{}, Yes{}, k0, kb, kb + TILE_B);
    ring_wait();
    buf = buf == NBUF - 1 ? 0 : buf + 1;
  }
  flush_mask();
  for (; t < ntiles; ++t) {  // wave done (causal): keep the DMA ring and barriers going
    if (t + NBUF - 1 < ntiles) issue(t + NBUF - 1, buf == 0 ? NBUF - 1 : buf - 1);
    ring_wait();
    buf = buf == NBUF - 1 ? 0 : buf + 1;
  }

  // ---- epilogue: combine the two halves' partial sums, normalise, store O and LSE
#pragma unroll
  for (int u = 0; u < QB; ++u) {
    const float lt = l[u] + __shfl_xor(l[u], 32, 64);
    // dropout's 1 / keep applied once here instead of to every kept probability
    const float inv = lt > 0.f ? (DROP ? inv_keep : 1.f) / lt : 0.f;
    T* orow = out + (BLLM_SEQ_ROW0 + min(qi[u], T_ - 1)) * (long)H * HD + (long)h * HD;
    // 16-B stores (mma.h pair16): lane (q, half hh) holds d = 8 gq + 4 hh + 0..3 of each
    // 32-column tile.  Every lane swaps (cross-lane); only the store is guarded.
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int gq = 0; gq < 4; gq += 2) {
        const uint32_t lo[2] = {pack2<T>(o[u][dt][4 * gq + 0] * inv, o[u][dt][4 * gq + 1] * inv),
                               pack2<T>(o[u][dt][4 * gq + 2] * inv, o[u][dt][4 * gq + 3] * inv)};
        const uint32_t hi[2] = {pack2<T>(o[u][dt][4 * gq + 4] * inv, o[u][dt][4 * gq + 5] * inv),
                                pack2<T>(o[u][dt][4 * gq + 6] * inv, o[u][dt][4 * gq + 7] * inv)};
        const uint4 v = pair16(lo, hi);
        if (qi[u] < T_) *reinterpret_cast<uint4*>(orow + dt * 32 + 8 * gq + 8 * hh) = v;
      }
    if (qi[u] < T_ && hh == 0) lse[BLLM_SEQ_STAT0(h) + qi[u]] = m[u] + log2f(lt);
  }
}

#undef BLLM_SEQ_KERNEL
#undef BLLM_SEQ_T
#undef BLLM_SEQ_CU
#undef BLLM_SEQ_ROW0
#undef BLLM_SEQ_STAT0
#undef BLLM_SEQ_NROWS
#undef BLLM_SEQ_ENTER
