// discover_kernels.hip — discovery and context search (included by index_search.hip after
// reco_kernels.hip): Qdrant's DiscoverQuery ("nearest to this target, but on the positive side of
// these (positive, negative) pairs") and ContextQuery (the pairs alone). Contract: include/ragmi.h
// "Discovery queries", DESIGN.md §R20. A request's n pairs fill the 32 query slots of one pass —
// pair i's positive in slot i, its negative in slot 16 + i, a discover target in slot 15 (its
// partner slot 31 stays zero) — so in the MFMA tile product a lane's acc0 and acc1 hold BOTH
// scores of pair (lane & 15): the pair's sign or loss needs no cross-lane traffic, and a row's
// rank or loss sum is one 16-lane DPP reduction (reco_sum16).
//
// The passes are recommend's (reco_kernels.hip), with this file's bound function:
//  hot: disc_sample_kernel (per sample tile the max of L over matching rows), lk_bound_kernel
//       (eps = 0: T = the k-th largest), disc_collect_kernel (rows with U >= T; kLkCap kept, all
//       counted), disc_rescore_kernel (exact e_x by exact_scores_pairs, combined as the contract
//       says), lk_final_kernel (eps = 0: emit, or tighten T, or leave the request unanswered).
//  full: disc_full_score_kernel, then the full pass's sort and emit.
// Saturation. A score here is discontinuous (a rank is a sum of signs) or saturates (a context
// score is 0 over a large part of the corpus), so a request can have more than kLkCap rows tied
// at the top; no threshold separates them. lk_final_kernel leaves an overflowing request
// unanswered as soon as the tightened threshold — the kept candidates' k-th exact score — is not
// above the round's T; the bound function makes that happen in the FIRST round for the rows that
// saturate exactly: L is the exact score where the certificate proves it (context: every pair
// certainly satisfied, L = 0, the maximum; discover: a zero target scores exactly sig(0), its eps
// is 0), so T already is the tied score and one sample, one collect and the full pass is all a
// saturated request costs.
namespace ragmi {

constexpr int kDiscover = 0, kContext = 1;
constexpr int kDiscTargetSlot = 15;            // the target's slot; pairs 0..14 beside it
constexpr int kDiscMaxPairs = 15;              // ragmi.h RAG_DISCOVER_MAX_PAIRS
constexpr int kCtxMaxPairs = 16;               // ragmi.h RAG_CONTEXT_MAX_PAIRS
// reco_par words this file uses (the buffer is recommend's; its counters [2], [3] are not
// touched, so rag_index_reco_stats does not move): [0] 0.0f, the eps lk_bound_kernel /
// lk_final_kernel subtract; [1] the context half-width w; [4] the target's eps as the bound uses
// it; (ints) [5] candidates the last round that ran counted, [6] rounds run
constexpr int kDiscParW = 1, kDiscParEt = 4, kDiscParCnt = 5, kDiscParRounds = 6;

// example x of a request -> its query slot: x = 2 i the positive of pair i, 2 i + 1 its negative,
// x = 2 n the target
__device__ __forceinline__ int disc_slot(int x, int n) {
  return x == 2 * n ? kDiscTargetSlot : (x & 1) ? kRecoSide + (x >> 1) : (x >> 1);
}

// The contract's discover score: fp32(rank + sig(t)), sig(t) = 0.5 (t / (1 + |t|) + 1) in fp64 on
// the fp32 value, the add in fp64, one rounding. rank is a small integer, exact in fp32.
// Non-decreasing in rank and in t: every fp64 step and the rounding is.
__device__ __forceinline__ float disc_score(float rank, float t) {
  const double td = (double)t;
  return (float)((double)rank + 0.5 * (td / (1.0 + fabs(td)) + 1.0));
}

// The contract's context loss of one pair from d = e_p - e_n - 2^-23 (fp64): m / (1 + |m|),
// m = min(d, 0). <= 0, > -1, non-decreasing in d and 1-Lipschitz (|l'| = 1 / (1 + |m|)^2 <= 1).
__device__ __forceinline__ double ctx_loss(double d) {
  const double m = fmin(d, 0.0);
  return m / (1.0 + fabs(m));
}

// the [32][D] query block of a request (grid 32, block 64): pair i's positive in slot i, its
// negative in slot 16 + i, the target (discover) in slot 15, unused slots zero. qprep_kernel
// (B = 32) then prepares it, as for recommend.
template <int D>
__global__ __launch_bounds__(64) void disc_assemble_kernel(const float* __restrict__ target,
                                                           const float* __restrict__ pos,
                                                           const float* __restrict__ neg, int n,
                                                           float* __restrict__ q32) {
  const int b = blockIdx.x;
  const float* src = nullptr;
  if (b < kRecoSide) {
    if (b < n) src = pos + (int64_t)b * D;
    else if (target && b == kDiscTargetSlot) src = target;
  } else if (b - kRecoSide < n) {
    src = neg + (int64_t)(b - kRecoSide) * D;
  }
  for (int c = threadIdx.x; c < D; c += 64) q32[(int64_t)b * D + c] = src ? src[c] : 0.0f;
}

// after qprep: the request's parameters (one wave).
// Context half-width w. Per pair lane the bound forms dU >= d_i >= dL (disc_bound) and the fp32
// loss lU = fp32(ctx_loss(dU)) (lL likewise); S is their fp32 sum over the 16 lanes (reco_sum16:
// 15 adds), the exact score s = fp32(sum_i l_i), l_i = ctx_loss(d_i) in fp64. ctx_loss is
// non-decreasing, so l_i <= ctx_loss(dU), and
//   s - S_U <= n 2^-25           (each lU's rounding from fp64: |l| < 1, half an ulp <= 2^-25)
//            + 15 n 2^-24        (<= 15 fp32 roundings of partial sums, each partial <= n in
//                                 magnitude as |l| < 1: half an ulp <= n 2^-24)
//            + n 2^-24           (s's own rounding from fp64; the fp64 accumulation's error is
//                                 far below it)
//            + 2 n 2^-24         (the fp32 rounding of S +- w itself, |S +- w| < 2 n)
// and the mirror for S_L: below 18.5 n 2^-24 < n 2^-19 = w, exact in fp32. The eps of the
// examples are inside dU / dL, not in w: the loss is 1-Lipschitz but clamps at 0, and widening d
// keeps a certainly satisfied pair at exactly 0.
// Discover target eps. A zero target (zero or non-finite vector) has all-zero fragments and an
// all-zero qn: its MFMA score and its exact score are both exactly 0 for every row, so the bound
// may take eps_t = 0 — which makes L = U = the exact score for a row whose pairs are all certain.
template <int D>
__global__ __launch_bounds__(64) void disc_prep_kernel(const float* __restrict__ eps,
                                                       const float* __restrict__ qn, int n,
                                                       float* __restrict__ par) {
  const int lane = threadIdx.x;
  bool nz = false;
  for (int c = lane; c < D; c += 64) nz = nz || qn[kDiscTargetSlot * D + c] != 0.0f;
  const bool any = __any(nz);
  if (lane != 0) return;
  par[kRecoParZero] = 0.0f;
  par[kDiscParW] = (float)n * 0x1p-19f;
  par[kDiscParEt] = any ? eps[kDiscTargetSlot] : 0.0f;
}

// this lane's part of a request: whether (lane & 15) is a pair / the target's lane, the qprep
// bounds of its two slots (ea of the target's lane: the target's), the context half-width
struct DiscLane {
  bool pair, tgt;
  float ea, eb;
  float w;
};

template <int KIND>
__device__ __forceinline__ DiscLane disc_lane(const float* __restrict__ eps,
                                              const float* __restrict__ par, int n, int lane) {
  DiscLane q;
  q.pair = (lane & 15) < n;
  q.tgt = KIND == kDiscover && (lane & 15) == kDiscTargetSlot;
  q.ea = q.tgt ? par[kDiscParEt] : eps[lane & 15];
  q.eb = eps[kRecoSide + (lane & 15)];
  q.w = par[kDiscParW];
  return q;
}

// The certified bound of a tile's rows from its MFMA scores (acc0: slot l & 15, acc1: slot
// 16 + (l & 15); lane l holds rows 4 (l >> 4) + r, r < 4). Returns, in every lane, the bound of
// row 4 (l >> 4) + (l & 3) of the tile: UPPER ? U : L with L <= exact score <= U.
// a +- eps is formed in fp32 and still bounds e (reco_bound: eps carries 2^-22 of absolute slack,
// the rounding is below 2^-23). With xl = a_p - eps_p <= e_p <= xu = a_p + eps_p and yl / yu for
// the negative:
//   DISCOVER: xl > yu proves e_p > e_n (the term is +1), xu < yl proves e_p < e_n (-1); otherwise
//   the term is +1 in U and -1 in L, the exact tie's 0 between them. The terms are summed over
//   the 16 lanes (small integers: exact), the target's a_t +- eps_t comes from lane 15 of the DPP
//   row (a max over the row with -inf elsewhere), and U / L = disc_score(rank, t), the contract's
//   own function, monotone in both.
//   CONTEXT: d_i = e_p - e_n - 2^-23. dU = fl(xu - yl) >= d_i: |xu - yl| < 4, so the rounding is
//   at most 2^-23, what the contract subtracts. dL = fl(fl(xl - yu) - 2^-21) <= d_i: the two
//   roundings add at most 2^-22 and the contract's 2^-23 fits in the rest. U = min(S_U + w, 0)
//   and L = S_L - w (disc_prep_kernel); the clamp is safe because every l_i <= 0, so the exact
//   score is <= 0. When S_L == 0 every lL is 0 (they are <= 0, and a sum of non-positive fp32
//   numbers is 0 only if all are), so every dL >= 0, every d_i >= 0, every l_i = 0 and the exact
//   score is exactly 0: L = 0 then, not -w.
template <int KIND, bool UPPER>
__device__ __forceinline__ float disc_bound(const floatx4& acc0, const floatx4& acc1,
                                            const DiscLane& q, int lane) {
  const int r = lane & 3;
  if constexpr (KIND == kDiscover) {
    const float dt = UPPER ? q.ea : -q.ea;
    float rk[4], tg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float term = 0.0f;
      if (q.pair) {
        if (UPPER) term = (acc0[i] + q.ea < acc1[i] - q.eb) ? -1.0f : 1.0f;
        else term = (acc0[i] - q.ea > acc1[i] + q.eb) ? 1.0f : -1.0f;
      }
      rk[i] = reco_sum16(term);
      tg[i] = reco_max16(q.tgt ? acc0[i] + dt : kNegInf);
    }
    const float k = r == 0 ? rk[0] : r == 1 ? rk[1] : r == 2 ? rk[2] : rk[3];
    const float t = r == 0 ? tg[0] : r == 1 ? tg[1] : r == 2 ? tg[2] : tg[3];
    return disc_score(k, t);
  } else {
    float s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float l = 0.0f;
      if (q.pair) {
        const float d = UPPER ? (acc0[i] + q.ea) - (acc1[i] - q.eb)
                              : ((acc0[i] - q.ea) - (acc1[i] + q.eb)) - 0x1p-21f;
        if (d < 0.0f) l = (float)ctx_loss((double)d);
      }
      s[i] = reco_sum16(l);
    }
    const float x = r == 0 ? s[0] : r == 1 ? s[1] : r == 2 ? s[2] : s[3];
    if (UPPER) return fminf(x + q.w, 0.0f);
    return x == 0.0f ? 0.0f : x - q.w;
  }
}

// step 1: smax[j] = max over the matching rows of sample tile j of L(r), -inf where none
// (reco_sample_kernel's shape)
template <int D, bool FILTER, int KIND>
__global__ __launch_bounds__(256) void disc_sample_kernel(const half8* __restrict__ corpus,
                                                          const uint32_t* __restrict__ tags,
                                                          const uint32_t* __restrict__ filt,
                                                          const half8* __restrict__ qfrag,
                                                          const float* __restrict__ eps,
                                                          const float* __restrict__ par, int n,
                                                          int n_rows, int n_tiles, int n_sample,
                                                          float* __restrict__ smax) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (j >= n_sample) return;
  const int t = (int)(((int64_t)j * n_tiles) / n_sample);
  const DiscLane q = disc_lane<KIND>(eps, par, n, lane);
  uint32_t fm = 0, fv = 0;
  if constexpr (FILTER) {
    fm = filt[0];
    fv = filt[1];
  }
  floatx4 acc0, acc1;
  reco_tile_scores<D>(corpus, t, qfrag, lane, acc0, acc1);
  const float lo = disc_bound<KIND, false>(acc0, acc1, q, lane);
  const int row = t * kTileRows + 4 * (lane >> 4) + (lane & 3);
  float m = reco_row_ok<FILTER>(lane, row, n_rows, tags, fm, fv) ? lo : kNegInf;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  if (lane == 0) smax[j] = m;
}

// step 2: every tile, one wave per tile per step (grid-stride, reco_collect_kernel's shape): the
// matching rows with U >= thr[0] appended to cand (kLkCap kept, cnt[0] counts all).
// round > 0: only if the previous round asked for it.
template <int D, bool FILTER, int KIND>
__global__ __launch_bounds__(256) void disc_collect_kernel(const half8* __restrict__ corpus,
                                                           const uint32_t* __restrict__ tags,
                                                           const uint32_t* __restrict__ filt,
                                                           const half8* __restrict__ qfrag,
                                                           const float* __restrict__ eps,
                                                           const float* __restrict__ par, int n,
                                                           int n_rows, int n_tiles,
                                                           const float* __restrict__ thr,
                                                           int* __restrict__ cnt,
                                                           int* __restrict__ cand,
                                                           const int* __restrict__ again,
                                                           const int* __restrict__ need,
                                                           int round) {
  constexpr int S = steps<D>();
  if (!need[round] || !again[0]) return;
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * 4;
  const int w0 = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const DiscLane q = disc_lane<KIND>(eps, par, n, lane);
  const float T = thr[0];
  uint32_t fm = 0, fv = 0;
  if constexpr (FILTER) {
    fm = filt[0];
    fv = filt[1];
  }
  // D <= 384: the fragments of both slot halves stay in registers for the whole launch
  // (reco_collect_kernel); wider rows re-read them per chunk
  constexpr bool QREG = S <= 12;
  half8 qra[QREG ? S : 1], qrb[QREG ? S : 1];
  if constexpr (QREG) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      qra[s] = qfrag[s * 64 + lane];
      qrb[s] = qfrag[(S + s) * 64 + lane];
    }
  }
  for (int t = w0; t < n_tiles; t += nw) {
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (QREG) {
      const half8* p = corpus + (int64_t)t * (S * 64) + lane;
      half8 a[S];
#pragma unroll
      for (int s = 0; s < S; ++s) a[s] = __builtin_nontemporal_load(p + s * 64);
      tile_mfma<S>(a, qra, qrb, acc0, acc1);
    } else {
      reco_tile_scores<D>(corpus, t, qfrag, lane, acc0, acc1);
    }
    const float hi = disc_bound<KIND, true>(acc0, acc1, q, lane);
    const int row = t * kTileRows + 4 * (lane >> 4) + (lane & 3);
    if (reco_row_ok<FILTER>(lane, row, n_rows, tags, fm, fv) && hi >= T) {
      const int pos = atomicAdd(&cnt[0], 1);
      if (pos < kLkCap) cand[pos] = row;
    }
  }
}

// The exact scores of up to G = reco_group(E) rows by one wave, E = 2 n (+ 1 with a target)
// examples: the gather is recommend's (reco_gather_group: lane g E + x holds e of row g against
// example x, every slot of every trip but the last a real pair), then the contract's combine in
// lane g, the pairs in order. Returns row (lane)'s score in lanes < G, whatever elsewhere.
__host__ __device__ __forceinline__ int disc_examples(int kind, int n) {
  return 2 * n + (kind == kDiscover ? 1 : 0);
}

template <int D, typename RowFn>
__device__ __forceinline__ float disc_exact_group(const half8* __restrict__ corpus,
                                                  const float* __restrict__ rows32,
                                                  const float* __restrict__ qn, int kind, int n,
                                                  RowFn row_of, int lane) {
  const int E = disc_examples(kind, n);
  const float val = reco_gather_group<D>(
      corpus, rows32, qn, E, [&](int x) { return disc_slot(x, n); }, row_of, lane);
  float rank = 0.0f;
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    const float ep = __shfl(val, (lane * E + 2 * i) & 63, 64);
    const float en = __shfl(val, (lane * E + 2 * i + 1) & 63, 64);
    if (kind == kDiscover)
      rank += ep > en ? 1.0f : ep < en ? -1.0f : 0.0f;
    else
      sum += ctx_loss((double)ep - (double)en - 0x1p-23);
  }
  float s;
  if (kind == kDiscover) {
    const float et = __shfl(val, (lane * E + 2 * n) & 63, 64);
    s = disc_score(rank, et);
  } else {
    s = (float)sum;
  }
  if (s == 0.0f) s = 0.0f;   // -0 and +0 compare equal: one key for both
  return s;
}

// step 3a: exact scores of the kept candidates -> es_g (reco_rescore_kernel's shape and
// per-workgroup share); workgroup 0 notes the round's count for rag_index_discover_stats.
// (Nothing resets those two words per request: they are the last hot pass's that ran a round —
// round 0 always runs, except over an index without rows, where the stats keep the previous
// request's values, as recommend's do.)
template <int D>
__global__ __launch_bounds__(256) void disc_rescore_kernel(const half8* __restrict__ corpus,
                                                           const float* __restrict__ qn, int kind,
                                                           int n, const int* __restrict__ cnt,
                                                           const int* __restrict__ cand,
                                                           const int* __restrict__ again,
                                                           const int* __restrict__ need, int round,
                                                           float* __restrict__ es_g,
                                                           const float* __restrict__ rows32,
                                                           float* __restrict__ par) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (!need[round] || !again[0]) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    reinterpret_cast<int*>(par)[kDiscParCnt] = cnt[0];
    reinterpret_cast<int*>(par)[kDiscParRounds] = round + 1;
  }
  const int m = min(cnt[0], kLkCap);
  const int E = disc_examples(kind, n);
  const int G = reco_group(E), per_wg = reco_rescore_per_wg(E);
  const int c0 = blockIdx.x * per_wg, c1 = min(m, c0 + per_wg);
  for (int i0 = c0 + wid * G; i0 < c1; i0 += 4 * G) {
    const float s = disc_exact_group<D>(
        corpus, rows32, qn, kind, n, [&](int g) { return i0 + g < c1 ? cand[i0 + g] : -1; },
        lane);
    if (lane < G && i0 + lane < c1) es_g[i0 + lane] = s;
  }
}

// full pass: every row's exact score -> (key, row) for the full pass's sort
// (reco_full_score_kernel's shape: key 0 for a row the filter refuses)
template <int D, bool FILTER>
__global__ __launch_bounds__(256) void disc_full_score_kernel(const half8* __restrict__ corpus,
                                                              const uint32_t* __restrict__ tags,
                                                              const uint32_t* __restrict__ filt,
                                                              const float* __restrict__ qn,
                                                              int kind, int n, int n_rows,
                                                              const float* __restrict__ rows32,
                                                              uint32_t* __restrict__ keys,
                                                              int* __restrict__ vals,
                                                              int* __restrict__ n_match) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = gridDim.x * 4;
  const int G = reco_group(disc_examples(kind, n));
  uint32_t fm = 0, fv = 0;
  if constexpr (FILTER) {
    fm = filt[0];
    fv = filt[1];
  }
  int m = 0;
  for (int64_t r0 = (int64_t)wave * G; r0 < n_rows; r0 += (int64_t)nw * G) {
    const float s = disc_exact_group<D>(
        corpus, rows32, qn, kind, n,
        [&](int g) { return r0 + g < n_rows ? (int)(r0 + g) : -1; }, lane);
    const int64_t row = r0 + lane;
    if (lane < G && row < n_rows) {
      bool ok = true;
      if constexpr (FILTER) ok = (tags[row] & fm) == fv;
      keys[row] = ok ? fkey(s) : 0u;
      vals[row] = (int)row;
      m += ok ? 1 : 0;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m += __shfl_xor(m, d, 64);
  if (lane == 0 && m > 0) atomicAdd(n_match, m);
}

// diagnostic (rag_index_discover_bounds): the hot pass's [L, U] of rows[i], one wave per row, by
// the pass's own tile arithmetic and bound function. A row outside [0, n_rows) is never read:
// (-inf, +inf).
template <int D, int KIND>
__global__ __launch_bounds__(64) void disc_bounds_kernel(const half8* __restrict__ corpus,
                                                         const half8* __restrict__ qfrag,
                                                         const float* __restrict__ eps,
                                                         const float* __restrict__ par, int n_pairs,
                                                         const int64_t* __restrict__ rows,
                                                         int64_t n, int64_t n_rows,
                                                         float* __restrict__ out_lo,
                                                         float* __restrict__ out_hi) {
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int lane = threadIdx.x;
  const int64_t row = rows[i];
  if (row < 0 || row >= n_rows) {
    if (lane == 0) {
      out_lo[i] = kNegInf;
      out_hi[i] = __builtin_inff();
    }
    return;
  }
  const DiscLane q = disc_lane<KIND>(eps, par, n_pairs, lane);
  floatx4 acc0, acc1;
  reco_tile_scores<D>(corpus, row >> 4, qfrag, lane, acc0, acc1);
  const float lo = disc_bound<KIND, false>(acc0, acc1, q, lane);
  const float hi = disc_bound<KIND, true>(acc0, acc1, q, lane);
  // the lane that holds this row: group (row & 15) >> 2, r = row & 3
  if (lane == (int)(((row & 15) >> 2) * 16 + (row & 3))) {
    out_lo[i] = lo;
    out_hi[i] = hi;
  }
}

}  // namespace ragmi
