// reco_kernels.hip — recommend queries (included by index_search.hip after largek_kernels.hip):
// "more like these points, less like those" (Qdrant's RecommendQuery; contract in
// include/ragmi.h "Recommend queries"). One request's P positive and N negative
// examples fill the 32 query slots of a pass — positives from slot 0, negatives from slot 16 —
// so the MFMA tile product scores every example against 16 rows at once: a lane's acc0 holds
// slot (lane & 15), a positive, and its acc1 slot 16 + (lane & 15), a negative, and a row's
// "best positive" / "best negative" / "sum" is one reduction over the 16 lanes of a DPP row.
//
// Hot pass (BEST_SCORE, SUM_SCORES; k <= RAG_MAX_K_LARGE), one stream of the fp16 rows:
//  1. reco_sample_kernel over n_sample tiles (the large-k pass's choice): per tile the max over
//     matching rows of L(r), a lower bound of the row's exact combined score. lk_bound_kernel
//     (eps = 0): T = the k-th largest maximum. They come from k distinct rows with exact score
//     >= L, so the k-th best exact score is >= T. Fewer than k finite maxima: T = -inf.
//  2. reco_collect_kernel: every tile scored; each matching row with U(r) >= T, U an upper bound
//     of its exact combined score, is appended to the candidate list (kLkCap kept, all counted).
//  3. reco_rescore_kernel: the candidates' exact e_i (exact_scores_pairs) combined exactly as the
//     contract says; lk_final_kernel (eps = 0) emits the k best by (score desc, row asc), or on
//     overflow tightens T to the kept candidates' k-th exact score and asks for another round;
//     a request still overflowing after kLkRounds is counted unanswered, never truncated.
// Full pass: reco_full_score_kernel scores every row exactly, then the full pass's sort and emit.
namespace ragmi {

constexpr int kRecoSide = 16;   // examples per side (ragmi.h RAG_RECO_MAX_SIDE)
constexpr int kRecoAverage = 0, kRecoBest = 1, kRecoSum = 2;   // ragmi.h RAG_RECO_*
// reco_par (floats): [0] 0.0f — the eps lk_bound_kernel / lk_final_kernel subtract: L and U are
// bounds already —, [1] the SUM_SCORES half-width; (ints) [2] candidates the last round that ran
// counted, [3] rounds run
constexpr int kRecoParZero = 0, kRecoParWsum = 1, kRecoParCnt = 2, kRecoParRounds = 3;

// slot of example x (positives first): positives from 0, negatives from 16
__device__ __forceinline__ int reco_slot(int x, int P) { return x < P ? x : kRecoSide + (x - P); }

// sig(x) = 0.5 (x / (1 + |x|) + 1) in fp64 on the fp32 value, rounded once to fp32. Every step
// (the exact widening, 1 + |x|, the IEEE division, + 1, the exact halving, the rounding) is
// non-decreasing in x, so sig is; sig >= 0 as x / (1 + |x|) >= -1.
__device__ __forceinline__ float reco_sig(float x) {
  const double xd = (double)x;
  return (float)(0.5 * (xd / (1.0 + fabs(xd)) + 1.0));
}

// F of the contract: sig(mp) if mp > mn else -sig(mn); mp / mn = -inf for an empty side (not
// both). Non-decreasing in mp and non-increasing in mn, the step at mp = mn included: the
// branch mp > mn gives a value >= 0, the other one <= 0. sig is evaluated on the finite
// argument of the branch taken only.
__device__ __forceinline__ float reco_best(float mp, float mn) {
  const bool pos = mp > mn;
  const float s = reco_sig(pos ? mp : mn);
  return pos ? s : -s;
}

// the [32][D] query block of a request: positives from slot 0, negatives from slot 16, unused
// slots zero (grid 32, block 64). qprep_kernel(B = 32) then prepares it: an unused slot is a
// zero query (qn = 0, fragments 0), and so is a zero-vector example, which scores exactly 0
// against every row.
template <int D>
__global__ __launch_bounds__(64) void reco_assemble_kernel(const float* __restrict__ pos, int P,
                                                           const float* __restrict__ neg, int N,
                                                           float* __restrict__ q32) {
  const int b = blockIdx.x;
  const float* src = nullptr;
  if (b < kRecoSide) {
    if (b < P) src = pos + (int64_t)b * D;
  } else if (b - kRecoSide < N) {
    src = neg + (int64_t)(b - kRecoSide) * D;
  }
  for (int c = threadIdx.x; c < D; c += 64) q32[(int64_t)b * D + c] = src ? src[c] : 0.0f;
}

// after qprep: the request's parameters. SUM_SCORES half-width: the row's combined MFMA sum S
// (fp32, reduced over 16 lanes) against the exact score s = fp32(sum e_i - sum e_j):
//   |S - s| <= sum_i eps_i                      (each |a_i - e_i| <= eps_i, qprep)
//            + 31 * 2^-24 * 36                  (<= 31 fp32 roundings of partial sums, each
//                                                partial <= 32 * 1.1 < 36 in magnitude)
//            + 2^-24 * 36                       (s's own rounding from fp64; the fp64
//                                                accumulation's error is far below it)
//            + 2^-24 * 40                       (the fp32 rounding of S +- w itself)
// The last three are below 34 * 40 * 2^-24 < 2^-13.5; w = sum eps_i + 2^-12, rounded up.
__global__ __launch_bounds__(64) void reco_prep_kernel(const float* __restrict__ eps, int P, int N,
                                                       float* __restrict__ par) {
  if (threadIdx.x != 0) return;
  double w = 0.0;
  for (int i = 0; i < P; ++i) w += (double)eps[i];
  for (int j = 0; j < N; ++j) w += (double)eps[kRecoSide + j];
  w = (w + 0x1p-12) * (1.0 + 0x1p-20);
  float wf = (float)w;
  if ((double)wf < w) wf = nextafterf(wf, __builtin_inff());
  par[kRecoParZero] = 0.0f;
  par[kRecoParWsum] = wf;   // (the counters stay: they are the last HOT pass's, whose round 0
                            // always runs and writes them — reco_rescore_kernel)
}

// AVERAGE_VECTOR's target v from the normalised examples qn [32][D]: one thread per component,
// the examples in order, in fp64, one rounding
__global__ __launch_bounds__(256) void reco_average_kernel(const float* __restrict__ qn, int D,
                                                           int P, int N, float* __restrict__ v) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  double sp = 0.0;
  for (int i = 0; i < P; ++i) sp += (double)qn[(int64_t)i * D + c];
  const double ap = sp / (double)P;
  double t = ap;
  if (N > 0) {
    double sn = 0.0;
    for (int j = 0; j < N; ++j) sn += (double)qn[(int64_t)(kRecoSide + j) * D + c];
    const double an = sn / (double)N;
    t = ap + (ap - an);
  }
  v[c] = (float)t;
}

// this lane's two slots of a request: whether they hold an example and their qprep bound
struct RecoLane {
  bool la, lb;
  float ea, eb;
  float wsum;
};

__device__ __forceinline__ RecoLane reco_lane(const float* __restrict__ eps,
                                              const float* __restrict__ par, int P, int N,
                                              int lane) {
  RecoLane q;
  q.la = (lane & 15) < P;
  q.lb = (lane & 15) < N;
  q.ea = eps[lane & 15];
  q.eb = eps[kRecoSide + (lane & 15)];
  q.wsum = par[kRecoParWsum];
  return q;
}

__device__ __forceinline__ float reco_max16(float v) {
  v = fmax_nc(v, xor_lane_f<1>(v));
  v = fmax_nc(v, xor_lane_f<2>(v));
  v = fmax_nc(v, xor_lane_f<4>(v));
  return fmax_nc(v, xor_lane_f<8>(v));
}

__device__ __forceinline__ float reco_sum16(float v) {
  v += xor_lane_f<1>(v);
  v += xor_lane_f<2>(v);
  v += xor_lane_f<4>(v);
  return v + xor_lane_f<8>(v);
}

// The certified bound of a tile's rows from its MFMA scores (acc0: positives, acc1: negatives;
// lane l holds rows 4 (l >> 4) + r, r < 4, of slots l & 15 and 16 + (l & 15)). Returns, in
// every lane, the bound of row 4 (l >> 4) + (l & 3) of the tile: UPPER ? U : L with
// L <= exact combined score <= U.
//   BEST: mpU = max_i (a_i + eps_i), mpL = max_i (a_i - eps_i), mnU / mnL likewise, unused slots
//   -inf; U = F(mpU, mnL), L = F(mpL, mnU) by F's monotonicity. a_i +- eps_i is formed in fp32:
//   eps_i carries 2^-22 of absolute slack beyond the proven bound (qprep_slot) and the sum's
//   rounding is at most 2^-24 * |a_i +- eps_i| < 2^-23, so the rounded value still bounds e_i.
//   SUM: S -+ wsum (reco_prep_kernel).
template <int STRAT, bool UPPER>
__device__ __forceinline__ float reco_bound(const floatx4& acc0, const floatx4& acc1,
                                            const RecoLane& q, int lane) {
  const int r = lane & 3;
  if constexpr (STRAT == kRecoBest) {
    // the positive side moves with the bound, the negative side against it
    const float dp = UPPER ? q.ea : -q.ea, dn = UPPER ? -q.eb : q.eb;
    float mp[4], mn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mp[i] = reco_max16(q.la ? acc0[i] + dp : kNegInf);
      mn[i] = reco_max16(q.lb ? acc1[i] + dn : kNegInf);
    }
    const float p = r == 0 ? mp[0] : r == 1 ? mp[1] : r == 2 ? mp[2] : mp[3];
    const float n = r == 0 ? mn[0] : r == 1 ? mn[1] : r == 2 ? mn[2] : mn[3];
    return reco_best(p, n);
  } else {
    float s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      s[i] = reco_sum16((q.la ? acc0[i] : 0.0f) - (q.lb ? acc1[i] : 0.0f));
    const float x = r == 0 ? s[0] : r == 1 ? s[1] : r == 2 ? s[2] : s[3];
    return UPPER ? x + q.wsum : x - q.wsum;
  }
}

// MFMA scores of tile t against the request's 32 slots, the k-steps in order (the same
// accumulation order in every kernel of the pass, so sample, collect and the diagnostic bounds
// see the same a_i): fragments from global memory in chunks of 8 (D = 384: 4) k-steps
template <int D>
__device__ __forceinline__ void reco_tile_scores(const half8* __restrict__ corpus, int64_t t,
                                                 const half8* __restrict__ qfrag, int lane,
                                                 floatx4& acc0, floatx4& acc1) {
  constexpr int S = steps<D>();
  acc0 = acc1 = floatx4{0.f, 0.f, 0.f, 0.f};
  tile_scores_chunked<S, S % 8 == 0 ? 8 : 4>(corpus + t * (S * 64) + lane, qfrag, lane, acc0,
                                             acc1);
}

// does the lane's row (l & 15 < 4: row 16 t + 4 (l >> 4) + (l & 3)) exist and pass the filter?
template <bool FILTER>
__device__ __forceinline__ bool reco_row_ok(int lane, int row, int n_rows,
                                            const uint32_t* __restrict__ tags, uint32_t fm,
                                            uint32_t fv) {
  bool ok = (lane & 15) < 4 && row < n_rows;
  if constexpr (FILTER) ok = ok && ((tags[ok ? row : 0] & fm) == fv);
  return ok;
}

// step 1: smax[j] = max over the matching rows of sample tile j of L(r), -inf where none
// (one wave per sample tile, tile (j n_tiles) / n_sample as sample_tiles spreads them)
template <int D, bool FILTER, int STRAT>
__global__ __launch_bounds__(256) void reco_sample_kernel(const half8* __restrict__ corpus,
                                                          const uint32_t* __restrict__ tags,
                                                          const uint32_t* __restrict__ filt,
                                                          const half8* __restrict__ qfrag,
                                                          const float* __restrict__ eps,
                                                          const float* __restrict__ par, int P,
                                                          int N, int n_rows, int n_tiles,
                                                          int n_sample, float* __restrict__ smax) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (j >= n_sample) return;
  const int t = (int)(((int64_t)j * n_tiles) / n_sample);
  const RecoLane q = reco_lane(eps, par, P, N, lane);
  uint32_t fm = 0, fv = 0;
  if constexpr (FILTER) {
    fm = filt[0];
    fv = filt[1];
  }
  floatx4 acc0, acc1;
  reco_tile_scores<D>(corpus, t, qfrag, lane, acc0, acc1);
  const float lo = reco_bound<STRAT, false>(acc0, acc1, q, lane);
  const int row = t * kTileRows + 4 * (lane >> 4) + (lane & 3);
  float m = reco_row_ok<FILTER>(lane, row, n_rows, tags, fm, fv) ? lo : kNegInf;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  if (lane == 0) smax[j] = m;
}

// step 2: every tile, one wave per tile per step (grid-stride, lk_collect_kernel's shape): the
// matching rows with U >= thr[0] appended to cand (kLkCap kept, cnt[0] counts all).
// round > 0: only if the previous round asked for it.
template <int D, bool FILTER, int STRAT>
__global__ __launch_bounds__(256) void reco_collect_kernel(const half8* __restrict__ corpus,
                                                           const uint32_t* __restrict__ tags,
                                                           const uint32_t* __restrict__ filt,
                                                           const half8* __restrict__ qfrag,
                                                           const float* __restrict__ eps,
                                                           const float* __restrict__ par, int P,
                                                           int N, int n_rows, int n_tiles,
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
  const RecoLane q = reco_lane(eps, par, P, N, lane);
  const float T = thr[0];
  uint32_t fm = 0, fv = 0;
  if constexpr (FILTER) {
    fm = filt[0];
    fv = filt[1];
  }
  // D <= 384: the fragments of both sides stay in registers for the whole launch
  // (lk_collect_kernel); wider rows re-read them per chunk
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
    const float hi = reco_bound<STRAT, true>(acc0, acc1, q, lane);
    const int row = t * kTileRows + 4 * (lane >> 4) + (lane & 3);
    if (reco_row_ok<FILTER>(lane, row, n_rows, tags, fm, fv) && hi >= T) {
      const int pos = atomicAdd(&cnt[0], 1);
      if (pos < kLkCap) cand[pos] = row;
    }
  }
}

// The exact combined scores of up to G = reco_group(E) rows by one wave, E = P + N: the G E
// (row, example) pairs of the group, pair p = g E + x, scored 8 per memory round trip
// (exact_scores_pairs) in reco_trips(E) trips, pair p's e_i(r) landing in lane p — G E <= 64, and
// every slot of every trip but the last is a real pair —, then the combine of the contract.
// row_of(g) (wave-uniform) is row g of the group, -1 for none. Returns row (lane)'s score in
// lanes < G, whatever elsewhere.
__host__ __device__ __forceinline__ int reco_group(int E) { return E <= 8 ? 8 : 64 / E; }
__host__ __device__ __forceinline__ int reco_trips(int E) { return (reco_group(E) * E + 7) / 8; }

// the gather half: lane p's e of pair p = g E + x, x's query slot being slot_of(x) (shared with
// discover_kernels.hip)
template <int D, typename SlotFn, typename RowFn>
__device__ __forceinline__ float reco_gather_group(const half8* __restrict__ corpus,
                                                   const float* __restrict__ rows32,
                                                   const float* __restrict__ qn, int E,
                                                   SlotFn slot_of, RowFn row_of, int lane) {
  constexpr int NC = 8;
  const int G = reco_group(E);
  const int trips = reco_trips(E);
  float val = 0.0f;   // lane p holds pair p = g E + x of the group
  for (int t = 0; t < trips; ++t) {
    int rows[NC], qoff[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int p = t * NC + j, g = p / E, x = p - g * E;
      rows[j] = g < G ? row_of(g) : -1;
      qoff[j] = slot_of(x) * D;
    }
    float sc[NC];
    exact_scores_pairs<D, NC>(corpus, rows, qoff, qn, lane, sc, rows32);
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lane == t * NC + j) val = sc[j];
  }
  return val;
}

template <int D, typename RowFn>
__device__ __forceinline__ float reco_exact_group(const half8* __restrict__ corpus,
                                                  const float* __restrict__ rows32,
                                                  const float* __restrict__ qn, int P, int N,
                                                  int strat, RowFn row_of, int lane) {
  const int E = P + N;
  const float val = reco_gather_group<D>(
      corpus, rows32, qn, E, [&](int x) { return reco_slot(x, P); }, row_of, lane);
  // lane g combines pairs g E .. g E + E - 1 in example order, positives first
  float mp = kNegInf, mn = kNegInf;
  double sum = 0.0;
  for (int x = 0; x < E; ++x) {
    const float e = __shfl(val, (lane * E + x) & 63, 64);
    if (x < P) {
      mp = fmaxf(mp, e);
      sum += (double)e;
    } else {
      mn = fmaxf(mn, e);
      sum -= (double)e;
    }
  }
  float s = strat == kRecoBest ? reco_best(mp, mn) : (float)sum;
  if (s == 0.0f) s = 0.0f;   // -0 and +0 compare equal: one key for both
  return s;
}

// step 3a: exact combined scores of the kept candidates -> es_g, `per_wg` candidates per
// workgroup (grid kLkCap / per_wg, reco_rescore_per_wg); workgroup 0 notes the round's count for
// rag_index_reco_stats. per_wg: each wave takes whole groups, about 8 memory round trips in
// all — with 256 candidates per workgroup whatever E, a (16, 16) request's ~600 candidates were
// 256 dependent round trips per wave: 2.65 ms per request at 10M rows against 1.32 ms for (1, 0)
__host__ __device__ __forceinline__ int reco_rescore_per_wg(int E) {
  const int trips = reco_trips(E);
  return 4 * reco_group(E) * (trips >= 8 ? 1 : 8 / trips);
}

template <int D>
__global__ __launch_bounds__(256) void reco_rescore_kernel(const half8* __restrict__ corpus,
                                                           const float* __restrict__ qn, int P,
                                                           int N, int strat,
                                                           const int* __restrict__ cnt,
                                                           const int* __restrict__ cand,
                                                           const int* __restrict__ again,
                                                           const int* __restrict__ need, int round,
                                                           float* __restrict__ es_g,
                                                           const float* __restrict__ rows32,
                                                           float* __restrict__ par) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (!need[round] || !again[0]) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    reinterpret_cast<int*>(par)[kRecoParCnt] = cnt[0];
    reinterpret_cast<int*>(par)[kRecoParRounds] = round + 1;
  }
  const int n = min(cnt[0], kLkCap);
  const int G = reco_group(P + N), per_wg = reco_rescore_per_wg(P + N);
  const int c0 = blockIdx.x * per_wg, c1 = min(n, c0 + per_wg);
  for (int i0 = c0 + wid * G; i0 < c1; i0 += 4 * G) {
    const float s = reco_exact_group<D>(
        corpus, rows32, qn, P, N, strat, [&](int g) { return i0 + g < c1 ? cand[i0 + g] : -1; },
        lane);
    if (lane < G && i0 + lane < c1) es_g[i0 + lane] = s;
  }
}

// full pass: every row's exact combined score -> (key, row) for the full pass's sort
// (full_score_kernel's outputs: key 0 for a row the filter refuses)
template <int D, bool FILTER>
__global__ __launch_bounds__(256) void reco_full_score_kernel(const half8* __restrict__ corpus,
                                                              const uint32_t* __restrict__ tags,
                                                              const uint32_t* __restrict__ filt,
                                                              const float* __restrict__ qn, int P,
                                                              int N, int strat, int n_rows,
                                                              const float* __restrict__ rows32,
                                                              uint32_t* __restrict__ keys,
                                                              int* __restrict__ vals,
                                                              int* __restrict__ n_match) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = gridDim.x * 4;
  const int G = reco_group(P + N);
  uint32_t fm = 0, fv = 0;
  if constexpr (FILTER) {
    fm = filt[0];
    fv = filt[1];
  }
  int m = 0;
  for (int64_t r0 = (int64_t)wave * G; r0 < n_rows; r0 += (int64_t)nw * G) {
    const float s = reco_exact_group<D>(
        corpus, rows32, qn, P, N, strat,
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

// diagnostic (rag_index_reco_bounds): the hot pass's [L, U] of rows[i], one wave per row, by the
// pass's own tile arithmetic and bound function. A row outside [0, n_rows) is never read:
// (-inf, +inf).
template <int D, int STRAT>
__global__ __launch_bounds__(64) void reco_bounds_kernel(const half8* __restrict__ corpus,
                                                         const half8* __restrict__ qfrag,
                                                         const float* __restrict__ eps,
                                                         const float* __restrict__ par, int P,
                                                         int N, const int64_t* __restrict__ rows,
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
  const RecoLane q = reco_lane(eps, par, P, N, lane);
  floatx4 acc0, acc1;
  reco_tile_scores<D>(corpus, row >> 4, qfrag, lane, acc0, acc1);
  const float lo = reco_bound<STRAT, false>(acc0, acc1, q, lane);
  const float hi = reco_bound<STRAT, true>(acc0, acc1, q, lane);
  // the lane that holds this row: group (row & 15) >> 2, r = row & 3
  if (lane == (int)(((row & 15) >> 2) * 16 + (row & 3))) {
    out_lo[i] = lo;
    out_hi[i] = hi;
  }
}

}  // namespace ragmi
