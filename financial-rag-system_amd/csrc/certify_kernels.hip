// certify_kernels.hip — the exactness certificate of a search pass (included by index_search.hip
// after scan_kernels.hip and seed_kernels.hip): the canonical exact score (exact_scores_*),
// select_kernel (the scan's per-wave lists -> the exact top-k, or a verdict that the lists do
// not prove it), band_kernel (tier 1 of the 6-bit route, spread over every CU) and rescan_kernel
// (tier 2: the shard streamed once more for the queries select could not certify), with the
// bookkeeping they share (ExactStats, mark_unanswered_kernel).
namespace ragmi {

constexpr int kCandCap = 256;   // select: compacted heads at/above the lane-max threshold
constexpr int kBandLists = 32;  // select tier 1: lists gathered per chunk (8 per wave)
// ... after the 6-bit prescan (select_kernel<D, FILTER, kBandLists6>): its band is ~200 rows in
// as many lists per query, seven chunks of 32; 128 per chunk make that two gather round trips
// (the build with kBandSlices = 0 of index_search.hip; production spreads tier 1, next)
constexpr int kBandLists6 = 128;
// ... spread over the chip (select_kernel<D, FILTER, kBandHead> then band_kernel, below): the
// head instantiation gathers nothing; on verdict 1 it leaves a record per query in the workspace
//   rec[q][0] n_q: the qualifying lists (-1: not tier 1, band_kernel's workgroups return)
//   rec[q][1], [2] L and e_k (float bits)   [32..63], [64..95] A's exact scores and rows, sorted
//   rec[q][kBandRecHdr ...] the ids of the n_q lists
// pub[q][slice] is a slice's 32 best band rows (scores, rows) and its full-list flag at [64];
// tk[q] the query's arrival ticket (zero between passes)
constexpr int kBandHead = 0;
constexpr int kBandSlicesMax = 16;
constexpr int kBandRecHdr = 96;
constexpr int kBandRec = kBandRecHdr + kMaxLists;
constexpr int kBandPub = 72;
struct BandWs {
  int* rec;
  int* pub;
  int* tk;
};

// Wave 0 merges the four waves' top-32 lists (best first, one row of ws / wi per wave) out of
// LDS: lanes 0..31 end with the best 32 of the 128 entries, best first. `none` pads list 0 in
// lanes 32..63 before the first merge. (thresh_kernel and select's step 1a run the same loop
// on scores alone with synthetic ids; they keep their own text.)
template <typename IdT>
__device__ __forceinline__ void merge4_top32(const float (&ws)[4][32], const IdT (&wi)[4][32],
                                             int lane, IdT none, float& s, IdT& id) {
  s = lane < 32 ? ws[0][lane] : kNegInf;
  id = lane < 32 ? wi[0][lane] : none;
  for (int v = 1; v < 4; ++v) {
    if (lane >= 32) {
      s = ws[v][63 - lane];
      id = wi[v][63 - lane];
    }
    bitonic_merge64(s, id, lane);
  }
}

// ----------------------------------------------------------------------------------------
// canonical exact score of one stored row against a normalised fp32 query, by one wave:
// lane l accumulates the 8-element chunks c = l, l+64, ... with fp64 fma in order, then a
// xor butterfly (32..1) in fp64; lane 0's sum rounded to fp32. oracle/scan_ref.c
// (orc_exact_score) restates this order bit for bit.
// NC (row, query) pairs at once: every row chunk is loaded before any arithmetic, so the
// wave pays one memory round trip instead of NC dependent ones. rows[i] < 0 => out[i] = -inf.
// Query i is qn + qoff[i] (wave-uniform offsets).
// ----------------------------------------------------------------------------------------
template <int D, int NC>
__device__ __forceinline__ void exact_scores_pairs(const half8* __restrict__ corpus,
                                                   const int (&rows)[NC],
                                                   const int (&qoff)[NC],
                                                   const float* __restrict__ qn, int lane,
                                                   float (&out)[NC],
                                                   const float* __restrict__ rows32) {
  constexpr int S = steps<D>();
  double acc[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) acc[i] = 0.0;
  for (int c = lane; c < D / 8; c += 64) {
    // stored row elements as fp32: fp16 storage widens the tile16 halves (exact), fp32
    // storage reads the fp32 row (rows32 != nullptr, wave-uniform)
    float h[NC][8];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int row = rows[i] < 0 ? 0 : rows[i];
      if (rows32) {
        const float4* p = reinterpret_cast<const float4*>(rows32 + (int64_t)row * D + 8 * c);
        const float4 u = p[0], v = p[1];
        h[i][0] = u.x; h[i][1] = u.y; h[i][2] = u.z; h[i][3] = u.w;
        h[i][4] = v.x; h[i][5] = v.y; h[i][6] = v.z; h[i][7] = v.w;
      } else {
        const half8 x =
            corpus[(int64_t)(row >> 4) * (S * 64) + (c >> 2) * 64 + (c & 3) * 16 + (row & 15)];
#pragma unroll
        for (int j = 0; j < 8; ++j) h[i][j] = (float)x[j];
      }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const float* qq = qn + qoff[i];
      const float4 qa = *reinterpret_cast<const float4*>(qq + 8 * c);
      const float4 qb = *reinterpret_cast<const float4*>(qq + 8 * c + 4);
      double x = acc[i];
      x = fma((double)h[i][0], (double)qa.x, x);
      x = fma((double)h[i][1], (double)qa.y, x);
      x = fma((double)h[i][2], (double)qa.z, x);
      x = fma((double)h[i][3], (double)qa.w, x);
      x = fma((double)h[i][4], (double)qb.x, x);
      x = fma((double)h[i][5], (double)qb.y, x);
      x = fma((double)h[i][6], (double)qb.z, x);
      x = fma((double)h[i][7], (double)qb.w, x);
      acc[i] = x;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = acc[i] + __shfl_xor(acc[i], d, 64);
  }
#pragma unroll
  for (int i = 0; i < NC; ++i)
    out[i] = rows[i] < 0 ? kNegInf : (float)__shfl(acc[i], 0, 64);
}

// the same, every pair against one query
template <int D, int NC>
__device__ __forceinline__ void exact_scores_wave(const half8* __restrict__ corpus,
                                                  const int (&rows)[NC],
                                                  const float* __restrict__ qq, int lane,
                                                  float (&out)[NC],
                                                  const float* __restrict__ rows32) {
  int qoff[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) qoff[i] = 0;
  exact_scores_pairs<D, NC>(corpus, rows, qoff, qq, lane, out, rows32);
}

// ----------------------------------------------------------------------------------------
// Exactness bookkeeping of a search pass (rag_index_exactness_stats):
//   tier[q]  the path that certified query q's result: 0 check, 1 tier 1, 2 tier 2
//   cnt[2]   running totals of tier-1 / tier-2 queries
// ----------------------------------------------------------------------------------------
struct ExactStats {
  int* tier;
  unsigned long long* cnt;
  float* t2;        // [B][2] tier-2 hand-off: (L, e_k) of each tier-2 query (rescan_kernel)
};

// Query bq's result row: lanes < k of one wave hold (s, id) sorted best-first
__device__ __forceinline__ void emit_topk(float s, int id, int lane, int bq, int k,
                                          int64_t id_offset, float* __restrict__ out_s,
                                          int64_t* __restrict__ out_i,
                                          int32_t* __restrict__ out_packed) {
  if (lane < k) {
    const bool ok = s != kNegInf;
    if (out_packed) {
      // multi-GPU exchange format: [B][k][2] int32 = (score bits, global row; -1 = none)
      out_packed[((int64_t)bq * k + lane) * 2] = __float_as_int(s);
      out_packed[((int64_t)bq * k + lane) * 2 + 1] = ok ? (int32_t)(id + id_offset) : -1;
    } else {
      out_s[(int64_t)bq * k + lane] = s;
      out_i[(int64_t)bq * k + lane] = ok ? (int64_t)id + id_offset : (int64_t)-1;
    }
  }
}

// Tier 2 (one thread): query bq is handed to rescan_kernel (launched after every select, many
// workgroups). Its floor L and the k-th exact score of A go to the hand-off record; nothing is
// emitted by the caller (the rescan writes this query's output)
__device__ __forceinline__ void hand_to_tier2(const ExactStats& fb, int bq, float L, float e_k,
                                              const float* __restrict__ eps_t2) {
  fb.tier[bq] = 2;
  // the rescan bands on fp16 MFMA scores: after an int8 prescan (eps_t2 = qprep's fp16
  // bound; `eps` is then the prescan's) its floor is e_k - the fp16 bound, not this L
  fb.t2[2 * bq] = eps_t2 ? e_k - eps_t2[bq] : L;
  fb.t2[2 * bq + 1] = e_k;
  atomicAdd(&fb.cnt[1], 1ull);
}

// One chunk of tier 1 (select_kernel step 5, band_kernel), by a 256-thread workgroup: the lists
// qlist[c0 .. c0 + BL) of the query's nql qualifying ones (slot b of the group part_s / part_i /
// heads_n point at) are gathered, their entries >= L outside A (a_row: A's rows, one per lane
// and half-wave) go to the LDS band buffer and are rescored, and wave 0 folds them into its
// running exact top-32 (rs, ri in lanes 0..31, by (score desc, row asc)). false: a full list
// holds an entry >= L (verdict = 2, nothing rescored). `more`: another chunk follows (the band
// buffer is reset for it). n_band is zero on entry; rnd counts the rounds across chunks.
template <int D, int BL, typename ListP>
__device__ __forceinline__ bool band_chunk(ListP qlist, int c0, int nql, bool more,
                                           const float* __restrict__ part_s,
                                           const int* __restrict__ part_i,
                                           const int* __restrict__ heads_n, int n_lists, int b,
                                           float L, int a_row, const half8* __restrict__ corpus,
                                           const float* __restrict__ qq,
                                           const float* __restrict__ rows32,
                                           int (&band)[BL * kKS], int& n_band,
                                           float (&n_s)[2][32], int (&n_i)[2][32], int& verdict,
                                           float& rs, int& ri, int& rnd) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  auto at = [&](int l, int pos) { return ((int64_t)l * kQ + b) * kKS + pos; };
  // gather: a half-wave per list, a lane per entry; wave w takes the chunk's lists w, w + 4,
  // ... Every load is issued before the first use (clamped, selects afterwards: step 1).
  constexpr int kG = BL / 8;
  const int pos = lane & (kKS - 1);
  float gs[kG];
  int gi[kG], gn[kG];
#pragma unroll
  for (int j = 0; j < kG; ++j) {
    const int l = qlist[min(c0 + (2 * j + (lane >> 5)) * 4 + wid, nql - 1)];
    gs[j] = part_s[at(l, pos)];
    gi[j] = part_i[at(l, pos)];
    gn[j] = heads_n[(int64_t)b * n_lists + l];
  }
#pragma unroll
  for (int j = 0; j < kG; ++j) {
    // entries past a list's length are stale memory
    const bool in = c0 + (2 * j + (lane >> 5)) * 4 + wid < nql && pos < gn[j] && gs[j] >= L;
    // lane 31 of the half-wave holds the tail: a full list may have dropped a row >= L
    if (in && gn[j] >= kKS && pos == kKS - 1) verdict = 2;
    bool in_a = false;
#pragma unroll
    for (int t = 0; t < 32; ++t) in_a |= gi[j] == __builtin_amdgcn_readlane(a_row, t);
    if (in && !in_a) band[atomicAdd(&n_band, 1)] = gi[j];
  }
  __syncthreads();
  if (verdict == 2) return false;
  // rescoring: the band rows 32 per round, 8 per wave; wave 0 folds each round into the
  // running exact top-32
  const int nb = n_band;
  for (int r0 = 0; r0 < nb; r0 += 32, ++rnd) {
    int rows[8];
    float es[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = r0 + wid * 8 + j;
      const int r = band[min(c, nb - 1)];
      rows[j] = c < nb ? r : -1;
    }
    exact_scores_wave<D, 8>(corpus, rows, qq, lane, es, rows32);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        n_s[rnd & 1][wid * 8 + j] = es[j];
        n_i[rnd & 1][wid * 8 + j] = rows[j] >= 0 ? rows[j] : kIdNone32;
      }
    }
    // one barrier per round: round r + 2 overwrites this slot only after round r + 1's
    // barrier, which wave 0 reaches after the read below
    __syncthreads();
    if (wid == 0) {
      if (lane >= 32) {
        rs = n_s[rnd & 1][lane - 32];
        ri = n_i[rnd & 1][lane - 32];
      }
      bitonic_sort64(rs, ri, lane);
    }
  }
  if (more) {   // the band buffer is reused by the next chunk
    __syncthreads();
    if (tid == 0) n_band = 0;
    __syncthreads();
  }
  return true;
}

// ----------------------------------------------------------------------------------------
// select: one 256-thread workgroup per query merges the n_lists sorted per-wave top-32
// lists (approximate MFMA scores) into the exact top-k.
//  1. top-32 of the list HEADS. Any entry of a list whose head is not among the 32 best
//     heads is beaten by those 32 heads, so the global top-32 lies inside the 32 selected
//     lists. (Threshold from lane maxima -> compaction -> small sort; exact column-sort
//     fallback when ties push more than kCandCap heads past the threshold.)
//  2. each wave merges 8 of the selected lists (prefetched) -> wave 0 merges the 4 results:
//     A = the approximate top-32, a_32 its last score.
//  3. exact rescoring of the 32 candidates (exact_score_wave), 8 per wave.
//  4. sort by (exact score desc, row asc); e_k = the k-th exact score.
//  5. exactness check. Every row r outside A has a(r) <= a_32, so e(r) <= a_32 + eps_q
//     (qprep's bound). If e_k > a_32 + eps_q (or A holds every matching row), the k best of
//     A are the exact top-k: emit. Otherwise every true top-k row has e >= e_k, hence
//     a >= L = e_k - eps_q, and:
//     tier 1 (here): if L >= the scan's seed (no such row was pruned) and no per-wave list
//       whose tail is >= L is full (none dropped one), every row with a >= L sits in some
//       list. The lists whose head is >= L come from the head scores step 1 still holds in
//       registers; their entries are gathered a half-wave per list, every load of a chunk of
//       kBandLists lists issued before the first use (the list's tail rides on lane 31 of the
//       same load: the fullness check). Entries >= L that are not in A go to an LDS band
//       buffer and are rescored 32 per round (8 per wave); the result is the top-k of A's 32
//       exact scores and theirs. One gather round trip, one rescoring round trip per 32 new
//       rows and one merge per round, whatever the number of lists below kBandLists; more
//       lists cost a chunk each, with a running top-32 across chunks (band_chunk).
//       After the 6-bit prescan every query takes tier 1 with ~200 qualifying lists: there the
//       head instantiation (BL = kBandHead) stops at the verdict, writes L, e_k, A by exact
//       score and the qualifying lists to the workspace, and band_kernel, launched next with S
//       workgroups per query, runs the same chunks spread over the chip and emits (below).
//     tier 2 (rescan_kernel): otherwise the shard is streamed once more for this query by
//       the rescan kernel launched after every select (its workgroups split the shard); here
//       select only records L and e_k. Only inputs with more than 32 in-band rows inside one
//       wave's share of the tiles (or a seed above L) get there. After an int8 prescan
//       (scan_kernel_i8, scan_kernel_i6) the list scores are upper bounds u >= e: a row outside A has
//       e <= u <= a_32, the same check with a := u and eps the prescan's slack; a true top-k
//       row has u >= e >= e_k >= L, so tier 1 reads the same lists. (Round 2 ran this pass
//       inside select, on the query's one workgroup: a single-CU pass over the whole shard,
//       ~0.1 s at 10M rows — unbounded by the chip's bandwidth; VERDICT/ADVICE r2.)
// ----------------------------------------------------------------------------------------
template <int D, bool FILTER, int BL = kBandLists>
__global__ __launch_bounds__(256) void select_kernel(const float* __restrict__ part_s,
                                                     const int* __restrict__ part_i,
                                                     const float* __restrict__ heads_s,
                                                     const int* __restrict__ heads_i,
                                                     const int* __restrict__ heads_n,
                                                     int n_lists,
                                                     const half8* __restrict__ corpus,
                                                     const uint32_t* __restrict__ tags,
                                                     const uint32_t* __restrict__ filt,
                                                     const half8* __restrict__ qfrag,
                                                     int n_rows,
                                                     const float* __restrict__ qn, int k,
                                                     const float* __restrict__ eps,
                                                     const float* __restrict__ seed_thr,
                                                     ExactStats fb, int64_t id_offset,
                                                     float* __restrict__ out_s,
                                                     int64_t* __restrict__ out_i,
                                                     int32_t* __restrict__ out_packed,
                                                     const float* __restrict__ rows32,
                                                     const float* __restrict__ eps_t2 = nullptr,
                                                     BandWs bw = {}) {
  constexpr bool kHead = BL == kBandHead;            // (its gather below is dead code)
  constexpr int kChunk = kHead ? kBandLists : BL;
  __shared__ float w_s[4][32];
  __shared__ int64_t w_i[4][32];
  __shared__ int sel[32];
  __shared__ int sel_n[32];
  __shared__ float cand_s[kCandCap];
  __shared__ int64_t cand_i[kCandCap];
  __shared__ int n_cand;
  __shared__ float head_t;
  __shared__ float c_s[4][32];
  __shared__ int c_i[4][32];
  __shared__ float e_s[32];
  __shared__ int e_i[32];
  __shared__ int qlist[kMaxLists];   // tier 1: lists whose head is >= L
  __shared__ int n_q;
  __shared__ int band[kChunk * kKS];   // tier 1: a chunk's rows with a >= L outside A
  __shared__ int n_band;
  __shared__ float n_s[2][32];       // tier 1: a round's exact scores / rows (two rounds in
  __shared__ int n_i[2][32];         // flight: one barrier per round)
  __shared__ int verdict;            // 0 exact, 1 tier 1, 2 tier 2
  __shared__ float floor_L, floor_E;
  // query bq of the batch = slot b of query group grp (the scan's per-group lists)
  const int bq = blockIdx.x, grp = bq / kQ, b = bq % kQ;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // the check's two constants, read here: their round trip is over long before step 5
  const float eps_q = eps[bq], seed_q = seed_thr[bq];
  part_s += (int64_t)grp * n_lists * (kQ * kKS);
  part_i += (int64_t)grp * n_lists * (kQ * kKS);
  heads_s += (int64_t)grp * kQ * n_lists;
  heads_i += (int64_t)grp * kQ * n_lists;
  heads_n += (int64_t)grp * kQ * n_lists;
  auto at = [&](int l, int pos) { return ((int64_t)l * kQ + b) * kKS + pos; };

  // ---- 1. the 32 best list heads (a list = one scan wave). Heads are ranked by (score desc,
  //      row asc) with the list index carried in the low bits of a 64-bit id (row << 11 |
  //      list): select needs no knowledge of which tiles a wave scanned (static interleave,
  //      dynamic tile queue or the rescan's own order).
  constexpr int kCols = kMaxLists / 256;
  static_assert(kMaxLists <= 2048, "list index packs into 11 bits");
  auto hid = [](int row, int l) { return ((int64_t)row << 11) | (int64_t)l; };
  constexpr int64_t kId64None = INT64_MAX;
  float hs[kCols];
  int64_t hr[kCols];
  // unconditional (clamped) loads, selects afterwards: a load under a data-dependent branch
  // makes hipcc wait vmcnt(0) per element (one round trip each)
#pragma unroll
  for (int j = 0; j < kCols; ++j) {
    const int l = min((j * 4 + wid) * 64 + lane, n_lists - 1);
    hs[j] = heads_s[(int64_t)b * n_lists + l];
    hr[j] = hid(heads_i[(int64_t)b * n_lists + l], l);
  }
  float lmax = kNegInf;
#pragma unroll
  for (int j = 0; j < kCols; ++j) {
    const int l = (j * 4 + wid) * 64 + lane;
    const bool ok = l < n_lists && hs[j] != kNegInf;
    hs[j] = ok ? hs[j] : kNegInf;
    hr[j] = ok ? hr[j] : kId64None;
    lmax = fmaxf(lmax, hs[j]);
  }
  // 1a. T = 32nd largest lane maximum (the maxima of 32 distinct lanes are 32 distinct heads,
  //     so at least 32 heads score >= T and every top-32 head scores >= T)
  {
    float m = lmax;
    int id = tid;
    bitonic_sort64(m, id, lane);
    if (lane < 32) w_s[wid][lane] = m;
  }
  if (tid == 0) {
    n_cand = 0;
    n_q = 0;
    n_band = 0;
    verdict = 0;
  }
  __syncthreads();
  if (wid == 0) {
    float m = lane < 32 ? w_s[0][lane] : kNegInf;
    int id = lane;
    for (int v = 1; v < 4; ++v) {
      if (lane >= 32) {
        m = w_s[v][63 - lane];
        id = 64 * v + lane;
      }
      bitonic_merge64(m, id, lane);
    }
    const float t32 = __shfl(m, 31, 64);
    if (lane == 0) head_t = t32;
  }
  __syncthreads();
  // 1b. compact the heads scoring >= T (typically ~35) into LDS
  {
    const float T = head_t;
#pragma unroll
    for (int j = 0; j < kCols; ++j) {
      if (hs[j] != kNegInf && hs[j] >= T) {
        const int p = atomicAdd(&n_cand, 1);
        if (p < kCandCap) {
          cand_s[p] = hs[j];
          cand_i[p] = hr[j];
        }
      }
    }
  }
  __syncthreads();
  const int nc = n_cand;
  if (nc <= kCandCap) {
    // 1c. top-32 of the compacted heads: each wave sorts 64 of them, wave 0 merges
    float m = kNegInf;
    int64_t id = kId64None;
    if (64 * wid + lane < nc) {
      m = cand_s[64 * wid + lane];
      id = cand_i[64 * wid + lane];
    }
    if (64 * wid < nc) bitonic_sort64(m, id, lane);
    if (lane < 32) {
      w_s[wid][lane] = m;
      w_i[wid][lane] = id;
    }
  } else {
    // 1c'. adversarial ties (more than kCandCap heads at the threshold): exact column sort
    float cs = kNegInf;
    int64_t ci = kId64None;
#pragma unroll
    for (int j = 0; j < kCols; ++j) {
      if (!__ballot(hs[j] != kNegInf)) continue;   // wave-uniform: empty column
      float x = hs[j];
      int64_t id = hr[j];
      bitonic_sort64(x, id, lane);
      const float rx = __shfl(x, 63 - lane, 64);
      const int64_t ri = (int64_t)(((uint64_t)(uint32_t)__shfl((int)(id >> 32), 63 - lane, 64) << 32) |
                                   (uint32_t)__shfl((int)id, 63 - lane, 64));
      if (lane >= 32) {
        cs = rx;
        ci = ri;
      }
      bitonic_merge64(cs, ci, lane);
      if (lane >= 32) {
        cs = kNegInf;
        ci = kId64None;
      }
    }
    if (lane < 32) {
      w_s[wid][lane] = cs;
      w_i[wid][lane] = ci;
    }
  }
  __syncthreads();
  if (wid == 0) {
    float x;
    int64_t id;
    merge4_top32(w_s, w_i, lane, kId64None, x, id);
    if (lane < 32) {
      const int l = (x != kNegInf) ? (int)(id & 2047) : -1;
      sel[lane] = l;
      sel_n[lane] = l >= 0 ? heads_n[(int64_t)b * n_lists + l] : 0;
    }
  }
  __syncthreads();

  // ---- 2. merge the selected lists: wave w takes lists sel[8w .. 8w+7]
  {
    float ls[8];
    int li[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int l = sel[wid * 8 + j];
      const int pos = (j == 0 ? lane : 63 - lane) & (kKS - 1);  // lanes 32..63: reversed
      const int64_t off = at(l < 0 ? 0 : l, pos);
      ls[j] = part_s[off];
      li[j] = part_i[off];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // entries past a list's length were not written this search (stale memory)
      const int pos = (j == 0 ? lane : 63 - lane) & (kKS - 1);
      const bool use = sel[wid * 8 + j] >= 0 && ((j == 0) ? lane < 32 : lane >= 32) &&
                       pos < sel_n[wid * 8 + j];
      ls[j] = use ? ls[j] : kNegInf;
      li[j] = use ? li[j] : kIdNone32;
    }
    float s = ls[0];
    int id = li[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) {
      if (lane >= 32) {
        s = ls[j];
        id = li[j];
      }
      bitonic_merge64(s, id, lane);
    }
    if (lane < 32) {
      c_s[wid][lane] = s;
      c_i[wid][lane] = id;
    }
  }
  __syncthreads();
  if (wid == 0) {
    float s;
    int id;
    merge4_top32(c_s, c_i, lane, kIdNone32, s, id);
    if (lane < 32) {
      c_s[0][lane] = s;
      c_i[0][lane] = id;
    }
  }
  __syncthreads();

  const float* qq = qn + (int64_t)bq * D;
  // ---- 3. exact rescoring, 8 candidates per wave (one round trip)
  {
    int rows[8];
    float es[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = wid * 8 + j;
      rows[j] = c_s[0][c] != kNegInf ? c_i[0][c] : -1;
    }
    exact_scores_wave<D, 8>(corpus, rows, qq, lane, es, rows32);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        e_s[wid * 8 + j] = es[j];
        e_i[wid * 8 + j] = rows[j] >= 0 ? rows[j] : kIdNone32;
      }
    }
  }
  __syncthreads();

  auto emit = [&](float s, int id) {   // wave 0, lanes < k: (s, id) sorted best-first
    emit_topk(s, id, lane, bq, k, id_offset, out_s, out_i, out_packed);
  };

  // ---- 4. order by exact score; 5. exactness check
  float rs = kNegInf;   // wave 0, lanes 0..31: A by exact score, best first; under tier 1 the
  int ri = kIdNone32;   // running exact top-32
  if (wid == 0) {
    if (lane < 32) {
      rs = e_s[lane];
      ri = e_i[lane];
    }
    bitonic_sort64(rs, ri, lane);
    int v = 0;
    {
      const float ek = __shfl(rs, k - 1, 64);
      const float a32 = c_s[0][kKS - 1];
      float L = 0.0f;
      // a32 == -inf: fewer than 32 finite candidates, i.e. A holds every matching row (a
      // finite seed implies >= 32 rows above it)
      if (!(a32 == kNegInf || ek > a32 + eps_q)) {
        L = ek - eps_q;
        v = (L >= seed_q) ? 1 : 2;
      }
      if (lane == 0) {
        verdict = v;
        floor_L = L;
        floor_E = ek;
      }
    }
    if (v == 0) {
      emit(rs, ri);
      if (lane == 0) fb.tier[bq] = 0;
    }
    if constexpr (kHead) {
      // ---- head: the record band_kernel reads (launched next on the stream): A by exact score
      int* rq = bw.rec + (int64_t)bq * kBandRec;
      if (lane < 32 && v == 1) {
        rq[32 + lane] = __float_as_int(rs);
        rq[64 + lane] = ri;
      }
      if (lane == 0 && v != 1) rq[0] = -1;
    }
  }
  __syncthreads();
  if (verdict == 0) return;
  if constexpr (kHead) {
    // tier 1 is band_kernel's: the qualifying lists (as below) go to the record, n_q last; tier 2
    // by the seed is handed over here
    int* rq = bw.rec + (int64_t)bq * kBandRec;
    if (verdict == 1) {
#pragma unroll
      for (int j = 0; j < kCols; ++j)
        if (hs[j] != kNegInf && hs[j] >= floor_L)
          rq[kBandRecHdr + atomicAdd(&n_q, 1)] = (j * 4 + wid) * 64 + lane;
      __syncthreads();
    }
    if (tid == 0) {
      if (verdict == 1) {
        rq[0] = n_q;
        rq[1] = __float_as_int(floor_L);
        rq[2] = __float_as_int(floor_E);
      } else {
        hand_to_tier2(fb, bq, floor_L, floor_E, eps_t2);
      }
    }
    return;
  }

  // ---- tier 1: every row with approximate score >= L is in a list (checked by the gather).
  //      The qualifying lists, from step 1's head scores (list of hs[j] = (4j + wid) 64 + lane)
  const float L = floor_L;
  const bool seeded = verdict == 1;   // read before the gather may write it
  if (seeded) {
#pragma unroll
    for (int j = 0; j < kCols; ++j)
      if (hs[j] != kNegInf && hs[j] >= L) qlist[atomicAdd(&n_q, 1)] = (j * 4 + wid) * 64 + lane;
  }
  __syncthreads();
  const int nql = seeded ? n_q : 0;
  const int a_row = e_i[lane & 31];   // A's rows, one per lane: their exact scores are known
  int rnd = 0;
  for (int c0 = 0; c0 < nql; c0 += kChunk)
    if (!band_chunk<D, kChunk>(qlist, c0, nql, c0 + kChunk < nql, part_s, part_i, heads_n, n_lists,
                               b, L, a_row, corpus, qq, rows32, band, n_band, n_s, n_i, verdict,
                               rs, ri, rnd))
      break;
  if (verdict == 2) {
    if (tid == 0) hand_to_tier2(fb, bq, L, floor_E, eps_t2);
    return;
  }
  // tier 1 certified: the top-k of A and the band rows, by (exact score desc, row asc)
  if (tid == 0) {
    fb.tier[bq] = 1;
    atomicAdd(&fb.cnt[0], 1ull);
  }
  if (wid == 0) emit(rs, ri);
}

// ----------------------------------------------------------------------------------------
// band: tier 1 of the queries select_kernel<D, FILTER, kBandHead> left a record for, spread over
// the chip (the 6-bit prescan: every query takes tier 1 with ~200 qualifying lists, and one
// workgroup per query kept 32 CUs busy for ~0.3 ms beside the other batch's scan). Grid (S, Bq):
// workgroup (s, bq) takes the chunks s, s + S, ... of kBandLists qualifying lists of query bq
// (band_chunk, select's own gather and rescoring) and keeps the 32 best of ITS band rows; a full
// list with an entry >= L ends its work. It publishes the 32 pairs and the full-list flag to
// pub[bq][s] and arrives at the query's ticket (rescan_kernel's publish sequence, below); slices
// with no chunk arrive too. The last arriver of bq either hands the query to tier 2 (a slice saw a
// full list) or merges A with the S slice lists and emits the top-k by (exact score desc, row
// asc) - the top-k of A and all band rows, whichever slice held them - then re-arms the ticket
// for the workspace's next pass (stream order). Every slice rewrites its flag in every pass.
// ----------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void band_kernel(const float* __restrict__ part_s,
                                                   const int* __restrict__ part_i,
                                                   const int* __restrict__ heads_n, int n_lists,
                                                   const half8* __restrict__ corpus,
                                                   const float* __restrict__ qn, int k,
                                                   BandWs bw, ExactStats fb,
                                                   const float* __restrict__ eps_t2,
                                                   int64_t id_offset, float* __restrict__ out_s,
                                                   int64_t* __restrict__ out_i,
                                                   int32_t* __restrict__ out_packed,
                                                   const float* __restrict__ rows32) {
  __shared__ int band[kBandLists * kKS];
  __shared__ int n_band;
  __shared__ float n_s[2][32];
  __shared__ int n_i[2][32];
  __shared__ int verdict;   // 2: a full list of this slice holds an entry >= L
  __shared__ int last;
  const int S = gridDim.x, s = blockIdx.x, bq = blockIdx.y, grp = bq / kQ, b = bq % kQ;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // plain loads of the head's record: a kernel boundary lies between its stores and these
  const int* rq = bw.rec + (int64_t)bq * kBandRec;
  const int nql = rq[0];
  if (nql < 0) return;   // not a tier-1 query (block-uniform)
  const float L = __int_as_float(rq[1]), floor_E = __int_as_float(rq[2]);
  const int a_row = rq[64 + (lane & 31)];
  part_s += (int64_t)grp * n_lists * (kQ * kKS);
  part_i += (int64_t)grp * n_lists * (kQ * kKS);
  heads_n += (int64_t)grp * kQ * n_lists;
  const float* qq = qn + (int64_t)bq * D;
  if (tid == 0) {
    n_band = 0;
    verdict = 1;
  }
  __syncthreads();
  float rs = kNegInf;   // wave 0, lanes 0..31: the slice's running exact top-32
  int ri = kIdNone32;
  int rnd = 0;
  constexpr int BL = kBandLists;
  for (int c0 = s * BL; c0 < nql; c0 += S * BL)
    if (!band_chunk<D, BL>(rq + kBandRecHdr, c0, nql, c0 + S * BL < nql, part_s, part_i, heads_n,
                           n_lists, b, L, a_row, corpus, qq, rows32, band, n_band, n_s, n_i,
                           verdict, rs, ri, rnd))
      break;
  int* pub = bw.pub + ((int64_t)bq * kBandSlicesMax + s) * kBandPub;
  if (wid == 0 && lane < 32) {
    pub[lane] = __float_as_int(rs);
    pub[32 + lane] = ri;
  }
  if (tid == 0) pub[64] = verdict == 2;
  // ---- publish: stores drained, agent release, then the ticket (rescan_kernel)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = atomicAdd(&bw.tk[bq], 1) == S - 1;
  }
  __syncthreads();
  if (!last) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  // ---- last arriver of bq (wave 0): the S flags, then A and the S lists -> the exact top-k.
  //      The lists are loaded 8 ahead of their merges, and one whose best entry scores below
  //      the running 32nd is skipped (rescan_kernel's tail)
  if (wid != 0) return;
  const int* pq = bw.pub + (int64_t)bq * kBandSlicesMax * kBandPub;
  const bool full = __ballot(lane < S && pq[(lane < S ? lane : 0) * kBandPub + 64] != 0) != 0;
  if (full) {
    if (lane == 0) hand_to_tier2(fb, bq, L, floor_E, eps_t2);
  } else {
    float x = lane < 32 ? __int_as_float(rq[32 + lane]) : kNegInf;
    int id = lane < 32 ? rq[64 + lane] : kIdNone32;
    constexpr int kPf = 8;
    for (int u0 = 0; u0 < S; u0 += kPf) {
      float xs[kPf];
      int is[kPf];
#pragma unroll
      for (int u = 0; u < kPf; ++u) {
        const int* p = pq + min(u0 + u, S - 1) * kBandPub + (lane >= 32 ? 63 - lane : 0);
        const bool use = u0 + u < S && lane >= 32;
        xs[u] = use ? __int_as_float(p[0]) : kNegInf;
        is[u] = use ? p[32] : kIdNone32;
      }
#pragma unroll
      for (int u = 0; u < kPf; ++u) {
        const float head = __shfl(xs[u], 63, 64), t32 = __shfl(x, 31, 64);
        if (head < t32 || head == kNegInf) continue;   // wave-uniform
        if (lane >= 32) {
          x = xs[u];
          id = is[u];
        }
        bitonic_merge64(x, id, lane);
      }
    }
    emit_topk(x, id, lane, bq, k, id_offset, out_s, out_i, out_packed);
    if (lane == 0) {
      fb.tier[bq] = 1;
      atomicAdd(&fb.cnt[0], 1ull);
    }
  }
  if (lane == 0) bw.tk[bq] = 0;   // re-armed for the workspace's next pass (stream order)
}

// ----------------------------------------------------------------------------------------
// rescan (tier 2 of select's certificate; round 4): launched after every select with R
// workgroups. Each returns at once (two loads and a ballot per wave) unless select marked a
// query of the pass. Otherwise the workgroups split the shard's tiles (t = 4r + w, step 4R:
// rows increase per wave, as the strict `> thr` tie rule needs) and serve ALL marked queries
// in one stream of the shard per 16 of them (kRescanQ = one MFMA column tile; D = 384 passes
// hold <= 32 queries, so at most two streams):
//   * the marked queries' B-fragments are gathered from qprep's into LDS (column j = the j-th
//     marked query), and every tile gets the scan's MFMA scores a(r) against all of them;
//   * query j's rows with a >= band_j = max(L_j, thr_j - eps_j) may be in its top-k (L from
//     select: every true top-k row has a >= L; thr_j = the wave's running 32nd exact score,
//     starting just below e_k, the k-th exact score select saw); a tile with such a row for
//     query j is re-scored exactly for j, all 16 rows at once (exact_tile_scores: the tile
//     image re-read from L2, the canonical fp64 order), and its rows with e > thr_j merge into
//     the wave's running exact top-32 of j (LDS; thr_j rises with it);
//   * each workgroup merges its 4 waves' lists per query and publishes them; the workgroup that
//     arrives last at the pass ticket (one per launch) merges the R lists of every marked query
//     and emits its exact top-k. The global top-k lies in the union of the per-wave top-32s.
// Round 3 streamed the shard once per marked query with v_dot2 and re-scored candidates two
// rows per memory round trip: 4 marked queries cost 8.4 ms at 1.25M rows and 10.7 ms at 10M
// (profiles/r03zz_tier2_latency.jsonl), and its 64-register budget spilled to scratch.
// Visibility (MI355X_MICROARCH.md, inter-workgroup hand-off): list stores, every wave's
// vmcnt(0), barrier, one lane's agent release fence + vmcnt(0), the ticket add; the last
// arriver's one agent acquire + vmcnt(0), barrier, then plain loads.
// ----------------------------------------------------------------------------------------
constexpr int kRescanMaxWG = 512;
constexpr int kRescanQ = 16;   // marked queries per stream of the shard (one MFMA column tile)

// the canonical butterfly of exact_tile_scores on a lane's 16 partials: sg ^ 8, 4, 2, 1 in the
// lane, then lane ^ 32, lane ^ 16; fp32 rounding of the fp64 sum
__device__ __forceinline__ float exact_tree(double (&p)[16]) {
#pragma unroll
  for (int d = 8; d > 0; d >>= 1) {
#pragma unroll
    for (int i = 0; i < d; ++i) p[i] = p[i] + p[i + d];
  }
  double y = p[0] + __shfl_xor(p[0], 32, 64);
  y = y + __shfl_xor(y, 16, 64);
  return (float)y;
}

// Canonical exact scores (exact_scores_pairs' arithmetic bit for bit) of the 16
// rows of tile t against one normalised query qq, all rows at once. Lane (h, r) = (lane >> 4,
// lane & 15) reads row 16t + r's chunks c = 4s + h: the tile16 image itself (fp16 storage) or
// the fp32 rows. Canonical lane l = 4 sg + h of exact_scores_pairs sums the chunks l, l + 64,
// ..., i.e. s = sg, sg + 16, ... in that order, so this lane keeps those partials p[sg]. The
// canonical xor butterfly over l (d = 32 .. 1) is d = 32, 16, 8, 4 -> sg ^ 8, 4, 2, 1 inside the
// lane, then d = 2, 1 -> h ^ 2, h ^ 1 = lane ^ 32, lane ^ 16. IEEE addition commutes, so each
// pair sums to the canonical value whichever operand comes first. Every lane of row r returns
// row r's score.
template <int D, bool F32>
__device__ __forceinline__ float exact_tile_scores(const half8* __restrict__ corpus,
                                                   const float* __restrict__ rows32, int t,
                                                   const float* __restrict__ qq, int lane) {
  constexpr int S = steps<D>();
  const int h = lane >> 4, r = lane & 15;
  double p[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) p[i] = 0.0;
  // opaque zero offset of every load: the tile's loads do not depend on the query, and
  // without it the compiler hoisted them (and their fp32 conversions) out of the caller's
  // loop over queries
  int zoff = 0;
  asm volatile("" : "+v"(zoff));
  const half8* tp = corpus + (int64_t)t * (S * 64) + lane;
  const float* rp = F32 ? rows32 + ((int64_t)t * kTileRows + r) * D + 8 * h : nullptr;
  const float* qp = qq + 8 * h;
  // G k-steps per group; the next group's addresses depend (opaque asm) on this group's
  // last fp64 sum, so its loads issue after this group's registers are consumed: left free,
  // the compiler hoisted every step's tile and query loads (S x 12 registers) to the top and
  // spilled (sched_barrier did not stop it). One L2 round trip per group.
  constexpr int G = 2;
#pragma unroll
  for (int s0 = 0; s0 < S; s0 += G) {
    float x[G][8];
    float4 qa[G], qb[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int s = s0 + g;
      if constexpr (F32) {
        const float4 u = *reinterpret_cast<const float4*>(rp + 32 * s + zoff);
        const float4 v = *reinterpret_cast<const float4*>(rp + 32 * s + 4 + zoff);
        x[g][0] = u.x; x[g][1] = u.y; x[g][2] = u.z; x[g][3] = u.w;
        x[g][4] = v.x; x[g][5] = v.y; x[g][6] = v.z; x[g][7] = v.w;
      } else {
        const half8 v = tp[s * 64 + zoff];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[g][i] = (float)v[i];
      }
      qa[g] = *reinterpret_cast<const float4*>(qp + 32 * s + zoff);
      qb[g] = *reinterpret_cast<const float4*>(qp + 32 * s + 4 + zoff);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      double a = p[(s0 + g) & 15];
      a = fma((double)x[g][0], (double)qa[g].x, a);
      a = fma((double)x[g][1], (double)qa[g].y, a);
      a = fma((double)x[g][2], (double)qa[g].z, a);
      a = fma((double)x[g][3], (double)qa[g].w, a);
      a = fma((double)x[g][4], (double)qb[g].x, a);
      a = fma((double)x[g][5], (double)qb[g].y, a);
      a = fma((double)x[g][6], (double)qb[g].z, a);
      a = fma((double)x[g][7], (double)qb[g].w, a);
      p[(s0 + g) & 15] = a;
    }
    asm volatile("" : "+v"(zoff) : "v"(p[(s0 + G - 1) & 15]));
  }
  return exact_tree(p);
}

// exact_tile_scores for D <= 384 with the tile already in registers (the scan-order image a
// lane streamed: a[s] = row 16t + r, dims 32s + 8h .. +7 = chunk 4s + h) and the query as
// fp64 in LDS (qd = its D values): no memory round trip besides the LDS reads. Groups of G
// steps chained by the opaque asm dependency of exact_tile_scores (LDS reads hoisted above
// the fp64 FMAs spilled the same way).
template <int D>
__device__ __forceinline__ float exact_tile_scores_reg(const half8 (&a)[steps<D>()],
                                                       const double* qd, int lane) {
  constexpr int S = steps<D>();
  static_assert(S <= 16, "one chunk per canonical lane");
  const int h = lane >> 4;
  double p[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) p[i] = 0.0;
  int zoff = 0;
  asm volatile("" : "+v"(zoff));
  constexpr int G = 2;
#pragma unroll
  for (int s0 = 0; s0 < S; s0 += G) {
    double2 qv[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        qv[g][i] = *reinterpret_cast<const double2*>(qd + 32 * (s0 + g) + 8 * h + 2 * i + zoff);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      half8 v = a[s0 + g];
      asm volatile("" : "+v"(v));   // per call: no fp32 / fp64 copy of the tile hoisted
      double x = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x = fma((double)(float)v[2 * i], qv[g][i].x, x);
        x = fma((double)(float)v[2 * i + 1], qv[g][i].y, x);
      }
      p[s0 + g] = x;
    }
    asm volatile("" : "+v"(zoff) : "v"(p[s0 + G - 1]));
  }
  return exact_tree(p);
}

template <int D, bool FILTER>
__global__ __launch_bounds__(kScanBlock, 2) void rescan_kernel(
    const int* __restrict__ tier, const float* __restrict__ t2, int Bq,
    const half8* __restrict__ corpus, const uint32_t* __restrict__ tags,
    const uint32_t* __restrict__ filt, const half8* __restrict__ qfrag, int n_rows,
    const float* __restrict__ qn, int k, const float* __restrict__ eps,
    float* __restrict__ lst_s, int* __restrict__ lst_i, int* __restrict__ ticket,
    int64_t id_offset, float* __restrict__ out_s, int64_t* __restrict__ out_i,
    int32_t* __restrict__ out_packed, const float* __restrict__ rows32) {
  constexpr int S = steps<D>();
  // D <= 384: a whole tile per chunk (48 registers) in a two-slot ring, and fp16-storage exact
  // scores straight from those registers with the queries in LDS as fp64 (exact_tile_scores_reg);
  // D = 1024: chunks of 8 k-steps and the exact scores from an L2 re-read (exact_tile_scores)
  constexpr bool REG = S <= 12;
  constexpr int CS = REG ? S : 8;          // k-steps per streamed chunk
  constexpr int NCH = S / CS;              // chunks per tile: 1, or even (two-slot ring)
  static_assert(S % CS == 0 && (NCH == 1 || NCH % 2 == 0), "two-slot chunk ring");
  __shared__ half8 bl[S * 64];                         // B-fragments of the marked queries
  __shared__ float ws[kWavesPerWG][kRescanQ][kKS];     // per-wave running exact top-32s
  __shared__ int wi[kWavesPerWG][kRescanQ][kKS];
  __shared__ double qd[REG ? kRescanQ * D : 2];        // marked queries' qn as fp64 (REG)
  __shared__ int fq[128];                              // marked queries, ascending
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // ---- the pass's marked queries (Bq <= 128): none -> return, the common case
  const uint64_t todo0 = __ballot(lane < Bq && tier[lane < Bq ? lane : 0] == 2);
  const uint64_t todo1 = __ballot(lane + 64 < Bq && tier[lane + 64 < Bq ? lane + 64 : 0] == 2);
  if (!(todo0 | todo1)) return;
  const int nf = __popcll(todo0) + __popcll(todo1);
  if (tid < 128) {
    const uint64_t m = tid < 64 ? todo0 : todo1;
    if ((m >> lane) & 1)
      fq[__popcll(m & ((1ull << lane) - 1)) + (tid < 64 ? 0 : __popcll(todo0))] = tid;
  }
  const int R = gridDim.x;
  const int gw = blockIdx.x * kWavesPerWG + wid, nw = R * kWavesPerWG;
  const int n_tiles = (n_rows + kTileRows - 1) / kTileRows;
  int t_first, t_step, n_mine;
  tile_sequence<true>(gw, nw, n_tiles, t_first, t_step, n_mine);
  const char* cbase = reinterpret_cast<const char*>(corpus);
  const int voff = lane * 16;
  const int j = lane & 15;   // the lane's MFMA column = marked query qb + j of the stream
  // default cache policy: a tile with candidates is re-read from L2 by exact_tile_scores
  auto load = [&](half8(&a)[CS], int t_in, int c) __attribute__((always_inline)) {
    const int t = __builtin_amdgcn_readfirstlane(t_in);
    tile_load<CS, false>(a, cbase + (int64_t)t * (S * 1024) + c * (CS * 1024), voff);
    __builtin_amdgcn_sched_barrier(0);
  };

  for (int qb = 0; qb < nf; qb += kRescanQ) {
    const int nq = min(kRescanQ, nf - qb);
    __syncthreads();   // fq written; the previous stream's LDS reads done
    for (int idx = tid; idx < S * 64; idx += kScanBlock) {
      const int jj = idx & 15;
      half8 v = {};
      if (jj < nq) {
        const int q = fq[qb + jj], s = idx >> 6, hh = (idx >> 4) & 3;
        v = qfrag[(q / kQ) * (2 * S * 64) + (((q % kQ) >> 4) * S + s) * 64 + hh * 16 + (q & 15)];
      }
      bl[idx] = v;
    }
    if constexpr (REG)
      for (int idx = tid; idx < nq * D; idx += kScanBlock)
        qd[idx] = (double)qn[(int64_t)fq[qb + idx / D] * D + idx % D];
#pragma unroll
    for (int e = 0; e < kRescanQ * kKS / 64; ++e) {
      (&ws[wid][0][0])[lane + 64 * e] = kNegInf;
      (&wi[wid][0][0])[lane + 64 * e] = kIdNone32;
    }
    // column j's query: floor L, running threshold, bound, filter
    const bool live = j < nq;
    const int qj = live ? fq[qb + j] : 0;
    const float L = t2[2 * qj], ej = eps[qj];
    float thr = nextafterf(t2[2 * qj + 1], kNegInf);
    uint32_t fm = 0, fv = 0;
    if constexpr (FILTER) {
      fm = filt[2 * qj];
      fv = filt[2 * qj + 1];
    }
    float band = live ? fmaxf(L, thr - ej) : __builtin_inff();
    __syncthreads();

    // one tile's MFMA scores -> its marked-query candidates (cur: the tile's registers, REG)
    auto candidates = [&](const floatx4& acc, int t, const half8* cur)
                          __attribute__((always_inline)) {
      // rows 16t + 4(lane >> 4) + i of column j: any inside j's band?
      const int rbase = t * kTileRows + 4 * (lane >> 4);
      uint4 tg = {0u, 0u, 0u, 0u};
      if constexpr (FILTER) tg = *reinterpret_cast<const uint4*>(tags + rbase);
      bool hit = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bool ok = rbase + i < n_rows && acc[i] >= band;
        if constexpr (FILTER) {
          const uint32_t tr = i == 0 ? tg.x : i == 1 ? tg.y : i == 2 ? tg.z : tg.w;
          ok = ok && ((tr & fm) == fv);
        }
        hit = hit || ok;
      }
      const uint64_t bm = __ballot(hit);
      uint32_t qm = (uint32_t)((bm | (bm >> 16) | (bm >> 32) | (bm >> 48)) & 0xffffu);
      if (!qm) return;
      const int row = t * kTileRows + j;      // lanes 0..15 carry row 16t + lane below
      uint32_t rt = 0;
      if constexpr (FILTER) rt = tags[row < n_rows ? row : 0];
      while (qm) {
        const int c = __builtin_ctz(qm);
        qm &= qm - 1;
        const float tc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(thr), c));
        float e;
        const int q = __builtin_amdgcn_readlane(qj, c);
        if (rows32) {
          e = exact_tile_scores<D, true>(corpus, rows32, t, qn + (int64_t)q * D, lane);
        } else {
          if constexpr (REG)
            e = exact_tile_scores_reg<D>(*reinterpret_cast<const half8(*)[S]>(cur), qd + c * D,
                                         lane);
          else
            e = exact_tile_scores<D, false>(corpus, rows32, t, qn + (int64_t)q * D, lane);
        }
        bool cand = lane < 16 && row < n_rows && e > tc;
        if constexpr (FILTER) {
          const uint32_t fmc = __builtin_amdgcn_readlane(fm, c);
          const uint32_t fvc = __builtin_amdgcn_readlane(fv, c);
          cand = cand && ((rt & fmc) == fvc);
        }
        if (!__ballot(cand)) continue;
        float s = cand ? e : kNegInf;
        int id = cand ? row : kIdNone32;
        if (lane >= 32) {
          s = ws[wid][c][lane - 32];
          id = wi[wid][c][lane - 32];
        }
        lds_fence();
        bitonic_sort64(s, id, lane);
        if (lane < 32) {
          ws[wid][c][lane] = s;
          wi[wid][c][lane] = id;
        }
        lds_fence();
        const float nt = __shfl(s, 31, 64);
        if (j == c) {
          thr = fmaxf(thr, nt);
          band = fmaxf(L, thr - ej);
        }
      }
    };

    if (n_mine > 0) {
      half8 ra[CS], rb[CS];
      if constexpr (NCH == 1) {
        // whole tiles, slots alternating per tile (REG)
        auto tile_of = [&](int jt) { return t_first + min(jt, n_mine - 1) * t_step; };
        auto score = [&](const half8(&a)[CS]) __attribute__((always_inline)) {
          floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < CS; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], bl[s * 64 + lane], acc, 0, 0, 0);
          return acc;
        };
        load(ra, t_first, 0);
        for (int jt = 0; jt < n_mine; jt += 2) {
          load(rb, tile_of(jt + 1), 0);
          candidates(score(ra), tile_of(jt), ra);
          if (jt + 1 >= n_mine) break;
          load(ra, tile_of(jt + 2), 0);
          candidates(score(rb), tile_of(jt + 1), rb);
        }
      } else {
        load(ra, t_first, 0);
        for (int jt = 0; jt < n_mine; ++jt) {
          const int t = t_first + jt * t_step;
          const int tn = t_first + min(jt + 1, n_mine - 1) * t_step;
          floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            if (c % 2 == 0) {
              load(rb, t, c + 1);
#pragma unroll
              for (int s = 0; s < CS; ++s)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ra[s], bl[(c * CS + s) * 64 + lane],
                                                             acc, 0, 0, 0);
            } else {
              if (c + 1 < NCH)
                load(ra, t, c + 1);
              else
                load(ra, tn, 0);
#pragma unroll
              for (int s = 0; s < CS; ++s)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(rb[s], bl[(c * CS + s) * 64 + lane],
                                                             acc, 0, 0, 0);
            }
          }
          candidates(acc, t, nullptr);
        }
      }
    }
    __syncthreads();
    // this workgroup's 32 best per query of the stream (wave w: queries w, w + 4, ...)
    for (int c = wid; c < nq; c += kWavesPerWG) {
      float x = lane < 32 ? ws[0][c][lane] : kNegInf;
      int id = lane < 32 ? wi[0][c][lane] : kIdNone32;
      for (int v = 1; v < kWavesPerWG; ++v) {
        if (lane >= 32) {
          x = ws[v][c][63 - lane];
          id = wi[v][c][63 - lane];
        }
        bitonic_merge64(x, id, lane);
      }
      const int64_t o = ((int64_t)fq[qb + c] * kRescanMaxWG + blockIdx.x) * kKS;
      if (lane < 32) {
        lst_s[o + lane] = x;
        lst_i[o + lane] = id;
      }
    }
  }
  // ---- publish: stores drained, agent release, then the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = atomicAdd(ticket, 1) == R - 1;
  }
  __syncthreads();
  if (!last) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  // ---- last arriver: each marked query's R lists -> its exact top-k (wave w merges lists
  //      w, w + 4, ...; wave 0 the four results). The lists are loaded 8 at a time ahead of
  //      their merges (one L2 round trip per 8 lists, not per list: the serial per-list loads
  //      made this tail ~0.5 ms for 4 marked queries at R = 512), and a list whose best entry
  //      scores below the running 32nd is skipped (none of its entries can enter).
  constexpr int kPf = 8;
  for (int i = 0; i < nf; ++i) {
    const int q = fq[i];
    float x = kNegInf;
    int id = kIdNone32;
    for (int b0 = wid; b0 < R; b0 += kWavesPerWG * kPf) {
      float xs[kPf];
      int is[kPf];
#pragma unroll
      for (int u = 0; u < kPf; ++u) {
        const int w2 = b0 + kWavesPerWG * u;
        const int64_t o = ((int64_t)q * kRescanMaxWG + min(w2, R - 1)) * kKS + 63 - lane;
        const bool use = w2 < R && lane >= 32;
        xs[u] = use ? lst_s[lane >= 32 ? o : 0] : kNegInf;
        is[u] = use ? lst_i[lane >= 32 ? o : 0] : kIdNone32;
      }
#pragma unroll
      for (int u = 0; u < kPf; ++u) {
        const float head = __shfl(xs[u], 63, 64), t32 = __shfl(x, 31, 64);
        if (head < t32 || head == kNegInf) continue;   // wave-uniform
        if (lane >= 32) {
          x = xs[u];
          id = is[u];
        }
        bitonic_merge64(x, id, lane);
      }
    }
    if (lane < 32) {
      ws[wid][0][lane] = x;
      wi[wid][0][lane] = id;
    }
    __syncthreads();
    if (wid == 0) {
      x = lane < 32 ? ws[0][0][lane] : kNegInf;
      id = lane < 32 ? wi[0][0][lane] : kIdNone32;
      for (int v = 1; v < kWavesPerWG; ++v) {
        if (lane >= 32) {
          x = ws[v][0][63 - lane];
          id = wi[v][0][63 - lane];
        }
        bitonic_merge64(x, id, lane);
      }
      if (lane < k) {
        const bool ok = x != kNegInf;
        if (out_packed) {
          out_packed[((int64_t)q * k + lane) * 2] = __float_as_int(x);
          out_packed[((int64_t)q * k + lane) * 2 + 1] = ok ? (int32_t)(id + id_offset) : -1;
        } else {
          out_s[(int64_t)q * k + lane] = x;
          out_i[(int64_t)q * k + lane] = ok ? (int64_t)id + id_offset : (int64_t)-1;
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) *ticket = 0;   // re-armed for the workspace's next pass (stream order)
}

// Diagnostic stand-in for a skipped rescan launch (RAGMI_RESCAN_WG=0 under
// RAG_CREATE_DIAGNOSTIC): the pass's marked queries get no output, so they are re-marked
// tier 3 and counted as unanswered (rag_index_unanswered) instead of passing as certified.
__global__ __launch_bounds__(64) void mark_unanswered_kernel(int* __restrict__ tier, int Bq,
                                                             unsigned long long* __restrict__ cnt) {
  int n = 0;
  for (int q = threadIdx.x; q < Bq; q += 64)
    if (tier[q] == 2) {
      tier[q] = 3;
      ++n;
    }
  for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d, 64);
  if (threadIdx.x == 0 && n > 0) atomicAdd(&cnt[2], (unsigned long long)n);
}

}  // namespace ragmi
