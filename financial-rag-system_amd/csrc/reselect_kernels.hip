// reselect_kernels.hip — re-selection from a query's exact candidate list (included by
// index_search.hip after certify_kernels.hip): mmr_kernel picks k diverse hits (rag_index_mmr),
// group_select_kernel deals the list into groups by payload key (rag_group_select),
// rrf_fuse_kernel fuses a request's L lists by reciprocal rank (rag_fuse_rrf). All take one
// workgroup per query and read candidate lists, never the scan's state.
namespace ragmi {

// ----------------------------------------------------------------------------------------
// MMR (maximal marginal relevance): k diverse hits re-selected from a query's exact top-C
// list (rag_index_mmr). One workgroup of kMmrBlock threads per query walks the
// greedy steps; the candidate list and the running maxima stay in LDS.
//   n       = min(ncand[b], C, leading candidates whose row lies in [0, cap_rows))
//   step 0  selects j = 0
//   after selecting s: maxsim[j] = max(maxsim[j], sim(s, j)) for every unselected j, where
//           sim(s, j) is the canonical exact score (exact_scores_wave: fp64 fma per lane chunk,
//           xor butterfly, one rounding) of stored row r_j against stored row r_s as fp32
//   step t  selects the unselected j with the largest
//           val[j] = (double)(1.0f - div) * rel[j] - (double)div * maxsim[j]
//           (both products exact in fp64, one rounding), ties to the smallest j
// Per step: the selected row is de-tiled into LDS as row-major fp32; each wave scores 8
// unselected candidates per memory round trip against it, folds them into maxsim and keeps
// its best (val, j); the waves' bests meet in LDS. Two barriers per step, no global traffic
// but the candidate rows. A selected candidate's row slot in LDS is set to -1, which is what
// exact_scores_wave skips. Output in selection order: global row, rel[j], j; -1 / -inf / -1
// past the n-th pick.
// ----------------------------------------------------------------------------------------
constexpr int kMmrBlock = 512;
constexpr int kMmrWaves = kMmrBlock / 64;
constexpr int kMmrMaxC = 1024;    // RAG_MMR_MAX_CANDIDATES

template <int D>
__global__ __launch_bounds__(kMmrBlock) void mmr_kernel(const half8* __restrict__ corpus,
                                                        const float* __restrict__ rows32,
                                                        int64_t cap_rows,
                                                        const float* __restrict__ cand_s,
                                                        const int64_t* __restrict__ cand_r,
                                                        int C, int k,
                                                        const float* __restrict__ diversity,
                                                        const int32_t* __restrict__ ncand,
                                                        float* __restrict__ out_s,
                                                        int64_t* __restrict__ out_i,
                                                        int32_t* __restrict__ out_pos) {
  constexpr int S = steps<D>();
  constexpr int NC = 8;
  __shared__ __attribute__((aligned(16))) float sel_row[D];   // the selected row, fp32
  __shared__ float rel[kMmrMaxC];
  __shared__ float maxsim[kMmrMaxC];
  __shared__ int row_of[kMmrMaxC];       // candidate's stored row; -1 once selected / absent
  __shared__ double wbest_v[kMmrWaves];
  __shared__ int wbest_j[kMmrWaves];
  __shared__ int n_sh;

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* cs = cand_s + (int64_t)b * C;
  const int64_t* cr = cand_r + (int64_t)b * C;
  const int limit = max(0, min(C, ncand ? ncand[b] : C));
  if (tid == 0) n_sh = limit;
  __syncthreads();
  for (int j = tid; j < C; j += kMmrBlock) {
    const int64_t r = j < limit ? cr[j] : -1;
    const bool ok = r >= 0 && r < cap_rows;
    row_of[j] = ok ? (int)r : -1;
    rel[j] = cs[j];
    maxsim[j] = kNegInf;
    if (j < limit && !ok) atomicMin(&n_sh, j);   // the list ends at its first absent row
  }
  __syncthreads();
  const int n = n_sh;
  const int picks = min(k, n);
  const float div = diversity[b];
  const float lam = 1.0f - div;

  int s = 0, made = picks;
  for (int t = 0; t < picks; ++t) {
    // every thread knows s; its row is still in row_of (cleared after the barrier below)
    const int srow = row_of[s];
    if (tid == 0) {
      out_s[(int64_t)b * k + t] = rel[s];
      out_i[(int64_t)b * k + t] = cr[s];
      if (out_pos) out_pos[(int64_t)b * k + t] = s;
    }
    if (t + 1 == picks) break;
    if (rows32) {
      for (int d = tid; d < D; d += kMmrBlock) sel_row[d] = rows32[(int64_t)srow * D + d];
    } else {
      for (int c = tid; c < D / 8; c += kMmrBlock) {
        const half8 x =
            corpus[(int64_t)(srow >> 4) * (S * 64) + (c >> 2) * 64 + (c & 3) * 16 + (srow & 15)];
#pragma unroll
        for (int e = 0; e < 8; ++e) sel_row[8 * c + e] = (float)x[e];
      }
    }
    __syncthreads();                  // sel_row complete; everyone has read row_of[s]
    if (tid == 0) row_of[s] = -1;     // seen past this step's last barrier; until then j == s
                                      // is skipped by index below
    double best_v = -__builtin_inf();
    int best_j = 0x7fffffff;
    for (int j0 = wid * NC; j0 < n; j0 += kMmrWaves * NC) {
      int rows[NC];
      bool any = false;
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        rows[i] = j0 + i < n && j0 + i != s ? row_of[j0 + i] : -1;
        any |= rows[i] >= 0;
      }
      if (!any) continue;             // wave-uniform: row_of is read at wave-uniform indices
      float sc[NC];
      exact_scores_wave<D, NC>(corpus, rows, sel_row, lane, sc, rows32);
      float mine = kNegInf;
      int my_row = -1;
#pragma unroll
      for (int i = 0; i < NC; ++i)
        if (lane == i) {
          mine = sc[i];
          my_row = rows[i];
        }
      if (lane < NC && my_row >= 0) {
        const int j = j0 + lane;
        const float m = fmaxf(maxsim[j], mine);
        maxsim[j] = m;
        const double v = (double)lam * (double)rel[j] - (double)div * (double)m;
        if (v > best_v) {             // a lane meets its j in ascending order
          best_v = v;
          best_j = j;
        }
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const double ov = __shfl_xor(best_v, d, 64);
      const int oj = __shfl_xor(best_j, d, 64);
      if (ov > best_v || (ov == best_v && oj < best_j)) {
        best_v = ov;
        best_j = oj;
      }
    }
    if (lane == 0) {
      wbest_v[wid] = best_v;
      wbest_j[wid] = best_j;
    }
    __syncthreads();
    best_v = wbest_v[0];
    best_j = wbest_j[0];
#pragma unroll
    for (int w = 1; w < kMmrWaves; ++w) {
      const double ov = wbest_v[w];
      const int oj = wbest_j[w];
      if (ov > best_v || (ov == best_v && oj < best_j)) {
        best_v = ov;
        best_j = oj;
      }
    }
    if (best_j >= n) {                // only if no val compared (NaN scores handed in): stop
      made = t + 1;
      break;
    }
    s = best_j;
  }
  for (int t = made + tid; t < k; t += kMmrBlock) {
    out_s[(int64_t)b * k + t] = kNegInf;
    out_i[(int64_t)b * k + t] = -1;
    if (out_pos) out_pos[(int64_t)b * k + t] = -1;
  }
}

// ----------------------------------------------------------------------------------------
// grouped search (rag_group_select; the tag gather that feeds it is
// gather_tags_kernel, rows_kernels.hip).
// group_select_kernel: the sequential walk of include/ragmi.h over one query's candidate list,
// in parallel form. One workgroup per query; it reads only its input arrays (no index).
//   key[j]   = tag[j] & key_mask, in LDS (16 KiB at C = 4096)
//   rank[j]  = number of i < j with key[i] == key[j]
//   first[j] = key[j] != 0 && rank[j] == 0; the group index of a key = the number of firsts
//              before its own first
//   emit iff key[j] != 0, group index < G, rank < S, at out[b][group][rank]
// The list is walked in trips of kGrpBlock candidates, in order, against a table of the groups
// opened so far (s_gkey, in opening order; s_cnt, their candidates seen in earlier trips). A
// candidate looks its key up in the table (the earlier trips), then counts the earlier
// candidates of its own trip with its key, so rank = s_cnt[group] + the in-trip count and a
// trip costs ng / 4 + at most kGrpBlock / 4 LDS reads per lane however long the list is. A key
// that is in neither is a first: it takes index ng + the number of this trip's earlier firsts
// (ballot / popcount per wave, wave totals in LDS) and enters the table while that is < G; a
// later candidate of the trip with the same key reads the index back from its first's lane
// (s_tg). A candidate whose group already holds S hits, or whose key is unknown when G groups
// are open, can never be emitted and takes no further part. Both loops read LDS four keys at a
// time at a wave-uniform address (a broadcast: no bank conflict); the in-trip one runs to the
// wave's last candidate and a lane masks off the entries at or past its own j.
// Every position is a pure function of the inputs: integer LDS atomics only (min, add), whose
// results do not depend on their order, so the output is the same on every run. Every output
// element is written exactly once: the emitted entries in the trips, the padding (-inf / -1 /
// -1, key 0, fill 0) after the last one from the counts.
// ----------------------------------------------------------------------------------------
constexpr int kGrpBlock = 512;
constexpr int kGrpMaxC = 4096;      // RAG_GROUPS_MAX_CANDIDATES
constexpr int kGrpMaxG = 1024;      // RAG_GROUPS_MAX
constexpr int kGrpMaxCells = 4096;  // G * S

__global__ __launch_bounds__(kGrpBlock) void group_select_kernel(
    const float* __restrict__ cand_s, const int64_t* __restrict__ cand_r,
    const uint32_t* __restrict__ cand_t, const int32_t* __restrict__ ncand, int C,
    uint32_t key_mask, int G, int S, uint32_t* __restrict__ out_keys, int32_t* __restrict__ out_fill,
    float* __restrict__ out_s, int64_t* __restrict__ out_r, int32_t* __restrict__ out_pos,
    int32_t* __restrict__ out_count) {
  __shared__ __attribute__((aligned(16))) uint32_t s_key[kGrpMaxC];
  __shared__ __attribute__((aligned(16))) uint32_t s_gkey[kGrpMaxG];   // keys of the open groups
  __shared__ int s_cnt[kGrpMaxG];    // their candidates seen in the earlier trips
  __shared__ int s_tg[kGrpBlock];    // group index of this trip's firsts, by lane
  __shared__ int s_wcnt[kGrpBlock / 64];
  __shared__ int s_n;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = blockIdx.x;
  cand_s += b * C;
  cand_r += b * C;
  cand_t += b * C;
  const int64_t obase = b * G * S;

  if (tid == 0) {
    int n0 = C;
    if (ncand) n0 = min(C, max(0, ncand[b]));
    s_n = n0;
  }
  for (int g = tid; g < ((G + 3) & ~3); g += kGrpBlock) {   // <= kGrpMaxG; 0 matches no live key
    s_gkey[g] = 0u;
    s_cnt[g] = 0;
  }
  __syncthreads();
  for (int j = tid; j < C; j += kGrpBlock) {
    s_key[j] = cand_t[j] & key_mask;
    if (cand_r[j] < 0) atomicMin(&s_n, j);   // the list ends at its first absent row
  }
  __syncthreads();
  const int n = s_n;

  const unsigned long long below = (1ull << lane) - 1ull;
  int ng = 0;   // open groups (uniform)
  for (int base = 0; base < n; base += kGrpBlock) {
    const int j = base + tid;
    uint32_t key = j < n ? s_key[j] : 0u;
    int g = -1, before = 0;
    if (key != 0u) {
      for (int e = 0; e < ng; e += 4) {
        const uint4 k4 = *reinterpret_cast<const uint4*>(&s_gkey[e]);
        g = k4.x == key ? e : k4.y == key ? e + 1 : k4.z == key ? e + 2 : k4.w == key ? e + 3 : g;
      }
      if (g >= 0) before = s_cnt[g];
      // its group is full, or no group is left to open: never emitted (nor are its key's others)
      if (g >= 0 ? before >= S : ng >= G) key = 0u;
    }
    int rank_in = 0, fin = -1;   // this trip's earlier candidates with the key; the first of them
    if (key != 0u) {
      const int lend = min(n, base + (w + 1) * 64);   // wave-uniform: the wave's last candidate
      for (int i = base; i < lend; i += 4) {
        const uint4 k4 = *reinterpret_cast<const uint4*>(&s_key[i]);
        const bool m0 = i < j && k4.x == key;
        const bool m1 = i + 1 < j && k4.y == key;
        const bool m2 = i + 2 < j && k4.z == key;
        const bool m3 = i + 3 < j && k4.w == key;
        if (fin < 0) fin = m0 ? i : m1 ? i + 1 : m2 ? i + 2 : m3 ? i + 3 : -1;
        rank_in += (int)m0 + (int)m1 + (int)m2 + (int)m3;
      }
    }
    const bool first = key != 0u && g < 0 && rank_in == 0;
    const unsigned long long fb = __ballot(first);
    if (lane == 0) s_wcnt[w] = __popcll(fb);
    __syncthreads();   // every lane has read the table and the counts
    int wbase = 0, tot = 0;
    for (int u = 0; u < kGrpBlock / 64; ++u) {
      const int t = s_wcnt[u];
      if (u < w) wbase += t;
      tot += t;
    }
    if (first) {
      g = ng + wbase + __popcll(fb & below);
      s_tg[tid] = g;
      if (g < G) s_gkey[g] = key;
    }
    __syncthreads();   // this trip's firsts are in s_tg
    if (key != 0u && g < 0) g = s_tg[fin - base];
    if (key != 0u && g < G) {
      const int rank = before + rank_in;
      if (first) out_keys[b * G + g] = key;
      if (rank < S) {
        const int64_t o = obase + (int64_t)g * S + rank;
        out_s[o] = cand_s[j];
        out_r[o] = cand_r[j];
        if (out_pos) out_pos[o] = j;
      }
      atomicAdd(&s_cnt[g], 1);
    }
    ng = min(ng + tot, G);
    __syncthreads();   // table, counts, s_tg and s_wcnt are settled for the next trip
  }
  for (int g = tid; g < G; g += kGrpBlock) {
    out_fill[b * G + g] = min(s_cnt[g], S);
    if (g >= ng) out_keys[b * G + g] = 0u;
  }
  const int cells = G * S;
  for (int e = tid; e < cells; e += kGrpBlock) {
    const int g = e / S, r = e - g * S;
    if (r >= s_cnt[g]) {
      out_s[obase + e] = kNegInf;
      out_r[obase + e] = -1;
      if (out_pos) out_pos[obase + e] = -1;
    }
  }
  if (tid == 0) {
    out_count[b * 2] = ng;
    out_count[b * 2 + 1] = n;
  }
}

// ----------------------------------------------------------------------------------------
// reciprocal rank fusion (rag_fuse_rrf). One workgroup per request fuses its L
// candidate lists of C rows each; it reads only its input arrays (no index). L * C <= kRrfMaxE.
//   n[l]     = min(ncand[b][l] clamped to [0, C], leading entries of list l with row >= 0)
//   entry e  = l * C + p is live iff p < n[l]; its contribution is 1.0 / (double)(rrf_k + p)
//   fused(r) = (float) of the fp64 sum, from 0.0, of the contributions of the live entries
//              holding r, in ascending e (= list ascending, position ascending)
//   output   = the distinct rows by (fused descending, row ascending), the first k of them
// The live entries sit in LDS as (row as uint64, e); a dead entry's row is ~0, above every
// live one (rows are >= 0). A bitonic sort over N = the power of two >= L * C orders them by
// (row, e), so the entries of a row are one run in summation order. The lane at a run's head
// walks the run and adds in fp64; the results wait in registers past a barrier (the walks read
// what the results overwrite), then the head's slot becomes (row, ~bits of the fused fp32) and
// every other slot dead. The fused values are positive and finite, so ~bits ascending is the
// value descending; a second bitonic sort by (~bits, row) leaves the result at the front.
// The order is total over distinct rows, so the output is a pure function of the inputs:
// integer LDS atomics only (min for n[l], add for the count of heads). Every output element
// is written exactly once, in loops of kRrfBlock (C and k may both exceed the block).
// ----------------------------------------------------------------------------------------
constexpr int kRrfBlock = 512;
constexpr int kRrfMaxL = 16;       // RAG_FUSION_MAX_LISTS
constexpr int kRrfMaxE = 4096;     // RAG_FUSION_MAX_ENTRIES
constexpr int kRrfPer = kRrfMaxE / kRrfBlock;   // slots per thread at the limit

// N slots of (k64, k32), ascending by (k64, k32) if RowMajor else by (k32, k64). N is a power
// of two >= 2; every thread of the block calls it. Ends on a barrier.
template <bool RowMajor>
__device__ __forceinline__ void rrf_bitonic(uint64_t* k64, uint32_t* k32, int N, int tid) {
  for (int size = 2; size <= N; size <<= 1) {
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (N >> 1); t += kRrfBlock) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int hi = lo | j;
        const uint64_t a64 = k64[lo], b64 = k64[hi];
        const uint32_t a32 = k32[lo], b32 = k32[hi];
        const bool gt = RowMajor ? (a64 > b64 || (a64 == b64 && a32 > b32))
                                 : (a32 > b32 || (a32 == b32 && a64 > b64));
        if (gt == ((lo & size) == 0)) {
          k64[lo] = b64;
          k64[hi] = a64;
          k32[lo] = b32;
          k32[hi] = a32;
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kRrfBlock) void rrf_fuse_kernel(
    const int64_t* __restrict__ cand_r, const int32_t* __restrict__ ncand, int L, int C, int k,
    int rrf_k, float* __restrict__ out_s, int64_t* __restrict__ out_r,
    int32_t* __restrict__ out_count) {
  __shared__ uint64_t s_row[kRrfMaxE];
  __shared__ uint32_t s_aux[kRrfMaxE];   // e, then ~bits of the fused value
  __shared__ int s_n[kRrfMaxL];
  __shared__ int s_m;
  constexpr uint64_t kDead = ~0ull;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int E = L * C;               // <= kRrfMaxE
  int N = 2;
  while (N < E) N <<= 1;             // <= kRrfMaxE
  cand_r += b * E;

  if (tid < L) s_n[tid] = ncand ? min(C, max(0, ncand[b * L + tid])) : C;
  if (tid == 0) s_m = 0;
  __syncthreads();
  for (int e = tid; e < E; e += kRrfBlock) {
    const int l = e / C, p = e - l * C;
    if (cand_r[e] < 0) atomicMin(&s_n[l], p);   // a list ends at its first negative row
  }
  __syncthreads();
  for (int e = tid; e < N; e += kRrfBlock) {
    uint64_t r = kDead;
    if (e < E) {
      const int l = e / C, p = e - l * C;
      if (p < s_n[l]) r = (uint64_t)cand_r[e];
    }
    s_row[e] = r;
    s_aux[e] = (uint32_t)e;
  }
  __syncthreads();
  rrf_bitonic<true>(s_row, s_aux, N, tid);

  uint32_t fused[kRrfPer];           // ~bits for a run's head, ~0 for every other slot
  int heads = 0;
#pragma unroll
  for (int u = 0; u < kRrfPer; ++u) {
    const int i = tid + u * kRrfBlock;
    fused[u] = ~0u;
    if (i >= N) continue;
    const uint64_t r = s_row[i];
    if (r == kDead || (i > 0 && s_row[i - 1] == r)) continue;
    double sum = 0.0;
    for (int j = i; j < N && s_row[j] == r; ++j) {
      const int e = (int)s_aux[j];
      const int p = e - (e / C) * C;
      sum += 1.0 / (double)((int64_t)rrf_k + p);
    }
    fused[u] = ~__float_as_uint((float)sum);
    ++heads;
  }
  if (heads) atomicAdd(&s_m, heads);
  __syncthreads();                   // every walk has read its run
#pragma unroll
  for (int u = 0; u < kRrfPer; ++u) {
    const int i = tid + u * kRrfBlock;
    if (i >= N) continue;
    if (fused[u] == ~0u) s_row[i] = kDead;
    s_aux[i] = fused[u];
  }
  __syncthreads();
  rrf_bitonic<false>(s_row, s_aux, N, tid);

  const int m = s_m;                 // distinct rows, <= E <= N
  for (int t = tid; t < k; t += kRrfBlock) {
    const bool live = t < m;
    out_s[b * k + t] = live ? __uint_as_float(~s_aux[t]) : kNegInf;
    out_r[b * k + t] = live ? (int64_t)s_row[t] : -1;
  }
  if (out_count && tid == 0) out_count[b] = m;
}

}  // namespace ragmi
