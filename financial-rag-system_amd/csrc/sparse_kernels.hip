// sparse_kernels.hip — the sparse column of an index (include/ragmi.h "Sparse vectors"): its
// storage kernels (fill / write / gather / move / df), the per-pass query table (sp_prep_kernel)
// and the streaming scorer (sp_score_kernel) behind rag_index_sparse_search. Included by
// index_search.hip after largek_kernels.hip, whose bound, final and emit kernels select from
// the scores computed here.
namespace ragmi {

constexpr int kSpQueryNnz = 64;      // RAG_SPARSE_MAX_QUERY_NNZ: slots of a padded query
constexpr uint32_t kSpNone = 0xFFFFu;  // RAG_SPARSE_TERM_NONE
constexpr int kSpTerms = 65535;      // terms lie in [0, kSpTerms)
constexpr int kSpUnion = 512;        // RAG_SPARSE_MAX_UNION: distinct terms of one pass's queries
constexpr int kSpBlock = 256;        // storage kernels: one thread per slot
constexpr int kSpScoreBlock = 512;   // scorer: 8 waves per workgroup
constexpr int kSpWaves = kSpScoreBlock / 64;
constexpr int kSpRowGroup = 4;       // rows whose first 64 terms a wave loads together
constexpr int kSpTileRows = 16;      // rows of a sample tile

// The query table of one pass, in the workspace (uint32 words) and, copied, in LDS:
//   [kSpTabU]        U, the distinct terms of the pass's queries
//   [kSpTabOver]     1 when U > kSpUnion: the pass is left unanswered
//   [kSpTabFilt ..)  (mask, value) per query, (0, 0) = every row
//   [kSpTabEps ..)   32 fp32 zeros: the eps of lk_bound_kernel / lk_final_kernel (scores are exact)
//   [kSpTabBits ..)  the membership bitmap, bit t % 32 of word t / 32
//   [kSpTabPref ..)  uint16 per bitmap word: the members below the word
//   [kSpTabMask ..)  per union term j: bit q set when query q holds the term
//   [kSpTabW ..)     W[j][q] fp32, query q's weight of union term j (0 where it has none)
constexpr int kSpTabU = 0, kSpTabOver = 1;
constexpr int kSpTabFilt = 16;
constexpr int kSpTabEps = kSpTabFilt + 2 * kQ;
constexpr int kSpTabBits = kSpTabEps + kQ;
constexpr int kSpBitWords = 2048;
constexpr int kSpTabPref = kSpTabBits + kSpBitWords;
constexpr int kSpTabMask = kSpTabPref + kSpBitWords / 2;
constexpr int kSpTabW = kSpTabMask + kSpUnion;
constexpr int kSpTabWords = kSpTabW + kSpUnion * kQ;

// ----------------------------------------------------------------------------------------
// storage: terms uint16 [cap][S], vals fp32 [cap][S]; one thread per slot; a row index outside
// [0, cap_rows) is never dereferenced
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpBlock) void sp_fill_kernel(uint16_t* __restrict__ terms,
                                                           float* __restrict__ vals, int64_t i0,
                                                           int64_t i1) {
  const int64_t i = i0 + (int64_t)blockIdx.x * kSpBlock + threadIdx.x;
  if (i < i1) {
    terms[i] = (uint16_t)kSpNone;
    vals[i] = 0.0f;
  }
}

__global__ __launch_bounds__(kSpBlock) void sp_write_kernel(
    uint16_t* __restrict__ terms, float* __restrict__ vals, const int64_t* __restrict__ rows,
    const uint16_t* __restrict__ in_t, const float* __restrict__ in_v, int64_t n, int S,
    int64_t cap_rows) {
  const int64_t idx = (int64_t)blockIdx.x * kSpBlock + threadIdx.x;
  if (idx >= n * S) return;
  const int64_t r = rows[idx / S];
  if (r < 0 || r >= cap_rows) return;
  const int64_t to = r * S + idx % S;
  terms[to] = in_t[idx];
  vals[to] = in_v[idx];
}

__global__ __launch_bounds__(kSpBlock) void sp_gather_kernel(
    const uint16_t* __restrict__ terms, const float* __restrict__ vals,
    const int64_t* __restrict__ rows, int64_t n, int S, int64_t cap_rows,
    uint16_t* __restrict__ out_t, float* __restrict__ out_v) {
  const int64_t idx = (int64_t)blockIdx.x * kSpBlock + threadIdx.x;
  if (idx >= n * S) return;
  const int64_t r = rows[idx / S];
  const bool ok = r >= 0 && r < cap_rows;
  const int64_t from = ok ? r * S + idx % S : 0;
  out_t[idx] = ok ? terms[from] : (uint16_t)kSpNone;
  out_v[idx] = ok ? vals[from] : 0.0f;
}

__global__ __launch_bounds__(kSpBlock) void sp_move_kernel(
    uint16_t* __restrict__ terms, float* __restrict__ vals, const int64_t* __restrict__ src_rows,
    const int64_t* __restrict__ dst_rows, int64_t n, int S, int64_t cap_rows) {
  const int64_t idx = (int64_t)blockIdx.x * kSpBlock + threadIdx.x;
  if (idx >= n * S) return;
  const int64_t s = src_rows[idx / S], d = dst_rows[idx / S];
  if (s < 0 || s >= cap_rows || d < 0 || d >= cap_rows) return;
  const int c = (int)(idx % S);
  terms[d * S + c] = terms[s * S + c];
  vals[d * S + c] = vals[s * S + c];
}

// document frequency: out[t] += 1 per slot of the rows below the count that holds term t
// (`slots` = count * S); integer atomics only
__global__ __launch_bounds__(kSpBlock) void sp_df_kernel(const uint16_t* __restrict__ terms,
                                                         int64_t slots,
                                                         unsigned long long* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kSpBlock + threadIdx.x; i < slots;
       i += (int64_t)gridDim.x * kSpBlock) {
    const uint32_t t = terms[i];
    if (t < (uint32_t)kSpTerms) atomicAdd(&out[t], 1ull);
  }
}

// ----------------------------------------------------------------------------------------
// The pass's query table from its padded queries (q_terms uint16 [Bq][64] ascending, q_vals fp32
// [Bq][64], q_nnz int32 [Bq], read clamped to [0, 64]; a term >= 65535 is ignored). One
// workgroup. filt: the queries' (mask, value) pairs or NULL.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sp_prep_kernel(const uint16_t* __restrict__ q_terms,
                                                      const float* __restrict__ q_vals,
                                                      const int32_t* __restrict__ q_nnz, int Bq,
                                                      const uint32_t* __restrict__ filt,
                                                      uint32_t* __restrict__ tab) {
  __shared__ uint32_t bits[kSpBitWords];
  __shared__ uint32_t pref[kSpBitWords];
  __shared__ int part[256];
  const int tid = threadIdx.x;
  for (int i = tid; i < kSpBitWords; i += 256) bits[i] = 0u;
  __syncthreads();
  auto entry = [&](int idx, uint32_t& t) -> bool {   // slot idx of the pass holds a query term
    const int q = idx / kSpQueryNnz, i = idx % kSpQueryNnz;
    const int nz = min(max(q_nnz[q], 0), kSpQueryNnz);
    if (i >= nz) return false;
    t = q_terms[idx];
    return t < (uint32_t)kSpTerms;
  };
  for (int idx = tid; idx < Bq * kSpQueryNnz; idx += 256) {
    uint32_t t;
    if (entry(idx, t)) atomicOr(&bits[t >> 5], 1u << (t & 31));
  }
  __syncthreads();
  // members below each word: thread tid owns words 8 tid .. 8 tid + 7
  int own = 0;
  for (int j = 0; j < 8; ++j) own += __popc(bits[8 * tid + j]);
  part[tid] = own;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) {
      const int c = part[i];
      part[i] = run;
      run += c;
    }
    tab[kSpTabU] = (uint32_t)run;
    tab[kSpTabOver] = run > kSpUnion ? 1u : 0u;
  }
  __syncthreads();
  int below = part[tid];
  for (int j = 0; j < 8; ++j) {
    pref[8 * tid + j] = (uint32_t)below;
    below += __popc(bits[8 * tid + j]);
  }
  __syncthreads();
  const int U = (int)tab[kSpTabU];
  for (int i = tid; i < kSpBitWords; i += 256) tab[kSpTabBits + i] = bits[i];
  for (int i = tid; i < kSpBitWords / 2; i += 256)
    tab[kSpTabPref + i] = pref[2 * i] | (pref[2 * i + 1] << 16);   // U <= 2048: 16 bits each
  for (int i = tid; i < kQ; i += 256) {
    const bool on = filt != nullptr && i < Bq;
    tab[kSpTabFilt + 2 * i] = on ? filt[2 * i] : 0u;
    tab[kSpTabFilt + 2 * i + 1] = on ? filt[2 * i + 1] : 0u;
    tab[kSpTabEps + i] = 0u;
  }
  if (U > kSpUnion) return;   // workgroup-uniform
  for (int i = tid; i < U; i += 256) tab[kSpTabMask + i] = 0u;
  for (int i = tid; i < U * kQ; i += 256) tab[kSpTabW + i] = 0u;
  __syncthreads();
  for (int idx = tid; idx < Bq * kSpQueryNnz; idx += 256) {
    uint32_t t;
    if (!entry(idx, t)) continue;
    const int q = idx / kSpQueryNnz;
    const int j = (int)pref[t >> 5] + __popc(bits[t >> 5] & ((1u << (t & 31)) - 1u));
    tab[kSpTabW + j * kQ + q] = __float_as_uint(q_vals[idx]);
    atomicOr(&tab[kSpTabMask + j], 1u << q);
  }
}

// ----------------------------------------------------------------------------------------
// The scorer. score(q, r) = fp32(sum over the slots of r in stored order whose term occurs in q
// of (double)val * (double)w_q), accumulated in fp64; -0.0 taken as +0.0. A wave scores one row
// at a time against every query of the pass: it reads 64 slots per step (2 B terms; 4 B values
// only in a step with a hit), tests membership in the LDS bitmap per lane, ballots, walks the
// hits in ascending lane order (slot order: the contract's order), and lane q adds
// val * W[j][q] to query q's accumulator (lanes q and q + 32 read one LDS address: a broadcast,
// and consecutive q consecutive banks). The first empty slot ends the row (rows are padded).
// ----------------------------------------------------------------------------------------
struct SpLds {
  uint32_t bits[kSpBitWords];
  uint32_t pref[kSpBitWords / 2];
  uint32_t mask[kSpUnion];
  float W[kSpUnion * kQ];
};

// the table into LDS (whole workgroup); false when the pass overflowed the union cap
__device__ __forceinline__ bool sp_load_table(const uint32_t* __restrict__ tab, SpLds& L) {
  if (tab[kSpTabOver]) return false;
  const int U = min((int)tab[kSpTabU], kSpUnion);
  for (int i = threadIdx.x; i < kSpBitWords; i += blockDim.x) L.bits[i] = tab[kSpTabBits + i];
  for (int i = threadIdx.x; i < kSpBitWords / 2; i += blockDim.x) L.pref[i] = tab[kSpTabPref + i];
  for (int i = threadIdx.x; i < U; i += blockDim.x) L.mask[i] = tab[kSpTabMask + i];
  for (int i = threadIdx.x; i < U * kQ; i += blockDim.x)
    L.W[i] = __uint_as_float(tab[kSpTabW + i]);
  __syncthreads();
  return true;
}

// one row: `t` holds this lane's term of the row's first 64 slots (kSpNone past S); acc / hit
// are lane (q = lane & 31)'s fp64 sum and its "shares a term" bit
__device__ __forceinline__ void sp_score_row(const uint16_t* __restrict__ trow,
                                             const float* __restrict__ vrow, int S, uint32_t t,
                                             const SpLds& L, int lane, double& acc,
                                             uint32_t& hit) {
  const int ql = lane & 31;
  acc = 0.0;
  hit = 0u;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    if (s0 > 0) t = s < S ? (uint32_t)trow[s] : kSpNone;
    if ((uint32_t)__builtin_amdgcn_readfirstlane((int)t) == kSpNone) break;   // lane 0: slot s0 < S
    const uint32_t word = L.bits[t >> 5];
    const bool mem = (word >> (t & 31)) & 1u;
    unsigned long long hits = __ballot(mem);
    if (hits == 0ull) continue;
    float v = 0.0f;
    int j = 0;
    if (mem) {
      v = vrow[s];
      const uint32_t p = L.pref[t >> 6];
      j = (int)(((t >> 5) & 1u) ? (p >> 16) : (p & 0xFFFFu)) +
          __popc(word & ((1u << (t & 31)) - 1u));
    }
    while (hits) {
      const int src = __ffsll((long long)hits) - 1;
      hits &= hits - 1ull;
      const int jj = __shfl(j, src, 64);
      const float vv = __shfl(v, src, 64);
      acc = fma((double)vv, (double)L.W[jj * kQ + ql], acc);
      hit |= (L.mask[jj] >> ql) & 1u;
    }
  }
}

// rows [ra, rb) by one wave, kSpRowGroup rows' first terms loaded together; on(row, score,
// eligible) per row with this lane's query's score. Eligible: the lane's query exists, shares a
// term with the row, and the row's tag passes its filter.
template <typename F>
__device__ __forceinline__ void sp_wave_rows(const uint16_t* __restrict__ terms,
                                             const float* __restrict__ vals,
                                             const uint32_t* __restrict__ tags, int S, int ra,
                                             int rb, int Bq, uint32_t fm, uint32_t fv,
                                             const SpLds& L, int lane, F&& on) {
  for (int r0 = ra; r0 < rb; r0 += kSpRowGroup) {
    uint32_t t[kSpRowGroup];
#pragma unroll
    for (int i = 0; i < kSpRowGroup; ++i)
      t[i] = (r0 + i < rb && lane < S)
                 ? (uint32_t)__builtin_nontemporal_load(terms + (int64_t)(r0 + i) * S + lane)
                 : kSpNone;
#pragma unroll
    for (int i = 0; i < kSpRowGroup; ++i) {
      const int row = r0 + i;
      if (row >= rb) break;
      double acc;
      uint32_t hit;
      sp_score_row(terms + (int64_t)row * S, vals + (int64_t)row * S, S, t[i], L, lane, acc, hit);
      float s = (float)acc;
      if (s == 0.0f) s = 0.0f;   // -0.0 (an underflowed negative sum) is +0.0
      const bool ok = (lane & 31) < Bq && hit && (tags[row] & fm) == fv;
      on(row, s, ok);
    }
  }
}

enum { kSpSample = 0, kSpCollect = 1, kSpFull = 2 };

// MODE kSpSample: per sample tile i < n_sample (tile i * n_tiles / n_sample, 16 rows) and query
//   q the largest eligible score into smax[q][n_sample] (-inf: none), for lk_bound_kernel.
// MODE kSpCollect: every row; an eligible row with score >= thr[q] is appended, with its score,
//   to query q's candidates (at most kLkCap kept, cnt counts all) — lk_collect_kernel's rule,
//   the score being exact already. round > 0: only when marked, only the marked queries.
// MODE kSpFull: one query; keys[row] = fkey(score) of an eligible row, else 0; vals_out[row] =
//   row; *n_match counts the eligible rows (full_score_kernel's outputs).
template <int MODE>
__global__ __launch_bounds__(kSpScoreBlock) void sp_score_kernel(
    const uint16_t* __restrict__ terms, const float* __restrict__ vals,
    const uint32_t* __restrict__ tags, int S, int n_rows, int Bq, const uint32_t* __restrict__ tab,
    int n_tiles, int n_sample, float* __restrict__ smax,                       // sample
    const float* __restrict__ thr, int* __restrict__ cnt, int* __restrict__ cand,
    float* __restrict__ es, const int* __restrict__ again, const int* __restrict__ need,
    int round,                                                                  // collect
    uint32_t* __restrict__ keys, int* __restrict__ vals_out, int* __restrict__ n_match) {  // full
  __shared__ SpLds L;
  const int lane = threadIdx.x & 63, ql = lane & 31;
  const int wave = blockIdx.x * kSpWaves + (threadIdx.x >> 6);
  const int nw = gridDim.x * kSpWaves;
  if constexpr (MODE == kSpCollect)
    if (!need[round]) return;
  const bool live = sp_load_table(tab, L);   // workgroup-uniform
  const uint32_t fm = tab[kSpTabFilt + 2 * ql], fv = tab[kSpTabFilt + 2 * ql + 1];
  if constexpr (MODE == kSpSample) {
    for (int i = wave; i < n_sample; i += nw) {
      float best = kNegInf;
      if (live) {
        const int tile = (int)((int64_t)i * n_tiles / n_sample);
        const int ra = tile * kSpTileRows, rb = min(ra + kSpTileRows, n_rows);
        sp_wave_rows(terms, vals, tags, S, ra, rb, Bq, fm, fv, L, lane,
                     [&](int, float s, bool ok) { best = ok && s > best ? s : best; });
      }
      if (lane < kQ) smax[(int64_t)lane * n_sample + i] = best;
    }
  } else if constexpr (MODE == kSpCollect) {
    if (!live) return;
    const bool mine = lane < Bq && again[ql];
    const float th = mine ? thr[ql] : __builtin_inff();
    for (int ra = wave * kSpRowGroup; ra < n_rows; ra += nw * kSpRowGroup)
      sp_wave_rows(terms, vals, tags, S, ra, min(ra + kSpRowGroup, n_rows), Bq, fm, fv, L, lane,
                   [&](int row, float s, bool ok) {
                     if (mine && ok && s >= th) {
                       const int pos = atomicAdd(&cnt[ql], 1);
                       if (pos < kLkCap) {
                         cand[ql * kLkCap + pos] = row;
                         es[ql * kLkCap + pos] = s;
                       }
                     }
                   });
  } else {
    int m = 0;
    if (live)
      for (int ra = wave * kSpRowGroup; ra < n_rows; ra += nw * kSpRowGroup)
        sp_wave_rows(terms, vals, tags, S, ra, min(ra + kSpRowGroup, n_rows), 1, fm, fv, L, lane,
                     [&](int row, float s, bool ok) {
                       if (lane == 0) {
                         keys[row] = ok ? fkey(s) : 0u;
                         vals_out[row] = row;
                         m += ok ? 1 : 0;
                       }
                     });
    else
      for (int row = wave * 64 + lane; row < n_rows; row += nw * 64) {
        keys[row] = 0u;
        vals_out[row] = row;
      }
    if (lane == 0 && m > 0) atomicAdd(n_match, m);
  }
}

// after the last round of a hot pass: a pass whose queries' term union exceeded kSpUnion is
// unanswered (its outputs are -inf / -1 already: nothing was collected)
__global__ __launch_bounds__(64) void sp_overflow_kernel(const uint32_t* __restrict__ tab, int Bq,
                                                         int* __restrict__ tier,
                                                         unsigned long long* __restrict__ fb_cnt) {
  if (!tab[kSpTabOver]) return;
  if ((int)threadIdx.x < Bq) tier[threadIdx.x] = 3;
  if (threadIdx.x == 0) atomicAdd(&fb_cnt[2], (unsigned long long)Bq);
}

}  // namespace ragmi
