// order_kernels.hip — ranking and counting over the payload columns (included by
// index_store.hip after rows_kernels.hip, whose select chunking, scan and KeyCols it uses): the
// kernels behind rag_index_order_rows (order_by: the `limit` best rows of one key column) and
// rag_index_facet_counts (facet: rows per code of one tag field), DESIGN.md §R16.
//
// Both stream the columns the way select_flags does: a lane owns 4 consecutive rows, r a multiple
// of 4, one 16-byte load of the view / tags and two 16-byte loads of the keys, issued only when
// r < count — the columns hold a multiple of 16 rows, so the loads stay inside them. A row at or
// past `count` is never eligible, whatever its (unspecified) key or tag holds.
//
// No reference counterpart: the reference never scrolls, orders or facets; it leaves all three to
// the Qdrant server.
namespace ragmi {

// ----------------------------------------------------------------------------------------
// order_rows. A row is eligible when r < count, bit 0 of view[r] is set (view == nullptr: every
// row), key != RAG_KEY_ABSENT and lo <= key <= hi (signed). Every key is mapped to a RANK, an
// unsigned 64-bit number of which the smaller is the better in both directions:
//   rank = key ^ 2^63 (the biased key), complemented for RAG_ORDER_DESC
// so the order asked for is (rank asc, row asc) and one code path serves both directions.
//
//   order_hist_kernel  x 8   radix select of the limit-th smallest rank, 8-bit digits, most
//                            significant first. Pass p counts digit p of the eligible rows whose
//                            p leading digits equal the prefix found so far: an LDS histogram per
//                            workgroup, added to the pass's own 256 global counters. Pass p + 1
//                            (every workgroup of it) reads pass p's counters and fixes digit p
//                            itself (order_resolve), so nothing runs between two passes.
//   order_count_kernel       fixes the last digit: the threshold T and how many rows of rank T
//                            are wanted; then per chunk of kSelChunk rows the eligible rows of
//                            rank < T and those of rank == T
//   order_scan_kernel        exclusive prefix sums of both over the chunks; out_n
//   order_emit_kernel        the rows of rank < T from their offsets, then the rows of rank == T
//                            in row order while the list is not full
//   order_sort_kernel        one workgroup sorts the <= RAG_ORDER_MAX pairs by (rank, row) in LDS
//                            and pads the tail
// Fewer eligible rows than `limit` (pass 0's counters say so) sets the state's `all` flag: the
// later passes return at once and every eligible row is emitted.
// Atomics add integer counts only; every position is a pure function of the columns, so the
// output is the same bits on every run.
// ----------------------------------------------------------------------------------------
constexpr int kOrdBlock = 256;
constexpr int kOrdRows = kOrdBlock * 4;   // rows per workgroup step of a histogram pass
constexpr int kOrdWgPerCu = 4;            // 16 waves per CU, 48 B in flight per lane
constexpr int kOrdPasses = 8;
constexpr int kOrdSortBlock = 1024;
static_assert(kSelBlock == kOrdBlock, "order_count / order_emit walk select's chunks");

using u64 = unsigned long long;

// the select's state going into pass p: the p leading digits of the threshold, how many rows of
// that prefix are still wanted, and "fewer eligible rows than the limit"
struct OrderState {
  u64 prefix;
  u64 need;
  u64 all;
  u64 pad;
};

struct OrderArgs {
  const uint32_t* view;   // nullptr: every row < count
  const int64_t* keys;
  int64_t count;
  int64_t lo, hi;
  uint32_t desc;
};

__device__ __forceinline__ u64 order_rank(int64_t key, uint32_t desc) {
  const u64 b = (u64)key ^ 0x8000000000000000ull;
  return desc ? ~b : b;
}

__device__ __forceinline__ int64_t order_key(u64 rank, uint32_t desc) {
  return (int64_t)((desc ? ~rank : rank) ^ 0x8000000000000000ull);
}

// rows r .. r + 3: e[j] = eligible, k[j] = key, u[j] = rank (k, u are 0 where nothing was
// loaded). A lane whose 4 rows all fail the program does not load their keys: under a selective
// filter most waves then read the view alone, 4 B per row instead of 12.
__device__ __forceinline__ void order_load(const OrderArgs& a, int64_t r, bool (&e)[4],
                                           int64_t (&k)[4], u64 (&u)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    e[j] = false;
    k[j] = 0;
    u[j] = 0ull;
  }
  if (r < a.count) {
    uint4 v4 = make_uint4(1u, 1u, 1u, 1u);
    if (a.view) {
      v4 = *reinterpret_cast<const uint4*>(a.view + r);
      if (((v4.x | v4.y | v4.z | v4.w) & 1u) == 0u) return;
    }
    const longlong2* kp = reinterpret_cast<const longlong2*>(a.keys + r);
    const longlong2 k01 = kp[0], k23 = kp[1];
    const uint32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
    k[0] = k01.x;
    k[1] = k01.y;
    k[2] = k23.x;
    k[3] = k23.y;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e[j] = r + j < a.count && (v[j] & 1u) && k[j] != RAG_KEY_ABSENT && a.lo <= k[j] &&
             k[j] <= a.hi;
      u[j] = order_rank(k[j], a.desc);
    }
  }
}

// bins[d] += 1 for every lane with `e` set; one add of the lanes' count when they all name the
// same bin (timestamps of one second share 7 digits: the per-lane adds would serialise).
// Called by whole waves.
template <typename T>
__device__ __forceinline__ void hist_add(T* bins, bool e, uint32_t d) {
  const u64 m = __ballot(e);
  if (m == 0) return;
  const int leader = __ffsll((long long)m) - 1;
  const uint32_t d0 = __shfl(d, leader);
  if (__ballot(e && d == d0) == m) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&bins[d0], (T)__popcll(m));
  } else if (e) {
    atomicAdd(&bins[d], (T)1);
  }
}

// The state going into pass p >= 1, from the state going into pass p - 1 and that pass's
// counters: digit p - 1 of the threshold is the bin in which the running count reaches `need`.
// Called by every thread of a kOrdBlock workgroup; all return the same value.
__device__ OrderState order_resolve(const u64* __restrict__ hist, const OrderState* state, int p,
                                    int limit) {
  __shared__ u64 s_wave[kOrdBlock / 64];
  __shared__ OrderState s_out;
  OrderState in = {0ull, (u64)limit, 0ull, 0ull};
  if (p > 1) in = state[p - 1];
  if (in.all) return in;   // uniform
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const u64 v = hist[(p - 1) * 256 + tid];
  u64 x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const u64 y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_wave[w] = x;
  if (tid == 0) s_out = OrderState{~0ull, in.need, 1ull, 0ull};   // need > the bins' total
  __syncthreads();
  u64 base = 0;
  for (int i = 0; i < w; ++i) base += s_wave[i];
  const u64 incl = base + x, excl = incl - v;
  if (excl < in.need && in.need <= incl)   // at most one thread
    s_out = OrderState{(in.prefix << 8) | (u64)tid, in.need - excl, 0ull, 0ull};
  __syncthreads();
  const OrderState out = s_out;
  __syncthreads();   // s_out may be written again by a later call
  return out;
}

// hist: [kOrdPasses][256] counters, zero at the call's start; state: [kOrdPasses + 1]
__global__ __launch_bounds__(kOrdBlock) void order_hist_kernel(OrderArgs a, int p, int limit,
                                                               u64* __restrict__ hist,
                                                               OrderState* state) {
  __shared__ uint32_t s_h[256];
  const int tid = threadIdx.x;
  OrderState st = {0ull, (u64)limit, 0ull, 0ull};
  if (p > 0) {
    st = order_resolve(hist, state, p, limit);
    if (blockIdx.x == 0 && tid == 0) state[p] = st;
    if (st.all) return;
  }
  s_h[tid] = 0u;
  __syncthreads();
  const int shift = 56 - 8 * p;
  const int64_t step = (int64_t)gridDim.x * kOrdRows;
  for (int64_t base = (int64_t)blockIdx.x * kOrdRows; base < a.count; base += step) {
    bool e[4];
    int64_t k[4];
    u64 u[4];
    order_load(a, base + tid * 4, e, k, u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = e[j] && (p == 0 || ((u[j] >> shift) >> 8) == st.prefix);
      hist_add(s_h, in, (uint32_t)(u[j] >> shift) & 255u);
    }
  }
  __syncthreads();
  if (s_h[tid]) atomicAdd(&hist[p * 256 + tid], (u64)s_h[tid]);
}

// a row of the list for sure (rank below the threshold; every eligible row when `all`) / a row of
// the threshold's rank
__device__ __forceinline__ void order_classes(const OrderState& st, const bool (&e)[4],
                                              const u64 (&u)[4], bool (&fl)[4], bool (&fe)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fl[j] = e[j] && (st.all || u[j] < st.prefix);
    fe[j] = e[j] && !st.all && u[j] == st.prefix;
  }
}

__global__ __launch_bounds__(kOrdBlock) void order_count_kernel(
    OrderArgs a, int limit, const u64* __restrict__ hist, OrderState* state,
    int64_t* __restrict__ less, int64_t* __restrict__ eq) {
  __shared__ int wsum[2][kOrdBlock / 64];
  const int tid = threadIdx.x;
  const OrderState st = order_resolve(hist, state, kOrdPasses, limit);
  if (blockIdx.x == 0 && tid == 0) state[kOrdPasses] = st;
  int cl = 0, ce = 0;   // wave-uniform
  for (int it = 0; it < kSelIters; ++it) {
    const int64_t r = (int64_t)blockIdx.x * kSelChunk + it * (kOrdBlock * 4) + tid * 4;
    bool e[4], fl[4], fe[4];
    int64_t k[4];
    u64 u[4];
    order_load(a, r, e, k, u);
    order_classes(st, e, u, fl, fe);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cl += __popcll(__ballot(fl[j]));
      ce += __popcll(__ballot(fe[j]));
    }
  }
  if ((tid & 63) == 0) {
    wsum[0][tid >> 6] = cl;
    wsum[1][tid >> 6] = ce;
  }
  __syncthreads();
  if (tid < 2) {
    int s = 0;
    for (int w = 0; w < kOrdBlock / 64; ++w) s += wsum[tid][w];
    (tid == 0 ? less : eq)[blockIdx.x] = s;
  }
}

// less / eq [nb] -> exclusive prefix sums in place; tot[0] = the rows of rank below the
// threshold; out_n[0] = entries the call writes, out_n[1] = eligible rows (pass 0's counters)
__global__ __launch_bounds__(kSelScanBlock) void order_scan_kernel(
    int64_t* __restrict__ less, int64_t* __restrict__ eq, int nb, const u64* __restrict__ hist,
    const OrderState* __restrict__ state, int64_t* __restrict__ tot,
    int64_t* __restrict__ out_n) {
  __shared__ u64 s_el[256 / 64];
  const int tid = threadIdx.x;
  const int64_t nl = scan_chunks(less, nb);
  const int64_t ne = scan_chunks(eq, nb);
  if (tid < 256) {
    u64 x = hist[tid];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    if ((tid & 63) == 0) s_el[tid >> 6] = x;
  }
  __syncthreads();
  if (tid == 0) {
    const OrderState st = state[kOrdPasses];
    const int64_t take = st.all ? 0 : (ne < (int64_t)st.need ? ne : (int64_t)st.need);
    tot[0] = nl;
    out_n[0] = nl + take;
    out_n[1] = (int64_t)(s_el[0] + s_el[1] + s_el[2] + s_el[3]);
  }
}

// out_keys / out_rows [limit]: nothing at or past `limit` is written
__global__ __launch_bounds__(kOrdBlock) void order_emit_kernel(
    OrderArgs a, int limit, const OrderState* __restrict__ state,
    const int64_t* __restrict__ less_off, const int64_t* __restrict__ eq_off,
    const int64_t* __restrict__ tot, int64_t* __restrict__ out_keys,
    int64_t* __restrict__ out_rows) {
  __shared__ int wcnt[2][kOrdBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const OrderState st = state[kOrdPasses];
  int64_t bl = less_off[blockIdx.x];
  int64_t be = tot[0] + eq_off[blockIdx.x];
  const u64 below = (1ull << lane) - 1ull;
  for (int it = 0; it < kSelIters; ++it) {
    const int64_t r = (int64_t)blockIdx.x * kSelChunk + it * (kOrdBlock * 4) + tid * 4;
    bool e[4], fl[4], fe[4];
    int64_t k[4];
    u64 u[4];
    order_load(a, r, e, k, u);
    order_classes(st, e, u, fl, fe);
    int pl = 0, pe = 0, wl = 0, we = 0;   // lanes own rows in order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u64 b0 = __ballot(fl[j]), b1 = __ballot(fe[j]);
      pl += __popcll(b0 & below);
      wl += __popcll(b0);
      pe += __popcll(b1 & below);
      we += __popcll(b1);
    }
    if (lane == 0) {
      wcnt[0][w] = wl;
      wcnt[1][w] = we;
    }
    __syncthreads();
    int basel = 0, totl = 0, basee = 0, tote = 0;
    for (int i = 0; i < kOrdBlock / 64; ++i) {
      const int tl = wcnt[0][i], te = wcnt[1][i];
      if (i < w) {
        basel += tl;
        basee += te;
      }
      totl += tl;
      tote += te;
    }
    int64_t posl = bl + basel + pl, pose = be + basee + pe;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (fl[j]) {
        if (posl < limit) {
          out_keys[posl] = k[j];
          out_rows[posl] = r + j;
        }
        ++posl;
      }
      if (fe[j]) {
        if (pose < limit) {   // the first `need` rows of the threshold's rank, in row order
          out_keys[pose] = k[j];
          out_rows[pose] = r + j;
        }
        ++pose;
      }
    }
    bl += totl;
    be += tote;
    __syncthreads();
  }
}

// The first n = out_n[0] pairs sorted by (rank, row) in LDS (bitonic over n2 slots, n2 the power
// of two at or above `limit`; 16 n2 bytes of dynamic LDS); entries n .. limit - 1 become
// (RAG_KEY_ABSENT, -1). One workgroup.
__global__ __launch_bounds__(kOrdSortBlock) void order_sort_kernel(
    int64_t* __restrict__ keys, int64_t* __restrict__ rows, const int64_t* __restrict__ out_n,
    int limit, int n2, uint32_t desc) {
  extern __shared__ u64 s_rank[];
  int64_t* const s_row = reinterpret_cast<int64_t*>(s_rank + n2);
  const int tid = threadIdx.x;
  const int64_t n_all = out_n[0];
  const int n = (int)(n_all < limit ? n_all : limit);
  for (int i = tid; i < n2; i += kOrdSortBlock) {
    s_rank[i] = i < n ? order_rank(keys[i], desc) : ~0ull;
    s_row[i] = i < n ? rows[i] : INT64_MAX;   // padding sorts behind every pair
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < n2 / 2; t += kOrdSortBlock) {   // one thread per compared pair
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), o = i | j;
        const u64 ua = s_rank[i], ub = s_rank[o];
        const int64_t ra = s_row[i], rb = s_row[o];
        const bool gt = ua > ub || (ua == ub && ra > rb);
        if (gt == ((i & k) == 0)) {
          s_rank[i] = ub;
          s_rank[o] = ua;
          s_row[i] = rb;
          s_row[o] = ra;
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < limit; i += kOrdSortBlock) {
    keys[i] = i < n ? order_key(s_rank[i], desc) : RAG_KEY_ABSENT;
    rows[i] = i < n ? s_row[i] : -1;
  }
}

// ----------------------------------------------------------------------------------------
// facet_counts: out[c] = eligible rows whose code of one tag field, (tag >> shift) & 0xFFFF, is
// c, for c <= n_codes; a stored code above n_codes is not counted and indexes nothing. A row is
// eligible when r < count and bit 0 of view[r] is set (view == nullptr: every row). `out` is
// zero when the kernel starts.
//   LDS_BINS   n_codes + 1 <= kFacetLdsBins: the bins live in LDS (4 (n_codes + 1) bytes of
//              dynamic LDS) and a workgroup adds its non-zero bins to `out` once, at its end
//   otherwise  every count goes to `out` directly
// Both are exact integer sums, whatever order the adds arrive in.
// ----------------------------------------------------------------------------------------
constexpr int kFacetBlock = 256;
constexpr int kFacetIters = 4;
constexpr int kFacetChunk = kFacetBlock * 4 * kFacetIters;   // rows per workgroup step
constexpr int kFacetWgPerCu = 2;   // fewer workgroups, fewer flushes of the same bins
constexpr int kFacetLdsBins = 8192;

template <bool LDS_BINS>
__global__ __launch_bounds__(kFacetBlock) void facet_kernel(
    const uint32_t* __restrict__ tags, const uint32_t* __restrict__ view, int64_t count,
    uint32_t shift, uint32_t n_codes, u64* __restrict__ out) {
  extern __shared__ uint32_t s_bins[];
  const int tid = threadIdx.x;
  if (LDS_BINS) {
    for (uint32_t i = tid; i <= n_codes; i += kFacetBlock) s_bins[i] = 0u;
    __syncthreads();
  }
  const int64_t step = (int64_t)gridDim.x * kFacetChunk;
  for (int64_t base = (int64_t)blockIdx.x * kFacetChunk; base < count; base += step) {
    uint4 t4[kFacetIters], v4[kFacetIters];
#pragma unroll
    for (int it = 0; it < kFacetIters; ++it) {
      const int64_t r = base + it * (kFacetBlock * 4) + tid * 4;
      t4[it] = make_uint4(0u, 0u, 0u, 0u);
      v4[it] = make_uint4(1u, 1u, 1u, 1u);
      if (r < count) {
        t4[it] = *reinterpret_cast<const uint4*>(tags + r);
        if (view) v4[it] = *reinterpret_cast<const uint4*>(view + r);
      }
    }
#pragma unroll
    for (int it = 0; it < kFacetIters; ++it) {
      const int64_t r = base + it * (kFacetBlock * 4) + tid * 4;
      const uint32_t t[4] = {t4[it].x, t4[it].y, t4[it].z, t4[it].w};
      const uint32_t v[4] = {v4[it].x, v4[it].y, v4[it].z, v4[it].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t c = (t[j] >> shift) & 0xFFFFu;
        const bool e = r + j < count && (v[j] & 1u) && c <= n_codes;
        if (LDS_BINS)
          hist_add(s_bins, e, c);
        else
          hist_add(out, e, c);
      }
    }
  }
  if (LDS_BINS) {
    __syncthreads();
    for (uint32_t i = tid; i <= n_codes; i += kFacetBlock)
      if (s_bins[i]) atomicAdd(&out[i], (u64)s_bins[i]);
  }
}

}  // namespace ragmi
