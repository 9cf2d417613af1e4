// scan_kernels.hip — the streaming pass of a search: every stored tile MFMA-scored against
// the pass's queries, each wave keeping its own top-32 per query (included by index_search.hip
// after prep_kernels.hip, which defines the tile16 layout).
//
// Three top-k structures and the kernel each serves: ScanTopK / scan_kernel (D = 384, query
// fragments in VGPRs, pending candidates in LDS), RegTopK / scan_lds_kernel (D = 1024, query
// fragments in LDS, pending in VGPRs), WideTopK / scan_wide_kernel (D = 1024, one query tile
// per wave), plus the int8 prescan on ScanTopK (scan_kernel_i8: D = 384, both int8 query planes
// in VGPRs, rows ranked by an upper bound of their exact score) and the VALU ablation of the scan. The tile helpers the later passes share
// (tile_mfma, tile_rsrc, tile_load, tile_sequence) live here, next to their first user.
namespace ragmi {

typedef _Float16 half2v __attribute__((ext_vector_type(2)));
constexpr int kKS = 32;           // candidates kept per (wave, query)
constexpr int kP = 8;             // pending slots per (lane, query tile)
constexpr int kWavesPerWG = 4;
constexpr int kScanBlock = 64 * kWavesPerWG;   // scan_kernel / rescan_kernel block (launch_fixed)
constexpr int kMaxLists = 2048;   // max scan waves (= per-wave lists) per pass
constexpr int kLdsPerWave = 4096; // dwords: keep_s[32][32] keep_i[32][32] pend_s[2][8][64] pend_i[2][8][64]
constexpr int kTileQStride = 16;  // ints between the 8 per-XCD tile-queue heads (64 B apart)
constexpr int kDynChunk = 2;      // tiles per dequeue of the dynamic scan schedule

// ----------------------------------------------------------------------------------------
// scan: each wave streams a contiguous range of tiles, MFMA-scores them against the 32
// queries, and keeps its own top-32 per query.
//
// Per tile and query tile qt the accumulator gives lane l the scores of query 16qt+(l&15)
// for rows 16t + 4(l>>4) + {0..3}. Top-k bookkeeping per wave:
//   thr_qt (VGPR)  current 32nd-best score of the lane's query (-inf until 32 are known)
//   pending        lane-private LDS slots [qt][slot][lane] for scores > thr
//   keep           LDS [32 queries][32] sorted best-first
// A query whose lanes hold > kP-4 pending entries is flushed: its 32 kept + 4x8 pending
// entries are bitonic-sorted across the wave and the best 32 kept (thr := 32nd). Rows are
// visited in increasing order per wave, so a later row never beats an equal-scored earlier
// one and the strict `> thr` filter is exact for the (score desc, row asc) order.
// ----------------------------------------------------------------------------------------
struct WaveTopK {
  float* keep_s;
  int* keep_i;
  float* pend_s;
  int* pend_i;
};

__device__ __forceinline__ void lds_fence() {
  // LDS ops of one wave complete in order; this stops the compiler from reordering
  // the cross-lane LDS traffic around the flush.
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

__device__ __forceinline__ void flush_query(const WaveTopK& w, int q, int lane, float& thr0,
                                            int& cnt0, float& thr1, int& cnt1) {
  const int qt = q >> 4, c = q & 15;
  float s;
  int id;
  int pidx = 0;
  if (lane < 32) {
    s = w.keep_s[q * kKS + lane];
    id = w.keep_i[q * kKS + lane];
  } else {
    const int pl = lane - 32;
    const int src = c + 16 * (pl >> 3);
    const int slot = pl & 7;
    pidx = (qt * kP + slot) * 64 + src;
    s = w.pend_s[pidx];
    id = w.pend_i[pidx];
  }
  lds_fence();
  bitonic_sort64(s, id, lane);
  if (lane < 32) {
    w.keep_s[q * kKS + lane] = s;
    w.keep_i[q * kKS + lane] = id;
  } else {
    w.pend_s[pidx] = kNegInf;
    w.pend_i[pidx] = kIdNone32;
  }
  lds_fence();
  const float nt = __shfl(s, 31, 64);
  // value selects, not a branch on qt: a qt-dependent choice between the thr0/thr1 (cnt0/cnt1)
  // references becomes a select of pointers into the caller's state, which keeps that state
  // in memory (promoted to LDS: a ds_read + lgkmcnt wait on every tile of the scan)
  const bool mine = (lane & 15) == c;
  const bool m0 = mine && qt == 0, m1 = mine && qt != 0;
  thr0 = m0 ? fmaxf(thr0, nt) : thr0;
  cnt0 = m0 ? 0 : cnt0;
  thr1 = m1 ? fmaxf(thr1, nt) : thr1;
  cnt1 = m1 ? 0 : cnt1;
}

__device__ __forceinline__ void flush_mask(const WaveTopK& w, uint64_t b, int qt, int lane,
                                           float& thr0, int& cnt0, float& thr1, int& cnt1) {
  uint32_t m = (uint32_t)((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xffffu);
  while (m) {
    const int c = __builtin_ctz(m);
    m &= m - 1;
    flush_query(w, qt * 16 + c, lane, thr0, cnt0, thr1, cnt1);
  }
}

// Per-wave top-k state of a scan (shared by the VGPR-query and LDS-query scan kernels).
struct ScanTopK {
  WaveTopK w;
  float thr0, thr1;
  int cnt0, cnt1;
  uint32_t fm0, fv0, fm1, fv1;
};

template <bool FILTER>
__device__ __forceinline__ void topk_init(ScanTopK& st, int* lds, int wid, int lane,
                                          const float* __restrict__ seed_thr,
                                          const uint32_t* __restrict__ filt) {
  st.w.keep_s = reinterpret_cast<float*>(lds + wid * kLdsPerWave);
  st.w.keep_i = lds + wid * kLdsPerWave + 1024;
  st.w.pend_s = reinterpret_cast<float*>(lds + wid * kLdsPerWave + 2048);
  st.w.pend_i = lds + wid * kLdsPerWave + 3072;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    st.w.keep_s[lane + 64 * j] = kNegInf;
    st.w.keep_i[lane + 64 * j] = kIdNone32;
    st.w.pend_s[lane + 64 * j] = kNegInf;
    st.w.pend_i[lane + 64 * j] = kIdNone32;
  }
  lds_fence();
  // Seed thresholds: seed_thr[q] is a lower bound of the global 32nd-best score (32 rows
  // scoring >= it exist, sample_kernel), so rows scoring below it can never be in the top-32.
  // `> pred(T)` == `>= T`; thresholds only ever rise.
  st.thr0 = kNegInf;
  st.thr1 = kNegInf;
  if (seed_thr) {
    const float T0 = seed_thr[lane & 15], T1 = seed_thr[16 + (lane & 15)];
    st.thr0 = T0 == kNegInf ? kNegInf : nextafterf(T0, kNegInf);
    st.thr1 = T1 == kNegInf ? kNegInf : nextafterf(T1, kNegInf);
  }
  st.cnt0 = 0;
  st.cnt1 = 0;
  st.fm0 = st.fv0 = st.fm1 = st.fv1 = 0;
  if constexpr (FILTER) {
    st.fm0 = filt[2 * (lane & 15)];
    st.fv0 = filt[2 * (lane & 15) + 1];
    st.fm1 = filt[2 * (16 + (lane & 15))];
    st.fv1 = filt[2 * (16 + (lane & 15)) + 1];
  }
}

// Scores of tile t (acc0: queries 0-15, acc1: 16-31; lane rows 16t + 4(l>>4) + r) -> pending
// entries above the thresholds, flushing queries whose lanes run out of pending slots.
// The tile's tags (FILTER: rows rbase .. rbase + 3 of lane group lane >> 4) come in `tg`,
// loaded by the caller together with the tile's vectors (scan_kernel) or just before
// (topk_tile below).
template <bool FILTER>
__device__ __forceinline__ void topk_tile_tg(ScanTopK& st, const floatx4& acc0,
                                             const floatx4& acc1, int t, int n_rows,
                                             const uint4& tg, int lane) {
  const int rbase = t * kTileRows + 4 * (lane >> 4);
  // every tile but the shard's last is full: no per-row bound check there (wave-uniform)
  const bool full = (t + 1) * kTileRows <= n_rows;
  float v0[4], v1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool ok = full || (rbase + r) < n_rows;
    bool ok0 = ok, ok1 = ok;
    if constexpr (FILTER) {
      const uint32_t tr = r == 0 ? tg.x : r == 1 ? tg.y : r == 2 ? tg.z : tg.w;
      ok0 = ok0 && ((tr & st.fm0) == st.fv0);
      ok1 = ok1 && ((tr & st.fm1) == st.fv1);
    }
    v0[r] = ok0 ? acc0[r] : kNegInf;
    v1[r] = ok1 ? acc1[r] : kNegInf;
  }
  const float m0 = fmax_nc(fmax_nc(v0[0], v0[1]), fmax_nc(v0[2], v0[3]));
  const float m1 = fmax_nc(fmax_nc(v1[0], v1[1]), fmax_nc(v1[2], v1[3]));
  if (__ballot((m0 > st.thr0) || (m1 > st.thr1))) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (v0[r] > st.thr0) {
        st.w.pend_s[st.cnt0 * 64 + lane] = v0[r];
        st.w.pend_i[st.cnt0 * 64 + lane] = rbase + r;
        ++st.cnt0;
      }
      if (v1[r] > st.thr1) {
        st.w.pend_s[(kP + st.cnt1) * 64 + lane] = v1[r];
        st.w.pend_i[(kP + st.cnt1) * 64 + lane] = rbase + r;
        ++st.cnt1;
      }
    }
    lds_fence();
    const uint64_t b0 = __ballot(st.cnt0 > kP - 4);
    const uint64_t b1 = __ballot(st.cnt1 > kP - 4);
    if (b0) flush_mask(st.w, b0, 0, lane, st.thr0, st.cnt0, st.thr1, st.cnt1);
    if (b1) flush_mask(st.w, b1, 1, lane, st.thr0, st.cnt0, st.thr1, st.cnt1);
  }
}

template <bool FILTER>
__device__ __forceinline__ void topk_tile(ScanTopK& st, const floatx4& acc0, const floatx4& acc1,
                                          int t, int n_rows, const uint32_t* __restrict__ tags,
                                          int lane) {
  uint4 tg = {0u, 0u, 0u, 0u};
  if constexpr (FILTER)
    tg = *reinterpret_cast<const uint4*>(tags + t * kTileRows + 4 * (lane >> 4));
  topk_tile_tg<FILTER>(st, acc0, acc1, t, n_rows, tg, lane);
}

// One pass of the end-of-scan sort of pending-only queries: 64 / W queries at once, one per
// W-lane block. The lane's query is q (-1: none) and j its position in the block; the block
// gathers slots 0 .. W/4 - 1 of the query's four lanes, sorts them and writes the head of the
// keep list.
template <int W>
__device__ __forceinline__ void sort_pending(const WaveTopK& w, int q, int j, int lane) {
  constexpr int SH = W == 8 ? 1 : W == 16 ? 2 : 3;   // log2 of the slots per lane
  float s = kNegInf;
  int id = kIdNone32;
  if (q >= 0) {
    const int pidx = (((q >> 4) * kP + (j & ((1 << SH) - 1))) * 64) + (q & 15) + 16 * (j >> SH);
    s = w.pend_s[pidx];
    id = w.pend_i[pidx];
  }
  lds_fence();
  if constexpr (W == 8) bitonic_sort8x8(s, id, lane);
  else if constexpr (W == 16) bitonic_sort16x4(s, id, lane);
  else bitonic_sort32x2(s, id, lane);
  if (q >= 0) {
    w.keep_s[q * kKS + j] = s;
    w.keep_i[q * kKS + j] = id;
  }
  lds_fence();
}

// A wave's NQ keep lists (LDS, [NQ][32] best-first) at the end of its scan -> list l of the
// pass's nw per query: the finite entries to ps / pi ([NQ][32]), and for query q0 + c its head
// and its length.
template <int NQ>
__device__ __forceinline__ void write_lists(const float* keep_s, const int* keep_i, int lane,
                                            int q0, int l, int nw, float* __restrict__ ps,
                                            int* __restrict__ pi, float* __restrict__ heads_s,
                                            int* __restrict__ heads_i, int* __restrict__ heads_n) {
#pragma unroll
  for (int j = 0; j < NQ / 2; ++j) {
    const float v = keep_s[lane + 64 * j];
    if (v != kNegInf) {
      ps[lane + 64 * j] = v;
      pi[lane + 64 * j] = keep_i[lane + 64 * j];
    }
  }
  if (lane < NQ) {
    int n = 0;
    for (int j = 0; j < kKS; ++j) n += keep_s[lane * kKS + j] != kNegInf;
    const int q = q0 + lane;
    heads_s[q * nw + l] = keep_s[lane * kKS];
    heads_i[q * nw + l] = n > 0 ? keep_i[lane * kKS] : kIdNone32;
    heads_n[q * nw + l] = n;
  }
}

// End of scan: flush what is pending and write this wave's sorted list (finite entries), its
// head and its length per query.
// SORT: 2 = pending-only queries sorted eight per pass in 8-lane blocks when each of their
// lanes holds <= 2 entries, else four per pass in 16-lane blocks (production: after a tile's
// flush check no lane holds more than kP - 4 = 4 pending entries of a query, so slots 4..7 are
// empty and a query has at most 16 entries), 1 = two per pass in 32-lane blocks (the round-1
// path, A/B), 0 = not sorted (timing probe, results invalid)
template <int SORT = 2>
__device__ __forceinline__ void topk_finish(ScanTopK& st, int lane, int gw, int nw,
                                            float* __restrict__ part_s, int* __restrict__ part_i,
                                            float* __restrict__ heads_s,
                                            int* __restrict__ heads_i, int* __restrict__ heads_n) {
  WaveTopK& w = st.w;
  // With seeded thresholds most queries never flushed during the scan: their keep list is
  // empty and their <= 32 pending entries (4 lanes x 8 slots) only need a 32-wide sort, two
  // queries per pass. Queries with a non-empty keep list take flush_query.
  {
    const uint64_t b0 = __ballot(st.cnt0 > 0);
    const uint64_t b1 = __ballot(st.cnt1 > 0);
    const uint32_t p0 = (uint32_t)((b0 | (b0 >> 16) | (b0 >> 32) | (b0 >> 48)) & 0xffffu);
    const uint32_t p1 = (uint32_t)((b1 | (b1 >> 16) | (b1 >> 32) | (b1 >> 48)) & 0xffffu);
    const uint32_t pend = p0 | (p1 << 16);
    const uint32_t kept =
        (uint32_t)__ballot(lane < kQ && w.keep_s[(lane & 31) * kKS] != kNegInf);
    uint32_t full = pend & kept;
    uint32_t only = pend & ~kept;
    while (full) {
      const int q = __builtin_ctz(full);
      full &= full - 1;
      flush_query(w, q, lane, st.thr0, st.cnt0, st.thr1, st.cnt1);
    }
    if (SORT == 0) only = 0;
    if (SORT == 2) {
      // queries whose four lanes hold <= 2 pending entries each (<= 8 in all): eight per pass
      // in 8-lane blocks, slots 0..1 of lanes c + 16 g (the common case: ~2 entries per query
      // and wave at the 8-GPU shard size); the rest take the 16-lane pass below
      const uint64_t g0 = __ballot(st.cnt0 > 2), g1 = __ballot(st.cnt1 > 2);
      const uint32_t big = (uint32_t)((g0 | (g0 >> 16) | (g0 >> 32) | (g0 >> 48)) & 0xffffu) |
                           ((uint32_t)((g1 | (g1 >> 16) | (g1 >> 32) | (g1 >> 48)) & 0xffffu) << 16);
      uint32_t small = only & ~big;
      only &= big;
      while (small) {
        int qv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          qv[t] = small ? __builtin_ctz(small) : -1;
          if (small) small &= small - 1;
        }
        const int sub = lane >> 3, j = lane & 7;
        int q = qv[0];
#pragma unroll
        for (int t = 1; t < 8; ++t) q = sub == t ? qv[t] : q;
        sort_pending<8>(w, q, j, lane);
      }
    }
    while (SORT == 2 && only) {
      int qv[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        qv[t] = only ? __builtin_ctz(only) : -1;
        if (only) only &= only - 1;
      }
      const int sub = lane >> 4, j = lane & 15;
      const int q = sub == 0 ? qv[0] : sub == 1 ? qv[1] : sub == 2 ? qv[2] : qv[3];
      sort_pending<16>(w, q, j, lane);
    }
    while (SORT == 1 && only) {
      const int qa = __builtin_ctz(only);
      only &= only - 1;
      const int qb = only ? __builtin_ctz(only) : -1;
      if (only) only &= only - 1;
      sort_pending<32>(w, lane < 32 ? qa : qb, lane & 31, lane);
    }
  }
  write_lists<kQ>(w.keep_s, w.keep_i, lane, 0, gw, nw, part_s + (int64_t)gw * (kQ * kKS),
                  part_i + (int64_t)gw * (kQ * kKS), heads_s, heads_i, heads_n);
}

// Tile product: N k-steps of one tile (a: A-fragments) against the two query tiles (b0:
// queries 0-15, b1: 16-31), accumulated in k-step order, the two chains interleaved.
template <int N>
__device__ __forceinline__ void tile_mfma(const half8 (&a)[N], const half8 (&b0)[N],
                                          const half8 (&b1)[N], floatx4& acc0, floatx4& acc1) {
#pragma unroll
  for (int s = 0; s < N; ++s) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b0[s], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b1[s], acc1, 0, 0, 0);
  }
}

// Buffer descriptor over `bytes` bytes at p (wave-uniform): raw, unstrided, offsets checked
// against `bytes`. The flags word is the descriptor's last dword: DATA_FORMAT = 32 (bits
// 15-18 = 4; a descriptor with format 0 is invalid on gfx9), every other field 0 — no swizzle,
// no index stride, no typed conversion.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// N consecutive k-steps (1 KiB each, lane l's half8 at voff = 16 l) from tp (wave-uniform),
// as buffer loads off one descriptor: the address lives in SGPRs and the per-lane part is one
// VGPR, so no 64-bit address VGPRs are live across a scan loop (their reuse as load
// destinations forced a vmcnt(0) at the loop head). NT: non-temporal.
template <int N, bool NT>
__device__ __forceinline__ void tile_load(half8 (&a)[N], const char* tp, int voff) {
  const __amdgpu_buffer_rsrc_t rs = tile_rsrc(tp, N * 1024);
#pragma unroll
  for (int s = 0; s < N; ++s) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, s * 1024, NT ? 2 : 0);
    a[s] = __builtin_bit_cast(half8, v);
  }
}

// Tile sequence of wave gw of nw: t_j = t_first + j * t_step, j < n_mine (always increasing,
// which the strict `> thr` tie rule relies on). STRIDED: t = gw, gw + nw, ... (the chip sweeps
// one window of the corpus at a time); else contiguous ranges.
template <bool STRIDED>
__device__ __forceinline__ void tile_sequence(int gw, int nw, int n_tiles, int& t_first,
                                              int& t_step, int& n_mine) {
  if constexpr (STRIDED) {
    t_first = gw;
    t_step = nw;
    n_mine = gw < n_tiles ? (n_tiles - 1 - gw) / nw + 1 : 0;
  } else {
    t_first = (int)((int64_t)n_tiles * gw / nw);
    t_step = 1;
    n_mine = (int)((int64_t)n_tiles * (gw + 1) / nw) - t_first;
  }
}

// Variant knobs (A/B'd by rag_bench_scan; the production instance is scan_kernel<D, F>):
//   MODE 0 full scan + top-k; 1 MFMA only (running max, no top-k); 2 loads only; 3 full scan
//        without the end-of-scan sort of pending-only queries (timing probe, results invalid);
//        4 full scan with the round-1 end-of-scan sort (two queries per 32-lane pass, A/B)
//   STRIDED tile order gw, gw+nw, ... (the chip sweeps one window) vs contiguous ranges
//   NT non-temporal corpus loads (the corpus is read once per search; MI355X_MICROARCH
//      'nt-weights': once-read streams)
//   SB sched_barrier after each tile's load batch, so the scheduler cannot sink the next
//      tile's loads below the current tile's wait (which leaves one tile in flight)
//   DYN > 0 (diagnostic, rag_bench_scan variants 9-12; round 2): dynamic tile queue instead
//      of the static interleave — waves dequeue chunks of DYN tiles from per-XCD heads (tileq,
//      zeroed before each launch): head x hands out chunks x, x + 8, x + 16, ... in increasing
//      order, so every wave still visits increasing rows (the strict `> thr` tie rule). The
//      next chunk's dequeue is issued when a chunk starts. Measured and dropped
//      (profiles/r02_scan_dyn.jsonl): loads-only 0.142 -> 0.180 ms at 1.25M rows, 1.099 ->
//      1.356 ms at 10M; production 15-20% slower with chunks of 2 or 4, 48% with 1. The
//      returning atomic sits in the wave's in-order vmcnt queue, so every later tile load of
//      the wave waits out its ~2-3 us fabric round trip: each dequeue stalls the wave's stream.
// Query B-operands live in VGPRs (2 x D/32 half8 per lane): the D = 384 production kernel.
template <int D, bool FILTER, int MODE = 0, bool STRIDED = true, bool NT = true, bool SB = true,
          int DYN = 0>
__global__ __launch_bounds__(kScanBlock, 2) void scan_kernel(
    const half8* __restrict__ corpus, const uint32_t* __restrict__ tags,
    const uint32_t* __restrict__ filt, const half8* __restrict__ qfrag, int n_rows, int n_tiles,
    const float* __restrict__ seed_thr, float* __restrict__ part_s, int* __restrict__ part_i,
    float* __restrict__ heads_s, int* __restrict__ heads_i, int* __restrict__ heads_n,
    int* __restrict__ tileq = nullptr) {
  constexpr int S = steps<D>();
  __shared__ int lds[kWavesPerWG * kLdsPerWave];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  ScanTopK st;
  topk_init<FILTER>(st, lds, wid, lane, seed_thr, filt);

  const int gw = blockIdx.x * kWavesPerWG + __builtin_amdgcn_readfirstlane(wid);
  const int nw = gridDim.x * kWavesPerWG;
  int t_first, t_step, n_mine;
  tile_sequence<STRIDED>(gw, nw, n_tiles, t_first, t_step, n_mine);

  half8 q0[S], q1[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    q0[s] = qfrag[s * 64 + lane];
    q1[s] = qfrag[(S + s) * 64 + lane];
  }

  float vmax = kNegInf;   // MODE 1/2: keeps the work alive
  // tg: the tile's tags (FILTER), loaded with its vectors (the static-interleave loop below);
  // the dynamic-queue diagnostic passes have_tg = false and loads them here
  auto process_v = [&](const half8(&a)[S], int t, const uint4& tg, bool have_tg)
      __attribute__((always_inline)) {
    if constexpr (MODE == 2) {
      half8 x = a[0];
#pragma unroll
      for (int s = 1; s < S; ++s) x += a[s];
      vmax = fmaxf(vmax, (float)(x[0] + x[1] + x[2] + x[3] + x[4] + x[5] + x[6] + x[7]));
    } else {
      floatx4 acc0 = {0.f, 0.f, 0.f, 0.f};
      floatx4 acc1 = {0.f, 0.f, 0.f, 0.f};
      tile_mfma<S>(a, q0, q1, acc0, acc1);
      if constexpr (MODE == 0 || MODE >= 3) {
        if (have_tg)
          topk_tile_tg<FILTER>(st, acc0, acc1, t, n_rows, tg, lane);
        else
          topk_tile<FILTER>(st, acc0, acc1, t, n_rows, tags, lane);
      } else
        vmax = fmaxf(vmax, fmaxf(fmaxf(fmaxf(acc0[0], acc0[1]), fmaxf(acc0[2], acc0[3])),
                                 fmaxf(fmaxf(acc1[0], acc1[1]), fmaxf(acc1[2], acc1[3]))));
    }
  };

  // One tile's load batch: its vectors (tile_load: buffer loads off a wave-uniform per-tile
  // descriptor) and, where the caller passes `tg` under FILTER, its 64 B of tags.
  const char* cbase = reinterpret_cast<const char*>(corpus);
  const int voff = lane * 16;
  auto load_t = [&](half8(&a)[S], int t_in, uint4* tg = nullptr) __attribute__((always_inline)) {
    const int t = __builtin_amdgcn_readfirstlane(t_in);
    tile_load<S, NT>(a, cbase + (int64_t)t * (S * 1024), voff);
    if constexpr (FILTER) {
      if (tg)
        *tg = __builtin_bit_cast(
            uint4, __builtin_amdgcn_raw_buffer_load_b128(
                       tile_rsrc(tags + (int64_t)t * kTileRows, kTileRows * 4), (lane >> 4) * 16,
                       0, 0));
    }
    if constexpr (SB) __builtin_amdgcn_sched_barrier(0);
  };
  if constexpr (DYN > 0) {
    const int xcd = blockIdx.x & 7;
    int* head = tileq + kTileQStride * xcd;
    // The head address is hidden behind an opaque zero offset: with a provably uniform address
    // the AMDGPU atomic optimizer rewrites the atomic into a wave-reduced one whose result is
    // consumed (readfirstlane) right after the issue, i.e. a vmcnt(0) wait on every dequeue.
    int zoff = 0;
    asm volatile("" : "+v"(zoff));
    auto deq = [&]() __attribute__((always_inline)) {
      int v = 0;
      if (lane == 0)
        v = __hip_atomic_fetch_add(head + zoff, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return v;   // lane 0's VGPR; read (readfirstlane) only when the chunk is needed
    };
    int pend = deq();
    int cb = 0, ce = 0;          // current chunk: tiles [cb, ce) (wave-uniform)
    // once the queue is empty every call returns -1 (at most two dequeues past the last chunk)
    auto next_tile = [&]() __attribute__((always_inline)) {
      if (cb >= ce) {
        cb = (8 * __builtin_amdgcn_readfirstlane(pend) + xcd) * DYN;
        ce = min(cb + DYN, n_tiles);
        pend = deq();
      }
      return cb < ce ? cb++ : -1;
    };
    half8 a0[S], a1[S];
    const uint4 tz = {0u, 0u, 0u, 0u};
    int t_cur = next_tile();
    if (t_cur >= 0) {
      load_t(a0, t_cur);
      while (true) {
        int t_nxt = next_tile();
        load_t(a1, t_nxt >= 0 ? t_nxt : t_cur);
        process_v(a0, t_cur, tz, false);
        if (t_nxt < 0) break;
        t_cur = t_nxt;
        t_nxt = next_tile();
        load_t(a0, t_nxt >= 0 ? t_nxt : t_cur);
        process_v(a1, t_cur, tz, false);
        if (t_nxt < 0) break;
        t_cur = t_nxt;
      }
    }
  } else if (n_mine > 0) {
    half8 a0[S], a1[S];
    // FILTER: the tile's 64 B of tags ride in the same load batch as its vectors. Loaded inside
    // topk_tile (after the next tile's loads were issued) the tag load was the youngest
    // vector-memory op, so waiting for it waited for the next tile's vectors too: one tile in
    // flight instead of two (filtered 10M line, round 3: 0.825 of the spec vs 0.88 unfiltered).
    uint4 tg0 = {0u, 0u, 0u, 0u}, tg1 = tg0;
    auto load = [&](half8(&a)[S], uint4& tg, int j) __attribute__((always_inline)) {
      load_t(a, t_first + j * t_step, &tg);
    };
    load(a0, tg0, 0);
    int j = 0;
    while (true) {
      load(a1, tg1, min(j + 1, n_mine - 1));
      process_v(a0, t_first + j * t_step, tg0, true);
      if (++j >= n_mine) break;
      load(a0, tg0, min(j + 1, n_mine - 1));
      process_v(a1, t_first + j * t_step, tg1, true);
      if (++j >= n_mine) break;
    }
  }
  if constexpr (MODE == 1 || MODE == 2) {
    if (vmax == 12345.0f) part_s[gw] = vmax;   // never true in practice; defeats DCE
    return;
  }
  topk_finish<MODE == 3 ? 0 : MODE == 4 ? 1 : 2>(st, lane, gw, nw, part_s, part_i, heads_s,
                                                 heads_i, heads_n);
}

// ----------------------------------------------------------------------------------------
// int8 prescan (D = 384, fp16 storage): the scan over the int8 copy of the corpus
// (prep_kernels.hip "int8 scan copy"), half the bytes of the fp16 scan. What enters the top-k
// is not an approximate score but the upper bound u(r, q) >= e(r, q) of u_bound, so a row
// outside the lists has e <= u <= the 32nd-best u, and select's certificate keeps its shape
// with a := u and a tiny eps (certify_kernels.hip). Same ScanTopK / topk_tile_tg / topk_finish
// and list format as scan_kernel.
// ----------------------------------------------------------------------------------------
// Per-lane constants of the int8 query batch: the planes' B-fragments of both query tiles and
// the u_bound parameters of the lane's two queries (16 qt + (lane & 15)).
template <int D>
struct Query8 {
  intx4 h0[steps8<D>()], l0[steps8<D>()], h1[steps8<D>()], l1[steps8<D>()];
  float sq0, A0, C0, sq1, A1, C1;
};

template <int D>
__device__ __forceinline__ void query8_load(Query8<D>& q, const intx4* __restrict__ qfrag8,
                                            const float* __restrict__ qp8, int lane) {
  constexpr int S = steps8<D>();
#pragma unroll
  for (int s = 0; s < S; ++s) {
    q.h0[s] = qfrag8[(0 * S + s) * 64 + lane];
    q.l0[s] = qfrag8[(1 * S + s) * 64 + lane];
    q.h1[s] = qfrag8[(2 * S + s) * 64 + lane];
    q.l1[s] = qfrag8[(3 * S + s) * 64 + lane];
  }
  const float4 p0 = *reinterpret_cast<const float4*>(qp8 + 4 * (lane & 15));
  const float4 p1 = *reinterpret_cast<const float4*>(qp8 + 4 * (16 + (lane & 15)));
  q.sq0 = p0.x; q.A0 = p0.y; q.C0 = p0.z;
  q.sq1 = p1.x; q.A1 = p1.y; q.C1 = p1.z;
}

// The integer dots I of one tile of a copy against both planes of the 32 queries, in the
// accumulator layout of tile_mfma (h0 / l0: queries 0-15, h1 / l1: 16-31)
struct Dots {
  intx4 h0, l0, h1, l1;
};

// ... and their upper bounds u in format Copy's form (sc / er: scales and errors of the lane's
// four C/D rows 4(lane >> 4) + r). The one place u is evaluated: the scans, the seed sample and
// rag_index_prescan_bounds all come here.
template <int D, typename Copy>
__device__ __forceinline__ void dots_u(const Dots& d, const Query8<D>& q, const float4& sc,
                                       const float4& er, floatx4& u0, floatx4& u1) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float s_r = r == 0 ? sc.x : r == 1 ? sc.y : r == 2 ? sc.z : sc.w;
    const float e_r = r == 0 ? er.x : r == 1 ? er.y : r == 2 ? er.z : er.w;
    u0[r] = Copy::bound(d.h0[r], d.l0[r], s_r, e_r, q.sq0, q.A0, q.C0);
    u1[r] = Copy::bound(d.h1[r], d.l1[r], s_r, e_r, q.sq1, q.A1, q.C1);
  }
}

// One int8 tile (a: its D/64 A-fragments) against the 32 queries -> the upper bounds u, in the
// accumulator layout of tile_mfma (u0: queries 0-15, u1: 16-31)
template <int D>
__device__ __forceinline__ void tile_u8(const intx4 (&a)[steps8<D>()], const Query8<D>& q,
                                        const float4& sc, const float4& er, floatx4& u0,
                                        floatx4& u1) {
  Dots d;
  d.h0 = d.l0 = d.h1 = d.l1 = intx4{0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < steps8<D>(); ++s) {
    d.h0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], q.h0[s], d.h0, 0, 0, 0);
    d.h1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], q.h1[s], d.h1, 0, 0, 0);
    d.l0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], q.l0[s], d.l0, 0, 0, 0);
    d.l1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], q.l1[s], d.l1, 0, 0, 0);
  }
  dots_u<D, Copy8>(d, q, sc, er, u0, u1);
}

// scales and errors of the lane's four C/D rows of tile t, by plain loads
__device__ __forceinline__ void tile_meta(const float* __restrict__ meta, int64_t t, int lane,
                                          float4& sc, float4& er) {
  sc = *reinterpret_cast<const float4*>(meta + t * 32 + 4 * (lane >> 4));
  er = *reinterpret_cast<const float4*>(meta + t * 32 + 16 + 4 * (lane >> 4));
}

// the int8 copy's tile t: its D/64 fragments by non-temporal loads, then tile_u8
template <int D>
__device__ __forceinline__ void Copy8::tile_u_at(const char* __restrict__ data,
                                                 const float* __restrict__ meta, int64_t t,
                                                 const Query8<D>& q, int lane, floatx4& u0,
                                                 floatx4& u1) {
  constexpr int S = steps8<D>();
  const intx4* tp = reinterpret_cast<const intx4*>(data) + t * (S * 64) + lane;
  intx4 a[S];
#pragma unroll
  for (int s = 0; s < S; ++s) a[s] = __builtin_nontemporal_load(tp + s * 64);
  float4 sc, er;
  tile_meta(meta, t, lane, sc, er);
  tile_u8<D>(a, q, sc, er, u0, u1);
}

// ---- what the two prescan kernels share; their pipelines are their own ----
// A wave's start: its top-k state, its place in the grid, its strided sequence of tile PAIRS
// (pairs p_first + j p_step, j < n_mine) and the query batch
struct PairWalk {
  int gw, nw, p_first, p_step, n_mine;
};

template <int D, bool FILTER>
__device__ __forceinline__ void prescan_start(ScanTopK& st, PairWalk& w, Query8<D>& q, int* lds,
                                              int wid, int lane, const float* __restrict__ seed_thr,
                                              const uint32_t* __restrict__ filt, int n_tiles,
                                              const intx4* __restrict__ qfrag8,
                                              const float* __restrict__ qp8) {
  topk_init<FILTER>(st, lds, wid, lane, seed_thr, filt);
  w.gw = blockIdx.x * kWavesPerWG + __builtin_amdgcn_readfirstlane(wid);
  w.nw = gridDim.x * kWavesPerWG;
  const int n_pairs = (n_tiles + 1) / 2;
  tile_sequence<true>(w.gw, w.nw, n_pairs, w.p_first, w.p_step, w.n_mine);
  query8_load<D>(q, qfrag8, qp8, lane);
}

// What rides in a pair's load batch beside its image: the scales and errors of the lane's four
// C/D rows of both tiles and, under FILTER, their tags. The tag column ends at n_tiles * 16
// rows, so the pair's tag descriptor is clipped there (out-of-range buffer loads return 0)
struct PairSide {
  float4 sc[2], er[2];
  uint4 tg[2];
};

template <bool FILTER>
__device__ __forceinline__ void pair_side_load(PairSide& b, const float* __restrict__ meta,
                                               const uint32_t* __restrict__ tags, int p,
                                               int n_tiles, int goff) {
  const __amdgpu_buffer_rsrc_t rm = tile_rsrc(meta + (int64_t)p * 64, 256);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    b.sc[u] = __builtin_bit_cast(float4,
                                 __builtin_amdgcn_raw_buffer_load_b128(rm, goff, u * 128, 0));
    b.er[u] = __builtin_bit_cast(
        float4, __builtin_amdgcn_raw_buffer_load_b128(rm, goff, u * 128 + 64, 0));
  }
  if constexpr (FILTER) {
    const int left = min(2, n_tiles - 2 * p);   // tiles of this pair the tag column holds
    const __amdgpu_buffer_rsrc_t rt =
        tile_rsrc(tags + (int64_t)p * (2 * kTileRows), left * kTileRows * 4);
#pragma unroll
    for (int u = 0; u < 2; ++u)
      b.tg[u] = __builtin_bit_cast(
          uint4, __builtin_amdgcn_raw_buffer_load_b128(rt, goff, u * (kTileRows * 4), 0));
  } else {
    b.tg[0] = b.tg[1] = uint4{0u, 0u, 0u, 0u};
  }
}

// MODE 1 (MFMA + bound only): the max of a tile's eight bounds of a lane keeps them alive ...
__device__ __forceinline__ float max8(const floatx4& u0, const floatx4& u1) {
  return fmaxf(fmaxf(fmaxf(u0[0], u0[1]), fmaxf(u0[2], u0[3])),
               fmaxf(fmaxf(u1[0], u1[1]), fmaxf(u1[2], u1[3])));
}
// ... and the store that is never taken in practice keeps the max: defeats DCE
__device__ __forceinline__ void keep_alive(float vmax, float* __restrict__ part_s, int gw) {
  if (vmax == 12345.0f) part_s[gw] = vmax;
}

// The scan walks PAIRS of tiles (32 rows, 12 KiB + 256 B of meta per load batch, two batches
// in flight): the same bytes in flight per wave as the fp16 scan's two 12 KiB tiles, which is
// what keeps HBM busy at one wave per SIMD. c8 / meta hold an even number of tiles (the index
// allocates one spare); the tag column ends at n_tiles * 16 rows, so the pair's tag
// descriptor is clipped there (out-of-range buffer loads return 0) and the rows of a spare
// tile fail topk_tile_tg's bound check.
// MODE as scan_kernel's: 0 production, 1 MFMA + bound only (no top-k), 2 loads only.
template <int D, bool FILTER, int MODE = 0>
__global__ __launch_bounds__(kScanBlock, 1) void scan_kernel_i8(
    const char* __restrict__ c8, const float* __restrict__ meta,
    const uint32_t* __restrict__ tags, const uint32_t* __restrict__ filt,
    const intx4* __restrict__ qfrag8, const float* __restrict__ qp8, int n_rows, int n_tiles,
    const float* __restrict__ seed_thr, float* __restrict__ part_s, int* __restrict__ part_i,
    float* __restrict__ heads_s, int* __restrict__ heads_i, int* __restrict__ heads_n) {
  constexpr int S = steps8<D>();
  __shared__ int lds[kWavesPerWG * kLdsPerWave];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  ScanTopK st;
  PairWalk pw;
  Query8<D> q;
  prescan_start<D, FILTER>(st, pw, q, lds, wid, lane, seed_thr, filt, n_tiles, qfrag8, qp8);
  const int gw = pw.gw, nw = pw.nw;
  const int p_first = pw.p_first, p_step = pw.p_step, n_mine = pw.n_mine;

  struct Batch {
    intx4 a[2][S];
    PairSide side;
  };
  const int voff = lane * 16, goff = (lane >> 4) * 16;
  auto load = [&](Batch& b, int j) __attribute__((always_inline)) {
    const int p = __builtin_amdgcn_readfirstlane(p_first + j * p_step);
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(c8 + (int64_t)p * (2 * S * 1024), 2 * S * 1024);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int s = 0; s < S; ++s)
        b.a[u][s] = __builtin_bit_cast(
            intx4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (u * S + s) * 1024, 2));
    pair_side_load<FILTER>(b.side, meta, tags, p, n_tiles, goff);
    __builtin_amdgcn_sched_barrier(0);
  };
  float vmax = kNegInf;   // MODE 1/2: keeps the work alive
  auto process = [&](const Batch& b, int j) __attribute__((always_inline)) {
    const int p = p_first + j * p_step;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if constexpr (MODE == 2) {
        intx4 x = b.a[u][0];
#pragma unroll
        for (int s = 1; s < S; ++s) x += b.a[u][s];
        vmax = fmaxf(vmax, (float)(x[0] + x[1] + x[2] + x[3]) + b.side.sc[u].x + b.side.er[u].x);
      } else {
        floatx4 u0, u1;
        tile_u8<D>(b.a[u], q, b.side.sc[u], b.side.er[u], u0, u1);
        if constexpr (MODE == 0)
          topk_tile_tg<FILTER>(st, u0, u1, 2 * p + u, n_rows, b.side.tg[u], lane);
        else
          vmax = fmaxf(vmax, max8(u0, u1));
      }
    }
  };
  if (n_mine > 0) {
    Batch b0, b1;
    load(b0, 0);
    int j = 0;
    while (true) {
      load(b1, min(j + 1, n_mine - 1));
      process(b0, j);
      if (++j >= n_mine) break;
      load(b0, min(j + 1, n_mine - 1));
      process(b1, j);
      if (++j >= n_mine) break;
    }
  }
  if constexpr (MODE != 0) {
    keep_alive(vmax, part_s, gw);
    return;
  }
  topk_finish<2>(st, lane, gw, nw, part_s, part_i, heads_s, heads_i, heads_n);
}

// ----------------------------------------------------------------------------------------
// 6-bit prescan (D = 384, fp16 storage, the largest shards): the scan over the 6-bit copy
// (prep_kernels.hip "6-bit scan copy"), 0.755 of the int8 scan's bytes. Same bound, same query
// planes, same lists; the A-fragments (bytes 4 v) are unpacked from the packed dwords
// (unpack6) and the stored scale is s_r / 4.
// ----------------------------------------------------------------------------------------
// The dots of one 6-bit tile (w: the lane's eighteen packed dwords of it,
// pair6_dword(u, s, c) - 18 u)
template <int D>
__device__ __forceinline__ void tile_dots6(const uint32_t (&w)[3 * steps8<D>()],
                                           const Query8<D>& q, Dots& d) {
  d.h0 = d.l0 = d.h1 = d.l1 = intx4{0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < steps8<D>(); ++s) {
    const intx4 a = unpack6(w[3 * s], w[3 * s + 1], w[3 * s + 2]);
    d.h0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, q.h0[s], d.h0, 0, 0, 0);
    d.h1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, q.h1[s], d.h1, 0, 0, 0);
    d.l0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, q.l0[s], d.l0, 0, 0, 0);
    d.l1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, q.l1[s], d.l1, 0, 0, 0);
  }
}

// the lane's 36 dwords of pair `pair` by non-temporal loads (seed sample, diagnostic bounds)
__device__ __forceinline__ void pair6_load(uint32_t (&w)[36], const char* __restrict__ c6,
                                           int64_t pair, int lane) {
  const intx4* pp = reinterpret_cast<const intx4*>(c6 + pair * kPair6Bytes) + lane;
#pragma unroll
  for (int L = 0; L < 9; ++L) {
    const intx4 x = __builtin_nontemporal_load(pp + L * 64);
#pragma unroll
    for (int j = 0; j < 4; ++j) w[4 * L + j] = (uint32_t)x[j];
  }
}

// the 6-bit copy's tile t: its pair (pair6_load), then the dots and bounds of its half
template <int D>
__device__ __forceinline__ void Copy6::tile_u_at(const char* __restrict__ data,
                                                 const float* __restrict__ meta, int64_t t,
                                                 const Query8<D>& q, int lane, floatx4& u0,
                                                 floatx4& u1) {
  static_assert(D == 384, "pair6 layout");
  uint32_t w[36], wt[18];
  pair6_load(w, data, t >> 1, lane);
#pragma unroll
  for (int g = 0; g < 18; ++g) wt[g] = (t & 1) ? w[18 + g] : w[g];
  float4 sc, er;
  tile_meta(meta, t, lane, sc, er);
  Dots d;
  tile_dots6<D>(wt, q, d);
  dots_u<D, Copy6>(d, q, sc, er, u0, u1);
}

// As scan_kernel_i8: strided pairs of tiles, one buffer descriptor per pair, the pair's meta
// and tags in the same load batch. A pair is 9 KiB (nine loads) + 256 B of meta; THREE batches
// are in flight per wave (27.8 KiB against the int8 scan's 24.5), the registers the narrower
// unit frees. c6 / meta hold whole pairs; the tag descriptor is clipped at n_tiles * 16 rows
// and the rows of a spare tile fail topk_tile_tg's bound check.
// The bound and the top-k check of a tile run ONE TILE LATE, in the basic block that issues the
// next tile's MFMAs: with one wave per SIMD nothing else hides them, and checked right behind
// its own MFMA chain a tile's ~90 bound / compare instructions and the ballot's branch ran
// with the matrix pipe idle (production 0.57 ms against 0.445 for MFMA + bound).
// MODE: 0 production, 1 MFMA + bound only (no top-k), 2 loads only, 3 loads + unpack.
template <int D, bool FILTER, int MODE = 0>
__global__ __launch_bounds__(kScanBlock, 1) void scan_kernel_i6(
    const char* __restrict__ c6, const float* __restrict__ meta,
    const uint32_t* __restrict__ tags, const uint32_t* __restrict__ filt,
    const intx4* __restrict__ qfrag8, const float* __restrict__ qp8, int n_rows, int n_tiles,
    const float* __restrict__ seed_thr, float* __restrict__ part_s, int* __restrict__ part_i,
    float* __restrict__ heads_s, int* __restrict__ heads_i, int* __restrict__ heads_n) {
  static_assert(D == 384, "pair6 layout");
  __shared__ int lds[kWavesPerWG * kLdsPerWave];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  ScanTopK st;
  PairWalk pw;
  Query8<D> q;
  prescan_start<D, FILTER>(st, pw, q, lds, wid, lane, seed_thr, filt, n_tiles, qfrag8, qp8);
  const int gw = pw.gw, nw = pw.nw;
  const int p_first = pw.p_first, p_step = pw.p_step, n_mine = pw.n_mine;
  // The lo planes live in accumulation registers, which the MFMAs read as they read vector
  // registers: three batches in flight and both planes do not fit the 256 vector registers, and
  // left to itself the allocator parks fragments there and copies each back before its use
  // (27 copies per tile)
#pragma unroll
  for (int s = 0; s < steps8<D>(); ++s) {
    asm volatile("" : "+a"(q.l0[s]));
    asm volatile("" : "+a"(q.l1[s]));
  }

  struct Batch {
    intx4 x[9];
    PairSide side;
  };
  const int voff = lane * 16, goff = (lane >> 4) * 16;
  auto load = [&](Batch& b, int j) __attribute__((always_inline)) {
    const int p = __builtin_amdgcn_readfirstlane(p_first + j * p_step);
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(c6 + (int64_t)p * kPair6Bytes, kPair6Bytes);
#pragma unroll
    for (int L = 0; L < 9; ++L)
      b.x[L] = __builtin_bit_cast(intx4,
                                  __builtin_amdgcn_raw_buffer_load_b128(rs, voff, L * 1024, 2));
    pair_side_load<FILTER>(b.side, meta, tags, p, n_tiles, goff);
    __builtin_amdgcn_sched_barrier(0);
  };
  float vmax = kNegInf;   // MODE 1/2/3: keeps the work alive
  // the tile whose dots await their bound and check. Before the first: the spare tile n_tiles
  // with zero scales, whose rows all fail topk_tile_tg's bound check
  // (two sets of dots, one per tile of a pair, written in turn: no copy between them)
  struct Held {
    float4 sc, er;
    uint4 tg;
    int t;
  } held;
  Dots dots[2];
  dots[1].h0 = dots[1].l0 = dots[1].h1 = dots[1].l1 = intx4{0, 0, 0, 0};
  held.sc = held.er = float4{0.f, 0.f, 0.f, 0.f};
  held.tg = uint4{0u, 0u, 0u, 0u};
  held.t = n_tiles;
  auto check_held = [&](const Dots& d) __attribute__((always_inline)) {
    floatx4 u0, u1;
    dots_u<D, Copy6>(d, q, held.sc, held.er, u0, u1);
    if constexpr (MODE == 0) {
      // a full tile (wave-uniform; every tile but the shard's last) skips the per-row checks
      const int t = __builtin_amdgcn_readfirstlane(held.t);
      if ((t + 1) * kTileRows <= n_rows)
        topk_tile_tg<FILTER>(st, u0, u1, t, 0x7fffffff, held.tg, lane);
      else
        topk_tile_tg<FILTER>(st, u0, u1, t, n_rows, held.tg, lane);
    } else {
      vmax = fmaxf(vmax, max8(u0, u1));
    }
  };
  auto process = [&](const Batch& b, int j) __attribute__((always_inline)) {
    const int p = p_first + j * p_step;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if constexpr (MODE == 2) {
        intx4 x = b.x[0];
#pragma unroll
        for (int L = 1; L < 9; ++L) x += b.x[L];
        if (u == 0) vmax = fmaxf(vmax, (float)(x[0] + x[1] + x[2] + x[3]));
        vmax = fmaxf(vmax, b.side.sc[u].x + b.side.er[u].x);
      } else {
        uint32_t w[18];
#pragma unroll
        for (int g = 0; g < 18; ++g) w[g] = (uint32_t)b.x[(18 * u + g) >> 2][(18 * u + g) & 3];
        if constexpr (MODE == 3) {
          intx4 x = {0, 0, 0, 0};
#pragma unroll
          for (int s = 0; s < steps8<D>(); ++s) x += unpack6(w[3 * s], w[3 * s + 1], w[3 * s + 2]);
          vmax = fmaxf(vmax, (float)(x[0] + x[1] + x[2] + x[3]) + b.side.sc[u].x + b.side.er[u].x);
        } else {
          tile_dots6<D>(w, q, dots[u]);   // issued first; the held tile's check beside them
          check_held(dots[u ^ 1]);
          held.sc = b.side.sc[u];
          held.er = b.side.er[u];
          held.tg = b.side.tg[u];
          held.t = 2 * p + u;
        }
      }
    }
  };
  if (n_mine > 0) {
    Batch b0, b1, b2;
    const auto at = [&](int j) { return min(j, n_mine - 1); };
    load(b0, 0);
    load(b1, at(1));
    int j = 0;
    while (true) {
      load(b2, at(j + 2));
      process(b0, j);
      if (++j >= n_mine) break;
      load(b0, at(j + 2));
      process(b1, j);
      if (++j >= n_mine) break;
      load(b1, at(j + 2));
      process(b2, j);
      if (++j >= n_mine) break;
    }
    if constexpr (MODE == 0 || MODE == 1) check_held(dots[1]);   // the last tile
  }
  if constexpr (MODE != 0) {
    keep_alive(vmax, part_s, gw);
    return;
  }
  topk_finish<2>(st, lane, gw, nw, part_s, part_i, heads_s, heads_i, heads_n);
}

// u of the 16 rows of tile t of a copy against the pass's 32 queries, by one wave, through the
// format's tile_u_at: out[q * n + i] for the requested row i = 16 t + (its position in the
// tile). One wave per requested row (rag_index_prescan_bounds; a test's direct view of the
// certificate's premise).
template <int D, typename Copy>
__global__ __launch_bounds__(64) void prescan_bounds_kernel(
    const char* __restrict__ data, const float* __restrict__ meta,
    const intx4* __restrict__ qfrag8, const float* __restrict__ qp8,
    const int64_t* __restrict__ rows, int64_t n, int64_t n_rows, int B,
    float* __restrict__ out) {
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int lane = threadIdx.x;
  const int64_t row = rows[i];
  if (row < 0 || row >= n_rows) {   // not a stored row: never dereferenced
    if (lane < B) out[(int64_t)lane * n + i] = kNegInf;
    return;
  }
  Query8<D> q;
  query8_load<D>(q, qfrag8, qp8, lane);
  floatx4 u0, u1;
  Copy::template tile_u_at<D>(data, meta, row >> 4, q, lane, u0, u1);
  // lane holds rows 4(lane >> 4) + r of queries (lane & 15), 16 + (lane & 15)
  const int r = (int)(row & 15) - 4 * (lane >> 4);
  if (r >= 0 && r < 4) {
    const int qa = lane & 15, qb = 16 + (lane & 15);
    const float va = r == 0 ? u0[0] : r == 1 ? u0[1] : r == 2 ? u0[2] : u0[3];
    const float vb = r == 0 ? u1[0] : r == 1 ? u1[1] : r == 2 ? u1[2] : u1[3];
    if (qa < B) out[(int64_t)qa * n + i] = va;
    if (qb < B) out[(int64_t)qb * n + i] = vb;
  }
}

// ---- register-pending top-k (LDS-query scan): the pending candidates of a lane live in
// VGPRs (8 slots per query tile, pushed by shifting: static register indices), so a wave's
// LDS is only its keep lists (8 KB) plus a 512-B gather scratch — which lets 8 waves share one
// workgroup's 64 KB of query fragments (2 waves per SIMD).
constexpr int kRP = 8;          // pending slots per (lane, query tile); flush at > kRP - 4
constexpr int kLdsWaves = 8;    // waves per scan_lds_kernel workgroup
constexpr int kLdsBlock = 64 * kLdsWaves;

struct RegTopK {
  float* keep_s;   // LDS [32 queries][32] best-first
  int* keep_i;
  float* xs;       // LDS [64] gather scratch
  int* xi;
  float thr0, thr1;
  int cnt0, cnt1;
  float p0s[kRP], p1s[kRP];
  int p0i[kRP], p1i[kRP];
  uint32_t fm0, fv0, fm1, fv1;
};

template <bool FILTER>
__device__ __forceinline__ void rtopk_init(RegTopK& st, int* lds, int wid, int lane,
                                           const float* __restrict__ seed_thr,
                                           const uint32_t* __restrict__ filt) {
  int* base = lds + wid * (2 * kQ * kKS + 128);
  st.keep_s = reinterpret_cast<float*>(base);
  st.keep_i = base + kQ * kKS;
  st.xs = reinterpret_cast<float*>(base + 2 * kQ * kKS);
  st.xi = base + 2 * kQ * kKS + 64;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    st.keep_s[lane + 64 * j] = kNegInf;
    st.keep_i[lane + 64 * j] = kIdNone32;
  }
#pragma unroll
  for (int sl = 0; sl < kRP; ++sl) {
    st.p0s[sl] = st.p1s[sl] = kNegInf;
    st.p0i[sl] = st.p1i[sl] = kIdNone32;
  }
  lds_fence();
  st.thr0 = st.thr1 = kNegInf;
  if (seed_thr) {
    const float T0 = seed_thr[lane & 15], T1 = seed_thr[16 + (lane & 15)];
    st.thr0 = T0 == kNegInf ? kNegInf : nextafterf(T0, kNegInf);
    st.thr1 = T1 == kNegInf ? kNegInf : nextafterf(T1, kNegInf);
  }
  st.cnt0 = st.cnt1 = 0;
  st.fm0 = st.fv0 = st.fm1 = st.fv1 = 0;
  if constexpr (FILTER) {
    st.fm0 = filt[2 * (lane & 15)];
    st.fv0 = filt[2 * (lane & 15) + 1];
    st.fm1 = filt[2 * (16 + (lane & 15))];
    st.fv1 = filt[2 * (16 + (lane & 15)) + 1];
  }
}

// this lane's pending entries of query tile qt -> scratch slots (lane >> 4) * 8 + sl (+ off)
__device__ __forceinline__ void rtopk_spill(const RegTopK& st, int qt, int lane, int off) {
#pragma unroll
  for (int sl = 0; sl < kRP; ++sl) {
    st.xs[off + (lane >> 4) * kRP + sl] = qt == 0 ? st.p0s[sl] : st.p1s[sl];
    st.xi[off + (lane >> 4) * kRP + sl] = qt == 0 ? st.p0i[sl] : st.p1i[sl];
  }
}

__device__ __forceinline__ void rtopk_clear(RegTopK& st, int qt) {
#pragma unroll
  for (int sl = 0; sl < kRP; ++sl) {
    if (qt == 0) {
      st.p0s[sl] = kNegInf;
      st.p0i[sl] = kIdNone32;
    } else {
      st.p1s[sl] = kNegInf;
      st.p1i[sl] = kIdNone32;
    }
  }
  if (qt == 0) st.cnt0 = 0; else st.cnt1 = 0;
}

// merge query q's keep list (32) with its pending entries (4 lanes x 8 slots), keep 32
__device__ __forceinline__ void rtopk_flush(RegTopK& st, int q, int lane) {
  const int qt = q >> 4, c = q & 15;
  const bool owner = (lane & 15) == c;
  if (owner) rtopk_spill(st, qt, lane, 0);
  lds_fence();
  float s;
  int id;
  if (lane < 32) {
    s = st.keep_s[q * kKS + lane];
    id = st.keep_i[q * kKS + lane];
  } else {
    s = st.xs[lane - 32];
    id = st.xi[lane - 32];
  }
  lds_fence();
  bitonic_sort64(s, id, lane);
  if (lane < 32) {
    st.keep_s[q * kKS + lane] = s;
    st.keep_i[q * kKS + lane] = id;
  }
  lds_fence();
  const float nt = __shfl(s, 31, 64);
  if (owner) {
    rtopk_clear(st, qt);
    if (qt == 0) st.thr0 = fmaxf(st.thr0, nt); else st.thr1 = fmaxf(st.thr1, nt);
  }
}

__device__ __forceinline__ void rtopk_flush_mask(RegTopK& st, uint64_t b, int qt, int lane) {
  uint32_t m = (uint32_t)((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xffffu);
  while (m) {
    const int c = __builtin_ctz(m);
    m &= m - 1;
    rtopk_flush(st, qt * 16 + c, lane);
  }
}

template <bool FILTER>
__device__ __forceinline__ void rtopk_tile(RegTopK& st, const floatx4& acc0, const floatx4& acc1,
                                           int t, int n_rows, const uint32_t* __restrict__ tags,
                                           int lane) {
  const int rbase = t * kTileRows + 4 * (lane >> 4);
  uint4 tg = {0u, 0u, 0u, 0u};
  if constexpr (FILTER) tg = *reinterpret_cast<const uint4*>(tags + rbase);
  // every tile but the shard's last is full: no per-row bound check there (wave-uniform)
  const bool full = (t + 1) * kTileRows <= n_rows;
  float v0[4], v1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool ok = full || (rbase + r) < n_rows;
    bool ok0 = ok, ok1 = ok;
    if constexpr (FILTER) {
      const uint32_t tr = r == 0 ? tg.x : r == 1 ? tg.y : r == 2 ? tg.z : tg.w;
      ok0 = ok0 && ((tr & st.fm0) == st.fv0);
      ok1 = ok1 && ((tr & st.fm1) == st.fv1);
    }
    v0[r] = ok0 ? acc0[r] : kNegInf;
    v1[r] = ok1 ? acc1[r] : kNegInf;
  }
  const float m0 = fmax_nc(fmax_nc(v0[0], v0[1]), fmax_nc(v0[2], v0[3]));
  const float m1 = fmax_nc(fmax_nc(v1[0], v1[1]), fmax_nc(v1[2], v1[3]));
  if (__ballot((m0 > st.thr0) || (m1 > st.thr1))) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (v0[r] > st.thr0) {
#pragma unroll
        for (int sl = kRP - 1; sl > 0; --sl) {
          st.p0s[sl] = st.p0s[sl - 1];
          st.p0i[sl] = st.p0i[sl - 1];
        }
        st.p0s[0] = v0[r];
        st.p0i[0] = rbase + r;
        ++st.cnt0;
      }
      if (v1[r] > st.thr1) {
#pragma unroll
        for (int sl = kRP - 1; sl > 0; --sl) {
          st.p1s[sl] = st.p1s[sl - 1];
          st.p1i[sl] = st.p1i[sl - 1];
        }
        st.p1s[0] = v1[r];
        st.p1i[0] = rbase + r;
        ++st.cnt1;
      }
    }
    const uint64_t b0 = __ballot(st.cnt0 > kRP - 4);
    const uint64_t b1 = __ballot(st.cnt1 > kRP - 4);
    if (b0) rtopk_flush_mask(st, b0, 0, lane);
    if (b1) rtopk_flush_mask(st, b1, 1, lane);
  }
}

__device__ __forceinline__ void rtopk_finish(RegTopK& st, int lane, int gw, int nw,
                                             float* __restrict__ part_s, int* __restrict__ part_i,
                                             float* __restrict__ heads_s,
                                             int* __restrict__ heads_i,
                                             int* __restrict__ heads_n) {
  const uint64_t b0 = __ballot(st.cnt0 > 0);
  const uint64_t b1 = __ballot(st.cnt1 > 0);
  const uint32_t p0 = (uint32_t)((b0 | (b0 >> 16) | (b0 >> 32) | (b0 >> 48)) & 0xffffu);
  const uint32_t p1 = (uint32_t)((b1 | (b1 >> 16) | (b1 >> 32) | (b1 >> 48)) & 0xffffu);
  const uint32_t pend = p0 | (p1 << 16);
  const uint32_t kept = (uint32_t)__ballot(lane < kQ && st.keep_s[(lane & 31) * kKS] != kNegInf);
  uint32_t full = pend & kept;
  uint32_t only = pend & ~kept;
  while (full) {
    const int q = __builtin_ctz(full);
    full &= full - 1;
    rtopk_flush(st, q, lane);
  }
  // queries that never flushed: their <= 32 pending entries only need a 32-wide sort, two
  // queries per pass (scratch halves 0..31 and 32..63)
  while (only) {
    const int qa = __builtin_ctz(only);
    only &= only - 1;
    const int qb = only ? __builtin_ctz(only) : -1;
    if (only) only &= only - 1;
    if ((lane & 15) == (qa & 15)) rtopk_spill(st, qa >> 4, lane, 0);
    if (qb >= 0 && (lane & 15) == (qb & 15)) rtopk_spill(st, qb >> 4, lane, 32);
    lds_fence();
    const int q = lane < 32 ? qa : qb;
    const int j = lane & 31;
    float s = kNegInf;
    int id = kIdNone32;
    if (q >= 0) {
      s = st.xs[lane];
      id = st.xi[lane];
    }
    lds_fence();
    bitonic_sort32x2(s, id, lane);
    if (q >= 0) {
      st.keep_s[q * kKS + j] = s;
      st.keep_i[q * kKS + j] = id;
    }
    lds_fence();
  }
  write_lists<kQ>(st.keep_s, st.keep_i, lane, 0, gw, nw, part_s + (int64_t)gw * (kQ * kKS),
                  part_i + (int64_t)gw * (kQ * kKS), heads_s, heads_i, heads_n);
}

// LDS-query scan for wide rows (D = 1024: the B-operands of 32 queries are 64 KB, too many
// VGPRs). The fragments are staged into LDS once per workgroup (one 8-wave workgroup per CU:
// 64 KB queries + 8 x 8.5 KB keep lists / scratch; pending candidates in VGPRs); each wave
// streams its tiles in chunks of 8 k-steps (8 KB) through a ring of D/256 chunk registers,
// so while one chunk is multiplied the rest of the tile (and the next tile's first chunks)
// are in flight. Per chunk: 8 A-fragments (buffer loads off a wave-uniform descriptor),
// 16 B-fragments from LDS (lane-linear: conflict-free), 16 MFMAs.
//
// Batches of more than 32 queries run as G query groups in ONE launch: grid = G x R
// workgroups; the G workgroups of tile range r (one per group) are dealt to the same XCD
// back to back (blocks go round-robin over the 8 XCDs) and walk identical tile sequences, so
// a tile comes from HBM once and from that XCD's L2 for the other G-1 groups (instead of G
// full passes over the corpus).
// NT: non-temporal loads (single group: the corpus is read once); shared groups need the
// default policy so the tile stays in L2 for the partner groups.
constexpr int kShareEvery = 2;    // progress exchange every 2 tiles
constexpr int kShareLead = 2;     // max tiles a wave may run ahead of its partners
constexpr int kShareSpin = 256;   // bounded wait (x s_sleep 4 = 256 clocks each)

template <int D, bool FILTER, bool NT>
__global__ __launch_bounds__(kLdsBlock, 1) void scan_lds_kernel(
    const half8* __restrict__ corpus, const uint32_t* __restrict__ tags,
    const uint32_t* __restrict__ filt, const half8* __restrict__ qfrag, int n_rows, int n_tiles,
    const float* __restrict__ seed_thr, float* __restrict__ part_s, int* __restrict__ part_i,
    float* __restrict__ heads_s, int* __restrict__ heads_i, int* __restrict__ heads_n,
    int groups, int* __restrict__ progress) {
  constexpr int S = steps<D>(), CH = 8, NCH = S / CH;
  static_assert(S % CH == 0 && NCH >= 2, "LDS-query scan: D must be a multiple of 256 (>= 512)");
  __shared__ int lds[kLdsWaves * (2 * kQ * kKS + 128)];
  __shared__ half8 qb[2 * S * 64];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  // block -> (tile range r, query group g); gridDim.x = groups * R with R % 8 == 0
  const int R = gridDim.x / groups;
  const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
  const int r = (loc / groups) * 8 + xcd, g = loc % groups;
  qfrag += g * (2 * S * 64);
  filt += g * (2 * kQ);
  seed_thr += g * kQ;
  const int nw = R * kLdsWaves;                      // lists per group
  part_s += (int64_t)g * nw * (kQ * kKS);
  part_i += (int64_t)g * nw * (kQ * kKS);
  heads_s += (int64_t)g * kQ * nw;
  heads_i += (int64_t)g * kQ * nw;
  heads_n += (int64_t)g * kQ * nw;
  for (int i = threadIdx.x; i < 2 * S * 64; i += 64 * kLdsWaves) qb[i] = qfrag[i];
  RegTopK st;
  rtopk_init<FILTER>(st, lds, wid, lane, seed_thr, filt);
  __syncthreads();

  const int gw = r * kLdsWaves + __builtin_amdgcn_readfirstlane(wid);
  int t_first, t_step, n_mine;
  tile_sequence<true>(gw, nw, n_tiles, t_first, t_step, n_mine);

  if (n_mine > 0) {
    half8 buf[NCH][CH];
    const char* cbase = reinterpret_cast<const char*>(corpus);
    const int voff = lane * 16;
    auto load_chunk = [&](half8(&a)[CH], int j, int c) {
      const int t = __builtin_amdgcn_readfirstlane(t_first + j * t_step);
      tile_load<CH, NT>(a, cbase + (int64_t)t * (S * 1024) + c * (CH * 1024), voff);
      __builtin_amdgcn_sched_barrier(0);
    };
#pragma unroll
    for (int c = 0; c < NCH; ++c) load_chunk(buf[c], 0, c);
    for (int j = 0; j < n_mine; ++j) {
      if constexpr (!NT) {
        // Shared groups: keep this wave within kShareLead tiles of its partner waves (same
        // tile sequence, other query groups), so the partners' reads of a tile hit the L2
        // line this wave's read brought in. Progress words are agent-scope atomics; the wait
        // is bounded (a throttle, never a dependency: if a partner is not running, the wave
        // proceeds after kShareSpin polls).
        if ((j & (kShareEvery - 1)) == 0) {
          int* mine = progress + (int64_t)gw * groups;
          if (lane == 0)
            __hip_atomic_store(mine + g, j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          for (int it = 0; it < kShareSpin; ++it) {
            int lag = 0;
            for (int gg = 0; gg < groups; ++gg) {
              const int v = __hip_atomic_load(mine + gg, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
              lag = max(lag, (j + 1) - v);
            }
            if (__builtin_amdgcn_readfirstlane(lag) <= kShareLead) break;
            __builtin_amdgcn_s_sleep(4);
          }
        }
      }
      const int jn = min(j + 1, n_mine - 1);
      floatx4 acc0 = {0.f, 0.f, 0.f, 0.f};
      floatx4 acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int s = 0; s < CH; ++s) {
          const half8 b0 = qb[(c * CH + s) * 64 + lane];
          const half8 b1 = qb[(S + c * CH + s) * 64 + lane];
          acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(buf[c][s], b0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(buf[c][s], b1, acc1, 0, 0, 0);
        }
        load_chunk(buf[c], jn, c);
      }
      rtopk_tile<FILTER>(st, acc0, acc1, t_first + j * t_step, n_rows, tags, lane);
    }
  }
  if constexpr (!NT) {
    // finished (or no tiles): never hold partners back
    if (lane == 0)
      __hip_atomic_store(progress + (int64_t)gw * groups + g, 0x3fffffff, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  rtopk_finish(st, lane, gw, nw, part_s, part_i, heads_s, heads_i, heads_n);
}

// ---- one-query-tile register top-k (scan_wide_kernel): 16 queries per wave, pending in
// VGPRs, keep lists in LDS (4 KB/wave), and the flush gathers the pending entries with lane
// shuffles instead of an LDS scratch.
struct WideTopK {
  float* keep_s;   // LDS [16][32]
  int* keep_i;
  float thr;
  int cnt;
  float ps[kRP];
  int pi[kRP];
};

__device__ __forceinline__ void wtopk_init(WideTopK& st, int* keep, int lane,
                                           const float* __restrict__ seed_thr) {
  st.keep_s = reinterpret_cast<float*>(keep);
  st.keep_i = keep + 16 * kKS;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    st.keep_s[lane + 64 * j] = kNegInf;
    st.keep_i[lane + 64 * j] = kIdNone32;
  }
#pragma unroll
  for (int sl = 0; sl < kRP; ++sl) {
    st.ps[sl] = kNegInf;
    st.pi[sl] = kIdNone32;
  }
  lds_fence();
  st.thr = kNegInf;
  if (seed_thr) {
    const float T = seed_thr[lane & 15];
    st.thr = T == kNegInf ? kNegInf : nextafterf(T, kNegInf);
  }
  st.cnt = 0;
}

// pending entry (lane's slot `sl` of lane `src`), for 32 consumer lanes: consumer j takes
// slot j & 7 of lane (c + 16 * (j >> 3)) — the 4 lanes x 8 slots of query column c
__device__ __forceinline__ void wtopk_gather(const WideTopK& st, int c, int j, float& s, int& id) {
  const int src = c + 16 * ((j >> 3) & 3), want = j & 7;
  s = kNegInf;
  id = kIdNone32;
#pragma unroll
  for (int sl = 0; sl < kRP; ++sl) {
    const float vs = __shfl(st.ps[sl], src, 64);
    const int vi = __shfl(st.pi[sl], src, 64);
    if (want == sl) {
      s = vs;
      id = vi;
    }
  }
}

__device__ __forceinline__ void wtopk_flush(WideTopK& st, int c, int lane) {
  // the shuffles run on all 64 lanes (a source lane must be active); lanes 0..31 then take
  // the keep list instead
  float s;
  int id;
  wtopk_gather(st, c, lane & 31, s, id);
  if (lane < 32) {
    s = st.keep_s[c * kKS + lane];
    id = st.keep_i[c * kKS + lane];
  }
  lds_fence();
  bitonic_sort64(s, id, lane);
  if (lane < 32) {
    st.keep_s[c * kKS + lane] = s;
    st.keep_i[c * kKS + lane] = id;
  }
  lds_fence();
  const float nt = __shfl(s, 31, 64);
  if ((lane & 15) == c) {
#pragma unroll
    for (int sl = 0; sl < kRP; ++sl) {
      st.ps[sl] = kNegInf;
      st.pi[sl] = kIdNone32;
    }
    st.cnt = 0;
    st.thr = fmaxf(st.thr, nt);
  }
}

__device__ __forceinline__ void wtopk_tile(WideTopK& st, const floatx4& acc, int t, int n_rows,
                                           int lane) {
  const int rbase = t * kTileRows + 4 * (lane >> 4);
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = (rbase + r) < n_rows ? acc[r] : kNegInf;
  const float m = fmax_nc(fmax_nc(v[0], v[1]), fmax_nc(v[2], v[3]));
  if (__ballot(m > st.thr)) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (v[r] > st.thr) {
#pragma unroll
        for (int sl = kRP - 1; sl > 0; --sl) {
          st.ps[sl] = st.ps[sl - 1];
          st.pi[sl] = st.pi[sl - 1];
        }
        st.ps[0] = v[r];
        st.pi[0] = rbase + r;
        ++st.cnt;
      }
    }
    const uint64_t bm = __ballot(st.cnt > kRP - 4);
    if (bm) {
      uint32_t mm = (uint32_t)((bm | (bm >> 16) | (bm >> 32) | (bm >> 48)) & 0xffffu);
      while (mm) {
        const int c = __builtin_ctz(mm);
        mm &= mm - 1;
        wtopk_flush(st, c, lane);
      }
    }
  }
}

// end of scan: flush, then write this wave's 16 query rows of its group's list b
__device__ __forceinline__ void wtopk_finish(WideTopK& st, int lane, int qt, int b, int nw,
                                             float* __restrict__ part_s, int* __restrict__ part_i,
                                             float* __restrict__ heads_s,
                                             int* __restrict__ heads_i,
                                             int* __restrict__ heads_n) {
  const uint64_t bp = __ballot(st.cnt > 0);
  const uint32_t pend = (uint32_t)((bp | (bp >> 16) | (bp >> 32) | (bp >> 48)) & 0xffffu);
  const uint32_t kept = (uint32_t)__ballot(lane < 16 && st.keep_s[(lane & 15) * kKS] != kNegInf);
  uint32_t full = pend & kept;
  uint32_t only = pend & ~kept;
  while (full) {
    const int c = __builtin_ctz(full);
    full &= full - 1;
    wtopk_flush(st, c, lane);
  }
  while (only) {   // never-flushed columns: 32-wide sorts, two columns per pass
    const int ca = __builtin_ctz(only);
    only &= only - 1;
    const int cb = only ? __builtin_ctz(only) : -1;
    if (only) only &= only - 1;
    const int c = lane < 32 ? ca : cb;
    float s;
    int id;
    wtopk_gather(st, c < 0 ? 0 : c, lane & 31, s, id);
    if (c < 0) {
      s = kNegInf;
      id = kIdNone32;
    }
    bitonic_sort32x2(s, id, lane);
    if (c >= 0) {
      st.keep_s[c * kKS + (lane & 31)] = s;
      st.keep_i[c * kKS + (lane & 31)] = id;
    }
    lds_fence();
  }
  write_lists<16>(st.keep_s, st.keep_i, lane, qt * 16, b, nw,
                  part_s + (int64_t)b * (kQ * kKS) + qt * 16 * kKS,
                  part_i + (int64_t)b * (kQ * kKS) + qt * 16 * kKS, heads_s, heads_i, heads_n);
}

// Wide rows, several query groups, ONE pass over the corpus (D = 1024, 2..4 groups of 32,
// unfiltered): each workgroup (8 waves, one per CU) streams its tiles t = b, b + nb, ... into
// a 4-tile LDS ring by direct global->LDS loads (global_load_lds_dwordx4; the tile16 layout
// is already lane-linear, so the LDS image is the HBM image), three tiles in flight, and ALL
// 8 waves consume every tile: wave w = (group w/2, query tile w%2) holds its 16 queries'
// fragments over all 1024 dims in VGPRs (32 half8) and runs their top-k (16 columns,
// register pending). A tile is read from HBM once for all groups. Sync: counted vmcnt + one
// raw s_barrier per tile (tile j landed AND every wave is done with tile j-1, whose slot the
// next load reuses). The loop issues no VMEM besides the ring loads, so the counts are exact.
constexpr int kWideBufs = 4;
constexpr int kWideWaves = 8;
constexpr int kWideBlock = 64 * kWideWaves;
constexpr int kWidePre = 8;   // tile-fragment LDS reads in flight ahead of the MFMA chain

// MODE (diagnostic timing variants, rag_bench_scan at dim 1024): 0 production; 1 no top-k (MFMA + a
// running max); 2 loads and barriers only; 3 production with an infinite threshold (the
// per-tile check runs, no candidate is ever taken: results invalid); 4 loads, barriers and
// the tile-fragment LDS reads, no MFMA (round 4's half-tile ring, MODE 5, was measured no faster
// and removed in round 5). NT: ring loads with the non-temporal policy.
template <int D, int MODE = 0, bool NT = false>
__global__ __launch_bounds__(kWideBlock, 1) void scan_wide_kernel(
    const half8* __restrict__ corpus, const half8* __restrict__ qfrag, int n_rows, int n_tiles,
    const float* __restrict__ seed_thr, float* __restrict__ part_s, int* __restrict__ part_i,
    float* __restrict__ heads_s, int* __restrict__ heads_i, int* __restrict__ heads_n,
    int groups) {
  constexpr int S = steps<D>();
  constexpr int TILE = S * 64;                                   // half8 per tile
  constexpr int TK = 2 * 16 * kKS;                               // ints of keep state per wave
  static_assert(S * 1024 == kWideWaves * 4096, "wide scan: 8 waves x 4 KB = one tile");
  // one LDS object (ring | keep lists): a second __shared__ object next to a
  // global_load_lds target can make hipcc drain vmcnt before every ds_read
  __shared__ half8 lds[kWideBufs * TILE + kWideWaves * TK / 4];
  half8* ring = lds;
  int* keep = reinterpret_cast<int*>(lds + kWideBufs * TILE);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = wid >> 1, qt = wid & 1;
  const bool active = g < groups;
  const int nb = gridDim.x, b = blockIdx.x;
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  const uint32_t ring_addr = lds_addr_of(ring);

  half8 qf[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const half8 z = {};
    qf[s] = active ? qfrag[g * (2 * S * 64) + (qt * S + s) * 64 + lane] : z;
  }
  WideTopK st;
  wtopk_init(st, keep + wid * TK, lane, active ? seed_thr + g * kQ + qt * 16 : nullptr);
  if constexpr (MODE == 3) st.thr = __builtin_inff();
  const int nw = nb;                                             // lists per group
  part_s += (int64_t)g * nw * (kQ * kKS);
  part_i += (int64_t)g * nw * (kQ * kKS);
  heads_s += (int64_t)g * kQ * nw;
  heads_i += (int64_t)g * kQ * nw;
  heads_n += (int64_t)g * kQ * nw;

  // settle the query-fragment loads here: left pending into the loop, hipcc would put a
  // `vmcnt(0)` (draining the DMA ring) before their first MFMA use in every iteration
#pragma unroll
  for (int s = 0; s < S; ++s) asm volatile("" : "+v"(qf[s]));
  asm volatile("" : "+v"(st.thr));
  const int n_mine = b < n_tiles ? (n_tiles - 1 - b) / nb + 1 : 0;
  const char* cbase = reinterpret_cast<const char*>(corpus);
  auto issue = [&](int j) {   // this wave's 4 KB of tile j -> ring slot j % 4
    if (j < n_mine) {
      const int t = b + j * nb;
      const char* src = cbase + (int64_t)t * (S * 1024) + wid_u * 4096 + lane * 16;
      const uint32_t dst = ring_addr + (j % kWideBufs) * (TILE * 16) + wid_u * 4096;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (NT)
          glds16_nt(src + i * 1024, dst + i * 1024);
        else
          glds16(src + i * 1024, dst + i * 1024);
      }
    }
  };
  issue(0);
  issue(1);
  issue(2);
  for (int j = 0; j < n_mine; ++j) {
    const int later = min(2, n_mine - 1 - j);                  // tiles issued after j
    if (later == 2)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (later == 1)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();   // tile j landed for all; everyone is past tile j-1
    asm volatile("" ::: "memory");  // no LDS read of tile j may be scheduled above it
    issue(j + 3);                   // slot (j+3)%4 == (j-1)%4
    if (active && MODE != 2) {       // waves of absent groups (B <= 96) only stage and sync
      const half8* tb = ring + (j % kWideBufs) * TILE + lane;
      floatx4 acc = {0.f, 0.f, 0.f, 0.f};
      // Tile fragments read kWidePre steps ahead of the MFMA chain. Left to itself hipcc
      // keeps only two reads in flight, so every MFMA waits out a full (contended) LDS
      // latency: 32 of those per tile per wave outlast the tile's HBM time. The MFMA order
      // (and so every fp32 sum) is unchanged.
      half8 a[S];
#pragma unroll
      for (int s = 0; s < S; ++s) a[s] = tb[s * 64];
      if constexpr (MODE == 4) {   // the LDS reads without the MFMAs (diagnostic)
        uint32_t x = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) x ^= __builtin_bit_cast(uint4, a[s]).x;
        st.cnt ^= (int)x;
        continue;
      }
#pragma unroll
      for (int s = 0; s < S; ++s)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], qf[s], acc, 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, kWidePre, 0);    // DS reads
#pragma unroll
      for (int s = 0; s < S - kWidePre; ++s) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);         // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);         // one DS read
      }
      __builtin_amdgcn_sched_group_barrier(0x008, kWidePre, 0);
      if constexpr (MODE == 0 || MODE == 3) {
        wtopk_tile(st, acc, b + j * nb, n_rows, lane);
      } else {
        st.thr = fmax_nc(st.thr, fmax_nc(fmax_nc(acc[0], acc[1]), fmax_nc(acc[2], acc[3])));
      }
    }
  }
  if constexpr (MODE == 1) {
    if (active && st.thr == 1e30f) heads_n[0] = 0;    // keeps the MFMAs live
  }
  if constexpr (MODE == 4) {
    if (active && st.cnt == 0x1234567) heads_n[0] = 0;  // keeps the LDS reads live
  }
  if constexpr (MODE == 0 || MODE == 3)
    if (active) wtopk_finish(st, lane, qt, b, nw, part_s, part_i, heads_s, heads_i, heads_n);
}

// ----------------------------------------------------------------------------------------
// VALU ablation of the scan (rag_bench_scan variant 8; north_star's literal "MFMA only for
// the encoders' GEMMs"): the same 32-query dot products with v_dot2_f32_f16 (2 fp16 MACs per
// lane per instruction) instead of MFMA. Lane = row: a wave takes 64-row groups g = gw,
// gw + nw, ... of a row-group-major copy of the corpus (rows64[(g*C + c)*64 + lane] = the
// 8-dim chunk c of row 64g + lane: every load is one coalesced 1 KB wave read), while the
// 32 queries' chunk c is wave-uniform, read by scalar loads from qc[c][32]. 128 dot2 per
// chunk per lane, no cross-lane reduction. The 64 x 32 scores are then transposed through LDS
// into the MFMA accumulator layout so the production top-k (topk_tile, seeded thresholds)
// runs unchanged. Diagnostic only (results are not selected).
// ----------------------------------------------------------------------------------------
template <int D>
__global__ void rows64_kernel(const half8* __restrict__ corpus, int64_t n_rows,
                              half8* __restrict__ rows64) {
  constexpr int C = D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (row, chunk)
  if (idx >= n_rows * C) return;
  const int64_t r = idx / C;
  const int c = (int)(idx % C);
  rows64[((r >> 6) * C + c) * 64 + (r & 63)] = corpus[tile_slot<D>(r, c)];
}

template <int D>
__global__ __launch_bounds__(64) void qchunk_kernel(const float* __restrict__ qn,
                                                    half8* __restrict__ qc) {
  constexpr int C = D / 8;
  const int q = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += 64) {
    half8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = f32_to_f16(qn[q * D + 8 * c + j]);
    qc[c * kQ + q] = h;
  }
}

template <int D>
__global__ __launch_bounds__(256, 2) void scan_valu_kernel(
    const half8* __restrict__ rows64, const half8* __restrict__ qc, int n_rows, int n_groups,
    const float* __restrict__ seed_thr, float* __restrict__ part_s, int* __restrict__ part_i,
    float* __restrict__ heads_s, int* __restrict__ heads_i, int* __restrict__ heads_n) {
  constexpr int C = D / 8, PF = 8;
  static_assert(C % PF == 0, "chunks");
  __shared__ int lds[kWavesPerWG * kLdsPerWave];
  __shared__ float tr[kWavesPerWG][kQ / 2][64];   // 4 KB per wave: two WGs per CU
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  ScanTopK st;
  topk_init<false>(st, lds, wid, lane, seed_thr, nullptr);
  const int gw = blockIdx.x * kWavesPerWG + __builtin_amdgcn_readfirstlane(wid);
  const int nw = gridDim.x * kWavesPerWG;
  for (int g = gw; g < n_groups; g += nw) {
    const half8* rp = rows64 + (int64_t)g * C * 64 + lane;
    half8 ring[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) ring[u] = __builtin_nontemporal_load(rp + u * 64);
    float acc[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) acc[q] = 0.f;
    for (int c0 = 0; c0 < C; c0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const half8 a = ring[u];
        // prefetch PF chunks ahead (clamped: the last chunk is re-read, an L1/L2 hit, instead
        // of a branch around the load)
        ring[u] = __builtin_nontemporal_load(rp + min(c0 + PF + u, C - 1) * 64);
        // 8 queries' chunks (32 SGPRs of scalar loads) at a time. The empty asm takes the
        // group's sums as inputs and "rewrites" a zero offset of the query address, so the
        // next group's scalar loads depend on this group's dot products: without it the
        // scheduler hoists every group's loads to the top and spills SGPRs through VGPR
        // lanes. (The offset, not the pointer: a pointer out of an asm loses the const
        // provenance that lets the loads be scalar.)
        int zo = 0;
#pragma unroll
        for (int q0 = 0; q0 < kQ; q0 += 8) {
#pragma unroll
          for (int q = q0; q < q0 + 8; ++q) {
            const half8 b = qc[(c0 + u) * kQ + q + zo];   // wave-uniform: scalar loads
            float x = acc[q];
            x = __builtin_amdgcn_fdot2(half2v{a[0], a[1]}, half2v{b[0], b[1]}, x, false);
            x = __builtin_amdgcn_fdot2(half2v{a[2], a[3]}, half2v{b[2], b[3]}, x, false);
            x = __builtin_amdgcn_fdot2(half2v{a[4], a[5]}, half2v{b[4], b[5]}, x, false);
            x = __builtin_amdgcn_fdot2(half2v{a[6], a[7]}, half2v{b[6], b[7]}, x, false);
            acc[q] = x;
          }
          asm volatile("" : "+s"(zo)
                       : "v"(acc[q0]), "v"(acc[q0 + 1]), "v"(acc[q0 + 2]), "v"(acc[q0 + 3]),
                         "v"(acc[q0 + 4]), "v"(acc[q0 + 5]), "v"(acc[q0 + 6]), "v"(acc[q0 + 7]));
        }
      }
    }
    floatx4 a0[4], a1[4];       // the 4 tiles' scores in the MFMA accumulator layout
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int q = 0; q < kQ / 2; ++q) tr[wid][q][lane] = acc[h * 16 + q];
      lds_fence();
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(&tr[wid][lane & 15][16 * tt + 4 * (lane >> 4)]);
        if (h == 0) a0[tt] = v; else a1[tt] = v;
      }
      lds_fence();
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int t = 4 * g + tt;
      if (t * kTileRows >= n_rows) break;
      topk_tile<false>(st, a0[tt], a1[tt], t, n_rows, nullptr, lane);
    }
  }
  topk_finish(st, lane, gw, nw, part_s, part_i, heads_s, heads_i, heads_n);
}

}  // namespace ragmi
