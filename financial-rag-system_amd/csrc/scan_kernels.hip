// scan_kernels.hip — in-HBM flat cosine index for gfx950 (MI355X): upsert, query prep,
// brute-force MFMA scan with a per-wave top-k, and the exact-rescoring merges.
//
// Replaces the Qdrant server's COSINE collection behind QdrantClient.query_points / upsert
// (reference main.py:215-239, ingest.py:148-175).
//
// Storage layout in HBM ("tile16"): rows are grouped in tiles of 16; a tile is stored in the
// exact order the v_mfma_f32_16x16x32_f16 A-operand wants it, so every wave-wide load of the
// scan is one perfectly coalesced 1 KiB dwordx4 (16 B/lane x 64 lanes):
//     tile t, k-step s (32 dims), lane l = h*16 + r  ->  8 halves  row 16t+r, dims 32s+8h..+7
//     half8 index = t*(D/32)*64 + s*64 + l
// The query batch (32 queries = two 16-wide MFMA column tiles) is prepared into the matching
// B-operand order and kept in VGPRs for the whole scan.
#include "device_common.hpp"

namespace ragmi {

constexpr int kTileRows = 16;
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
constexpr int kQ = 32;            // queries per pass
constexpr int kKS = 32;           // candidates kept per (wave, query)
constexpr int kP = 8;             // pending slots per (lane, query tile)
constexpr int kWavesPerWG = 4;
constexpr int kScanBlock = 64 * kWavesPerWG;   // scan_kernel / rescan_kernel block (launch_fixed)
constexpr int kMaxLists = 2048;   // max scan waves (= per-wave lists) per pass
constexpr int kLdsPerWave = 4096; // dwords: keep_s[32][32] keep_i[32][32] pend_s[2][8][64] pend_i[2][8][64]
constexpr int kTileQStride = 16;  // ints between the 8 per-XCD tile-queue heads (64 B apart)
constexpr int kDynChunk = 2;      // tiles per dequeue of the dynamic scan schedule

template <int D>
__host__ __device__ constexpr int steps() { return D / 32; }

// ----------------------------------------------------------------------------------------
// upsert: one wave per vector. Canonical normalisation -> fp16 (RNE) -> tile16 slot.
// ----------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(64) void upsert_kernel(const float* __restrict__ vecs,
                                                    const int64_t* __restrict__ rows,
                                                    const uint32_t* __restrict__ tags_in,
                                                    half8* __restrict__ corpus,
                                                    uint32_t* __restrict__ tags, int64_t n,
                                                    int64_t cap_rows,
                                                    float* __restrict__ rows32 = nullptr) {
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int lane = threadIdx.x;
  const int64_t row = rows[i];
  if (row < 0 || row >= cap_rows) return;  // host validates; never write out of bounds
  const float* x = vecs + i * D;
  const double norm = sqrt(canon_sumsq<D>(x, lane));
  const int64_t t = row >> 4;
  const int r = (int)(row & 15);
  for (int c = lane; c < D / 8; c += 64) {
    half8 h;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      y[j] = canon_scale(x[8 * c + j], norm);
      h[j] = f32_to_f16(y[j]);
    }
    const int s = c >> 2, hh = c & 3;
    corpus[t * (steps<D>() * 64) + s * 64 + hh * 16 + r] = h;
    if (rows32) {   // fp32 storage: the normalised fp32 row itself (exact rescoring operand)
      float4* o = reinterpret_cast<float4*>(rows32 + row * D + 8 * c);
      o[0] = float4{y[0], y[1], y[2], y[3]};
      o[1] = float4{y[4], y[5], y[6], y[7]};
    }
  }
  if (lane == 0) tags[row] = tags_in ? tags_in[i] : 0u;
}

// ----------------------------------------------------------------------------------------
// query prep: one wave per query slot (32 slots; slots >= B are zero).
//   qn    [32][D] fp32 canonical-normalised queries (exact rescoring operand)
//   qfrag [2][D/32][64] half8: B-operand fragments, lane l -> query 16*qt + (l&15),
//         dims 32s + 8(l>>4) .. +7
//   filt  [32][2] (tag mask, tag value) per query slot
//   eps   [32] bound on |MFMA score - exact score| over every stored row (see below)
//
// Error bound. Stored rows c are fp16 roundings of unit vectors (||c||_2 <= kRowNorm); the
// scan scores a = MFMA(c, h) with h = fp16(qn) and fp32 accumulation over D products (each
// product exact in fp32), the exact score is e = fp32(sum c_k qn_k). Then
//   |a - e| <= ||c|| ||h - qn||            (query rounding, Cauchy-Schwarz)
//            + D 2^-23 ||c|| ||h||          (<= D roundings of the fp32 accumulator, each
//                                            <= 1 ulp: holds for any internal MFMA order)
//            + 2^-23                        (e's own fp32 rounding)
//            [+ store_eps]                  (fp32 storage: the exact score reads the fp32 row
//                                            c32 while the scan reads c = fp16(c32):
//                                            |sum (c - c32) qn| <= ||c - c32|| ||qn|| <=
//                                            2^-11 ||c32|| + 2^-25 sqrt(D), times ||qn||)
// inflated by 2^-10 relative + 2^-22 absolute so the fp32 comparisons that use it in select
// stay conservative.
// ----------------------------------------------------------------------------------------
constexpr double kRowNorm = 1.001;   // fp16(unit vector): ||c|| <= 1 + 2^-11 + sqrt(D) 2^-25

// one query slot b by one wave. The B-fragment goes to qf (global or an LDS image of the same
// layout); qn / filt / eps are written only when `publish` (the fused qprep_sample_kernel:
// every workgroup builds the fragments it samples with, workgroup 0 publishes)
template <int D>
__device__ __forceinline__ void qprep_slot(const float* __restrict__ q, int B, int b, int lane,
                                           const uint32_t* __restrict__ filt_in,
                                           float* __restrict__ qn, half8* __restrict__ qf,
                                           uint32_t* __restrict__ filt, float* __restrict__ eps,
                                           double store_eps, bool publish,
                                           uint32_t* __restrict__ filt_copy = nullptr,
                                           half8* __restrict__ qf_glob = nullptr) {
  const bool live = b < B;
  if (lane == 0) {
    // per-query payload filter (mask, value); padding / unfiltered queries match every row
    const uint32_t fm = (live && filt_in) ? filt_in[2 * b] : 0u;
    const uint32_t fv = (live && filt_in) ? filt_in[2 * b + 1] : 0u;
    if (publish) {
      filt[2 * b] = fm;
      filt[2 * b + 1] = fv;
    }
    if (filt_copy) {
      filt_copy[2 * b] = fm;
      filt_copy[2 * b + 1] = fv;
    }
  }
  double norm = 0.0;
  if (live) norm = sqrt(canon_sumsq<D>(q + (int64_t)b * D, lane));
  const int qt = b >> 4, c16 = b & 15;
  double dq2 = 0.0, hh2 = 0.0;   // ||h - qn||^2, ||h||^2 (lane partials)
  for (int c = lane; c < D / 8; c += 64) {
    half8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float y = live ? canon_scale(q[(int64_t)b * D + 8 * c + j], norm) : 0.0f;
      if (publish) qn[b * D + 8 * c + j] = y;
      h[j] = f32_to_f16(y);
      const double hd = (double)h[j], dd = hd - (double)y;
      dq2 = fma(dd, dd, dq2);
      hh2 = fma(hd, hd, hh2);
    }
    const int s = c >> 2, hh = c & 3;
    qf[(qt * steps<D>() + s) * 64 + hh * 16 + c16] = h;
    if (qf_glob) qf_glob[(qt * steps<D>() + s) * 64 + hh * 16 + c16] = h;
  }
  if (!publish) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    dq2 += __shfl_xor(dq2, d, 64);
    hh2 += __shfl_xor(hh2, d, 64);
  }
  if (lane == 0) {
    double e = kRowNorm * sqrt(dq2) + (double)D * 0x1p-23 * kRowNorm * sqrt(hh2) + 0x1p-23 +
               store_eps;
    e = e * (1.0 + 0x1p-10) + 0x1p-22;
    eps[b] = live ? (float)(e * (1.0 + 0x1p-20)) : 0.0f;   // rounded up past fp32's RNE
  }
}

template <int D>
__global__ __launch_bounds__(64) void qprep_kernel(const float* __restrict__ q, int B,
                                                   const uint32_t* __restrict__ filt_in,
                                                   float* __restrict__ qn,
                                                   half8* __restrict__ qfrag,
                                                   uint32_t* __restrict__ filt,
                                                   float* __restrict__ eps,
                                                   double store_eps = 0.0) {
  qprep_slot<D>(q, B, blockIdx.x, threadIdx.x, filt_in, qn, qfrag, filt, eps, store_eps, true);
}

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
        float s = kNegInf;
        int id = kIdNone32;
        if (q >= 0) {
          const int pidx = (((q >> 4) * kP + (j & 1)) * 64) + (q & 15) + 16 * (j >> 1);
          s = w.pend_s[pidx];
          id = w.pend_i[pidx];
        }
        lds_fence();
        bitonic_sort8x8(s, id, lane);
        if (q >= 0) {
          w.keep_s[q * kKS + j] = s;
          w.keep_i[q * kKS + j] = id;
        }
        lds_fence();
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
      float s = kNegInf;
      int id = kIdNone32;
      if (q >= 0) {
        const int pidx = (((q >> 4) * kP + (j & 3)) * 64) + (q & 15) + 16 * (j >> 2);
        s = w.pend_s[pidx];
        id = w.pend_i[pidx];
      }
      lds_fence();
      bitonic_sort16x4(s, id, lane);
      if (q >= 0) {
        w.keep_s[q * kKS + j] = s;
        w.keep_i[q * kKS + j] = id;
      }
      lds_fence();
    }
    while (SORT == 1 && only) {
      const int qa = __builtin_ctz(only);
      only &= only - 1;
      const int qb = only ? __builtin_ctz(only) : -1;
      if (only) only &= only - 1;
      const int q = lane < 32 ? qa : qb;
      const int j = lane & 31;
      float s = kNegInf;
      int id = kIdNone32;
      if (q >= 0) {
        const int pidx = (((q >> 4) * kP + (j & 7)) * 64) + (q & 15) + 16 * (j >> 3);
        s = w.pend_s[pidx];
        id = w.pend_i[pidx];
      }
      lds_fence();
      bitonic_sort32x2(s, id, lane);
      if (q >= 0) {
        w.keep_s[q * kKS + j] = s;
        w.keep_i[q * kKS + j] = id;
      }
      lds_fence();
    }
  }
  float* ps = part_s + (int64_t)gw * (kQ * kKS);
  int* pi = part_i + (int64_t)gw * (kQ * kKS);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float v = w.keep_s[lane + 64 * j];
    if (v != kNegInf) {
      ps[lane + 64 * j] = v;
      pi[lane + 64 * j] = w.keep_i[lane + 64 * j];
    }
  }
  if (lane < kQ) {
    int n = 0;
    for (int j = 0; j < kKS; ++j) n += w.keep_s[lane * kKS + j] != kNegInf;
    heads_s[lane * nw + gw] = w.keep_s[lane * kKS];
    heads_i[lane * nw + gw] = n > 0 ? w.keep_i[lane * kKS] : kIdNone32;
    heads_n[lane * nw + gw] = n;
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
#pragma unroll
      for (int s = 0; s < S; ++s) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], q0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], q1[s], acc1, 0, 0, 0);
      }
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

  // Buffer loads off a wave-uniform per-tile descriptor: the address lives in SGPRs and the
  // per-lane part is one VGPR (lane*16), so no 64-bit address VGPRs are live across the
  // loop (their reuse as load destinations forced a vmcnt(0) at the loop head).
  const char* cbase = reinterpret_cast<const char*>(corpus);
  const int voff = lane * 16;
  auto load_t = [&](half8(&a)[S], int t_in) __attribute__((always_inline)) {
    const int t = __builtin_amdgcn_readfirstlane(t_in);
    const char* tp = cbase + (int64_t)t * (S * 1024);
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(tp), 0, S * 1024, 0x00020000);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, s * 1024, NT ? 2 : 0);
      a[s] = __builtin_bit_cast(half8, v);
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
    auto load = [&](half8(&a)[S], uint4& tg, int j) {
      const int t = __builtin_amdgcn_readfirstlane(t_first + j * t_step);
      const char* tp = cbase + (int64_t)t * (S * 1024);
      const __amdgpu_buffer_rsrc_t rs =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(tp), 0, S * 1024, 0x00020000);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, s * 1024, NT ? 2 : 0);
        a[s] = __builtin_bit_cast(half8, v);
      }
      if constexpr (FILTER) {
        const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint32_t*>(tags + (int64_t)t * kTileRows), 0, kTileRows * 4, 0x00020000);
        tg = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                           rt, (lane >> 4) * 16, 0, 0));
      }
      if constexpr (SB) __builtin_amdgcn_sched_barrier(0);
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
  float* ps = part_s + (int64_t)gw * (kQ * kKS);
  int* pi = part_i + (int64_t)gw * (kQ * kKS);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float v = st.keep_s[lane + 64 * j];
    if (v != kNegInf) {
      ps[lane + 64 * j] = v;
      pi[lane + 64 * j] = st.keep_i[lane + 64 * j];
    }
  }
  if (lane < kQ) {
    int n = 0;
    for (int j = 0; j < kKS; ++j) n += st.keep_s[lane * kKS + j] != kNegInf;
    heads_s[lane * nw + gw] = st.keep_s[lane * kKS];
    heads_i[lane * nw + gw] = n > 0 ? st.keep_i[lane * kKS] : kIdNone32;
    heads_n[lane * nw + gw] = n;
  }
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
      const char* tp = cbase + (int64_t)t * (S * 1024) + c * (CH * 1024);
      const __amdgpu_buffer_rsrc_t rs =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(tp), 0, CH * 1024, 0x00020000);
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, s * 1024, NT ? 2 : 0);
        a[s] = __builtin_bit_cast(half8, v);
      }
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
  float* ps = part_s + (int64_t)b * (kQ * kKS) + qt * 16 * kKS;
  int* pi = part_i + (int64_t)b * (kQ * kKS) + qt * 16 * kKS;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = st.keep_s[lane + 64 * j];
    if (v != kNegInf) {
      ps[lane + 64 * j] = v;
      pi[lane + 64 * j] = st.keep_i[lane + 64 * j];
    }
  }
  if (lane < 16) {
    int n = 0;
    for (int j = 0; j < kKS; ++j) n += st.keep_s[lane * kKS + j] != kNegInf;
    const int q = qt * 16 + lane;
    heads_s[q * nw + b] = st.keep_s[lane * kKS];
    heads_i[q * nw + b] = n > 0 ? st.keep_i[lane * kKS] : kIdNone32;
    heads_n[q * nw + b] = n;
  }
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
  constexpr int C = D / 8, S = steps<D>();
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (row, chunk)
  if (idx >= n_rows * C) return;
  const int64_t r = idx / C;
  const int c = (int)(idx % C);
  rows64[((r >> 6) * C + c) * 64 + (r & 63)] =
      corpus[(r >> 4) * (S * 64) + (c >> 2) * 64 + (c & 3) * 16 + (r & 15)];
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

// ----------------------------------------------------------------------------------------
// sample: seed thresholds for the scan. Sample wave w scores the corpus tiles
//   t = (j * n_tiles) / n_sample, j = w, w + n_waves, ...   (spread over the shard)
// and writes, per query, the max score over its (valid, filter-passing) rows to
// smax[w][q]. The 32nd largest of these per-wave maxima comes from 32 distinct rows, so it
// is a lower bound of the global 32nd-best score: thresh_kernel turns it into seed_thr.
// ----------------------------------------------------------------------------------------
// per-query maxima of one wave's two sample tiles (sc[tile][query half]) -> smax[q][j]
template <bool FILTER>
__device__ __forceinline__ void sample_epilogue(const floatx4 (&sc)[2][2], int t0, int t1,
                                                bool two, int j0, int lane,
                                                const uint32_t* __restrict__ tags,
                                                const uint32_t* __restrict__ filt, int n_rows,
                                                int n_sample, float* __restrict__ smax) {
  uint32_t fm0 = 0, fv0 = 0, fm1 = 0, fv1 = 0;
  if constexpr (FILTER) {
    fm0 = filt[2 * (lane & 15)];
    fv0 = filt[2 * (lane & 15) + 1];
    fm1 = filt[2 * (16 + (lane & 15))];
    fv1 = filt[2 * (16 + (lane & 15)) + 1];
  }
  float mx[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = u == 0 ? t0 : t1;
    const floatx4 acc0 = sc[u][0], acc1 = sc[u][1];
    const int rbase = t * kTileRows + 4 * (lane >> 4);
    uint4 tg = {0u, 0u, 0u, 0u};
    if constexpr (FILTER) tg = *reinterpret_cast<const uint4*>(tags + rbase);
    float m0 = kNegInf, m1 = kNegInf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = (rbase + r) < n_rows;
      bool ok0 = ok, ok1 = ok;
      if constexpr (FILTER) {
        const uint32_t tr = r == 0 ? tg.x : r == 1 ? tg.y : r == 2 ? tg.z : tg.w;
        ok0 = ok0 && ((tr & fm0) == fv0);
        ok1 = ok1 && ((tr & fm1) == fv1);
      }
      m0 = ok0 ? fmax_nc(m0, acc0[r]) : m0;
      m1 = ok1 ? fmax_nc(m1, acc1[r]) : m1;
    }
    // lanes l, l^16, l^32, l^48 hold the same queries
    m0 = fmaxf(m0, __shfl_xor(m0, 16, 64));
    m0 = fmaxf(m0, __shfl_xor(m0, 32, 64));
    m1 = fmaxf(m1, __shfl_xor(m1, 16, 64));
    m1 = fmaxf(m1, __shfl_xor(m1, 32, 64));
    mx[u][0] = m0;
    mx[u][1] = m1;
  }
  if (lane < 16) {
    smax[(int64_t)lane * n_sample + j0] = mx[0][0];
    smax[(int64_t)(16 + lane) * n_sample + j0] = mx[0][1];
    if (two) {
      smax[(int64_t)lane * n_sample + j0 + 1] = mx[1][0];
      smax[(int64_t)(16 + lane) * n_sample + j0 + 1] = mx[1][1];
    }
  }
}

template <int D, bool FILTER>
__global__ __launch_bounds__(256) void sample_kernel(const half8* __restrict__ corpus,
                                                     const uint32_t* __restrict__ tags,
                                                     const uint32_t* __restrict__ filt,
                                                     const half8* __restrict__ qfrag,
                                                     int n_rows, int n_tiles, int n_sample,
                                                     float* __restrict__ smax) {
  constexpr int S = steps<D>();
  // query group (32 queries) blockIdx.y: its fragments, filters and maxima
  qfrag += blockIdx.y * (2 * S * 64);
  filt += blockIdx.y * (2 * kQ);
  smax += (int64_t)blockIdx.y * kQ * n_sample;
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // two sample tiles per wave (j = 2w, 2w+1), all loads in flight at once
  const int j0 = 2 * w;
  if (j0 >= n_sample) return;
  const bool two = j0 + 1 < n_sample;
  const int t0 = (int)(((int64_t)j0 * n_tiles) / n_sample);
  const int t1 = two ? (int)(((int64_t)(j0 + 1) * n_tiles) / n_sample) : t0;
  const half8* p0 = corpus + (int64_t)t0 * (S * 64) + lane;
  const half8* p1 = corpus + (int64_t)t1 * (S * 64) + lane;
  // scores of the two sample tiles: all loads in flight at once (D <= 384), or in chunks of 8
  // k-steps with the query fragments re-read from L2 (wide rows: 4 x D/32 half8 would spill)
  floatx4 sc[2][2];
  if constexpr (S <= 12) {
    half8 a0[S], a1[S], b0[S], b1[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      a0[s] = __builtin_nontemporal_load(p0 + s * 64);
      a1[s] = __builtin_nontemporal_load(p1 + s * 64);
      b0[s] = qfrag[s * 64 + lane];
      b1[s] = qfrag[(S + s) * 64 + lane];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const half8(&a)[S] = u == 0 ? a0 : a1;
      floatx4 acc0 = {0.f, 0.f, 0.f, 0.f};
      floatx4 acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < S; ++s) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b1[s], acc1, 0, 0, 0);
      }
      sc[u][0] = acc0;
      sc[u][1] = acc1;
    }
  } else {
    constexpr int CH = 8;
    static_assert(S % CH == 0, "sample: wide D must be a multiple of 256");
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const half8* p = u == 0 ? p0 : p1;
      floatx4 acc0 = {0.f, 0.f, 0.f, 0.f};
      floatx4 acc1 = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < S / CH; ++c) {
        half8 a[CH], b0[CH], b1[CH];
#pragma unroll
        for (int s = 0; s < CH; ++s) {
          a[s] = __builtin_nontemporal_load(p + (c * CH + s) * 64);
          b0[s] = qfrag[(c * CH + s) * 64 + lane];
          b1[s] = qfrag[(S + c * CH + s) * 64 + lane];
        }
#pragma unroll
        for (int s = 0; s < CH; ++s) {
          acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b0[s], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b1[s], acc1, 0, 0, 0);
        }
      }
      sc[u][0] = acc0;
      sc[u][1] = acc1;
    }
  }
  sample_epilogue<FILTER>(sc, t0, t1, two, j0, lane, tags, filt, n_rows, n_sample, smax);
}

// qprep + sample in ONE launch (D <= 384, one query group; round 3): every workgroup builds the
// 32 queries' B-fragments itself (qprep_slot, 8 slots per wave, into an LDS image of qfrag's
// layout) and samples its tiles against them; workgroup 0 also publishes qn / qfrag / filt / eps
// for the scan and select. The fragments are those qprep_kernel writes (same arithmetic), so
// the maxima, the seeds and every result are unchanged. Why: at small shards each launch of a
// search pass costs ~3 us of throughput (1.25M rows, 4 passes in flight: one more tiny kernel
// per pass measured -1.8%, profiles/r03c_rescan_ab.jsonl); this removes qprep's.
template <int D, bool FILTER>
__global__ __launch_bounds__(256) void qprep_sample_kernel(
    const float* __restrict__ q, int B, const uint32_t* __restrict__ filt_in,
    float* __restrict__ qn, half8* __restrict__ qfrag, uint32_t* __restrict__ filt,
    float* __restrict__ eps, double store_eps, const half8* __restrict__ corpus,
    const uint32_t* __restrict__ tags, int n_rows, int n_tiles, int n_sample,
    float* __restrict__ smax) {
  constexpr int S = steps<D>();
  static_assert(S <= 12, "qprep_sample_kernel: D <= 384");
  __shared__ half8 qf_l[2 * S * 64];
  __shared__ uint32_t filt_l[2 * kQ];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool publish = blockIdx.x == 0;
  for (int b = wid; b < kQ; b += 4)
    qprep_slot<D>(q, B, b, lane, filt_in, qn, qf_l, filt, eps, store_eps, publish, filt_l,
                  publish ? qfrag : nullptr);
  __syncthreads();
  const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(wid);
  const int j0 = 2 * w;
  if (j0 >= n_sample) return;
  const bool two = j0 + 1 < n_sample;
  const int t0 = (int)(((int64_t)j0 * n_tiles) / n_sample);
  const int t1 = two ? (int)(((int64_t)(j0 + 1) * n_tiles) / n_sample) : t0;
  const half8* p0 = corpus + (int64_t)t0 * (S * 64) + lane;
  const half8* p1 = corpus + (int64_t)t1 * (S * 64) + lane;
  floatx4 sc[2][2];
  half8 a0[S], a1[S], b0[S], b1[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    a0[s] = __builtin_nontemporal_load(p0 + s * 64);
    a1[s] = __builtin_nontemporal_load(p1 + s * 64);
    b0[s] = qf_l[s * 64 + lane];
    b1[s] = qf_l[(S + s) * 64 + lane];
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const half8(&a)[S] = u == 0 ? a0 : a1;
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f};
    floatx4 acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b0[s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b1[s], acc1, 0, 0, 0);
    }
    sc[u][0] = acc0;
    sc[u][1] = acc1;
  }
  sample_epilogue<FILTER>(sc, t0, t1, two, j0, lane, tags, filt_l, n_rows, n_sample, smax);
}

constexpr int kSampleGroups = 4;   // query groups of 32 per wide pass (index_capi kMaxGroups)

// D = 1024 with several query groups: one pass over each sample tile for ALL groups (the
// grouped sample_kernel re-read every tile once per group: 4x the bytes at B = 128). Same MFMA
// order per (tile, group, query half) as sample_kernel, so the same maxima.
template <int D, bool FILTER>
__global__ __launch_bounds__(256) void sample_wide_kernel(const half8* __restrict__ corpus,
                                                          const uint32_t* __restrict__ tags,
                                                          const uint32_t* __restrict__ filt,
                                                          const half8* __restrict__ qfrag,
                                                          int n_rows, int n_tiles, int n_sample,
                                                          float* __restrict__ smax, int groups) {
  constexpr int S = steps<D>();
  constexpr int CH = 8;
  static_assert(S % CH == 0, "sample_wide: D must be a multiple of 256");
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j0 = 2 * w;
  if (j0 >= n_sample) return;
  const bool two = j0 + 1 < n_sample;
  const int t0 = (int)(((int64_t)j0 * n_tiles) / n_sample);
  const int t1 = two ? (int)(((int64_t)(j0 + 1) * n_tiles) / n_sample) : t0;
  const half8* p0 = corpus + (int64_t)t0 * (S * 64) + lane;
  const half8* p1 = corpus + (int64_t)t1 * (S * 64) + lane;
  floatx4 acc[kSampleGroups][2][2];
#pragma unroll
  for (int g = 0; g < kSampleGroups; ++g)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[g][u][0] = acc[g][u][1] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < S / CH; ++c) {
    half8 a0[CH], a1[CH];
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      a0[s] = __builtin_nontemporal_load(p0 + (c * CH + s) * 64);
      a1[s] = __builtin_nontemporal_load(p1 + (c * CH + s) * 64);
    }
#pragma unroll
    for (int g = 0; g < kSampleGroups; ++g) {
      if (g < groups) {
        const half8* qg = qfrag + g * (2 * S * 64);
        half8 b0[CH], b1[CH];
#pragma unroll
        for (int s = 0; s < CH; ++s) {
          b0[s] = qg[(c * CH + s) * 64 + lane];
          b1[s] = qg[(S + c * CH + s) * 64 + lane];
        }
#pragma unroll
        for (int s = 0; s < CH; ++s) {
          acc[g][0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[s], b0[s], acc[g][0][0], 0, 0, 0);
          acc[g][0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[s], b1[s], acc[g][0][1], 0, 0, 0);
          acc[g][1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[s], b0[s], acc[g][1][0], 0, 0, 0);
          acc[g][1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[s], b1[s], acc[g][1][1], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kSampleGroups; ++g)
    if (g < groups)
      sample_epilogue<FILTER>(acc[g], t0, t1, two, j0, lane, tags, filt + g * (2 * kQ), n_rows,
                              n_sample, smax + (int64_t)g * kQ * n_sample);
}

// thresh: one 256-thread workgroup per query slot: seed_thr[q] = 32nd largest of
// smax[0..n_waves)[q] (-inf if fewer than 32 are finite). The sample scores come from the
// scan's own MFMA arithmetic (same operands, same accumulation order), so T is a lower bound
// of the 32nd-best scan score and pruning below it never loses a row of the approximate
// top-32. The seed is lowered further, by max(kSeedMargin (1 + |T|), 3 eps_q), so that the
// rows select's tier-1 exactness fallback needs (approximate score >= e_k - eps_q >= T -
// 2 eps_q) were never pruned: select checks L >= seed and otherwise takes the rescan.
constexpr float kSeedMargin = 1e-3f;
constexpr int kMaxSample = 4096;        // sample tiles per query group, D <= 384
constexpr int kMaxSampleWide = 16384;   // D = 1024 (32 KB tiles: 50M rows = 3.1M tiles)
constexpr int kCandCap = 256;   // select: compacted heads at/above the lane-max threshold

template <int MAXS>
__global__ __launch_bounds__(256) void thresh_kernel(const float* __restrict__ smax,
                                                     int n_sample, const float* __restrict__ eps,
                                                     float* __restrict__ seed_thr) {
  // Each lane takes the max over its group of sample tiles (disjoint groups), each wave
  // sorts its 64 group maxima, wave 0 merges the four top-32s: the 32nd best of the group
  // maxima is attained by 32 distinct rows, so it is a valid lower bound.
  __shared__ float w_s[4][32];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  smax += (int64_t)blockIdx.y * kQ * n_sample;   // query group
  seed_thr += blockIdx.y * kQ;
  eps += blockIdx.y * kQ;
  const float* v = smax + (int64_t)q * n_sample;
  float m = kNegInf;
  float x[MAXS / 256];
#pragma unroll
  for (int i = 0; i < MAXS / 256; ++i) x[i] = v[min(tid + 256 * i, n_sample - 1)];
#pragma unroll
  for (int i = 0; i < MAXS / 256; ++i) m = (tid + 256 * i < n_sample) ? fmaxf(m, x[i]) : m;
  int id = tid;
  bitonic_sort64(m, id, lane);
  if (lane < 32) w_s[wid][lane] = m;
  __syncthreads();
  if (wid == 0) {
    float s = lane < 32 ? w_s[0][lane] : kNegInf;
    int i2 = lane;
    for (int w = 1; w < 4; ++w) {
      if (lane >= 32) {
        s = w_s[w][63 - lane];
        i2 = 64 * w + lane;
      }
      bitonic_merge64(s, i2, lane);
    }
    const float t32 = __shfl(s, 31, 64);
    if (lane == 0)
      seed_thr[q] = t32 == kNegInf
                        ? kNegInf
                        : t32 - fmaxf(kSeedMargin * (1.0f + fabsf(t32)), 3.0f * eps[q]);
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
//       list: rescore all of them exactly and emit their top-k.
//     tier 2 (rescan_kernel): otherwise the shard is streamed once more for this query by
//       the rescan kernel launched after every select (its workgroups split the shard); here
//       select only records L and e_k. Only inputs with more than 32 in-band rows inside one
//       wave's share of the tiles (or a seed above L) get there. (Round 2 ran this pass
//       inside select, on the query's one workgroup: a single-CU pass over the whole shard,
//       ~0.1 s at 10M rows — unbounded by the chip's bandwidth; VERDICT/ADVICE r2.)
// ----------------------------------------------------------------------------------------
template <int D, bool FILTER>
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
                                                     const float* __restrict__ rows32) {
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
  __shared__ int verdict;            // 0 exact, 1 tier 1, 2 tier 2
  __shared__ float floor_L, floor_E;
  // query bq of the batch = slot b of query group grp (the scan's per-group lists)
  const int bq = blockIdx.x, grp = bq / kQ, b = bq % kQ;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
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
    float x = lane < 32 ? w_s[0][lane] : kNegInf;
    int64_t id = lane < 32 ? w_i[0][lane] : kId64None;
    for (int v = 1; v < 4; ++v) {
      if (lane >= 32) {
        x = w_s[v][63 - lane];
        id = w_i[v][63 - lane];
      }
      bitonic_merge64(x, id, lane);
    }
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
    float s = lane < 32 ? c_s[0][lane] : kNegInf;
    int id = lane < 32 ? c_i[0][lane] : kIdNone32;
    for (int v = 1; v < 4; ++v) {
      if (lane >= 32) {
        s = c_s[v][63 - lane];
        id = c_i[v][63 - lane];
      }
      bitonic_merge64(s, id, lane);
    }
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
  };

  // ---- 4. order by exact score; 5. exactness check
  if (wid == 0) {
    float s = lane < 32 ? e_s[lane] : kNegInf;
    int id = lane < 32 ? e_i[lane] : kIdNone32;
    bitonic_sort64(s, id, lane);
    int v = 0;
    {
      const float ek = __shfl(s, k - 1, 64);
      const float a32 = c_s[0][kKS - 1];
      const float e = eps[bq];
      float L = 0.0f;
      // a32 == -inf: fewer than 32 finite candidates, i.e. A holds every matching row (a
      // finite seed implies >= 32 rows above it)
      if (!(a32 == kNegInf || ek > a32 + e)) {
        L = ek - e;
        v = (L >= seed_thr[bq]) ? 1 : 2;
      }
      if (lane == 0) {
        verdict = v;
        floor_L = L;
        floor_E = ek;
      }
    }
    if (v == 0) {
      emit(s, id);
      if (lane == 0) fb.tier[bq] = 0;
    }
  }
  __syncthreads();
  if (verdict == 0) return;

  // ---- tier 1: every row with approximate score >= L is in a list (checked below)
  const float L = floor_L;
  if (verdict == 1)
  for (int l = tid; l < n_lists; l += 256) {
    const float h = heads_s[(int64_t)b * n_lists + l];
    if (h != kNegInf && h >= L) {
      const int n = heads_n[(int64_t)b * n_lists + l];
      if (n >= kKS && part_s[at(l, kKS - 1)] >= L) verdict = 2;   // full list: may have dropped one
      const int p = atomicAdd(&n_q, 1);
      qlist[p] = l;
    }
  }
  __syncthreads();
  float rs = kNegInf;   // each wave's running exact top-32 (lanes 0..31, best first)
  int ri = kIdNone32;
  if (verdict == 2) {
    // ---- tier 2: handed to rescan_kernel (launched after every select, many workgroups):
    // its floor L and the k-th exact score of A go to the hand-off record; nothing is emitted
    // here (the rescan writes this query's output)
    if (tid == 0) {
      fb.tier[bq] = 2;
      fb.t2[2 * bq] = L;
      fb.t2[2 * bq + 1] = floor_E;
      atomicAdd(&fb.cnt[1], 1ull);
    }
    return;
  } else {   // tier 1
  if (tid == 0) {
    fb.tier[bq] = 1;
    atomicAdd(&fb.cnt[0], 1ull);
  }
  // each wave: its share of the qualifying lists, entries >= L (a prefix of each sorted
  // list) rescored 8 at a time into the running exact top-32
  const int nql = n_q;
  for (int i = wid; i < nql; i += 4) {
    const int l = qlist[i];
    const int n = heads_n[(int64_t)b * n_lists + l];
    float s = kNegInf;
    int id = kIdNone32;
    if (lane < kKS && lane < n) {
      s = part_s[at(l, lane)];
      id = part_i[at(l, lane)];
    }
    const int m = __popcll(__ballot(lane < kKS && lane < n && s >= L));
    for (int c0 = 0; c0 < m; c0 += 8) {
      int rows[8];
      float es[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = __shfl(id, min(c0 + j, 63), 64);
        rows[j] = c0 + j < m ? r : -1;
      }
      exact_scores_wave<D, 8>(corpus, rows, qq, lane, es, rows32);
      float ns = kNegInf;
      int ni = kIdNone32;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (lane == 32 + j && rows[j] >= 0) {
          ns = es[j];
          ni = rows[j];
        }
      }
      if (lane >= 32) {
        rs = ns;
        ri = ni;
      }
      bitonic_sort64(rs, ri, lane);
    }
  }
  }   // tier 1
  if (lane < 32) {
    c_s[wid][lane] = rs;
    c_i[wid][lane] = ri;
  }
  __syncthreads();
  if (wid == 0) {
    float s = lane < 32 ? c_s[0][lane] : kNegInf;
    int id = lane < 32 ? c_i[0][lane] : kIdNone32;
    for (int v = 1; v < 4; ++v) {
      if (lane >= 32) {
        s = c_s[v][63 - lane];
        id = c_i[v][63 - lane];
      }
      bitonic_merge64(s, id, lane);
    }
    emit(s, id);
  }
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
    const char* tp = cbase + (int64_t)t * (S * 1024) + c * (CS * 1024);
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(tp), 0, CS * 1024, 0x00020000);
#pragma unroll
    for (int s = 0; s < CS; ++s)
      a[s] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, s * 1024, 0));
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

// ----------------------------------------------------------------------------------------
// merge of exact per-shard lists: n_lists x [B][k] -> [B][k]
// ----------------------------------------------------------------------------------------
// Where the lists lie is a fetch policy: fetch(l, b, pos, s, id) loads entry `pos` of list l
// for query b and leaves (s, id) alone where that entry is padding (id < 0).
//
// StackedLists: one contiguous [n_lists][B][k] array, as an RCCL all-gather leaves it. PACKED:
// the [n_lists][B][k][2] int32 (score bits, row) exchange format of rag_index_search_packed
// (one all-gather instead of two); in_s then points at it.
template <bool PACKED>
struct StackedLists {
  const float* __restrict__ in_s;
  const int64_t* __restrict__ in_i;
  int B, k;
  __device__ __forceinline__ void operator()(int l, int b, int pos, float& s, int64_t& id) const {
    const int64_t off = ((int64_t)l * B + b) * k + pos;
    if constexpr (PACKED) {
      const int2 pv = reinterpret_cast<const int2*>(in_s)[off];
      if (pv.y >= 0) {
        s = __int_as_float(pv.x);
        id = pv.y;
      }
    } else {
      const int64_t v = in_i[off];
      if (v >= 0) {
        s = in_s[off];
        id = v;
      }
    }
  }
};

// GatheredLists: n separate packed [B][k][2] lists of shard-local rows (the shard set,
// rag_shardset_search: every shard's list stays where its search or its peer copy wrote it).
// The table travels in the kernel arguments (~1 KB), so no search uploads one; a valid local
// row becomes the global id local * mul + add[l].
constexpr int kMaxShards = 64;   // RAG_MAX_SHARDS
struct GatheredLists {
  const int2* list[kMaxShards];
  int64_t add[kMaxShards];
  int64_t mul;
  int k;
  __device__ __forceinline__ void operator()(int l, int b, int pos, float& s, int64_t& id) const {
    const int2 pv = list[l][(int64_t)b * k + pos];
    if (pv.y >= 0) {
      s = __int_as_float(pv.x);
      id = (int64_t)pv.y * mul + add[l];
    }
  }
  // out_empty[l * B + b] = 1 when list l holds nothing for query b (lists are best-first, so
  // its first id says so): one lane per list, the first kMaxShards threads of the workgroup
  __device__ __forceinline__ void flag_empty(int n_lists, int B, int b, uint8_t* out_empty) const {
    const int l = threadIdx.x;
    if (out_empty && l < n_lists) out_empty[l * B + b] = list[l][(int64_t)b * k].y < 0 ? 1 : 0;
  }
};

// k <= 32: one wave per query; lanes 0-31 hold the running best, lanes 32-63 the next list
template <class Fetch>
__device__ __forceinline__ void merge_exact_body(const Fetch& fetch_list, int n_lists, int k,
                                                 float* __restrict__ out_s,
                                                 int64_t* __restrict__ out_i) {
  const int b = blockIdx.x, lane = threadIdx.x;
  auto fetch = [&](int l, int pos, float& s, int64_t& id) {
    s = kNegInf;
    id = INT64_MAX;
    if (l < n_lists && pos < k) fetch_list(l, b, pos, s, id);
  };
  float s;
  int64_t id;
  if (lane < 32)
    fetch(0, lane, s, id);
  else {
    s = kNegInf;
    id = INT64_MAX;
  }
  for (int l = 1; l < n_lists; ++l) {
    if (lane >= 32) fetch(l, 63 - lane, s, id);
    bitonic_merge64(s, id, lane);
  }
  if (lane < k) {
    const bool ok = s != kNegInf;
    out_s[(int64_t)b * k + lane] = s;
    out_i[(int64_t)b * k + lane] = ok ? id : (int64_t)-1;
  }
}

template <bool PACKED>
__global__ __launch_bounds__(64) void merge_exact_kernel(const float* __restrict__ in_s,
                                                         const int64_t* __restrict__ in_i,
                                                         int n_lists, int B, int k,
                                                         float* __restrict__ out_s,
                                                         int64_t* __restrict__ out_i) {
  merge_exact_body(StackedLists<PACKED>{in_s, in_i, B, k}, n_lists, k, out_s, out_i);
}

__global__ __launch_bounds__(64) void merge_gather_kernel(const GatheredLists lists, int n_lists,
                                                          int B, float* __restrict__ out_s,
                                                          int64_t* __restrict__ out_i,
                                                          uint8_t* __restrict__ out_empty) {
  merge_exact_body(lists, n_lists, lists.k, out_s, out_i);
  lists.flag_empty(n_lists, B, blockIdx.x, out_empty);
}

// the same merge for 32 < k <= kLkMerge (the large-k path's exchange, round 5): one 256-thread
// workgroup per query keeps the running best k in LDS (ms / mi, 2 * kLkMerge entries each);
// each further list's k entries go beside them and a bitonic sort of the 2k by (score desc,
// row asc) keeps the first k
constexpr int kLkMerge = 4096;
template <class Fetch>
__device__ __forceinline__ void merge_large_body(const Fetch& fetch_list, int n_lists, int k,
                                                 float* ms, int64_t* mi,
                                                 float* __restrict__ out_s,
                                                 int64_t* __restrict__ out_i) {
  const int b = blockIdx.x;
  int P = 1;
  while (P < 2 * k) P <<= 1;
  for (int i = threadIdx.x; i < P; i += 256) {
    float s = kNegInf;
    int64_t id = INT64_MAX;
    if (i < k) fetch_list(0, b, i, s, id);
    ms[i] = s;
    mi[i] = id;
  }
  // (each per-shard list is sorted best-first already: one list needs no sort)
  for (int l = 1; l < n_lists; ++l) {
    __syncthreads();
    for (int i = threadIdx.x; i < P - k; i += 256) {
      float s = kNegInf;
      int64_t id = INT64_MAX;
      if (i < k) fetch_list(l, b, i, s, id);
      ms[k + i] = s;
      mi[k + i] = id;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = threadIdx.x; i < P; i += 256) {
          const int j = i ^ stride;
          if (j > i) {
            const bool best_first = (i & size) == 0;
            const float a = ms[i], c = ms[j];
            const int64_t ia = mi[i], ic = mi[j];
            const bool a_better = (a > c) || (a == c && ia < ic);
            if (best_first != a_better) {
              ms[i] = c;
              ms[j] = a;
              mi[i] = ic;
              mi[j] = ia;
            }
          }
        }
        __syncthreads();
      }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += 256) {
    const float s = ms[j];
    const bool ok = s != kNegInf;
    out_s[(int64_t)b * k + j] = s;
    out_i[(int64_t)b * k + j] = ok ? mi[j] : (int64_t)-1;
  }
}

template <bool PACKED>
__global__ __launch_bounds__(256) void merge_large_kernel(const float* __restrict__ in_s,
                                                          const int64_t* __restrict__ in_i,
                                                          int n_lists, int B, int k,
                                                          float* __restrict__ out_s,
                                                          int64_t* __restrict__ out_i) {
  __shared__ float ms[2 * kLkMerge];
  __shared__ int64_t mi[2 * kLkMerge];
  merge_large_body(StackedLists<PACKED>{in_s, in_i, B, k}, n_lists, k, ms, mi, out_s, out_i);
}

__global__ __launch_bounds__(256) void merge_gather_large_kernel(
    const GatheredLists lists, int n_lists, int B, float* __restrict__ out_s,
    int64_t* __restrict__ out_i, uint8_t* __restrict__ out_empty) {
  __shared__ float ms[2 * kLkMerge];
  __shared__ int64_t mi[2 * kLkMerge];
  merge_large_body(lists, n_lists, lists.k, ms, mi, out_s, out_i);
  lists.flag_empty(n_lists, B, blockIdx.x, out_empty);
}

// Unpacked shard-set path (k > kLkMerge, or the full exact pass): the stacked local ids
// [n_lists][B][k] become global in place, list l's id -> id * mul + l (-1 stays -1), and
// out_empty[l * B + b] (may be NULL) says whether list l holds nothing for query b.
// Grid: (blocks over B * k, n_lists).
__global__ __launch_bounds__(256) void remap_ids_kernel(int64_t* __restrict__ ids, int B, int k,
                                                        int64_t mul,
                                                        uint8_t* __restrict__ out_empty) {
  const int l = blockIdx.y;
  const int64_t n = (int64_t)B * k;
  int64_t* list = ids + (int64_t)l * n;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const int64_t id = list[j];
    if (id >= 0) list[j] = id * mul + l;
    if (out_empty && j % k == 0) out_empty[(int64_t)l * B + j / k] = id < 0 ? 1 : 0;
  }
}

// ----------------------------------------------------------------------------------------
// export: tile16 -> row-major fp16 (one thread per 8-half chunk)
// ----------------------------------------------------------------------------------------
template <int D>
__global__ void export_kernel(const half8* __restrict__ corpus, int64_t row0, int64_t n,
                              half8* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * (D / 8)) return;
  const int64_t i = idx / (D / 8);
  const int c = (int)(idx % (D / 8));
  const int64_t row = row0 + i;
  const int64_t t = row >> 4;
  const int r = (int)(row & 15);
  out[idx] = corpus[t * (steps<D>() * 64) + (c >> 2) * 64 + (c & 3) * 16 + r];
}

// ----------------------------------------------------------------------------------------
// import: row-major fp16 -> tile16, stored bits unchanged (persistence: loading a saved shard
// must not renormalise already-normalised rows)
// ----------------------------------------------------------------------------------------
template <int D>
__global__ void import_kernel(const half8* __restrict__ in, int64_t row0, int64_t n,
                              half8* __restrict__ corpus) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * (D / 8)) return;
  const int64_t i = idx / (D / 8);
  const int c = (int)(idx % (D / 8));
  const int64_t row = row0 + i;
  corpus[(row >> 4) * (steps<D>() * 64) + (c >> 2) * 64 + (c & 3) * 16 + (row & 15)] = in[idx];
}

// import, fp32 storage: row-major fp32 rows (already normalised) -> rows32 unchanged and the
// scan's fp16 tile16 copy by the same RNE conversion as upsert (f32_to_f16), so a reloaded
// index is bit-identical to the one that was saved
template <int D>
__global__ void import32_kernel(const float* __restrict__ in, int64_t row0, int64_t n,
                                half8* __restrict__ corpus, float* __restrict__ rows32) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * (D / 8)) return;
  const int64_t i = idx / (D / 8);
  const int c = (int)(idx % (D / 8));
  const int64_t row = row0 + i;
  const float* src = in + i * D + 8 * c;
  half8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    rows32[row * D + 8 * c + j] = src[j];
    h[j] = f32_to_f16(src[j]);
  }
  corpus[(row >> 4) * (steps<D>() * 64) + (c >> 2) * 64 + (c & 3) * 16 + (row & 15)] = h;
}

// ----------------------------------------------------------------------------------------
// Exact top-k for RAG_MAX_K < k <= RAG_MAX_K_LARGE (round 5): Qdrant's
// query_points takes any `limit` (reference main.py:215,232-237); the scan's per-wave lists
// hold 32. A pass of <= 32 queries runs, after qprep:
//  1. sample_kernel over n_sample tiles spread over the shard (per tile and query the max MFMA
//     score a of its matching rows) and lk_bound_kernel: T = the k-th largest of those maxima.
//     They come from k distinct rows, each with exact score e >= a - eps (qprep's bound), so
//     the k-th best exact score e_k >= T - eps and every exact top-k row has
//     a >= e - eps >= T - 2 eps = thr. (Fewer than k finite maxima: thr = -inf.)
//  2. lk_collect_kernel: every tile MFMA-scored; each matching row with a >= thr is appended
//     to its query's candidate list (at most kLkCap kept; the counter counts them all).
//  3. lk_final_kernel: per query, the candidates are rescored exactly (exact_scores_wave: the
//     canonical fp64 order of select / the oracle) and the k best by (score desc, row asc) are
//     emitted. They contain the exact top-k, so the result is exact. If the list overflowed,
//     the k-th best exact score e' among the kept candidates (real rows: e_k >= e') gives a
//     tighter thr = e' - eps, and steps 2-3 run again for that query (kLkRounds launches in
//     all; later ones return at once unless a query was marked). A query still overflowing in
//     the last round (more than kLkCap rows tied within 2 eps of its k-th best) is recorded
//     as unanswered (tier 3, rag_index_unanswered), never silently truncated.
// ----------------------------------------------------------------------------------------
constexpr int kLkMax = 4096;       // largest k (ragmi.h RAG_MAX_K_LARGE)
constexpr int kLkCap = 16384;      // candidates kept per query and round (exact scores in LDS)
constexpr int kLkRounds = 3;
constexpr int kLkSampleMax = 16384;

// order-preserving uint32 key of a float (larger float -> larger key; -inf smallest finite)
__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the kk-th largest of the n keys key(i), 1 <= kk <= n (multiplicity counted; 256 threads):
// a radix select over 8-bit digits, most significant first — each pass an LDS histogram of the
// keys that match the digits chosen so far, then wave 0 scans the 256 bins from the top (a
// wave-wide prefix sum) for the digit where the count reaches kk. 4 passes where a bisection
// over the 32 key bits took 32 (round 5: lk_bound 166 us for 16384 keys).
template <typename KeyFn>
__device__ uint32_t radix_kth_key(KeyFn key, int n, int kk, int* hist, int* sh) {
  uint32_t prefix = 0, mask = 0;
  int need = kk;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const uint32_t v = key(i);
      if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1);
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      // lane l holds digits 255 - 4l .. 252 - 4l (descending); inclusive scan over lanes
      const int l = threadIdx.x;
      int bv[4], sl = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bv[j] = hist[255 - 4 * l - j];
        sl += bv[j];
      }
      int incl = sl;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (l >= o) incl += t;
      }
      const int excl = incl - sl;
      if (excl < need && need <= incl) {       // exactly one lane
        int c = excl, d = 255 - 4 * l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          d = 255 - 4 * l - j;
          if (c + bv[j] >= need) break;
          c += bv[j];
        }
        sh[0] = d;
        sh[1] = need - c;
      }
    }
    __syncthreads();
    prefix |= (uint32_t)sh[0] << shift;
    mask |= 255u << shift;
    need = sh[1];
    __syncthreads();
  }
  return prefix;
}

// per query q < B: thr[q] from the sample maxima smax [32][n_sample]; resets the round state
__global__ __launch_bounds__(256) void lk_bound_kernel(const float* __restrict__ smax,
                                                       int n_sample, int k,
                                                       const float* __restrict__ eps,
                                                       float* __restrict__ thr,
                                                       int* __restrict__ cnt,
                                                       int* __restrict__ again,
                                                       int* __restrict__ need) {
  __shared__ uint32_t keys[kLkSampleMax];
  __shared__ int red, hist[256], sh[2];
  const int q = blockIdx.x;
  int fin = 0;
  for (int i = threadIdx.x; i < n_sample; i += 256) {
    const float v = smax[(int64_t)q * n_sample + i];
    keys[i] = fkey(v);
    fin += v != kNegInf;
  }
  if (threadIdx.x == 0) red = 0;
  __syncthreads();
  atomicAdd(&red, fin);
  __syncthreads();
  const int n_fin = red;
  __syncthreads();
  float th = kNegInf;
  if (n_fin >= k) {
    const float T = fkey_inv(radix_kth_key([&](int i) { return keys[i]; }, n_sample, k, hist, sh));
    const double d = (double)T - 2.0 * (double)eps[q];
    th = (float)d;
    if ((double)th > d) th = nextafterf(th, kNegInf);   // round toward -inf
  }
  if (threadIdx.x == 0) {
    thr[q] = th;
    cnt[q] = 0;
    again[q] = 1;     // round 0 processes every query
  }
  if (q == 0 && threadIdx.x < kLkRounds) need[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;
}

// every tile against the pass's queries: append matching rows with a >= thr[q]. One wave per
// tile per step (grid-stride). round > 0: only if the previous round marked a query, and only
// the marked queries.
template <int D, bool FILTER>
__global__ __launch_bounds__(256) void lk_collect_kernel(const half8* __restrict__ corpus,
                                                         const uint32_t* __restrict__ tags,
                                                         const uint32_t* __restrict__ filt,
                                                         const half8* __restrict__ qfrag,
                                                         int n_rows, int n_tiles, int B,
                                                         const float* __restrict__ thr,
                                                         int* __restrict__ cnt,
                                                         int* __restrict__ cand,
                                                         const int* __restrict__ again,
                                                         const int* __restrict__ need, int round) {
  constexpr int S = steps<D>();
  if (!need[round]) return;
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * 4;
  const int w0 = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // this lane's two queries: (l & 15) and 16 + (l & 15)
  const int qa = lane & 15, qb = 16 + (lane & 15);
  const bool la = qa < B && again[qa], lb = qb < B && again[qb];
  const float ta = la ? thr[qa] : __builtin_inff(), tb = lb ? thr[qb] : __builtin_inff();
  uint32_t fma_ = 0, fva = 0, fmb = 0, fvb = 0;
  if constexpr (FILTER) {
    fma_ = filt[2 * qa];
    fva = filt[2 * qa + 1];
    fmb = filt[2 * qb];
    fvb = filt[2 * qb + 1];
  }
  // D <= 384: the two query groups' fragments stay in registers for the whole launch (24
  // half8); reloading them per tile tripled the vector-memory instructions per tile
  // (k = 33 collect 1.34 ms vs the scan's 1.08 over the same 10M rows, round 5)
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
    const half8* p = corpus + (int64_t)t * (S * 64) + lane;
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    constexpr int CH = S <= 12 ? S : 8;
    static_assert(S % CH == 0, "k-step chunks");
    for (int c = 0; c < S / CH; ++c) {
      half8 a[CH], b0[CH], b1[CH];
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        a[s] = __builtin_nontemporal_load(p + (c * CH + s) * 64);
        if constexpr (QREG) {
          b0[s] = qra[c * CH + s];
          b1[s] = qrb[c * CH + s];
        } else {
          b0[s] = qfrag[(c * CH + s) * 64 + lane];
          b1[s] = qfrag[(S + c * CH + s) * 64 + lane];
        }
      }
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], b1[s], acc1, 0, 0, 0);
      }
    }
    const int rbase = t * kTileRows + 4 * (lane >> 4);
    uint4 tg = {0u, 0u, 0u, 0u};
    if constexpr (FILTER) tg = *reinterpret_cast<const uint4*>(tags + rbase);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + r;
      if (row >= n_rows) break;
      bool oka = acc0[r] >= ta, okb = acc1[r] >= tb;
      if constexpr (FILTER) {
        const uint32_t tr = r == 0 ? tg.x : r == 1 ? tg.y : r == 2 ? tg.z : tg.w;
        oka = oka && ((tr & fma_) == fva);
        okb = okb && ((tr & fmb) == fvb);
      }
      if (oka) {
        const int pos = atomicAdd(&cnt[qa], 1);
        if (pos < kLkCap) cand[qa * kLkCap + pos] = row;
      }
      if (okb) {
        const int pos = atomicAdd(&cnt[qb], 1);
        if (pos < kLkCap) cand[qb * kLkCap + pos] = row;
      }
    }
  }
}

// per query (workgroup q < B): exact rescoring of the candidates, then the top-k by
// (score desc, row asc) -> output; on overflow a tighter thr and another round (see above).
// 3a. exact scores of query q's kept candidates (lk_collect's list), 256 candidates per
// workgroup, grid (kLkCap / 256, B): the same canonical fp64 order as select / the oracle
// (exact_scores_wave), 8 rows per wave per round trip. One workgroup per query rescored
// ~1,300 candidates at k = 33 in ~0.6 ms of serial round trips (round 5).
template <int D>
__global__ __launch_bounds__(256) void lk_rescore_kernel(const half8* __restrict__ corpus,
                                                         const float* __restrict__ qn,
                                                         const int* __restrict__ cnt,
                                                         const int* __restrict__ cand,
                                                         const int* __restrict__ again,
                                                         const int* __restrict__ need, int round,
                                                         float* __restrict__ es_g,
                                                         const float* __restrict__ rows32) {
  const int q = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (!need[round] || !again[q]) return;
  const int n = min(cnt[q], kLkCap);
  const int c0 = blockIdx.x * 256, c1 = min(n, c0 + 256);
  if (c0 >= c1) return;
  const int* cq = cand + (int64_t)q * kLkCap;
  const float* qq = qn + (int64_t)q * D;
  constexpr int NC = 8;
  for (int i0 = c0 + wid * NC; i0 < c1; i0 += 4 * NC) {
    int rows[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) rows[j] = i0 + j < c1 ? cq[i0 + j] : -1;
    float sc[NC];
    exact_scores_wave<D, NC>(corpus, rows, qq, lane, sc, rows32);
    if (lane == 0)
#pragma unroll
      for (int j = 0; j < NC; ++j)
        if (i0 + j < c1) es_g[(int64_t)q * kLkCap + i0 + j] = sc[j];
  }
}

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

template <int D>
__global__ __launch_bounds__(256) void lk_final_kernel(const half8* __restrict__ corpus,
                                                       const float* __restrict__ qn, int k,
                                                       int* __restrict__ cnt,
                                                       const int* __restrict__ cand,
                                                       const float* __restrict__ es_g,
                                                       const float* __restrict__ eps,
                                                       float* __restrict__ thr,
                                                       int* __restrict__ again,
                                                       int* __restrict__ need, int round,
                                                       int* __restrict__ tier,
                                                       unsigned long long* __restrict__ fb_cnt,
                                                       int64_t id_offset,
                                                       float* __restrict__ out_s,
                                                       int64_t* __restrict__ out_i,
                                                       int32_t* __restrict__ out_packed,
                                                       const float* __restrict__ rows32) {
  __shared__ float es[kLkCap];            // exact scores of the kept candidates
  __shared__ float ss[kLkMax];            // the selected entries (sorted in place)
  __shared__ int si[kLkMax];
  __shared__ int red, red2, verdict, hist[256], sh[2];
  const int q = blockIdx.x;
  if (!need[round] || !again[q]) return;
  const int total = cnt[q];
  const int n = min(total, kLkCap);
  const int* cq = cand + (int64_t)q * kLkCap;
  // 1. the kept candidates' exact scores (lk_rescore_kernel, spread over many workgroups)
  for (int i = threadIdx.x; i < n; i += 256) es[i] = es_g[(int64_t)q * kLkCap + i];
  __syncthreads();
  // block-wide count of the candidates passing pred(i)
  auto count_if = [&](auto pred) -> int {
    int m = 0;
    for (int i = threadIdx.x; i < n; i += 256) m += pred(i) ? 1 : 0;
    if (threadIdx.x == 0) red = 0;
    __syncthreads();
    atomicAdd(&red, m);
    __syncthreads();
    const int r = red;
    __syncthreads();
    return r;
  };
  // 2. tkey = the key of the kk-th best exact score among the kept candidates
  const int kk = min(k, n);
  uint32_t tkey = 0;
  if (kk > 0) tkey = radix_kth_key([&](int i) { return fkey(es[i]); }, n, kk, hist, sh);
  if (total > kLkCap) {
    // overflow: the kept candidates are real rows, so e_k >= fkey_inv(tkey) and every exact
    // top-k row has a >= that - eps: a tighter threshold for the next round
    if (threadIdx.x == 0) {
      verdict = 0;                            // 0: unanswered, 1: another round
      if (round + 1 < kLkRounds && n >= k) {
        const double d = (double)fkey_inv(tkey) - (double)eps[q];
        float th = (float)d;
        if ((double)th > d) th = nextafterf(th, kNegInf);
        if (th > thr[q]) {
          thr[q] = th;
          cnt[q] = 0;
          need[round + 1] = 1;                // (again[q] stays 1)
          verdict = 1;
        }
      }
      if (!verdict) {                         // no progress possible: tier 3
        tier[q] = 3;
        atomicAdd(&fb_cnt[2], 1ull);
        again[q] = 0;
      }
    }
    __syncthreads();
    if (verdict) return;
    for (int j = threadIdx.x; j < k; j += 256) {
      if (out_packed) {
        out_packed[((int64_t)q * k + j) * 2] = __float_as_int(kNegInf);
        out_packed[((int64_t)q * k + j) * 2 + 1] = -1;
      } else {
        out_s[(int64_t)q * k + j] = kNegInf;
        out_i[(int64_t)q * k + j] = -1;
      }
    }
    return;
  }
  // 3. the selected set: every candidate with key > tkey, then the ties (key == tkey) by row
  //    ascending up to kk — rcut = the largest admitted tie row
  const int gt = kk > 0 ? count_if([&](int i) { return fkey(es[i]) > tkey; }) : 0;
  const int need_eq = kk - gt;
  int rcut = -1;
  if (need_eq > 0) {
    // the largest r with #{ties with row < r} < need_eq: then row r is a tie row and exactly
    // need_eq ties have row <= r (rows are distinct within a round)
    uint32_t r = 0;
    for (int bit = 30; bit >= 0; --bit) {
      const uint32_t c = r | (1u << bit);
      if (count_if([&](int i) { return fkey(es[i]) == tkey && (uint32_t)cq[i] < c; }) < need_eq)
        r = c;
    }
    rcut = (int)r;
  }
  if (threadIdx.x == 0) red2 = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) {
    const float s = es[i];
    const uint32_t key = fkey(s);
    const int row = cq[i];
    if (kk > 0 && (key > tkey || (key == tkey && row <= rcut))) {
      const int p = atomicAdd(&red2, 1);
      if (p < kLkMax) {
        ss[p] = s;
        si[p] = row;
      }
    }
  }
  __syncthreads();
  // 4. bitonic sort of the kk selected entries by (score desc, row asc), padded to P
  int P = 1;
  while (P < kk) P <<= 1;
  for (int i = kk + threadIdx.x; i < P; i += 256) {
    ss[i] = kNegInf;
    si[i] = kIdNone32;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < P; i += 256) {
        const int j = i ^ stride;
        if (j > i) {
          const bool best_first = (i & size) == 0;
          const float a = ss[i], b = ss[j];
          const int ia = si[i], ib = si[j];
          const bool a_better = (a > b) || (a == b && ia < ib);
          if (best_first != a_better) {
            ss[i] = b;
            ss[j] = a;
            si[i] = ib;
            si[j] = ia;
          }
        }
      }
      __syncthreads();
    }
  for (int j = threadIdx.x; j < k; j += 256) {
    const bool ok = j < kk;
    const float s = ok ? ss[j] : kNegInf;
    const int id = ok ? si[j] : -1;
    if (out_packed) {
      out_packed[((int64_t)q * k + j) * 2] = __float_as_int(s);
      out_packed[((int64_t)q * k + j) * 2 + 1] = ok ? (int32_t)(id + id_offset) : -1;
    } else {
      out_s[(int64_t)q * k + j] = s;
      out_i[(int64_t)q * k + j] = ok ? (int64_t)id + id_offset : (int64_t)-1;
    }
  }
  if (threadIdx.x == 0) {
    tier[q] = 0;
    again[q] = 0;
  }
}

// ----------------------------------------------------------------------------------------
// Exact top-k for ANY k (round 6, VERDICT r5 item 7 / ADVICE r5): Qdrant's query_points
// answers any `limit` (reference main.py:215,232-239, whose `except Exception` would turn a
// refusal into "no documents"). For k > RAG_MAX_K_LARGE — and for a large-k query that more
// than kLkCap near-ties left unanswered — one query at a time:
//  1. full_score_kernel: every row scored exactly (exact_scores_wave, the canonical fp64
//     order of select / lk_final / the oracle); key = fkey(score) for a row that passes the
//     query's filter, 0 (below every real score's key) for one that does not; value = row.
//  2. a stable radix sort of (key, row) pairs, keys descending (hipcub): equal keys keep
//     their row-ascending input order, i.e. (score desc, row asc) — the oracle's order.
//  3. full_emit_kernel: the first k entries (the n_match matching rows first), -inf / -1
//     padding past n_match.
// A rare path by construction (≈3 ms per query at 10M rows); no candidate list, no
// threshold, so nothing can overflow.
// ----------------------------------------------------------------------------------------
template <int D, bool FILTER>
__global__ __launch_bounds__(256) void full_score_kernel(const half8* __restrict__ corpus,
                                                         const uint32_t* __restrict__ tags,
                                                         const uint32_t* __restrict__ filt,
                                                         const float* __restrict__ qq,
                                                         int n_rows,
                                                         const float* __restrict__ rows32,
                                                         uint32_t* __restrict__ keys,
                                                         int* __restrict__ vals,
                                                         int* __restrict__ n_match) {
  constexpr int NC = 8;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = gridDim.x * 4;
  uint32_t fm = 0, fv = 0;
  if constexpr (FILTER) {
    fm = filt[0];
    fv = filt[1];
  }
  int m = 0;
  for (int r0 = wave * NC; r0 < n_rows; r0 += nw * NC) {
    int rows[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) rows[i] = r0 + i < n_rows ? r0 + i : -1;
    float sc[NC];
    exact_scores_wave<D, NC>(corpus, rows, qq, lane, sc, rows32);
    float s = sc[0];
#pragma unroll
    for (int i = 1; i < NC; ++i)
      if (lane == i) s = sc[i];
    const int row = r0 + lane;
    if (lane < NC && row < n_rows) {
      bool ok = true;
      if constexpr (FILTER) ok = (tags[row] & fm) == fv;
      if (s == 0.0f) s = 0.0f;               // -0 and +0 compare equal: one key for both
      keys[row] = ok ? fkey(s) : 0u;
      vals[row] = row;
      m += ok ? 1 : 0;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m += __shfl_xor(m, d, 64);
  if (lane == 0 && m > 0) atomicAdd(n_match, m);
}

__global__ __launch_bounds__(256) void full_emit_kernel(const uint32_t* __restrict__ keys,
                                                        const int* __restrict__ vals,
                                                        const int* __restrict__ n_match, int k,
                                                        int64_t id_offset,
                                                        float* __restrict__ out_s,
                                                        int64_t* __restrict__ out_i,
                                                        int32_t* __restrict__ out_packed) {
  const int m = *n_match;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < k;
       j += (int64_t)gridDim.x * 256) {
    const bool ok = j < m;
    const float s = ok ? fkey_inv(keys[j]) : kNegInf;
    const int64_t id = ok ? (int64_t)vals[j] + id_offset : (int64_t)-1;
    if (out_packed) {
      out_packed[2 * j] = __float_as_int(s);
      out_packed[2 * j + 1] = (int32_t)id;
    } else {
      out_s[j] = s;
      out_i[j] = id;
    }
  }
}

// Merge for k > kLkMerge (round 6: the sharded search of a `limit` past the large-k pass's
// exchange, ragmi.dist.ShardedIndex): per query, the n_lists * k entries (padding: id < 0) are
// ordered by three stable radix sorts (hipcub, one instantiation: 32-bit keys descending) —
// by the complement of the id's low word, then of its high word (so: id ascending), then by
// the order-preserving score key — so ties stay id-ascending: the (score desc, id asc) order
// of merge_exact_kernel / merge_large_kernel for any k. Padding gets key 0 in every pass, below
// every id and every score.
template <bool PACKED>
__global__ __launch_bounds__(256) void merge_any_ids_kernel(const float* __restrict__ in_s,
                                                            const int64_t* __restrict__ in_i,
                                                            int n_lists, int B, int k, int b,
                                                            const int* __restrict__ pos_in,
                                                            int word,
                                                            uint32_t* __restrict__ key,
                                                            int* __restrict__ pos) {
  const int64_t n = (int64_t)n_lists * k;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const int p = pos_in ? pos_in[j] : (int)j;
    const int64_t off = ((int64_t)(p / k) * B + b) * k + p % k;
    int64_t id;
    if constexpr (PACKED) id = reinterpret_cast<const int2*>(in_s)[off].y;
    else id = in_i[off];
    const uint32_t w = (uint32_t)((uint64_t)id >> (32 * word));
    key[j] = id >= 0 ? ~w : 0u;
    pos[j] = p;
  }
}

template <bool PACKED>
__global__ __launch_bounds__(256) void merge_any_scores_kernel(const float* __restrict__ in_s,
                                                               const int64_t* __restrict__ in_i,
                                                               int n_lists, int B, int k, int b,
                                                               const int* __restrict__ pos_in,
                                                               uint32_t* __restrict__ key,
                                                               int* __restrict__ pos) {
  const int64_t n = (int64_t)n_lists * k;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const int p = pos_in[j];
    const int64_t off = ((int64_t)(p / k) * B + b) * k + p % k;
    float sc;
    int64_t id;
    if constexpr (PACKED) {
      const int2 pv = reinterpret_cast<const int2*>(in_s)[off];
      sc = __int_as_float(pv.x);
      id = pv.y;
    } else {
      sc = in_s[off];
      id = in_i[off];
    }
    if (sc == 0.0f) sc = 0.0f;                  // -0 and +0: one key
    key[j] = id >= 0 ? fkey(sc) : 0u;
    pos[j] = p;
  }
}

template <bool PACKED>
__global__ __launch_bounds__(256) void merge_any_emit_kernel(const float* __restrict__ in_s,
                                                             const int64_t* __restrict__ in_i,
                                                             int B, int k, int b,
                                                             const uint32_t* __restrict__ key,
                                                             const int* __restrict__ pos,
                                                             float* __restrict__ out_s,
                                                             int64_t* __restrict__ out_i) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < k; j += (int64_t)gridDim.x * 256) {
    const int p = pos[j];
    const int64_t off = ((int64_t)(p / k) * B + b) * k + p % k;
    float sc = kNegInf;
    int64_t id = -1;
    if (key[j] != 0u) {
      if constexpr (PACKED) {
        const int2 pv = reinterpret_cast<const int2*>(in_s)[off];
        sc = __int_as_float(pv.x);
        id = pv.y;
      } else {
        sc = in_s[off];
        id = in_i[off];
      }
    }
    out_s[(int64_t)b * k + j] = sc;
    out_i[(int64_t)b * k + j] = id;
  }
}

}  // namespace ragmi
