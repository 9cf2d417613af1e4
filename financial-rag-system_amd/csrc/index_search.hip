// index_search.hip — the search side of the flat index's extern "C" boundary (declared in
// include/ragmi.h): the workspace tables, the launch sequence of a search pass (qprep -> scan ->
// select) and of the large-k and full passes, the rag_index_search* entry points, the merges of
// and re-selections over their lists, the scan's probes and profile readers, CU-mask streams.
// Entry points enqueue on the caller's stream or (*_host) stage through device memory.
#include "index_host.hpp"
// one header per pass, in dependency order (why merge and reselect are here: DESIGN.md §4c)
#include "prep_kernels.hip"
#include "scan_kernels.hip"
#include "seed_kernels.hip"
#include "certify_kernels.hip"
#include "merge_kernels.hip"
#include "largek_kernels.hip"
#include "reco_kernels.hip"
#include "discover_kernels.hip"
#include "sparse_kernels.hip"
#include "reselect_kernels.hip"
#include "formula_kernels.hip"

#include <hipcub/hipcub.hpp>

using namespace ragmi;

namespace {

// *avg_ms = device time per call of `reps` back-to-back calls of `one` (launches on the null
// stream), after one warm-up call
template <typename F>
int time_launches(int reps, F&& one, double* avg_ms) {
  EventPair ev;
  RAG_HIP(ev.create());
  one();  // warm
  RAG_HIP(hipEventRecord(ev.a, nullptr));
  for (int r = 0; r < reps; ++r) one();
  RAG_HIP(hipEventRecord(ev.b, nullptr));
  RAG_HIP(hipEventSynchronize(ev.b));
  float ms = 0.f;
  RAG_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
  RAG_HIP(hipGetLastError());
  *avg_ms = ms / reps;
  return RAG_OK;
}

// the full pass's and merge_any_k's sort (stable, keys descending): the one hipcub instantiation
hipError_t sort_pairs_desc(void* tmp, size_t tmp_bytes, const uint32_t* k_in, uint32_t* k_out,
                           const int* v_in, int* v_out, int n, hipStream_t st) {
  return hipcub::DeviceRadixSort::SortPairsDescending(tmp, tmp_bytes, k_in, k_out, v_in, v_out, n,
                                                      0, 32, st);
}

// The large-k buffers, allocated together on first use (ensure_lk)
std::array<WsBuf, 7> lk_buffers(Workspace& w) {
  const size_t Q = kQ;
  return {ws_buf(w.lk_smax, Q * kLkSampleMax * 4), ws_buf(w.lk_thr, Q * 4),
          ws_buf(w.lk_cnt, Q * 4),                 ws_buf(w.lk_again, Q * 4),
          ws_buf(w.lk_need, 64),                   ws_buf(w.lk_cand, Q * kLkCap * 4),
          ws_buf(w.lk_es, Q * kLkCap * 4)};
}

// The recommend buffers, allocated together on first use (ensure_reco): the query block
// [32][1024] + the AVERAGE_VECTOR target [1024], and the parameter words (kRecoPar*)
constexpr size_t kRecoQFloats = (size_t)(kQ + 1) * 1024;
std::array<WsBuf, 2> reco_buffers(Workspace& w) {
  return {ws_buf(w.reco_q, kRecoQFloats * 4), ws_buf(w.reco_par, 64, true)};
}

// The buffers every Workspace of `h` holds from creation to destruction (h->dim, groups and
// max_wgs set), in allocation order (alloc_workspaces: one hipMalloc each; free_workspaces)
std::array<WsBuf, 25> ws_buffers(const rag_index* h, Workspace& w) {
  const size_t G = (size_t)h->groups, Q = kQ, dim = (size_t)h->dim;
  const size_t max_lists = (size_t)std::min(h->max_wgs * kWavesPerWG, kMaxLists);
  return {ws_buf(w.qn, G * Q * dim * 4),
          ws_buf(w.qfrag, G * 2 * (dim / 32) * 64 * 16),
          ws_buf(w.filt, G * Q * 2 * 4),
          ws_buf(w.smax, G * (dim > 384 ? kMaxSampleWide : kMaxSample) * Q * 4),
          ws_buf(w.heads_s, G * kMaxLists * Q * 4),
          ws_buf(w.heads_i, G * kMaxLists * Q * 4),
          ws_buf(w.heads_n, G * kMaxLists * Q * 4),
          ws_buf(w.seed, G * Q * 4),
          ws_buf(w.part_s, G * max_lists * Q * kKS * 4),
          ws_buf(w.part_i, G * max_lists * Q * kKS * 4),
          ws_buf(w.progress, G * kMaxLists * 4),
          ws_buf(w.eps, G * Q * 4),
          ws_buf(w.fb_tier, G * Q * 4, true),
          ws_buf(w.fb_cnt, 32, true),
          ws_buf(w.tileq, 8 * kTileQStride * 4, true),
          ws_buf(w.t2, G * Q * 2 * 4),
          ws_buf(w.t2_s, G * Q * kRescanMaxWG * 32 * 4),
          ws_buf(w.t2_i, G * Q * kRescanMaxWG * 32 * 4),
          ws_buf(w.t2_tk, 64, true),
          ws_buf(w.qfrag8, h->copy[kCopy8].data ? 4 * (dim / 64) * 64 * 16 : 0),
          ws_buf(w.qp8, h->copy[kCopy8].data ? Q * 4 * 4 : 0),
          ws_buf(w.eps8, h->copy[kCopy8].data ? Q * 4 : 0),
          // (an index that keeps the int8 copy may start a 6-bit one later: ensure_copy6)
          ws_buf(w.bd_rec, h->copy[kCopy8].data ? Q * kBandRec * 4 : 0),
          ws_buf(w.bd_pub, h->copy[kCopy8].data ? Q * kBandSlicesMax * kBandPub * 4 : 0),
          ws_buf(w.bd_tk, h->copy[kCopy8].data ? Q * 4 : 0, true)};
}

// qprep's extra error-bound term for fp32 storage (prep_kernels.hip qprep_kernel): the exact
// score reads the fp32 row c32, the scan its fp16 rounding c: |sum (c - c32) qn| <=
// ||c - c32|| ||qn|| <= (2^-11 ||c32|| + 2^-25 sqrt(D)) (1 + 2^-20), ||c32|| <= 1 + 2^-20
double store_eps(const rag_index* h) {
  if (h->storage != RAG_STORE_FP32) return 0.0;
  return (0x1p-11 * (1.0 + 0x1p-20) + 0x1p-25 * std::sqrt((double)h->dim)) * (1.0 + 0x1p-20);
}

// Bumped by every CU-mask stream creation / rag_stream_destroy: a workspace's cached CU
// count is re-read when it changed, so a stream created later at a destroyed partition
// stream's address (with another mask, or none) never inherits the old count.
std::atomic<uint64_t> g_stream_gen{1};

// CUs a stream may run on: its CU mask (rag_stream_create_cu_partition gives each of the
// batches in flight its own share of the CUs), popcounted once per workspace binding; the null
// stream and unmasked streams -> every CU. The scan grids are sized to it (launch_search_pass).
int stream_cus(const rag_index* h, hipStream_t st) {
  if (!st) return h->n_cu;
  uint32_t mask[32] = {};
  const uint32_t words = (uint32_t)std::min(32, (h->n_cu + 31) / 32);
  if (hipExtStreamGetCUMask(st, words, mask) != hipSuccess) {
    (void)hipGetLastError();
    return h->n_cu;
  }
  int n = 0;
  for (uint32_t i = 0; i < words; ++i) n += __builtin_popcount(mask[i]);
  return n > 0 && n < h->n_cu ? n : h->n_cu;
}

// D <= 384 (one query group): qprep fused into the sample launch (qprep_sample_kernel);
// RAGMI_FUSED_PREP=0 (diagnostic A/B, ragmi::Knob) keeps the separate qprep launch
bool fused_prep() {
  static ragmi::Knob k("RAGMI_FUSED_PREP");
  return k.get(1) != 0;
}

// Workgroups of the tier-2 rescan launch: ~128 tiles each, at most one per CU. A marked pass
// streams the shard at the chip's rate with that many, and the idle launch (every pass) costs
// one dispatch per workgroup, each needing a CU with the rescan's 79 KB of LDS free beside the
// other streams' scans. Round 4 sweep (profiles/r04m_rescan_grid.jsonl), 1.25M rows, 4 in
// flight, qps / 4 marked queries' added ms at 1.25M / 10M rows: 512 workgroups (two per CU)
// 209.3K / 0.45 / 1.36, 256: 210.4K / 0.53 / 1.21, 128: 210.7K / 0.80 / 2.18.
// Round 6 A/B (profiles/r06_legs/r06af_*, r06ag_*): capped at the 64 CUs the 10M-row scan
// leaves free, the idle launch no longer waits beside the other batch's scan — 10M rows 29.03
// / 29.03K qps vs 28.93 / 28.21K — but the 1.25M-row line (partitioned streams) lost 0.7%
// (222.5 / 224.4K vs 223.1 / 226.9K) and a marked pass took 1.45 / 4.37 ms instead of 0.51 /
// 1.23 ms at 1.25M / 10M rows: the default stays.
// RAGMI_RESCAN_WG (diagnostic A/B) caps it; 0 = skip (queries left tier 3, unanswered).
int rescan_grid(const rag_index* h) {
  static ragmi::Knob k("RAGMI_RESCAN_WG");
  const int cap = k.get(kRescanMaxWG);
  if (cap <= 0) return 0;
  const int64_t n_tiles = (h->count + 15) / 16;
  return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)cap, (int64_t)kRescanMaxWG,
                                                      (int64_t)h->n_cu, n_tiles / 128}));
}

// Slices per query of the 6-bit route's tier 1 (band_kernel, grid (kBandSlices, Bq)): 4 make 128
// workgroups of a 32-query pass with ~50 of a query's ~200 qualifying lists each, two gather
// chunks. Measured at 10M rows with builds that took the count from the environment, same visit,
// queries/s: 4 slices 63.8-64.2K, 8 (one workgroup per CU, one chunk each) 62.9-63.3K, and in
// another visit 4 / 8 / 16: 65.2K / 64.6K / 63.5K, against 63.0K with tier 1 inside select
// (DESIGN.md R17). A compile-time choice (no RAGMI_* knob): 1 .. kBandSlicesMax; 0 builds tier 1
// inside select's one workgroup per query with the wider gather chunk (kBandLists6), as before
// band_kernel
constexpr int kBandSlices = 4;
static_assert(kBandSlices >= 0 && kBandSlices <= kBandSlicesMax, "bd_pub holds kBandSlicesMax lists");

// RAGMI_SAMPLE_DIV (diagnostic A/B): 1 / the sampled fraction of the shard's tiles
int sample_div() {
  static ragmi::Knob k("RAGMI_SAMPLE_DIV");
  return std::max(1, k.get(128));
}

// tiles of a seed sample: ~0.8% of the shard's, at least 256 (small shards: all), at most `cap`
int seed_sample(int n_tiles, int cap) {
  return std::min({n_tiles, std::max(256, n_tiles / sample_div()), cap});
}

// sample + thresh: seed thresholds for the scan (see sample_kernel), the queries prepared
template <int D, bool FILTER>
void launch_seed(rag_index* h, Workspace& w, int groups, const uint32_t* tags, hipStream_t st) {
  const int n_tiles = (int)((h->count + 15) / 16);
  if (n_tiles == 0) return;   // the scan visits no tile; seeds are never read
  // D = 1024 tiles are 32 KB and config 5 shards hold up to 3.1M of them: a 4096-tile cap
  // would sample 0.13% of a 50M-row shard and let ~25K rows per query past the seed
  constexpr int kCap = D > 384 ? kMaxSampleWide : kMaxSample;
  const int n_sample = seed_sample(n_tiles, kCap);
  if constexpr (D > 384)   // every query group in one pass over each sample tile
    sample_wide_kernel<D, FILTER><<<dim3((n_sample + 7) / 8), dim3(256), 0, st>>>(
        h->corpus, tags, w.filt, w.qfrag, (int)h->count, n_tiles, n_sample, w.smax, groups);
  else
    sample_kernel<D, FILTER><<<dim3((n_sample + 7) / 8, groups), dim3(256), 0, st>>>(
        h->corpus, tags, w.filt, w.qfrag, (int)h->count, n_tiles, n_sample, w.smax);
  thresh_kernel<kCap><<<dim3(kQ, groups), dim3(256), 0, st>>>(w.smax, n_sample, w.eps, w.seed);
}

// the same with qprep fused into the sample launch (D <= 384; runs with nothing to sample too)
template <int D, bool FILTER>
void launch_prep_seed(rag_index* h, Workspace& w, const float* q, int Bq, const uint32_t* filt_in,
                      const uint32_t* tags, hipStream_t st) {
  if constexpr (D <= 384) {
    const int n_tiles = (int)((h->count + 15) / 16);
    const int n_sample = seed_sample(n_tiles, kMaxSample);
    qprep_sample_kernel<D, FILTER><<<dim3(std::max(1, (n_sample + 7) / 8)), dim3(256), 0, st>>>(
        q, Bq, filt_in, w.qn, w.qfrag, w.filt, w.eps, store_eps(h), h->corpus, tags,
        (int)h->count, n_tiles, n_sample, w.smax);
    if (n_sample > 0)
      thresh_kernel<kMaxSample><<<dim3(kQ, 1), dim3(256), 0, st>>>(w.smax, n_sample, w.eps,
                                                                  w.seed);
  }
}

// Does a k <= RAG_MAX_K pass of `h` scan the int8 copy (rag_index_set_prescan)? Only an index
// that keeps the copy (dim 384, fp16 storage). Auto: passes over at least RAG_PRESCAN_MIN_ROWS
// rows, filtered or not (10M rows: unfiltered 1.82x, per-query ticker filter 1.82x; 500K rows
// 1.03x; DESIGN.md "int8 prescan"); below that a step is launch-bound and the wider
// certificate band (tier 1 for a sixth to a third of the queries) buys nothing.
bool use_prescan(const rag_index* h, int k) {
  return h->copy[kCopy8].data && RAG_PRESCAN_ROUTES(h->prescan, h->dim, h->storage, k, h->count);
}

// ... and does it scan the 6-bit copy instead? Only where the index keeps one (capacity from
// RAG_PRESCAN6_MIN_ROWS, or mode RAG_PRESCAN_ALWAYS6 set). Auto: from RAG_PRESCAN6_MIN_ROWS
// rows
bool use_prescan6(const rag_index* h, int k) {
  return h->copy[kCopy6].data && RAG_PRESCAN6_ROUTES(h->prescan, h->dim, h->storage, k, h->count);
}

// The copy a k <= RAG_MAX_K pass of `h` streams: none (the fp16 rows), the int8 or the 6-bit one
CopyKind pass_copy(const rag_index* h, int k) {
  if (!use_prescan(h, k)) return kNoCopy;
  return use_prescan6(h, k) ? kCopy6 : kCopy8;
}

// Query prep and seeds of a prescan pass over copy `kind`: qprep's outputs plus the int8 planes
// (qprep8_kernel), then launch_seed's sample of the shard scored with that copy's own upper
// bound u (sample_kernel_q) and thresh_kernel on it
template <int D>
void launch_prep8(rag_index* h, Workspace& w, const float* q, int Bq, const uint32_t* filt,
                  const uint32_t* tags, hipStream_t st, CopyKind kind) {
  qprep8_kernel<D><<<dim3(kQ), dim3(64), 0, st>>>(q, Bq, filt, w.qn, w.qfrag, w.filt, w.eps,
                                                  w.qfrag8, w.qp8, w.eps8);
  const int nt = (int)((h->count + 15) / 16);
  if (nt == 0) return;   // the scan visits no tile; seeds are never read
  const int n_sample = seed_sample(nt, kMaxSample);
  with_filter(filt, [&](auto f) {
    with_copy(kind, [&](auto c) {
      sample_kernel_q<D, decltype(f)::value, typename decltype(c)::type>
          <<<dim3((n_sample + 7) / 8), dim3(256), 0, st>>>(
              h->copy[kind].data, h->copy[kind].meta, tags, w.filt,
              reinterpret_cast<const intx4*>(w.qfrag8), w.qp8, (int)h->count, nt, n_sample,
              w.smax);
    });
  });
  thresh_kernel<kMaxSample><<<dim3(kQ, 1), dim3(256), 0, st>>>(w.smax, n_sample, w.eps8, w.seed);
}

// a CU-partitioned stream (cus < n_cu; 0: none): the same per-CU occupancy over its CUs only
bool partitioned(const rag_index* h, int cus) { return cus > 0 && cus < h->n_cu; }
int max_wgs_on(const rag_index* h, int cus) { return partitioned(h, cus) ? 2 * cus : h->max_wgs; }

// Workgroups of the D <= 384 scan (queries in VGPRs) on a stream of `cus` CUs.
// One scan workgroup on 3/4 of the CUs (h->scan_wgs), not two on every CU: measured on
// one MI355X (profiles/r03j_scan_wgs_*.jsonl, interleaved processes, 2 reps each) 10M rows
// 27.19K qps / 83.0% of the HBM roofline at 512 workgroups -> 28.67-28.82K / 86.2-86.7% at
// 192 (224: 86.0-86.6%, 256: 85.6-86.1%, 288: 66.2% — one CU in eight with a second
// workgroup makes the launch wait on them —, 160: 82.9%, 128: 72.5%); 2.5M rows 99.3K ->
// 103.1K; 1.25M rows with 4 in flight 189K -> 199K (union 0.71 -> 0.76). Fewer, longer
// wave streams keep HBM as busy as twice as many, each wave's fixed start / end-of-scan
// list work is paid by 768 waves instead of 2048 (select merges that many fewer lists), and
// the free CUs take the other streams' query prep, sampling and select beside the scan
// instead of behind it. RAGMI_SCAN_WGS overrides the cap (diagnostic A/B).
int scan_grid(const rag_index* h, int cus, bool filtered, CopyKind copy) {
  static ragmi::Knob k_wgs("RAGMI_SCAN_WGS");
  const int wg_env = k_wgs.get(0) > 0 ? std::max(8, k_wgs.get(0)) : 0;
  const bool part = partitioned(h, cus);
  const int max_wgs = max_wgs_on(h, cus);
  // Filtered scans (a tag load and compare per row) keep two workgroups per CU: 10M rows,
  // per-query ticker filter, serial order: 26.8 / 27.0K qps at 512 vs 25.7 / 26.1K at 192
  // (scan 1.170 vs 1.21-1.24 ms, profiles/r03u_filtered_wgs.jsonl)
  // On a CU-partitioned stream (the batches in flight on disjoint CU sets) one workgroup per
  // CU of its share: 1.25M rows, 4 batches in flight on quarter-CU streams, 64 workgroups
  // 222-223K qps vs 205K at 48, 210-218K at 128, and 206-208K for 4 unpartitioned streams at
  // the default grid (scripts/diag/cu_partition.py, profiles/r05c_cu_partition.jsonl; bench lines
  // 222.7-223.3K vs 207.0-207.6K, profiles/r05d_partition_lines.jsonl)
  // the int8 prescan holds both query planes in VGPRs (one workgroup per CU at most), so its
  // filtered passes take the unfiltered grid
  // the 6-bit prescan is bound by instruction issue where the int8 one is bound by HBM (its
  // top-k and bound arithmetic no longer hide under the loads): one workgroup on EVERY CU,
  // 10M rows 59.2K qps at 192 workgroups, 62.4K at 224, 63.6K at 256
  const int wg_cap = wg_env ? wg_env
                     : (filtered && copy == kNoCopy) ? max_wgs
                     : part ? cus
                     : copy == kCopy6 ? h->n_cu
                                      : h->scan_wgs;
  const int64_t n_tiles = (h->count + 15) / 16;
  const int grid = (int)std::min<int64_t>(std::min(max_wgs, wg_cap),
                                          std::max<int64_t>(1, (n_tiles + 3) / 4));
  return std::min(grid, kMaxLists / kWavesPerWG);
}

// go(args...) of launch_search_pass for the D <= 384 scan kernel named: a timed launch carries
// its own timestamps (launch_fixed_timed). A macro: RAG_HIP's message names the kernel
#define RAG_SCAN_GO(...)                                                                      \
  [&](auto... args) -> int {                                                                  \
    if (timed)                                                                                \
      RAG_HIP(launch_fixed_timed<kScanBlock>(__VA_ARGS__, dim3(grid), 0, st, pp.a, pp.b, args...)); \
    else                                                                                      \
      launch_fixed<kScanBlock>(__VA_ARGS__, dim3(grid), 0, st, args...);                      \
    return RAG_OK;                                                                            \
  }

template <int D>
int launch_search_pass(rag_index* h, Workspace& w, const PassArgs& a, hipStream_t st) {
  const uint32_t* const filt = a.filt;
  const int Bq = a.Bq;
  // Bq <= 32 * h->groups queries: `groups` query groups of 32 (one for D <= 384)
  const int groups = (Bq + kQ - 1) / kQ;
  CopyKind copy = kNoCopy;   // the scan copy this pass streams
  if constexpr (D == 384) copy = pass_copy(h, a.k);
  // fused qprep + sample only in free scan order (small shards, several scans overlapping):
  // there it is +1.1% (1.25M rows, 4 in flight, profiles/r03d_fused_prep_ab.jsonl); with the
  // scans chained (>= 4M rows) its 256-thread workgroups of ~180 registers, which cannot share a
  // CU with scan workgroups, landed between a scan's workgroups and stretched the scan launch
  // (10M rows: scan 0.76 vs 0.83 of the roofline, same qps, profiles/r03i_headline_prep_ab.jsonl)
  if (copy != kNoCopy) {
    ++h->copy_passes[copy];   // rag_index_prescan_passes (the caller holds h->mu)
    // the seed is then a lower bound of the 32nd-best u, which the prescan's thresholds compare
    if constexpr (D == 384) launch_prep8<D>(h, w, a.q, Bq, filt, a.tags, st, copy);
  } else if (D <= 384 && groups == 1 && fused_prep() && h->serial_scans == 0) {
    with_filter(filt, [&](auto f) {
      launch_prep_seed<D, decltype(f)::value>(h, w, a.q, Bq, filt, a.tags, st);
    });
  } else {
    qprep_kernel<D><<<dim3(groups * kQ), dim3(64), 0, st>>>(a.q, Bq, filt, w.qn, w.qfrag, w.filt,
                                                            w.eps, store_eps(h));
    with_filter(filt, [&](auto f) {
      launch_seed<D, decltype(f)::value>(h, w, groups, a.tags, st);
    });
  }
  const int64_t n_tiles = (h->count + 15) / 16;
  // D <= 384: queries in VGPRs, 2 workgroups per CU; wider rows: queries in LDS, 1 per CU,
  // R workgroups per query group (R % 8 == 0: XCD pairing of the groups, scan_lds_kernel)
  constexpr bool kLdsQ = D > 384;
  int grid;
  const bool part = partitioned(h, w.cus);
  const int max_wgs = max_wgs_on(h, w.cus);
  if constexpr (kLdsQ) {
    const int per_group = std::max(8, (max_wgs / 2 / groups) & ~7);
    const int need = (int)std::min<int64_t>(
        per_group, ((n_tiles + kLdsWaves - 1) / kLdsWaves + 7) & ~int64_t(7));
    grid = std::max(8, std::min(need, kMaxLists / kLdsWaves));
  } else {
    grid = scan_grid(h, w.cus, filt != nullptr, copy);
  }
  const hipStream_t caller = st;
  if (h->serial_scans == 1) {
    if (!h->scan_done) RAG_HIP(hipEventCreateWithFlags(&h->scan_done, hipEventDisableTiming));
    // (keyed on scan_any, not on scan_last being non-null: a scan on the null stream leaves
    // scan_last == nullptr, and testing the handle let the next pass on another stream skip
    // its wait — the filtered 10M line's scans overlapped, traced: 2.2 ms launches, 1.24 ms
    // apart)
    if (h->scan_any && h->scan_last != st) RAG_HIP(hipStreamWaitEvent(st, h->scan_done, 0));
  } else if (h->serial_scans == 2) {
    if (!h->scan_stream) RAG_HIP(hipStreamCreateWithFlags(&h->scan_stream, hipStreamNonBlocking));
    if (!w.ev_in) RAG_HIP(hipEventCreateWithFlags(&w.ev_in, hipEventDisableTiming));
    if (!w.ev_out) RAG_HIP(hipEventCreateWithFlags(&w.ev_out, hipEventDisableTiming));
    RAG_HIP(hipEventRecord(w.ev_in, st));
    RAG_HIP(hipStreamWaitEvent(h->scan_stream, w.ev_in, 0));
    st = h->scan_stream;
  }
  ProfPair pp{};
  const bool timed = h->prof > 0 && (h->prof_seq++ % h->prof) == 0;
  if (timed) {
    RAG_HIP(hipEventCreate(&pp.a));
    RAG_HIP(hipEventCreate(&pp.b));
    // the LDS-query / wide scans (a memset + launch, or one launch): marker events around them;
    // the 384-d scan times its own dispatch (RAG_SCAN_GO below)
    if constexpr (kLdsQ) RAG_HIP(hipEventRecord(pp.a, st));
  }
  // go(the arguments scan_kernel and scan_lds_kernel share, then `tail`)
  const auto with_scan_args = [&](auto&& go, auto... tail) {
    return go(h->corpus, a.tags, w.filt, w.qfrag, (int)h->count, (int)n_tiles, w.seed, w.part_s,
              w.part_i, w.heads_s, w.heads_i, w.heads_n, tail...);
  };
  const bool wide = kLdsQ && groups > 1 && !filt;
  if (wide) {
    // RAGMI_WIDE_WGS (diagnostic A/B): workgroup cap of the wide scan (default one per CU)
    static ragmi::Knob k_wide("RAGMI_WIDE_WGS");
    const int wide_env = k_wide.get(0) > 0 ? std::max(8, k_wide.get(0)) : 0;
    const int cap = wide_env ? std::min(wide_env, max_wgs / 2) : max_wgs / 2;
    grid = (int)std::min<int64_t>(cap, std::max<int64_t>(1, n_tiles));
  }
  if constexpr (kLdsQ) {
    const dim3 g3(grid * groups);
    if (wide) {
      // all groups in every workgroup, one pass over the corpus (scan_wide_kernel)
      // ring loads non-temporal (the corpus is read once per pass): 50M x 1024, B = 128
      // 70.3% -> 71.2% of the HBM roofline, loads-only 80.1% -> 85.8%
      // (profiles/r01h_wide_nt.jsonl). The diagnostic variants run only via rag_bench_scan.
      launch_fixed<kWideBlock>(scan_wide_kernel<D, 0, true>, dim3(grid), 0, st, h->corpus,
                               w.qfrag, (int)h->count, (int)n_tiles, w.seed, w.part_s,
                               w.part_i, w.heads_s, w.heads_i, w.heads_n, groups);
    } else {
      // one group: non-temporal ring loads; several: the groups share tiles through the
      // throttle words, zeroed first
      if (groups > 1)
        RAG_HIP(hipMemsetAsync(w.progress, 0, (size_t)grid * kLdsWaves * groups * 4, st));
      const auto launch = [&](auto nt) {
        with_filter(filt, [&](auto f) {
          with_scan_args(
              [&](auto... args) {
                launch_fixed<kLdsBlock>(
                    scan_lds_kernel<D, decltype(f)::value, decltype(nt)::value>, g3, 0, st,
                    args...);
              },
              groups, w.progress);
        });
      };
      if (groups == 1)
        launch(std::true_type{});
      else
        launch(std::false_type{});
    }
  } else {
    const int rc = with_filter(filt, [&](auto f) -> int {
      constexpr bool F = decltype(f)::value;
      if constexpr (D == 384) {
        // go(the arguments the two prescan kernels share)
        const auto with_copy_args = [&](auto&& go) {
          return go(h->copy[copy].data, h->copy[copy].meta, a.tags, w.filt,
                    reinterpret_cast<const intx4*>(w.qfrag8), w.qp8, (int)h->count, (int)n_tiles,
                    w.seed, w.part_s, w.part_i, w.heads_s, w.heads_i, w.heads_n);
        };
        if (copy == kCopy6) return with_copy_args(RAG_SCAN_GO(scan_kernel_i6<D, F>));
        if (copy == kCopy8) return with_copy_args(RAG_SCAN_GO(scan_kernel_i8<D, F>));
      }
      return with_scan_args(RAG_SCAN_GO(scan_kernel<D, F>), nullptr);
    });
    if (rc) return rc;
  }
  if (timed) {
    if constexpr (kLdsQ) RAG_HIP(hipEventRecord(pp.b, st));
    h->prof_pairs.push_back(pp);
  }
  if (h->serial_scans == 1) {
    RAG_HIP(hipEventRecord(h->scan_done, st));
    h->scan_last = st;
    h->scan_any = true;
  } else if (h->serial_scans == 2) {
    RAG_HIP(hipEventRecord(w.ev_out, st));
    RAG_HIP(hipStreamWaitEvent(caller, w.ev_out, 0));
    st = caller;
  }
  const int n_lists = wide ? grid : grid * (kLdsQ ? kLdsWaves : kWavesPerWG);   // per group
  const ExactStats fb{w.fb_tier, w.fb_cnt, w.t2};
  // select certifies every query's top-k; its fallbacks (list re-scoring, a workgroup-local
  // second pass over the shard) run inside the same launch
  // (after the 6-bit prescan every query takes tier 1, its band spanning ~200 lists: the head
  // instantiation stops at the verdict and band_kernel spreads tier 1 over the chip)
  const BandWs bw{w.bd_rec, w.bd_pub, w.bd_tk};
  with_filter(filt, [&](auto f) {
    with_flag(copy == kCopy6, [&](auto six) {
      constexpr int BL = !(D == 384 && decltype(six)::value) ? kBandLists
                         : kBandSlices > 0                   ? kBandHead
                                                             : kBandLists6;
      select_kernel<D, decltype(f)::value, BL><<<dim3(Bq), dim3(256), 0, st>>>(
          w.part_s, w.part_i, w.heads_s, w.heads_i, w.heads_n, n_lists, h->corpus, a.tags, w.filt,
          w.qfrag, (int)h->count, w.qn, a.k, copy != kNoCopy ? w.eps8 : w.eps, w.seed, fb,
          a.id_offset, a.out_s, a.out_i, a.out_packed, h->rows32,
          copy != kNoCopy ? w.eps : nullptr, bw);
    });
  });
  if constexpr (D == 384 && kBandSlices > 0) {
    if (copy == kCopy6)
      band_kernel<D><<<dim3(kBandSlices, Bq), dim3(256), 0, st>>>(
          w.part_s, w.part_i, w.heads_n, n_lists, h->corpus, w.qn, a.k, bw, fb, w.eps,
          a.id_offset, a.out_s, a.out_i, a.out_packed, h->rows32);
  }
  // tier 2 of the certificate (rescan_kernel): returns at once unless select marked a query
  // of the pass; otherwise its R workgroups stream the shard once per 16 marked queries.
  // RAGMI_RESCAN_WG (diagnostic A/B) caps R; 0 skips the launch, and mark_unanswered_kernel
  // then records the marked queries as unanswered (tier 3, rag_index_unanswered): timing only
  const int R = std::min(rescan_grid(h), part ? w.cus : h->n_cu);
  if (R > 0) {
    with_filter(filt, [&](auto f) {
      launch_fixed<kScanBlock>(rescan_kernel<D, decltype(f)::value>, dim3(R), 0, st, w.fb_tier,
                               w.t2, Bq, h->corpus, a.tags, w.filt, w.qfrag, (int)h->count, w.qn,
                               a.k, w.eps, w.t2_s, w.t2_i, w.t2_tk, a.id_offset, a.out_s, a.out_i,
                               a.out_packed, h->rows32);
    });
  } else {
    mark_unanswered_kernel<<<dim3(1), dim3(64), 0, st>>>(w.fb_tier, Bq, w.fb_cnt);
  }
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}
#undef RAG_SCAN_GO

int ensure_lk(Workspace& w) {
  if (w.lk_cand) return RAG_OK;
  // all seven or none (a partial set would be re-allocated, and leaked, by the next large-k call)
  if (ragmi::ws_alloc_all(lk_buffers(w)) != hipSuccess) {
    (void)hipGetLastError();
    return ragmi::fail(RAG_ENOMEM, "large-k workspace allocation failed");
  }
  return RAG_OK;
}

// One search pass of <= 32 queries by the full exact path (largek_kernels.hip "Exact top-k
// for ANY k"): k > RAG_MAX_K_LARGE, or rag_index_search_full. Per query: exact scores of every
// row, a stable descending radix sort of (key, row), the first k emitted. The sort buffers
// (16 B per row + hipcub's scratch) are stream-ordered allocations released at the pass's end.
template <int D>
int launch_full_pass(rag_index* h, Workspace& w, const PassArgs& a, hipStream_t st) {
  const int Bq = a.Bq, k = a.k;
  qprep_kernel<D><<<dim3(kQ), dim3(64), 0, st>>>(a.q, Bq, a.filt, w.qn, w.qfrag, w.filt, w.eps,
                                                  store_eps(h));
  RAG_HIP(hipGetLastError());
  const int n = (int)h->count;
  // query j's top k out of the sorted (keys, rows), of which n_match[0] matched its filter
  auto emit = [&](int j, const uint32_t* keys, const int* rows, const int* n_match) {
    full_emit_kernel<<<dim3((unsigned)std::min<int64_t>(1024, (k + 255) / 256)), dim3(256), 0,
                       st>>>(keys, rows, n_match, k, a.id_offset,
                             a.out_s ? a.out_s + (int64_t)j * k : nullptr,
                             a.out_i ? a.out_i + (int64_t)j * k : nullptr,
                             a.out_packed ? a.out_packed + (int64_t)j * k * 2 : nullptr);
  };
  StreamScratch scratch(st);
  if (n == 0) {
    RAG_HIP(scratch.alloc(4));
    int* zero = reinterpret_cast<int*>(scratch.p);
    RAG_HIP(hipMemsetAsync(zero, 0, 4, st));
    for (int j = 0; j < Bq; ++j) emit(j, nullptr, nullptr, zero);
    RAG_HIP(hipGetLastError());
    return RAG_OK;
  }
  size_t tmp_bytes = 0;
  RAG_HIP(hipcub::DeviceRadixSort::SortPairsDescending(
      nullptr, tmp_bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
      static_cast<const int*>(nullptr), static_cast<int*>(nullptr), n, 0, 32, st));
  const size_t nb = (size_t)n * 4;
  const size_t m_off = 4 * nb, t_off = m_off + 256;
  RAG_HIP(scratch.alloc(t_off + tmp_bytes));
  char* const buf = scratch.p;
  uint32_t* k_in = reinterpret_cast<uint32_t*>(buf);
  uint32_t* k_out = reinterpret_cast<uint32_t*>(buf + nb);
  int* v_in = reinterpret_cast<int*>(buf + 2 * nb);
  int* v_out = reinterpret_cast<int*>(buf + 3 * nb);
  int* n_match = reinterpret_cast<int*>(buf + m_off);
  void* tmp = buf + t_off;
  RAG_HIP(hipMemsetAsync(n_match, 0, 4 * kQ, st));
  // one wave per 8 rows per step; up to 8 workgroups per CU
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(8 * h->n_cu, (n + 31) / 32));
  int rc = RAG_OK;
  for (int j = 0; j < Bq && rc == RAG_OK; ++j) {
    with_filter(a.filt, [&](auto f) {
      constexpr bool F = decltype(f)::value;
      full_score_kernel<D, F><<<dim3(grid), dim3(256), 0, st>>>(
          h->corpus, a.tags, F ? w.filt + 2 * j : nullptr, w.qn + (int64_t)j * D, n, h->rows32,
          k_in, v_in, n_match + j);
    });
    if (hipGetLastError() != hipSuccess ||
        sort_pairs_desc(tmp, tmp_bytes, k_in, k_out, v_in, v_out, n, st) != hipSuccess) {
      rc = ragmi::fail(RAG_EHIP, "full exact pass: score / sort launch failed");
      break;
    }
    emit(j, k_out, v_out, n_match + j);
    if (hipGetLastError() != hipSuccess) rc = ragmi::fail(RAG_EHIP, "full exact pass: emit");
  }
  // the pass certifies every query (tier 0) by construction
  (void)hipMemsetAsync(w.fb_tier, 0, 4 * kQ, st);
  return rc;
}

// One search pass of <= 32 queries for RAG_MAX_K < k <= RAG_MAX_K_LARGE (largek_kernels.hip,
// "Exact top-k for RAG_MAX_K < k"): qprep, a sample of the shard's tiles for the bound, then
// kLkRounds (collect, final) launch pairs; rounds after the first return at once unless a
// query's candidate list overflowed in the previous one.
template <int D>
int launch_large_k_pass(rag_index* h, Workspace& w, const PassArgs& a, hipStream_t st) {
  const uint32_t* const filt = a.filt;
  const int Bq = a.Bq, k = a.k;
  int rc = ensure_lk(w);
  if (rc) return rc;
  qprep_kernel<D><<<dim3(kQ), dim3(64), 0, st>>>(a.q, Bq, filt, w.qn, w.qfrag, w.filt, w.eps,
                                                  store_eps(h));
  const int n_tiles = (int)((h->count + 15) / 16);
  // bound sample: >= 4k tiles (so k distinct-row maxima exist with margin), >= 1/32 of the
  // shard, at most kLkSampleMax
  const int n_sample = n_tiles == 0 ? 0 : std::min({n_tiles, std::max(4 * k, n_tiles / 32),
                                                    kLkSampleMax});
  if (n_sample > 0)
    with_filter(filt, [&](auto f) {
      sample_kernel<D, decltype(f)::value><<<dim3((n_sample + 7) / 8, 1), dim3(256), 0, st>>>(
          h->corpus, a.tags, w.filt, w.qfrag, (int)h->count, n_tiles, n_sample, w.lk_smax);
    });
  lk_bound_kernel<<<dim3(Bq), dim3(256), 0, st>>>(w.lk_smax, n_sample, k, w.eps, w.lk_thr,
                                                  w.lk_cnt, w.lk_again, w.lk_need);
  // collection grid: two workgroups per CU (10M rows, k = 33: 1.54-1.55 ms per pass vs
  // 1.57-1.64 at four, 2.37 at one; k = 100 1.64 either way; profiles/r05q_large_k_grid.jsonl)
  const int cgrid = (int)std::max<int64_t>(1, std::min<int64_t>(2 * h->n_cu, (n_tiles + 3) / 4));
  for (int r = 0; r < kLkRounds; ++r) {
    with_filter(filt, [&](auto f) {
      lk_collect_kernel<D, decltype(f)::value><<<dim3(cgrid), dim3(256), 0, st>>>(
          h->corpus, a.tags, w.filt, w.qfrag, (int)h->count, n_tiles, Bq, w.lk_thr, w.lk_cnt,
          w.lk_cand, w.lk_again, w.lk_need, r);
    });
    lk_rescore_kernel<D><<<dim3(kLkCap / 256, Bq), dim3(256), 0, st>>>(
        h->corpus, w.qn, w.lk_cnt, w.lk_cand, w.lk_again, w.lk_need, r, w.lk_es, h->rows32);
    lk_final_kernel<D><<<dim3(Bq), dim3(256), 0, st>>>(
        h->corpus, w.qn, k, w.lk_cnt, w.lk_cand, w.lk_es, w.eps, w.lk_thr, w.lk_again, w.lk_need, r,
        w.fb_tier, w.fb_cnt, a.id_offset, a.out_s, a.out_i, a.out_packed, h->rows32);
  }
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// k > RAG_MAX_K_LARGE: per query, three stable radix sorts over the n_lists * k entries
// (merge_any_*; the full pass's sort_pairs_desc); stream-ordered scratch released at the end
template <bool PACKED>
int merge_any_k(const float* in_s, const int64_t* in_i, int n_lists, int B, int k, float* out_s,
                int64_t* out_i, hipStream_t st) {
  const int64_t n64 = (int64_t)n_lists * k;
  if (n64 > 0x7fffffff) return ragmi::fail(RAG_ERANGE, "merge: n_lists * k too large");
  const int n = (int)n64;
  size_t tmp = 0;
  RAG_HIP(hipcub::DeviceRadixSort::SortPairsDescending(
      nullptr, tmp, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
      static_cast<const int*>(nullptr), static_cast<int*>(nullptr), n, 0, 32, st));
  // keys in/out + positions in/out: 16 B per entry, + scratch (256-B aligned)
  const size_t nb = (size_t)n;
  StreamScratch buf(st);
  const size_t t_off = (nb * 16 + 255) & ~(size_t)255;
  RAG_HIP(buf.alloc(t_off + tmp));
  uint32_t* ka = reinterpret_cast<uint32_t*>(buf.p);
  uint32_t* kb = ka + nb;
  int* pa = reinterpret_cast<int*>(kb + nb);
  int* pb = pa + nb;
  void* scratch = buf.p + t_off;
  const dim3 g((unsigned)std::min<int64_t>(1024, (n64 + 255) / 256));
  const dim3 ge((unsigned)std::min<int64_t>(1024, ((int64_t)k + 255) / 256));
  auto sort = [&]() {   // (ka, pa) -> (kb, pb), stable, keys descending
    return sort_pairs_desc(scratch, tmp, ka, kb, pa, pb, n, st) == hipSuccess;
  };
  int rc = RAG_OK;
  for (int b = 0; b < B && rc == RAG_OK; ++b) {
    bool ok = true;
    for (int word = 0; word < 2 && ok; ++word) {   // id ascending: low word, then high word
      merge_any_ids_kernel<PACKED><<<g, dim3(256), 0, st>>>(
          in_s, in_i, n_lists, B, k, b, word ? pb : nullptr, word, ka, pa);
      ok = hipGetLastError() == hipSuccess && sort();
    }
    if (ok) {
      merge_any_scores_kernel<PACKED><<<g, dim3(256), 0, st>>>(in_s, in_i, n_lists, B, k, b, pb,
                                                               ka, pa);
      ok = hipGetLastError() == hipSuccess && sort();
    }
    if (ok) {
      merge_any_emit_kernel<PACKED><<<ge, dim3(256), 0, st>>>(in_s, in_i, B, k, b, kb, pb, out_s,
                                                              out_i);
      ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) rc = ragmi::fail(RAG_EHIP, "merge: sort / launch failed");
  }
  return rc;
}

// rag_merge_topk (in_s, in_i) / rag_merge_topk_packed (PACKED: in_s holds the int32 pairs, in_i
// is unused) behind their argument checks: the merge kernel by the size of k
template <bool PACKED>
int merge_topk(const float* in_s, const int64_t* in_i, int n_lists, int B, int k, float* out_s,
               int64_t* out_i, hipStream_t st) {
  if (B == 0) return RAG_OK;
  if (k > RAG_MAX_K_LARGE) return merge_any_k<PACKED>(in_s, in_i, n_lists, B, k, out_s, out_i, st);
  if (k > RAG_MAX_K)
    merge_large_kernel<PACKED><<<dim3(B), dim3(256), 0, st>>>(in_s, in_i, n_lists, B, k, out_s,
                                                             out_i);
  else
    merge_exact_kernel<PACKED><<<dim3(B), dim3(64), 0, st>>>(in_s, in_i, n_lists, B, k, out_s,
                                                            out_i);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// the argument rules of every search entry point, checked before any HIP call
int search_args(const float* q, int B, int k, const float* out_s, const int64_t* out_i,
                const int32_t* out_packed) {
  if (B < 0 || (B > 0 && (!q || (!out_packed && (!out_s || !out_i)))))
    return ragmi::fail(RAG_EINVAL, "bad search args");
  if (k < 1) return ragmi::fail(RAG_ERANGE, "k must be >= 1");
  if (out_packed && k > RAG_MAX_K_LARGE)
    return ragmi::fail(RAG_ERANGE, "packed (exchange) search: k must be <= RAG_MAX_K_LARGE=4096");
  return RAG_OK;
}

// a packed search's ids (id_offset + row) fit its int32 pairs
int packed_ids_args(const rag_index* h, int64_t id_offset) {
  if (id_offset < 0 || id_offset + h->count > INT32_MAX)
    return ragmi::fail(RAG_ERANGE, "packed ids are int32: global rows must stay below 2^31");
  return RAG_OK;
}

// The workspace of a pass of Bq queries on stream `st` (lock held): the slot bound to `st`, a
// free one, or — every slot being bound to another stream whose last pass may still be running —
// the least recently used one after a device drain; bound to `st`, its CU count current
int take_workspace(rag_index* h, hipStream_t st, int Bq, Workspace** out) {
  Workspace* lru = nullptr;
  Workspace* wp = pick_slot(h->ws, st, lru);
  if (!wp) {
    RAG_HIP(hipDeviceSynchronize());
    wp = lru;
  }
  Workspace& w = *wp;
  const uint64_t gen = g_stream_gen.load(std::memory_order_acquire);
  if (!w.used || w.owner != st || w.cus == 0 || w.cus_gen != gen) {
    w.cus = stream_cus(h, st);
    w.cus_gen = gen;
  }
  w.used = true;
  w.owner = st;
  w.tick = ++h->ws_tick;
  h->last_ws = &w;
  h->last_bq = Bq;
  *out = wp;
  return RAG_OK;
}

// full: the full exact path for every query (rag_index_search_full); it is also taken for
// k > RAG_MAX_K_LARGE (unpacked output only: the exchange merge holds at most that many)
// tags: the column the passes filter on: the stored tags, or rag_index_search_view's view
int search_locked(rag_index* h, const float* q, int B, int k, const uint32_t* filt,
                  int64_t id_offset, float* out_s, int64_t* out_i, int32_t* out_packed,
                  hipStream_t st, bool full = false, const uint32_t* tags = nullptr) {
  if (const int rc = search_args(q, B, k, out_s, out_i, out_packed)) return rc;
  if (!tags) tags = h->tags;
  full = full || k > RAG_MAX_K_LARGE;
  RAG_HIP(hipSetDevice(h->device));
  const bool large = k > RAG_MAX_K || full;
  const int per_pass = large ? kQ : kQ * h->groups;
  for (int b0 = 0; b0 < B; b0 += per_pass) {
    const int Bq = std::min(per_pass, B - b0);
    Workspace* wp = nullptr;
    if (const int rc = take_workspace(h, st, Bq, &wp)) return rc;
    Workspace& w = *wp;
    const PassArgs a{q + (int64_t)b0 * h->dim,
                     Bq,
                     k,
                     filt ? filt + 2 * b0 : nullptr,
                     tags,
                     id_offset,
                     out_packed ? nullptr : out_s + (int64_t)b0 * k,
                     out_packed ? nullptr : out_i + (int64_t)b0 * k,
                     out_packed ? out_packed + (int64_t)b0 * k * 2 : nullptr};
    const auto dim = [&](auto&& pass) { return with_dim(h->dim, pass); };
    const int rc =
        full    ? dim([&](auto d) { return launch_full_pass<decltype(d)::value>(h, w, a, st); })
        : large ? dim([&](auto d) { return launch_large_k_pass<decltype(d)::value>(h, w, a, st); })
                : dim([&](auto d) { return launch_search_pass<decltype(d)::value>(h, w, a, st); });
    if (rc) return rc;
  }
  return RAG_OK;
}

// ---- recommend queries (reco_kernels.hip; the contract: ragmi.h "Recommend queries") ----

// one request's examples (device pointers, [n][dim] fp32) and its strategy
struct RecoArgs {
  const float* pos;
  int P;
  const float* neg;
  int N;
  int strat;
};

// the argument rules of the recommend entry points, checked before any HIP call
int reco_args(const RecoArgs& r, bool average_ok) {
  static_assert(kRecoSide == RAG_RECO_MAX_SIDE && kRecoAverage == RAG_RECO_AVERAGE &&
                    kRecoBest == RAG_RECO_BEST && kRecoSum == RAG_RECO_SUM && 2 * kRecoSide == kQ,
                "reco_kernels.hip's slots and strategies");
  if (r.P < 0 || r.N < 0 || r.P > RAG_RECO_MAX_SIDE || r.N > RAG_RECO_MAX_SIDE)
    return ragmi::fail(RAG_ERANGE,
                       "recommend: a side holds 0 to RAG_RECO_MAX_SIDE=16 examples");
  if (r.strat != RAG_RECO_BEST && r.strat != RAG_RECO_SUM &&
      !(average_ok && r.strat == RAG_RECO_AVERAGE))
    return ragmi::fail(RAG_EINVAL, average_ok
                                       ? "recommend: unknown strategy (RAG_RECO_AVERAGE=0, "
                                         "RAG_RECO_BEST=1, RAG_RECO_SUM=2)"
                                       : "recommend: bounds exist for RAG_RECO_BEST=1 and "
                                         "RAG_RECO_SUM=2 only");
  if (r.P + r.N == 0) return ragmi::fail(RAG_EINVAL, "recommend: needs at least one example");
  if (r.strat == RAG_RECO_AVERAGE && r.P == 0)
    return ragmi::fail(RAG_EINVAL, "recommend: RAG_RECO_AVERAGE needs a positive example");
  if ((r.P > 0 && !r.pos) || (r.N > 0 && !r.neg))
    return ragmi::fail(RAG_EINVAL, "recommend: a NULL example pointer");
  return RAG_OK;
}

int ensure_reco(Workspace& w) {
  if (w.reco_q) return RAG_OK;
  if (ragmi::ws_alloc_all(reco_buffers(w)) != hipSuccess) {
    (void)hipGetLastError();
    return ragmi::fail(RAG_ENOMEM, "recommend workspace allocation failed");
  }
  return RAG_OK;
}

// the request's query block in w: slots assembled, prepared by qprep (qn, qfrag, eps), and the
// request's parameters
template <int D>
int launch_reco_prep(rag_index* h, Workspace& w, const RecoArgs& r, hipStream_t st) {
  static_assert(D <= 1024, "reco_q holds [32][1024]");
  if (const int rc = ensure_reco(w)) return rc;
  reco_assemble_kernel<D><<<dim3(kQ), dim3(64), 0, st>>>(r.pos, r.P, r.neg, r.N, w.reco_q);
  qprep_kernel<D><<<dim3(kQ), dim3(64), 0, st>>>(w.reco_q, kQ, nullptr, w.qn, w.qfrag, w.filt,
                                                  w.eps, store_eps(h));
  reco_prep_kernel<<<dim3(1), dim3(64), 0, st>>>(w.eps, r.P, r.N, w.reco_par);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// go(strategy tag) with the strategy as a compile-time constant (BEST or SUM)
template <typename F>
auto with_reco_strategy(int strat, F&& f) {
  if (strat == kRecoBest) return f(std::integral_constant<int, kRecoBest>{});
  return f(std::integral_constant<int, kRecoSum>{});
}

// The hot pass of one BEST / SUM request, k <= RAG_MAX_K_LARGE (reco_kernels.hip): prep, the
// sample and its bound, then kLkRounds (collect, rescore, final) launch triples. a.filt: the
// request's (mask, value) pair or nullptr. Always over the fp16 rows.
template <int D>
int launch_reco_hot(rag_index* h, Workspace& w, const RecoArgs& r, const PassArgs& a,
                    hipStream_t st) {
  if (const int rc = ensure_lk(w)) return rc;
  if (const int rc = launch_reco_prep<D>(h, w, r, st)) return rc;
  const int k = a.k;
  const int n_tiles = (int)((h->count + 15) / 16);
  // the large-k pass's sample (launch_large_k_pass)
  const int n_sample = n_tiles == 0 ? 0 : std::min({n_tiles, std::max(4 * k, n_tiles / 32),
                                                    kLkSampleMax});
  const int cgrid = (int)std::max<int64_t>(1, std::min<int64_t>(2 * h->n_cu, (n_tiles + 3) / 4));
  const int per_wg = reco_rescore_per_wg(r.P + r.N);
  const int rgrid = (kLkCap + per_wg - 1) / per_wg;
  with_filter(a.filt, [&](auto f) {
    with_reco_strategy(r.strat, [&](auto s) {
      constexpr bool F = decltype(f)::value;
      constexpr int STRAT = decltype(s)::value;
      if (n_sample > 0)
        reco_sample_kernel<D, F, STRAT><<<dim3((n_sample + 3) / 4), dim3(256), 0, st>>>(
            h->corpus, a.tags, a.filt, w.qfrag, w.eps, w.reco_par, r.P, r.N, (int)h->count,
            n_tiles, n_sample, w.lk_smax);
      // T = the k-th largest sample maximum (L is a bound already: the eps it subtracts is 0)
      lk_bound_kernel<<<dim3(1), dim3(256), 0, st>>>(w.lk_smax, n_sample, k, w.reco_par,
                                                     w.lk_thr, w.lk_cnt, w.lk_again, w.lk_need);
      for (int round = 0; round < kLkRounds; ++round) {
        reco_collect_kernel<D, F, STRAT><<<dim3(cgrid), dim3(256), 0, st>>>(
            h->corpus, a.tags, a.filt, w.qfrag, w.eps, w.reco_par, r.P, r.N, (int)h->count,
            n_tiles, w.lk_thr, w.lk_cnt, w.lk_cand, w.lk_again, w.lk_need, round);
        reco_rescore_kernel<D><<<dim3(rgrid), dim3(256), 0, st>>>(
            h->corpus, w.qn, r.P, r.N, r.strat, w.lk_cnt, w.lk_cand, w.lk_again, w.lk_need, round,
            w.lk_es, h->rows32, w.reco_par);
        lk_final_kernel<D><<<dim3(1), dim3(256), 0, st>>>(
            h->corpus, w.qn, k, w.lk_cnt, w.lk_cand, w.lk_es, w.reco_par, w.lk_thr, w.lk_again,
            w.lk_need, round, w.fb_tier, w.fb_cnt, a.id_offset, a.out_s, a.out_i, nullptr,
            h->rows32);
      }
    });
  });
  RAG_HIP(hipGetLastError());
  ++h->reco_hot;
  h->reco_last = &w;
  return RAG_OK;
}

// The full pass of a request whose every row `score` scores exactly (recommend, discover), any
// k: score(grid, keys, rows, n_match) launches the score kernel (reco_full_score_kernel's
// outputs), then the full pass's stable sort and emit (launch_full_pass). No thresholds: nothing
// can overflow. `what` names the request in the error.
template <typename ScoreFn>
int launch_scored_full(rag_index* h, Workspace& w, const PassArgs& a, hipStream_t st,
                       const char* what, ScoreFn score) {
  const int n = (int)h->count, k = a.k;
  const dim3 egrid((unsigned)std::min<int64_t>(1024, ((int64_t)k + 255) / 256));
  StreamScratch scratch(st);
  if (n == 0) {
    RAG_HIP(scratch.alloc(4));
    RAG_HIP(hipMemsetAsync(scratch.p, 0, 4, st));
    full_emit_kernel<<<egrid, dim3(256), 0, st>>>(nullptr, nullptr,
                                                  reinterpret_cast<const int*>(scratch.p), k,
                                                  a.id_offset, a.out_s, a.out_i, nullptr);
    RAG_HIP(hipGetLastError());
    return RAG_OK;
  }
  size_t tmp_bytes = 0;
  RAG_HIP(hipcub::DeviceRadixSort::SortPairsDescending(
      nullptr, tmp_bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
      static_cast<const int*>(nullptr), static_cast<int*>(nullptr), n, 0, 32, st));
  const size_t nb = (size_t)n * 4;
  const size_t m_off = 4 * nb, t_off = m_off + 256;
  RAG_HIP(scratch.alloc(t_off + tmp_bytes));
  char* const buf = scratch.p;
  uint32_t* k_in = reinterpret_cast<uint32_t*>(buf);
  uint32_t* k_out = reinterpret_cast<uint32_t*>(buf + nb);
  int* v_in = reinterpret_cast<int*>(buf + 2 * nb);
  int* v_out = reinterpret_cast<int*>(buf + 3 * nb);
  int* n_match = reinterpret_cast<int*>(buf + m_off);
  RAG_HIP(hipMemsetAsync(n_match, 0, 4, st));
  // one wave per reco_group rows per step; up to 8 workgroups per CU (launch_full_pass)
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(8 * h->n_cu, (n + 3) / 4));
  score(grid, k_in, v_in, n_match);
  if (hipGetLastError() != hipSuccess ||
      sort_pairs_desc(buf + t_off, tmp_bytes, k_in, k_out, v_in, v_out, n, st) != hipSuccess)
    return ragmi::fail(RAG_EHIP, what);
  full_emit_kernel<<<egrid, dim3(256), 0, st>>>(k_out, v_out, n_match, k, a.id_offset, a.out_s,
                                                a.out_i, nullptr);
  RAG_HIP(hipGetLastError());
  (void)hipMemsetAsync(w.fb_tier, 0, 4, st);   // certified by construction
  return RAG_OK;
}

// The full pass of one BEST / SUM request
template <int D>
int launch_reco_full(rag_index* h, Workspace& w, const RecoArgs& r, const PassArgs& a,
                     hipStream_t st) {
  if (const int rc = launch_reco_prep<D>(h, w, r, st)) return rc;
  ++h->reco_full;
  return launch_scored_full(
      h, w, a, st, "recommend full pass: score / sort launch failed",
      [&](int grid, uint32_t* k_in, int* v_in, int* n_match) {
        with_filter(a.filt, [&](auto f) {
          reco_full_score_kernel<D, decltype(f)::value><<<dim3(grid), dim3(256), 0, st>>>(
              h->corpus, a.tags, a.filt, w.qn, r.P, r.N, r.strat, (int)h->count, h->rows32, k_in,
              v_in, n_match);
        });
      });
}

// AVERAGE_VECTOR's target of a request in w.reco_q's tail (reco_average_kernel)
template <int D>
int launch_reco_average(rag_index* h, Workspace& w, const RecoArgs& r, hipStream_t st) {
  if (const int rc = launch_reco_prep<D>(h, w, r, st)) return rc;
  reco_average_kernel<<<grid1d(D, 256), dim3(256), 0, st>>>(w.qn, D, r.P, r.N,
                                                            w.reco_q + (size_t)kQ * 1024);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// one recommend request under the handle's lock; tags: the stored tags or a filter view
int recommend_locked(rag_index* h, const RecoArgs& r, int k, const uint32_t* filt,
                     const uint32_t* tags, int64_t id_offset, bool full, float* out_s,
                     int64_t* out_i, hipStream_t st) {
  Workspace* wp = nullptr;
  if (const int rc = take_workspace(h, st, 1, &wp)) return rc;
  Workspace& w = *wp;
  if (r.strat == kRecoAverage) {
    // v is the query of the ordinary exact search, every route of it included
    const int rc = with_dim(h->dim, [&](auto d) {
      return launch_reco_average<decltype(d)::value>(h, w, r, st);
    });
    if (rc) return rc;
    return search_locked(h, w.reco_q + (size_t)kQ * 1024, 1, k, filt, id_offset, out_s, out_i,
                         nullptr, st, full, tags);
  }
  const PassArgs a{nullptr, 1, k, filt, tags, id_offset, out_s, out_i, nullptr};
  full = full || k > RAG_MAX_K_LARGE;
  return with_dim(h->dim, [&](auto d) {
    constexpr int D = decltype(d)::value;
    return full ? launch_reco_full<D>(h, w, r, a, st) : launch_reco_hot<D>(h, w, r, a, st);
  });
}

// ---- discovery queries (discover_kernels.hip; the contract: ragmi.h "Discovery queries") ----

// one request: the target ([dim] fp32, device; NULL: a context search) and its n pairs
// (pos / neg [n][dim])
struct DiscArgs {
  const float* target;
  const float* pos;
  const float* neg;
  int n;
  int kind() const { return target ? kDiscover : kContext; }
};

// the argument rules of the discover entry points, checked before any HIP call
int disc_args(const DiscArgs& r) {
  static_assert(kDiscMaxPairs == RAG_DISCOVER_MAX_PAIRS && kCtxMaxPairs == RAG_CONTEXT_MAX_PAIRS &&
                    kCtxMaxPairs == kRecoSide && kDiscTargetSlot == kDiscMaxPairs &&
                    2 * kCtxMaxPairs == kQ,
                "discover_kernels.hip's slots: pair i in slots i and 16 + i, the target in 15");
  if (r.target) {
    if (r.n < 0 || r.n > RAG_DISCOVER_MAX_PAIRS)
      return ragmi::fail(RAG_ERANGE,
                         "discover: a request with a target holds 0 to "
                         "RAG_DISCOVER_MAX_PAIRS=15 pairs");
  } else {
    if (r.n == 0)
      return ragmi::fail(RAG_EINVAL, "discover: a context search (no target) needs a pair");
    if (r.n < 0 || r.n > RAG_CONTEXT_MAX_PAIRS)
      return ragmi::fail(RAG_ERANGE,
                         "discover: a context search holds 1 to RAG_CONTEXT_MAX_PAIRS=16 pairs");
  }
  if (r.n > 0 && (!r.pos || !r.neg))
    return ragmi::fail(RAG_EINVAL, "discover: a NULL pair pointer");
  return RAG_OK;
}

// the request's query block in w (recommend's buffers): slots assembled, prepared by qprep, and
// the request's parameters
template <int D>
int launch_disc_prep(rag_index* h, Workspace& w, const DiscArgs& r, hipStream_t st) {
  static_assert(D <= 1024, "reco_q holds [32][1024]");
  if (const int rc = ensure_reco(w)) return rc;
  disc_assemble_kernel<D><<<dim3(kQ), dim3(64), 0, st>>>(r.target, r.pos, r.neg, r.n, w.reco_q);
  qprep_kernel<D><<<dim3(kQ), dim3(64), 0, st>>>(w.reco_q, kQ, nullptr, w.qn, w.qfrag, w.filt,
                                                  w.eps, store_eps(h));
  disc_prep_kernel<D><<<dim3(1), dim3(64), 0, st>>>(w.eps, w.qn, r.n, w.reco_par);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// go(kind tag) with the kind as a compile-time constant
template <typename F>
auto with_disc_kind(int kind, F&& f) {
  if (kind == kDiscover) return f(std::integral_constant<int, kDiscover>{});
  return f(std::integral_constant<int, kContext>{});
}

// The hot pass of one request, k <= RAG_MAX_K_LARGE (discover_kernels.hip): launch_reco_hot's
// sequence with this feature's kernels. A saturated request (more than kLkCap rows tied at its
// k-th score) overflows round 0 with T already at the tied score, so lk_final_kernel leaves it
// unanswered there and the later rounds' launches return at once.
template <int D>
int launch_disc_hot(rag_index* h, Workspace& w, const DiscArgs& r, const PassArgs& a,
                    hipStream_t st) {
  if (const int rc = ensure_lk(w)) return rc;
  if (const int rc = launch_disc_prep<D>(h, w, r, st)) return rc;
  const int k = a.k, kind = r.kind();
  const int n_tiles = (int)((h->count + 15) / 16);
  // the large-k pass's sample (launch_large_k_pass)
  const int n_sample = n_tiles == 0 ? 0 : std::min({n_tiles, std::max(4 * k, n_tiles / 32),
                                                    kLkSampleMax});
  const int cgrid = (int)std::max<int64_t>(1, std::min<int64_t>(2 * h->n_cu, (n_tiles + 3) / 4));
  const int per_wg = reco_rescore_per_wg(disc_examples(kind, r.n));
  const int rgrid = (kLkCap + per_wg - 1) / per_wg;
  with_filter(a.filt, [&](auto f) {
    with_disc_kind(kind, [&](auto kd) {
      constexpr bool F = decltype(f)::value;
      constexpr int KIND = decltype(kd)::value;
      if (n_sample > 0)
        disc_sample_kernel<D, F, KIND><<<dim3((n_sample + 3) / 4), dim3(256), 0, st>>>(
            h->corpus, a.tags, a.filt, w.qfrag, w.eps, w.reco_par, r.n, (int)h->count, n_tiles,
            n_sample, w.lk_smax);
      // T = the k-th largest sample maximum (L is a bound already: the eps it subtracts is 0)
      lk_bound_kernel<<<dim3(1), dim3(256), 0, st>>>(w.lk_smax, n_sample, k, w.reco_par,
                                                     w.lk_thr, w.lk_cnt, w.lk_again, w.lk_need);
      for (int round = 0; round < kLkRounds; ++round) {
        disc_collect_kernel<D, F, KIND><<<dim3(cgrid), dim3(256), 0, st>>>(
            h->corpus, a.tags, a.filt, w.qfrag, w.eps, w.reco_par, r.n, (int)h->count, n_tiles,
            w.lk_thr, w.lk_cnt, w.lk_cand, w.lk_again, w.lk_need, round);
        disc_rescore_kernel<D><<<dim3(rgrid), dim3(256), 0, st>>>(
            h->corpus, w.qn, kind, r.n, w.lk_cnt, w.lk_cand, w.lk_again, w.lk_need, round,
            w.lk_es, h->rows32, w.reco_par);
        lk_final_kernel<D><<<dim3(1), dim3(256), 0, st>>>(
            h->corpus, w.qn, k, w.lk_cnt, w.lk_cand, w.lk_es, w.reco_par, w.lk_thr, w.lk_again,
            w.lk_need, round, w.fb_tier, w.fb_cnt, a.id_offset, a.out_s, a.out_i, nullptr,
            h->rows32);
      }
    });
  });
  RAG_HIP(hipGetLastError());
  ++h->disc_hot;
  h->disc_last = &w;
  return RAG_OK;
}

// The full pass of one request, any k
template <int D>
int launch_disc_full(rag_index* h, Workspace& w, const DiscArgs& r, const PassArgs& a,
                     hipStream_t st) {
  if (const int rc = launch_disc_prep<D>(h, w, r, st)) return rc;
  ++h->disc_full;
  return launch_scored_full(
      h, w, a, st, "discover full pass: score / sort launch failed",
      [&](int grid, uint32_t* k_in, int* v_in, int* n_match) {
        with_filter(a.filt, [&](auto f) {
          disc_full_score_kernel<D, decltype(f)::value><<<dim3(grid), dim3(256), 0, st>>>(
              h->corpus, a.tags, a.filt, w.qn, r.kind(), r.n, (int)h->count, h->rows32, k_in,
              v_in, n_match);
        });
      });
}

// one discover / context request under the handle's lock; tags: the stored tags or a filter view
int discover_locked(rag_index* h, const DiscArgs& r, int k, const uint32_t* filt,
                    const uint32_t* tags, int64_t id_offset, bool full, float* out_s,
                    int64_t* out_i, hipStream_t st) {
  Workspace* wp = nullptr;
  if (const int rc = take_workspace(h, st, 1, &wp)) return rc;
  Workspace& w = *wp;
  const PassArgs a{nullptr, 1, k, filt, tags, id_offset, out_s, out_i, nullptr};
  full = full || k > RAG_MAX_K_LARGE;
  return with_dim(h->dim, [&](auto d) {
    constexpr int D = decltype(d)::value;
    return full ? launch_disc_full<D>(h, w, r, a, st) : launch_disc_hot<D>(h, w, r, a, st);
  });
}

// ---- sparse vectors (sparse_kernels.hip; the contract: ragmi.h "Sparse vectors") ----

static_assert(kSpQueryNnz == RAG_SPARSE_MAX_QUERY_NNZ && kSpNone == RAG_SPARSE_TERM_NONE &&
                  kSpUnion == RAG_SPARSE_MAX_UNION,
              "sparse_kernels.hip's constants");

// the padded queries of a sparse search (device pointers): terms uint16 [B][64], values fp32
// [B][64], nonzeros int32 [B]
struct SparseQueries {
  const uint16_t* terms;
  const float* vals;
  const int32_t* nnz;
};

int ensure_sparse(Workspace& w) {
  if (w.sp_tab) return RAG_OK;
  if (hipMalloc(reinterpret_cast<void**>(&w.sp_tab), (size_t)kSpTabWords * 4) != hipSuccess) {
    (void)hipGetLastError();
    w.sp_tab = nullptr;
    return ragmi::fail(RAG_ENOMEM, "sparse workspace allocation failed");
  }
  return RAG_OK;
}

// the query table of queries [b0, b0 + Bq) of `sq` in w.sp_tab; filt: their pairs or nullptr
void launch_sparse_prep(Workspace& w, const SparseQueries& sq, int b0, int Bq,
                        const uint32_t* filt, hipStream_t st) {
  sp_prep_kernel<<<dim3(1), dim3(256), 0, st>>>(
      sq.terms + (int64_t)b0 * kSpQueryNnz, sq.vals + (int64_t)b0 * kSpQueryNnz, sq.nnz + b0, Bq,
      filt, w.sp_tab);
}

// the scorer's grid: two workgroups per CU (their LDS tables fill the CU), fewer for few rows
int sparse_grid(const rag_index* h, int64_t wave_items) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(2 * h->n_cu,
                                                      (wave_items + kSpWaves - 1) / kSpWaves));
}

// The hot pass of <= 32 sparse queries, k <= RAG_MAX_K_LARGE: the large-k pass's selection
// (launch_large_k_pass) over exact scores — a sample of 16-row tiles and lk_bound_kernel's
// threshold (eps = 0), kLkRounds (collect, final) pairs; lk_final_kernel reads the scores the
// collect wrote, so nothing is rescored. a.q is unused.
int launch_sparse_hot(rag_index* h, Workspace& w, const SparseQueries& sq, int b0,
                      const PassArgs& a, hipStream_t st) {
  if (const int rc = ensure_lk(w)) return rc;
  const int Bq = a.Bq, k = a.k, S = h->sp_slots, n = (int)h->count;
  launch_sparse_prep(w, sq, b0, Bq, a.filt, st);
  const float* zero_eps = reinterpret_cast<const float*>(w.sp_tab + kSpTabEps);
  const int n_tiles = (n + kSpTileRows - 1) / kSpTileRows;
  const int n_sample = n_tiles == 0 ? 0 : std::min({n_tiles, std::max(4 * k, n_tiles / 32),
                                                    kLkSampleMax});
  if (n_sample > 0)
    sp_score_kernel<kSpSample><<<dim3(sparse_grid(h, n_sample)), dim3(kSpScoreBlock), 0, st>>>(
        h->sp_terms, h->sp_vals, a.tags, S, n, Bq, w.sp_tab, n_tiles, n_sample, w.lk_smax,
        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr);
  lk_bound_kernel<<<dim3(Bq), dim3(256), 0, st>>>(w.lk_smax, n_sample, k, zero_eps, w.lk_thr,
                                                  w.lk_cnt, w.lk_again, w.lk_need);
  const int cgrid = sparse_grid(h, ((int64_t)n + kSpRowGroup - 1) / kSpRowGroup);
  for (int r = 0; r < kLkRounds; ++r) {
    sp_score_kernel<kSpCollect><<<dim3(cgrid), dim3(kSpScoreBlock), 0, st>>>(
        h->sp_terms, h->sp_vals, a.tags, S, n, Bq, w.sp_tab, 0, 0, nullptr, w.lk_thr, w.lk_cnt,
        w.lk_cand, w.lk_es, w.lk_again, w.lk_need, r, nullptr, nullptr, nullptr);
    // (the kernel's dim and row pointers serve the dense rescoring only: unused here)
    lk_final_kernel<384><<<dim3(Bq), dim3(256), 0, st>>>(
        nullptr, nullptr, k, w.lk_cnt, w.lk_cand, w.lk_es, zero_eps, w.lk_thr, w.lk_again,
        w.lk_need, r, w.fb_tier, w.fb_cnt, a.id_offset, a.out_s, a.out_i, nullptr, nullptr);
  }
  sp_overflow_kernel<<<dim3(1), dim3(64), 0, st>>>(w.sp_tab, Bq, w.fb_tier, w.fb_cnt);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// The full pass of <= 32 sparse queries, any k: one query at a time every row scored, the full
// pass's stable sort and emit (launch_full_pass). Always answers: one query's terms never exceed
// the union cap.
int launch_sparse_full(rag_index* h, Workspace& w, const SparseQueries& sq, int b0,
                       const PassArgs& a, hipStream_t st) {
  const int Bq = a.Bq, k = a.k, n = (int)h->count;
  const dim3 egrid((unsigned)std::min<int64_t>(1024, ((int64_t)k + 255) / 256));
  StreamScratch scratch(st);
  if (n == 0) {
    RAG_HIP(scratch.alloc(4));
    RAG_HIP(hipMemsetAsync(scratch.p, 0, 4, st));
    for (int j = 0; j < Bq; ++j)
      full_emit_kernel<<<egrid, dim3(256), 0, st>>>(
          nullptr, nullptr, reinterpret_cast<const int*>(scratch.p), k, a.id_offset,
          a.out_s + (int64_t)j * k, a.out_i + (int64_t)j * k, nullptr);
    RAG_HIP(hipGetLastError());
    return RAG_OK;
  }
  size_t tmp_bytes = 0;
  RAG_HIP(hipcub::DeviceRadixSort::SortPairsDescending(
      nullptr, tmp_bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
      static_cast<const int*>(nullptr), static_cast<int*>(nullptr), n, 0, 32, st));
  const size_t nb = (size_t)n * 4;
  const size_t m_off = 4 * nb, t_off = m_off + 256;
  RAG_HIP(scratch.alloc(t_off + tmp_bytes));
  char* const buf = scratch.p;
  uint32_t* k_in = reinterpret_cast<uint32_t*>(buf);
  uint32_t* k_out = reinterpret_cast<uint32_t*>(buf + nb);
  int* v_in = reinterpret_cast<int*>(buf + 2 * nb);
  int* v_out = reinterpret_cast<int*>(buf + 3 * nb);
  int* n_match = reinterpret_cast<int*>(buf + m_off);
  RAG_HIP(hipMemsetAsync(n_match, 0, 4 * kQ, st));
  const int grid = sparse_grid(h, ((int64_t)n + kSpRowGroup - 1) / kSpRowGroup);
  for (int j = 0; j < Bq; ++j) {
    launch_sparse_prep(w, sq, b0 + j, 1, a.filt ? a.filt + 2 * j : nullptr, st);
    sp_score_kernel<kSpFull><<<dim3(grid), dim3(kSpScoreBlock), 0, st>>>(
        h->sp_terms, h->sp_vals, a.tags, h->sp_slots, n, 1, w.sp_tab, 0, 0, nullptr, nullptr,
        nullptr, nullptr, nullptr, nullptr, nullptr, 0, k_in, v_in, n_match + j);
    if (hipGetLastError() != hipSuccess ||
        sort_pairs_desc(buf + t_off, tmp_bytes, k_in, k_out, v_in, v_out, n, st) != hipSuccess)
      return ragmi::fail(RAG_EHIP, "sparse full pass: score / sort launch failed");
    full_emit_kernel<<<egrid, dim3(256), 0, st>>>(k_out, v_out, n_match + j, k, a.id_offset,
                                                  a.out_s + (int64_t)j * k,
                                                  a.out_i + (int64_t)j * k, nullptr);
    RAG_HIP(hipGetLastError());
  }
  (void)hipMemsetAsync(w.fb_tier, 0, 4 * kQ, st);   // answered by construction
  return RAG_OK;
}

// a sparse search under the handle's lock; tags: the stored tags or a filter view
int sparse_search_locked(rag_index* h, const SparseQueries& sq, int B, int k,
                         const uint32_t* filt, const uint32_t* tags, int64_t id_offset, bool full,
                         float* out_s, int64_t* out_i, hipStream_t st) {
  full = full || k > RAG_MAX_K_LARGE;
  for (int b0 = 0; b0 < B; b0 += kQ) {
    const int Bq = std::min(kQ, B - b0);
    Workspace* wp = nullptr;
    if (const int rc = take_workspace(h, st, Bq, &wp)) return rc;
    if (const int rc = ensure_sparse(*wp)) return rc;
    const PassArgs a{nullptr, Bq, k, filt ? filt + 2 * b0 : nullptr, tags, id_offset,
                     out_s + (int64_t)b0 * k, out_i + (int64_t)b0 * k, nullptr};
    const int rc = full ? launch_sparse_full(h, *wp, sq, b0, a, st)
                        : launch_sparse_hot(h, *wp, sq, b0, a, st);
    if (rc) return rc;
  }
  return RAG_OK;
}

// rag_index_sparse_write / _gather: the shared argument checks, then `launch(grid, stream)` under
// the handle's lock
template <typename F>
int sparse_rows_call(rag_index* h, const int64_t* rows, const void* t, const void* v, int64_t n,
                     void* stream, F&& launch) {
  ragmi::clear_error();
  if (n < 0) return ragmi::fail(RAG_EINVAL, "sparse: n must be >= 0");
  if (n > 0 && (!rows || !t || !v))
    return ragmi::fail(RAG_EINVAL, "sparse: a NULL rows, terms or values pointer");
  if (!h) return ragmi::fail(RAG_EINVAL, "sparse: index is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->sp_slots == 0)
    return ragmi::fail(RAG_EINVAL, "sparse: no sparse column (call rag_index_sparse_create)");
  if (n == 0) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  launch(grid1d(n * h->sp_slots, kSpBlock), static_cast<hipStream_t>(stream));
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// a sparse column of `cap` rows of S slots: rows [0, keep) copied from the old column (may be
// NULL with keep = 0), the rest empty. On the null stream; synchronises the device.
int alloc_sparse(int64_t cap, int S, const uint16_t* old_t, const float* old_v, int64_t keep,
                 DeviceBuf<uint16_t>& nt, DeviceBuf<float>& nv) {
  const int64_t slots = cap * S, kept = keep * S;
  if (nt.alloc((size_t)std::max<int64_t>(slots, 1) * 2) != hipSuccess ||
      nv.alloc((size_t)std::max<int64_t>(slots, 1) * 4) != hipSuccess) {
    (void)hipGetLastError();
    return ragmi::fail(RAG_ENOMEM, "hipMalloc(sparse column) failed");
  }
  RAG_HIP(hipDeviceSynchronize());
  if (kept > 0) {
    RAG_HIP(hipMemcpy(nt.p, old_t, (size_t)kept * 2, hipMemcpyDeviceToDevice));
    RAG_HIP(hipMemcpy(nv.p, old_v, (size_t)kept * 4, hipMemcpyDeviceToDevice));
  }
  if (slots > kept) {
    sp_fill_kernel<<<grid1d(slots - kept, kSpBlock), dim3(kSpBlock), 0, nullptr>>>(nt.p, nv.p,
                                                                                   kept, slots);
    RAG_HIP(hipGetLastError());
  }
  RAG_HIP(hipDeviceSynchronize());
  return RAG_OK;
}

// Diagnostic A/B of scan variants (see scan_kernel's knobs). Returns avg device ms/launch.
template <int D, int V>
void launch_variant(rag_index* h, Workspace& w, int grid, hipStream_t st) {
  const int n_tiles = (int)((h->count + 15) / 16);
  // 0 prod (seeded) | 1 unseeded | 2 contiguous | 3 mfma-only | 4 loads-only | 5 no-nt
  // 6 no-sb | 9 / 10 / 11 dynamic tile queue, chunks of 2 / 1 / 4 tiles | 12 dynamic (2),
  // loads only | 13 / 14 static production / loads only (9-14: each launch timed on its own,
  // the queue heads zeroed between launches outside the timed window) | 15 production without
  // the end-of-scan sort of pending-only queries (results invalid) | 16 production with the
  // round-1 end-of-scan sort (two pending-only queries per 32-lane pass)
  constexpr int MODE = V == 3 ? 1 : V == 4 || V == 12 || V == 14 ? 2 : V == 15 ? 3 : V == 16 ? 4 : 0;
  constexpr bool STRIDED = V != 2;
  constexpr bool NT = V != 5;
  constexpr bool SB = V != 6;
  constexpr int DYN = V == 9 || V == 12 ? 2 : V == 10 ? 1 : V == 11 ? 4 : 0;
  launch_fixed<kScanBlock>(scan_kernel<D, false, MODE, STRIDED, NT, SB, DYN>, dim3(grid), 0, st,
                           h->corpus, h->tags, w.filt, w.qfrag, (int)h->count, n_tiles,
                           V == 1 ? nullptr : w.seed, w.part_s, w.part_i, w.heads_s, w.heads_i,
                           w.heads_n, w.tileq);
}

template <int D>
int bench_scan(rag_index* h, const float* q, int B, int variant, int reps, double* avg_ms) {
  Workspace& w = h->ws[0];
  RAG_HIP(hipDeviceSynchronize());
  qprep_kernel<D><<<dim3(kQ), dim3(64), 0, nullptr>>>(q, std::min(B, kQ), nullptr, w.qn,
                                                      w.qfrag, w.filt, w.eps, store_eps(h));
  launch_seed<D, false>(h, w, 1, h->tags, nullptr);
  // variant 7: the production kernel with every seed threshold at +inf, i.e. the top-k's
  // per-tile compares and branches with no candidate ever taken (its fixed cost)
  if (variant == 7)
    RAG_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(w.seed), 0x7f800000, kQ));
  // the production grid of an unfiltered fp16 pass on an unpartitioned stream
  const int grid = scan_grid(h, 0, false, kNoCopy);
#ifdef RAGMI_DIAG_BUILD
  const int64_t n_tiles = (h->count + 15) / 16;
  // variant 8: the v_dot2 VALU ablation over a row-group-major copy of the corpus
  DeviceBuf<half8> rows64, qc;
  const int n_groups = (int)((h->count + 63) / 64);
  const int vgrid = std::min(h->max_wgs, std::max(1, (n_groups + 3) / 4));
  if (variant == 8) {
    RAG_HIP(rows64.alloc((size_t)n_groups * 64 * D * 2));
    RAG_HIP(qc.alloc((size_t)kQ * D * 2));
    RAG_HIP(hipMemset(rows64.p, 0, (size_t)n_groups * 64 * D * 2));
    rows64_kernel<D><<<grid1d(h->count * (D / 8), 256), dim3(256), 0, nullptr>>>(
        h->corpus, h->count, rows64.p);
    qchunk_kernel<D><<<dim3(kQ), dim3(64), 0, nullptr>>>(w.qn, qc.p);
  }
  // variants 17 / 18 / 19: the int8 prescan (scan_kernel_i8) at its production grid —
  // production, MFMA + bound only (no top-k), loads only. Variants 20 / 21 / 22 / 23 / 24: the
  // 6-bit prescan (scan_kernel_i6) at its own — the same three, loads + unpack, production with
  // every seed at +inf (the top-k's fixed cost: no candidate is ever taken)
  if (variant >= 17) {
    const CopyKind kind = variant >= 20 ? kCopy6 : kCopy8;
    if constexpr (D == 384) {
      if (!h->copy[kind].data)
        return ragmi::fail(RAG_EINVAL, kind == kCopy6 ? "variants 20-24: index keeps no 6-bit copy"
                                                      : "variants 17-19: index keeps no int8 copy");
      launch_prep8<D>(h, w, q, std::min(B, kQ), nullptr, h->tags, nullptr, kind);
      if (variant == 24)
        RAG_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(w.seed), 0x7f800000, kQ));
      const int grid = scan_grid(h, 0, false, kind);
      const int mode = variant == 24 ? 0 : variant - (kind == kCopy6 ? 20 : 17);
      const auto go = [&](auto kernel) {
        launch_fixed<kScanBlock>(kernel, dim3(grid), 0, nullptr, h->copy[kind].data,
                                 h->copy[kind].meta, h->tags, w.filt,
                                 reinterpret_cast<const intx4*>(w.qfrag8), w.qp8, (int)h->count,
                                 (int)n_tiles, w.seed, w.part_s, w.part_i, w.heads_s, w.heads_i,
                                 w.heads_n);
      };
      return time_launches(reps, [&]() {
        if (kind == kCopy8) {
          if (mode == 0) go(scan_kernel_i8<D, false, 0>);
          else if (mode == 1) go(scan_kernel_i8<D, false, 1>);
          else go(scan_kernel_i8<D, false, 2>);
        } else {
          if (mode == 0) go(scan_kernel_i6<D, false, 0>);
          else if (mode == 1) go(scan_kernel_i6<D, false, 1>);
          else if (mode == 2) go(scan_kernel_i6<D, false, 2>);
          else go(scan_kernel_i6<D, false, 3>);
        }
      }, avg_ms);
    } else {
      return ragmi::fail(RAG_EINVAL, kind == kCopy6 ? "variants 20-24: dim 384 only"
                                                    : "variants 17-19: dim 384 only");
    }
  }
#endif
  auto one = [&]() {
#ifndef RAGMI_DIAG_BUILD
    // production library: the production scan only (variants 0 and 7); the MODE / DYN /
    // VALU probes are instantiated in the diagnostic build alone
    launch_variant<D, 0>(h, w, grid, nullptr);
#else
    if (variant == 8) {
      scan_valu_kernel<D><<<dim3(vgrid), dim3(256), 0, nullptr>>>(
          rows64.p, qc.p, (int)h->count, n_groups, w.seed, w.part_s, w.part_i, w.heads_s,
          w.heads_i, w.heads_n);
      return;
    }
    switch (variant) {
      case 0: launch_variant<D, 0>(h, w, grid, nullptr); break;
      case 1: launch_variant<D, 1>(h, w, grid, nullptr); break;
      case 2: launch_variant<D, 2>(h, w, grid, nullptr); break;
      case 3: launch_variant<D, 3>(h, w, grid, nullptr); break;
      case 4: launch_variant<D, 4>(h, w, grid, nullptr); break;
      case 5: launch_variant<D, 5>(h, w, grid, nullptr); break;
      case 7: launch_variant<D, 0>(h, w, grid, nullptr); break;
      case 15: launch_variant<D, 15>(h, w, grid, nullptr); break;
      case 16: launch_variant<D, 16>(h, w, grid, nullptr); break;
      default: launch_variant<D, 6>(h, w, grid, nullptr); break;
    }
#endif
  };
#ifdef RAGMI_DIAG_BUILD
  if (variant >= 9 && variant <= 14) {
    // one launch per event pair; the tile-queue heads are zeroed before each, outside it
    float ms = 0.f;
    EventPair ev;
    RAG_HIP(ev.create());
    for (int r = -1; r < reps; ++r) {
      RAG_HIP(hipMemsetAsync(w.tileq, 0, 8 * kTileQStride * 4, nullptr));
      RAG_HIP(hipEventRecord(ev.a, nullptr));
      switch (variant) {
        case 9: launch_variant<D, 9>(h, w, grid, nullptr); break;
        case 10: launch_variant<D, 10>(h, w, grid, nullptr); break;
        case 11: launch_variant<D, 11>(h, w, grid, nullptr); break;
        case 12: launch_variant<D, 12>(h, w, grid, nullptr); break;
        case 13: launch_variant<D, 0>(h, w, grid, nullptr); break;
        default: launch_variant<D, 14>(h, w, grid, nullptr); break;
      }
      RAG_HIP(hipEventRecord(ev.b, nullptr));
      RAG_HIP(hipEventSynchronize(ev.b));
      float m1 = 0.f;
      RAG_HIP(hipEventElapsedTime(&m1, ev.a, ev.b));
      if (r >= 0) ms += m1;   // r = -1: warm-up
    }
    RAG_HIP(hipGetLastError());
    *avg_ms = ms / reps;
    return RAG_OK;
  }
#endif
  return time_launches(reps, one, avg_ms);
}

// Diagnostic A/B of the wide (D = 1024, 33..128 queries, unfiltered) scan's variants
// (scan_wide_kernel MODE 0..4; 0 is production). Returns avg device ms/launch.
template <int D>
int bench_wide(rag_index* h, const float* q, int B, int mode, int reps, double* avg_ms) {
  Workspace& w = h->ws[0];
  const int groups = (std::min(B, kQ * kMaxGroups) + kQ - 1) / kQ;
  if (groups < 2) return ragmi::fail(RAG_EINVAL, "wide scan variants need 33..128 queries");
  RAG_HIP(hipDeviceSynchronize());
  qprep_kernel<D><<<dim3(groups * kQ), dim3(64), 0, nullptr>>>(
      q, std::min(B, groups * kQ), nullptr, w.qn, w.qfrag, w.filt, w.eps, store_eps(h));
  launch_seed<D, false>(h, w, groups, h->tags, nullptr);
  const int64_t n_tiles = (h->count + 15) / 16;
  const int grid = (int)std::min<int64_t>(h->max_wgs / 2, std::max<int64_t>(1, n_tiles));
  auto one = [&]() {
#define RAG_WIDE(MODE)                                                                     \
  launch_fixed<kWideBlock>(scan_wide_kernel<D, MODE, true>, dim3(grid), 0, nullptr,          \
                           h->corpus, w.qfrag, (int)h->count, (int)n_tiles, w.seed, w.part_s, \
                           w.part_i, w.heads_s, w.heads_i, w.heads_n, groups)
#ifdef RAGMI_DIAG_BUILD
    switch (mode) {
      case 1: RAG_WIDE(1); break;
      case 2: RAG_WIDE(2); break;
      case 3: RAG_WIDE(3); break;
      case 4: RAG_WIDE(4); break;
      default: RAG_WIDE(0); break;
    }
#else
    RAG_WIDE(0);
#endif
#undef RAG_WIDE
  };
  return time_launches(reps, one, avg_ms);
}

// tot += the tier-1 / tier-2 / unanswered totals of the ring (lock held; drains the device)
int read_fb_totals(rag_index* h, unsigned long long (&tot)[3]) {
  RAG_HIP(hipSetDevice(h->device));
  RAG_HIP(hipDeviceSynchronize());
  for (auto& w : h->ws) {
    unsigned long long c[3];
    RAG_HIP(hipMemcpy(c, w.fb_cnt, sizeof(c), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) tot[i] += c[i];
  }
  return RAG_OK;
}

// a stream of `device` (made current for the call only) restricted to the CUs of `mask`
int create_masked_stream(int device, const uint32_t* mask, uint32_t words, void** out) {
  int prev = 0;
  RAG_HIP(hipGetDevice(&prev));
  RAG_HIP(hipSetDevice(device));
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, words, mask);
  (void)hipSetDevice(prev);
  if (e != hipSuccess)
    return ragmi::fail(RAG_EHIP, std::string("hipExtStreamCreateWithCUMask: ") + hipGetErrorString(e));
  *out = st;
  g_stream_gen.fetch_add(1, std::memory_order_acq_rel);
  return RAG_OK;
}

}  // namespace

hipError_t ragmi::alloc_workspaces(rag_index* h) {
  hipError_t e = hipSuccess;
  // one hipMalloc per buffer, in the table's order (see ragmi/dist.py on allocation placement)
  for (auto& w : h->ws)
    if (e == hipSuccess) e = ws_alloc_all(ws_buffers(h, w));
  return e;
}

void ragmi::free_workspaces(rag_index* h) {
  for (auto& w : h->ws) {
    ws_free_all(ws_buffers(h, w));
    ws_free_all(lk_buffers(w));
    ws_free_all(reco_buffers(w));
    if (w.sp_tab) (void)hipFree(w.sp_tab);
    w.sp_tab = nullptr;
    if (w.ev_in) (void)hipEventDestroy(w.ev_in);
    if (w.ev_out) (void)hipEventDestroy(w.ev_out);
  }
}

int ragmi::remap_shard_ids(int64_t* ids, int B, int k, int n, uint8_t* out_empty, hipStream_t st) {
  const unsigned gx = (unsigned)std::min<size_t>(1024, ((size_t)B * k + 255) / 256);
  remap_ids_kernel<<<dim3(gx, n), dim3(256), 0, st>>>(ids, B, k, n, out_empty);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

int ragmi::sparse_move_rows(rag_index* h, const int64_t* src_rows, const int64_t* dst_rows,
                            int64_t n, hipStream_t st) {
  sp_move_kernel<<<grid1d(n * h->sp_slots, kSpBlock), dim3(kSpBlock), 0, st>>>(
      h->sp_terms, h->sp_vals, src_rows, dst_rows, n, h->sp_slots, h->cap_rows);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

int ragmi::sparse_reserve(rag_index* h, int64_t cap) {
  DeviceBuf<uint16_t> nt;
  DeviceBuf<float> nv;
  if (const int rc = alloc_sparse(cap, h->sp_slots, h->sp_terms, h->sp_vals, h->cap_rows, nt, nv))
    return rc;
  (void)hipFree(h->sp_terms);
  (void)hipFree(h->sp_vals);
  h->sp_terms = nt.release();
  h->sp_vals = nv.release();
  return RAG_OK;
}

extern "C" {

int rag_index_search(rag_index_t* h, const float* q, int B, int k, const uint32_t* filters,
                     int64_t id_offset, float* out_s, int64_t* out_i, void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  return search_locked(h, q, B, k, filters, id_offset, out_s, out_i, nullptr,
                       static_cast<hipStream_t>(stream));
}

int rag_index_search_full(rag_index_t* h, const float* q, int B, int k, const uint32_t* filters,
                          int64_t id_offset, float* out_s, int64_t* out_i, void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  return search_locked(h, q, B, k, filters, id_offset, out_s, out_i, nullptr,
                       static_cast<hipStream_t>(stream), true);
}

int rag_index_search_packed(rag_index_t* h, const float* q, int B, int k,
                            const uint32_t* filters, int64_t id_offset, int32_t* out_packed,
                            void* stream) {
  ragmi::clear_error();
  if (!h || (B > 0 && !out_packed)) return ragmi::fail(RAG_EINVAL, "bad packed search args");
  if (const int rc = packed_ids_args(h, id_offset)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  return search_locked(h, q, B, k, filters, id_offset, nullptr, nullptr, out_packed,
                       static_cast<hipStream_t>(stream));
}

int rag_index_search_host(rag_index_t* h, const float* q, int B, int k,
                          const uint32_t* filters, int64_t id_offset, float* out_s,
                          int64_t* out_i) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (const int rc = search_args(q, B, k, out_s, out_i, nullptr)) return rc;
  if (B == 0) return RAG_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  // staging offsets rounded to 16 B (the int64 ids must be 8-B aligned for any B * k)
  auto up16 = [](size_t x) { return (x + 15) & ~size_t(15); };
  const size_t qb = up16((size_t)B * h->dim * 4), sb = up16((size_t)B * k * 4);
  const size_t ib = up16((size_t)B * k * 8), fb = (size_t)B * 8;
  int rc = ensure_stage(h, qb + sb + ib + fb + 64);
  if (rc) return rc;
  char* base = static_cast<char*>(h->stage);
  RAG_HIP(hipDeviceSynchronize());
  RAG_HIP(hipMemcpy(base, q, (size_t)B * h->dim * 4, hipMemcpyHostToDevice));
  if (filters) RAG_HIP(hipMemcpy(base + qb + sb + ib, filters, fb, hipMemcpyHostToDevice));
  rc = search_locked(h, reinterpret_cast<float*>(base), B, k,
                     filters ? reinterpret_cast<uint32_t*>(base + qb + sb + ib) : nullptr,
                     id_offset, reinterpret_cast<float*>(base + qb),
                     reinterpret_cast<int64_t*>(base + qb + sb), nullptr, nullptr);
  if (rc) return rc;
  RAG_HIP(hipDeviceSynchronize());
  RAG_HIP(hipMemcpy(out_s, base + qb, (size_t)B * k * 4, hipMemcpyDeviceToHost));
  RAG_HIP(hipMemcpy(out_i, base + qb + sb, (size_t)B * k * 8, hipMemcpyDeviceToHost));
  return RAG_OK;
}

int rag_index_search_view(rag_index_t* h, const float* q, int B, int k, const uint32_t* progs,
                          int64_t words, int n_programs, const uint32_t* filters,
                          int64_t id_offset, int flags, float* out_s, int64_t* out_i,
                          int32_t* out_packed, void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (const int rc = view_args(progs, words, n_programs)) return rc;
  if (flags & ~RAG_SEARCH_FULL) return ragmi::fail(RAG_EINVAL, "view search: unknown flags");
  if (const int rc = search_args(q, B, k, out_s, out_i, out_packed)) return rc;
  if (out_packed && (flags & RAG_SEARCH_FULL))
    return ragmi::fail(RAG_EINVAL, "view search: the full exact pass has no packed form");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  if (out_packed)
    if (const int rc = packed_ids_args(h, id_offset)) return rc;
  if (B == 0) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  // view and search under this one hold of the lock: a delete moves rows (and their tags)
  // under the same lock, so the view cannot disagree with the rows the passes read
  uint32_t* v = nullptr;
  if (const int rc = acquire_view(h, st, &v)) return rc;
  if (const int rc = launch_filter_view(h, progs, words, n_programs, v, st)) return rc;
  return search_locked(h, q, B, k, filters, id_offset, out_s, out_i, out_packed, st,
                       (flags & RAG_SEARCH_FULL) != 0, v);
}

// ---- recommend queries (reco_kernels.hip) ----

int rag_index_recommend(rag_index_t* h, const float* pos, int n_pos, const float* neg, int n_neg,
                        int strategy, int k, const uint32_t* progs, int64_t words, int n_programs,
                        const uint32_t* filter, int64_t id_offset, int flags, float* out_s,
                        int64_t* out_i, void* stream) {
  ragmi::clear_error();
  const RecoArgs r{pos, n_pos, neg, n_neg, strategy};
  if (const int rc = reco_args(r, true)) return rc;
  if (k < 1) return ragmi::fail(RAG_ERANGE, "recommend: k must be >= 1");
  if (flags & ~RAG_SEARCH_FULL) return ragmi::fail(RAG_EINVAL, "recommend: unknown flags");
  if (progs) {
    if (const int rc = view_args(progs, words, n_programs)) return rc;
  } else if (words != 0 || n_programs != 0) {
    return ragmi::fail(RAG_EINVAL, "recommend: programs is NULL but words / n_programs are not 0");
  }
  if (!out_s || !out_i) return ragmi::fail(RAG_EINVAL, "recommend: a NULL output pointer");
  if (!h) return ragmi::fail(RAG_EINVAL, "recommend: index is NULL");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  // view and passes under this one hold of the lock (rag_index_search_view)
  const uint32_t* tags = h->tags;
  if (progs) {
    uint32_t* v = nullptr;
    if (const int rc = acquire_view(h, st, &v)) return rc;
    if (const int rc = launch_filter_view(h, progs, words, n_programs, v, st)) return rc;
    tags = v;
  }
  return recommend_locked(h, r, k, filter, tags, id_offset, (flags & RAG_SEARCH_FULL) != 0, out_s,
                          out_i, st);
}

// ---- sparse vectors (sparse_kernels.hip) ----

int rag_index_sparse_create(rag_index_t* h, int slots) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "sparse_create: index is NULL");
  if (slots < 16 || slots > RAG_SPARSE_MAX_SLOTS || slots % 16 != 0)
    return ragmi::fail(RAG_EINVAL, "sparse_create: slots must be a multiple of 16 in [16, 512]");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->sp_slots == slots) return RAG_OK;
  if (h->sp_slots != 0)
    return ragmi::fail(RAG_EINVAL, "sparse_create: the column exists with another slot count");
  RAG_HIP(hipSetDevice(h->device));
  DeviceBuf<uint16_t> nt;
  DeviceBuf<float> nv;
  if (const int rc = alloc_sparse(h->cap_rows, slots, nullptr, nullptr, 0, nt, nv)) return rc;
  h->sp_terms = nt.release();
  h->sp_vals = nv.release();
  h->sp_slots = slots;
  return RAG_OK;
}

int rag_index_sparse_slots(const rag_index_t* h) { return h ? h->sp_slots : 0; }

int rag_index_sparse_write(rag_index_t* h, const int64_t* rows, const uint16_t* terms,
                           const float* vals, int64_t n, void* stream) {
  return sparse_rows_call(h, rows, terms, vals, n, stream, [&](dim3 grid, hipStream_t st) {
    sp_write_kernel<<<grid, dim3(kSpBlock), 0, st>>>(h->sp_terms, h->sp_vals, rows, terms, vals, n,
                                                     h->sp_slots, h->cap_rows);
  });
}

int rag_index_sparse_gather(rag_index_t* h, const int64_t* rows, int64_t n, uint16_t* out_terms,
                            float* out_vals, void* stream) {
  return sparse_rows_call(h, rows, out_terms, out_vals, n, stream, [&](dim3 grid, hipStream_t st) {
    sp_gather_kernel<<<grid, dim3(kSpBlock), 0, st>>>(h->sp_terms, h->sp_vals, rows, n,
                                                      h->sp_slots, h->cap_rows, out_terms,
                                                      out_vals);
  });
}

int rag_index_sparse_df(rag_index_t* h, int64_t* out_df, void* stream) {
  ragmi::clear_error();
  if (!out_df) return ragmi::fail(RAG_EINVAL, "sparse_df: a NULL output pointer");
  if (!h) return ragmi::fail(RAG_EINVAL, "sparse_df: index is NULL");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->sp_slots == 0)
    return ragmi::fail(RAG_EINVAL, "sparse_df: no sparse column (call rag_index_sparse_create)");
  RAG_HIP(hipSetDevice(h->device));
  RAG_HIP(hipMemsetAsync(out_df, 0, (size_t)kSpTerms * 8, st));
  const int64_t slots = h->count * h->sp_slots;
  if (slots > 0) {
    const int64_t grid = std::min<int64_t>(8 * h->n_cu, (slots + kSpBlock - 1) / kSpBlock);
    sp_df_kernel<<<dim3((unsigned)grid), dim3(kSpBlock), 0, st>>>(
        h->sp_terms, slots, reinterpret_cast<unsigned long long*>(out_df));
    RAG_HIP(hipGetLastError());
  }
  return RAG_OK;
}

int rag_index_sparse_search(rag_index_t* h, const uint16_t* q_terms, const float* q_vals,
                            const int32_t* q_nnz, int B, int k, const uint32_t* progs,
                            int64_t words, int n_programs, const uint32_t* filters,
                            int64_t id_offset, int flags, float* out_s, int64_t* out_i,
                            void* stream) {
  ragmi::clear_error();
  if (B < 0 || (B > 0 && (!q_terms || !q_vals || !q_nnz || !out_s || !out_i)))
    return ragmi::fail(RAG_EINVAL, "sparse_search: bad arguments (B < 0 or a NULL pointer)");
  if (k < 1) return ragmi::fail(RAG_ERANGE, "sparse_search: k must be >= 1");
  if (flags & ~RAG_SEARCH_FULL) return ragmi::fail(RAG_EINVAL, "sparse_search: unknown flags");
  if (progs) {
    if (const int rc = view_args(progs, words, n_programs)) return rc;
  } else if (words != 0 || n_programs != 0) {
    return ragmi::fail(RAG_EINVAL,
                       "sparse_search: programs is NULL but words / n_programs are not 0");
  }
  if (!h) return ragmi::fail(RAG_EINVAL, "sparse_search: index is NULL");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->sp_slots == 0)
    return ragmi::fail(RAG_EINVAL,
                       "sparse_search: no sparse column (call rag_index_sparse_create)");
  if (B == 0) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  // view and passes under this one hold of the lock (rag_index_search_view)
  const uint32_t* tags = h->tags;
  if (progs) {
    uint32_t* v = nullptr;
    if (const int rc = acquire_view(h, st, &v)) return rc;
    if (const int rc = launch_filter_view(h, progs, words, n_programs, v, st)) return rc;
    tags = v;
  }
  return sparse_search_locked(h, SparseQueries{q_terms, q_vals, q_nnz}, B, k, filters, tags,
                              id_offset, (flags & RAG_SEARCH_FULL) != 0, out_s, out_i, st);
}

int rag_index_reco_bounds(rag_index_t* h, const float* pos, int n_pos, const float* neg, int n_neg,
                          int strategy, const int64_t* rows_dev, int64_t n, float* out_lo,
                          float* out_hi, void* stream) {
  ragmi::clear_error();
  const RecoArgs r{pos, n_pos, neg, n_neg, strategy};
  if (const int rc = reco_args(r, false)) return rc;
  if (n < 0 || (n > 0 && (!rows_dev || !out_lo || !out_hi)))
    return ragmi::fail(RAG_EINVAL, "reco_bounds: a NULL row or output pointer");
  if (n > 0x7fffffff) return ragmi::fail(RAG_ERANGE, "reco_bounds: n too large for one call");
  if (!h) return ragmi::fail(RAG_EINVAL, "reco_bounds: index is NULL");
  if (n == 0) return RAG_OK;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  Workspace* wp = nullptr;
  if (const int rc = take_workspace(h, st, 1, &wp)) return rc;
  Workspace& w = *wp;
  return with_dim(h->dim, [&](auto d) {
    constexpr int D = decltype(d)::value;
    if (const int rc = launch_reco_prep<D>(h, w, r, st)) return rc;
    with_reco_strategy(r.strat, [&](auto s) {
      reco_bounds_kernel<D, decltype(s)::value><<<dim3((unsigned)n), dim3(64), 0, st>>>(
          h->corpus, w.qfrag, w.eps, w.reco_par, r.P, r.N, rows_dev, n, h->count, out_lo, out_hi);
    });
    RAG_HIP(hipGetLastError());
    return (int)RAG_OK;
  });
}

int rag_index_reco_vector(rag_index_t* h, const float* pos, int n_pos, const float* neg, int n_neg,
                          float* out_v, void* stream) {
  ragmi::clear_error();
  const RecoArgs r{pos, n_pos, neg, n_neg, RAG_RECO_AVERAGE};
  if (const int rc = reco_args(r, true)) return rc;
  if (!out_v) return ragmi::fail(RAG_EINVAL, "reco_vector: a NULL output pointer");
  if (!h) return ragmi::fail(RAG_EINVAL, "reco_vector: index is NULL");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  Workspace* wp = nullptr;
  if (const int rc = take_workspace(h, st, 1, &wp)) return rc;
  const int rc = with_dim(h->dim, [&](auto d) {
    return launch_reco_average<decltype(d)::value>(h, *wp, r, st);
  });
  if (rc) return rc;
  RAG_HIP(hipMemcpyAsync(out_v, wp->reco_q + (size_t)kQ * 1024, (size_t)h->dim * 4,
                         hipMemcpyDeviceToDevice, st));
  return RAG_OK;
}

int rag_index_reco_stats(rag_index_t* h, int64_t out[4]) {
  ragmi::clear_error();
  if (!h || !out) return ragmi::fail(RAG_EINVAL, "reco_stats: bad args");
  std::lock_guard<std::mutex> lk(h->mu);
  out[0] = h->reco_hot;
  out[1] = h->reco_full;
  out[2] = out[3] = 0;
  if (h->reco_last) {
    RAG_HIP(hipSetDevice(h->device));
    RAG_HIP(hipDeviceSynchronize());
    int32_t c[2];
    RAG_HIP(hipMemcpy(c, reinterpret_cast<const int32_t*>(h->reco_last->reco_par) + kRecoParCnt,
                      sizeof(c), hipMemcpyDeviceToHost));
    out[2] = c[0];
    out[3] = c[1];
  }
  return RAG_OK;
}

// ---- discovery queries (discover_kernels.hip) ----

int rag_index_discover(rag_index_t* h, const float* target, const float* pos, const float* neg,
                       int n_pairs, int k, const uint32_t* progs, int64_t words, int n_programs,
                       const uint32_t* filter, int64_t id_offset, int flags, float* out_s,
                       int64_t* out_i, void* stream) {
  ragmi::clear_error();
  const DiscArgs r{target, pos, neg, n_pairs};
  if (const int rc = disc_args(r)) return rc;
  if (k < 1) return ragmi::fail(RAG_ERANGE, "discover: k must be >= 1");
  if (flags & ~RAG_SEARCH_FULL) return ragmi::fail(RAG_EINVAL, "discover: unknown flags");
  if (progs) {
    if (const int rc = view_args(progs, words, n_programs)) return rc;
  } else if (words != 0 || n_programs != 0) {
    return ragmi::fail(RAG_EINVAL, "discover: programs is NULL but words / n_programs are not 0");
  }
  if (!out_s || !out_i) return ragmi::fail(RAG_EINVAL, "discover: a NULL output pointer");
  if (!h) return ragmi::fail(RAG_EINVAL, "discover: index is NULL");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  // view and passes under this one hold of the lock (rag_index_search_view)
  const uint32_t* tags = h->tags;
  if (progs) {
    uint32_t* v = nullptr;
    if (const int rc = acquire_view(h, st, &v)) return rc;
    if (const int rc = launch_filter_view(h, progs, words, n_programs, v, st)) return rc;
    tags = v;
  }
  return discover_locked(h, r, k, filter, tags, id_offset, (flags & RAG_SEARCH_FULL) != 0, out_s,
                         out_i, st);
}

int rag_index_discover_bounds(rag_index_t* h, const float* target, const float* pos,
                              const float* neg, int n_pairs, const int64_t* rows_dev, int64_t n,
                              float* out_lo, float* out_hi, void* stream) {
  ragmi::clear_error();
  const DiscArgs r{target, pos, neg, n_pairs};
  if (const int rc = disc_args(r)) return rc;
  if (n < 0 || (n > 0 && (!rows_dev || !out_lo || !out_hi)))
    return ragmi::fail(RAG_EINVAL, "discover_bounds: a NULL row or output pointer");
  if (n > 0x7fffffff) return ragmi::fail(RAG_ERANGE, "discover_bounds: n too large for one call");
  if (!h) return ragmi::fail(RAG_EINVAL, "discover_bounds: index is NULL");
  if (n == 0) return RAG_OK;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  Workspace* wp = nullptr;
  if (const int rc = take_workspace(h, st, 1, &wp)) return rc;
  Workspace& w = *wp;
  return with_dim(h->dim, [&](auto d) {
    constexpr int D = decltype(d)::value;
    if (const int rc = launch_disc_prep<D>(h, w, r, st)) return rc;
    with_disc_kind(r.kind(), [&](auto kd) {
      disc_bounds_kernel<D, decltype(kd)::value><<<dim3((unsigned)n), dim3(64), 0, st>>>(
          h->corpus, w.qfrag, w.eps, w.reco_par, r.n, rows_dev, n, h->count, out_lo, out_hi);
    });
    RAG_HIP(hipGetLastError());
    return (int)RAG_OK;
  });
}

int rag_index_discover_stats(rag_index_t* h, int64_t out[4]) {
  ragmi::clear_error();
  if (!h || !out) return ragmi::fail(RAG_EINVAL, "discover_stats: bad args");
  std::lock_guard<std::mutex> lk(h->mu);
  out[0] = h->disc_hot;
  out[1] = h->disc_full;
  out[2] = out[3] = 0;
  if (h->disc_last) {
    RAG_HIP(hipSetDevice(h->device));
    RAG_HIP(hipDeviceSynchronize());
    int32_t c[2];
    RAG_HIP(hipMemcpy(c, reinterpret_cast<const int32_t*>(h->disc_last->reco_par) + kDiscParCnt,
                      sizeof(c), hipMemcpyDeviceToHost));
    out[2] = c[0];
    out[3] = c[1];
  }
  return RAG_OK;
}

// ---- MMR re-selection (mmr_kernel, reselect_kernels.hip) ----

int rag_index_mmr(rag_index_t* h, const float* cand_s, const int64_t* cand_r, int B, int C, int k,
                  const float* diversity, const int32_t* ncand, float* out_s, int64_t* out_i,
                  int32_t* out_pos, void* stream) {
  ragmi::clear_error();
  static_assert(ragmi::kMmrMaxC == RAG_MMR_MAX_CANDIDATES, "mmr_kernel's LDS lists");
  if (C < 1 || C > RAG_MMR_MAX_CANDIDATES)
    return ragmi::fail(RAG_ERANGE, "mmr: C must be in [1, RAG_MMR_MAX_CANDIDATES=1024]");
  if (k < 1) return ragmi::fail(RAG_ERANGE, "mmr: k must be >= 1");
  if (B < 0) return ragmi::fail(RAG_EINVAL, "mmr: B must be >= 0");
  if (!h) return ragmi::fail(RAG_EINVAL, "mmr: index is NULL");
  if (B > 0 && (!cand_s || !cand_r || !diversity || !out_s || !out_i))
    return ragmi::fail(RAG_EINVAL, "mmr: a NULL candidate, diversity or output pointer");
  if (B == 0) return RAG_OK;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  const int rc = with_dim(h->dim, [&](auto d) {
    ragmi::mmr_kernel<decltype(d)::value><<<dim3((unsigned)B), dim3(ragmi::kMmrBlock), 0, st>>>(
        h->corpus, h->rows32, h->cap_rows, cand_s, cand_r, C, k, diversity, ncand, out_s, out_i,
        out_pos);
    return RAG_OK;
  });
  if (rc) return rc;
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// ---- grouped search: group selection (reselect_kernels.hip) ----

int rag_group_select(const float* cand_s, const int64_t* cand_r, const uint32_t* cand_t,
                     const int32_t* ncand, int B, int C, uint32_t key_mask, int G, int S,
                     uint32_t* out_keys, int32_t* out_fill, float* out_s, int64_t* out_r,
                     int32_t* out_pos, int32_t* out_count, void* stream) {
  ragmi::clear_error();
  static_assert(ragmi::kGrpMaxC == RAG_GROUPS_MAX_CANDIDATES && ragmi::kGrpMaxG == RAG_GROUPS_MAX &&
                    ragmi::kGrpMaxCells == RAG_GROUPS_MAX_CELLS &&
                    RAG_GROUPS_MAX_CANDIDATES == RAG_MAX_K_LARGE,
                "group_select_kernel's LDS arrays");
  if (C < 1 || C > RAG_GROUPS_MAX_CANDIDATES)
    return ragmi::fail(RAG_ERANGE, "group_select: C must be in [1, RAG_GROUPS_MAX_CANDIDATES=4096]");
  if (G < 1 || G > RAG_GROUPS_MAX)
    return ragmi::fail(RAG_ERANGE, "group_select: G must be in [1, RAG_GROUPS_MAX=1024]");
  if (S < 1) return ragmi::fail(RAG_ERANGE, "group_select: S must be >= 1");
  if ((int64_t)G * S > RAG_GROUPS_MAX_CELLS)
    return ragmi::fail(RAG_ERANGE, "group_select: G * S must be <= RAG_GROUPS_MAX_CELLS=4096");
  if (key_mask == 0) return ragmi::fail(RAG_EINVAL, "group_select: key_mask is 0");
  if (B < 0) return ragmi::fail(RAG_EINVAL, "group_select: B must be >= 0");
  if (B > 0 && (!cand_s || !cand_r || !cand_t || !out_keys || !out_fill || !out_s || !out_r ||
                !out_count))
    return ragmi::fail(RAG_EINVAL, "group_select: a NULL candidate or output pointer");
  if (B == 0) return RAG_OK;
  ragmi::group_select_kernel<<<dim3((unsigned)B), dim3(ragmi::kGrpBlock), 0,
                               static_cast<hipStream_t>(stream)>>>(
      cand_s, cand_r, cand_t, ncand, C, key_mask, G, S, out_keys, out_fill, out_s, out_r, out_pos,
      out_count);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// ---- fusion queries: reciprocal rank fusion of candidate lists (reselect_kernels.hip) ----

int rag_fuse_rrf(const int64_t* cand_r, const int32_t* ncand, int B, int L, int C, int k,
                 int rrf_k, float* out_s, int64_t* out_r, int32_t* out_count, void* stream) {
  ragmi::clear_error();
  static_assert(ragmi::kRrfMaxL == RAG_FUSION_MAX_LISTS &&
                    ragmi::kRrfMaxE == RAG_FUSION_MAX_ENTRIES &&
                    (ragmi::kRrfMaxE & (ragmi::kRrfMaxE - 1)) == 0 &&
                    ragmi::kRrfMaxE % ragmi::kRrfBlock == 0,
                "rrf_fuse_kernel's LDS arrays and its sort");
  if (L < 1 || L > RAG_FUSION_MAX_LISTS)
    return ragmi::fail(RAG_ERANGE, "fuse_rrf: L must be in [1, RAG_FUSION_MAX_LISTS=16]");
  if (C < 1) return ragmi::fail(RAG_ERANGE, "fuse_rrf: C must be >= 1");
  if ((int64_t)L * C > RAG_FUSION_MAX_ENTRIES)
    return ragmi::fail(RAG_ERANGE, "fuse_rrf: L * C must be <= RAG_FUSION_MAX_ENTRIES=4096");
  if (k < 1) return ragmi::fail(RAG_EINVAL, "fuse_rrf: k must be >= 1");
  if (rrf_k < 1) return ragmi::fail(RAG_EINVAL, "fuse_rrf: rrf_k must be >= 1");
  if (B < 0) return ragmi::fail(RAG_EINVAL, "fuse_rrf: B must be >= 0");
  if (B > 0 && (!cand_r || !out_s || !out_r))
    return ragmi::fail(RAG_EINVAL, "fuse_rrf: a NULL candidate or output pointer");
  if (B == 0) return RAG_OK;
  ragmi::rrf_fuse_kernel<<<dim3((unsigned)B), dim3(ragmi::kRrfBlock), 0,
                           static_cast<hipStream_t>(stream)>>>(cand_r, ncand, L, C, k, rrf_k,
                                                               out_s, out_r, out_count);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// ---- formula queries: prefetched candidates re-scored by a program (formula_kernels.hip) ----

int rag_formula_rescore(const float* cand_s, const int64_t* cand_r, const uint32_t* cand_t,
                        const int64_t* const* cand_keys, const int32_t* ncand,
                        const uint32_t* prog, int64_t words, int B, int L, int C, int k,
                        float* out_s, int64_t* out_r, int32_t* out_count, uint32_t* out_status,
                        void* stream) {
  ragmi::clear_error();
  static_assert(ragmi::kFmlBlock == ragmi::kRrfBlock && ragmi::kFmlPer <= 32 &&
                    ragmi::kFmlMaxOps * ragmi::kFmlOp + ragmi::kFmlHdr +
                            ragmi::kFmlMaxConds * RAG_FILTER_REC_WORDS < (1 << 20),
                "formula_rescore_kernel's sort, its head mask and its staged records");
  if (L < 1 || L > RAG_FUSION_MAX_LISTS)
    return ragmi::fail(RAG_ERANGE, "formula_rescore: L must be in [1, RAG_FUSION_MAX_LISTS=16]");
  if (C < 1) return ragmi::fail(RAG_ERANGE, "formula_rescore: C must be >= 1");
  if ((int64_t)L * C > RAG_FUSION_MAX_ENTRIES)
    return ragmi::fail(RAG_ERANGE,
                       "formula_rescore: L * C must be <= RAG_FUSION_MAX_ENTRIES=4096");
  if (k < 1) return ragmi::fail(RAG_EINVAL, "formula_rescore: k must be >= 1");
  if (B < 0) return ragmi::fail(RAG_EINVAL, "formula_rescore: B must be >= 0");
  if (B > 0 && (!cand_s || !cand_r || !prog || !out_s || !out_r || !out_status))
    return ragmi::fail(RAG_EINVAL,
                       "formula_rescore: a NULL candidate, program or output pointer");
  if (B > 0 && words < RAG_FORMULA_HDR_WORDS)
    return ragmi::fail(RAG_EINVAL, "formula_rescore: words must be >= RAG_FORMULA_HDR_WORDS=2");
  if (B == 0) return RAG_OK;
  ragmi::FormulaKeys keys;
  for (int c = 0; c < RAG_KEYS_MAX_COLS; ++c) keys.col[c] = cand_keys ? cand_keys[c] : nullptr;
  // a blob the kernel can index with 32 bits: nothing a program names lies past its records
  const uint32_t w32 = (uint32_t)std::min<int64_t>(words, (int64_t)1 << 30);
  ragmi::formula_rescore_kernel<<<dim3((unsigned)B), dim3(ragmi::kFmlBlock), 0,
                                  static_cast<hipStream_t>(stream)>>>(
      cand_s, cand_r, cand_t, keys, ncand, prog, w32, L, C, k, out_s, out_r, out_count,
      out_status);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

int rag_merge_topk(const float* in_s, const int64_t* in_i, int n_lists, int B, int k,
                   float* out_s, int64_t* out_i, void* stream) {
  ragmi::clear_error();
  if (n_lists < 1 || B < 0 || k < 1)
    return ragmi::fail(RAG_EINVAL, "bad merge args");
  return merge_topk<false>(in_s, in_i, n_lists, B, k, out_s, out_i,
                           static_cast<hipStream_t>(stream));
}

int rag_merge_topk_packed(const int32_t* in_packed, int n_lists, int B, int k, float* out_s,
                          int64_t* out_i, void* stream) {
  ragmi::clear_error();
  if (n_lists < 1 || B < 0 || k < 1 || (B > 0 && !in_packed))
    return ragmi::fail(RAG_EINVAL, "bad merge args");
  return merge_topk<true>(reinterpret_cast<const float*>(in_packed), nullptr, n_lists, B, k,
                          out_s, out_i, static_cast<hipStream_t>(stream));
}

int rag_merge_topk_gather(const int32_t* const* lists, int n_lists, int B, int k, int64_t id_mul,
                          const int64_t* id_add, float* out_s, int64_t* out_i, uint8_t* out_empty,
                          void* stream) {
  ragmi::clear_error();
  if (!lists || !id_add || n_lists < 1 || n_lists > RAG_MAX_SHARDS || B < 0 || k < 1 ||
      (B > 0 && (!out_s || !out_i)))
    return ragmi::fail(RAG_EINVAL, "bad gather-merge args (1 <= n_lists <= RAG_MAX_SHARDS=64)");
  if (k > RAG_MAX_K_LARGE)
    return ragmi::fail(RAG_ERANGE, "gather-merge: k must be <= RAG_MAX_K_LARGE=4096");
  ragmi::GatheredLists g;
  for (int l = 0; l < ragmi::kMaxShards; ++l) {
    g.list[l] = l < n_lists ? reinterpret_cast<const int2*>(lists[l]) : nullptr;
    g.add[l] = l < n_lists ? id_add[l] : 0;
    if (l < n_lists && B > 0 && !lists[l])
      return ragmi::fail(RAG_EINVAL, "gather-merge: a list pointer is NULL");
  }
  if (B == 0) return RAG_OK;
  g.mul = id_mul;
  g.k = k;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (k > RAG_MAX_K)
    ragmi::merge_gather_large_kernel<<<dim3(B), dim3(256), 0, st>>>(g, n_lists, B, out_s, out_i,
                                                                     out_empty);
  else
    ragmi::merge_gather_kernel<<<dim3(B), dim3(64), 0, st>>>(g, n_lists, B, out_s, out_i,
                                                              out_empty);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

int rag_bench_scan(rag_index_t* h, const float* queries_dev, int B, int variant, int reps,
                   double* avg_ms) {
  ragmi::clear_error();
#ifndef RAGMI_DIAG_BUILD
  if (variant != 0 && (variant != 7 || (h && h->dim != 384)))
    return ragmi::fail(RAG_EINVAL, "variant: 0 (production) or 7 (dim 384: seeds at +inf); the "
                                   "scan's timing probes are in the diagnostic build only");
#endif
  if (!h || !queries_dev || B < 1 || reps < 1 || !avg_ms || variant < 0 || variant > 24)
    return ragmi::fail(RAG_EINVAL, "bad bench args");
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  // (not with_dim: each dim has its own probe, built for that dim alone)
  if (h->dim == 1024) {
    if (variant > 4) return ragmi::fail(RAG_EINVAL, "dim 1024: wide scan variants 0..4");
    return bench_wide<1024>(h, queries_dev, B, variant, reps, avg_ms);
  }
  return bench_scan<384>(h, queries_dev, B, variant, reps, avg_ms);
}

int rag_index_exactness_stats(rag_index_t* h, int64_t* tier1, int64_t* tier2,
                               int32_t* last_tiers, int n_last) {
  ragmi::clear_error();
  if (!h || !tier1 || !tier2 || n_last < 0 || (n_last > 0 && !last_tiers))
    return ragmi::fail(RAG_EINVAL, "bad exactness stats args");
  std::lock_guard<std::mutex> lk(h->mu);
  unsigned long long tot[3] = {};
  if (const int rc = read_fb_totals(h, tot)) return rc;
  *tier1 = (int64_t)tot[0];
  *tier2 = (int64_t)tot[1];
  if (n_last > 0) {
    const int n = h->last_ws ? std::min(n_last, h->last_bq) : 0;
    for (int i = n; i < n_last; ++i) last_tiers[i] = -1;
    if (n > 0)
      RAG_HIP(hipMemcpy(last_tiers, h->last_ws->fb_tier, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  return RAG_OK;
}

int rag_index_unanswered(rag_index_t* h, int64_t* n) {
  ragmi::clear_error();
  if (!h || !n) return ragmi::fail(RAG_EINVAL, "bad args");
  std::lock_guard<std::mutex> lk(h->mu);
  unsigned long long tot[3] = {};
  if (const int rc = read_fb_totals(h, tot)) return rc;
  *n = (int64_t)tot[2];
  return RAG_OK;
}

int rag_profile_enable(rag_index_t* h, int enable) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  h->prof = enable < 0 ? 0 : enable;
  h->prof_seq = 0;
  return RAG_OK;
}

int rag_index_set_scan_order(rag_index_t* h, int serial) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  h->serial_scans = serial < 0 || serial > 2 ? 1 : serial;
  h->scan_last = nullptr;
  h->scan_any = false;
  return RAG_OK;
}

int rag_index_set_prescan(rag_index_t* h, int mode) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (mode < RAG_PRESCAN_OFF || mode > RAG_PRESCAN_ALWAYS6)
    return ragmi::fail(RAG_EINVAL,
                       "prescan mode must be 0 (off), 1 (auto), 2 (always) or 3 (always 6-bit)");
  std::lock_guard<std::mutex> lk(h->mu);
  if (mode == RAG_PRESCAN_ALWAYS6) {   // an index below the threshold builds its 6-bit copy now
    const int rc = ragmi::ensure_copy6(h);
    if (rc) return rc;
  }
  h->prescan = mode;
  return RAG_OK;
}

int rag_index_prescan(const rag_index_t* h) { return h ? h->prescan : -1; }

int rag_index_prescan_passes(rag_index_t* h, int64_t* n) {
  ragmi::clear_error();
  if (!h || !n) return ragmi::fail(RAG_EINVAL, "bad args");
  std::lock_guard<std::mutex> lk(h->mu);
  *n = h->copy_passes[ragmi::kCopy8] + h->copy_passes[ragmi::kCopy6];
  return RAG_OK;
}

int rag_index_prescan6_passes(rag_index_t* h, int64_t* n) {
  ragmi::clear_error();
  if (!h || !n) return ragmi::fail(RAG_EINVAL, "bad args");
  std::lock_guard<std::mutex> lk(h->mu);
  *n = h->copy_passes[ragmi::kCopy6];
  return RAG_OK;
}

int rag_index_prescan_bounds(rag_index_t* h, const float* q, int B, const int64_t* rows_dev,
                             int64_t n, float* out_u) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (B < 1 || B > ragmi::kQ || !q || n < 0 || (n > 0 && (!rows_dev || !out_u)))
    return ragmi::fail(RAG_EINVAL, "bad prescan_bounds args (1 <= B <= 32)");
  if (n > 0x7fffffff) return ragmi::fail(RAG_ERANGE, "n too large for one call");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->copy[ragmi::kCopy8].data)
    return ragmi::fail(RAG_EINVAL, "index keeps no int8 scan copy (dim 384, fp16 storage only)");
  if (n == 0) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  RAG_HIP(hipDeviceSynchronize());   // workspace 0 may belong to a running pass
  Workspace& w = h->ws[0];
  qprep8_kernel<384><<<dim3(kQ), dim3(64), 0, nullptr>>>(q, B, nullptr, w.qn, w.qfrag, w.filt,
                                                         w.eps, w.qfrag8, w.qp8, w.eps8);
  // the bound of the copy a k = 1 pass streams in the current mode (the int8 one where none)
  const ragmi::CopyKind kind = use_prescan6(h, 1) ? ragmi::kCopy6 : ragmi::kCopy8;
  ragmi::with_copy(kind, [&](auto c) {
    prescan_bounds_kernel<384, typename decltype(c)::type>
        <<<dim3((unsigned)n), dim3(64), 0, nullptr>>>(
            h->copy[kind].data, h->copy[kind].meta, reinterpret_cast<const intx4*>(w.qfrag8),
            w.qp8, rows_dev, n, h->count, B, out_u);
  });
  RAG_HIP(hipGetLastError());
  RAG_HIP(hipDeviceSynchronize());
  return RAG_OK;
}

int rag_stream_create_cu_partition(int device, int part, int parts, void** out) {
  ragmi::clear_error();
  if (!out || parts < 1 || part < 0 || part >= parts)
    return ragmi::fail(RAG_EINVAL, "need 0 <= part < parts and an output pointer");
  *out = nullptr;
  int n_cu = 0;
  RAG_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
  // a part of >= 8 consecutive CU ids holds a CU of every XCD (bit i is on XCD i % 8); a
  // smaller one would leave XCDs without a bit, and those run on ALL their CUs
  if (parts > n_cu / 8) return ragmi::fail(RAG_EINVAL, "at most n_cu / 8 parts (8 CUs each)");
  // contiguous CU ids [part n / parts, (part + 1) n / parts)
  std::vector<uint32_t> mask((size_t)(n_cu + 31) / 32, 0u);
  const int c0 = (int)((int64_t)part * n_cu / parts), c1 = (int)((int64_t)(part + 1) * n_cu / parts);
  for (int c = c0; c < c1; ++c) mask[(size_t)c / 32] |= 1u << (c % 32);
  return create_masked_stream(device, mask.data(), (uint32_t)mask.size(), out);
}

int rag_stream_create_cu_mask(int device, const uint32_t* mask, int words, void** out) {
  ragmi::clear_error();
  if (!out || !mask || words < 1 || words > 32)
    return ragmi::fail(RAG_EINVAL, "need a mask of 1..32 words and an output pointer");
  *out = nullptr;
  int n = 0;
  for (int i = 0; i < words; ++i) n += __builtin_popcount(mask[i]);
  if (n == 0) return ragmi::fail(RAG_EINVAL, "empty CU mask");
  // bit i is a CU of XCD i % 8, and an XCD left with no bit runs on ALL its CUs (measured,
  // profiles/r06_cu_mask/r06s_cu_mask_probe.jsonl): such a mask would not restrict anything
  // there, so it is refused
  uint32_t xcds = 0;
  for (int i = 0; i < words * 32; ++i)
    if (mask[i / 32] >> (i % 32) & 1u) xcds |= 1u << (i % 8);
  if (xcds != 0xffu)
    return ragmi::fail(RAG_EINVAL, "CU mask must enable at least one CU of every XCD (bit i "
                                   "is on XCD i % 8)");
  return create_masked_stream(device, mask, (uint32_t)words, out);
}

#ifdef RAGMI_DIAG_BUILD
// where a stream's workgroups run (diagnostic): per workgroup (XCC_ID, HW_ID) hardware
// registers, for mapping CU-mask bits to XCDs / shader engines / CUs
__global__ void cu_probe_kernel(int32_t* out) {
  uint32_t x, hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  // hold the CU a little so later workgroups spread over the allowed CUs
  const long long t0 = clock64();
  while (clock64() - t0 < 20000) {
  }
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = (int32_t)x;
    out[2 * blockIdx.x + 1] = (int32_t)hw;
  }
}
#endif

int rag_diag_cu_probe(void* stream, int n_wg, int32_t* out_dev) {
  ragmi::clear_error();
#ifdef RAGMI_DIAG_BUILD
  if (n_wg < 1 || !out_dev) return ragmi::fail(RAG_EINVAL, "n_wg >= 1 and an output buffer");
  cu_probe_kernel<<<dim3(n_wg), dim3(64), 0, static_cast<hipStream_t>(stream)>>>(out_dev);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
#else
  (void)stream; (void)n_wg; (void)out_dev;
  return ragmi::fail(RAG_EINVAL, "rag_diag_cu_probe: diagnostic build only");
#endif
}

int rag_stream_destroy(void* stream) {
  ragmi::clear_error();
  if (!stream) return RAG_OK;
  g_stream_gen.fetch_add(1, std::memory_order_acq_rel);
  RAG_HIP(hipStreamDestroy(static_cast<hipStream_t>(stream)));
  return RAG_OK;
}

int rag_profile_scan_ms(rag_index_t* h, double* total_ms, int64_t* launches) {
  ragmi::clear_error();
  if (!h || !total_ms || !launches) return ragmi::fail(RAG_EINVAL, "bad args");
  std::lock_guard<std::mutex> lk(h->mu);
  double tot = 0.0;
  for (auto& p : h->prof_pairs) {
    RAG_HIP(hipEventSynchronize(p.b));
    float ms = 0.f;
    RAG_HIP(hipEventElapsedTime(&ms, p.a, p.b));
    tot += ms;
  }
  *launches = (int64_t)h->prof_pairs.size();
  *total_ms = tot;
  drop_prof_pairs(h);
  return RAG_OK;
}

int rag_profile_scan_intervals(rag_index_t* h, double* start_ms, double* end_ms, int64_t cap,
                               int64_t* launches) {
  ragmi::clear_error();
  if (!h || !launches || cap < 0 || (cap > 0 && (!start_ms || !end_ms)))
    return ragmi::fail(RAG_EINVAL, "bad args");
  std::lock_guard<std::mutex> lk(h->mu);
  const int64_t n = (int64_t)h->prof_pairs.size();
  for (int64_t i = 0; i < n; ++i) RAG_HIP(hipEventSynchronize(h->prof_pairs[(size_t)i].b));
  // every interval relative to the first recorded launch's start event (events of different
  // streams on one device share the device clock; an earlier launch reads negative)
  for (int64_t i = 0; i < n && i < cap; ++i) {
    const ProfPair& p = h->prof_pairs[(size_t)i];
    float a = 0.f, b = 0.f;
    RAG_HIP(hipEventElapsedTime(&a, h->prof_pairs[0].a, p.a));
    RAG_HIP(hipEventElapsedTime(&b, h->prof_pairs[0].a, p.b));
    start_ms[i] = a;
    end_ms[i] = b;
  }
  drop_prof_pairs(h);
  *launches = n;
  return RAG_OK;
}

}  // extern "C"
