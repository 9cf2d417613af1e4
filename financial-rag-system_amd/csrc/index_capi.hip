// index_capi.hip — extern "C" boundary of the flat index (declared in include/ragmi.h).
//
// Host side of the Qdrant replacement: handle lifetime, capacity growth, workspace ring,
// kernel launch sequence of one search (qprep -> scan -> select). No compute runs
// on the host; every entry point either enqueues on the caller's stream or (for *_host)
// stages through device memory and synchronises.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ragmi.h"
#include "common_host.hpp"
// the device layer, one header per pass, in dependency order
#include "prep_kernels.hip"
#include "scan_kernels.hip"
#include "seed_kernels.hip"
#include "certify_kernels.hip"
#include "merge_kernels.hip"
#include "largek_kernels.hip"
#include "reselect_kernels.hip"
#include "rows_kernels.hip"
#include "filter_kernels.hip"

#include <hipcub/hipcub.hpp>

using ragmi::half8;
using ragmi::DeviceBuf;
using ragmi::WsBuf;
using ragmi::ws_buf;

namespace {

// Per-pass workspace slots. A slot is bound to the stream of its last pass: passes on the
// same stream are ordered by the stream itself, so the hot path records no events at all (an
// event record idles the queue for ~5 us between kernels). Up to kRing streams search
// concurrently without interference; a further stream drains the device once and rebinds
// the least recently used slot. (Round 4: 8 slots. With 4, a fifth stream in flight rebinds on
// every pass: 1.25M rows, 5-8 streams 137-141K qps; with 8, 5 / 6 / 8 streams 186-205K, and
// 4 streams stay the fastest at 209-210K, profiles/r04t_streams_hwqueues.jsonl.)
constexpr int kRing = 8;
constexpr int kMaxGroups = 4;   // query groups of 32 per pass (wide rows)

struct Workspace {
  float* qn = nullptr;
  half8* qfrag = nullptr;
  uint32_t* filt = nullptr;
  float* smax = nullptr;      // [kMaxLists][32] per-sample-wave maxima
  float* seed = nullptr;      // [32] seed thresholds
  float* part_s = nullptr;
  int* part_i = nullptr;
  float* heads_s = nullptr;   // [32][n_lists]
  int* heads_i = nullptr;
  int* heads_n = nullptr;
  int* progress = nullptr;      // [lists][groups] shared-group scan throttle words
  float* eps = nullptr;         // [groups][32] per-query |MFMA - exact| score bound (qprep)
  int* fb_tier = nullptr;       // [groups][32] certifying path per query of the last pass
  unsigned long long* fb_cnt = nullptr;   // [3] tier-1 / tier-2 / unanswered totals since creation
  int* tileq = nullptr;         // [8][kTileQStride] per-XCD tile-queue heads (dynamic scan)
  // tier-2 hand-off select -> rescan_kernel: (L, e_k) per query, the rescan workgroups' lists
  // [query][kRescanMaxWG][32] and the launch's arrival ticket (zero between passes)
  float* t2 = nullptr;
  float* t2_s = nullptr;
  int* t2_i = nullptr;
  int* t2_tk = nullptr;
  // int8 prescan (indexes that keep the int8 copy): the queries' int8 planes, their u_bound
  // parameters [32][4] and the certificate's eps for a pass ranked by u (qprep8_kernel)
  char* qfrag8 = nullptr;
  float* qp8 = nullptr;
  float* eps8 = nullptr;
  // large-k path (k > RAG_MAX_K; lk_* kernels), allocated on first use: sample maxima
  // [32][kLkSampleMax], per query thr / count / round flag, round flags, candidates
  // [32][kLkCap]
  float* lk_smax = nullptr;
  float* lk_thr = nullptr;
  int* lk_cnt = nullptr;
  int* lk_again = nullptr;
  int* lk_need = nullptr;
  int* lk_cand = nullptr;
  float* lk_es = nullptr;       // [32][kLkCap] exact scores of the candidates (lk_rescore)
  hipEvent_t ev_in = nullptr;   // scan-stream order: caller stream -> scan stream -> caller
  hipEvent_t ev_out = nullptr;
  hipStream_t owner = nullptr;  // stream of the last pass that used this slot
  int cus = 0;                  // CUs the owner stream may use (its CU mask; stream_cus)
  uint64_t cus_gen = 0;         // g_stream_gen when `cus` was read
  bool used = false;
  uint64_t tick = 0;            // last use (LRU rebinding)
};

struct ProfPair {
  hipEvent_t a, b;
};

// A filter view column (rag_index_search_view), bound to the stream of its last call as a
// Workspace is: calls on one stream are ordered by the stream, so the next view kernel
// overwrites the column only after the previous call's passes have read it (acquire_view)
struct ViewSlot {
  uint32_t* p = nullptr;
  size_t bytes = 0;
  hipStream_t owner = nullptr;
  bool used = false;
  uint64_t tick = 0;
};

// One search pass's share of a search call: at most one pass's queries, their filters and the
// output rows they fill (out_packed, or out_s and out_i); `tags` is the tag column every kernel
// of the pass filters on: the stored tags, or a filter view of them (rag_index_search_view)
struct PassArgs {
  const float* q;
  int Bq, k;
  const uint32_t* filt;
  const uint32_t* tags;
  int64_t id_offset;
  float* out_s;
  int64_t* out_i;
  int32_t* out_packed;
};

// Runtime value -> compile-time constant, handed to a generic lambda that reads it as
// decltype(tag)::value (the idiom of bert_capi.hip): `filt != nullptr` as a bool_constant ...
template <typename F>
auto with_filter(const uint32_t* filt, F&& f) {
  if (filt) return f(std::bool_constant<true>{});
  return f(std::bool_constant<false>{});
}

// ... and the handle's dim as an integral_constant; the lambda returns the status
template <typename F>
int with_dim(int dim, F&& f) {
  if (dim == 384) return f(std::integral_constant<int, 384>{});
  if (dim == 1024) return f(std::integral_constant<int, 1024>{});
  return ragmi::fail(RAG_EINVAL, "unsupported dim (built: 384, 1024)");
}

// The slot (Workspace, SetSlot) a call on stream `st` takes: the one bound to `st`, else the
// first unused one. Neither: nullptr, every slot being bound to another stream whose last call
// may still be running; `lru` is the least recently used one, for the caller to wait for and
// rebind.
template <typename Slot, size_t N>
Slot* pick_slot(Slot (&slots)[N], hipStream_t st, Slot*& lru) {
  lru = &slots[0];
  for (auto& s : slots)
    if (s.tick < lru->tick) lru = &s;
  for (auto& s : slots)
    if (s.used && s.owner == st) return &s;
  for (auto& s : slots)
    if (!s.used) return &s;
  return nullptr;
}

// Transient resources of one call, released on every return path.
// Stream-ordered scratch: freed on the stream it was allocated on
struct StreamScratch {
  hipStream_t st;
  char* p = nullptr;
  explicit StreamScratch(hipStream_t s) : st(s) {}
  StreamScratch(const StreamScratch&) = delete;
  ~StreamScratch() {
    if (p) (void)hipFreeAsync(p, st);
  }
  hipError_t alloc(size_t bytes) { return hipMallocAsync(reinterpret_cast<void**>(&p), bytes, st); }
};

// a pair of timing events
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  hipError_t create() {
    const hipError_t e = hipEventCreate(&a);
    return e != hipSuccess ? e : hipEventCreate(&b);
  }
};

// *ms = device time of `reps` back-to-back calls of `one` (launches on the null stream), after
// one warm-up call
template <typename F>
int time_launches(int reps, F&& one, float* ms) {
  EventPair ev;
  RAG_HIP(ev.create());
  one();  // warm
  RAG_HIP(hipEventRecord(ev.a, nullptr));
  for (int r = 0; r < reps; ++r) one();
  RAG_HIP(hipEventRecord(ev.b, nullptr));
  RAG_HIP(hipEventSynchronize(ev.b));
  RAG_HIP(hipEventElapsedTime(ms, ev.a, ev.b));
  return RAG_OK;
}

// The large-k buffers, allocated together on first use (ensure_lk)
std::array<WsBuf, 7> lk_buffers(Workspace& w) {
  using namespace ragmi;
  const size_t Q = kQ;
  return {ws_buf(w.lk_smax, Q * kLkSampleMax * 4), ws_buf(w.lk_thr, Q * 4),
          ws_buf(w.lk_cnt, Q * 4),                 ws_buf(w.lk_again, Q * 4),
          ws_buf(w.lk_need, 64),                   ws_buf(w.lk_cand, Q * kLkCap * 4),
          ws_buf(w.lk_es, Q * kLkCap * 4)};
}

}  // namespace

struct rag_index {
  int dim = 0;
  bool diagnostic = false;   // counted in ragmi::diagnostic_handles() (common_host.hpp)
  int device = 0;
  int64_t cap_rows = 0;   // multiple of 16
  int64_t count = 0;
  half8* corpus = nullptr;
  uint32_t* tags = nullptr;
  // key columns (rag_index_keys_create; rows_kernels.hip): n_keys int64 columns of cap_rows
  // keys, the tag array's extent; entries at or past n_keys are nullptr
  int64_t* keys[RAG_KEYS_MAX_COLS] = {};
  int n_keys = 0;
  // storage (rag_index_create_ex): RAG_STORE_FP16 keeps only the scan's fp16 tile16 rows;
  // RAG_STORE_FP32 also the normalised fp32 rows (row-major [cap][dim]), which the exact
  // rescoring reads — Qdrant's default Float32 datatype
  int storage = RAG_STORE_FP16;
  float* rows32 = nullptr;
  // int8 scan copy (dim 384, fp16 storage; prep_kernels.hip): the tile16x64 image and the
  // per-row (scale, error) meta, both over cap_rows / 16 + 1 tiles (the prescan walks tile
  // pairs); rebuilt from the stored fp16 rows after every write of `corpus` (requant)
  char* c8 = nullptr;
  float* meta8 = nullptr;
  int prescan = 1;        // rag_index_set_prescan: 0 off, 1 auto, 2 always
  int n_cu = 256;
  int max_wgs = 0;        // scan workgroups at full occupancy
  int scan_wgs = 0;       // D <= 384 scan grid cap: 3/4 of the CUs (launch_search_pass)
  int groups = 1;         // query groups of 32 per search pass
  std::mutex mu;
  Workspace ws[kRing];
  uint64_t ws_tick = 0;
  ViewSlot views[kRing];          // filter view columns, allocated on first use per stream
  uint64_t view_tick = 0;
  Workspace* last_ws = nullptr;   // workspace of the most recent search pass
  int last_bq = 0;                // its query count
  // host staging for *_host entry points
  void* stage = nullptr;
  size_t stage_bytes = 0;
  // profiling
  // scan order (rag_index_set_scan_order): when set, every scan launch waits for the
  // previous one (on whichever stream it ran), so passes on several streams overlap their
  // query prep / seeding / select with another pass's scan but never two scans
  // 0 free, 1 serial (event chain across the callers' streams), 2 serial on the handle's own
  // scan stream (each pass hands its scan to it and waits for it before select)
  int serial_scans = 0;
  hipStream_t scan_stream = nullptr;
  hipEvent_t scan_done = nullptr;
  hipStream_t scan_last = nullptr;
  bool scan_any = false;       // a scan has been chained since set_scan_order (scan_last may be
                               // the null stream, whose handle is nullptr)
  int prof = 0;                // 0 off; n > 0: time every n-th scan launch
  int64_t prof_seq = 0;
  std::vector<ProfPair> prof_pairs;
};

namespace {

int64_t round16(int64_t n) { return (n + 15) & ~int64_t(15); }

// The buffers every Workspace of `h` holds from creation to destruction (h->dim, groups and
// max_wgs set), in allocation order: rag_index_create_ex gives each its own hipMalloc in this
// order, rag_index_destroy frees them.
std::array<WsBuf, 22> ws_buffers(const rag_index* h, Workspace& w) {
  using namespace ragmi;
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
          ws_buf(w.qfrag8, h->c8 ? 4 * (dim / 64) * 64 * 16 : 0),
          ws_buf(w.qp8, h->c8 ? Q * 4 * 4 : 0),
          ws_buf(w.eps8, h->c8 ? Q * 4 : 0)};
}

// Which indexes keep the int8 scan copy
bool keeps_copy8(const rag_index* h) { return h->dim == 384 && h->storage == RAG_STORE_FP16; }

size_t copy8_bytes(const rag_index* h, int64_t cap_rows) {
  return (size_t)(cap_rows / 16 + 1) * (h->dim / 64) * 1024;
}
size_t meta8_bytes(int64_t cap_rows) { return (size_t)(cap_rows / 16 + 1) * 32 * 4; }

// the copy's two buffers for `cap_rows` rows, zeroed (freed by the caller's DeviceBufs on error)
int alloc_copy8(const rag_index* h, int64_t cap_rows, DeviceBuf<char>& c8, DeviceBuf<float>& m8) {
  if (c8.alloc(copy8_bytes(h, cap_rows)) != hipSuccess ||
      m8.alloc(meta8_bytes(cap_rows)) != hipSuccess)
    return ragmi::fail(RAG_ENOMEM, "hipMalloc(int8 scan copy) failed");
  RAG_HIP(hipMemset(c8.p, 0, copy8_bytes(h, cap_rows)));
  RAG_HIP(hipMemset(m8.p, 0, meta8_bytes(cap_rows)));
  return RAG_OK;
}

// The int8 copy of rows[i] (device list) or row0 + i, i < n, rebuilt from the stored fp16 rows:
// enqueued on `st` right after the kernel that wrote them
int requant(rag_index* h, const int64_t* rows, int64_t row0, int64_t n, hipStream_t st) {
  if (!h->c8 || n <= 0) return RAG_OK;
  ragmi::requant_kernel<384><<<dim3((unsigned)n), dim3(64), 0, st>>>(
      h->corpus, rows, row0, n, h->cap_rows, h->c8, h->meta8);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

int alloc_corpus(rag_index* h, int64_t cap_rows, half8** corpus, uint32_t** tags) {
  const size_t cbytes = (size_t)cap_rows * h->dim * 2;
  RAG_HIP(hipMalloc(reinterpret_cast<void**>(corpus), std::max<size_t>(cbytes, 16)));
  if (hipMalloc(reinterpret_cast<void**>(tags), std::max<size_t>(cap_rows * 4, 16)) !=
      hipSuccess) {
    (void)hipFree(*corpus);
    *corpus = nullptr;
    return ragmi::fail(RAG_ENOMEM, "hipMalloc(tags) failed");
  }
  RAG_HIP(hipMemset(*corpus, 0, std::max<size_t>(cbytes, 16)));
  RAG_HIP(hipMemset(*tags, 0, std::max<size_t>(cap_rows * 4, 16)));
  return RAG_OK;
}

int ensure_stage(rag_index* h, size_t bytes) {
  if (h->stage_bytes >= bytes) return RAG_OK;
  if (h->stage) (void)hipFree(h->stage);
  h->stage = nullptr;
  h->stage_bytes = 0;
  RAG_HIP(hipMalloc(&h->stage, bytes));
  h->stage_bytes = bytes;
  return RAG_OK;
}

// qprep's extra error-bound term for fp32 storage (prep_kernels.hip qprep_kernel): the exact
// score reads the fp32 row c32, the scan its fp16 rounding c: |sum (c - c32) qn| <=
// ||c - c32|| ||qn|| <= (2^-11 ||c32|| + 2^-25 sqrt(D)) (1 + 2^-20), ||c32|| <= 1 + 2^-20
double store_eps(const rag_index* h) {
  if (h->storage != RAG_STORE_FP32) return 0.0;
  return (0x1p-11 * (1.0 + 0x1p-20) + 0x1p-25 * std::sqrt((double)h->dim)) * (1.0 + 0x1p-20);
}

// Bumped by every rag_stream_create_cu_partition / rag_stream_destroy: a workspace's cached CU
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

// sample + thresh: seed thresholds for the scan (see sample_kernel). ~0.8% of the shard's
// tiles, spread evenly, at least 256 tiles (all of them for small shards).
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
  const int cap = k.get(ragmi::kRescanMaxWG);
  if (cap <= 0) return 0;
  const int64_t n_tiles = (h->count + 15) / 16;
  return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)cap, (int64_t)ragmi::kRescanMaxWG,
                                                      (int64_t)h->n_cu, n_tiles / 128}));
}

// RAGMI_SAMPLE_DIV (diagnostic A/B): 1 / the sampled fraction of the shard's tiles
int sample_div() {
  static ragmi::Knob k("RAGMI_SAMPLE_DIV");
  return std::max(1, k.get(128));
}

template <int D, bool FILTER>
void launch_seed(rag_index* h, Workspace& w, int groups, hipStream_t st,
                 const float* q = nullptr, int Bq = 0, const uint32_t* filt_in = nullptr,
                 const uint32_t* tags = nullptr) {
  using namespace ragmi;
  if (!tags) tags = h->tags;
  const int n_tiles = (int)((h->count + 15) / 16);
  if (q) {     // fused: qprep inside the sample launch (also when there is nothing to sample)
    if constexpr (D <= 384) {
      const int div_f = sample_div();
      const int n_sample = n_tiles == 0 ? 0 : std::min({n_tiles, std::max(256, n_tiles / div_f),
                                                        kMaxSample});
      qprep_sample_kernel<D, FILTER><<<dim3(std::max(1, (n_sample + 7) / 8)), dim3(256), 0, st>>>(
          q, Bq, filt_in, w.qn, w.qfrag, w.filt, w.eps, store_eps(h), h->corpus, tags,
          (int)h->count, n_tiles, n_sample, w.smax);
      if (n_sample > 0)
        thresh_kernel<kMaxSample><<<dim3(kQ, 1), dim3(256), 0, st>>>(w.smax, n_sample, w.eps,
                                                                    w.seed);
    }
    return;
  }
  if (n_tiles == 0) return;   // the scan visits no tile; seeds are never read
  const int div = sample_div();
  // D = 1024 tiles are 32 KB and config 5 shards hold up to 3.1M of them: a 4096-tile cap
  // would sample 0.13% of a 50M-row shard and let ~25K rows per query past the seed
  constexpr int kCap = D > 384 ? kMaxSampleWide : kMaxSample;
  const int n_sample = std::min({n_tiles, std::max(256, n_tiles / div), kCap});
  if constexpr (D > 384)   // every query group in one pass over each sample tile
    sample_wide_kernel<D, FILTER><<<dim3((n_sample + 7) / 8), dim3(256), 0, st>>>(
        h->corpus, tags, w.filt, w.qfrag, (int)h->count, n_tiles, n_sample, w.smax, groups);
  else
    sample_kernel<D, FILTER><<<dim3((n_sample + 7) / 8, groups), dim3(256), 0, st>>>(
        h->corpus, tags, w.filt, w.qfrag, (int)h->count, n_tiles, n_sample, w.smax);
  thresh_kernel<kCap><<<dim3(kQ, groups), dim3(256), 0, st>>>(w.smax, n_sample, w.eps, w.seed);
}

// Does a k <= RAG_MAX_K pass of `h` scan the int8 copy (rag_index_set_prescan)? Only an index
// that keeps the copy (dim 384, fp16 storage). Auto: passes over at least RAG_PRESCAN_MIN_ROWS
// rows, filtered or not (10M rows: unfiltered 1.82x, per-query ticker filter 1.82x; 500K rows
// 1.03x; DESIGN.md "int8 prescan"); below that a step is launch-bound and the wider
// certificate band (tier 1 for a sixth to a third of the queries) buys nothing.
bool use_prescan(const rag_index* h, int k) {
  return h->c8 && RAG_PRESCAN_ROUTES(h->prescan, h->dim, h->storage, k, h->count);
}

// Query prep and seeds of an int8 prescan pass: qprep's outputs plus the int8 planes
// (qprep8_kernel), then launch_seed's sample of the shard scored with the prescan's own upper
// bound u (sample_kernel_i8) and thresh_kernel on it
template <int D>
void launch_prep8(rag_index* h, Workspace& w, const float* q, int Bq, const uint32_t* filt,
                  const uint32_t* tags, hipStream_t st) {
  using namespace ragmi;
  qprep8_kernel<D><<<dim3(kQ), dim3(64), 0, st>>>(q, Bq, filt, w.qn, w.qfrag, w.filt, w.eps,
                                                  w.qfrag8, w.qp8, w.eps8);
  const int nt = (int)((h->count + 15) / 16);
  if (nt == 0) return;   // the scan visits no tile; seeds are never read
  const int n_sample = std::min({nt, std::max(256, nt / sample_div()), kMaxSample});
  with_filter(filt, [&](auto f) {
    sample_kernel_i8<D, decltype(f)::value><<<dim3((n_sample + 7) / 8), dim3(256), 0, st>>>(
        h->c8, h->meta8, tags, w.filt, reinterpret_cast<const intx4*>(w.qfrag8), w.qp8,
        (int)h->count, nt, n_sample, w.smax);
  });
  thresh_kernel<kMaxSample><<<dim3(kQ, 1), dim3(256), 0, st>>>(w.smax, n_sample, w.eps8, w.seed);
}

template <int D>
int launch_search_pass(rag_index* h, Workspace& w, const PassArgs& a, hipStream_t st) {
  using namespace ragmi;
  const uint32_t* const filt = a.filt;
  const int Bq = a.Bq;
  // Bq <= 32 * h->groups queries: `groups` query groups of 32 (one for D <= 384)
  const int groups = (Bq + kQ - 1) / kQ;
  bool i8 = false;
  if constexpr (D == 384) i8 = use_prescan(h, a.k);
  // fused qprep + sample only in free scan order (small shards, several scans overlapping):
  // there it is +1.1% (1.25M rows, 4 in flight, profiles/r03d_fused_prep_ab.jsonl); with the
  // scans chained (>= 4M rows) its 256-thread workgroups of ~180 registers, which cannot share a
  // CU with scan workgroups, landed between a scan's workgroups and stretched the scan launch
  // (10M rows: scan 0.76 vs 0.83 of the roofline, same qps, profiles/r03i_headline_prep_ab.jsonl)
  if (i8) {
    // the seed is then a lower bound of the 32nd-best u, which the prescan's thresholds compare
    if constexpr (D == 384) launch_prep8<D>(h, w, a.q, Bq, filt, a.tags, st);
  } else if (D <= 384 && groups == 1 && fused_prep() && h->serial_scans == 0) {
    with_filter(filt, [&](auto f) {
      launch_seed<D, decltype(f)::value>(h, w, groups, st, a.q, Bq, filt, a.tags);
    });
  } else {
    qprep_kernel<D><<<dim3(groups * kQ), dim3(64), 0, st>>>(a.q, Bq, filt, w.qn, w.qfrag, w.filt,
                                                            w.eps, store_eps(h));
    with_filter(filt, [&](auto f) {
      launch_seed<D, decltype(f)::value>(h, w, groups, st, nullptr, 0, nullptr, a.tags);
    });
  }
  const int64_t n_tiles = (h->count + 15) / 16;
  // D <= 384: queries in VGPRs, 2 workgroups per CU; wider rows: queries in LDS, 1 per CU,
  // R workgroups per query group (R % 8 == 0: XCD pairing of the groups, scan_lds_kernel)
  constexpr bool kLdsQ = D > 384;
  int grid;
  // a CU-partitioned stream (w.cus < n_cu): the same per-CU occupancy over its CUs only
  const bool part = w.cus > 0 && w.cus < h->n_cu;
  const int max_wgs = part ? 2 * w.cus : h->max_wgs;
  if constexpr (kLdsQ) {
    const int per_group = std::max(8, (max_wgs / 2 / groups) & ~7);
    const int need = (int)std::min<int64_t>(
        per_group, ((n_tiles + kLdsWaves - 1) / kLdsWaves + 7) & ~int64_t(7));
    grid = std::max(8, std::min(need, kMaxLists / kLdsWaves));
  } else {
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
    static ragmi::Knob k_wgs("RAGMI_SCAN_WGS");
    const int wg_env = k_wgs.get(0) > 0 ? std::max(8, k_wgs.get(0)) : 0;
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
    const int wg_cap = wg_env ? wg_env : (filt && !i8) ? max_wgs : part ? w.cus : h->scan_wgs;
    grid = (int)std::min<int64_t>(std::min(max_wgs, wg_cap),
                                  std::max<int64_t>(1, (n_tiles + 3) / 4));
    grid = std::min(grid, kMaxLists / kWavesPerWG);
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
    // the 384-d scan times its own dispatch (launch_fixed_timed below)
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
        if (i8) {
          // timed exactly as the fp16 launch is (its own dispatch packet)
          const auto go = [&](auto... args) -> int {
            if (timed)
              RAG_HIP(launch_fixed_timed<kScanBlock>(scan_kernel_i8<D, F>, dim3(grid), 0, st, pp.a,
                                                     pp.b, args...));
            else
              launch_fixed<kScanBlock>(scan_kernel_i8<D, F>, dim3(grid), 0, st, args...);
            return RAG_OK;
          };
          return go(static_cast<const char*>(h->c8), static_cast<const float*>(h->meta8), a.tags,
                    static_cast<const uint32_t*>(w.filt),
                    reinterpret_cast<const intx4*>(w.qfrag8), static_cast<const float*>(w.qp8),
                    (int)h->count, (int)n_tiles, static_cast<const float*>(w.seed), w.part_s,
                    w.part_i, w.heads_s, w.heads_i, w.heads_n);
        }
      }
      return with_scan_args(
          [&](auto... args) -> int {
            // the timed launch carries its own start / end timestamps (launch_fixed_timed)
            if (timed)
              RAG_HIP(launch_fixed_timed<kScanBlock>(scan_kernel<D, F>, dim3(grid), 0, st, pp.a,
                                                     pp.b, args...));
            else
              launch_fixed<kScanBlock>(scan_kernel<D, F>, dim3(grid), 0, st, args...);
            return RAG_OK;
          },
          nullptr);
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
  with_filter(filt, [&](auto f) {
    select_kernel<D, decltype(f)::value><<<dim3(Bq), dim3(256), 0, st>>>(
        w.part_s, w.part_i, w.heads_s, w.heads_i, w.heads_n, n_lists, h->corpus, a.tags, w.filt,
        w.qfrag, (int)h->count, w.qn, a.k, i8 ? w.eps8 : w.eps, w.seed, fb, a.id_offset, a.out_s,
        a.out_i, a.out_packed, h->rows32, i8 ? w.eps : nullptr);
  });
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

// One search pass of <= 32 queries for RAG_MAX_K < k <= RAG_MAX_K_LARGE (largek_kernels.hip,
// "Exact top-k for RAG_MAX_K < k"): qprep, a sample of the shard's tiles for the bound, then
// kLkRounds (collect, final) launch pairs; rounds after the first return at once unless a
// query's candidate list overflowed in the previous one.
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
  using namespace ragmi;
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
        hipcub::DeviceRadixSort::SortPairsDescending(tmp, tmp_bytes,
                                                     static_cast<const uint32_t*>(k_in), k_out,
                                                     static_cast<const int*>(v_in), v_out, n, 0,
                                                     32, st) != hipSuccess) {
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

// k > RAG_MAX_K_LARGE: per query, three stable radix sorts over the n_lists * k entries
// (merge_kernels.hip merge_any_*; the full pass's SortPairsDescending<uint32, int>, no other
// hipcub instantiation); stream-ordered scratch released at the end
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
    size_t t = tmp;
    return hipcub::DeviceRadixSort::SortPairsDescending(scratch, t,
                                                        static_cast<const uint32_t*>(ka), kb,
                                                        static_cast<const int*>(pa), pb, n, 0, 32,
                                                        st) == hipSuccess;
  };
  int rc = RAG_OK;
  for (int b = 0; b < B && rc == RAG_OK; ++b) {
    bool ok = true;
    for (int word = 0; word < 2 && ok; ++word) {   // id ascending: low word, then high word
      ragmi::merge_any_ids_kernel<PACKED><<<g, dim3(256), 0, st>>>(
          in_s, in_i, n_lists, B, k, b, word ? pb : nullptr, word, ka, pa);
      ok = hipGetLastError() == hipSuccess && sort();
    }
    if (ok) {
      ragmi::merge_any_scores_kernel<PACKED><<<g, dim3(256), 0, st>>>(in_s, in_i, n_lists, B, k,
                                                                      b, pb, ka, pa);
      ok = hipGetLastError() == hipSuccess && sort();
    }
    if (ok) {
      ragmi::merge_any_emit_kernel<PACKED><<<ge, dim3(256), 0, st>>>(in_s, in_i, B, k, b, kb, pb,
                                                                     out_s, out_i);
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
    ragmi::merge_large_kernel<PACKED><<<dim3(B), dim3(256), 0, st>>>(in_s, in_i, n_lists, B, k,
                                                                    out_s, out_i);
  else
    ragmi::merge_exact_kernel<PACKED><<<dim3(B), dim3(64), 0, st>>>(in_s, in_i, n_lists, B, k,
                                                                   out_s, out_i);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

template <int D>
int launch_large_k_pass(rag_index* h, Workspace& w, const PassArgs& a, hipStream_t st) {
  using namespace ragmi;
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

// rag_index_import_rows (T = uint16_t: fp16 rows into an fp16-storage index) and
// rag_index_import_rows32 (T = float: fp32 rows into an fp32-storage index, the scan's fp16
// copy derived on the device): staged through device memory, synchronous
template <typename T>
int import_rows(rag_index* h, int64_t row0, int64_t n, const T* rows, const uint32_t* tags,
                int64_t new_count) {
  constexpr bool k32 = std::is_same_v<T, float>;
  ragmi::clear_error();
  if (!h || (n > 0 && !rows) || row0 < 0 || n < 0 || row0 + n > h->cap_rows)
    return ragmi::fail(RAG_EINVAL, "bad import range (reserve capacity first)");
  if (k32 && !h->rows32) return ragmi::fail(RAG_EINVAL, "index has fp16 storage (no fp32 rows)");
  if (!k32 && h->rows32)
    return ragmi::fail(RAG_EINVAL, "fp32-storage index: load its fp32 rows (rag_index_import_rows32)");
  if (new_count < 0 || new_count > h->cap_rows)
    return ragmi::fail(RAG_ERANGE, "new_count exceeds capacity");
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  if (n > 0) {
    const size_t bytes = (size_t)n * h->dim * sizeof(T);
    int rc = ensure_stage(h, bytes);
    if (rc) return rc;
    RAG_HIP(hipDeviceSynchronize());
    RAG_HIP(hipMemcpy(h->stage, rows, bytes, hipMemcpyHostToDevice));
    rc = with_dim(h->dim, [&](auto d) {
      constexpr int D = decltype(d)::value;
      const dim3 grid((unsigned)((n * (D / 8) + 255) / 256));
      if constexpr (k32)
        ragmi::import32_kernel<D><<<grid, dim3(256), 0, nullptr>>>(
            static_cast<const float*>(h->stage), row0, n, h->corpus, h->rows32);
      else
        ragmi::import_kernel<D><<<grid, dim3(256), 0, nullptr>>>(
            static_cast<const half8*>(h->stage), row0, n, h->corpus);
      return RAG_OK;
    });
    if (rc) return rc;
    RAG_HIP(hipGetLastError());
    rc = requant(h, nullptr, row0, n, nullptr);
    if (rc) return rc;
    if (tags)
      RAG_HIP(hipMemcpy(h->tags + row0, tags, (size_t)n * 4, hipMemcpyHostToDevice));
    RAG_HIP(hipDeviceSynchronize());
  }
  h->count = new_count;
  return RAG_OK;
}

// The three export entry points: their shared range check, then `body` under the handle's lock
// on its device (need32: only an fp32-storage index has the rows)
template <typename F>
int export_range(rag_index* h, const void* out, int64_t row0, int64_t n, bool need32, F&& body) {
  ragmi::clear_error();
  if (!h || !out || row0 < 0 || n < 0 || row0 + n > h->cap_rows)
    return ragmi::fail(RAG_EINVAL, "bad export range");
  if (need32 && !h->rows32) return ragmi::fail(RAG_EINVAL, "index has fp16 storage (no fp32 rows)");
  if (n == 0) return RAG_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  return body();
}

int upsert_locked(rag_index* h, const float* vecs, const int64_t* rows, const uint32_t* tags,
                  int64_t n, int64_t new_count, hipStream_t st) {
  if (n < 0 || (n > 0 && (!vecs || !rows))) return ragmi::fail(RAG_EINVAL, "bad upsert args");
  if (new_count < 0 || new_count > h->cap_rows)
    return ragmi::fail(RAG_ERANGE, "new_count exceeds capacity (call rag_index_reserve)");
  if (n > 0x7fffffff) return ragmi::fail(RAG_ERANGE, "n too large for one upsert");
  RAG_HIP(hipSetDevice(h->device));
  if (n > 0) {
    const int rc = with_dim(h->dim, [&](auto d) {
      ragmi::upsert_kernel<decltype(d)::value><<<dim3((unsigned)n), dim3(64), 0, st>>>(
          vecs, rows, tags, h->corpus, h->tags, n, h->cap_rows, h->rows32);
      return RAG_OK;
    });
    if (rc) return rc;
    RAG_HIP(hipGetLastError());
    if (const int rq = requant(h, rows, 0, n, st)) return rq;
  }
  h->count = new_count;
  return RAG_OK;
}

// full: the full exact path for every query (rag_index_search_full); it is also taken for
// k > RAG_MAX_K_LARGE (unpacked output only: the exchange merge holds at most that many)
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

// tags: the column the passes filter on, the stored tags unless the caller evaluated a filter
// view of them (search_view_locked)
int search_locked(rag_index* h, const float* q, int B, int k, const uint32_t* filt,
                  int64_t id_offset, float* out_s, int64_t* out_i, int32_t* out_packed,
                  hipStream_t st, bool full = false, const uint32_t* tags = nullptr) {
  if (const int rc = search_args(q, B, k, out_s, out_i, out_packed)) return rc;
  if (!tags) tags = h->tags;
  full = full || k > RAG_MAX_K_LARGE;
  RAG_HIP(hipSetDevice(h->device));
  const bool large = k > RAG_MAX_K || full;
  const int per_pass = large ? ragmi::kQ : ragmi::kQ * h->groups;
  for (int b0 = 0; b0 < B; b0 += per_pass) {
    const int Bq = std::min(per_pass, B - b0);
    Workspace* lru = nullptr;
    Workspace* wp = pick_slot(h->ws, st, lru);
    if (!wp) {
      // every slot is bound to another stream whose last pass may still be running
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

// Diagnostic A/B of scan variants (see scan_kernel's knobs). Returns avg device ms/launch.
template <int D, int V>
void launch_variant(rag_index* h, Workspace& w, int grid, hipStream_t st) {
  using namespace ragmi;
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
  using namespace ragmi;
  Workspace& w = h->ws[0];
  RAG_HIP(hipDeviceSynchronize());
  qprep_kernel<D><<<dim3(kQ), dim3(64), 0, nullptr>>>(q, std::min(B, kQ), nullptr, w.qn,
                                                      w.qfrag, w.filt, w.eps, store_eps(h));
  launch_seed<D, false>(h, w, 1, nullptr);
  // variant 7: the production kernel with every seed threshold at +inf, i.e. the top-k's
  // per-tile compares and branches with no candidate ever taken (its fixed cost)
  if (variant == 7)
    RAG_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(w.seed), 0x7f800000, kQ));
  const int64_t n_tiles = (h->count + 15) / 16;
  // the production grid (launch_search_pass: 3/4 of the CUs); RAGMI_SCAN_WGS overrides
  static ragmi::Knob k_wgs("RAGMI_SCAN_WGS");
  const int cap = k_wgs.get(0) > 0 ? std::max(8, k_wgs.get(0)) : h->scan_wgs;
  int grid = (int)std::min<int64_t>(std::min(h->max_wgs, cap), std::max<int64_t>(1, (n_tiles + 3) / 4));
  grid = std::min(grid, kMaxLists / kWavesPerWG);
#ifdef RAGMI_DIAG_BUILD
  // variant 8: the v_dot2 VALU ablation over a row-group-major copy of the corpus
  DeviceBuf<half8> rows64, qc;
  const int n_groups = (int)((h->count + 63) / 64);
  const int vgrid = std::min(h->max_wgs, std::max(1, (n_groups + 3) / 4));
  if (variant == 8) {
    RAG_HIP(rows64.alloc((size_t)n_groups * 64 * D * 2));
    RAG_HIP(qc.alloc((size_t)kQ * D * 2));
    RAG_HIP(hipMemset(rows64.p, 0, (size_t)n_groups * 64 * D * 2));
    const int64_t total = h->count * (D / 8);
    rows64_kernel<D><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr>>>(
        h->corpus, h->count, rows64.p);
    qchunk_kernel<D><<<dim3(kQ), dim3(64), 0, nullptr>>>(w.qn, qc.p);
  }
#endif
#ifdef RAGMI_DIAG_BUILD
  // variants 17 / 18 / 19: the int8 prescan (scan_kernel_i8) at the production grid —
  // production, MFMA + bound only (no top-k), loads only
  if (variant >= 17) {
    if constexpr (D == 384) {
      if (!h->c8) return ragmi::fail(RAG_EINVAL, "variants 17-19: index keeps no int8 copy");
      launch_prep8<D>(h, w, q, std::min(B, kQ), nullptr, h->tags, nullptr);
      const auto go = [&](auto mode) {
        launch_fixed<kScanBlock>(scan_kernel_i8<D, false, decltype(mode)::value>, dim3(grid), 0,
                                 nullptr, h->c8, h->meta8, h->tags, w.filt,
                                 reinterpret_cast<const intx4*>(w.qfrag8), w.qp8, (int)h->count,
                                 (int)n_tiles, w.seed, w.part_s, w.part_i, w.heads_s, w.heads_i,
                                 w.heads_n);
      };
      float ms8 = 0.f;
      const int rc8 = time_launches(reps, [&]() {
        if (variant == 17) go(std::integral_constant<int, 0>{});
        else if (variant == 18) go(std::integral_constant<int, 1>{});
        else go(std::integral_constant<int, 2>{});
      }, &ms8);
      if (rc8) return rc8;
      RAG_HIP(hipGetLastError());
      *avg_ms = ms8 / reps;
      return RAG_OK;
    } else {
      return ragmi::fail(RAG_EINVAL, "variants 17-19: dim 384 only");
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
  float ms = 0.f;
#ifdef RAGMI_DIAG_BUILD
  if (variant >= 9 && variant <= 14) {
    // one launch per event pair; the tile-queue heads are zeroed before each, outside it
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
  } else
#endif
  {
    const int rc = time_launches(reps, one, &ms);
    if (rc) return rc;
  }
  RAG_HIP(hipGetLastError());
  *avg_ms = ms / reps;
  return RAG_OK;
}

// Diagnostic A/B of the wide (D = 1024, 33..128 queries, unfiltered) scan's variants
// (scan_wide_kernel MODE 0..4; 0 is production). Returns avg device ms/launch.
template <int D>
int bench_wide(rag_index* h, const float* q, int B, int mode, int reps, double* avg_ms) {
  using namespace ragmi;
  Workspace& w = h->ws[0];
  const int groups = (std::min(B, kQ * kMaxGroups) + kQ - 1) / kQ;
  if (groups < 2) return ragmi::fail(RAG_EINVAL, "wide scan variants need 33..128 queries");
  RAG_HIP(hipDeviceSynchronize());
  qprep_kernel<D><<<dim3(groups * kQ), dim3(64), 0, nullptr>>>(
      q, std::min(B, groups * kQ), nullptr, w.qn, w.qfrag, w.filt, w.eps, store_eps(h));
  launch_seed<D, false>(h, w, groups, nullptr);
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
  float ms = 0.f;
  const int rc = time_launches(reps, one, &ms);
  if (rc) return rc;
  RAG_HIP(hipGetLastError());
  *avg_ms = ms / reps;
  return RAG_OK;
}

// the handle's key columns as the kernels take them
ragmi::KeyCols key_cols(const rag_index* h) {
  ragmi::KeyCols kc;
  for (int c = 0; c < RAG_KEYS_MAX_COLS; ++c) kc.col[c] = h->keys[c];
  return kc;
}

// A new key column of `cap` rows: rows [0, keep) copied from `old` (may be NULL with keep = 0),
// rows [keep, cap) RAG_KEY_ABSENT. On the null stream; the caller synchronises the device
// before and after.
int alloc_keys(int64_t cap, const int64_t* old, int64_t keep, DeviceBuf<int64_t>& out) {
  if (out.alloc((size_t)cap * 8) != hipSuccess)
    return ragmi::fail(RAG_ENOMEM, "hipMalloc(key column) failed");
  if (keep > 0) RAG_HIP(hipMemcpy(out.p, old, (size_t)keep * 8, hipMemcpyDeviceToDevice));
  if (cap > keep) {
    const dim3 grid((unsigned)((cap - keep + ragmi::kKeyBlock - 1) / ragmi::kKeyBlock));
    ragmi::fill_keys_kernel<<<grid, dim3(ragmi::kKeyBlock), 0, nullptr>>>(out.p, keep, cap);
    RAG_HIP(hipGetLastError());
  }
  return RAG_OK;
}

// The three indexed row copies behind move / gather / scatter: the shared argument checks,
// then one copy_rows_kernel launch on `st` under the handle's lock. pk32 goes with fp32
// storage exactly; new_count < 0 leaves the count alone (gather).
template <int MODE>
int copy_rows(rag_index* h, const int64_t* src_rows, const int64_t* dst_rows, int64_t n,
              half8* pk16, float* pk32, uint32_t* pktags, int64_t new_count, void* stream) {
  constexpr bool packed = MODE != ragmi::kRowsMove;
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (n < 0 || (n > 0 && ((MODE != ragmi::kRowsScatter && !src_rows) ||
                          (MODE != ragmi::kRowsGather && !dst_rows))))
    return ragmi::fail(RAG_EINVAL, "bad row list (n < 0, or n > 0 with NULL rows)");
  if (packed && n > 0 && (!pk16 || !pktags))
    return ragmi::fail(RAG_EINVAL, "packed fp16 rows and tags are required");
  if (packed && n > 0 && (pk32 != nullptr) != (h->rows32 != nullptr))
    return ragmi::fail(RAG_EINVAL, "packed fp32 rows go with fp32 storage, and only with it");
  if (n > h->cap_rows) return ragmi::fail(RAG_ERANGE, "more rows than the index has slots");
  if (new_count > h->cap_rows)
    return ragmi::fail(RAG_ERANGE, "new_count exceeds capacity (call rag_index_reserve)");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  if (n > 0) {
    const int rc = with_dim(h->dim, [&](auto d) {
      const dim3 grid((unsigned)((n + ragmi::kRowsGroup - 1) / ragmi::kRowsGroup));
      ragmi::copy_rows_kernel<decltype(d)::value, MODE><<<grid, dim3(ragmi::kRowsBlock), 0, st>>>(
          h->corpus, h->rows32, h->tags, src_rows, dst_rows, n, h->cap_rows, pk16, pk32, pktags);
      return RAG_OK;
    });
    if (rc) return rc;
    RAG_HIP(hipGetLastError());
    if constexpr (MODE == ragmi::kRowsMove)
      if (h->n_keys > 0) {   // the keys are a stored form of the row: they move with it
        const dim3 kgrid((unsigned)((n + ragmi::kKeyBlock - 1) / ragmi::kKeyBlock));
        ragmi::move_keys_kernel<<<kgrid, dim3(ragmi::kKeyBlock), 0, st>>>(
            key_cols(h), h->n_keys, src_rows, dst_rows, n, h->cap_rows);
        RAG_HIP(hipGetLastError());
      }
    if constexpr (MODE != ragmi::kRowsGather)   // move / scatter wrote the rows dst_rows
      if (const int rq = requant(h, dst_rows, 0, n, st)) return rq;
  }
  if (new_count >= 0) h->count = new_count;
  return RAG_OK;
}

}  // namespace

extern "C" {

const char* rag_last_error(void) { return ragmi::last_error().c_str(); }
const char* rag_version(void) { return "ragmi 0.1.0 (gfx950)"; }

int rag_index_create(int dim, int64_t capacity_rows, int device, rag_index_t** out) {
  return rag_index_create_ex(dim, capacity_rows, device, RAG_STORE_FP16, out);
}

int rag_index_create_ex(int dim, int64_t capacity_rows, int device, int storage,
                        rag_index_t** out) {
  ragmi::clear_error();
  if (!out) return ragmi::fail(RAG_EINVAL, "out is NULL");
  *out = nullptr;
  if (dim != 384 && dim != 1024) return ragmi::fail(RAG_EINVAL, "dim must be 384 or 1024");
  const bool diag = (storage & RAG_CREATE_DIAGNOSTIC) != 0;
  storage &= ~RAG_CREATE_DIAGNOSTIC;
  if (storage != RAG_STORE_FP16 && storage != RAG_STORE_FP32)
    return ragmi::fail(RAG_EINVAL, "storage must be RAG_STORE_FP16 or RAG_STORE_FP32");
  if (capacity_rows < 0 || capacity_rows > (int64_t(1) << 31) - 16)
    return ragmi::fail(RAG_ERANGE, "capacity_rows out of range [0, 2^31-16]");
  RAG_HIP(hipSetDevice(device));
  auto* h = new rag_index();
  h->dim = dim;
  h->device = device;
  h->cap_rows = round16(std::max<int64_t>(capacity_rows, 16));
  h->storage = storage;
  int rc = alloc_corpus(h, h->cap_rows, &h->corpus, &h->tags);
  if (rc) {
    delete h;
    return rc;
  }
  if (keeps_copy8(h)) {
    DeviceBuf<char> c8;
    DeviceBuf<float> m8;
    rc = alloc_copy8(h, h->cap_rows, c8, m8);
    if (rc) {
      rag_index_destroy(h);
      return rc;
    }
    h->c8 = c8.release();
    h->meta8 = m8.release();
  }
  if (storage == RAG_STORE_FP32) {
    const size_t b32 = (size_t)h->cap_rows * dim * 4;
    if (hipMalloc(reinterpret_cast<void**>(&h->rows32), b32) != hipSuccess ||
        hipMemset(h->rows32, 0, b32) != hipSuccess) {
      rag_index_destroy(h);
      return ragmi::fail(RAG_ENOMEM, "hipMalloc(rows32) failed");
    }
  }
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) !=
          hipSuccess ||
      n_cu <= 0)
    n_cu = 256;
  h->n_cu = n_cu;
  h->max_wgs = n_cu * 2;  // 2 x 256-thread workgroups per CU (__launch_bounds__(256, 2))
  h->scan_wgs = std::max(8, (n_cu * 3 / 4) & ~7);
  // wide rows (LDS-query scan) take up to 4 query groups (128 queries) per pass
  h->groups = dim > 384 ? kMaxGroups : 1;
  for (auto& w : h->ws) {
    // one hipMalloc per buffer, in the table's order (see ragmi/dist.py on allocation placement)
    if (ragmi::ws_alloc_all(ws_buffers(h, w)) != hipSuccess) {
      rag_index_destroy(h);
      return ragmi::fail(RAG_ENOMEM, "workspace allocation failed");
    }
  }
  if (diag) {
    h->diagnostic = true;
    ragmi::diagnostic_acquire();
  }
  *out = h;
  return RAG_OK;
}

int rag_diagnostic_build(void) {
#ifdef RAGMI_DIAG_BUILD
  return 1;
#else
  return 0;
#endif
}

int rag_knob_probe(const char* name, int dflt) {
  if (!name) return dflt;
  ragmi::Knob k(name);
  return k.get(dflt);
}

int rag_index_destroy(rag_index_t* h) {
  ragmi::clear_error();
  if (!h) return RAG_OK;
  if (h->diagnostic) ragmi::diagnostic_release();
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (auto& w : h->ws) {
    ragmi::ws_free_all(ws_buffers(h, w));
    ragmi::ws_free_all(lk_buffers(w));
    if (w.ev_in) (void)hipEventDestroy(w.ev_in);
    if (w.ev_out) (void)hipEventDestroy(w.ev_out);
  }
  for (auto& p : h->prof_pairs) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  if (h->scan_done) (void)hipEventDestroy(h->scan_done);
  if (h->scan_stream) (void)hipStreamDestroy(h->scan_stream);
  if (h->corpus) (void)hipFree(h->corpus);
  if (h->tags) (void)hipFree(h->tags);
  for (auto* k : h->keys)
    if (k) (void)hipFree(k);
  if (h->rows32) (void)hipFree(h->rows32);
  if (h->c8) (void)hipFree(h->c8);
  if (h->meta8) (void)hipFree(h->meta8);
  if (h->stage) (void)hipFree(h->stage);
  for (auto& v : h->views)
    if (v.p) (void)hipFree(v.p);
  delete h;
  return RAG_OK;
}

int rag_index_reserve(rag_index_t* h, int64_t capacity_rows) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (capacity_rows > (int64_t(1) << 31) - 16)
    return ragmi::fail(RAG_ERANGE, "capacity_rows out of range");
  std::lock_guard<std::mutex> lk(h->mu);
  const int64_t cap = round16(capacity_rows);
  if (cap <= h->cap_rows) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  // the new buffers are freed on every error return below; released once the handle owns them
  DeviceBuf<half8> nc;
  DeviceBuf<uint32_t> nt;
  DeviceBuf<float> n32;
  int rc = alloc_corpus(h, cap, &nc.p, &nt.p);
  if (rc) return rc;
  if (h->rows32) {
    const size_t b32 = (size_t)cap * h->dim * 4;
    if (n32.alloc(b32) != hipSuccess) return ragmi::fail(RAG_ENOMEM, "hipMalloc(rows32) failed");
    RAG_HIP(hipMemset(n32.p, 0, b32));
  }
  DeviceBuf<char> n8;
  DeviceBuf<float> nm8;
  if (h->c8) {
    rc = alloc_copy8(h, cap, n8, nm8);
    if (rc) return rc;
  }
  RAG_HIP(hipDeviceSynchronize());
  // the key columns regrow with the tags: old rows keep their keys, new rows hold ABSENT
  DeviceBuf<int64_t> nk[RAG_KEYS_MAX_COLS];
  for (int c = 0; c < h->n_keys; ++c)
    if ((rc = alloc_keys(cap, h->keys[c], h->cap_rows, nk[c]))) return rc;
  if (h->n_keys > 0) RAG_HIP(hipDeviceSynchronize());
  RAG_HIP(hipMemcpy(nc.p, h->corpus, (size_t)h->cap_rows * h->dim * 2, hipMemcpyDeviceToDevice));
  RAG_HIP(hipMemcpy(nt.p, h->tags, (size_t)h->cap_rows * 4, hipMemcpyDeviceToDevice));
  if (n32.p)
    RAG_HIP(hipMemcpy(n32.p, h->rows32, (size_t)h->cap_rows * h->dim * 4,
                      hipMemcpyDeviceToDevice));
  if (n8.p) {
    // whole tiles of the old capacity (its spare tile holds no row)
    RAG_HIP(hipMemcpy(n8.p, h->c8, (size_t)(h->cap_rows / 16) * (h->dim / 64) * 1024,
                      hipMemcpyDeviceToDevice));
    RAG_HIP(hipMemcpy(nm8.p, h->meta8, (size_t)(h->cap_rows / 16) * 32 * 4,
                      hipMemcpyDeviceToDevice));
    (void)hipFree(h->c8);
    (void)hipFree(h->meta8);
    h->c8 = n8.release();
    h->meta8 = nm8.release();
  }
  (void)hipFree(h->corpus);
  (void)hipFree(h->tags);
  if (h->rows32) (void)hipFree(h->rows32);
  h->corpus = nc.release();
  h->tags = nt.release();
  h->rows32 = n32.release();
  for (int c = 0; c < h->n_keys; ++c) {
    (void)hipFree(h->keys[c]);
    h->keys[c] = nk[c].release();
  }
  h->cap_rows = cap;
  return RAG_OK;
}

int64_t rag_index_capacity(const rag_index_t* h) { return h ? h->cap_rows : -1; }
int64_t rag_index_count(const rag_index_t* h) { return h ? h->count : -1; }
int rag_index_dim(const rag_index_t* h) { return h ? h->dim : -1; }

int rag_index_upsert(rag_index_t* h, const float* vecs, const int64_t* rows,
                     const uint32_t* tags, int64_t n, int64_t new_count, void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  return upsert_locked(h, vecs, rows, tags, n, new_count, static_cast<hipStream_t>(stream));
}

int rag_index_upsert_host(rag_index_t* h, const float* vecs, const int64_t* rows,
                          const uint32_t* tags, int64_t n, int64_t new_count) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (n < 0 || (n > 0 && (!vecs || !rows))) return ragmi::fail(RAG_EINVAL, "bad upsert args");
  for (int64_t i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= h->cap_rows)
      return ragmi::fail(RAG_ERANGE, "row slot beyond capacity (call rag_index_reserve)");
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  const size_t vb = (size_t)n * h->dim * 4, rb = (size_t)n * 8, tb = (size_t)n * 4;
  int rc = ensure_stage(h, vb + rb + tb + 64);
  if (rc) return rc;
  char* base = static_cast<char*>(h->stage);
  RAG_HIP(hipDeviceSynchronize());
  if (n > 0) {
    RAG_HIP(hipMemcpy(base, vecs, vb, hipMemcpyHostToDevice));
    RAG_HIP(hipMemcpy(base + vb, rows, rb, hipMemcpyHostToDevice));
    if (tags) RAG_HIP(hipMemcpy(base + vb + rb, tags, tb, hipMemcpyHostToDevice));
  }
  rc = upsert_locked(h, reinterpret_cast<float*>(base), reinterpret_cast<int64_t*>(base + vb),
                     tags ? reinterpret_cast<uint32_t*>(base + vb + rb) : nullptr, n, new_count,
                     nullptr);
  if (rc) return rc;
  RAG_HIP(hipDeviceSynchronize());
  return RAG_OK;
}

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
  if (id_offset < 0 || id_offset + h->count > INT32_MAX)
    return ragmi::fail(RAG_ERANGE, "packed ids are int32: global rows must stay below 2^31");
  std::lock_guard<std::mutex> lk(h->mu);
  return search_locked(h, q, B, k, filters, id_offset, nullptr, nullptr, out_packed,
                       static_cast<hipStream_t>(stream));
}

int rag_index_search_host(rag_index_t* h, const float* q, int B, int k,
                          const uint32_t* filters, int64_t id_offset, float* out_s,
                          int64_t* out_i) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (B < 0 || (B > 0 && (!q || !out_s || !out_i))) return ragmi::fail(RAG_EINVAL, "bad search args");
  if (k < 1) return ragmi::fail(RAG_ERANGE, "k must be >= 1");
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

int rag_index_export_rows(rag_index_t* h, int64_t row0, int64_t n, uint16_t* out) {
  return export_range(h, out, row0, n, false, [&]() -> int {
    const size_t bytes = (size_t)n * h->dim * 2;
    int rc = ensure_stage(h, bytes);
    if (rc) return rc;
    RAG_HIP(hipDeviceSynchronize());
    rc = with_dim(h->dim, [&](auto d) {
      constexpr int D = decltype(d)::value;
      const int blocks = (int)((n * (D / 8) + 255) / 256);
      ragmi::export_kernel<D><<<dim3(blocks), dim3(256), 0, nullptr>>>(
          h->corpus, row0, n, static_cast<half8*>(h->stage));
      return RAG_OK;
    });
    if (rc) return rc;
    RAG_HIP(hipGetLastError());
    RAG_HIP(hipDeviceSynchronize());
    RAG_HIP(hipMemcpy(out, h->stage, bytes, hipMemcpyDeviceToHost));
    return RAG_OK;
  });
}

int rag_index_import_rows(rag_index_t* h, int64_t row0, int64_t n, const uint16_t* rows,
                          const uint32_t* tags, int64_t new_count) {
  return import_rows(h, row0, n, rows, tags, new_count);
}

int rag_index_storage(const rag_index_t* h) { return h ? h->storage : -1; }

int rag_index_export_rows32(rag_index_t* h, int64_t row0, int64_t n, float* out) {
  return export_range(h, out, row0, n, true, [&]() -> int {
    RAG_HIP(hipDeviceSynchronize());
    RAG_HIP(hipMemcpy(out, h->rows32 + row0 * h->dim, (size_t)n * h->dim * 4,
                      hipMemcpyDeviceToHost));
    return RAG_OK;
  });
}

int rag_index_import_rows32(rag_index_t* h, int64_t row0, int64_t n, const float* rows,
                            const uint32_t* tags, int64_t new_count) {
  return import_rows(h, row0, n, rows, tags, new_count);
}

int rag_index_export_tags(rag_index_t* h, int64_t row0, int64_t n, uint32_t* out) {
  return export_range(h, out, row0, n, false, [&]() -> int {
    RAG_HIP(hipDeviceSynchronize());
    RAG_HIP(hipMemcpy(out, h->tags + row0, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RAG_OK;
  });
}

// ---- row removal: select, move, gather, scatter (rows_kernels.hip) ----

namespace {

// the ordered select (count / prefix sum / emit) over tag column `tags` of h->count rows
int select_locked(rag_index* h, const uint32_t* tags, uint32_t tag_mask, uint32_t tag_value,
                  int64_t* out_rows, int64_t cap, int64_t* out_n, hipStream_t st) {
  const int64_t count = h->count;
  const int nb = (int)((count + ragmi::kSelChunk - 1) / ragmi::kSelChunk);
  if (nb == 0) {
    RAG_HIP(hipMemsetAsync(out_n, 0, sizeof(int64_t), st));
    return RAG_OK;
  }
  StreamScratch offsets(st);   // matches per chunk, then their exclusive prefix sums
  RAG_HIP(offsets.alloc((size_t)nb * sizeof(int64_t)));
  int64_t* const off = reinterpret_cast<int64_t*>(offsets.p);
  ragmi::select_count_kernel<<<dim3((unsigned)nb), dim3(ragmi::kSelBlock), 0, st>>>(
      tags, count, tag_mask, tag_value, off);
  ragmi::select_scan_kernel<<<dim3(1), dim3(ragmi::kSelScanBlock), 0, st>>>(off, nb, out_n);
  if (cap > 0)
    ragmi::select_emit_kernel<<<dim3((unsigned)nb), dim3(ragmi::kSelBlock), 0, st>>>(
        tags, count, tag_mask, tag_value, off, out_rows, cap);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// ---- filter views (filter_kernels.hip) ----

// the blob rules of every *_view entry point, checked before any HIP call
int view_args(const uint32_t* progs, int64_t words, int n_programs) {
  if (!progs) return ragmi::fail(RAG_EINVAL, "filter view: the program blob is NULL");
  if (n_programs < 1 || n_programs > RAG_FILTER_MAX_PROGRAMS)
    return ragmi::fail(RAG_EINVAL, "filter view: n_programs must be in [1, RAG_FILTER_MAX_PROGRAMS=32]");
  if (words < (int64_t)n_programs * RAG_FILTER_REC_WORDS || words > UINT32_MAX)
    return ragmi::fail(RAG_EINVAL, "filter view: `words` is smaller than n_programs records of 41 "
                                   "words (or not below 2^32)");
  return RAG_OK;
}

// filter_view_kernel over the handle's cap_rows rows into `view` (>= cap_rows words)
int launch_filter_view(rag_index* h, const uint32_t* progs, int64_t words, int n_programs,
                       uint32_t* view, hipStream_t st) {
  using namespace ragmi;
  if (h->cap_rows == 0) return RAG_OK;
  const int64_t chunks = (h->cap_rows + kFvBlock * 4 - 1) / (kFvBlock * 4);
  const dim3 grid((unsigned)std::min<int64_t>(chunks, (int64_t)kFvWgPerCu * h->n_cu));
  // an index with key columns: the instantiations that know the RANGE atom (one more word of
  // LDS, the mask of the columns the blob names); without columns, the kernel as it always was
  const bool pool = words <= kFvLdsWords;
  const size_t lds = (pool ? (size_t)words : (size_t)n_programs * RAG_FILTER_REC_WORDS) * 4;
  const KeyCols kc = key_cols(h);
  const auto launch = [&](auto pool_lds, auto with_keys) {
    constexpr bool P = decltype(pool_lds)::value, K = decltype(with_keys)::value;
    filter_view_kernel<P, K><<<grid, dim3(kFvBlock), lds + (K ? 4 : 0), st>>>(
        h->tags, h->count, h->cap_rows, progs, (uint32_t)words, n_programs, view, kc, h->n_keys);
  };
  if (h->n_keys > 0) {
    if (pool) launch(std::true_type{}, std::true_type{});
    else launch(std::false_type{}, std::true_type{});
  } else {
    if (pool) launch(std::true_type{}, std::false_type{});
    else launch(std::false_type{}, std::false_type{});
  }
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// The view column of a call: a buffer kept per stream beside the workspace slots (ViewSlot), of
// the stored tags' extent, grown when the capacity grew. A stream-ordered allocation per call
// (as the full pass and the select take their scratch) was built and measured first: with view
// searches back to back the call then waited ~0.25 ms on the host before its first kernel, at
// 1M and at 10M rows alike, more than the whole 1M-row search. Kept buffers cost
// 4 B per row of capacity per stream that ever sent a general filter, and no call has anything
// to release, on any path. The slot of stream `st`, else an unused one; every slot bound to
// another stream whose last call may still read its column: the device is drained once and the
// least recently used slot rebound, as search_locked does for workspaces. hipFree waits for
// the device, so a column is never freed under a pass that reads it.
int acquire_view(rag_index* h, hipStream_t st, uint32_t** view) {
  ViewSlot* lru = nullptr;
  ViewSlot* sp = pick_slot(h->views, st, lru);
  if (!sp) {
    RAG_HIP(hipDeviceSynchronize());
    sp = lru;
  }
  const size_t need = std::max<size_t>((size_t)h->cap_rows * 4, 16);
  if (sp->bytes < need) {
    if (sp->p) (void)hipFree(sp->p);
    sp->p = nullptr;
    sp->bytes = 0;
    if (hipMalloc(reinterpret_cast<void**>(&sp->p), need) != hipSuccess) {
      (void)hipGetLastError();
      sp->p = nullptr;
      return ragmi::fail(RAG_ENOMEM, "hipMalloc(filter view) failed");
    }
    sp->bytes = need;
  }
  sp->used = true;
  sp->owner = st;
  sp->tick = ++h->view_tick;
  *view = sp->p;
  return RAG_OK;
}

}  // namespace

int rag_index_select_rows(rag_index_t* h, uint32_t tag_mask, uint32_t tag_value,
                          int64_t* out_rows, int64_t cap, int64_t* out_n, void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (!out_n || cap < 0 || (cap > 0 && !out_rows))
    return ragmi::fail(RAG_EINVAL, "bad select args (out_n NULL, or cap > 0 without out_rows)");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  return select_locked(h, h->tags, tag_mask, tag_value, out_rows, cap, out_n, st);
}

int rag_index_filter_view(rag_index_t* h, const uint32_t* progs, int64_t words, int n_programs,
                          uint32_t* out_view, void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (const int rc = view_args(progs, words, n_programs)) return rc;
  if (!out_view || (reinterpret_cast<uintptr_t>(out_view) & 15))
    return ragmi::fail(RAG_EINVAL, "filter view: out_view_dev is NULL or not 16-byte aligned");
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  return launch_filter_view(h, progs, words, n_programs, out_view,
                            static_cast<hipStream_t>(stream));
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
  if (out_packed && (id_offset < 0 || id_offset + h->count > INT32_MAX))
    return ragmi::fail(RAG_ERANGE, "packed ids are int32: global rows must stay below 2^31");
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

int rag_index_select_rows_view(rag_index_t* h, const uint32_t* progs, int64_t words,
                               int64_t* out_rows, int64_t cap, int64_t* out_n, void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (const int rc = view_args(progs, words, 1)) return rc;
  if (!out_n || cap < 0 || (cap > 0 && !out_rows))
    return ragmi::fail(RAG_EINVAL, "bad select args (out_n NULL, or cap > 0 without out_rows)");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  uint32_t* v = nullptr;
  if (const int rc = acquire_view(h, st, &v)) return rc;
  if (const int rc = launch_filter_view(h, progs, words, 1, v, st)) return rc;
  return select_locked(h, v, 1u, 1u, out_rows, cap, out_n, st);
}

int rag_index_move_rows(rag_index_t* h, const int64_t* src_rows, const int64_t* dst_rows,
                        int64_t n, int64_t new_count, void* stream) {
  if (new_count < 0) {
    ragmi::clear_error();
    return ragmi::fail(h ? RAG_ERANGE : RAG_EINVAL, h ? "new_count is negative" : "index is NULL");
  }
  return copy_rows<ragmi::kRowsMove>(h, src_rows, dst_rows, n, nullptr, nullptr, nullptr,
                                     new_count, stream);
}

int rag_index_gather_rows(rag_index_t* h, const int64_t* rows, int64_t n, uint16_t* out_f16,
                          float* out_f32, uint32_t* out_tags, void* stream) {
  return copy_rows<ragmi::kRowsGather>(h, rows, nullptr, n, reinterpret_cast<half8*>(out_f16),
                                       out_f32, out_tags, -1, stream);
}

int rag_index_scatter_rows(rag_index_t* h, const int64_t* rows, int64_t n, const uint16_t* in_f16,
                           const float* in_f32, const uint32_t* in_tags, int64_t new_count,
                           void* stream) {
  if (new_count < 0) {
    ragmi::clear_error();
    return ragmi::fail(h ? RAG_ERANGE : RAG_EINVAL, h ? "new_count is negative" : "index is NULL");
  }
  return copy_rows<ragmi::kRowsScatter>(
      h, nullptr, rows, n, reinterpret_cast<half8*>(const_cast<uint16_t*>(in_f16)),
      const_cast<float*>(in_f32), const_cast<uint32_t*>(in_tags), new_count, stream);
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

// ---- grouped search: tag gather (rows_kernels.hip) and group selection (reselect_kernels.hip) ----

int rag_index_gather_tags(rag_index_t* h, const int64_t* rows, int64_t n, uint32_t* out_tags,
                          void* stream) {
  ragmi::clear_error();
  if (n < 0) return ragmi::fail(RAG_EINVAL, "gather_tags: n must be >= 0");
  if (n > 0 && (!rows || !out_tags))
    return ragmi::fail(RAG_EINVAL, "gather_tags: a NULL rows or output pointer");
  if (!h) return ragmi::fail(RAG_EINVAL, "gather_tags: index is NULL");
  if (n == 0) return RAG_OK;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  const dim3 grid((unsigned)((n + ragmi::kTagBlock - 1) / ragmi::kTagBlock));
  ragmi::gather_tags_kernel<<<grid, dim3(ragmi::kTagBlock), 0, st>>>(h->tags, rows, n, h->cap_rows,
                                                                     out_tags);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// ---- key columns (rows_kernels.hip; the RANGE atom of filter_kernels.hip reads them) ----

int rag_index_keys_create(rag_index_t* h, int n_cols) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "keys_create: index is NULL");
  if (n_cols < 1 || n_cols > RAG_KEYS_MAX_COLS)
    return ragmi::fail(RAG_ERANGE, "keys_create: n_cols must be in [1, RAG_KEYS_MAX_COLS=4]");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n_cols <= h->n_keys) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  DeviceBuf<int64_t> nk[RAG_KEYS_MAX_COLS];
  for (int c = h->n_keys; c < n_cols; ++c)
    if (const int rc = alloc_keys(h->cap_rows, nullptr, 0, nk[c])) return rc;
  // searches in flight read the handle's columns by value: drain them before the count changes
  RAG_HIP(hipDeviceSynchronize());
  for (int c = h->n_keys; c < n_cols; ++c) h->keys[c] = nk[c].release();
  h->n_keys = n_cols;
  return RAG_OK;
}

int rag_index_keys_cols(const rag_index_t* h) { return h ? h->n_keys : -1; }

namespace {

// the shared argument checks of write_keys / gather_keys; *go = false when there is nothing to do
int keys_args(rag_index* h, const int64_t* rows, const void* other, int64_t n, bool* go) {
  *go = false;
  if (n < 0) return ragmi::fail(RAG_EINVAL, "keys: n must be >= 0");
  if (n > 0 && (!rows || !other)) return ragmi::fail(RAG_EINVAL, "keys: a NULL rows or keys pointer");
  if (!h) return ragmi::fail(RAG_EINVAL, "keys: index is NULL");
  *go = n > 0;
  return RAG_OK;
}

}  // namespace

int rag_index_write_keys(rag_index_t* h, int col, const int64_t* rows, const int64_t* keys,
                         int64_t n, void* stream) {
  ragmi::clear_error();
  bool go = false;
  if (const int rc = keys_args(h, rows, keys, n, &go)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  if (col < 0 || col >= h->n_keys)
    return ragmi::fail(RAG_ERANGE, "keys: no such column (call rag_index_keys_create)");
  if (!go) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  const dim3 grid((unsigned)((n + ragmi::kKeyBlock - 1) / ragmi::kKeyBlock));
  ragmi::write_keys_kernel<<<grid, dim3(ragmi::kKeyBlock), 0, st>>>(h->keys[col], rows, keys, n,
                                                                     h->cap_rows);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

int rag_index_gather_keys(rag_index_t* h, int col, const int64_t* rows, int64_t n,
                          int64_t* out_keys, void* stream) {
  ragmi::clear_error();
  bool go = false;
  if (const int rc = keys_args(h, rows, out_keys, n, &go)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  if (col < 0 || col >= h->n_keys)
    return ragmi::fail(RAG_ERANGE, "keys: no such column (call rag_index_keys_create)");
  if (!go) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  const dim3 grid((unsigned)((n + ragmi::kKeyBlock - 1) / ragmi::kKeyBlock));
  ragmi::gather_keys_kernel<<<grid, dim3(ragmi::kKeyBlock), 0, st>>>(h->keys[col], rows, n,
                                                                      h->cap_rows, out_keys);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

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

// ---------------------------------------------------------------------------------------
// shard set: N flat indexes searched as one (global row g on shard g % N at local row g / N)
// ---------------------------------------------------------------------------------------
namespace {

// Per-search buffers and events. A slot stays bound to the stream of its last search (that
// stream orders its reuse); another stream taking it first waits for the slot's `done` event,
// so concurrent searches on several streams never share a list buffer in flight.
constexpr int kSetSlots = 4;

struct SetSlot {
  hipEvent_t fan = nullptr, done = nullptr;      // merge device
  hipEvent_t join[RAG_MAX_SHARDS] = {};          // shard s's device
  char* stack = nullptr;                         // merge device: the shards' lists, side by side
  size_t stack_bytes = 0;
  char* remote[RAG_MAX_SHARDS] = {};             // shard s's device (s off the merge device):
  size_t remote_bytes[RAG_MAX_SHARDS] = {};      // queries, filters, its list
  hipStream_t owner = nullptr;
  bool used = false;
  uint64_t tick = 0;
};

// the calling thread's current device, put back on every exit path
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
  ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
};

static size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

struct rag_shardset {
  int n = 0;
  int dim = 0;
  int dev0 = 0;                                  // merge device = shard 0's
  rag_index* shard[RAG_MAX_SHARDS] = {};         // borrowed
  int dev[RAG_MAX_SHARDS] = {};                  // shard s's device (destroy reads no shard)
  hipStream_t stream[RAG_MAX_SHARDS] = {};       // shard s's own stream, on its device
  SetSlot slot[kSetSlots];
  uint64_t tick = 0;
  std::mutex mu;
};

namespace {

// grow *buf (on the current device) to `bytes`; the slot's last search is over first
static int set_ensure(SetSlot& sl, char** buf, size_t* have, size_t bytes) {
  if (*have >= bytes) return RAG_OK;
  if (sl.used) RAG_HIP(hipEventSynchronize(sl.done));
  if (*buf) RAG_HIP(hipFree(*buf));
  *buf = nullptr;
  *have = 0;
  RAG_HIP(hipMalloc(reinterpret_cast<void**>(buf), bytes));
  *have = bytes;
  return RAG_OK;
}

// progs (NULL: the plain search): the filter programs of a view search, `words` words for
// n_programs programs, on the merge device like the filters
static int shardset_search_locked(rag_shardset* set, const float* q, int B, int k, const uint32_t* filt,
                           bool full, float* out_s, int64_t* out_i, uint8_t* out_empty,
                           hipStream_t st, const uint32_t* progs = nullptr, int64_t words = 0,
                           int n_programs = 0) {
  const int n = set->n;
  const bool packed = !full && k <= RAG_MAX_K_LARGE;
  // all slots busy: the least recently used one, after its `done` event (below)
  SetSlot* lru = nullptr;
  SetSlot* sp = pick_slot(set->slot, st, lru);
  SetSlot& sl = sp ? *sp : *lru;
  RAG_HIP(hipSetDevice(set->dev0));
  if (sl.used && sl.owner != st) RAG_HIP(hipStreamWaitEvent(st, sl.done, 0));
  // stack: packed [n][B][k][2] int32, or scores [n][B][k] fp32 then ids [n][B][k] int64
  const size_t bk = (size_t)B * k;
  const size_t ids_off = up256((size_t)n * bk * 4);
  int rc = set_ensure(sl, &sl.stack, &sl.stack_bytes, packed ? (size_t)n * bk * 8
                                                             : ids_off + (size_t)n * bk * 8);
  if (rc) return rc;
  const size_t qb = up256((size_t)B * set->dim * 4), fb = up256((size_t)B * 8);
  const size_t pb = progs ? up256((size_t)words * 4) : 0;   // a remote shard's copy of the blob
  for (int s = 0; s < n; ++s)
    if (set->shard[s]->device != set->dev0) {
      RAG_HIP(hipSetDevice(set->shard[s]->device));
      rc = set_ensure(sl, &sl.remote[s], &sl.remote_bytes[s],
                      qb + fb + up256(bk * 4) + up256(bk * 8) + pb);
      if (rc) return rc;
    }
  RAG_HIP(hipSetDevice(set->dev0));
  RAG_HIP(hipEventRecord(sl.fan, st));
  sl.used = true;
  sl.owner = st;
  sl.tick = ++set->tick;
  // fan out: every shard searches on its own stream, behind the caller's stream
  for (int s = 0; s < n && rc == RAG_OK; ++s) {
    rag_index* h = set->shard[s];
    hipStream_t ss = set->stream[s];
    const bool remote = h->device != set->dev0;
    RAG_HIP(hipSetDevice(h->device));
    RAG_HIP(hipStreamWaitEvent(ss, sl.fan, 0));
    // where this shard's list goes on the merge device, and where its search writes it
    int32_t* pk = reinterpret_cast<int32_t*>(sl.stack) + (size_t)s * bk * 2;
    float* os = reinterpret_cast<float*>(sl.stack) + (size_t)s * bk;
    int64_t* oi = reinterpret_cast<int64_t*>(sl.stack + ids_off) + (size_t)s * bk;
    const float* qs = q;
    const uint32_t* fs = filt;
    char* r = sl.remote[s];
    if (remote) {
      RAG_HIP(hipMemcpyPeerAsync(r, h->device, q, set->dev0, (size_t)B * set->dim * 4, ss));
      qs = reinterpret_cast<const float*>(r);
      if (filt) {
        RAG_HIP(hipMemcpyPeerAsync(r + qb, h->device, filt, set->dev0, (size_t)B * 8, ss));
        fs = reinterpret_cast<const uint32_t*>(r + qb);
      }
    }
    const uint32_t* ps = progs;
    if (remote && progs) {
      char* const rp = r + qb + fb + up256(bk * 4) + up256(bk * 8);
      RAG_HIP(hipMemcpyPeerAsync(rp, h->device, progs, set->dev0, (size_t)words * 4, ss));
      ps = reinterpret_cast<const uint32_t*>(rp);
    }
    int32_t* w_pk = remote ? reinterpret_cast<int32_t*>(r + qb + fb) : pk;
    float* w_os = remote ? reinterpret_cast<float*>(r + qb + fb) : os;
    int64_t* w_oi = remote ? reinterpret_cast<int64_t*>(r + qb + fb + up256(bk * 4)) : oi;
    if (h->count == 0) {
      // nothing stored here yet (fewer rows than shards): an all -1 list
      if (packed) RAG_HIP(hipMemsetAsync(w_pk, 0xFF, bk * 8, ss));
      else RAG_HIP(hipMemsetAsync(w_oi, 0xFF, bk * 8, ss));
    } else if (progs) {
      rc = rag_index_search_view(h, qs, B, k, ps, words, n_programs, fs, 0,
                                 full ? RAG_SEARCH_FULL : 0, w_os, w_oi, packed ? w_pk : nullptr,
                                 ss);
    } else if (packed) {
      rc = rag_index_search_packed(h, qs, B, k, fs, 0, w_pk, ss);
    } else {
      rc = (full ? rag_index_search_full : rag_index_search)(h, qs, B, k, fs, 0, w_os, w_oi, ss);
    }
    if (rc) break;
    if (remote) {
      if (packed) {
        RAG_HIP(hipMemcpyPeerAsync(pk, set->dev0, w_pk, h->device, bk * 8, ss));
      } else {
        RAG_HIP(hipMemcpyPeerAsync(os, set->dev0, w_os, h->device, bk * 4, ss));
        RAG_HIP(hipMemcpyPeerAsync(oi, set->dev0, w_oi, h->device, bk * 8, ss));
      }
    }
    RAG_HIP(hipSetDevice(h->device));
    RAG_HIP(hipEventRecord(sl.join[s], ss));
  }
  if (rc) return rc;
  // join, then one merge on the caller's stream
  RAG_HIP(hipSetDevice(set->dev0));
  for (int s = 0; s < n; ++s) RAG_HIP(hipStreamWaitEvent(st, sl.join[s], 0));
  if (packed) {
    const int32_t* lists[RAG_MAX_SHARDS];
    int64_t add[RAG_MAX_SHARDS];
    for (int s = 0; s < n; ++s) {
      lists[s] = reinterpret_cast<const int32_t*>(sl.stack) + (size_t)s * bk * 2;
      add[s] = s;
    }
    rc = rag_merge_topk_gather(lists, n, B, k, n, add, out_s, out_i, out_empty, st);
  } else {
    const unsigned gx = (unsigned)std::min<size_t>(1024, (bk + 255) / 256);
    ragmi::remap_ids_kernel<<<dim3(gx, n), dim3(256), 0, st>>>(
        reinterpret_cast<int64_t*>(sl.stack + ids_off), B, k, n, out_empty);
    RAG_HIP(hipGetLastError());
    rc = rag_merge_topk(reinterpret_cast<const float*>(sl.stack),
                        reinterpret_cast<const int64_t*>(sl.stack + ids_off), n, B, k, out_s,
                        out_i, st);
  }
  if (rc) return rc;
  RAG_HIP(hipEventRecord(sl.done, st));
  return RAG_OK;
}

}  // namespace

int rag_shardset_create(rag_index_t* const* shards, int n_shards, rag_shardset_t** out) {
  ragmi::clear_error();
  if (!shards || !out) return ragmi::fail(RAG_EINVAL, "shard set: NULL argument");
  if (n_shards < 1 || n_shards > RAG_MAX_SHARDS)
    return ragmi::fail(RAG_EINVAL, "shard set: n_shards must be in [1, RAG_MAX_SHARDS=64]");
  for (int s = 0; s < n_shards; ++s) {
    if (!shards[s]) return ragmi::fail(RAG_EINVAL, "shard set: a shard handle is NULL");
    if (shards[s]->dim != shards[0]->dim || shards[s]->storage != shards[0]->storage)
      return ragmi::fail(RAG_EINVAL, "shard set: every shard must have the same dim and storage");
  }
  DeviceGuard guard;
  rag_shardset* set = new rag_shardset();
  set->n = n_shards;
  set->dim = shards[0]->dim;
  set->dev0 = shards[0]->device;
  for (int s = 0; s < n_shards; ++s) {
    set->shard[s] = shards[s];
    set->dev[s] = shards[s]->device;
  }
  auto make = [&]() -> int {
    for (int s = 0; s < n_shards; ++s) {
      RAG_HIP(hipSetDevice(shards[s]->device));
      RAG_HIP(hipStreamCreateWithFlags(&set->stream[s], hipStreamNonBlocking));
      for (auto& sl : set->slot)
        RAG_HIP(hipEventCreateWithFlags(&sl.join[s], hipEventDisableTiming));
    }
    RAG_HIP(hipSetDevice(set->dev0));
    for (auto& sl : set->slot) {
      RAG_HIP(hipEventCreateWithFlags(&sl.fan, hipEventDisableTiming));
      RAG_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    return RAG_OK;
  };
  const int rc = make();
  if (rc) {
    const std::string msg = ragmi::last_error();
    rag_shardset_destroy(set);
    return ragmi::fail(rc, msg);
  }
  *out = set;
  return RAG_OK;
}

int rag_shardset_destroy(rag_shardset_t* set) {
  ragmi::clear_error();
  if (!set) return RAG_OK;
  DeviceGuard guard;
  for (int s = 0; s < set->n; ++s) {
    (void)hipSetDevice(set->dev[s]);
    if (set->stream[s]) {
      (void)hipStreamSynchronize(set->stream[s]);
      (void)hipStreamDestroy(set->stream[s]);
    }
    for (auto& sl : set->slot) {
      if (sl.join[s]) (void)hipEventDestroy(sl.join[s]);
      if (sl.remote[s]) (void)hipFree(sl.remote[s]);
    }
  }
  (void)hipSetDevice(set->dev0);
  for (auto& sl : set->slot) {
    if (sl.used) (void)hipEventSynchronize(sl.done);
    if (sl.fan) (void)hipEventDestroy(sl.fan);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.stack) (void)hipFree(sl.stack);
  }
  delete set;
  return RAG_OK;
}

int rag_shardset_search(rag_shardset_t* set, const float* q, int B, int k, const uint32_t* filters,
                        int flags, float* out_s, int64_t* out_i, uint8_t* out_empty,
                        void* stream) {
  ragmi::clear_error();
  if (!set) return ragmi::fail(RAG_EINVAL, "shard set is NULL");
  if (k < 1) return ragmi::fail(RAG_EINVAL, "shard set search: k must be >= 1");
  if (B < 0 || (B > 0 && (!q || !out_s || !out_i)) || (flags & ~RAG_SHARDSET_FULL))
    return ragmi::fail(RAG_EINVAL, "bad shard set search args");
  if (B == 0) return RAG_OK;
  if ((int64_t)B * k > INT32_MAX)
    return ragmi::fail(RAG_ERANGE, "shard set search: B * k too large");
  DeviceGuard guard;
  std::lock_guard<std::mutex> lk(set->mu);
  const int rc = shardset_search_locked(set, q, B, k, filters, (flags & RAG_SHARDSET_FULL) != 0,
                                        out_s, out_i, out_empty, static_cast<hipStream_t>(stream));
  if (rc) {
    // a search that failed half way: let what it already started on the shard streams finish,
    // so nothing of it still writes into the slot when the next search takes it
    for (int s = 0; s < set->n; ++s) {
      (void)hipSetDevice(set->dev[s]);
      (void)hipStreamSynchronize(set->stream[s]);
    }
  }
  return rc;
}

int rag_shardset_search_view(rag_shardset_t* set, const float* q, int B, int k,
                             const uint32_t* progs, int64_t words, int n_programs,
                             const uint32_t* filters, int flags, float* out_s, int64_t* out_i,
                             uint8_t* out_empty, void* stream) {
  ragmi::clear_error();
  if (!set) return ragmi::fail(RAG_EINVAL, "shard set is NULL");
  if (const int rc = view_args(progs, words, n_programs)) return rc;
  if (k < 1) return ragmi::fail(RAG_EINVAL, "shard set search: k must be >= 1");
  if (B < 0 || (B > 0 && (!q || !out_s || !out_i)) || (flags & ~RAG_SHARDSET_FULL))
    return ragmi::fail(RAG_EINVAL, "bad shard set search args");
  if (B == 0) return RAG_OK;
  if ((int64_t)B * k > INT32_MAX)
    return ragmi::fail(RAG_ERANGE, "shard set search: B * k too large");
  DeviceGuard guard;
  std::lock_guard<std::mutex> lk(set->mu);
  const int rc = shardset_search_locked(set, q, B, k, filters, (flags & RAG_SHARDSET_FULL) != 0,
                                        out_s, out_i, out_empty, static_cast<hipStream_t>(stream),
                                        progs, words, n_programs);
  if (rc) {
    // as rag_shardset_search: what a failed search started on the shard streams finishes first
    for (int s = 0; s < set->n; ++s) {
      (void)hipSetDevice(set->dev[s]);
      (void)hipStreamSynchronize(set->stream[s]);
    }
  }
  return rc;
}

int rag_bench_scan(rag_index_t* h, const float* queries_dev, int B, int variant, int reps,
                   double* avg_ms) {
  ragmi::clear_error();
#ifndef RAGMI_DIAG_BUILD
  if (variant != 0 && (variant != 7 || (h && h->dim != 384)))
    return ragmi::fail(RAG_EINVAL, "variant: 0 (production) or 7 (dim 384: seeds at +inf); the "
                                   "scan's timing probes are in the diagnostic build only");
#endif
  if (!h || !queries_dev || B < 1 || reps < 1 || !avg_ms || variant < 0 || variant > 19)
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
  RAG_HIP(hipSetDevice(h->device));
  RAG_HIP(hipDeviceSynchronize());
  unsigned long long t1 = 0, t2 = 0;
  for (auto& w : h->ws) {
    unsigned long long c[2];
    RAG_HIP(hipMemcpy(c, w.fb_cnt, sizeof(c), hipMemcpyDeviceToHost));
    t1 += c[0];
    t2 += c[1];
  }
  *tier1 = (int64_t)t1;
  *tier2 = (int64_t)t2;
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
  RAG_HIP(hipSetDevice(h->device));
  RAG_HIP(hipDeviceSynchronize());
  unsigned long long tot = 0;
  for (auto& w : h->ws) {
    unsigned long long c[3];
    RAG_HIP(hipMemcpy(c, w.fb_cnt, sizeof(c), hipMemcpyDeviceToHost));
    tot += c[2];
  }
  *n = (int64_t)tot;
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
  if (mode < RAG_PRESCAN_OFF || mode > RAG_PRESCAN_ALWAYS)
    return ragmi::fail(RAG_EINVAL, "prescan mode must be 0 (off), 1 (auto) or 2 (always)");
  std::lock_guard<std::mutex> lk(h->mu);
  h->prescan = mode;
  return RAG_OK;
}

int rag_index_prescan(const rag_index_t* h) { return h ? h->prescan : -1; }

int rag_index_prescan_bounds(rag_index_t* h, const float* q, int B, const int64_t* rows_dev,
                             int64_t n, float* out_u) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (B < 1 || B > ragmi::kQ || !q || n < 0 || (n > 0 && (!rows_dev || !out_u)))
    return ragmi::fail(RAG_EINVAL, "bad prescan_bounds args (1 <= B <= 32)");
  if (n > 0x7fffffff) return ragmi::fail(RAG_ERANGE, "n too large for one call");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->c8)
    return ragmi::fail(RAG_EINVAL, "index keeps no int8 scan copy (dim 384, fp16 storage only)");
  if (n == 0) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  RAG_HIP(hipDeviceSynchronize());   // workspace 0 may belong to a running pass
  Workspace& w = h->ws[0];
  using namespace ragmi;
  qprep8_kernel<384><<<dim3(kQ), dim3(64), 0, nullptr>>>(q, B, nullptr, w.qn, w.qfrag, w.filt,
                                                         w.eps, w.qfrag8, w.qp8, w.eps8);
  prescan_bounds_kernel<384><<<dim3((unsigned)n), dim3(64), 0, nullptr>>>(
      h->c8, h->meta8, reinterpret_cast<const intx4*>(w.qfrag8), w.qp8, rows_dev, n, h->count, B,
      out_u);
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
  // (the stream belongs to the current device: switch to `device` for the call only)
  int prev = 0;
  RAG_HIP(hipGetDevice(&prev));
  RAG_HIP(hipSetDevice(device));
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data());
  (void)hipSetDevice(prev);
  if (e != hipSuccess)
    return ragmi::fail(RAG_EHIP, std::string("hipExtStreamCreateWithCUMask: ") + hipGetErrorString(e));
  *out = st;
  g_stream_gen.fetch_add(1, std::memory_order_acq_rel);
  return RAG_OK;
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
  int prev = 0;
  RAG_HIP(hipGetDevice(&prev));
  RAG_HIP(hipSetDevice(device));
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask);
  (void)hipSetDevice(prev);
  if (e != hipSuccess)
    return ragmi::fail(RAG_EHIP, std::string("hipExtStreamCreateWithCUMask: ") + hipGetErrorString(e));
  *out = st;
  g_stream_gen.fetch_add(1, std::memory_order_acq_rel);
  return RAG_OK;
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
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  *launches = (int64_t)h->prof_pairs.size();
  *total_ms = tot;
  h->prof_pairs.clear();
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
  for (auto& p : h->prof_pairs) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  h->prof_pairs.clear();
  *launches = n;
  return RAG_OK;
}

}  // extern "C"
