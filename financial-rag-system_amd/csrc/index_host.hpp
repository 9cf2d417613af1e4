// index_host.hpp — what the index's host units share: the handle and its
// workspace ring, the dispatch and scope helpers, the functions that cross a unit boundary.
// Host code only: every definition is a type, a template or inline.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common_host.hpp"
#include "device_common.hpp"   // half8, launch_fixed

namespace ragmi {

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
  // tier 1 spread over the chip after the 6-bit prescan (certify_kernels.hip band_kernel): the
  // head's per-query records [32][kBandRec], the slices' lists [32][kBandSlicesMax][kBandPub] and
  // the per-query arrival tickets [32] (zero between passes)
  int* bd_rec = nullptr;
  int* bd_pub = nullptr;
  int* bd_tk = nullptr;
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
  // recommend passes (reco_kernels.hip), allocated on first use: the request's [32][1024] query
  // block followed by AVERAGE_VECTOR's target [1024], and the request's parameters / the last
  // hot pass's counters (kRecoPar*)
  float* reco_q = nullptr;
  float* reco_par = nullptr;
  // sparse searches (sparse_kernels.hip), allocated on first use: the pass's query table
  // (kSpTabWords words)
  uint32_t* sp_tab = nullptr;
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
// decltype(tag)::value (the idiom of bert_capi.hip): a flag as a bool_constant,
// `filt != nullptr` as one ...
template <typename F>
auto with_flag(bool on, F&& f) {
  if (on) return f(std::bool_constant<true>{});
  return f(std::bool_constant<false>{});
}
template <typename F>
auto with_filter(const uint32_t* filt, F&& f) {
  return with_flag(filt != nullptr, static_cast<F&&>(f));
}

// ... and the handle's dim as an integral_constant; the lambda returns the status
template <typename F>
int with_dim(int dim, F&& f) {
  if (dim == 384) return f(std::integral_constant<int, 384>{});
  if (dim == 1024) return f(std::integral_constant<int, 1024>{});
  return fail(RAG_EINVAL, "unsupported dim (built: 384, 1024)");
}

// The scan copies an index may keep beside its fp16 rows (dim 384, fp16 storage; prep_kernels.hip
// "int8 scan copy", "6-bit scan copy"), and the copy a search pass streams (kNoCopy: the fp16
// rows themselves). A copy is its image and its per-row (scale, error) meta, both over
// cap_rows / 16 + 1 tiles (the prescans walk tile pairs; the 6-bit image holds whole pairs)
enum CopyKind : int { kNoCopy = -1, kCopy8 = 0, kCopy6 = 1 };
constexpr int kCopies = 2;
struct ScanCopy {
  char* data = nullptr;
  float* meta = nullptr;
};

// ... and a copy kind as its device format (prep_kernels.hip Copy8 / Copy6), read by the lambda
// as typename decltype(c)::type
struct Copy8;
struct Copy6;
template <typename T>
struct type_tag {
  using type = T;
};
template <typename F>
auto with_copy(CopyKind kind, F&& f) {
  if (kind == kCopy6) return f(type_tag<Copy6>{});
  return f(type_tag<Copy8>{});
}

// The slot (Workspace, ViewSlot, SetSlot) a call on stream `st` takes: the one bound to `st`,
// else the first unused one. Neither: nullptr, every slot being bound to another stream whose
// last call may still be running; `lru` is the least recently used one, for the caller to wait
// for and rebind.
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

inline int64_t round16(int64_t n) { return (n + 15) & ~int64_t(15); }

// the 1-D grid of a launch with one thread (or one group of threads) per item
inline dim3 grid1d(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

}  // namespace ragmi

struct rag_index {
  int dim = 0;
  bool diagnostic = false;   // counted in ragmi::diagnostic_handles() (common_host.hpp)
  int device = 0;
  int64_t cap_rows = 0;   // multiple of 16
  int64_t count = 0;
  ragmi::half8* corpus = nullptr;
  uint32_t* tags = nullptr;
  // key columns (rag_index_keys_create; rows_kernels.hip): n_keys int64 columns of cap_rows
  // keys, the tag array's extent; entries at or past n_keys are nullptr
  int64_t* keys[RAG_KEYS_MAX_COLS] = {};
  int n_keys = 0;
  // sparse column (rag_index_sparse_create; sparse_kernels.hip): sp_slots slots per row, terms
  // uint16 [cap_rows][sp_slots] and values fp32 alike; nullptr / 0 in an index without one
  uint16_t* sp_terms = nullptr;
  float* sp_vals = nullptr;
  int sp_slots = 0;
  // storage (rag_index_create_ex): RAG_STORE_FP16 keeps only the scan's fp16 tile16 rows;
  // RAG_STORE_FP32 also the normalised fp32 rows (row-major [cap][dim]), which the exact
  // rescoring reads — Qdrant's default Float32 datatype
  int storage = RAG_STORE_FP16;
  float* rows32 = nullptr;
  // scan copies, by CopyKind: the int8 one wherever the index can keep one (dim 384, fp16
  // storage), the 6-bit one only where it is used: capacity at least RAG_PRESCAN6_MIN_ROWS, or
  // mode RAG_PRESCAN_ALWAYS6 set (ensure_copy6). Every copy kept is rebuilt from the stored fp16
  // rows after every write of `corpus` (requant)
  ragmi::ScanCopy copy[ragmi::kCopies];
  int prescan = 1;        // rag_index_set_prescan: 0 off, 1 auto, 2 always (int8), 3 always 6-bit
  // passes that streamed each copy (rag_index_prescan_passes: their sum; _prescan6_passes)
  int64_t copy_passes[ragmi::kCopies] = {};
  // recommend passes since creation by path, and the workspace of the last hot one
  // (rag_index_reco_stats)
  int64_t reco_hot = 0, reco_full = 0;
  ragmi::Workspace* reco_last = nullptr;
  // the same for discover / context passes (rag_index_discover_stats): counters of their own
  int64_t disc_hot = 0, disc_full = 0;
  ragmi::Workspace* disc_last = nullptr;
  int n_cu = 256;
  int max_wgs = 0;        // scan workgroups at full occupancy
  int scan_wgs = 0;       // D <= 384 scan grid cap: 3/4 of the CUs (scan_grid)
  int groups = 1;         // query groups of 32 per search pass
  std::mutex mu;
  ragmi::Workspace ws[ragmi::kRing];
  uint64_t ws_tick = 0;
  ragmi::ViewSlot views[ragmi::kRing];   // filter view columns, allocated on first use per stream
  uint64_t view_tick = 0;
  ragmi::Workspace* last_ws = nullptr;   // workspace of the most recent search pass
  int last_bq = 0;                       // its query count
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
  std::vector<ragmi::ProfPair> prof_pairs;
};

namespace ragmi {

// the one drain of prof_pairs: destroys the timed scan launches' event pairs recorded so far
inline void drop_prof_pairs(rag_index* h) {
  for (auto& p : h->prof_pairs) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  h->prof_pairs.clear();
}

// host staging of the *_host / import / export entry points, grown on demand
inline int ensure_stage(rag_index* h, size_t bytes) {
  if (h->stage_bytes >= bytes) return RAG_OK;
  if (h->stage) (void)hipFree(h->stage);
  h->stage = nullptr;
  h->stage_bytes = 0;
  RAG_HIP(hipMalloc(&h->stage, bytes));
  h->stage_bytes = bytes;
  return RAG_OK;
}

// ---- functions that cross a unit boundary (not in the library's dynamic symbols) ----
#pragma GCC visibility push(hidden)
// index_search.hip: a new handle's workspaces (dim, groups, max_wgs, copies set), one hipMalloc per
// buffer in the tables' order; their release; the shard set's id remap (remap_ids_kernel)
// ... the sparse column of an index that has one (lock held): its rows moved with their dense
// rows on `st` (rag_index_move_rows), regrown to `cap` rows with the old rows kept and the new
// ones empty (rag_index_reserve, before cap_rows changes; synchronous)
int sparse_move_rows(rag_index* h, const int64_t* src_rows, const int64_t* dst_rows, int64_t n,
                     hipStream_t st);
int sparse_reserve(rag_index* h, int64_t cap);
hipError_t alloc_workspaces(rag_index* h);
void free_workspaces(rag_index* h);
int remap_shard_ids(int64_t* ids, int B, int k, int n, uint8_t* out_empty, hipStream_t st);
// index_store.hip: the blob rules of every *_view entry point, checked before any HIP call; the
// view column of a call on `st`; filter_view_kernel over the handle's rows into it (lock held)
int view_args(const uint32_t* progs, int64_t words, int n_programs);
int acquire_view(rag_index* h, hipStream_t st, uint32_t** view);
int launch_filter_view(rag_index* h, const uint32_t* progs, int64_t words, int n_programs,
                       uint32_t* view, hipStream_t st);
// index_store.hip: the 6-bit scan copy of an index that can keep one (dim 384, fp16 storage) and
// has none yet, allocated and built from the stored rows; synchronous (lock held)
int ensure_copy6(rag_index* h);
#pragma GCC visibility pop

}  // namespace ragmi
