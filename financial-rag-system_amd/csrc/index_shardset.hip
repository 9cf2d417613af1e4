// index_shardset.hip — the shard set of the flat index's extern "C" boundary (declared in
// include/ragmi.h): N flat indexes searched as one (global row g on shard g % N at local row
// g / N). Host orchestration over rag_index_search* and rag_merge_topk*: no kernel header.
#include "index_host.hpp"

using namespace ragmi;

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

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

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
int set_ensure(SetSlot& sl, char** buf, size_t* have, size_t bytes) {
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
int shardset_search_locked(rag_shardset* set, const float* q, int B, int k, const uint32_t* filt,
                           bool full, float* out_s, int64_t* out_i, uint8_t* out_empty,
                           hipStream_t st, const uint32_t* progs, int64_t words, int n_programs) {
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
    rc = remap_shard_ids(reinterpret_cast<int64_t*>(sl.stack + ids_off), B, k, n, out_empty, st);
    if (rc) return rc;
    rc = rag_merge_topk(reinterpret_cast<const float*>(sl.stack),
                        reinterpret_cast<const int64_t*>(sl.stack + ids_off), n, B, k, out_s,
                        out_i, st);
  }
  if (rc) return rc;
  RAG_HIP(hipEventRecord(sl.done, st));
  return RAG_OK;
}

// rag_shardset_search (view false: progs unused) and rag_shardset_search_view
int shardset_search(rag_shardset* set, const float* q, int B, int k, bool view,
                    const uint32_t* progs, int64_t words, int n_programs, const uint32_t* filters,
                    int flags, float* out_s, int64_t* out_i, uint8_t* out_empty, void* stream) {
  ragmi::clear_error();
  if (!set) return ragmi::fail(RAG_EINVAL, "shard set is NULL");
  if (view)
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
    // a search that failed half way: let what it already started on the shard streams finish,
    // so nothing of it still writes into the slot when the next search takes it
    for (int s = 0; s < set->n; ++s) {
      (void)hipSetDevice(set->dev[s]);
      (void)hipStreamSynchronize(set->stream[s]);
    }
  }
  return rc;
}

}  // namespace

extern "C" {

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
  return shardset_search(set, q, B, k, false, nullptr, 0, 0, filters, flags, out_s, out_i,
                         out_empty, stream);
}

int rag_shardset_search_view(rag_shardset_t* set, const float* q, int B, int k,
                             const uint32_t* progs, int64_t words, int n_programs,
                             const uint32_t* filters, int flags, float* out_s, int64_t* out_i,
                             uint8_t* out_empty, void* stream) {
  return shardset_search(set, q, B, k, true, progs, words, n_programs, filters, flags, out_s,
                         out_i, out_empty, stream);
}

}  // extern "C"
