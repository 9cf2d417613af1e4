// index_store.hip — the storage side of the flat index's extern "C" boundary (declared in
// include/ragmi.h): handle lifetime and capacity growth, upsert / import / export, row movement
// (select, move, gather, scatter), key columns and filter views, order_rows and facet_counts.
#include "index_host.hpp"
// prep_kernels.hip for upsert_kernel / requant_kernel: all templates or inlined, so two units
#include "prep_kernels.hip"
#include "rows_kernels.hip"
#include "order_kernels.hip"
#include "filter_kernels.hip"

using namespace ragmi;

namespace {

// Which indexes keep scan copies: the int8 one always, the 6-bit one from its threshold
bool keeps_copy8(const rag_index* h) { return h->dim == 384 && h->storage == RAG_STORE_FP16; }

// Image bytes of `tiles` tiles of a copy: dim / 64 KiB a tile for the int8 one; whole pairs of
// tiles for the 6-bit one (an odd last tile's pair counts with its spare half)
size_t tiles_bytes(CopyKind kind, int dim, int64_t tiles) {
  return kind == kCopy6 ? (size_t)((tiles + 1) / 2) * ragmi::kPair6Bytes
                        : (size_t)tiles * (dim / 64) * 1024;
}
// a copy's image over cap_rows / 16 + 1 tiles (one spare: the prescans walk tile pairs), its meta
size_t copy_bytes(CopyKind kind, int dim, int64_t cap_rows) {
  return tiles_bytes(kind, dim, cap_rows / 16 + 1);
}
size_t meta_bytes(int64_t cap_rows) { return (size_t)(cap_rows / 16 + 1) * 32 * 4; }

// a copy's two buffers before the handle owns them (freed on every error return)
struct CopyBufs {
  DeviceBuf<char> data;
  DeviceBuf<float> meta;
};

// the buffers of copy `kind` for `cap_rows` rows, zeroed
int alloc_copy(CopyKind kind, int dim, int64_t cap_rows, CopyBufs& b) {
  if (b.data.alloc(copy_bytes(kind, dim, cap_rows)) != hipSuccess ||
      b.meta.alloc(meta_bytes(cap_rows)) != hipSuccess)
    return ragmi::fail(RAG_ENOMEM, kind == kCopy6 ? "hipMalloc(6-bit scan copy) failed"
                                                  : "hipMalloc(int8 scan copy) failed");
  RAG_HIP(hipMemset(b.data.p, 0, copy_bytes(kind, dim, cap_rows)));
  RAG_HIP(hipMemset(b.meta.p, 0, meta_bytes(cap_rows)));
  return RAG_OK;
}

// The handle takes `nb` as its copy `kind`. What the copy held so far moves over first (reserve):
// whole tiles of the old capacity, whose spare tile holds no row; for the 6-bit copy whole pairs,
// an odd last tile's with its spare half. A copy that starts here holds no row yet.
int grow_copy(rag_index* h, CopyKind kind, CopyBufs& nb) {
  ScanCopy& c = h->copy[kind];
  if (c.data) {
    const int64_t tiles = h->cap_rows / 16;
    RAG_HIP(hipMemcpy(nb.data.p, c.data, tiles_bytes(kind, h->dim, tiles),
                      hipMemcpyDeviceToDevice));
    RAG_HIP(hipMemcpy(nb.meta.p, c.meta, (size_t)tiles * 32 * 4, hipMemcpyDeviceToDevice));
    (void)hipFree(c.data);
    (void)hipFree(c.meta);
  }
  c.data = nb.data.release();
  c.meta = nb.meta.release();
  return RAG_OK;
}

// copy `kind` of an index that has none, over its present capacity (creation, ensure_copy6;
// reserve runs the same two steps around its own allocations)
int start_copy(rag_index* h, CopyKind kind) {
  CopyBufs b;
  const int rc = alloc_copy(kind, h->dim, h->cap_rows, b);
  return rc ? rc : grow_copy(h, kind, b);
}

// requant_kernel in the format of copy `kind`, over rows[i] or row0 + i, i < n
void launch_requant(const rag_index* h, CopyKind kind, const int64_t* rows, int64_t row0,
                    int64_t n, hipStream_t st) {
  with_copy(kind, [&](auto c) {
    ragmi::requant_kernel<384, typename decltype(c)::type><<<dim3((unsigned)n), dim3(64), 0, st>>>(
        h->corpus, rows, row0, n, h->cap_rows, h->copy[kind].data, h->copy[kind].meta);
  });
}

// The scan copies of rows[i] (device list) or row0 + i, i < n, rebuilt from the stored fp16
// rows: enqueued on `st` right after the kernel that wrote them
int requant(rag_index* h, const int64_t* rows, int64_t row0, int64_t n, hipStream_t st) {
  if (!h->copy[kCopy8].data || n <= 0) return RAG_OK;
  for (int k = 0; k < kCopies; ++k)
    if (h->copy[k].data) launch_requant(h, (CopyKind)k, rows, row0, n, st);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// a whole copy from the stored rows (a copy that starts late: reserve, ensure_copy6); synchronous
int rebuild_copy(rag_index* h, CopyKind kind) {
  if (h->count > 0) launch_requant(h, kind, nullptr, 0, h->count, nullptr);
  RAG_HIP(hipGetLastError());
  RAG_HIP(hipDeviceSynchronize());
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

// One element of an imported row as fp64, exact; false for a non-finite one. fp16 by its
// exponent bits (no float conversion of an inf or NaN): (h & 0x7fff) << 13 read as fp32 is the
// value scaled by 2^-112, normal or subnormal.
inline bool import_value(uint16_t h, double& v) {
  if ((h & 0x7c00u) == 0x7c00u) return false;
  const uint32_t u = (uint32_t)(h & 0x7fffu) << 13;
  float f;
  std::memcpy(&f, &u, 4);
  v = (double)(f * 0x1p112f);   // the sign does not enter the norm
  return true;
}
inline bool import_value(float x, double& v) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return false;
  v = (double)x;
  return true;
}

// The rows an import may write: every element finite and the fp64 L2 norm at most kRowNorm, what
// every certificate assumes of a stored row (device_common.hpp). The first row that is neither is
// named in the error; nothing has been copied by then.
template <typename T>
int check_import_rows(const T* rows, int64_t row0, int64_t n, int dim) {
  for (int64_t r = 0; r < n; ++r) {
    const T* x = rows + r * dim;
    double s = 0.0;
    for (int k = 0; k < dim; ++k) {
      double v;
      if (!import_value(x[k], v))
        return ragmi::fail(RAG_EINVAL, "import: row " + std::to_string(row0 + r) +
                                           " holds a non-finite element (index " +
                                           std::to_string(k) + ")");
      s += v * v;
    }
    const double norm = std::sqrt(s);
    if (norm > ragmi::kRowNorm)
      return ragmi::fail(RAG_EINVAL, "import: row " + std::to_string(row0 + r) + " has norm " +
                                         std::to_string(norm) + " > " +
                                         std::to_string(ragmi::kRowNorm) +
                                         ": not a stored (normalised) row");
  }
  return RAG_OK;
}

// rag_index_import_rows (T = uint16_t: fp16 rows into an fp16-storage index) and
// rag_index_import_rows32 (T = float: fp32 rows into an fp32-storage index, the scan's fp16
// copy derived on the device): checked on the host (check_import_rows), then staged through
// device memory, synchronous
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
  if (const int rc = check_import_rows(rows, row0, n, h->dim)) return rc;
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
      const dim3 grid = grid1d(n * (D / 8), 256);
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
    ragmi::fill_keys_kernel<<<grid1d(cap - keep, kKeyBlock), dim3(kKeyBlock), 0, nullptr>>>(
        out.p, keep, cap);
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
      ragmi::copy_rows_kernel<decltype(d)::value, MODE>
          <<<grid1d(n, kRowsGroup), dim3(ragmi::kRowsBlock), 0, st>>>(
              h->corpus, h->rows32, h->tags, src_rows, dst_rows, n, h->cap_rows, pk16, pk32,
              pktags);
      return RAG_OK;
    });
    if (rc) return rc;
    RAG_HIP(hipGetLastError());
    if constexpr (MODE == ragmi::kRowsMove)
      if (h->n_keys > 0) {   // the keys are a stored form of the row: they move with it
        ragmi::move_keys_kernel<<<grid1d(n, kKeyBlock), dim3(ragmi::kKeyBlock), 0, st>>>(
            key_cols(h), h->n_keys, src_rows, dst_rows, n, h->cap_rows);
        RAG_HIP(hipGetLastError());
      }
    if constexpr (MODE == ragmi::kRowsMove)
      if (h->sp_slots > 0)   // and so is the sparse row
        if (const int rs = ragmi::sparse_move_rows(h, src_rows, dst_rows, n, st)) return rs;
    if constexpr (MODE != ragmi::kRowsGather)   // move / scatter wrote the rows dst_rows
      if (const int rq = requant(h, dst_rows, 0, n, st)) return rq;
  }
  if (new_count >= 0) h->count = new_count;
  return RAG_OK;
}

// move / scatter set the count: a negative one is refused before copy_rows's checks
int negative_count(const rag_index* h) {
  ragmi::clear_error();
  return ragmi::fail(h ? RAG_ERANGE : RAG_EINVAL, h ? "new_count is negative" : "index is NULL");
}

// the ordered select (count / prefix sum / emit) over tag column `tags` of the rows
// [row0, h->count): the chunks from row0's on
int select_locked(rag_index* h, const uint32_t* tags, uint32_t tag_mask, uint32_t tag_value,
                  int64_t row0, int64_t* out_rows, int64_t cap, int64_t* out_n, hipStream_t st) {
  const int64_t count = h->count;
  const int nb = row0 >= count ? 0
                               : (int)((count + ragmi::kSelChunk - 1) / ragmi::kSelChunk -
                                       row0 / ragmi::kSelChunk);
  if (nb == 0) {
    RAG_HIP(hipMemsetAsync(out_n, 0, sizeof(int64_t), st));
    return RAG_OK;
  }
  StreamScratch offsets(st);   // matches per chunk, then their exclusive prefix sums
  RAG_HIP(offsets.alloc((size_t)nb * sizeof(int64_t)));
  int64_t* const off = reinterpret_cast<int64_t*>(offsets.p);
  ragmi::select_count_kernel<<<dim3((unsigned)nb), dim3(ragmi::kSelBlock), 0, st>>>(
      tags, row0, count, tag_mask, tag_value, off);
  ragmi::select_scan_kernel<<<dim3(1), dim3(ragmi::kSelScanBlock), 0, st>>>(off, nb, out_n);
  if (cap > 0)
    ragmi::select_emit_kernel<<<dim3((unsigned)nb), dim3(ragmi::kSelBlock), 0, st>>>(
        tags, row0, count, tag_mask, tag_value, off, out_rows, cap);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

// rag_index_select_rows, and (view) rag_index_select_rows_view / rag_index_select_rows_from over
// a one-program filter view, from row `row0` on
int select_rows(rag_index* h, const uint32_t* progs, int64_t words, bool view, uint32_t tag_mask,
                uint32_t tag_value, int64_t row0, int64_t* out_rows, int64_t cap, int64_t* out_n,
                void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "index is NULL");
  if (view)
    if (const int rc = view_args(progs, words, 1)) return rc;
  if (row0 < 0) return ragmi::fail(RAG_EINVAL, "select: row0 is negative");
  if (!out_n || cap < 0 || (cap > 0 && !out_rows))
    return ragmi::fail(RAG_EINVAL, "bad select args (out_n NULL, or cap > 0 without out_rows)");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  uint32_t* v = h->tags;
  if (view) {
    if (const int rc = acquire_view(h, st, &v)) return rc;
    if (const int rc = launch_filter_view(h, progs, words, 1, v, st)) return rc;
  }
  return select_locked(h, v, tag_mask, tag_value, row0, out_rows, cap, out_n, st);
}

// rag_index_write_keys / rag_index_gather_keys: the shared argument checks, the column check
// under the lock, then launch(column, grid, stream) of the one kernel that differs
template <typename F>
int keys_call(rag_index* h, int col, const int64_t* rows, const void* other, int64_t n,
              void* stream, F&& launch) {
  ragmi::clear_error();
  if (n < 0) return ragmi::fail(RAG_EINVAL, "keys: n must be >= 0");
  if (n > 0 && (!rows || !other)) return ragmi::fail(RAG_EINVAL, "keys: a NULL rows or keys pointer");
  if (!h) return ragmi::fail(RAG_EINVAL, "keys: index is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  if (col < 0 || col >= h->n_keys)
    return ragmi::fail(RAG_ERANGE, "keys: no such column (call rag_index_keys_create)");
  if (n == 0) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  launch(h->keys[col], grid1d(n, kKeyBlock), static_cast<hipStream_t>(stream));
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

}  // namespace

// ---- filter views (filter_kernels.hip; declared in index_host.hpp) ----

int ragmi::view_args(const uint32_t* progs, int64_t words, int n_programs) {
  if (!progs) return ragmi::fail(RAG_EINVAL, "filter view: the program blob is NULL");
  if (n_programs < 1 || n_programs > RAG_FILTER_MAX_PROGRAMS)
    return ragmi::fail(RAG_EINVAL, "filter view: n_programs must be in [1, RAG_FILTER_MAX_PROGRAMS=32]");
  if (words < (int64_t)n_programs * RAG_FILTER_REC_WORDS || words > UINT32_MAX)
    return ragmi::fail(RAG_EINVAL, "filter view: `words` is smaller than n_programs records of 41 "
                                   "words (or not below 2^32)");
  return RAG_OK;
}

// filter_view_kernel over the handle's cap_rows rows into `view` (>= cap_rows words)
int ragmi::launch_filter_view(rag_index* h, const uint32_t* progs, int64_t words, int n_programs,
                              uint32_t* view, hipStream_t st) {
  if (h->cap_rows == 0) return RAG_OK;
  const int64_t chunks = (h->cap_rows + kFvBlock * 4 - 1) / (kFvBlock * 4);
  const dim3 grid((unsigned)std::min<int64_t>(chunks, (int64_t)kFvWgPerCu * h->n_cu));
  // an index with key columns: the instantiations that know the RANGE atom (one more word of
  // LDS, the mask of the columns the blob names); without columns, the kernel as it always was
  const bool pool = words <= kFvLdsWords;
  const size_t lds = (pool ? (size_t)words : (size_t)n_programs * RAG_FILTER_REC_WORDS) * 4;
  const KeyCols kc = key_cols(h);
  with_flag(pool, [&](auto pool_lds) {
    with_flag(h->n_keys > 0, [&](auto with_keys) {
      constexpr bool P = decltype(pool_lds)::value, K = decltype(with_keys)::value;
      filter_view_kernel<P, K><<<grid, dim3(kFvBlock), lds + (K ? 4 : 0), st>>>(
          h->tags, h->count, h->cap_rows, progs, (uint32_t)words, n_programs, view, kc, h->n_keys);
    });
  });
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
int ragmi::acquire_view(rag_index* h, hipStream_t st, uint32_t** view) {
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

int ragmi::ensure_copy6(rag_index* h) {
  if (h->copy[kCopy6].data || !keeps_copy8(h)) return RAG_OK;
  RAG_HIP(hipSetDevice(h->device));
  RAG_HIP(hipDeviceSynchronize());   // no writer of the rows in flight
  const int rc = start_copy(h, kCopy6);
  return rc ? rc : rebuild_copy(h, kCopy6);
}

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
    rc = start_copy(h, kCopy8);
    if (!rc && h->cap_rows >= RAG_PRESCAN6_MIN_ROWS) rc = start_copy(h, kCopy6);
    if (rc) {
      rag_index_destroy(h);
      return rc;
    }
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
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      n_cu <= 0)
    n_cu = 256;
  h->n_cu = n_cu;
  h->max_wgs = n_cu * 2;  // 2 x 256-thread workgroups per CU (__launch_bounds__(256, 2))
  h->scan_wgs = std::max(8, (n_cu * 3 / 4) & ~7);
  // wide rows (LDS-query scan) take up to 4 query groups (128 queries) per pass
  h->groups = dim > 384 ? kMaxGroups : 1;
  if (alloc_workspaces(h) != hipSuccess) {
    rag_index_destroy(h);
    return ragmi::fail(RAG_ENOMEM, "workspace allocation failed");
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
  free_workspaces(h);
  drop_prof_pairs(h);
  if (h->scan_done) (void)hipEventDestroy(h->scan_done);
  if (h->scan_stream) (void)hipStreamDestroy(h->scan_stream);
  if (h->corpus) (void)hipFree(h->corpus);
  if (h->tags) (void)hipFree(h->tags);
  for (auto* k : h->keys)
    if (k) (void)hipFree(k);
  if (h->sp_terms) (void)hipFree(h->sp_terms);
  if (h->sp_vals) (void)hipFree(h->sp_vals);
  if (h->rows32) (void)hipFree(h->rows32);
  for (auto& c : h->copy) {
    if (c.data) (void)hipFree(c.data);
    if (c.meta) (void)hipFree(c.meta);
  }
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
  // every copy the index keeps grows with the rest, and the 6-bit one starts here when the
  // capacity reaches its threshold
  CopyBufs ncopy[kCopies];
  const bool start6 =
      !h->copy[kCopy6].data && keeps_copy8(h) && cap >= RAG_PRESCAN6_MIN_ROWS;
  for (int k = 0; k < kCopies; ++k)
    if (h->copy[k].data || (k == kCopy6 && start6))
      if ((rc = alloc_copy((CopyKind)k, h->dim, cap, ncopy[k]))) return rc;
  RAG_HIP(hipDeviceSynchronize());
  // the key columns regrow with the tags: old rows keep their keys, new rows hold ABSENT
  DeviceBuf<int64_t> nk[RAG_KEYS_MAX_COLS];
  for (int c = 0; c < h->n_keys; ++c)
    if ((rc = alloc_keys(cap, h->keys[c], h->cap_rows, nk[c]))) return rc;
  if (h->n_keys > 0) RAG_HIP(hipDeviceSynchronize());
  // the sparse column regrows too: old rows keep their slots, new rows are empty
  if (h->sp_slots > 0)
    if ((rc = ragmi::sparse_reserve(h, cap))) return rc;
  RAG_HIP(hipMemcpy(nc.p, h->corpus, (size_t)h->cap_rows * h->dim * 2, hipMemcpyDeviceToDevice));
  RAG_HIP(hipMemcpy(nt.p, h->tags, (size_t)h->cap_rows * 4, hipMemcpyDeviceToDevice));
  if (n32.p)
    RAG_HIP(hipMemcpy(n32.p, h->rows32, (size_t)h->cap_rows * h->dim * 4,
                      hipMemcpyDeviceToDevice));
  for (int k = 0; k < kCopies; ++k)
    if (ncopy[k].data.p)
      if ((rc = grow_copy(h, (CopyKind)k, ncopy[k]))) return rc;
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
  if (start6) return rebuild_copy(h, kCopy6);   // built from the rows just moved
  return RAG_OK;
}

int64_t rag_index_capacity(const rag_index_t* h) { return h ? h->cap_rows : -1; }
int64_t rag_index_count(const rag_index_t* h) { return h ? h->count : -1; }
int rag_index_dim(const rag_index_t* h) { return h ? h->dim : -1; }
int rag_index_storage(const rag_index_t* h) { return h ? h->storage : -1; }

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

int rag_index_export_rows(rag_index_t* h, int64_t row0, int64_t n, uint16_t* out) {
  return export_range(h, out, row0, n, false, [&]() -> int {
    const size_t bytes = (size_t)n * h->dim * 2;
    int rc = ensure_stage(h, bytes);
    if (rc) return rc;
    RAG_HIP(hipDeviceSynchronize());
    rc = with_dim(h->dim, [&](auto d) {
      constexpr int D = decltype(d)::value;
      ragmi::export_kernel<D><<<grid1d(n * (D / 8), 256), dim3(256), 0, nullptr>>>(
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

int rag_index_select_rows(rag_index_t* h, uint32_t tag_mask, uint32_t tag_value,
                          int64_t* out_rows, int64_t cap, int64_t* out_n, void* stream) {
  return select_rows(h, nullptr, 0, false, tag_mask, tag_value, 0, out_rows, cap, out_n, stream);
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

int rag_index_select_rows_view(rag_index_t* h, const uint32_t* progs, int64_t words,
                               int64_t* out_rows, int64_t cap, int64_t* out_n, void* stream) {
  return select_rows(h, progs, words, true, 1u, 1u, 0, out_rows, cap, out_n, stream);
}

int rag_index_select_rows_from(rag_index_t* h, const uint32_t* progs, int64_t words, int64_t row0,
                               int64_t* out_rows, int64_t cap, int64_t* out_n, void* stream) {
  if (!progs)   // every row: the (0, 0) select over the stored tags
    return select_rows(h, nullptr, 0, false, 0u, 0u, row0, out_rows, cap, out_n, stream);
  return select_rows(h, progs, words, true, 1u, 1u, row0, out_rows, cap, out_n, stream);
}

int rag_index_move_rows(rag_index_t* h, const int64_t* src_rows, const int64_t* dst_rows,
                        int64_t n, int64_t new_count, void* stream) {
  if (new_count < 0) return negative_count(h);
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
  if (new_count < 0) return negative_count(h);
  return copy_rows<ragmi::kRowsScatter>(
      h, nullptr, rows, n, reinterpret_cast<half8*>(const_cast<uint16_t*>(in_f16)),
      const_cast<float*>(in_f32), const_cast<uint32_t*>(in_tags), new_count, stream);
}

// ---- grouped search: tag gather (rows_kernels.hip) ----

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
  ragmi::gather_tags_kernel<<<grid1d(n, kTagBlock), dim3(ragmi::kTagBlock), 0, st>>>(
      h->tags, rows, n, h->cap_rows, out_tags);
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

int rag_index_write_keys(rag_index_t* h, int col, const int64_t* rows, const int64_t* keys,
                         int64_t n, void* stream) {
  return keys_call(h, col, rows, keys, n, stream, [&](int64_t* column, dim3 grid, hipStream_t st) {
    ragmi::write_keys_kernel<<<grid, dim3(ragmi::kKeyBlock), 0, st>>>(column, rows, keys, n,
                                                                       h->cap_rows);
  });
}

int rag_index_gather_keys(rag_index_t* h, int col, const int64_t* rows, int64_t n,
                          int64_t* out_keys, void* stream) {
  return keys_call(h, col, rows, out_keys, n, stream,
                   [&](int64_t* column, dim3 grid, hipStream_t st) {
    ragmi::gather_keys_kernel<<<grid, dim3(ragmi::kKeyBlock), 0, st>>>(column, rows, n,
                                                                        h->cap_rows, out_keys);
  });
}

// ---- order_by and facet (order_kernels.hip) ----

int rag_index_order_rows(rag_index_t* h, const uint32_t* progs, int64_t words, int col, int flags,
                         int64_t lo, int64_t hi, int limit, int64_t* out_keys, int64_t* out_rows,
                         int64_t* out_n, void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "order_rows: index is NULL");
  if (!out_keys || !out_rows || !out_n)
    return ragmi::fail(RAG_EINVAL, "order_rows: a NULL output pointer");
  if (limit < 1 || limit > RAG_ORDER_MAX)
    return ragmi::fail(RAG_ERANGE, "order_rows: limit must be in [1, RAG_ORDER_MAX=4096]");
  if (progs)
    if (const int rc = view_args(progs, words, 1)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  if (col < 0 || col >= h->n_keys)
    return ragmi::fail(RAG_ERANGE, "order_rows: no such column (call rag_index_keys_create)");
  RAG_HIP(hipSetDevice(h->device));
  uint32_t* view = nullptr;
  if (progs) {
    if (const int rc = acquire_view(h, st, &view)) return rc;
    if (const int rc = launch_filter_view(h, progs, words, 1, view, st)) return rc;
  }
  int n2 = 1;
  while (n2 < limit) n2 <<= 1;
  const uint32_t desc = (flags & RAG_ORDER_DESC) ? 1u : 0u;
  const int64_t count = h->count;
  const int nb = (int)((count + kSelChunk - 1) / kSelChunk);
  if (nb == 0) {   // nothing to rank: the sort pads the whole list
    RAG_HIP(hipMemsetAsync(out_n, 0, 2 * sizeof(int64_t), st));
  } else {
    // scratch: the passes' counters, the states, the total below the threshold, then per chunk
    // the rows below the threshold and the rows of its rank
    constexpr size_t kHist = (size_t)kOrdPasses * 256 * sizeof(u64);
    constexpr size_t kState = (size_t)(kOrdPasses + 1) * sizeof(OrderState);
    constexpr size_t kHead = kHist + kState + 2 * sizeof(int64_t);
    StreamScratch scratch(st);
    RAG_HIP(scratch.alloc(kHead + 2 * (size_t)nb * sizeof(int64_t)));
    RAG_HIP(hipMemsetAsync(scratch.p, 0, kHead, st));
    u64* const hist = reinterpret_cast<u64*>(scratch.p);
    OrderState* const state = reinterpret_cast<OrderState*>(scratch.p + kHist);
    int64_t* const tot = reinterpret_cast<int64_t*>(scratch.p + kHist + kState);
    int64_t* const less = tot + 2;
    int64_t* const eq = less + nb;
    const OrderArgs a{view, h->keys[col], count, lo, hi, desc};
    const int64_t steps = (count + kOrdRows - 1) / kOrdRows;
    const dim3 grid((unsigned)std::min<int64_t>(steps, (int64_t)kOrdWgPerCu * h->n_cu));
    for (int p = 0; p < kOrdPasses; ++p)
      order_hist_kernel<<<grid, dim3(kOrdBlock), 0, st>>>(a, p, limit, hist, state);
    order_count_kernel<<<dim3((unsigned)nb), dim3(kOrdBlock), 0, st>>>(a, limit, hist, state, less,
                                                                      eq);
    order_scan_kernel<<<dim3(1), dim3(kSelScanBlock), 0, st>>>(less, eq, nb, hist, state, tot,
                                                               out_n);
    order_emit_kernel<<<dim3((unsigned)nb), dim3(kOrdBlock), 0, st>>>(a, limit, state, less, eq,
                                                                     tot, out_keys, out_rows);
    RAG_HIP(hipGetLastError());
  }
  order_sort_kernel<<<dim3(1), dim3(kOrdSortBlock), (size_t)n2 * 16, st>>>(out_keys, out_rows,
                                                                         out_n, limit, n2, desc);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

int rag_index_facet_counts(rag_index_t* h, const uint32_t* progs, int64_t words, int field,
                           int n_codes, int64_t* out_counts, void* stream) {
  ragmi::clear_error();
  if (!h) return ragmi::fail(RAG_EINVAL, "facet_counts: index is NULL");
  if (!out_counts) return ragmi::fail(RAG_EINVAL, "facet_counts: the output pointer is NULL");
  if (field < 0 || field > 1)
    return ragmi::fail(RAG_ERANGE, "facet_counts: field must be 0 or 1");
  if (n_codes < 0 || n_codes > 65535)
    return ragmi::fail(RAG_ERANGE, "facet_counts: n_codes must be in [0, 65535]");
  if (progs)
    if (const int rc = view_args(progs, words, 1)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(h->mu);
  RAG_HIP(hipSetDevice(h->device));
  uint32_t* view = nullptr;
  if (progs) {
    if (const int rc = acquire_view(h, st, &view)) return rc;
    if (const int rc = launch_filter_view(h, progs, words, 1, view, st)) return rc;
  }
  const size_t bins = (size_t)n_codes + 1;
  RAG_HIP(hipMemsetAsync(out_counts, 0, bins * sizeof(int64_t), st));
  const int64_t count = h->count;
  if (count == 0) return RAG_OK;
  const int64_t steps = (count + kFacetChunk - 1) / kFacetChunk;
  const dim3 grid((unsigned)std::min<int64_t>(steps, (int64_t)kFacetWgPerCu * h->n_cu));
  u64* const out = reinterpret_cast<u64*>(out_counts);
  const uint32_t shift = 16u * (uint32_t)field;
  if (bins <= (size_t)kFacetLdsBins)
    facet_kernel<true><<<grid, dim3(kFacetBlock), bins * 4, st>>>(h->tags, view, count, shift,
                                                                  (uint32_t)n_codes, out);
  else
    facet_kernel<false><<<grid, dim3(kFacetBlock), 0, st>>>(h->tags, view, count, shift,
                                                            (uint32_t)n_codes, out);
  RAG_HIP(hipGetLastError());
  return RAG_OK;
}

}  // extern "C"
