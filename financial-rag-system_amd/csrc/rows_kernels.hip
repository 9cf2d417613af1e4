// rows_kernels.hip — row-wise access to the flat index (included by index_store.hip last; it
// needs only the tile16 layout of prep_kernels.hip): the ordered tag select and the indexed row
// copies behind rag_index_select_rows / move_rows / gather_rows / scatter_rows, the grouped
// search's tag gather behind rag_index_gather_tags (include/ragmi.h), the export / import
// of rows between tile16 and row-major (persistence), and the key columns' fill / write /
// gather / move (rag_index_keys_create, write_keys, gather_keys, move_rows).
//
// A deleted row is physically removed: a surviving row from the tail takes its slot in every
// stored form (the fp16 tile16 pieces, the fp32 row of an fp32-storage index, the tag, the key
// of every key column), bit for bit, and the count shrinks. The index stays dense, so the scan, select, large-k and
// full-pass kernels never learn that a delete happened ("Deleting points").
// No reference counterpart beyond QdrantClient.delete itself: the reference only ever upserts
// (ingest.py:171-175) and leaves removal to the Qdrant server.
namespace ragmi {

// ----------------------------------------------------------------------------------------
// select: rows row0 <= r < count with (tag[r] & mask) == value, ascending — an ordered stream
// compaction over the tag array in three launches (the chunks from row0's on: workgroup b takes
// chunk chunk0 + b, chunk0 = row0 / kSelChunk; rag_index_select_rows_from; row0 = 0 otherwise):
//   select_count_kernel   matches per chunk of kSelChunk rows (one workgroup per chunk)
//   select_scan_kernel    exclusive prefix sum over the chunks (one workgroup), total -> *out_n
//   select_emit_kernel    each chunk re-reads its tags (L2 / Infinity Cache warm) and writes
//                         its matches from its offset, in row order, while the offset < cap
// Every position is a pure function of the tags: no atomics, the same output on every run.
// A lane reads 4 consecutive tags as one dwordx4 (a wave 1 KiB per load).
// ----------------------------------------------------------------------------------------
constexpr int kSelBlock = 256;
constexpr int kSelIters = 4;
constexpr int kSelChunk = kSelBlock * 4 * kSelIters;   // rows per workgroup
constexpr int kSelScanBlock = 1024;

// f[j] = row r + j matches; r is a multiple of 4 and the tag array holds a multiple of 16
// rows, so the 16-byte load stays inside it whenever r < count
__device__ __forceinline__ void select_flags(const uint32_t* __restrict__ tags, int64_t r,
                                             int64_t row0, int64_t count, uint32_t mask,
                                             uint32_t value, bool (&f)[4]) {
  f[0] = f[1] = f[2] = f[3] = false;
  if (r < count) {
    const uint4 t = *reinterpret_cast<const uint4*>(tags + r);
    f[0] = r >= row0 && (t.x & mask) == value;
    f[1] = r + 1 >= row0 && r + 1 < count && (t.y & mask) == value;
    f[2] = r + 2 >= row0 && r + 2 < count && (t.z & mask) == value;
    f[3] = r + 3 >= row0 && r + 3 < count && (t.w & mask) == value;
  }
}

__global__ __launch_bounds__(kSelBlock) void select_count_kernel(
    const uint32_t* __restrict__ tags, int64_t row0, int64_t count, uint32_t mask, uint32_t value,
    int64_t* __restrict__ counts) {
  __shared__ int wsum[kSelBlock / 64];
  const int tid = threadIdx.x;
  int c = 0;   // wave-uniform
  for (int it = 0; it < kSelIters; ++it) {
    const int64_t r =
        (row0 / kSelChunk + blockIdx.x) * kSelChunk + it * (kSelBlock * 4) + tid * 4;
    bool f[4];
    select_flags(tags, r, row0, count, mask, value, f);
#pragma unroll
    for (int j = 0; j < 4; ++j) c += __popcll(__ballot(f[j]));
  }
  if ((tid & 63) == 0) wsum[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < kSelBlock / 64; ++w) s += wsum[w];
    counts[blockIdx.x] = s;
  }
}

// counts[0..nb) -> exclusive prefix sums in place, by one workgroup of kSelScanBlock threads;
// returns the total to every thread
__device__ int64_t scan_chunks(int64_t* __restrict__ counts, int nb) {
  constexpr int kWaves = kSelScanBlock / 64;
  __shared__ int wtot[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int64_t carry = 0;
  for (int b0 = 0; b0 < nb; b0 += kSelScanBlock) {
    const int i = b0 + tid;
    const int v = i < nb ? (int)counts[i] : 0;   // <= kSelChunk each
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) wtot[w] = x;
    __syncthreads();
    int wbase = 0, tot = 0;
    for (int u = 0; u < kWaves; ++u) {
      const int t = wtot[u];
      if (u < w) wbase += t;
      tot += t;
    }
    if (i < nb) counts[i] = carry + wbase + x - v;
    carry += tot;
    __syncthreads();
  }
  return carry;
}

// counts[0..nb) -> exclusive prefix sums in place; *out_n = the total
__global__ __launch_bounds__(kSelScanBlock) void select_scan_kernel(int64_t* __restrict__ counts,
                                                                    int nb,
                                                                    int64_t* __restrict__ out_n) {
  const int64_t total = scan_chunks(counts, nb);
  if (threadIdx.x == 0) *out_n = total;
}

__global__ __launch_bounds__(kSelBlock) void select_emit_kernel(
    const uint32_t* __restrict__ tags, int64_t row0, int64_t count, uint32_t mask, uint32_t value,
    const int64_t* __restrict__ offsets, int64_t* __restrict__ out, int64_t cap) {
  __shared__ int wcnt[kSelBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int64_t base = offsets[blockIdx.x];
  if (base >= cap) return;   // the whole chunk lies past the output (uniform)
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int it = 0; it < kSelIters; ++it) {
    const int64_t r =
        (row0 / kSelChunk + blockIdx.x) * kSelChunk + it * (kSelBlock * 4) + tid * 4;
    bool f[4];
    select_flags(tags, r, row0, count, mask, value, f);
    int pre = 0, wc = 0;   // matches in lower lanes / in the wave: lanes own rows in order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long b = __ballot(f[j]);
      pre += __popcll(b & below);
      wc += __popcll(b);
    }
    if (lane == 0) wcnt[w] = wc;
    __syncthreads();
    int wbase = 0, tot = 0;
    for (int u = 0; u < kSelBlock / 64; ++u) {
      const int t = wcnt[u];
      if (u < w) wbase += t;
      tot += t;
    }
    int64_t pos = base + wbase + pre;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (f[j]) {
        if (pos < cap) out[pos] = r + j;   // never past cap
        ++pos;
      }
    base += tot;
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------------------
// grouped search (rag_index_gather_tags; the group selection it feeds is
// group_select_kernel, reselect_kernels.hip).
// gather_tags_kernel: out[i] = tag[rows[i]] for rows in [0, cap_rows), 0 otherwise; a row index
// outside that range is never dereferenced.
// ----------------------------------------------------------------------------------------
constexpr int kTagBlock = 256;

__global__ __launch_bounds__(kTagBlock) void gather_tags_kernel(
    const uint32_t* __restrict__ tags, const int64_t* __restrict__ rows, int64_t n,
    int64_t cap_rows, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kTagBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rows[i];
  out[i] = (r >= 0 && r < cap_rows) ? tags[r] : 0u;
}

// ----------------------------------------------------------------------------------------
// indexed row copies. One workgroup per group of 16 (source, destination) pairs — a tile's
// worth, and the movers of a delete are mostly a contiguous tail, the holes often a
// contiguous run — copying every stored form of the rows:
//   kRowsMove     index row src[i] -> index row dst[i]        (in place; sets disjoint)
//   kRowsGather   index row rows[i] -> packed staging row i   (rows = src_rows)
//   kRowsScatter  packed staging row i -> index row rows[i]   (rows = dst_rows)
// Packed staging is row-major: pk16 [n][D/8] half8, pk32 [n][D] float, pktags [n].
// Lane order of the fp16 pieces: a wave takes one 32-dim k-step of the 16 rows, which in the
// tile is one contiguous 1 KiB when the rows are a tile (lane = hh * 16 + r, the layout's own
// order, for the move; for the packed forms the 4 pieces of a row's k-step go to neighbouring
// lanes, 64 contiguous bytes on the packed side and the same 1 KiB on the tile side).
// The fp32 rows are row-major on both sides: a wave copies 1 KiB of one row per instruction.
// An index row outside [0, cap_rows) is never dereferenced: its pair is skipped.
// ----------------------------------------------------------------------------------------
constexpr int kRowsBlock = 256;
constexpr int kRowsGroup = 16;
enum { kRowsMove = 0, kRowsGather = 1, kRowsScatter = 2 };

template <int D, int MODE>
__global__ __launch_bounds__(kRowsBlock) void copy_rows_kernel(
    half8* corpus, float* rows32, uint32_t* tags, const int64_t* __restrict__ src_rows,
    const int64_t* __restrict__ dst_rows, int64_t n, int64_t cap_rows, half8* pk16, float* pk32,
    uint32_t* pktags) {
  __shared__ int64_t s_src[kRowsGroup], s_dst[kRowsGroup];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kRowsGroup;
  if (tid < kRowsGroup) {
    const int64_t i = base + tid;
    int64_t s = -1, d = -1;
    if (i < n) {
      s = MODE == kRowsScatter ? i : src_rows[i];
      d = MODE == kRowsGather ? i : dst_rows[i];
      const bool s_ok = MODE == kRowsScatter || (s >= 0 && s < cap_rows);
      const bool d_ok = MODE == kRowsGather || (d >= 0 && d < cap_rows);
      if (!s_ok || !d_ok) s = d = -1;
    }
    s_src[tid] = s;
    s_dst[tid] = d;
  }
  __syncthreads();
  constexpr int kPieces = D / 8;
  for (int e = tid; e < kRowsGroup * kPieces; e += kRowsBlock) {
    int j, c;
    if (MODE == kRowsMove) {
      j = e & 15;
      c = e >> 4;
    } else {
      j = (e >> 2) & 15;
      c = ((e >> 6) << 2) | (e & 3);
    }
    const int64_t s = s_src[j], d = s_dst[j];
    if (s < 0) continue;
    const half8 v = MODE == kRowsScatter ? pk16[s * kPieces + c] : corpus[tile_slot<D>(s, c)];
    if (MODE == kRowsGather)
      pk16[d * kPieces + c] = v;
    else
      corpus[tile_slot<D>(d, c)] = v;
  }
  if (rows32) {
    constexpr int kQuads = D / 4;
    for (int e = tid; e < kRowsGroup * kQuads; e += kRowsBlock) {
      const int j = e / kQuads, c = e % kQuads;
      const int64_t s = s_src[j], d = s_dst[j];
      if (s < 0) continue;
      const float4* from = reinterpret_cast<const float4*>((MODE == kRowsScatter ? pk32 : rows32) + s * D);
      float4* to = reinterpret_cast<float4*>((MODE == kRowsGather ? pk32 : rows32) + d * D);
      to[c] = from[c];
    }
  }
  if (tid < kRowsGroup && s_src[tid] >= 0) {
    const int64_t s = s_src[tid], d = s_dst[tid];
    const uint32_t t = MODE == kRowsScatter ? pktags[s] : tags[s];
    if (MODE == kRowsGather)
      pktags[d] = t;
    else
      tags[d] = t;
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
  out[idx] = corpus[tile_slot<D>(row0 + i, c)];
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
  corpus[tile_slot<D>(row0 + i, c)] = in[idx];
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
  corpus[tile_slot<D>(row, c)] = h;
}

// ----------------------------------------------------------------------------------------
// key columns (include/ragmi.h "Key columns"): up to RAG_KEYS_MAX_COLS int64 columns of
// cap_rows keys beside the tags, what the RANGE atom of filter_view_kernel compares. One thread
// per element in all four kernels; a row index outside [0, cap_rows) is never dereferenced.
//   fill_keys_kernel    keys[r] = RAG_KEY_ABSENT for r in [row0, cap_rows) (create, reserve)
//   write_keys_kernel   keys[rows[i]] = vals[i]                  (rows distinct)
//   gather_keys_kernel  out[i] = keys[rows[i]], RAG_KEY_ABSENT outside — gather_tags' guard
//   move_keys_kernel    every column's key of row src[i] -> row dst[i], a pair with either row
//                       outside skipped, as copy_rows_kernel skips it (sets disjoint)
// ----------------------------------------------------------------------------------------
constexpr int kKeyBlock = 256;

// the index's columns as a kernel argument; entries at or past the column count are nullptr
struct KeyCols {
  int64_t* col[RAG_KEYS_MAX_COLS];
};

__global__ __launch_bounds__(kKeyBlock) void fill_keys_kernel(int64_t* __restrict__ keys,
                                                              int64_t row0, int64_t cap_rows) {
  const int64_t r = row0 + (int64_t)blockIdx.x * kKeyBlock + threadIdx.x;
  if (r < cap_rows) keys[r] = RAG_KEY_ABSENT;
}

__global__ __launch_bounds__(kKeyBlock) void write_keys_kernel(
    int64_t* __restrict__ keys, const int64_t* __restrict__ rows,
    const int64_t* __restrict__ vals, int64_t n, int64_t cap_rows) {
  const int64_t i = (int64_t)blockIdx.x * kKeyBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rows[i];
  if (r >= 0 && r < cap_rows) keys[r] = vals[i];
}

__global__ __launch_bounds__(kKeyBlock) void gather_keys_kernel(
    const int64_t* __restrict__ keys, const int64_t* __restrict__ rows, int64_t n,
    int64_t cap_rows, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kKeyBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rows[i];
  out[i] = (r >= 0 && r < cap_rows) ? keys[r] : RAG_KEY_ABSENT;
}

__global__ __launch_bounds__(kKeyBlock) void move_keys_kernel(
    KeyCols keys, int n_cols, const int64_t* __restrict__ src_rows,
    const int64_t* __restrict__ dst_rows, int64_t n, int64_t cap_rows) {
  const int64_t i = (int64_t)blockIdx.x * kKeyBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t s = src_rows[i], d = dst_rows[i];
  if (s < 0 || s >= cap_rows || d < 0 || d >= cap_rows) return;
#pragma unroll
  for (int c = 0; c < RAG_KEYS_MAX_COLS; ++c)
    if (c < n_cols) keys.col[c][d] = keys.col[c][s];
}

}  // namespace ragmi
