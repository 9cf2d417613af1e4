// rows_kernels.hip — row removal for the flat index (included by index_capi.hip after
// scan_kernels.hip): the ordered tag select and the indexed row copies behind
// rag_index_select_rows / move_rows / gather_rows / scatter_rows, and the grouped search's tag
// gather and group selection behind rag_index_gather_tags / rag_group_select (include/ragmi.h).
//
// A deleted row is physically removed: a surviving row from the tail takes its slot in every
// stored form (the fp16 tile16 pieces, the fp32 row of an fp32-storage index, the tag), bit
// for bit, and the count shrinks. The index stays dense, so the scan, select, large-k and
// full-pass kernels never learn that a delete happened ("Deleting points").
// No reference counterpart beyond QdrantClient.delete itself: the reference only ever upserts
// (ingest.py:171-175) and leaves removal to the Qdrant server.
namespace ragmi {

// ----------------------------------------------------------------------------------------
// select: rows r < count with (tag[r] & mask) == value, ascending — an ordered stream
// compaction over the tag array in three launches:
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
                                             int64_t count, uint32_t mask, uint32_t value,
                                             bool (&f)[4]) {
  f[0] = f[1] = f[2] = f[3] = false;
  if (r < count) {
    const uint4 t = *reinterpret_cast<const uint4*>(tags + r);
    f[0] = (t.x & mask) == value;
    f[1] = r + 1 < count && (t.y & mask) == value;
    f[2] = r + 2 < count && (t.z & mask) == value;
    f[3] = r + 3 < count && (t.w & mask) == value;
  }
}

__global__ __launch_bounds__(kSelBlock) void select_count_kernel(
    const uint32_t* __restrict__ tags, int64_t count, uint32_t mask, uint32_t value,
    int64_t* __restrict__ counts) {
  __shared__ int wsum[kSelBlock / 64];
  const int tid = threadIdx.x;
  int c = 0;   // wave-uniform
  for (int it = 0; it < kSelIters; ++it) {
    const int64_t r = (int64_t)blockIdx.x * kSelChunk + it * (kSelBlock * 4) + tid * 4;
    bool f[4];
    select_flags(tags, r, count, mask, value, f);
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

// counts[0..nb) -> exclusive prefix sums in place; *out_n = the total
__global__ __launch_bounds__(kSelScanBlock) void select_scan_kernel(int64_t* __restrict__ counts,
                                                                    int nb,
                                                                    int64_t* __restrict__ out_n) {
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
  if (tid == 0) *out_n = carry;
}

__global__ __launch_bounds__(kSelBlock) void select_emit_kernel(
    const uint32_t* __restrict__ tags, int64_t count, uint32_t mask, uint32_t value,
    const int64_t* __restrict__ offsets, int64_t* __restrict__ out, int64_t cap) {
  __shared__ int wcnt[kSelBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int64_t base = offsets[blockIdx.x];
  if (base >= cap) return;   // the whole chunk lies past the output (uniform)
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int it = 0; it < kSelIters; ++it) {
    const int64_t r = (int64_t)blockIdx.x * kSelChunk + it * (kSelBlock * 4) + tid * 4;
    bool f[4];
    select_flags(tags, r, count, mask, value, f);
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
// grouped search (rag_index_gather_tags, rag_group_select).
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

// group_select_kernel: the sequential walk of include/ragmi.h over one query's candidate list,
// in parallel form. One workgroup per query; it reads only its input arrays (no index).
//   key[j]   = tag[j] & key_mask, in LDS (16 KiB at C = 4096)
//   rank[j]  = number of i < j with key[i] == key[j]
//   first[j] = key[j] != 0 && rank[j] == 0; the group index of a key = the number of firsts
//              before its own first
//   emit iff key[j] != 0, group index < G, rank < S, at out[b][group][rank]
// The list is walked in trips of kGrpBlock candidates, in order, against a table of the groups
// opened so far (s_gkey, in opening order; s_cnt, their candidates seen in earlier trips). A
// candidate looks its key up in the table (the earlier trips), then counts the earlier
// candidates of its own trip with its key, so rank = s_cnt[group] + the in-trip count and a
// trip costs ng / 4 + at most kGrpBlock / 4 LDS reads per lane however long the list is. A key
// that is in neither is a first: it takes index ng + the number of this trip's earlier firsts
// (ballot / popcount per wave, wave totals in LDS) and enters the table while that is < G; a
// later candidate of the trip with the same key reads the index back from its first's lane
// (s_tg). A candidate whose group already holds S hits, or whose key is unknown when G groups
// are open, can never be emitted and takes no further part. Both loops read LDS four keys at a
// time at a wave-uniform address (a broadcast: no bank conflict); the in-trip one runs to the
// wave's last candidate and a lane masks off the entries at or past its own j.
// Every position is a pure function of the inputs: integer LDS atomics only (min, add), whose
// results do not depend on their order, so the output is the same on every run. Every output
// element is written exactly once: the emitted entries in the trips, the padding (-inf / -1 /
// -1, key 0, fill 0) after the last one from the counts.
// ----------------------------------------------------------------------------------------
constexpr int kGrpBlock = 512;
constexpr int kGrpMaxC = 4096;      // RAG_GROUPS_MAX_CANDIDATES
constexpr int kGrpMaxG = 1024;      // RAG_GROUPS_MAX
constexpr int kGrpMaxCells = 4096;  // G * S

__global__ __launch_bounds__(kGrpBlock) void group_select_kernel(
    const float* __restrict__ cand_s, const int64_t* __restrict__ cand_r,
    const uint32_t* __restrict__ cand_t, const int32_t* __restrict__ ncand, int C,
    uint32_t key_mask, int G, int S, uint32_t* __restrict__ out_keys, int32_t* __restrict__ out_fill,
    float* __restrict__ out_s, int64_t* __restrict__ out_r, int32_t* __restrict__ out_pos,
    int32_t* __restrict__ out_count) {
  __shared__ __attribute__((aligned(16))) uint32_t s_key[kGrpMaxC];
  __shared__ __attribute__((aligned(16))) uint32_t s_gkey[kGrpMaxG];   // keys of the open groups
  __shared__ int s_cnt[kGrpMaxG];    // their candidates seen in the earlier trips
  __shared__ int s_tg[kGrpBlock];    // group index of this trip's firsts, by lane
  __shared__ int s_wcnt[kGrpBlock / 64];
  __shared__ int s_n;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = blockIdx.x;
  cand_s += b * C;
  cand_r += b * C;
  cand_t += b * C;
  const int64_t obase = b * G * S;

  if (tid == 0) {
    int n0 = C;
    if (ncand) n0 = min(C, max(0, ncand[b]));
    s_n = n0;
  }
  for (int g = tid; g < ((G + 3) & ~3); g += kGrpBlock) {   // <= kGrpMaxG; 0 matches no live key
    s_gkey[g] = 0u;
    s_cnt[g] = 0;
  }
  __syncthreads();
  for (int j = tid; j < C; j += kGrpBlock) {
    s_key[j] = cand_t[j] & key_mask;
    if (cand_r[j] < 0) atomicMin(&s_n, j);   // the list ends at its first absent row
  }
  __syncthreads();
  const int n = s_n;

  const unsigned long long below = (1ull << lane) - 1ull;
  int ng = 0;   // open groups (uniform)
  for (int base = 0; base < n; base += kGrpBlock) {
    const int j = base + tid;
    uint32_t key = j < n ? s_key[j] : 0u;
    int g = -1, before = 0;
    if (key != 0u) {
      for (int e = 0; e < ng; e += 4) {
        const uint4 k4 = *reinterpret_cast<const uint4*>(&s_gkey[e]);
        g = k4.x == key ? e : k4.y == key ? e + 1 : k4.z == key ? e + 2 : k4.w == key ? e + 3 : g;
      }
      if (g >= 0) before = s_cnt[g];
      // its group is full, or no group is left to open: never emitted (nor are its key's others)
      if (g >= 0 ? before >= S : ng >= G) key = 0u;
    }
    int rank_in = 0, fin = -1;   // this trip's earlier candidates with the key; the first of them
    if (key != 0u) {
      const int lend = min(n, base + (w + 1) * 64);   // wave-uniform: the wave's last candidate
      for (int i = base; i < lend; i += 4) {
        const uint4 k4 = *reinterpret_cast<const uint4*>(&s_key[i]);
        const bool m0 = i < j && k4.x == key;
        const bool m1 = i + 1 < j && k4.y == key;
        const bool m2 = i + 2 < j && k4.z == key;
        const bool m3 = i + 3 < j && k4.w == key;
        if (fin < 0) fin = m0 ? i : m1 ? i + 1 : m2 ? i + 2 : m3 ? i + 3 : -1;
        rank_in += (int)m0 + (int)m1 + (int)m2 + (int)m3;
      }
    }
    const bool first = key != 0u && g < 0 && rank_in == 0;
    const unsigned long long fb = __ballot(first);
    if (lane == 0) s_wcnt[w] = __popcll(fb);
    __syncthreads();   // every lane has read the table and the counts
    int wbase = 0, tot = 0;
    for (int u = 0; u < kGrpBlock / 64; ++u) {
      const int t = s_wcnt[u];
      if (u < w) wbase += t;
      tot += t;
    }
    if (first) {
      g = ng + wbase + __popcll(fb & below);
      s_tg[tid] = g;
      if (g < G) s_gkey[g] = key;
    }
    __syncthreads();   // this trip's firsts are in s_tg
    if (key != 0u && g < 0) g = s_tg[fin - base];
    if (key != 0u && g < G) {
      const int rank = before + rank_in;
      if (first) out_keys[b * G + g] = key;
      if (rank < S) {
        const int64_t o = obase + (int64_t)g * S + rank;
        out_s[o] = cand_s[j];
        out_r[o] = cand_r[j];
        if (out_pos) out_pos[o] = j;
      }
      atomicAdd(&s_cnt[g], 1);
    }
    ng = min(ng + tot, G);
    __syncthreads();   // table, counts, s_tg and s_wcnt are settled for the next trip
  }
  for (int g = tid; g < G; g += kGrpBlock) {
    out_fill[b * G + g] = min(s_cnt[g], S);
    if (g >= ng) out_keys[b * G + g] = 0u;
  }
  const int cells = G * S;
  for (int e = tid; e < cells; e += kGrpBlock) {
    const int g = e / S, r = e - g * S;
    if (r >= s_cnt[g]) {
      out_s[obase + e] = kNegInf;
      out_r[obase + e] = -1;
      if (out_pos) out_pos[obase + e] = -1;
    }
  }
  if (tid == 0) {
    out_count[b * 2] = ng;
    out_count[b * 2 + 1] = n;
  }
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

// half8 slot of piece c (halves 8c .. 8c+7) of row `row` in the tile16 layout
template <int D>
__device__ __forceinline__ int64_t tile_slot(int64_t row, int c) {
  return (row >> 4) * (steps<D>() * 64) + (c >> 2) * 64 + (c & 3) * 16 + (row & 15);
}

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

}  // namespace ragmi
