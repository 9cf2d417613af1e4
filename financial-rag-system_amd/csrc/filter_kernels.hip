// filter_kernels.hip — the filter algebra's one kernel (included by index_store.hip after
// rows_kernels.hip, whose row access it follows): filter_view_kernel evaluates up to
// RAG_FILTER_MAX_PROGRAMS filter programs against every row's tag (and, on an index with key
// columns, its keys: the RANGE atom) and writes a derived tag column, bit s of
// view[r] = "row r passes program s". A search then runs unchanged with the
// view in place of the stored tags and the per-query filter (1 << s, 1 << s); the scan, select,
// large-k and full-pass kernels never learn that a filter was more than (mask, value)
// (DESIGN.md §R9). The blob's layout is the one of include/ragmi.h ("Filter programs"),
// restated by ragmi.filters.pack_view / eval_view_np.
//
// No reference counterpart: the reference only ever sends Filter(must=[MatchValue])
// (main.py:218-236) and leaves every other filter shape to the Qdrant server.
namespace ragmi {

constexpr int kFvBlock = 256;
constexpr int kFvRec = RAG_FILTER_REC_WORDS;   // words per program record
// LDS budget of the staged blob. Records always fit (32 x 41 words = 5.1 KiB). With its
// bitmap pool the whole blob is staged when it is at most 32 KiB: a CU's 160 KiB of LDS then
// still holds 5 workgroups of 4 waves, 20 of the CU's 32 wave slots, enough loads in flight
// for a kernel that only streams tags — and 32 KiB covers 262144 bitmap bits, i.e. every
// program of a call drawing on codebooks of a few thousand values. A larger pool (a field may
// hold 65535 codes: 8 KiB per atom, 2 MiB per call) is read from global memory, where it stays
// L2-resident: every workgroup reads the same words.
constexpr int kFvLdsWords = 8192;
// workgroups per CU of the launch: each stages the blob once and walks its share of the rows
constexpr int kFvWgPerCu = 4;

// POOL_LDS: the whole blob is in LDS (words <= kFvLdsWords), else only the records.
// tags / out: [cap_rows], cap_rows a multiple of 16 (the stored tag array's extent). Rows
// r < count get their bits, rows count <= r < cap_rows get 0; nothing past out[cap_rows - 1]
// is written. A lane owns 4 consecutive rows: one 16-byte load (select_flags' rule: r is a
// multiple of 4, so the load stays inside the array whenever r < count) and one 16-byte store.
// Memory safety does not depend on the blob: atom counts are clamped to 8, a truth-table index
// is < 256 by construction, and a bitmap word is read only when its index is < words.
//
// KEYS: the index has key columns (keys.col[c], c < n_cols, each int64 [cap_rows]) and the blob
// may hold RANGE atoms. The instantiations without the flag are the kernel as it was before
// RANGE existed, and an index without columns launches exactly those. With it:
//   - after the blob is staged, lane t looks at atom t % 8 of program t / 8 (32 x 8 = the
//     workgroup) and ORs into s_used the column of every RANGE atom the row loop will evaluate:
//     the columns the call reads, a wave-uniform mask;
//   - a lane loads its 4 consecutive keys of every such column ONCE per 4 rows, as two 16-byte
//     loads (r is a multiple of 4 and the extent a multiple of 16 rows, so the tags' in-bounds
//     argument carries over; only when r < count), however many atoms of however many programs
//     name the column: 8 B per row and referenced column, none for a column no atom names;
//   - a RANGE atom (p0 column, p1 word offset of lo low, lo high, hi low, hi high) is
//     key != RAG_KEY_ABSENT && lo <= key <= hi, signed. It is false, with neither its bounds nor
//     a key read, when p0 >= n_cols or p1 + 3 >= words: the blob stays untrusted. The bounds
//     come from LDS when the pool is staged, else from global memory (L2-resident, as the
//     bitmaps are).
// The atom loop stays wave-uniform; a program without a RANGE atom pays the one uniform branch
// per atom. The keys are held in registers indexed by compile-time constants only (the column
// is picked by a select chain), so nothing spills to scratch.
template <bool POOL_LDS, bool KEYS = false>
__global__ __launch_bounds__(kFvBlock) void filter_view_kernel(
    const uint32_t* __restrict__ tags, int64_t count, int64_t cap_rows,
    const uint32_t* __restrict__ blob, uint32_t words, int n_programs,
    uint32_t* __restrict__ out, KeyCols keys, int n_cols) {
  extern __shared__ uint32_t s_blob[];
  const int tid = threadIdx.x;
  const uint32_t n_rec = (uint32_t)n_programs * kFvRec;        // <= words (host check)
  const uint32_t n_stage = POOL_LDS ? words : n_rec;
  for (uint32_t i = tid; i < n_stage; i += kFvBlock) s_blob[i] = blob[i];
  uint32_t* const s_used = s_blob + n_stage;   // KEYS: one more word of dynamic LDS (the host's)
  if (KEYS && tid == 0) *s_used = 0u;
  __syncthreads();
  uint32_t used = 0u;
  if (KEYS) {
    static_assert(kFvBlock >= RAG_FILTER_MAX_PROGRAMS * RAG_FILTER_MAX_ATOMS, "one lane per atom");
    const int s = tid >> 3, a = tid & 7;
    if (s < n_programs) {
      const uint32_t* rec = s_blob + s * kFvRec;
      const uint32_t* d = rec + 9 + 4 * a;
      if ((uint32_t)a < min(rec[0], (uint32_t)RAG_FILTER_MAX_ATOMS) &&
          d[0] == RAG_FILTER_ATOM_RANGE && d[1] < (uint32_t)n_cols && (uint64_t)d[2] + 3 < words)
        atomicOr(s_used, 1u << d[1]);
    }
    __syncthreads();
    used = *s_used;
  }
  const int64_t step = (int64_t)gridDim.x * (kFvBlock * 4);
  for (int64_t r = (int64_t)blockIdx.x * (kFvBlock * 4) + tid * 4; r < cap_rows; r += step) {
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (r < count) {
      const uint4 t4 = *reinterpret_cast<const uint4*>(tags + r);
      const uint32_t t[4] = {t4.x, t4.y, t4.z, t4.w};
      int64_t kv[RAG_KEYS_MAX_COLS][4];
      if (KEYS) {
#pragma unroll
        for (int c = 0; c < RAG_KEYS_MAX_COLS; ++c) {
          kv[c][0] = kv[c][1] = kv[c][2] = kv[c][3] = RAG_KEY_ABSENT;
          if ((used >> c) & 1u) {                     // wave-uniform; implies c < n_cols
            const longlong2* kp = reinterpret_cast<const longlong2*>(keys.col[c] + r);
            const longlong2 k01 = kp[0], k23 = kp[1];
            kv[c][0] = k01.x;
            kv[c][1] = k01.y;
            kv[c][2] = k23.x;
            kv[c][3] = k23.y;
          }
        }
      }
      for (int s = 0; s < n_programs; ++s) {          // wave-uniform
        const uint32_t* rec = s_blob + s * kFvRec;
        const int na = (int)min(rec[0], (uint32_t)RAG_FILTER_MAX_ATOMS);
        uint32_t idx[4] = {0u, 0u, 0u, 0u};
        for (int a = 0; a < na; ++a) {                // wave-uniform
          const uint32_t* d = rec + 9 + 4 * a;
          const uint32_t kind = d[0], p0 = d[1], p1 = d[2], p2 = d[3];
          if (KEYS && kind == RAG_FILTER_ATOM_RANGE) {
            // p0 key column, p1 word offset in the blob of (lo, hi); false when either is out
            if (p0 < (uint32_t)n_cols && (uint64_t)p1 + 3 < words) {
              const uint32_t* b = POOL_LDS ? s_blob + p1 : blob + p1;
              const int64_t lo = (int64_t)(((uint64_t)b[1] << 32) | b[0]);
              const int64_t hi = (int64_t)(((uint64_t)b[3] << 32) | b[2]);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int64_t k = p0 == 0 ? kv[0][j] : p0 == 1 ? kv[1][j] : p0 == 2 ? kv[2][j]
                                                                                     : kv[3][j];
                idx[j] |= (uint32_t)(k != RAG_KEY_ABSENT && lo <= k && k <= hi) << a;
              }
            }
          } else if (kind == RAG_FILTER_ATOM_INSET) {
            // p0 field, p1 bitmap word offset in the blob, p2 bitmap length in bits
            const uint32_t shift = (p0 & 1u) * 16u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t code = (t[j] >> shift) & 0xFFFFu;
              const uint64_t w = (uint64_t)p1 + (code >> 5);
              uint32_t bits = 0u;
              if (code < p2 && w < words) bits = POOL_LDS ? s_blob[w] : blob[w];
              idx[j] |= ((bits >> (code & 31u)) & 1u) << a;
            }
          } else {
            // MASKEQ (and any unknown kind): p0 mask, p1 value
#pragma unroll
            for (int j = 0; j < 4; ++j) idx[j] |= (uint32_t)((t[j] & p0) == p1) << a;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] |= ((rec[1 + (idx[j] >> 5)] >> (idx[j] & 31u)) & 1u) << s;
      }
      if (r + 1 >= count) v[1] = 0u;
      if (r + 2 >= count) v[2] = 0u;
      if (r + 3 >= count) v[3] = 0u;
    }
    *reinterpret_cast<uint4*>(out + r) = make_uint4(v[0], v[1], v[2], v[3]);
  }
}

}  // namespace ragmi
