// merge_kernels.hip — merges of exact per-shard result lists into one (included by
// index_search.hip after certify_kernels.hip): where the lists lie (StackedLists, GatheredLists),
// the k <= 32 merge (merge_exact_*, merge_gather_kernel), the k <= kLkMerge merge
// (merge_large_*, merge_gather_large_kernel), the shard set's id remap, and the key / position
// kernels of the any-k merge (merge_any_*).
namespace ragmi {

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
