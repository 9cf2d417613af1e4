// seed_kernels.hip — the seed sample of a search pass (included by index_search.hip after
// scan_kernels.hip): a few thousand tiles spread over the shard are scored with the scan's own
// arithmetic (sample_kernel, the fused qprep_sample_kernel, sample_wide_kernel) and
// thresh_kernel turns their per-query maxima into seed_thr, the lower bound of the 32nd-best
// score that the scan starts its thresholds from.
namespace ragmi {

// ----------------------------------------------------------------------------------------
// sample: seed thresholds for the scan. Sample wave w scores the corpus tiles
//   t = (j * n_tiles) / n_sample, j = w, w + n_waves, ...   (spread over the shard)
// and writes, per query, the max score over its (valid, filter-passing) rows to
// smax[w][q]. The 32nd largest of these per-wave maxima comes from 32 distinct rows, so it
// is a lower bound of the global 32nd-best score: thresh_kernel turns it into seed_thr.
// ----------------------------------------------------------------------------------------
// A sample wave's tiles. Wave w of the grid takes the sample indices j0 = 2w and 2w + 1 (two
// tiles per wave, all loads in flight at once); the last wave of an odd n_sample has one
// (`two` false: t1 = t0 is scored again and its maxima are not written).
struct SampleTiles {
  int j0, t0, t1;
  bool two;
  const half8 *p0, *p1;   // the lane's first half8 of tile t0 / t1
};

// false: no tile for this wave (st is then not to be used)
template <int S>
__device__ __forceinline__ bool sample_tiles(SampleTiles& st, const half8* __restrict__ corpus,
                                             int n_tiles, int n_sample, int lane) {
  const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  st.j0 = 2 * w;
  if (st.j0 >= n_sample) return false;
  st.two = st.j0 + 1 < n_sample;
  st.t0 = (int)(((int64_t)st.j0 * n_tiles) / n_sample);
  st.t1 = st.two ? (int)(((int64_t)(st.j0 + 1) * n_tiles) / n_sample) : st.t0;
  st.p0 = corpus + (int64_t)st.t0 * (S * 64) + lane;
  st.p1 = corpus + (int64_t)st.t1 * (S * 64) + lane;
  return true;
}

// Scores of the two sample tiles for D <= 384: both tiles' vectors and the query fragments
// (qf: qfrag in global memory, or an LDS image of the same layout) all in flight at once.
template <int S>
__device__ __forceinline__ void sample_scores(const SampleTiles& st, const half8* qf, int lane,
                                              floatx4 (&sc)[2][2]) {
  half8 a0[S], a1[S], b0[S], b1[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    a0[s] = __builtin_nontemporal_load(st.p0 + s * 64);
    a1[s] = __builtin_nontemporal_load(st.p1 + s * 64);
    b0[s] = qf[s * 64 + lane];
    b1[s] = qf[(S + s) * 64 + lane];
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    sc[u][0] = sc[u][1] = floatx4{0.f, 0.f, 0.f, 0.f};
    tile_mfma<S>(u == 0 ? a0 : a1, b0, b1, sc[u][0], sc[u][1]);
  }
}

// Scores of one tile (p: the lane's first half8 of it) in chunks of CH k-steps, the query
// fragments re-read from qf (global; L2) per chunk: for rows too wide to hold whole in VGPRs.
template <int S, int CH>
__device__ __forceinline__ void tile_scores_chunked(const half8* p, const half8* __restrict__ qf,
                                                    int lane, floatx4& acc0, floatx4& acc1) {
  static_assert(S % CH == 0, "k-step chunks");
  for (int c = 0; c < S / CH; ++c) {
    half8 a[CH], b0[CH], b1[CH];
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      a[s] = __builtin_nontemporal_load(p + (c * CH + s) * 64);
      b0[s] = qf[(c * CH + s) * 64 + lane];
      b1[s] = qf[(S + c * CH + s) * 64 + lane];
    }
    tile_mfma<CH>(a, b0, b1, acc0, acc1);
  }
}

// per-query maxima of one wave's two sample tiles (sc[tile][query half]) -> smax[q][j]
template <bool FILTER>
__device__ __forceinline__ void sample_epilogue(const floatx4 (&sc)[2][2], const SampleTiles& st,
                                                int lane, const uint32_t* __restrict__ tags,
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
    const int t = u == 0 ? st.t0 : st.t1;
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
    smax[(int64_t)lane * n_sample + st.j0] = mx[0][0];
    smax[(int64_t)(16 + lane) * n_sample + st.j0] = mx[0][1];
    if (st.two) {
      smax[(int64_t)lane * n_sample + st.j0 + 1] = mx[1][0];
      smax[(int64_t)(16 + lane) * n_sample + st.j0 + 1] = mx[1][1];
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
  SampleTiles st;
  if (!sample_tiles<S>(st, corpus, n_tiles, n_sample, lane)) return;
  // scores of the two sample tiles: all loads in flight at once (D <= 384), or in chunks of 8
  // k-steps with the query fragments re-read from L2 (wide rows: 4 x D/32 half8 would spill)
  floatx4 sc[2][2];
  if constexpr (S <= 12) {
    sample_scores<S>(st, qfrag, lane, sc);
  } else {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sc[u][0] = sc[u][1] = floatx4{0.f, 0.f, 0.f, 0.f};
      tile_scores_chunked<S, 8>(u == 0 ? st.p0 : st.p1, qfrag, lane, sc[u][0], sc[u][1]);
    }
  }
  sample_epilogue<FILTER>(sc, st, lane, tags, filt, n_rows, n_sample, smax);
}

// sample for a pass that scans a copy (scan_kernel_i8 / scan_kernel_i6): the same sample tiles
// scored with that scan's own upper bound u (the format's tile_u_at), so thresh_kernel's seed is
// a lower bound of the 32nd-best u, which is what that scan's thresholds compare.
// Four waves per SIMD asked for: left to itself the allocator gave the same code three or four
// (136 or 120 registers) depending on what else the unit instantiates.
template <int D, bool FILTER, typename Copy>
__global__ __launch_bounds__(256, 4) void sample_kernel_q(
    const char* __restrict__ data, const float* __restrict__ meta,
    const uint32_t* __restrict__ tags, const uint32_t* __restrict__ filt,
    const intx4* __restrict__ qfrag8, const float* __restrict__ qp8, int n_rows, int n_tiles,
    int n_sample, float* __restrict__ smax) {
  const int lane = threadIdx.x & 63;
  SampleTiles st;
  // only the tile numbers are used: the format addresses its own tiles (tile_u_at)
  if (!sample_tiles<1>(st, reinterpret_cast<const half8*>(data), n_tiles, n_sample, lane)) return;
  Query8<D> q;
  query8_load<D>(q, qfrag8, qp8, lane);
  floatx4 sc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
    Copy::template tile_u_at<D>(data, meta, u == 0 ? st.t0 : st.t1, q, lane, sc[u][0], sc[u][1]);
  sample_epilogue<FILTER>(sc, st, lane, tags, filt, n_rows, n_sample, smax);
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
  SampleTiles st;
  if (!sample_tiles<S>(st, corpus, n_tiles, n_sample, lane)) return;
  floatx4 sc[2][2];
  sample_scores<S>(st, qf_l, lane, sc);
  sample_epilogue<FILTER>(sc, st, lane, tags, filt_l, n_rows, n_sample, smax);
}

constexpr int kSampleGroups = 4;   // query groups of 32 per wide pass (index_host.hpp kMaxGroups)

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
  SampleTiles st;
  if (!sample_tiles<S>(st, corpus, n_tiles, n_sample, lane)) return;
  floatx4 acc[kSampleGroups][2][2];
#pragma unroll
  for (int g = 0; g < kSampleGroups; ++g)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[g][u][0] = acc[g][u][1] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < S / CH; ++c) {
    half8 a0[CH], a1[CH];
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      a0[s] = __builtin_nontemporal_load(st.p0 + (c * CH + s) * 64);
      a1[s] = __builtin_nontemporal_load(st.p1 + (c * CH + s) * 64);
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
      sample_epilogue<FILTER>(acc[g], st, lane, tags, filt + g * (2 * kQ), n_rows, n_sample,
                              smax + (int64_t)g * kQ * n_sample);
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

}  // namespace ragmi
