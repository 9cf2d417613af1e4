// gemm_ws_kernels.hip — the loader-specialised GEMM of large token batches and the deferred
// LayerNorm its epilogues carry (included by bert_capi.hip after gemm_kernels.hip): gemm_ws_kernel,
// launched by launch_ws / launch_ws_large.
namespace ragmi::bert {

// ----------------------------------------------------------------------------------------
// Deferred LayerNorm (fp16x3, hidden 384, the WS GEMMs of large token batches). Between the
// sublayers the token rows' residual stream is kept un-normalised: z = x + sublayer output, as
// fp16 hi + lo planes, plus per row kDlParts partial statistics (mean, centred sum of squares)
// of its 64-column blocks, written by the producing GEMM's epilogue (kEpiResLn). LN(z) is never
// materialised for the token rows:
//  * the consuming GEMMs (QKV, FFN1: kEpiLnF16 / kEpiLnGeluF16) multiply z by W' = W diag(gamma)
//    and correct each row in the epilogue: LN(z) W^T + b = rs (z W'^T - mu c1) + c2, with
//    c1[n] = sum_k W'[n][k] (of the fp16x3 planes) and c2 = b + W beta, folded at encoder
//    creation;
//  * the next residual add (kEpiResLn) recomputes LN(z) per element from the planes and the row
//    statistics: x = (z - mu) rs gamma + beta (fp32), then z' = x + (A W^T + b).
// Per element of a 384-wide projection this replaces the fp32 y write, add_ln's reads of y and
// x and its write of x (16 B) with the residual read and the z write (8 B), and drops the
// add_ln launches.
// ----------------------------------------------------------------------------------------
enum EpiDl { kEpiLnF16 = 4, kEpiLnGeluF16 = 5, kEpiResLn = 6 };
constexpr int kDlH = 384, kDlParts = kDlH / 64;
struct DlArgs {
  const float* st_in = nullptr;    // [M][kDlParts] x {mean, M2}: stats of the A rows (Ln*) or of
                                   // the residual rows (ResLn; null = already normalised)
  float* st_out = nullptr;         // ResLn: stats of the rows written
  const float* gamma = nullptr;    // ResLn: the LayerNorm pending on the residual rows
  const float* beta = nullptr;
  const float* c1 = nullptr;       // Ln*: [N] column sums of W' (the bias argument is c2)
  float eps = 0.f;
};

// hi + lo fp16 planes (4 values each, as loaded) -> fp32 by v_fma_mix_f32 (hi * 1 + lo in one
// instruction; exact, as (float)hi + (float)lo). The inputs come from memory loads, never
// straight from an MFMA (no inline-asm hazard; see split16x2).
__device__ __forceinline__ floatx4 mix_f16x4(u32x2 h, u32x2 l) {
  floatx4 z;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    float lo, hi;
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,1]" : "=v"(lo) : "v"(h[d]), "v"(l[d]));
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]"
        : "=v"(hi) : "v"(h[d]), "v"(l[d]));
    z[2 * d] = lo;
    z[2 * d + 1] = hi;
  }
  return z;
}

// combine a row's kDlParts block statistics (s0..s2 = {mean_0, M2_0, mean_1, M2_1}, ...;
// Chan et al.'s pairwise update over equal 64-element blocks) into its mean and 1/sqrt(var+eps)
__device__ __forceinline__ void dl_row_stats(const floatx4& s0, const floatx4& s1,
                                             const floatx4& s2, float eps, float& mu, float& rs) {
  const float m[kDlParts] = {s0[0], s0[2], s1[0], s1[2], s2[0], s2[2]};
  float q = (s0[1] + s0[3]) + (s1[1] + s1[3]) + (s2[1] + s2[3]);
  mu = ((m[0] + m[1]) + (m[2] + m[3]) + (m[4] + m[5])) * (1.0f / kDlParts);
#pragma unroll
  for (int j = 0; j < kDlParts; ++j) {
    const float d = m[j] - mu;
    q += 64.f * d * d;
  }
  rs = rsqrtf(q * (1.0f / kDlH) + eps);
}

// A row's statistics as the epilogue holds them: the 4 lanes of row ml (g = lane >> 4) load
// floats 4g..4g+3 of its 12 (g < 3: blocks 2g, 2g+1; g = 3 nothing new) a whole tile before
// the epilogue needs them (4 VGPRs per row group; all 12 per lane would not
// fit beside the fragments), and the epilogue combines them across the lanes.
template <int FM>
__device__ __forceinline__ void dl_prefetch_stats(floatx4 (&dls)[FM], __amdgpu_buffer_rsrc_t rsi,
                                                  int wr, int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int ml = wr * 16 * FM + i * 16 + (lane & 15);
    // (lane group 3 re-reads group 2's floats; dl_lane_stats ignores them)
    dls[i] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(
                                             rsi, (ml * kDlParts * 2 + 4 * min(g, 2)) * 4, 0, 0));
  }
}

// mean and 1/sqrt(var + eps) of the row from the lane-split statistics (dl_row_stats' Chan
// combination, reduced over lanes l, l^16, l^32, l^48)
__device__ __forceinline__ void dl_lane_stats(const floatx4& v, int g, float eps, float& mu,
                                              float& rs) {
  float sm = g < 3 ? v[0] + v[2] : 0.f;
  sm += __shfl_xor(sm, 16, 64);
  sm += __shfl_xor(sm, 32, 64);
  mu = sm * (1.0f / kDlParts);
  float q = 0.f;
  if (g < 3) {
    const float d0 = v[0] - mu, d2 = v[2] - mu;
    q = (v[1] + v[3]) + 64.f * (d0 * d0 + d2 * d2);
  }
  q += __shfl_xor(q, 16, 64);
  q += __shfl_xor(q, 32, 64);
  rs = rsqrtf(q * (1.0f / kDlH) + eps);
}

// the deferred-LayerNorm epilogues of one wave's FM x FN fragments (its 64 columns are one
// stats block): fp16 hi + lo planes out through paired 16-B stores (store_f16_pair), ResLn also
// the block's {mean, M2} per row. lds_f: bias | c1 (Ln*) or bias | gamma | beta (ResLn).
// dls: the rows' prefetched statistics (dl_prefetch_stats); rs_out: the output stats panel
// from the tile's row m0.
// fragments (i, jp), (i, jp + 1) of a deferred-LN epilogue -> fp16 hi / lo planes (16-B
// paired stores, store_f16_pair)
template <int AUX, int FM, int FN>
__device__ __forceinline__ void dl_store_pair(const floatx4 (&acc)[FM][FN], int i, int jp, int ml,
                                              int N, int n0, int wc, int cofs,
                                              __amdgpu_buffer_rsrc_t rc,
                                              __amdgpu_buffer_rsrc_t rl) {
  const int vo = (ml * N + n0 + wc * (16 * FN) + jp * 16 + cofs) * 2;
  half4 ha, hb, la, lb;
  // (not split_half4: the two fragments' conversions interleave, as in pipe_epi_pair)
#pragma unroll
  for (int r = 0; r < 4; r += 2) {
    half2 h2, l2;
    split16x2(acc[i][jp][r], acc[i][jp][r + 1], h2, l2);
    ha[r] = h2[0]; ha[r + 1] = h2[1]; la[r] = l2[0]; la[r + 1] = l2[1];
    split16x2(acc[i][jp + 1][r], acc[i][jp + 1][r + 1], h2, l2);
    hb[r] = h2[0]; hb[r + 1] = h2[1]; lb[r] = l2[0]; lb[r + 1] = l2[1];
  }
  store_f16_pair<AUX>(ha, hb, rc, vo);
  store_f16_pair<AUX>(la, lb, rl, vo);
}

template <int EPI, typename CFG, int AUX>
__device__ __forceinline__ void ws_dl_epilogue(floatx4 (&acc)[CFG::FM][CFG::FN],
                                               const float* lds_f, __amdgpu_buffer_rsrc_t rc,
                                               __amdgpu_buffer_rsrc_t rl,
                                               const floatx4 (&dls)[CFG::FM],
                                               __amdgpu_buffer_rsrc_t rs_out, bool has_stats,
                                               int N, int n0, int wr, int wc, int lane,
                                               float eps) {
  constexpr int FM = CFG::FM, FN = CFG::FN, WTM = 16 * FM, WTN = 16 * FN;
  static_assert(WTN == 64 && FN % 2 == 0, "a wave's columns are one stats block");
  const int g = lane >> 4;
  const int cofs = 8 * ((g & 1) * 2 + (g >> 1));
  const float* bias_l = lds_f;
  const float* c1_l = lds_f + N;                          // Ln*
  const float *gam_l = lds_f + N, *bet_l = lds_f + 2 * N;  // ResLn
  // ResLn: residual z of row group i + 1 loaded before group i is computed (read before this
  // wave overwrites it; all four groups at once would spill)
  u32x2 zh[2][FN], zl[2][FN];
  auto load_res = [&](int i) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int vo = ((wr * WTM + i * 16 + (lane & 15)) * N + n0 + wc * WTN + j * 16 + 4 * g) * 2;
      zh[i & 1][j] = __builtin_amdgcn_raw_buffer_load_b64(rc, vo, 0, 0);
      zl[i & 1][j] = __builtin_amdgcn_raw_buffer_load_b64(rl, vo, 0, 0);
    }
  };
  if constexpr (EPI == kEpiResLn) load_res(0);
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    if constexpr (EPI == kEpiResLn)
      if (i + 1 < FM) load_res(i + 1);
    const int ml = wr * WTM + i * 16 + (lane & 15);
    float mu = 0.f, rs = 1.f;
    if (EPI != kEpiResLn || has_stats) dl_lane_stats(dls[i], g, eps, mu, rs);
    if constexpr (EPI == kEpiResLn) {
      // residual x = LN(z) = z rs gamma + (beta - mu rs gamma) from the planes; 4-wide vector
      // arithmetic throughout (gfx950 packed fp32: v_pk_fma / v_pk_add / v_pk_mul)
      const floatx4 a4 = {rs, rs, rs, rs}, b4 = {-mu * rs, -mu * rs, -mu * rs, -mu * rs};
      floatx4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int nl = n0 + wc * WTN + j * 16 + 4 * g;
        const floatx4 z = mix_f16x4(zh[i & 1][j], zl[i & 1][j]);
        const floatx4 b = *reinterpret_cast<const floatx4*>(bias_l + nl);
        floatx4 xr = z;
        if (has_stats)
          xr = __builtin_elementwise_fma(__builtin_elementwise_fma(z, a4, b4),
                                         *reinterpret_cast<const floatx4*>(gam_l + nl),
                                         *reinterpret_cast<const floatx4*>(bet_l + nl));
        acc[i][j] = (acc[i][j] + b) + xr;
        s4 += acc[i][j];
      }
      // the row's 64 columns sit in lanes l, l^16, l^32, l^48
      float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      const float mw = s * (1.0f / 64);
      const floatx4 m4 = {mw, mw, mw, mw};
      floatx4 q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const floatx4 d = acc[i][j] - m4;
        q4 = __builtin_elementwise_fma(d, d, q4);
      }
      float q = (q4[0] + q4[1]) + (q4[2] + q4[3]);
      q += __shfl_xor(q, 16, 64);
      q += __shfl_xor(q, 32, 64);
      if (g == 0) {
        const u32x2 d = {__builtin_bit_cast(uint32_t, mw), __builtin_bit_cast(uint32_t, q)};
        __builtin_amdgcn_raw_buffer_store_b64(d, rs_out,
                                              (ml * kDlParts + (n0 + wc * WTN) / 64) * 8, 0, 0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int nl = n0 + wc * WTN + j * 16 + 4 * g;
        const floatx4 c1 = *reinterpret_cast<const floatx4*>(c1_l + nl);
        const floatx4 c2 = *reinterpret_cast<const floatx4*>(bias_l + nl);
        const floatx4 nm4 = {-mu, -mu, -mu, -mu}, rs4 = {rs, rs, rs, rs};
        acc[i][j] = __builtin_elementwise_fma(rs4, __builtin_elementwise_fma(nm4, c1, acc[i][j]), c2);
        if constexpr (EPI == kEpiLnGeluF16) acc[i][j] = gelu_erf4(acc[i][j]);
      }
    }
    if constexpr (EPI == kEpiResLn) {   // z planes (default policy): row group by row group
#pragma unroll
      for (int jp = 0; jp < FN; jp += 2) dl_store_pair<AUX>(acc, i, jp, ml, N, n0, wc, cofs, rc, rl);
    }
  }
  // QKV / FFN1 outputs (non-temporal): column pair outer, row group inner — the plain
  // epilogue's order. Stored row group by row group like the z planes, these nt streams
  // measured 1.37 / 1.42x their bytes in WRITE_SIZE inside the forward, 1.12 / 1.10x in this
  // order (and FETCH 1.25 -> 1.22 / 1.55 -> 1.43x); the z planes go the other way (1.00 ->
  // 1.14 / 1.20x), so they keep theirs (profiles/r02t_fwd_pmc.jsonl,
  // r02u_fwd_pmc_storeorder_all.jsonl)
  if constexpr (EPI != kEpiResLn) {
#pragma unroll
    for (int jp = 0; jp < FN; jp += 2)
#pragma unroll
      for (int i = 0; i < FM; ++i)
        dl_store_pair<AUX>(acc, i, jp, wr * WTM + i * 16 + (lane & 15), N, n0, wc, cofs, rc, rl);
  }
}

// ----------------------------------------------------------------------------------------
// GEMM, loader-specialised pipe (gemm_ws_kernel; round 2): gemm_pipe_kernel's tiles and ring
// with the DMAs moved to 4 loader waves (one per SIMD), beside the 8 MFMA waves.
// Probes of gemm_pipe_kernel at 117K x 1152 x 384 fp16x3 (rag_bert_gemm variants 13-15):
// MFMAs + LDS reads + barriers 0.206 ms, DMAs alone 0.163 ms (~28 B/clk/CU of LDS-DMA intake),
// both 0.260 ms, + the epilogue stores 0.373 ms — the parts add instead of overlapping. Two
// couplings cause it: an LDS-DMA issue holds its wave for ~60-185 cycles (MI355X_MICROARCH
// price list), so the 6 DMAs every wave issued per step stalled the MFMA issue of both waves of
// a SIMD together (they leave the barrier in lockstep); and loads and stores share one
// in-order vmcnt, so a tile's stores had to complete before the next-but-one ring wait passed.
// Here the loader waves issue every DMA and wait only for DMAs (exact counts, no stores), and
// the MFMA waves issue only LDS reads, MFMAs and the epilogue's stores and never wait on
// vmcnt. One s_barrier per K step is the hand-off: the loaders pass it once stage g has
// landed, the MFMA waves once they are done reading stage g-1 (whose slot the loaders refill
// right after it). 12 waves: 3 per SIMD, <= 168 VGPRs each (the MFMA path needs ~145).
// ----------------------------------------------------------------------------------------
// block size of a gemm_ws_kernel instance: the MFMA waves plus one wave per loader
// (launch_fixed; its __launch_bounds__)
template <typename CFG> constexpr int kWsBlock = CFG::THREADS + 64 * CFG::LOADERS;

// PROBE (diagnostic timing probes of the forward's large-batch GEMM, rag_bert_gemm variants
// RAG_GEMM_WS_NO_STORE / _MFMA_ONLY / _DMA_ONLY; results meaningless): 6 = the epilogue without
// its stores, 7 = no DMAs and no stores (MFMAs, LDS reads and barriers only), 8 = no MFMAs and
// no stores (the DMA ring alone). The other round 2-4 probes and A/B forms of this kernel are
// gone (round 5); their measurements are in DESIGN.md.
template <int EPI, bool SPLIT, typename CFG, int PROBE = 0, int AUX = 0>
__global__ __launch_bounds__(kWsBlock<CFG>, 1) void gemm_ws_kernel(
    const _Float16* __restrict__ A, const _Float16* __restrict__ Al,
    const _Float16* __restrict__ W, const _Float16* __restrict__ Wl,
    const float* __restrict__ bias, int M, int N, int K, void* __restrict__ Cout,
    _Float16* __restrict__ Clo, DlArgs dl) {
  static_assert(EPI != kEpiAddLn && CFG::PRELOAD, "plain / deferred-LN epilogues, large tiles");
  static_assert(PROBE == 0 || PROBE == 6 || PROBE == 7 || PROBE == 8, "probe");
  constexpr bool DL = EPI == kEpiLnF16 || EPI == kEpiLnGeluF16 || EPI == kEpiResLn;
  static_assert(!DL || SPLIT, "deferred LayerNorm: fp16x3 only");
  constexpr int BM = CFG::BM, BN = CFG::BN, NS = CFG::NS, TH = CFG::THREADS;
  constexpr int LTH = 64 * CFG::LOADERS;            // loader threads
  constexpr int FM = CFG::FM, FN = CFG::FN, WTM = 16 * FM, WTN = 16 * FN;
  constexpr int BK = CFG::BK ? CFG::BK : kBK<SPLIT>, CPR = BK / 8, KSN = BK / 32;
  constexpr int NPL = SPLIT ? 2 : 1;
  constexpr int A_H8 = BM * CPR, W_H8 = BN * CPR;
  constexpr int STAGE_H8 = NPL * (A_H8 + W_H8);
  constexpr int LA = A_H8 / LTH, LW = W_H8 / LTH;  // DMAs per loader wave per plane
  constexpr int L = NPL * (LA + LW);               // DMAs per loader wave per stage
  constexpr bool P_NO_MFMA = PROBE == 8;
  constexpr bool P_NO_DMA = PROBE == 7;
  constexpr bool P_NO_STORE = PROBE == 6 || PROBE == 7 || PROBE == 8;
  constexpr int OUT_B = EPI == kEpiF32 ? 4 : 2;
  static_assert(A_H8 % LTH == 0 && W_H8 % LTH == 0 && FN % 2 == 0, "tile shape");
  static_assert((NS - 2) * (L + 1) <= 63, "vmcnt range");
  __shared__ half8 lds[NS * STAGE_H8 + kPipeBiasMax / 4];
  float* bias_l = reinterpret_cast<float*>(lds + NS * STAGE_H8);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lbase = lds_addr_of(lds);
  const int nN = N / BN, nM = (M + BM - 1) / BM;
  const int nk = K / BK;
  // Panel-aligned XCD placement (from 64 row panels up): workgroups b and b + 8 share an XCD
  // (round-robin dealing), so XCD x = b & 7 owns the A row panels x, x + 8, x + 16, ... and its
  // G / 8 workgroups walk those panels' tiles n-fastest with the K steps in the same order:
  // every n-tile of a panel runs on one XCD at about the same time and takes each K slice from
  // its L2 while the first reader's fetch is still there. FETCH_SIZE at 117K tokens fp16x3, per
  // algorithmic byte, QKV / FFN1 / O / FFN2: 2.15 / 2.94 / 1.46 / 1.25 with 32 consecutive
  // tiles per XCD (panels straddling two XCDs) and the rotated K order, 1.55 / 1.76 / 1.19 /
  // 1.22 aligned (time unchanged: the DMA intake per CU, not HBM, bounds these). Below 64
  // panels the XCDs' panel counts differ by up to 1/8, so the tiles are dealt evenly instead
  // (32 consecutive per XCD per round, rotated K order: 14.8K tokens 0.190 vs 0.244 ms).
  const int G = gridDim.x, per_xcd = G >> 3;    // G: a multiple of 8 (launcher)
  const int xcd = blockIdx.x & 7, lx = blockIdx.x >> 3;
  const bool aligned = nM >= 64;
  const int t_x = aligned ? (nM > xcd ? (nM - xcd + 7) >> 3 : 0) * nN : nM * nN;
  const int l0 = aligned ? lx : xcd * per_xcd + lx, stride = aligned ? per_xcd : G;
  // Split last round (aligned mode): when the XCD's last round of tiles would leave more
  // than half of its workgroups idle (r_x <= stride / 2 tiles), each of those r_x tiles runs
  // as two 128-row halves on two workgroups, so the round ends after a half tile instead of a
  // full one. A half tile keeps the 256-row ring image (rows past its 128 read as zeros
  // through the A panel's extent, so no bytes move for them); the MFMA waves of the upper
  // rows skip their MFMAs and stores (round 2: one layer at 117K tokens 1.252 / 1.247 vs
  // 1.263 / 1.273 ms without).
  const int r_x = aligned ? t_x % stride : 0;
  const bool halves = aligned && r_x > 0 && 2 * r_x <= stride;
  const int n_full = halves ? t_x / stride : l0 < t_x ? (t_x - l0 + stride - 1) / stride : 0;
  const int n_mine = n_full + (halves && lx < 2 * r_x ? 1 : 0);
  const int steps = n_mine * nk;
  // tile `it`: rows [m0, m_end) (m_end <= M) and n-tile nt
  auto tile_mn = [&](int it, int& m0, int& nt, int& m_end) __attribute__((always_inline)) {
    if (it < n_full) {
      const int t = it * stride + l0;
      m0 = (aligned ? xcd + 8 * (t / nN) : t / nN) * BM;
      nt = t % nN;
      m_end = min(M, m0 + BM);
    } else {                                  // the half tile of the split last round
      const int t = n_full * stride + (lx >> 1);
      m0 = (xcd + 8 * (t / nN)) * BM + (lx & 1) * (BM / 2);
      nt = t % nN;
      m_end = min(M, m0 + BM / 2);
    }
  };

  for (int i = tid * 4; i < N; i += (TH + LTH) * 4) {
    *reinterpret_cast<floatx4*>(bias_l + i) = *reinterpret_cast<const floatx4*>(bias + i);
    if constexpr (EPI == kEpiLnF16 || EPI == kEpiLnGeluF16)
      *reinterpret_cast<floatx4*>(bias_l + N + i) = *reinterpret_cast<const floatx4*>(dl.c1 + i);
    if constexpr (EPI == kEpiResLn)
      if (dl.st_in) {
        *reinterpret_cast<floatx4*>(bias_l + N + i) = *reinterpret_cast<const floatx4*>(dl.gamma + i);
        *reinterpret_cast<floatx4*>(bias_l + 2 * N + i) = *reinterpret_cast<const floatx4*>(dl.beta + i);
      }
  }
  __syncthreads();

  if (wid >= TH / 64) {
    // ---- loader waves: stage g+NS-1 issued after the barrier of step g ----
    const int lw = wid - TH / 64;
    uint32_t voA[LA], voW[LW];
#pragma unroll
    for (int i = 0; i < LA; ++i) voA[i] = dma_lane_offset<CPR>(lw * LA + i, lane, K);
#pragma unroll
    for (int i = 0; i < LW; ++i) voW[i] = dma_lane_offset<CPR>(lw * LW + i, lane, K);
    int it_i = 0, kt_i = 0, kr_i = 0, slot_i = 0;
    __amdgpu_buffer_rsrc_t rA0 = panel(A, 0), rA1 = rA0, rW0 = rA0, rW1 = rA0;
    auto issue_next = [&]() __attribute__((always_inline)) {
      if (it_i >= n_mine) return;
      if constexpr (P_NO_DMA) {
        if (++kt_i == nk) { kt_i = 0; ++it_i; }
        return;
      }
      if (kt_i == 0) {
        int m0, nt, m_end;
        tile_mn(it_i, m0, nt, m_end);
        const int n0 = nt * BN;
        kr_i = aligned ? 0 : nt % nk;   // rotated K order unless aligned
        const int64_t abytes = (int64_t)(m_end - m0) * K * 2, wbytes = (int64_t)BN * K * 2;
        rA0 = panel(A + (int64_t)m0 * K, abytes);
        rW0 = panel(W + (int64_t)n0 * K, wbytes);
        if constexpr (SPLIT) {
          rA1 = panel(Al + (int64_t)m0 * K, abytes);
          rW1 = panel(Wl + (int64_t)n0 * K, wbytes);
        }
      }
      const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)kr_i * (BK * 2));
      if (++kr_i == nk) kr_i = 0;
      const uint32_t slot = lbase + (uint32_t)slot_i * (STAGE_H8 * 16);
#pragma unroll
      for (int i = 0; i < LA; ++i) {
        const uint32_t d = slot + (uint32_t)((lw * LA + i) * 64 * 16);
        blds16(rA0, voA[i], soff, d);
        if constexpr (SPLIT) blds16(rA1, voA[i], soff, d + A_H8 * 16);
      }
#pragma unroll
      for (int i = 0; i < LW; ++i) {
        const uint32_t d = slot + (uint32_t)((NPL * A_H8 + (lw * LW + i) * 64) * 16);
        blds16(rW0, voW[i], soff, d);
        if constexpr (SPLIT) blds16(rW1, voW[i], soff, d + W_H8 * 16);
      }
      if (++kt_i == nk) { kt_i = 0; ++it_i; }
      if (++slot_i == NS) slot_i = 0;
    };
#pragma unroll
    for (int p = 0; p < NS - 1; ++p) issue_next();
    for (int g = 0; g < steps; ++g) {
      wait_ring<L, 0, NS - 2>(min(NS - 2, steps - 1 - g), false);   // stage g landed
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      issue_next();                     // stage g+NS-1 -> slot (g-1) % NS
    }
    return;
  }

  // ---- MFMA waves ----
  const int wr = wid / CFG::WAVES_N, wc = wid % CFG::WAVES_N;
  // (round 6 A/B builds, removed: static s_setprio 1 on MFMA waves 4-7, and s_setprio 1
  // around each step's MFMA chain — rerank forward 9.01-9.06 / 9.00-9.07 vs 8.98-9.04 ms,
  // chunk encode 3.16-3.17 / 3.16-3.18 vs 3.15-3.18: neutral; profiles/r06_ws_prio/. A
  // stagger — the odd workgroups owning a half tile ran it first, so their epilogue bursts
  // alternated with the others' MFMA phases — gave bitwise the same forward but 9.06-9.11 vs
  // 8.91-8.97 ms, chunk encode unchanged: a panel's n-tiles no longer ran on one XCD at the
  // same time to share its A slices in L2; profiles/r06_ws_stagger/)
  floatx4 acc[FM][FN] = {};
  int kt_c = 0, it_c = 0, slot_c = 0;
  half8 af[KSN][NPL][FM], wf[KSN][NPL][FN];
  // deferred LN: the current tile's row statistics, loaded right after the previous tile's
  // epilogue (a whole tile before they are used; loaded at the tile's first K step instead, the
  // compiler's waitcnt model put a vmcnt(0) there — a wait for the previous tile's stores)
  floatx4 dls[FM];
  auto prefetch = [&](int it) __attribute__((always_inline)) {
    if constexpr (DL) {
      if (dl.st_in && it < n_mine) {
        int m0, nt, m_end;
        tile_mn(it, m0, nt, m_end);
        const __amdgpu_buffer_rsrc_t rsi =
            panel(dl.st_in + (int64_t)m0 * kDlParts * 2, (int64_t)(m_end - m0) * kDlParts * 8);
        dl_prefetch_stats<FM>(dls, rsi, wr, lane);
      }
    }
  };
  prefetch(0);
  for (int g = 0; g < steps; ++g) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // done reading stage g-1
    __builtin_amdgcn_s_barrier();                        // stage g landed
    asm volatile("" ::: "memory");
    const half8* sa = lds + slot_c * STAGE_H8;
    const half8* sw = sa + NPL * A_H8;
    auto read_a = [&](int i) __attribute__((always_inline)) {   // (frag() moves the kernel)
#pragma unroll
      for (int ks = 0; ks < KSN; ++ks)
#pragma unroll
        for (int p = 0; p < NPL; ++p)
          af[ks][p][i] = sa[p * A_H8 + swz<CPR>(wr * WTM + i * 16 + (lane & 15), ks * 4 + (lane >> 4))];
    };
    // the upper-row MFMA waves of a half tile (split last round) have no rows: no reads,
    // MFMAs or stores (they still keep the ring's barriers)
    const bool idle = halves && it_c == n_full && wr >= CFG::WAVES_M / 2;
    if (!idle && !P_NO_MFMA) {
      // interleaved order: A_0, W_0..W_{FN-1}, A_1, ... read in the order the i-major MFMAs
      // consume them, with no barrier between the reads and the MFMAs, so the first MFMA
      // waits for 4 reads instead of 13 (all 8 waves issue their reads together after the
      // barrier; the LDS serves them interleaved). Round 2: 117K-token layer fp16x3 1.274 ->
      // 1.264 ms against all reads first (profiles/r02e_gemm_ilv.jsonl).
      read_a(0);
#pragma unroll
      for (int j = 0; j < FN; ++j)    // W_j's planes together: MFMA (0, j) needs 2 + 2j reads
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks)
#pragma unroll
          for (int p = 0; p < NPL; ++p)
            wf[ks][p][j] = sw[p * W_H8 + swz<CPR>(wc * WTN + j * 16 + (lane & 15), ks * 4 + (lane >> 4))];
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        if (i + 1 < FM) read_a(i + 1);
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            mma3<SPLIT>(acc[i][j], wf[ks][0][j], wf[ks][NPL - 1][j], af[ks][0][i],
                        af[ks][NPL - 1][i]);
      }
    }
    if (++slot_c == NS) slot_c = 0;
    if (++kt_c == nk) {               // tile done (stores never waited on)
      kt_c = 0;
      int m0, nt, m_end;
      tile_mn(it_c, m0, nt, m_end);
      ++it_c;
      const int n0 = nt * BN;
      const __amdgpu_buffer_rsrc_t rc = panel(static_cast<char*>(Cout) + (int64_t)m0 * N * OUT_B,
                                              (int64_t)(m_end - m0) * N * OUT_B);
      __amdgpu_buffer_rsrc_t rl = rc;
      if constexpr (SPLIT && EPI != kEpiF32)
        rl = panel(Clo + (int64_t)m0 * N, (int64_t)(m_end - m0) * N * 2);
      if (idle) {
        // no rows of this wave in the half tile
      } else if constexpr (DL) {
        const int64_t sb = (int64_t)(m_end - m0) * kDlParts * 8;
        const __amdgpu_buffer_rsrc_t rso = panel(dl.st_out + (int64_t)m0 * kDlParts * 2, dl.st_out ? sb : 0);
        ws_dl_epilogue<EPI, CFG, AUX>(acc, bias_l, rc, rl, dls, rso, dl.st_in != nullptr, N, n0,
                                      wr, wc, lane, dl.eps);
      } else {
        pipe_plain_epilogue<EPI, SPLIT, CFG, P_NO_STORE, AUX>(acc, bias_l, rc, rl, N, n0, wr, wc,
                                                              lane);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
      prefetch(it_c);
    }
  }
}

}  // namespace ragmi::bert
