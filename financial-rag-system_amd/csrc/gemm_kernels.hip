// gemm_kernels.hip — the encoder's GEMMs (included by bert_capi.hip after ln_kernels.hip): the
// tile GEMM gemm_kernel and the pipelined gemm_pipe_kernel with its epilogues (plain, and
// residual + LayerNorm over whole rows), launched by gemm and launch_pipe (gemm, gemm_add_ln).
namespace ragmi::bert {

#ifndef RAGMI_PIPE_PROBE
// build-time timing probe (ragmi/_build.py OUT.so -DRAGMI_PIPE_PROBE=n; results meaningless):
// 1 = no LDS reads / MFMAs in the query-batch tiles' K loop, 2 = no DMAs, 3 = neither
#define RAGMI_PIPE_PROBE 0
#endif
constexpr int kPipeProbe = RAGMI_PIPE_PROBE;

// ----------------------------------------------------------------------------------------
// GEMM: C[M,N] = A[M,K] . W[N,K]^T + bias[N]   (A fp16 row-major, W fp16 [N][K] = HF Linear)
// 128x128 tile, BK = 64 (fp16) / 32 (fp16x3), 256 threads = 2x2 waves of 64x64,
// v_mfma_f32_16x16x32_f16.
// Register-staged double-buffered LDS (one barrier per K step), XOR-swizzled 16-B chunks.
// ----------------------------------------------------------------------------------------
// kEpiAddLn (gemm_pipe_kernel<PipeRow> only): x = LN(x + A.W^T + bias) on whole rows
enum Epi { kEpiF16 = 0, kEpiGeluF16 = 1, kEpiF32 = 2, kEpiAddLn = 3 };

constexpr int BM = 128, BN = 128;

// K step: 64 for fp16 (2 planes: 64 KB double-buffered LDS), 32 for fp16x3 (4 planes, also
// 64 KB) so both modes fit two workgroups per CU.
template <bool SPLIT> constexpr int kBK = SPLIT ? 32 : 64;

template <int EPI, bool SPLIT>
__global__ __launch_bounds__(256) void gemm_kernel(const _Float16* __restrict__ A,
                                                   const _Float16* __restrict__ Al,
                                                   const _Float16* __restrict__ W,
                                                   const _Float16* __restrict__ Wl,
                                                   const float* __restrict__ bias, int M, int N,
                                                   int K, void* __restrict__ Cout,
                                                   _Float16* __restrict__ Clo) {
  // SPLIT (fp16x3): tiles of A_hi, A_lo, W_hi, W_lo; 3 MFMAs per product.
  constexpr int NP = SPLIT ? 4 : 2;                     // staged planes
  constexpr int BK = kBK<SPLIT>, CPR = BK / 8, LPT = BM * CPR / 256;   // loads/thread/plane
  // [buf][plane][row][CPR chunks]; also the epilogue's 4 x 32 x 68 fp32 staging (34 KB)
  constexpr int kLdsH8 = 2 * NP * BM * CPR > 4 * 32 * 68 / 4 ? 2 * NP * BM * CPR : 4 * 32 * 68 / 4;
  __shared__ half8 lds[kLdsH8];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  // XCD-aware tile order: blocks are dealt round-robin over the 8 XCDs, so XCD x runs
  // blocks x, x+8, ...; give it the contiguous tile range [x*cpx, (x+1)*cpx) with the N
  // tiles of one M tile adjacent, so the A panel is fetched into that XCD's L2 once and
  // reused by all N/BN column tiles (instead of once per XCD).
  const int nN = N / BN, nM = (M + BM - 1) / BM;
  const int cpx = gridDim.x >> 3;
  const int tile = (blockIdx.x & 7) * cpx + (blockIdx.x >> 3);
  if (tile >= nM * nN) return;
  const int m0 = (tile / nN) * BM, n0 = (tile % nN) * BN;
  const int nk = K / BK;
  const _Float16* src[4] = {A, W, Al, Wl};

  half8 rg[NP][LPT];
  auto gload = [&](int kt) {
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int i = 0; i < LPT; ++i) {
        const int c = tid + 256 * i;
        const int row = c / CPR, ch = c % CPR;
        const int r = (p & 1) ? (n0 + row) : min(m0 + row, M - 1);   // planes 0,2: A; 1,3: W
        rg[p][i] = *reinterpret_cast<const half8*>(src[p] + (int64_t)r * K + kt * BK + ch * 8);
      }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      half8* lp = lds + (buf * NP + p) * (BM * CPR);
#pragma unroll
      for (int i = 0; i < LPT; ++i) {
        const int c = tid + 256 * i;
        lp[swz<CPR>(c / CPR, c % CPR)] = rg[p][i];
      }
    }
  };

  floatx4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)   // (`= {}` as in the ring kernels moves this one)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    const half8* la = lds + (buf * NP + 0) * (BM * CPR);
    const half8* lb = lds + (buf * NP + 1) * (BM * CPR);
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      half8 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag<CPR>(la, wr * 64 + i * 16, ks, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) bf[j] = frag<CPR>(lb, wc * 64 + j * 16, ks, lane);
      if constexpr (SPLIT) {
        const half8* lal = lds + (buf * NP + 2) * (BM * CPR);
        const half8* lbl = lds + (buf * NP + 3) * (BM * CPR);
        half8 afl[4], bfl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) afl[i] = frag<CPR>(lal, wr * 64 + i * 16, ks, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) bfl[j] = frag<CPR>(lbl, wc * 64 + j * 16, ks, lane);
        // (not mma3: the lo terms of the whole tile are issued before its hi terms)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afl[i], bf[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bfl[j], acc[i][j], 0, 0, 0);
          }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) lstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue: lane holds C[rows 16i + 4(l>>4) + r][col 16j + (l&15)] of the wave's 64x64
  // tile. Stage 32-row halves through the (now idle) LDS as fp32 [32][68] per wave (stride
  // 68 dwords: the four 16-lane row groups land on disjoint banks), then each lane takes
  // 8 consecutive columns of a row: bias + activation + conversion there, and 16-B stores
  // (full 128-B row segments per 8 lanes) instead of 2-B scattered ones.
  constexpr int ES = 68;
  float* ep = reinterpret_cast<float*>(lds) + wid * (32 * ES);
  const int rr = lane >> 3, cc = (lane & 7) * 8;       // read: row rr + 8s, cols cc..cc+7
  const int gn = n0 + wc * 64 + cc;
  float bn[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bn[e] = bias[gn + e];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          ep[(i2 * 16 + 4 * (lane >> 4) + r) * ES + j * 16 + (lane & 15)] = acc[hf * 2 + i2][j][r];
    __builtin_amdgcn_s_waitcnt(0xc07f);                 // lgkmcnt(0): own LDS writes landed
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int s8 = 0; s8 < 4; ++s8) {
      const int lr = rr + 8 * s8;
      const int m = m0 + wr * 64 + hf * 32 + lr;
      const floatx4 lo4 = *reinterpret_cast<const floatx4*>(ep + lr * ES + cc);
      const floatx4 hi4 = *reinterpret_cast<const floatx4*>(ep + lr * ES + cc + 4);
      float v[8] = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[e] += bn[e];
        if constexpr (EPI == kEpiGeluF16) v[e] = gelu_erf(v[e]);
      }
      if (m < M) {
        if constexpr (EPI == kEpiF32) {
          float* o = static_cast<float*>(Cout) + (int64_t)m * N + gn;
          *reinterpret_cast<floatx4*>(o) = floatx4{v[0], v[1], v[2], v[3]};
          *reinterpret_cast<floatx4*>(o + 4) = floatx4{v[4], v[5], v[6], v[7]};
        } else {
          half8 h, l;
#pragma unroll
          for (int e = 0; e < 8; e += 2) {   // (not split_half4: it moves the fp16 instance)
            if constexpr (SPLIT) {
              half2 h2, l2;
              split16x2(v[e], v[e + 1], h2, l2);
              h[e] = h2[0]; h[e + 1] = h2[1]; l[e] = l2[0]; l[e + 1] = l2[1];
            } else {
              h[e] = (_Float16)v[e];
              h[e + 1] = (_Float16)v[e + 1];
            }
          }
          *reinterpret_cast<half8*>(static_cast<_Float16*>(Cout) + (int64_t)m * N + gn) = h;
          if constexpr (SPLIT) *reinterpret_cast<half8*>(Clo + (int64_t)m * N + gn) = l;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ----------------------------------------------------------------------------------------
// Persistent pipelined GEMM for large token counts (rerank batches, chunk encode):
// C[M,N] = A[M,K] . W[N,K]^T + bias, same epilogues as gemm_kernel.
//
// One 8-wave workgroup per CU loops over 256x128 output tiles (XCD-aware: in every round of
// gridDim.x tiles, the workgroups of one XCD take a contiguous tile range, so the N tiles of
// an A panel run on the same L2). K is short here (384 / 1024 / 1536), so a tile is only
// 6-24 K steps: a per-tile load prologue would expose one HBM latency per few hundred MFMA
// cycles. Instead the loads run on a flat (tile, k-step) sequence through a 3-stage LDS ring
// filled by direct buffer->LDS DMA (buffer_load_dwordx4 ... lds), two stages in flight,
// straight across tile boundaries — the next tile's first stages land while this tile's
// epilogue runs.
// Addressing is hoisted out of the loop: a tile's A and W panels are two buffer resources
// (wave-uniform SGPRs, rebuilt once per tile; A's extent ends at row M, so rows past M read
// as zeros), every lane's byte offset inside a panel is a launch constant (the XOR swizzle of
// the LDS image is applied to it), and a K step only moves the scalar soffset. A step costs
// 6 DMAs + their M0 writes besides its 32 (fp16) / 48 (fp16x3) MFMAs and 16 ds_read_b128.
// Sync per K step: counted `s_waitcnt vmcnt` + one raw s_barrier (step g landed for every
// wave AND every wave is done reading step g-1, whose slot the next DMA reuses). Besides the
// DMAs the loop issues only the epilogue's stores, a fixed number S per tile (buffer stores
// bounded to the M x N output: rows past M are dropped by the range check, never by exec
// masking), so every vmcnt is exact.
// Operands are swapped in the MFMA (D = W . A^T): lane l holds C[m][n .. n+3] for
// m = row (l & 15) of the fragment and 4 consecutive features n, so the epilogue adds bias
// (staged in LDS once per launch), applies GELU and stores 8-B (fp16) / 16-B (fp32) vectors
// straight from registers; the LDS stays the ring's.
// ----------------------------------------------------------------------------------------
// Two shapes of the same kernel (PipeCfg): LARGE — 256x128 tiles, 8 waves of 64x64, 3-stage
// ring, one workgroup per CU, persistent (rerank / chunk-encode token counts); SMALL —
// 64x64 tiles, 4 waves of 32x32, a 4-stage ring (fp16: the whole K = 384 of a tile in
// flight after the prologue), for query batches of a few hundred to a few thousand tokens,
// where a GEMM is a handful of tiles per CU and latency, not MFMA rate, sets its time.
constexpr int kPipeBiasMax = 4096;            // floats of bias staged in LDS (N <= 4096)
template <int BM_, int BN_, int WAVES_M_, int WAVES_N_, int NS_, int BK_ = 0, int LOADERS_ = 4,
          int BIAS_ = kPipeBiasMax>
struct PipeCfg {
  static constexpr int BM = BM_, BN = BN_, WAVES_M = WAVES_M_, WAVES_N = WAVES_N_, NS = NS_;
  static constexpr int BIAS = BIAS_;   // gemm_pipe_kernel's staged-vector area (floats)
  static constexpr int BK = BK_;   // K step; 0 = kBK<SPLIT> (64 fp16 / 32 fp16x3)
  static constexpr int LOADERS = LOADERS_;   // gemm_ws_kernel's loader waves
  static constexpr int THREADS = 64 * WAVES_M * WAVES_N;
  static constexpr int FM = BM / WAVES_M / 16, FN = BN / WAVES_N / 16;   // 16x16 frags/wave
  // a K step's fragments all loaded before its MFMAs (the large tiles; see the main loop)
  static constexpr bool PRELOAD = BM * BN >= 256 * 128;
};
using PipeLarge = PipeCfg<256, 128, 4, 2, 3>;
// whole 384-wide rows per tile (bge-small / MiniLM hidden size): the output projections with
// residual + LayerNorm fused into the epilogue (kEpiAddLn); 2 x 4 waves of 64 x 96
using PipeRow = PipeCfg<128, 384, 2, 4, 2>;
// (fp16x3: a 3-stage ring, 64 KB with the staged vectors, two workgroups per CU. Round 5
// A/B builds: 4 stages (2 per CU) and 6 / 8 stages (1 per CU, for GEMMs whose units fit the
// CUs) each ran the 32-query bge-small forward slower, 0.69 -> 0.71 / 0.72 / 0.73 ms, and
// config 2 at 72.6-74.5K -> 71.0-71.2K / 64.8-65.4K / 64.1K qps: a K step's time there is not
// the ring's latency; profiles/r05b_small_ring_depth_ab.jsonl)
// (wave grid, round 5 A/B builds: 2 x 1 / 1 x 2 / 1 x 1 waves of 32 x 64 / 64 x 32 / 64 x 64
// ran the 32-query forward in 0.757 / 0.762 / 0.99 ms vs 0.675 for 2 x 2 — fewer LDS fragment
// reads per step, but fewer waves to issue them; profiles/r05i_small_wave_grid_ab.jsonl)
template <bool SPLIT> using PipeSmall = PipeCfg<64, 64, 2, 2, SPLIT ? 3 : 4>;
// (Measured and removed in round 5 — numbers in DESIGN.md §R5: 256x256 / 256x192 PIPE tiles,
// register-blocked BIG / BIG128 shapes, BK-64 and 64x128 query-batch tiles, the one-loader and
// deferred-LN query-batch WS tiles, and the 256x192 ping-pong kernel.)
// fp16x3 query-batch GEMMs with N <= 2048 (round 6): a 2-stage ring and an 8 KB staged-vector
// area, 40 KB of LDS — four workgroups per CU instead of two, room for the config-2
// pipeline's concurrent batches. Bitwise the same outputs (same tiles, K order and epilogue);
// the 32-query forward alone 0.694 -> 0.704 ms, config 2 77.4-80.6K -> 80.0-81.5K qps over
// five interleaved pairs, config 3 unchanged (profiles/r06_small_ring/). Wider N (bge-large's
// 3072 / 4096) keeps PipeSmall<true>.
using PipeSmallR2 = PipeCfg<64, 64, 2, 2, 2, 0, 4, 2048>;
constexpr int PBM = PipeLarge::BM, PBN = PipeLarge::BN;
constexpr int kPipeThreads = PipeLarge::THREADS;

// fp16 out: fragments j, j+1 of a row pair up through one v_permlane16_swap per dword
// (lanes 16-31 of the j value <-> lanes 0-15 of the j+1 value, same for 48-63 / 32-47), after
// which every lane holds 8 consecutive columns: 16-B stores, half the store instructions of
// 8-B ones (the epilogue is store-issue-bound). Lane group g = lane >> 4 then owns columns
// 16 j + {0, 16, 8, 24}[g] .. +7 (byte offset vo).
template <int AUX = 0>
__device__ __forceinline__ void store_f16_pair(half4 xa, half4 xb, __amdgpu_buffer_rsrc_t rsc,
                                               int vo, int so = 0) {
  u32x2 a = __builtin_bit_cast(u32x2, xa), b = __builtin_bit_cast(u32x2, xb);
  const auto r0 = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
  const auto r1 = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
  const u32x4 d = {r0[0], r1[0], r0[1], r1[1]};
  __builtin_amdgcn_raw_buffer_store_b128(d, rsc, vo, so, AUX);
}

// the plain epilogues (kEpiF16 / kEpiGeluF16 / kEpiF32) of one wave's FM x FN accumulator
// fragments of the tile at column n0 (rc / rl: the output panels from the tile's row m0):
// bias (staged in LDS), GELU, then fp32 16-B stores or fp16 [+ lo plane] paired 16-B stores
// straight from registers — exactly pipe_plain_stores<EPI, SPLIT, CFG>() stores per wave (the
// ring's vmcnt accounting counts them). NO_STORE: timing probe, nothing written. AUX: the
// stores' cache policy (buffer-op aux bits; 2 = nt).
template <int EPI, bool SPLIT, typename CFG>
constexpr int pipe_plain_stores() {
  return EPI == kEpiF32 ? CFG::FM * CFG::FN : CFG::FM * CFG::FN / 2 * (SPLIT ? 2 : 1);
}

// one fragment pair (i, jp), (i, jp + 1) of it
template <int EPI, bool SPLIT, typename CFG, bool NO_STORE, int AUX = 0>
__device__ __forceinline__ void pipe_epi_pair(const floatx4& a0, const floatx4& a1, int i, int jp,
                                              const float* bias_l, __amdgpu_buffer_rsrc_t rc,
                                              __amdgpu_buffer_rsrc_t rl, int N, int n0, int wr,
                                              int wc, int lane) {
  constexpr int WTM = 16 * CFG::FM, WTN = 16 * CFG::FN;
  const int g = lane >> 4;
  const int ml = wr * WTM + i * 16 + (lane & 15);
  if constexpr (EPI == kEpiF32) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int nl = wc * WTN + (jp + h) * 16 + 4 * g;
      const floatx4 v = (h ? a1 : a0) + *reinterpret_cast<const floatx4*>(bias_l + n0 + nl);
      if (!NO_STORE || v[0] == 1234.5f)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rc,
                                               (ml * N + n0 + nl) * 4, 0, AUX);
    }
  } else {
    // fp16 out, two fragments per 16-B store (store_f16_pair)
    const int cofs = 8 * ((g & 1) * 2 + (g >> 1));
    const floatx4 b0 = *reinterpret_cast<const floatx4*>(bias_l + n0 + wc * WTN + jp * 16 + 4 * g);
    const floatx4 b1 = *reinterpret_cast<const floatx4*>(bias_l + n0 + wc * WTN + jp * 16 + 16 + 4 * g);
    const int vo = (ml * N + n0 + wc * WTN + jp * 16 + cofs) * 2;
    floatx4 va = a0 + b0, vb = a1 + b1;
    if constexpr (EPI == kEpiGeluF16) {
      va = gelu_erf4(va);
      vb = gelu_erf4(vb);
    }
    half4 ha, hb, la, lb;
    // (not split_half4: the two fragments' conversions interleave; folding moves hot kernels)
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      if constexpr (SPLIT) {
        half2 h2, l2;
        split16x2(va[r], va[r + 1], h2, l2);
        ha[r] = h2[0]; ha[r + 1] = h2[1]; la[r] = l2[0]; la[r + 1] = l2[1];
        split16x2(vb[r], vb[r + 1], h2, l2);
        hb[r] = h2[0]; hb[r + 1] = h2[1]; lb[r] = l2[0]; lb[r + 1] = l2[1];
      } else {
        ha[r] = (_Float16)va[r];
        ha[r + 1] = (_Float16)va[r + 1];
        hb[r] = (_Float16)vb[r];
        hb[r + 1] = (_Float16)vb[r + 1];
      }
    }
    if (!NO_STORE || va[0] == 1234.5f) store_f16_pair<AUX>(ha, hb, rc, vo);
    if constexpr (SPLIT)
      if (!NO_STORE || vb[0] == 1234.5f) store_f16_pair<AUX>(la, lb, rl, vo);
  }
}

template <int EPI, bool SPLIT, typename CFG, bool NO_STORE, int AUX = 0>
__device__ __forceinline__ void pipe_plain_epilogue(const floatx4 (&acc)[CFG::FM][CFG::FN],
                                                    const float* bias_l,
                                                    __amdgpu_buffer_rsrc_t rc,
                                                    __amdgpu_buffer_rsrc_t rl, int N, int n0,
                                                    int wr, int wc, int lane) {
#pragma unroll
  for (int jp = 0; jp < CFG::FN; jp += 2)
#pragma unroll
    for (int i = 0; i < CFG::FM; ++i)
      pipe_epi_pair<EPI, SPLIT, CFG, NO_STORE, AUX>(acc[i][jp], acc[i][jp + 1], i, jp, bias_l, rc,
                                                   rl, N, n0, wr, wc, lane);
}

// kEpiAddLn operands besides the GEMM's (Cout = the fp32 residual rows x, read and
// overwritten; Clo = the lo plane of the fp16x3 copy)
struct LnArgs {
  const float* gamma = nullptr;
  const float* beta = nullptr;
  _Float16* xh = nullptr;       // fp16 copy of the normalised rows (the next GEMM's A)
  float eps = 0.f;
};

// block size of a gemm_pipe_kernel instance (launch_fixed; its __launch_bounds__)
template <typename CFG> constexpr int kPipeBlock = CFG::THREADS;

template <int EPI, bool SPLIT, typename CFG>
__global__ __launch_bounds__(kPipeBlock<CFG>, 1) void gemm_pipe_kernel(
    const _Float16* __restrict__ A, const _Float16* __restrict__ Al,
    const _Float16* __restrict__ W, const _Float16* __restrict__ Wl,
    const float* __restrict__ bias, int M, int N, int K, void* __restrict__ Cout,
    _Float16* __restrict__ Clo, LnArgs ln, int ksplit = 1) {
  constexpr int BM = CFG::BM, BN = CFG::BN, NS = CFG::NS, TH = CFG::THREADS;
  constexpr int FM = CFG::FM, FN = CFG::FN, WTM = 16 * FM, WTN = 16 * FN;
  constexpr int BK = CFG::BK ? CFG::BK : kBK<SPLIT>, CPR = BK / 8;
  constexpr int NPL = SPLIT ? 2 : 1;                     // planes per operand (hi[, lo])
  constexpr int A_H8 = BM * CPR, W_H8 = BN * CPR;        // half8 per plane per stage
  constexpr int STAGE_H8 = NPL * (A_H8 + W_H8);
  constexpr int LA = A_H8 / TH, LW = W_H8 / TH;          // DMAs per wave per plane
  constexpr int L = NPL * (LA + LW);                      // DMAs per wave per stage
  // epilogue stores per wave: 16 B each; fp16 outputs pair two fragments per store
  // (kEpiAddLn: the fp32 rows and the fp16 copy [+ lo plane], 8-B stores for the latter).
  // The count is capped at what vmcnt can express: waiting until fewer ops are outstanding
  // than were issued after the awaited stage is only stricter.
  constexpr int S_ISSUED = EPI == kEpiF32   ? FM * FN
                           : EPI == kEpiAddLn ? FM * FN * (SPLIT ? 3 : 2)
                                              : FM * FN / 2 * (SPLIT ? 2 : 1);
  constexpr int S = S_ISSUED < 63 - (NS - 2) * L ? S_ISSUED : 63 - (NS - 2) * L;
  constexpr int OUT_B = EPI == kEpiF32 || EPI == kEpiAddLn ? 4 : 2;   // Cout element bytes
  static_assert(A_H8 % TH == 0 && W_H8 % TH == 0 && FN % 2 == 0, "tile shape");
  static_assert((NS - 2) * L + S <= 63, "vmcnt range");
  // kEpiAddLn keeps bias | gamma | beta | two [WAVES_N][BM] row-sum tables in the bias area
  static_assert(EPI != kEpiAddLn || 3 * BN + 2 * CFG::WAVES_N * BM <= CFG::BIAS,
                "LN staging");
  // one LDS object (ring | bias): a second __shared__ object beside a DMA target can make
  // hipcc drain vmcnt before every ds_read
  __shared__ half8 lds[NS * STAGE_H8 + CFG::BIAS / 4];
  float* bias_l = reinterpret_cast<float*>(lds + NS * STAGE_H8);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid / CFG::WAVES_N, wc = wid % CFG::WAVES_N;
  const uint32_t lbase = lds_addr_of(lds);
  // split-K (kEpiF32 only; the launcher checks K / BK % ksplit == 0 and N <= CFG::BIAS / 2):
  // work unit u = (tile u % n_tiles, K part u / n_tiles) over nk = K / BK / ksplit K steps;
  // part p writes its fp32 partial product to Cout + p M N, the bias only in part 0 (the
  // other parts read zeros staged in the upper half of the bias area); add_ln_kernel sums
  // the parts in order
  const int nN = N / BN, nM = (M + BM - 1) / BM, n_tiles = nM * nN;
  const int nk = K / BK / ksplit;
  const int n_units = n_tiles * ksplit;
  const int G = gridDim.x, per_xcd = G >> 3;
  const int off = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  const int n_mine = off < n_units ? (n_units - off + G - 1) / G : 0;
  const int steps = n_mine * nk;

  if (ksplit > 1)
    for (int i = tid * 4; i < N; i += TH * 4)
      *reinterpret_cast<floatx4*>(bias_l + CFG::BIAS / 2 + i) = floatx4{0.f, 0.f, 0.f, 0.f};
  // The staged vectors (bias [| gamma | beta]) are loaded into registers here and written to
  // LDS only after the ring prologue's DMAs are issued (below), so their load latency and the
  // first stages' run concurrently instead of back to back — a query-batch GEMM is one or two
  // tiles per workgroup, where that serial latency was a visible part of the launch.
  constexpr int NBV = CFG::BIAS / (TH * 4) > 0 ? CFG::BIAS / (TH * 4) : 1;
  constexpr int NLN = EPI == kEpiAddLn ? (BN + TH * 4 - 1) / (TH * 4) : 0;
  static_assert(NBV * TH * 4 >= CFG::BIAS, "every staged bias float has a register slot");
  floatx4 bv[NBV], gv[NLN > 0 ? NLN : 1], ev[NLN > 0 ? NLN : 1];
#pragma unroll
  for (int u = 0; u < NBV; ++u) {
    const int i = tid * 4 + u * TH * 4;
    if (i < N) bv[u] = *reinterpret_cast<const floatx4*>(bias + i);
  }
#pragma unroll
  for (int u = 0; u < NLN; ++u) {               // N == BN here (checked by the launcher)
    const int i = tid * 4 + u * TH * 4;
    if (i < N) {
      gv[u] = *reinterpret_cast<const floatx4*>(ln.gamma + i);
      ev[u] = *reinterpret_cast<const floatx4*>(ln.beta + i);
    }
  }
  auto stage_vectors = [&]() {
#pragma unroll
    for (int u = 0; u < NBV; ++u) {
      const int i = tid * 4 + u * TH * 4;
      if (i < N) *reinterpret_cast<floatx4*>(bias_l + i) = bv[u];
    }
#pragma unroll
    for (int u = 0; u < NLN; ++u) {
      const int i = tid * 4 + u * TH * 4;
      if (i < N) {
        *reinterpret_cast<floatx4*>(bias_l + BN + i) = gv[u];
        *reinterpret_cast<floatx4*>(bias_l + 2 * BN + i) = ev[u];
      }
    }
    __syncthreads();
  };

  // per-lane byte offsets inside a panel (launch constants) of this wave's DMA pieces
  uint32_t voA[LA], voW[LW];
#pragma unroll
  for (int i = 0; i < LA; ++i) voA[i] = dma_lane_offset<CPR>(wid * LA + i, lane, K);
#pragma unroll
  for (int i = 0; i < LW; ++i) voW[i] = dma_lane_offset<CPR>(wid * LW + i, lane, K);

  // issue side: next (tile iteration, k-step) to load, its panels and ring slot.
  // A tile's K steps run in a rotated order, starting at k-step (n-tile % nk): the nN tiles
  // that share an A panel (same XCD, same time) then touch different K slices of it at any
  // moment, so one of them takes each slice's L2 miss and the others hit, instead of all of
  // them waiting on the same HBM fetch at every step.
  int it_i = 0, kt_i = 0, kr_i = 0, slot_i = 0, kb_i = 0;
  __amdgpu_buffer_rsrc_t rA0 = panel(A, 0), rA1 = rA0, rW0 = rA0, rW1 = rA0;
  auto issue_next = [&]() {
    if (it_i >= n_mine) return;
    if (kt_i == 0) {
      const int unit = it_i * G + off;
      const int tile = unit % n_tiles;
      kb_i = (unit / n_tiles) * nk;
      const int m0 = (tile / nN) * BM, n0 = (tile % nN) * BN;
      kr_i = (tile % nN) % nk;
      const int64_t abytes = (int64_t)(M - m0) * K * 2, wbytes = (int64_t)BN * K * 2;
      rA0 = panel(A + (int64_t)m0 * K, abytes);
      rW0 = panel(W + (int64_t)n0 * K, wbytes);
      if constexpr (SPLIT) {
        rA1 = panel(Al + (int64_t)m0 * K, abytes);
        rW1 = panel(Wl + (int64_t)n0 * K, wbytes);
      }
    }
    // (wave-uniform by construction; readfirstlane keeps it an SGPR in every instance)
    const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)(kb_i + kr_i) * (BK * 2));
    if (++kr_i == nk) kr_i = 0;
    const uint32_t slot = lbase + (uint32_t)slot_i * (STAGE_H8 * 16);
#pragma unroll
    for (int i = 0; i < ((RAGMI_PIPE_PROBE & 2) ? 0 : LA); ++i) {
      const uint32_t d = slot + (uint32_t)((wid * LA + i) * 64 * 16);
      blds16(rA0, voA[i], soff, d);
      if constexpr (SPLIT) blds16(rA1, voA[i], soff, d + A_H8 * 16);
    }
#pragma unroll
    for (int i = 0; i < ((RAGMI_PIPE_PROBE & 2) ? 0 : LW); ++i) {
      const uint32_t d = slot + (uint32_t)((NPL * A_H8 + (wid * LW + i) * 64) * 16);
      blds16(rW0, voW[i], soff, d);
      if constexpr (SPLIT) blds16(rW1, voW[i], soff, d + W_H8 * 16);
    }
    if (++kt_i == nk) { kt_i = 0; ++it_i; }
    if (++slot_i == NS) slot_i = 0;
  };

  floatx4 acc[FM][FN] = {};

#pragma unroll
  for (int p = 0; p < NS - 1; ++p) issue_next();
  stage_vectors();
  int kt_c = 0, it_c = 0, slot_c = 0;
  for (int g = 0; g < steps; ++g) {
    // stages issued after step g: min(NS - 2, steps - 1 - g); plus the last epilogue's
    // stores when it ran at the end of step g-1
    wait_ring<L, S, NS - 2>(min(NS - 2, steps - 1 - g), g > 0 && kt_c == 0);
    __builtin_amdgcn_s_barrier();     // step g landed for all waves; all are past step g-1
    asm volatile("" ::: "memory");    // no LDS read of step g may be scheduled above it
    issue_next();                     // step g+NS-1 -> slot (g-1) % NS

    const half8* sa = lds + slot_c * STAGE_H8;
    const half8* sw = sa + NPL * A_H8;
    if constexpr (CFG::PRELOAD) {
      // every fragment of the K step issued back to back, then the MFMAs (left alone, the
      // compiler loads each fragment just before its first use and waits every few MFMAs;
      // this order measured ~3% faster on the 256-row tiles)
      constexpr int KSN = BK / 32;
      half8 af[KSN][NPL][FM], wf[KSN][NPL][FN];
#pragma unroll
      for (int ks = 0; ks < KSN; ++ks)
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
#pragma unroll
          for (int i = 0; i < FM; ++i)
            af[ks][p][i] = frag<CPR>(sa + p * A_H8, wr * WTM + i * 16, ks, lane);
#pragma unroll
          for (int j = 0; j < FN; ++j)
            wf[ks][p][j] = frag<CPR>(sw + p * W_H8, wc * WTN + j * 16, ks, lane);
        }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < KSN; ++ks)
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            mma3<SPLIT>(acc[i][j], wf[ks][0][j], wf[ks][NPL - 1][j], af[ks][0][i],
                        af[ks][NPL - 1][i]);
    }
#pragma unroll
    for (int ks = 0; ks < (CFG::PRELOAD || (kPipeProbe & 1) ? 0 : BK / 32); ++ks) {
      half8 af[FM], wf[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = frag<CPR>(sa, wr * WTM + i * 16, ks, lane);
#pragma unroll
      for (int j = 0; j < FN; ++j) wf[j] = frag<CPR>(sw, wc * WTN + j * 16, ks, lane);
      if constexpr (SPLIT) {
        half8 afl[FM], wfl[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) afl[i] = frag<CPR>(sa + A_H8, wr * WTM + i * 16, ks, lane);
#pragma unroll
        for (int j = 0; j < FN; ++j) wfl[j] = frag<CPR>(sw + W_H8, wc * WTN + j * 16, ks, lane);
        // (not mma3: the lo terms of the whole tile are issued before its hi terms)
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wfl[j], af[i], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], afl[i], acc[i][j], 0, 0, 0);
          }
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
    if (++slot_c == NS) slot_c = 0;

    if (++kt_c == nk) {               // tile done: epilogue from registers
      kt_c = 0;
      const int unit = it_c * G + off;
      const int tile = unit % n_tiles, kpart = unit / n_tiles;
      ++it_c;
      const int m0 = (tile / nN) * BM, n0 = (tile % nN) * BN;
      const int64_t cbytes = (int64_t)(M - m0) * N * OUT_B;
      const __amdgpu_buffer_rsrc_t rc =
          panel(static_cast<char*>(Cout) + ((int64_t)kpart * M + m0) * N * OUT_B, cbytes);
      __amdgpu_buffer_rsrc_t rl = rc;
      if constexpr (SPLIT && EPI != kEpiF32)
        rl = panel(Clo + (int64_t)m0 * N, (int64_t)(M - m0) * N * 2);
      if constexpr (EPI == kEpiAddLn) {
        // x = LN(x + acc + bias) over whole rows (BN == N, n0 = 0). Row statistics: a lane's
        // 4 FN values -> the 4 lane groups (shuffles) -> the WAVES_N waves of a row band (LDS
        // tables, one barrier each); two passes, mean then centred squares, as add_ln_kernel.
        // Every wave runs the same epilogues, so the extra barriers pair up across the
        // workgroup like the main loop's.
        const int g = lane >> 4;
        float* red = bias_l + 3 * BN;                      // [2][WAVES_N][BM]
        const float* gam = bias_l + BN;
        const float* bet = bias_l + 2 * BN;
        const __amdgpu_buffer_rsrc_t rh = panel(ln.xh + (int64_t)m0 * N, (int64_t)(M - m0) * N * 2);
        // Addressing: a per-lane byte offset per fragment row i (the row must sit in the
        // voffset: the buffer range check that drops rows past M ignores soffset) plus a
        // wave-uniform soffset per fragment column j — per-fragment lane offsets would be
        // hoisted out of the tile loop by the compiler and spilled (96 accumulators live).
        auto vf = [&](int i) { return ((wr * WTM + i * 16 + (lane & 15)) * N + 4 * g) * 4; };
        auto sf = [&](int j) { return (wc * WTN + j * 16) * 4; };
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const floatx4 bj = *reinterpret_cast<const floatx4*>(bias_l + wc * WTN + j * 16 + 4 * g);
#pragma unroll
          for (int i = 0; i < FM; ++i) {   // rows past M read as zeros (bounded panel)
            const u32x4 xr = __builtin_amdgcn_raw_buffer_load_b128(rc, vf(i), sf(j), 0);
            acc[i][j] += bj + __builtin_bit_cast(floatx4, xr);
          }
        }
        float mu[FM], rsd[FM];
#pragma unroll
        for (int i = 0; i < FM; ++i) mu[i] = rsd[i] = 0.f;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
          for (int i = 0; i < FM; ++i) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float d = acc[i][j][r] - mu[i];
                s = pass ? fmaf(d, d, s) : s + d;
              }
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (g == 0) red[(pass * CFG::WAVES_N + wc) * BM + wr * WTM + i * 16 + lane] = s;
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
#pragma unroll
          for (int i = 0; i < FM; ++i) {
            const int row = wr * WTM + i * 16 + (lane & 15);
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < CFG::WAVES_N; ++w) s += red[(pass * CFG::WAVES_N + w) * BM + row];
            if (pass == 0) mu[i] = s * (1.0f / BN);
            else rsd[i] = rsqrtf(s * (1.0f / BN) + ln.eps);
          }
        }
        // fp16 copy [+ lo plane]: 8-B stores straight from the fragment layout. (Paired 16-B
        // stores issue fewer stores than the 8-B count S; with S unchanged the next tile's
        // first ring stage was read before it landed: wrong dwords — round 2.)
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const floatx4 gj = *reinterpret_cast<const floatx4*>(gam + wc * WTN + j * 16 + 4 * g);
          const floatx4 ej = *reinterpret_cast<const floatx4*>(bet + wc * WTN + j * 16 + 4 * g);
#pragma unroll
          for (int i = 0; i < FM; ++i) {
            floatx4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (acc[i][j][r] - mu[i]) * rsd[i] * gj[r] + ej[r];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rc, vf(i),
                                                   sf(j), 0);
            half4 h, l;
            split_half4<SPLIT>(v, h, l);
            const int vh = vf(i) / 2;                  // same element offsets in fp16
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h), rh, vh,
                                                  sf(j) / 2, 0);
            if constexpr (SPLIT)
              __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, l), rl, vh,
                                                    sf(j) / 2, 0);
          }
        }
      } else {
        pipe_plain_epilogue<EPI, SPLIT, CFG, false>(
            acc, kpart ? bias_l + CFG::BIAS / 2 : bias_l, rc, rl, N, n0, wr, wc, lane);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

}  // namespace ragmi::bert
