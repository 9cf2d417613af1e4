// attn_kernels.hip — self-attention of the encoder forward (included by bert_capi.hip after
// gemm_ws_kernels.hip, whose deferred-LN statistics gather_cls_kernel reads): attn_kernel
// (launched by forward_t and rag_bert_attention), and gather_cls_kernel and attn_cls_kernel of
// the CLS-only last layer (forward_t).
namespace ragmi::bert {

// ----------------------------------------------------------------------------------------
// attention (varlen, one workgroup per (head, sequence), 8 waves (fp16) / 16 (fp16x3)).
// K and V of the sequence's keys are staged into LDS (all of them when they fit — always for
// head_dim 32, and for head_dim 64 up to ~288 keys in fp16x3 — else in chunks of kc keys),
// then every wave walks its own 16-query blocks over all key blocks of 32 with no further
// barriers.
// Transposed formulation keeps P in registers:
//   S^T[key][q] = K . Q^T   (A = K rows from LDS, B = Q^T fragments held for the block)
//   O^T[d][q]  += V^T . P^T (A = V^T rows from LDS, B = P^T = the lane's own S^T values)
// The MFMA C layout puts query q = lane&15 in every lane's column, so the softmax running
// max / sum and the O rescale are per-lane scalars; the P^T fragment slot 8g+j (g = lane>>4)
// holds key 4g+j (j<4) or 16+4g+(j-4) (j>=4) of the block, i.e. exactly the lane's two S^T
// accumulators. V stays row-major in LDS ([key][HD], 16-B copies from the Q|K|V rows) and
// the V^T fragment is gathered by two ds_read_b64_tr_b16 (gfx950 transposed LDS read: per
// 16-lane group, 4 rows x 16 columns delivered column-major): rows 4g..4g+3 and 16+4g..
// 16+4g+3 of the block — the P^T slot order, so no key permutation is stored anywhere.
// (Round 1 staged V^T with eight 2-byte LDS stores per 16-B chunk: SQ_LDS_BANK_CONFLICT
// 1.9e7 cycles per launch against 1.24e7 active LDS cycles at rerank size.)
// qkv: fp16 [T][3H] (Q | K | V; head h = columns h*HD .. +HD-1 of each); ctx: fp16 [T][H].
// LDS (dynamic) per plane: K [cap][HD] (16-B chunks swizzled as the GEMM images, swz_chunk)
// + V [cap][HD] (16-B chunk c of row r at c ^ attn_vsw(r), which spreads the 8 rows a 32-lane
// half reads over all 64 banks), cap = keys staged at once. Two fp16x3 workgroups share a CU
// up to ~300 keys.
// ----------------------------------------------------------------------------------------
template <bool SPLIT> constexpr int kAttnThreads = 512;   // 2 waves per SIMD per workgroup
constexpr int kAttnLdsMax = 160 * 1024;
// occupancy: head_dim 32 fp16 fits 64 VGPRs (8 waves per SIMD: four 8-wave workgroups per
// CU, LDS permitting) without spilling; head_dim 32 fp16x3 fits 128 (two workgroups per CU,
// so one stages its K/V while the other computes: rerank 10.33 -> 10.08 ms against 16-wave
// workgroups, one per CU); head_dim 64 is left unconstrained
template <int HD, bool SPLIT> constexpr int kAttnWavesPerEU = HD == 32 ? (SPLIT ? 4 : 8) : 1;

template <int HD>
__host__ __device__ constexpr int attn_lds_bytes(int cap, int planes) {
  return planes * 2 * cap * HD * 2;
}
// keys staged per chunk (multiple of 32): all of them if they fit, else the most that fit
template <int HD>
__host__ __device__ constexpr int attn_chunk_keys(int max_len, int planes) {
  const int sp = (max_len + 31) & ~31;
  int kc = sp;
  while (kc > 32 && attn_lds_bytes<HD>(kc, planes) > kAttnLdsMax) kc -= 32;
  return kc;
}

// V image chunk swizzle: a transposed read takes 32 B (16 columns) of each of 8 rows per
// 32-lane half (rows 4g + q, g = two groups); rows 128 / HD apart share a bank window, so the
// chunk pair is XORed by the row's window index
template <int HD>
__device__ __forceinline__ int attn_vsw(int r) {
  return ((r / (128 / HD)) & (HD / 16 - 1)) << 1;
}

template <int HD, bool SPLIT>
struct AttnState {
  static constexpr int DT = HD / 16, KS = HD / 32, NP = SPLIT ? 2 : 1;
  half8 qf[KS][NP];
  floatx4 o[DT];
  // row sums of P: fp16x3 by MFMA against a ones fragment (every element = l(q)); fp16 by
  // v_dot2 into l[0] (lane-partial, reduced across the lane groups at the end)
  floatx4 l;
  float m;
};

// VAR bit 512 (round 6, diagnostic build): the P scalings as scalar v_fma_f32 (fma_scalar)
// instead of the packed v_pk_fma_f32 of VPRE; bitwise the same values, measured neutral at the
// rerank shape (554: 0.2427-0.2436 ms vs 42: 0.2414-0.2428, profiles/r06_attn/): the loop is
// not bound by its vector issue.
// VAR (bit mask; rag_bert_attention A/Bs them): 1 = rolling Q prefetch, 2 = fp16x3 row sums
// by MFMA (else v_dot2), 4 = software-pipelined scores (block kb+1's K.Q^T MFMAs issued
// before block kb's softmax, so they run in the matrix pipe under its vector work), 8 = lean
// block (round 2): the block max by IEEE maximum (fmax_nc: no canonicalising v_max per MFMA
// result), the cross-lane max by v_permlane16/32_swap instead of two ds_bpermute
// round trips, P and O split by split16x2 (3 instead of 8 VALU per pair), and a block's V^T
// fragments read in one batch before its P.V MFMAs (one LDS wait instead of DT). Bitwise the
// same results as without it.
// Measured at the rerank shape (scripts/bench_attn.py, profiles/r02_attn_variants.jsonl):
// fp16x3 0.270-0.283 ms over all eight, 2 the fastest; fp16 0.140 ms without 4, 0.19-0.21
// with it (64-VGPR budget). The kernel's time is not in these (staging / latency bound).
// Bit 8 (profiles/r02e_lean_split.jsonl, same process): fp16x3 2 -> 10 0.281 -> 0.272 ms
// (the default since), fp16 unchanged (0.148 / 0.149: no split there).
// Bit 16 (two query blocks per wave side by side, bitwise the same; 114 VGPRs, no spill,
// same 4 waves per SIMD) measured slower at the rerank shape (profiles/r02q_attn_pairs.jsonl,
// same process, 7 rounds): 10 -> 26 0.254 -> 0.282 ms, 2 -> 18 0.268 -> 0.303: a diagnostic.
constexpr int kAttnVar = 42;
// rag_bert_attention's A/B slot in the production library: VAR 10 = 42 without the peeled,
// prefetched block loop (bitwise the same outputs, tests/test_attention_gpu.py)
constexpr int kAttnVarAB = 10;
// THREADS (round 6): 512 (8 waves) in general; 128 (2 waves) for query batches whose
// sequences are at most 32 tokens (2 query blocks, so 6 of 8 waves would only stage), which
// leaves the CUs' wave slots to the other batches in flight. A query block's arithmetic does
// not depend on which wave runs it: the outputs are bitwise the same.
template <int H, int HD, bool SPLIT, int VAR = kAttnVar, int THREADS = kAttnThreads<SPLIT>>
__global__ __launch_bounds__(THREADS, (kAttnWavesPerEU<HD, SPLIT>)) void attn_kernel(
    const _Float16* __restrict__ qkv, const _Float16* __restrict__ qkv_lo,
    const int* __restrict__ cu, int max_len, int kc, float scale, _Float16* __restrict__ ctx,
    _Float16* __restrict__ ctx_lo, int max_qb) {
  using St = AttnState<HD, SPLIT>;
  constexpr int NP = St::NP, KS = St::KS, DT = St::DT, KROW = HD, KCPR = HD / 8;
  constexpr int NW = THREADS / 64;
  extern __shared__ _Float16 alds[];
  // XCD-aware (sequence, head) order: blocks are dealt round-robin over the 8 XCDs, so give
  // XCD x a contiguous range of (sequence, head) pairs: the heads of one sequence run on one
  // XCD back to back and share the 128-B lines of the Q|K|V rows (64 B per head) in its L2
  // instead of each line being fetched once per head by different XCDs.
  constexpr int NH = H / HD;
  const int n_pairs = NH * (gridDim.x / NH);            // gridDim.x = NH * B rounded up to 8
  const int per_xcd = gridDim.x >> 3;
  const int pair = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (pair >= n_pairs) return;
  const int b = pair / NH, h = pair % NH;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // LDS was sized for max_len on the host: a longer sequence (a caller breaking the
  // max_len contract of rag_encoder_forward) is truncated rather than overrunning LDS
  const int base = cu[b], len = min(cu[b + 1] - cu[b], max_len);
  if (len <= 0) return;
  const int sp = (len + 31) & ~31;
  const int cap = min(sp, kc);                      // keys per staged chunk
  const int nch = (sp + cap - 1) / cap;
  _Float16* kls[2] = {alds, alds + 2 * cap * KROW};
  _Float16* vls[2] = {alds + cap * KROW, alds + 3 * cap * KROW};
  const _Float16* planes[2] = {qkv, qkv_lo};
  const int g = lane >> 4, ql = lane & 15;
  const float c2 = scale * 1.44269504088896341f;
  const float rescale_gap = 8.0f / c2;             // deferred-max threshold (score units)

  // ---- stage keys [k0, k0 + n) (n multiple of 32; zeros past len): K and V row-major,
  // 16-B chunks (swizzled: swz_chunk for K's row reads, attn_vsw for V's transposed reads)
  auto stage = [&](int k0, int n) {
    // timing probes (diagnostic build, round 6; results meaningless): VAR bit 256 = no staging
    // at all (LDS left as it is), bit 128 = zeros stored instead of the loaded K / V
    if constexpr ((VAR & 256) != 0) return;
    if constexpr ((VAR & 2048) != 0) {
      // VAR bit 2048 (round 6): the K / V images filled by LDS-DMA (buffer_load ... lds): one
      // wave-instruction writes 1 KB = 64 / KCPR whole rows, lane l to LDS chunk position
      // (row l / KCPR, chunk l % KCPR); the swizzles are XORs, so that position's source chunk
      // is the swizzle of the position. Rows past len read as zeros through the sequence's
      // buffer extent. No VGPR round trip, no ds_write; same bytes in the same LDS places.
      // Diagnostic build: bitwise 42's outputs but 0.342 vs 0.242 ms per rerank-shape launch
      // (profiles/r06_attn/r06n3_*) — each piece gathers 16 rows' 64-B segments 2,304 B apart.
      constexpr int RPP = 64 / KCPR;
      const int pieces = n / RPP, tot = NP * 2 * pieces;
      const int rl = lane / KCPR, q = lane % KCPR;
      __amdgpu_buffer_rsrc_t rs[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p)
        rs[p] = panel(planes[p] + (int64_t)base * (3 * H), (int64_t)len * (3 * H) * 2);
      const int wu = __builtin_amdgcn_readfirstlane(wid);   // piece indices wave-uniform
      for (int j = wu; j < tot; j += NW) {
        const int p = j / (2 * pieces), kv = (j / pieces) & 1, pc = j % pieces;
        const int r = pc * RPP + rl;
        const int ch = kv ? (q ^ attn_vsw<HD>(r)) : swz_chunk<KCPR>(r, q);
        const uint32_t voff =
            (uint32_t)((k0 + r) * (3 * H) + (kv ? 2 * H : H) + h * HD + 8 * ch) * 2u;
        const _Float16* dst = (kv ? vls[p] : kls[p]) + pc * RPP * KROW;
        blds16(p ? rs[NP - 1] : rs[0], voff, 0u,
               __builtin_amdgcn_readfirstlane(lds_addr_of(dst)));
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      return;
    }
    if constexpr ((VAR & 128) != 0) {
      for (int c = tid; c < n * (HD / 8); c += THREADS) {
        const int kl = c / (HD / 8), ch = c % (HD / 8);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          *reinterpret_cast<half8*>(kls[p] + kl * KROW + 8 * swz_chunk<KCPR>(kl, ch)) = half8{};
          *reinterpret_cast<half8*>(vls[p] + kl * HD + 8 * (ch ^ attn_vsw<HD>(kl))) = half8{};
        }
      }
      return;
    }
    if constexpr ((VAR & 64) != 0) {
      // VAR bit 64 (round 4): every staging load of up to SU passes issued before any LDS
      // store (one memory round trip per SU passes instead of one per pass); same bytes to
      // the same LDS places
      constexpr int SU = 2;
      constexpr int T = THREADS;
      const int total = n * (HD / 8);
      for (int c0 = tid; c0 < total; c0 += SU * T) {
        half8 kv[SU][NP], vv[SU][NP];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int c = c0 + u * T, kl = c / (HD / 8), ch = c % (HD / 8), key = k0 + kl;
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            kv[u][p] = half8{};
            vv[u][p] = half8{};
            if (c < total && key < len) {
              const _Float16* src = planes[p] + (int64_t)(base + key) * (3 * H) + h * HD + 8 * ch;
              kv[u][p] = *reinterpret_cast<const half8*>(src + H);
              vv[u][p] = *reinterpret_cast<const half8*>(src + 2 * H);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int c = c0 + u * T, kl = c / (HD / 8), ch = c % (HD / 8);
          if (c < total) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
              *reinterpret_cast<half8*>(kls[p] + kl * KROW + 8 * swz_chunk<KCPR>(kl, ch)) = kv[u][p];
              *reinterpret_cast<half8*>(vls[p] + kl * HD + 8 * (ch ^ attn_vsw<HD>(kl))) = vv[u][p];
            }
          }
        }
      }
      return;
    }
    for (int c = tid; c < n * (HD / 8); c += THREADS) {
      const int kl = c / (HD / 8), ch = c % (HD / 8), key = k0 + kl;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        half8 kv = {}, vv = {};
        if (key < len) {
          const _Float16* src = planes[p] + (int64_t)(base + key) * (3 * H) + h * HD + 8 * ch;
          kv = *reinterpret_cast<const half8*>(src + H);
          vv = *reinterpret_cast<const half8*>(src + 2 * H);
        }
        *reinterpret_cast<half8*>(kls[p] + kl * KROW + 8 * swz_chunk<KCPR>(kl, ch)) = kv;
        *reinterpret_cast<half8*>(vls[p] + kl * HD + 8 * (ch ^ attn_vsw<HD>(kl))) = vv;
      }
    }
  };
  // this lane's transposed-read offset (halves) for V^T fragment dt of a 32-key block at
  // row 0: lane 4q + pp of 16-lane group g supplies row 4g + q, columns 16 dt + 4 pp .. + 3
  // (the second read: rows + 16; the swizzle is the same for both and for every block)
  const int vq = (lane & 15) >> 2, vpp = lane & 3;
  auto voff = [&](int dt) {
    const int r = 4 * g + vq;
    return r * HD + 8 * ((2 * dt + (vpp >> 1)) ^ attn_vsw<HD>(r)) + 4 * (vpp & 1);
  };
  // the V^T fragment (plane p) at transposed-read offset vr: rows 4g .. 4g + 3 and 16 + 4g ..
  auto vfrag = [&](int p, int vr) {
    return __builtin_shufflevector(lds_read_tr16(vls[p] + vr),
                                   lds_read_tr16(vls[p] + vr + 16 * HD), 0, 1, 2, 3, 4, 5, 6, 7);
  };
  auto load_q = [&](half8 (&qf)[KS][NP], int qb) {
    const int r = min(qb * 16 + ql, len - 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int p = 0; p < NP; ++p)
        qf[ks][p] = *reinterpret_cast<const half8*>(
            planes[p] + (int64_t)(base + r) * (3 * H) + h * HD + 32 * ks + 8 * g);
  };
  auto reset = [&](St& st) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) st.o[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    st.l = floatx4{0.f, 0.f, 0.f, 0.f};
    st.m = kNegInf;
  };
  auto init = [&](St& st, int qb) {
    load_q(st.qf, qb);
    reset(st);
  };
  half8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (_Float16)1.0f;
  // S^T of the 32-key block at LDS position kb (terms hi first: not mma3's order)
  auto qk = [&](const St& st, int kb, floatx4 (&sc)[2]) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        sc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int krow = kb + 16 * j + ql;
          const int kr = krow * KROW + 8 * swz_chunk<KCPR>(krow, 4 * ks + g);
          const half8 kf = *reinterpret_cast<const half8*>(kls[0] + kr);
          sc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, st.qf[ks][0], sc[j], 0, 0, 0);
          if constexpr (SPLIT) {
            const half8 kfl = *reinterpret_cast<const half8*>(kls[1] + kr);
            sc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kfl, st.qf[ks][0], sc[j], 0, 0, 0);
            sc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, st.qf[ks][1], sc[j], 0, 0, 0);
          }
        }
      }
  };
  // softmax update and P.V for the block at LDS position kb (keys k0 + kb ..). mode (VAR bit
  // 32's peeled loop): 0 = is the block full? checked here; 1 = known full; 2 = known partial.
  // Bit 32 also issues the block's V^T fragment reads first, so their LDS latency runs under
  // the max / exp / split work instead of between the P.V MFMAs.
  auto softmax_pv_m = [&](St& st, int k0, int kb, floatx4 (&sc)[2], auto mode) {
      constexpr int MODE = decltype(mode)::value;
      constexpr bool VPRE = (VAR & 40) == 40;
      half8 vh[DT], vlo[DT];
      if constexpr (VPRE) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const int vr = kb * HD + voff(dt);
          vh[dt] = vfrag(0, vr);
          if constexpr (SPLIT) vlo[dt] = vfrag(1, vr);
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the reads ahead of the softmax
      }
      // lane: S^T[key k0 + kb + 16j + 4g + r][q]. Softmax in base 2 with the 1/sqrt(d) scale
      // folded into one FMA: p = 2^(s*c - m*c), c = scale*log2(e) > 0 (max commutes).
      float mx;
      if (MODE == 1 || (MODE == 0 && k0 + kb + 32 <= len)) {
        if constexpr ((VAR & 8) != 0)   // IEEE maximum: no per-input canonicalisation
          mx = fmax_nc(fmax_nc(fmax_nc(sc[0][0], sc[0][1]), fmax_nc(sc[0][2], sc[0][3])),
                       fmax_nc(fmax_nc(sc[1][0], sc[1][1]), fmax_nc(sc[1][2], sc[1][3])));
        else
          mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])),
                     fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
      } else {
        mx = kNegInf;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (k0 + kb + 16 * j + 4 * g + r >= len) sc[j][r] = kNegInf;
            mx = (VAR & 8) != 0 ? fmax_nc(mx, sc[j][r]) : fmaxf(mx, sc[j][r]);
          }
      }
      if constexpr ((VAR & 8) != 0) {
        // lanes l, l^16, l^32, l^48 hold the same query's other keys
        const uint32_t mu = __builtin_bit_cast(uint32_t, mx);
        const auto r16 = __builtin_amdgcn_permlane16_swap(mu, mu, false, false);
        mx = fmax_nc(__builtin_bit_cast(float, (uint32_t)r16[0]),
                     __builtin_bit_cast(float, (uint32_t)r16[1]));
        const uint32_t mu2 = __builtin_bit_cast(uint32_t, mx);
        const auto r32 = __builtin_amdgcn_permlane32_swap(mu2, mu2, false, false);
        mx = fmax_nc(__builtin_bit_cast(float, (uint32_t)r32[0]),
                     __builtin_bit_cast(float, (uint32_t)r32[1]));
      } else {
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      }
      // Deferred rescale: the running max only moves when some query's block max exceeds it
      // by more than 8 / c2 (P = 2^(s c2 - m c2) then stays <= 2^8, exact in the fp16 MFMA
      // operand and far from its range limit); otherwise the old max is kept and the
      // rescale of l and O (an exp2 and DT*4 + 1 multiplies per block) is skipped. The
      // normalisation divides by l summed from the same P, so the result is unchanged up to
      // rounding. Wave-uniform branch (ballot).
      if (__builtin_amdgcn_ballot_w64(mx > st.m + rescale_gap)) {
        const float mnew = fmaxf(st.m, mx);
        const float corr = __builtin_amdgcn_exp2f((st.m - mnew) * c2);
#pragma unroll
        for (int r = 0; r < 4; ++r) st.l[r] *= corr;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) st.o[dt][r] *= corr;
        st.m = mnew;
      }
      const float nm = -st.m * c2;
      half8 ph, pl = {};   // (pl: read by fp16x3 only)
      if constexpr (SPLIT && (VAR & 8) != 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; r += 2) {
            float e0, e1;
            if constexpr ((VAR & 512) != 0) {   // two scalar FMAs, never paired into a
              e0 = __builtin_amdgcn_exp2f(fma_scalar(sc[j][r], c2, nm));   // v_pk_fma_f32
              e1 = __builtin_amdgcn_exp2f(fma_scalar(sc[j][r + 1], c2, nm));
            } else if constexpr (VPRE) {   // the two scalings as one packed fp32 FMA (v_pk_fma_f32)
              typedef float f2 __attribute__((ext_vector_type(2)));
              const f2 t = __builtin_elementwise_fma(f2{sc[j][r], sc[j][r + 1]}, f2{c2, c2},
                                                     f2{nm, nm});
              e0 = __builtin_amdgcn_exp2f(t[0]);
              e1 = __builtin_amdgcn_exp2f(t[1]);
            } else {
              e0 = __builtin_amdgcn_exp2f(fmaf(sc[j][r], c2, nm));
              e1 = __builtin_amdgcn_exp2f(fmaf(sc[j][r + 1], c2, nm));
            }
            half2 h2, l2;
            split16x2(e0, e1, h2, l2);
            ph[4 * j + r] = h2[0]; ph[4 * j + r + 1] = h2[1];
            pl[4 * j + r] = l2[0]; pl[4 * j + r + 1] = l2[1];
          }
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(fmaf(sc[j][r], c2, nm));
            if constexpr (SPLIT) { const half2 s16_ = split16(e); ph[4 * j + r] = s16_[0]; pl[4 * j + r] = s16_[1]; }
            else ph[4 * j + r] = (_Float16)e;
          }
      }
      // row sum of P exactly as the MFMA sees it (hi [+ lo]). fp16x3: the same MFMA against
      // a ones fragment (the MFMA pipe has the slack there, the vector ALU does not: 2 MFMAs
      // for 8 v_dot2, and every lane ends up with its query's whole sum); fp16: v_dot2 (the
      // 64-VGPR budget of 8 waves per SIMD has no room for the fragment and accumulator)
      if constexpr (SPLIT && (VAR & 2)) {
        st.l = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pl, st.l, 0, 0, 0);
        st.l = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, ph, st.l, 0, 0, 0);
      } else {
        const half2 one2 = {(_Float16)1.0f, (_Float16)1.0f};
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          st.l[0] = __builtin_amdgcn_fdot2(half2{ph[2 * e2], ph[2 * e2 + 1]}, one2, st.l[0], false);
          if constexpr (SPLIT)
            st.l[0] = __builtin_amdgcn_fdot2(half2{pl[2 * e2], pl[2 * e2 + 1]}, one2, st.l[0], false);
        }
      }
      if constexpr ((VAR & 8) != 0) {
        if constexpr (!VPRE) {
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const int vr = kb * HD + voff(dt);
            vh[dt] = vfrag(0, vr);
            if constexpr (SPLIT) vlo[dt] = vfrag(1, vr);
          }
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) mma3<SPLIT>(st.o[dt], vh[dt], vlo[dt], ph, pl);
        return;
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int vr = kb * HD + voff(dt);
        half8 v = vfrag(0, vr), vl = {};
        if constexpr (SPLIT) vl = vfrag(1, vr);
        mma3<SPLIT>(st.o[dt], v, vl, ph, pl);
      }
  };
  auto softmax_pv = [&](St& st, int k0, int kb, floatx4 (&sc)[2]) {
    softmax_pv_m(st, k0, kb, sc, std::integral_constant<int, 0>{});
  };
  // VAR bit 32: the K fragments of a block (read one block ahead) and their S^T MFMAs
  auto kread = [&](int kb, half8 (&kf)[2][KS][NP]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int krow = kb + 16 * j + ql;
        const int kr = krow * KROW + 8 * swz_chunk<KCPR>(krow, 4 * ks + g);
#pragma unroll
        for (int p = 0; p < NP; ++p) kf[j][ks][p] = *reinterpret_cast<const half8*>(kls[p] + kr);
      }
  };
  auto kmma = [&](const St& st, const half8 (&kf)[2][KS][NP], floatx4 (&sc)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      sc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {   // the term order of qk()
        sc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[j][ks][0], st.qf[ks][0], sc[j], 0, 0, 0);
        if constexpr (SPLIT) {
          sc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[j][ks][1], st.qf[ks][0], sc[j], 0, 0, 0);
          sc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[j][ks][0], st.qf[ks][1], sc[j], 0, 0, 0);
        }
      }
    }
  };
  // keys [k0, k0 + n) of the staged chunk (LDS positions 0 .. n-1)
  auto attend = [&](St& st, int k0, int n) {
    if constexpr ((VAR & 32) != 0) {
      // Peeled loop: the blocks wholly inside the sequence run without the key mask (no
      // per-block branch, and no register copies between a masked and an unmasked version of
      // the scores); the last, partial block (if any) after them. Block kb + 32's K fragments
      // are read while block kb's softmax runs. Same arithmetic, same order: bitwise the
      // outputs of the variant without bit 32.
      const int nf = min(n, len - k0) & ~31;
      half8 kf[2][KS][NP];
      if (n > 0) kread(0, kf);
      if constexpr ((VAR & 4) != 0) {
        // + bit 4: block kb + 32's S^T MFMAs issued before block kb's softmax (they run in
        // the matrix pipe under its vector work), block kb + 64's K read behind them
        floatx4 sn[2];
        if (n > 0) {
          kmma(st, kf, sn);
          if (32 < n) kread(32, kf);
        }
        int kb = 0;
        for (; kb < nf; kb += 32) {
          floatx4 sc[2] = {sn[0], sn[1]};
          if (kb + 32 < n) {
            kmma(st, kf, sn);
            if (kb + 64 < n) kread(kb + 64, kf);
          }
          softmax_pv_m(st, k0, kb, sc, std::integral_constant<int, 1>{});
        }
        if (kb < n) softmax_pv_m(st, k0, kb, sn, std::integral_constant<int, 2>{});
        return;
      }
      for (int kb = 0; kb < nf; kb += 32) {
        floatx4 sc[2];
        kmma(st, kf, sc);
        if (kb + 32 < n) kread(kb + 32, kf);
        softmax_pv_m(st, k0, kb, sc, std::integral_constant<int, 1>{});
      }
      if (nf < n) {
        floatx4 sc[2];
        kmma(st, kf, sc);
        softmax_pv_m(st, k0, nf, sc, std::integral_constant<int, 2>{});
      }
    } else if constexpr ((VAR & 4) != 0) {
      floatx4 sn[2];
      qk(st, 0, sn);
      for (int kb = 0; kb < n; kb += 32) {
        floatx4 sc[2] = {sn[0], sn[1]};
        if (kb + 32 < n) qk(st, kb + 32, sn);
        softmax_pv(st, k0, kb, sc);
      }
    } else {
      for (int kb = 0; kb < n; kb += 32) {
        floatx4 sc[2];
        qk(st, kb, sc);
        softmax_pv(st, k0, kb, sc);
      }
    }
  };
  auto finish = [&](St& st, int qb) {
    float l = st.l[0];
    if constexpr (!(SPLIT && (VAR & 2))) {
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
    }
    const int q = qb * 16 + ql;
    if (q < len) {
      // lane: O^T[d = 16dt + 4g + r][q]
      const float inv = 1.0f / l;
      const int64_t off = (int64_t)(base + q) * H + h * HD + 4 * g;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        half4 a, al;
        if constexpr (SPLIT && (VAR & 8) != 0) {
#pragma unroll
          for (int r = 0; r < 4; r += 2) {   // (not split_half4: scaled per pair, as compiled)
            half2 h2, l2;
            split16x2(st.o[dt][r] * inv, st.o[dt][r + 1] * inv, h2, l2);
            a[r] = h2[0]; a[r + 1] = h2[1]; al[r] = l2[0]; al[r + 1] = l2[1];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float x = st.o[dt][r] * inv;
            if constexpr (SPLIT) { const half2 s16_ = split16(x); a[r] = s16_[0]; al[r] = s16_[1]; }
            else a[r] = (_Float16)x;
          }
        }
        *reinterpret_cast<half4*>(ctx + off + 16 * dt) = a;
        if constexpr (SPLIT) *reinterpret_cast<half4*>(ctx_lo + off + 16 * dt) = al;
      }
    }
  };

  const int nqb = min((len + 15) >> 4, max_qb);     // max_qb = 1: the CLS query block only
  if ((VAR & 16) != 0 && nch == 1) {
    // paired query blocks: a wave carries blocks qb and qb + NW through the key blocks side
    // by side (two independent score -> softmax -> P.V chains for the scheduler to interleave;
    // a rerank sequence of 200-288 tokens has 13-18 blocks, i.e. about one pair per wave of
    // the 8). A wave left with one block runs it twice and stores it once. Per block the
    // arithmetic is the single-block path's, so the outputs are bitwise the same.
    for (int qb = wid; qb < nqb; qb += 2 * NW) {
      const bool two = qb + NW < nqb;
      const int qb2 = two ? qb + NW : qb;
      St s0, s1;
      init(s0, qb);
      init(s1, qb2);
      if (qb == wid) {                  // first round: the Q loads ride under the staging
        stage(0, sp);
        __syncthreads();
      }
      for (int kb = 0; kb < sp; kb += 32) {
        floatx4 sc0[2], sc1[2];
        qk(s0, kb, sc0);
        qk(s1, kb, sc1);
        softmax_pv(s0, 0, kb, sc0);
        softmax_pv(s1, 0, kb, sc1);
      }
      finish(s0, qb);
      if (two) finish(s1, qb2);
    }
    if (wid >= nqb) {                   // a wave without a block still joins the staging
      stage(0, sp);
      __syncthreads();
    }
  } else if (nch == 1) {
    // rolling Q prefetch: a wave's first QPF query blocks are loaded before the K/V staging
    // (their latency hides behind it), and each later one while the block QPF ahead computes
    // (fp16 at head_dim 32 runs 8 waves per SIMD in 64 VGPRs: one block ahead fits)
    // (VAR bit 1024, round 6, diagnostic build: one block ahead in fp16x3 too — 8 VGPRs instead
    // of bit 1's 24, still 112 in all; bitwise 42's outputs, timing neutral: 1066 0.2486-0.2519
    // vs 42 0.2485-0.2507 ms, profiles/r06_attn/r06n2_*: the Q loads' latency is not exposed)
    constexpr int QPF = (VAR & 1) == 0 ? ((VAR & 1024) != 0 ? 1 : 0) : SPLIT || HD > 32 ? 3 : 1;
    half8 qpre[QPF > 0 ? QPF : 1][KS][NP];
#pragma unroll
    for (int i = 0; i < QPF; ++i)
      if (wid + i * NW < nqb) load_q(qpre[i], wid + i * NW);
    stage(0, sp);
    __syncthreads();
    for (int qb = wid; qb < nqb; qb += NW) {
      St st;
      if constexpr (QPF > 0) {
        reset(st);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            st.qf[ks][p] = qpre[0][ks][p];
#pragma unroll
            for (int i = 0; i + 1 < QPF; ++i) qpre[i][ks][p] = qpre[i + 1][ks][p];
          }
        if (qb + QPF * NW < nqb) load_q(qpre[QPF - 1], qb + QPF * NW);
      } else {
        init(st, qb);
      }
      attend(st, 0, sp);
      finish(st, qb);
    }
  } else {
    // keys do not fit at once: for each round of query blocks, stream the key chunks
    // (every wave joins every barrier; waves without a block this round only stage)
    for (int q0 = 0; q0 < nqb; q0 += NW) {
      const int qb = q0 + wid;
      St st;
      if (qb < nqb) init(st, qb);
      for (int ch = 0; ch < nch; ++ch) {
        const int k0 = ch * cap, n = min(cap, sp - k0);
        __syncthreads();
        stage(k0, n);
        __syncthreads();
        if (qb < nqb) attend(st, k0, n);
      }
      if (qb < nqb) finish(st, qb);
    }
  }
}

// ----------------------------------------------------------------------------------------
// last layer, CLS rows only: both heads read only the CLS token's final hidden state
// (sentence-transformers Pooling(cls); BertPooler takes hidden_states[:, 0]), and a token's
// row after the last attention depends on the other tokens only through that attention. So
// the last layer computes Q|K|V for every token (K, V are needed), attention for the first
// query block of each sequence, and everything after it — O-proj, residual + LN, FFN,
// residual + LN — on the B gathered CLS rows instead of all T tokens.
// gather: x_cls[b] = x[cu[b]], ctx_cls[b] = ctx[cu[b]] (+ lo plane); one wave per sequence.
// Deferred LayerNorm (st non-null, H = kDlH): the token rows hold z = xh + xl and its block
// statistics, and x_cls = LN(z) with (gamma, beta) = (g, bt).
// ----------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(64) void gather_cls_kernel(
    const float* __restrict__ x, const _Float16* __restrict__ xh,
    const _Float16* __restrict__ xl, const _Float16* __restrict__ ctx,
    const _Float16* __restrict__ ctx_lo, const int* __restrict__ cu, float* __restrict__ x_cls,
    _Float16* __restrict__ ctx_cls, _Float16* __restrict__ ctx_cls_lo,
    const float* __restrict__ st = nullptr, const float* __restrict__ g = nullptr,
    const float* __restrict__ bt = nullptr, float eps = 0.f,
    _Float16* __restrict__ xh_cls = nullptr, _Float16* __restrict__ xl_cls = nullptr) {
  // (ctx null: the CLS rows only, before a CLS-only attention, attn_cls_kernel; xh_cls /
  // xl_cls: also their hi / lo fp16 planes, the Q projection's operands)
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t r = cu[b];
  float mu = 0.f, rs = 1.f;
  if (H == kDlH && st) {
    const floatx4* sr = reinterpret_cast<const floatx4*>(st + r * kDlParts * 2);
    dl_row_stats(sr[0], sr[1], sr[2], eps, mu, rs);
  }
#pragma unroll
  for (int j = 0; j < H / 64; ++j) {
    const int c = lane + 64 * j;
    // (x null: the residual stream is xh + xl, add_ln_kernel<XF> / deferred LayerNorm)
    float v = x ? x[r * H + c] : (float)xh[r * H + c] + (float)xl[r * H + c];
    if (st) v = (v - mu) * rs * g[c] + bt[c];
    x_cls[(int64_t)b * H + c] = v;
    if (xh_cls) {
      const _Float16 hv = (_Float16)v;
      xh_cls[(int64_t)b * H + c] = hv;
      if (xl_cls) xl_cls[(int64_t)b * H + c] = (_Float16)(v - (float)hv);
    }
    if (ctx) {
      ctx_cls[(int64_t)b * H + c] = ctx[r * H + c];
      if (ctx_lo) ctx_cls_lo[(int64_t)b * H + c] = ctx_lo[r * H + c];
    }
  }
}

// ----------------------------------------------------------------------------------------
// CLS-only attention of the last encoder layer (round 4): the cross-encoder / bge heads read
// only the [CLS] row, so the last layer needs the attention output of one query per
// (sequence, head). One wave per (sequence, head), 4 heads per workgroup: lane j takes keys
// j, j + 64, ... of the sequence; scores from the fp16x3 planes in fp32 (the MFMA path's
// three products: k_hi q_hi + k_lo q_hi + k_hi q_lo), softmax in base 2 with the 1/sqrt(d)
// scale folded in, P . V against v_hi + v_lo, then one cross-lane combine (max, rescale, sum).
// kv: [T][2H] planes (K | V of every token: the last layer's K|V-only projection); q: [B][H]
// planes of the CLS rows' Q; out: [B][H] planes of the CLS rows' context.
// ----------------------------------------------------------------------------------------
constexpr int kAttnClsHeads = 4;
constexpr int kAttnClsBlock = 64 * kAttnClsHeads;   // launch_fixed / __launch_bounds__
template <int H, int HD>
__global__ __launch_bounds__(kAttnClsBlock) void attn_cls_kernel(
    const _Float16* __restrict__ kv, const _Float16* __restrict__ kv_lo,
    const _Float16* __restrict__ q, const _Float16* __restrict__ q_lo,
    const int* __restrict__ cu, int B, int max_len, float scale, _Float16* __restrict__ out,
    _Float16* __restrict__ out_lo) {
  static_assert(HD % 8 == 0 && (H / HD) % kAttnClsHeads == 0, "head groups");
  constexpr int NH = H / HD;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.x / (NH / kAttnClsHeads);
  const int h = (blockIdx.x % (NH / kAttnClsHeads)) * kAttnClsHeads + wv;
  if (b >= B) return;
  const int base = cu[b], len = min(cu[b + 1] - cu[b], max_len);
  float qh[HD], ql[HD];
#pragma unroll
  for (int c = 0; c < HD / 8; ++c) {
    const half8 a = *reinterpret_cast<const half8*>(q + (int64_t)b * H + h * HD + 8 * c);
    const half8 l = *reinterpret_cast<const half8*>(q_lo + (int64_t)b * H + h * HD + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      qh[8 * c + e] = (float)a[e];
      ql[8 * c + e] = (float)l[e];
    }
  }
  const float c2 = scale * 1.44269504088896341f;
  float m = kNegInf, l = 0.f, o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) o[d] = 0.f;
  for (int j = lane; j < len; j += 64) {
    const _Float16* kr = kv + (int64_t)(base + j) * (2 * H) + h * HD;
    const _Float16* krl = kv_lo + (int64_t)(base + j) * (2 * H) + h * HD;
    half8 k8[HD / 8], kl8[HD / 8], v8[HD / 8], vl8[HD / 8];
#pragma unroll
    for (int c = 0; c < HD / 8; ++c) {
      k8[c] = *reinterpret_cast<const half8*>(kr + 8 * c);
      kl8[c] = *reinterpret_cast<const half8*>(krl + 8 * c);
      v8[c] = *reinterpret_cast<const half8*>(kr + H + 8 * c);
      vl8[c] = *reinterpret_cast<const half8*>(krl + H + 8 * c);
    }
    float s0 = 0.f, s1 = 0.f;   // k_hi q_hi and the two correction products
#pragma unroll
    for (int c = 0; c < HD / 8; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float kh = (float)k8[c][e], klo = (float)kl8[c][e];
        s0 = fmaf(kh, qh[8 * c + e], s0);
        s1 = fmaf(klo, qh[8 * c + e], fmaf(kh, ql[8 * c + e], s1));
      }
    const float sc = (s0 + s1) * c2;
    const float mn = fmaxf(m, sc);
    const float corr = __builtin_amdgcn_exp2f(m - mn);   // m = -inf: 0
    const float p = __builtin_amdgcn_exp2f(sc - mn);
    l = l * corr + p;
#pragma unroll
    for (int c = 0; c < HD / 8; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        o[8 * c + e] = fmaf(p, (float)v8[c][e] + (float)vl8[c][e], o[8 * c + e] * corr);
    m = mn;
  }
  // combine the 64 lanes: common max, rescale, sums
  float mw = m;
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) mw = fmaxf(mw, __shfl_xor(mw, sh, 64));
  const float f = m == kNegInf ? 0.f : __builtin_amdgcn_exp2f(m - mw);
  l *= f;
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) l += __shfl_xor(l, sh, 64);
#pragma unroll
  for (int d = 0; d < HD; ++d) {
    float x = o[d] * f;
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) x += __shfl_xor(x, sh, 64);
    o[d] = x;
  }
  if (lane < HD) {
    float v = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) v = lane == d ? o[d] : v;
    v = v / l;
    const _Float16 hv = (_Float16)v;
    out[(int64_t)b * H + h * HD + lane] = hv;
    out_lo[(int64_t)b * H + h * HD + lane] = (_Float16)(v - (float)hv);
  }
}

}  // namespace ragmi::bert
