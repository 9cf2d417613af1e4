// ln_kernels.hip — the LayerNorm stages of the encoder forward (included by bert_capi.hip after
// bert_device.hpp): embeddings + LN (embed_ln_kernel) and residual + LN (add_ln_kernel,
// add_ln384_kernel), all launched by forward_t.
namespace ragmi::bert {

// ----------------------------------------------------------------------------------------
// embeddings: x = LN(word[id] + type[tt] + pos[p]); one wave per token, grid (ceil(L/4), B)
// ----------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(256) void embed_ln_kernel(
    const int* __restrict__ ids, const int* __restrict__ types, const int* __restrict__ cu,
    const float* __restrict__ wemb, const float* __restrict__ pemb, const float* __restrict__ temb,
    const float* __restrict__ g, const float* __restrict__ bt, float eps, int vocab,
    int type_vocab, int max_pos, float* __restrict__ x, _Float16* __restrict__ xh,
    _Float16* __restrict__ xl) {
  const int b = blockIdx.y;
  const int pos = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int len = cu[b + 1] - cu[b];
  if (pos >= len) return;
  const int64_t t = cu[b] + pos;
  // clamp: a bad id must never become an out-of-bounds gather
  const int id = min(max(ids[t], 0), vocab - 1);
  const int ty = min(max(types[t], 0), type_vocab - 1);
  const int pp = min(pos, max_pos - 1);
  float v[H / 64];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < H / 64; ++j) {
    const int c = lane + 64 * j;
    v[j] = wemb[(int64_t)id * H + c] + temb[ty * H + c] + pemb[pp * H + c];
    s += v[j];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  const float mu = s * (1.0f / H);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < H / 64; ++j) q += (v[j] - mu) * (v[j] - mu);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) q += __shfl_xor(q, d, 64);
  const float rs = rsqrtf(q * (1.0f / H) + eps);
#pragma unroll
  for (int j = 0; j < H / 64; ++j) {
    const int c = lane + 64 * j;
    const float y = (v[j] - mu) * rs * g[c] + bt[c];
    if (x) x[t * H + c] = y;                 // (null: fp16x3 residual kept as xh + xl only)
    _Float16 yh, yl;
    { const half2 s16_ = split16(y); yh = s16_[0]; yl = s16_[1]; }
    xh[t * H + c] = yh;
    if (xl) xl[t * H + c] = yl;
  }
}

// ----------------------------------------------------------------------------------------
// residual + LayerNorm: x = LN(x + y) (fp32, in place), xh = fp16(x); one wave per row.
// XF (fp16x3 only): the residual stream lives in the operand planes alone, x = xh + xl
// (fp16(x - xh) keeps x to 2^-22 relative), so the fp32 copy is neither read nor written:
// 12 instead of 20 bytes per element.
// ----------------------------------------------------------------------------------------
// y may hold `parts` split-K partial products (gemm_pipe_kernel ksplit > 1), part p at
// y + p * pstride: they are summed in part order (deterministic) before the residual add.
template <int H, bool XF = false>
__global__ __launch_bounds__(256) void add_ln_kernel(float* __restrict__ x,
                                                     const float* __restrict__ y,
                                                     const float* __restrict__ g,
                                                     const float* __restrict__ bt, float eps,
                                                     _Float16* __restrict__ xh,
                                                     _Float16* __restrict__ xl, int T,
                                                     int parts = 1, int64_t pstride = 0) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= T) return;
  float v[H / 64];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < H / 64; ++j) {
    const int c = lane + 64 * j;
    const float r = XF ? (float)xh[t * H + c] + (float)xl[t * H + c] : x[t * H + c];
    float yy = y[t * H + c];
    for (int p = 1; p < parts; ++p) yy += y[p * pstride + t * H + c];
    v[j] = r + yy;
    s += v[j];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  const float mu = s * (1.0f / H);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < H / 64; ++j) q += (v[j] - mu) * (v[j] - mu);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) q += __shfl_xor(q, d, 64);
  const float rs = rsqrtf(q * (1.0f / H) + eps);
#pragma unroll
  for (int j = 0; j < H / 64; ++j) {
    const int c = lane + 64 * j;
    const float o = (v[j] - mu) * rs * g[c] + bt[c];
    if constexpr (!XF) x[t * H + c] = o;
    _Float16 oh, ol;
    { const half2 s16_ = split16(o); oh = s16_[0]; ol = s16_[1]; }
    xh[t * H + c] = oh;
    if (xl) xl[t * H + c] = ol;
  }
}

// add_ln_kernel for hidden 384 (bge-small / MiniLM; round 3): lane l < 48 owns columns
// 8l .. 8l+7 — 16-B loads of the residual planes (or 2 x 16 B of the fp32 rows) and of each
// split-K part, 16-B plane stores — and both reductions run on wave_sum64. The small-batch
// forward's residual passes (2 per layer, ~87 launches per 32-query encode) were
// latency-bound on 2-byte accesses and 12 dependent ds_bpermute round trips.
// Same formula, parts summed in part order; the reduction order differs from add_ln_kernel's.
// ln384_rows: R rows t[0..R) of one wave (t < 0: none), every row's loads issued before any
// row's reductions (add_ln384_kernel: R = 1). Round 5 also ran it with R = 4 inside the SMALL
// split-K GEMM, the last arriving workgroup of each 64-row block finishing the block behind an
// agent-scope release / acquire ticket: bit-identical forward, but the per-unit L2 write-back
// of the release made the 32-query forward 0.71 -> 1.17 ms (profiles/r05r_split_ln_ab.jsonl).
template <bool XF, int R>
__device__ __forceinline__ void ln384_rows(float* __restrict__ x, const float* __restrict__ y,
                                           const float* __restrict__ g,
                                           const float* __restrict__ bt, float eps,
                                           _Float16* __restrict__ xh, _Float16* __restrict__ xl,
                                           const int64_t (&t)[R], int lane, int parts,
                                           int64_t pstride) {
  constexpr int H = 384;
  const bool on = lane < H / 8;
  float v[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t o = (t[r] < 0 ? 0 : t[r]) * H + 8 * (on ? lane : 0);
    if (on && t[r] >= 0) {
      floatx4 y0 = *reinterpret_cast<const floatx4*>(y + o);
      floatx4 y1 = *reinterpret_cast<const floatx4*>(y + o + 4);
#pragma unroll
      for (int p = 1; p < 4; ++p)
        if (p < parts) {
          y0 += *reinterpret_cast<const floatx4*>(y + p * pstride + o);
          y1 += *reinterpret_cast<const floatx4*>(y + p * pstride + o + 4);
        }
      if constexpr (XF) {
        const half8 h = *reinterpret_cast<const half8*>(xh + o);
        const half8 l = xl ? *reinterpret_cast<const half8*>(xl + o) : half8{};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[r][e] = ((float)h[e] + (float)l[e]) + (e < 4 ? y0[e] : y1[e - 4]);
      } else {
        const floatx4 r0 = *reinterpret_cast<const floatx4*>(x + o);
        const floatx4 r1 = *reinterpret_cast<const floatx4*>(x + o + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[r][e] = (e < 4 ? r0[e] : r1[e - 4]) + (e < 4 ? y0[e] : y1[e - 4]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[r][e] = 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (t[r] < 0) continue;                     // (wave-uniform)
    const int64_t o = t[r] * H + 8 * (on ? lane : 0);
    const float s = ((v[r][0] + v[r][1]) + (v[r][2] + v[r][3])) +
                    ((v[r][4] + v[r][5]) + (v[r][6] + v[r][7]));
    const float mu = wave_sum64(s) * (1.0f / H);
    float q = 0.f;
    if (on)
#pragma unroll
      for (int e = 0; e < 8; ++e) q = fmaf(v[r][e] - mu, v[r][e] - mu, q);
    const float rs = rsqrtf(wave_sum64(q) * (1.0f / H) + eps);
    if (!on) continue;
    const floatx4 g0 = *reinterpret_cast<const floatx4*>(g + 8 * lane);
    const floatx4 g1 = *reinterpret_cast<const floatx4*>(g + 8 * lane + 4);
    const floatx4 b0 = *reinterpret_cast<const floatx4*>(bt + 8 * lane);
    const floatx4 b1 = *reinterpret_cast<const floatx4*>(bt + 8 * lane + 4);
    float out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      out[e] = (v[r][e] - mu) * rs * (e < 4 ? g0[e] : g1[e - 4]) + (e < 4 ? b0[e] : b1[e - 4]);
    if constexpr (!XF) {
      *reinterpret_cast<floatx4*>(x + o) = floatx4{out[0], out[1], out[2], out[3]};
      *reinterpret_cast<floatx4*>(x + o + 4) = floatx4{out[4], out[5], out[6], out[7]};
    }
    half4 h0, l0, h1, l1;
    split_half4<true>(floatx4{out[0], out[1], out[2], out[3]}, h0, l0);
    split_half4<true>(floatx4{out[4], out[5], out[6], out[7]}, h1, l1);
    *reinterpret_cast<half8*>(xh + o) = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    if (xl)
      *reinterpret_cast<half8*>(xl + o) = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
  }
}

template <bool XF, bool L2 = false>
__global__ __launch_bounds__(256) void add_ln384_kernel(float* __restrict__ x,
                                                        const float* __restrict__ y,
                                                        const float* __restrict__ g,
                                                        const float* __restrict__ bt, float eps,
                                                        _Float16* __restrict__ xh,
                                                        _Float16* __restrict__ xl, int T,
                                                        int parts = 1, int64_t pstride = 0,
                                                        float* __restrict__ l2out = nullptr) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int64_t tr[1] = {t};
  const int lane = threadIdx.x & 63;
  ln384_rows<XF, 1>(x, y, g, bt, eps, xh, xl, tr, lane, parts, pstride);
  if constexpr (L2 && !XF) {
  // (round 6) the bge head fused into the last layer's residual + LayerNorm of the CLS rows:
  // out[t] = x[t] / max(||x[t]||, 1e-12) with cls_normalize_kernel's exact arithmetic — its
  // lane m holds columns m + 64 j, so the row just written goes through this wave's LDS
  // slice into that layout (one dispatch fewer per query-batch forward)
  __shared__ float rowbuf[4][384];
  float* rb = rowbuf[threadIdx.x >> 6];
  if (lane < 48) {
    const floatx4 a = *reinterpret_cast<const floatx4*>(x + t * 384 + 8 * lane);
    const floatx4 b = *reinterpret_cast<const floatx4*>(x + t * 384 + 8 * lane + 4);
    *reinterpret_cast<floatx4*>(rb + 8 * lane) = a;
    *reinterpret_cast<floatx4*>(rb + 8 * lane + 4) = b;
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float v[6];
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    v[j] = rb[lane + 64 * j];
    sq += v[j] * v[j];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) sq += __shfl_xor(sq, d, 64);
  const float inv = 1.0f / fmaxf(sqrtf(sq), 1e-12f);
#pragma unroll
  for (int j = 0; j < 6; ++j) l2out[t * 384 + lane + 64 * j] = v[j] * inv;
  }
}

}  // namespace ragmi::bert
