// bert_device.hpp — device helpers that more than one stage of the encoder forward uses (first
// of the encoder headers included by bert_capi.hip): the fp16x3 split and MFMA term, erf-GELU,
// the wave sum, the LDS image swizzle and fragment read, buffer panels, LDS-DMA, ring waits.
//
// BERT-small encoder forward for gfx950 (bge-small-en-v1.5 and
// ms-marco-MiniLM-L-6-v2 cross-encoder).
//
// Replaces the torch CPU forward behind sentence-transformers' SentenceTransformer.encode
// (reference main.py:80-84, 144-149, 211-213; main2.py:170-171) and CrossEncoder.predict
// (main.py:86-90, 241-247). Arithmetic follows transformers modeling_bert.py (post-LN,
// erf-GELU, softmax(QK^T/sqrt(d) + mask)V); see oracle/bert_ref.py.
//
// Numerics: GEMM operands fp16 (weights and activations), fp32 MFMA accumulation, fp32
// residual stream, fp32 LayerNorm/softmax statistics.
// Layout: sequences are PACKED (no padding): token t of sequence b sits at row cu[b] + pos.
// Right padding never changes a valid token's output (masked keys contribute exp(-inf) = 0),
// so packing is exact w.r.t. the padded reference.
#pragma once

#include "device_common.hpp"

namespace ragmi::bert {

// Built shapes (template parameters below): hidden H in {384, 768, 1024} with head_dim HD in
// {32, 64} (bge-small / MiniLM: 384/32; bge-base: 768/64; bge-large: 1024/64); intermediate
// size is a runtime GEMM dimension.

typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2 __attribute__((ext_vector_type(2)));

// fp16x3 split: v = hi + lo with hi = fp16(v), lo = fp16(v - hi); a*b ~ ah*bh + ah*bl + al*bh
// (relative error ~2^-22) on the fp16 MFMA pipe.
// v is pinned as an fp32 register value before either conversion: under -ffp-contract=fast
// the compiler may fuse the operation that produced v into the hi conversion (one rounding of
// the unrounded product / sum straight to fp16, v_fma_mix*_f16) while lo subtracts hi from
// the fp32-rounded v — where an fp16 rounding midpoint falls between the two, hi and lo
// disagree and hi + lo is off by one fp16 ulp (measured: 1-4 of ~1e5 attention outputs, every
// error exactly one ulp; tests/test_attention_gpu.py).
__device__ __forceinline__ half2 split16(float v) {   // {hi, lo}
  asm("" : "+v"(v));
  const _Float16 hi = (_Float16)v;
  return half2{hi, (_Float16)(v - (float)hi)};
}

// The same split of two values in 3 instructions instead of 8 (round 2): the hi pair by one
// v_cvt_pk_f16_f32, each lo by v_fma_mix{lo,hi}_f16 computing -hi * 1 + v exactly and rounding
// once to fp16. v - hi is exact in fp32 (Sterbenz: hi is within a factor 2 of v, or 0), so
// this is fp16(v - hi) bit for bit, as split16 computes it (which converts hi back to fp32,
// subtracts and converts again, and converts hi twice). Inputs pinned as above.
__device__ __forceinline__ void split16x2(float v0, float v1, half2& h, half2& l) {
  asm("" : "+v"(v0), "+v"(v1));
  h = half2{(_Float16)v0, (_Float16)v1};
  const uint32_t hu = __builtin_bit_cast(uint32_t, h);
  uint32_t lu;
  asm("v_fma_mixlo_f16 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, -%1, 1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(lu)
      : "v"(hu), "v"(v0), "v"(v1));
  l = __builtin_bit_cast(half2, lu);
}
// four fp32 values -> fp16 hi [and lo: SPLIT, by split16x2; else l is left alone]
template <bool SPLIT>
__device__ __forceinline__ void split_half4(const floatx4& v, half4& h, half4& l) {
#pragma unroll
  for (int r = 0; r < 4; r += 2) {
    if constexpr (SPLIT) {
      half2 h2, l2;
      split16x2(v[r], v[r + 1], h2, l2);
      h[r] = h2[0]; h[r + 1] = h2[1]; l[r] = l2[0]; l[r + 1] = l2[1];
    } else {
      h[r] = (_Float16)v[r];
      h[r + 1] = (_Float16)v[r + 1];
    }
  }
}

// erf-GELU, 0.5 x (1 + erf(x / sqrt 2)), with erfc(|z|) from Abramowitz & Stegun 7.1.26
// (|error of erf| <= 1.5e-7 absolute, i.e. at fp32 rounding level for the GELU output):
// 1 + erf(z) = 2 - erfc(z) for z >= 0 and erfc(-z) for z < 0 (no cancellation for z << 0).
// Two transcendentals (rcp, exp2) and 7 FMAs instead of the libm erff's branchy polynomial.
__device__ __forceinline__ float gelu_erf(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float q = fmaf(1.061405429f, t, -1.453152027f);
  q = fmaf(q, t, 1.421413741f);
  q = fmaf(q, t, -0.284496736f);
  q = fmaf(q, t, 0.254829592f);
  q *= t * __builtin_amdgcn_exp2f(-z * z * 1.44269504088896341f);   // erfc(z)
  return 0.5f * x * (x >= 0.f ? 2.0f - q : q);
}

// the same on 4 values at once: every non-transcendental step as 4-wide vector arithmetic
// (gfx950 packed fp32: v_pk_fma_f32 / v_pk_mul_f32 take 2 lanes' worth per instruction), the
// rcp / exp2 per value. Per value the same operations in the same order as gelu_erf.
__device__ __forceinline__ floatx4 gelu_erf4(floatx4 x) {
  const floatx4 z = __builtin_elementwise_abs(x) * 0.70710678118654752440f;
  const floatx4 d = __builtin_elementwise_fma((floatx4)(0.3275911f), z, (floatx4)(1.0f));
  floatx4 t, e;
  const floatx4 zz = -z * z * 1.44269504088896341f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    t[r] = __builtin_amdgcn_rcpf(d[r]);
    e[r] = __builtin_amdgcn_exp2f(zz[r]);
  }
  floatx4 q = __builtin_elementwise_fma((floatx4)(1.061405429f), t, (floatx4)(-1.453152027f));
  q = __builtin_elementwise_fma(q, t, (floatx4)(1.421413741f));
  q = __builtin_elementwise_fma(q, t, (floatx4)(-0.284496736f));
  q = __builtin_elementwise_fma(q, t, (floatx4)(0.254829592f));
  q *= t * e;
  floatx4 w;
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r] = x[r] >= 0.f ? 2.0f - q[r] : q[r];
  return 0.5f * x * w;
}

// Sum over the 64 lanes, the same bits in every lane: DPP within each 16-lane row (xor 1,
// xor 2, half-row mirror, row mirror — each step adds a lane's value to its partner's, and
// fp32 addition commutes, so partners agree), then the row pairs and halves by
// v_permlane16_swap / v_permlane32_swap. No LDS round trips (ds_bpermute: ~12 dependent ones
// for two butterfly reductions in add_ln_kernel).
__device__ __forceinline__ float dpp_add(float v, int ctrl_sel) {
  int d;
  switch (ctrl_sel) {   // dpp_ctrl must be an immediate
    case 0: d = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false); break;
    case 1: d = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false); break;
    case 2: d = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false); break;
    default: d = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false); break;
  }
  return v + __builtin_bit_cast(float, d);
}
__device__ __forceinline__ float wave_sum64(float v) {
  v = dpp_add(v, 0);   // quad_perm [1,0,3,2]
  v = dpp_add(v, 1);   // quad_perm [2,3,0,1]: every lane holds its quad's sum
  v = dpp_add(v, 2);   // row_half_mirror: + the other quad of the 8
  v = dpp_add(v, 3);   // row_mirror: + the other 8 of the row
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = __builtin_bit_cast(float, (uint32_t)r16[0]) + __builtin_bit_cast(float, (uint32_t)r16[1]);
  const uint32_t u2 = __builtin_bit_cast(uint32_t, v);
  const auto r32 = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
  return __builtin_bit_cast(float, (uint32_t)r32[0]) + __builtin_bit_cast(float, (uint32_t)r32[1]);
}

// 16-B chunk swizzle of a row-major [rows][CPR chunks] LDS image for the MFMA fragment read
// (lane l: row l & 15 of a 16-row block, chunk c0 + (l >> 4)), conflict-free under the
// ds_read_b128 lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59},
// {36-43,48-51,60-63} (MI355X_MICROARCH.md §LDS): each group's 16 lanes must cover all 64
// banks. CPR 8 (128-B rows, bank = 32 (r % 2) + 4 c'): c' = c ^ (r & 7). CPR 4 (64-B rows,
// bank = 16 (r % 4) + 4 c'): c' = c ^ 3 [r & 8] — a group pairs rows {0-3, 12-15} at chunk c
// with rows {4-11} at chunk c + 1, so the flip has to separate rows 0-7 from 8-15 (the
// round-1 flip by row quad, c ^ (r / 4 % 4), left rows 0-3 and 4-7 on the same banks:
// 2-way conflicts in every fp16x3 fragment read).
template <int CPR>
__device__ __forceinline__ int swz_chunk(int row, int chunk) {
  if constexpr (CPR == 8) return chunk ^ (row & 7);
  else return chunk ^ (((row >> 3) & 1) * 3);
}
template <int CPR>
__device__ __forceinline__ int swz(int row, int chunk) {
  return row * CPR + swz_chunk<CPR>(row, chunk);
}
// the lane's MFMA operand fragment of the 16 rows from row0 of such an image, 32-deep K
// sub-step ks
template <int CPR>
__device__ __forceinline__ half8 frag(const half8* plane, int row0, int ks, int lane) {
  return plane[swz<CPR>(row0 + (lane & 15), ks * 4 + (lane >> 4))];
}

// The lane's byte offset inside a row-major panel (rows of row_elems fp16) for 1-KB DMA piece
// `piece` of the lane-linear LDS image: LDS position q = 64 piece + lane holds row q / CPR,
// 16-B chunk (q % CPR) ^ swizzle(row). A launch constant.
template <int CPR>
__device__ __forceinline__ uint32_t dma_lane_offset(int piece, int lane, int row_elems) {
  const int q = piece * 64 + lane, r = q / CPR, cs = q % CPR;
  return (uint32_t)(r * row_elems + swz_chunk<CPR>(r, cs) * 8) * 2u;
}
// One product term of a GEMM step: acc += W . A on v_mfma_f32_16x16x32_f16; fp16x3 (SPLIT) the
// small terms first, W_lo A_hi + W_hi A_lo + W_hi A_hi — the tests pin this order bitwise.
// (!SPLIT: the lo fragments are not read.)
template <bool SPLIT>
__device__ __forceinline__ void mma3(floatx4& acc, const half8& w_hi, const half8& w_lo,
                                     const half8& a_hi, const half8& a_lo) {
  if constexpr (SPLIT) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w_lo, a_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w_hi, a_lo, acc, 0, 0, 0);
  }
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w_hi, a_hi, acc, 0, 0, 0);
}

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 16 B per lane buffer -> LDS DMA: lane l's bytes at panel + soff + voff land at LDS byte
// address lds_addr + 16 l. Inline asm for the same reason as glds16 (device_common.hpp).
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t rs, uint32_t voff, uint32_t soff,
                                       uint32_t lds_addr) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(rs), "s"(lds_addr), "s"(soff)
      : "memory");
}

// raw buffer resource over [base, base + bytes) from wave-uniform inputs (reads past the
// end return zeros, stores past it are dropped); bytes < 2^31 (checked by the launcher)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t panel(const void* base, int64_t bytes) {
  // every input made provably wave-uniform (T20): a descriptor the compiler cannot prove
  // uniform lands in VGPRs (asm "s" operand error / waterfall loops around buffer ops)
  const uint64_t a = (uint64_t)(uintptr_t)base;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  const int nb = bytes > 0 ? (int)bytes : 0;
  void* p = reinterpret_cast<void*>((uintptr_t)(((uint64_t)hi << 32) | lo));
  return __builtin_amdgcn_make_buffer_rsrc(p, 0, __builtin_amdgcn_readfirstlane(nb),
                                           0x00020000);
}

// s_waitcnt vmcnt(Y*L + (stored ? S : 0)) for a runtime Y in [0, Y_MAX] (vmcnt takes an
// immediate): Y = ring stages issued after the one being waited for
template <int L, int S, int Y>
__device__ __forceinline__ void wait_ring(int y, bool stored) {
  if (y == Y) {
    if (stored)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Y * L + S) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Y * L) : "memory");
    return;
  }
  if constexpr (Y > 0) wait_ring<L, S, Y - 1>(y, stored);
}

// s_waitcnt vmcnt(n) for a runtime n in [0, N] (the immediate is compile-time)
template <int N>
__device__ __forceinline__ void wait_vm(int n) {
  if (n >= N) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
    return;
  }
  if constexpr (N > 0) wait_vm<N - 1>(n);
}

typedef short short4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ half4 lds_read_tr16(const _Float16* p) {
  return __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) short4v*)(p)));
}

}  // namespace ragmi::bert
