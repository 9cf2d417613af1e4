// prep_kernels.hip — the storage layout of the in-HBM flat cosine index for gfx950 (MI355X)
// and the two kernels that write into it: ingest (upsert_kernel) and query prep (qprep_*).
// First of the device headers index_capi.hip includes; the scan, seed, certify, merge, large-k,
// re-select and row headers after it all read this layout.
//
// Replaces the Qdrant server's COSINE collection behind QdrantClient.query_points / upsert
// (reference main.py:215-239, ingest.py:148-175).
//
// Storage layout in HBM ("tile16"): rows are grouped in tiles of 16; a tile is stored in the
// exact order the v_mfma_f32_16x16x32_f16 A-operand wants it, so every wave-wide load of the
// scan is one perfectly coalesced 1 KiB dwordx4 (16 B/lane x 64 lanes):
//     tile t, k-step s (32 dims), lane l = h*16 + r  ->  8 halves  row 16t+r, dims 32s+8h..+7
//     half8 index = t*(D/32)*64 + s*64 + l
// The query batch (32 queries = two 16-wide MFMA column tiles) is prepared into the matching
// B-operand order and kept in VGPRs for the whole scan.
#include "device_common.hpp"

namespace ragmi {

constexpr int kTileRows = 16;
constexpr int kQ = 32;            // queries per pass

template <int D>
__host__ __device__ constexpr int steps() { return D / 32; }

// half8 slot of piece c (halves 8c .. 8c+7) of row `row` in the tile16 layout
template <int D>
__device__ __forceinline__ int64_t tile_slot(int64_t row, int c) {
  return (row >> 4) * (steps<D>() * 64) + (c >> 2) * 64 + (c & 3) * 16 + (row & 15);
}

// ----------------------------------------------------------------------------------------
// upsert: one wave per vector. Canonical normalisation -> fp16 (RNE) -> tile16 slot.
// ----------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(64) void upsert_kernel(const float* __restrict__ vecs,
                                                    const int64_t* __restrict__ rows,
                                                    const uint32_t* __restrict__ tags_in,
                                                    half8* __restrict__ corpus,
                                                    uint32_t* __restrict__ tags, int64_t n,
                                                    int64_t cap_rows,
                                                    float* __restrict__ rows32 = nullptr) {
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int lane = threadIdx.x;
  const int64_t row = rows[i];
  if (row < 0 || row >= cap_rows) return;  // host validates; never write out of bounds
  const float* x = vecs + i * D;
  const double norm = sqrt(canon_sumsq<D>(x, lane));
  for (int c = lane; c < D / 8; c += 64) {
    half8 h;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      y[j] = canon_scale(x[8 * c + j], norm);
      h[j] = f32_to_f16(y[j]);
    }
    corpus[tile_slot<D>(row, c)] = h;
    if (rows32) {   // fp32 storage: the normalised fp32 row itself (exact rescoring operand)
      float4* o = reinterpret_cast<float4*>(rows32 + row * D + 8 * c);
      o[0] = float4{y[0], y[1], y[2], y[3]};
      o[1] = float4{y[4], y[5], y[6], y[7]};
    }
  }
  if (lane == 0) tags[row] = tags_in ? tags_in[i] : 0u;
}

// ----------------------------------------------------------------------------------------
// query prep: one wave per query slot (32 slots; slots >= B are zero).
//   qn    [32][D] fp32 canonical-normalised queries (exact rescoring operand)
//   qfrag [2][D/32][64] half8: B-operand fragments, lane l -> query 16*qt + (l&15),
//         dims 32s + 8(l>>4) .. +7
//   filt  [32][2] (tag mask, tag value) per query slot
//   eps   [32] bound on |MFMA score - exact score| over every stored row (see below)
//
// Error bound. Stored rows c are fp16 roundings of unit vectors (||c||_2 <= kRowNorm); the
// scan scores a = MFMA(c, h) with h = fp16(qn) and fp32 accumulation over D products (each
// product exact in fp32), the exact score is e = fp32(sum c_k qn_k). Then
//   |a - e| <= ||c|| ||h - qn||            (query rounding, Cauchy-Schwarz)
//            + D 2^-23 ||c|| ||h||          (<= D roundings of the fp32 accumulator, each
//                                            <= 1 ulp: holds for any internal MFMA order)
//            + 2^-23                        (e's own fp32 rounding)
//            [+ store_eps]                  (fp32 storage: the exact score reads the fp32 row
//                                            c32 while the scan reads c = fp16(c32):
//                                            |sum (c - c32) qn| <= ||c - c32|| ||qn|| <=
//                                            2^-11 ||c32|| + 2^-25 sqrt(D), times ||qn||)
// inflated by 2^-10 relative + 2^-22 absolute so the fp32 comparisons that use it in select
// stay conservative.
// ----------------------------------------------------------------------------------------
constexpr double kRowNorm = 1.001;   // fp16(unit vector): ||c|| <= 1 + 2^-11 + sqrt(D) 2^-25

// one query slot b by one wave. The B-fragment goes to qf (global or an LDS image of the same
// layout); qn / filt / eps are written only when `publish` (the fused qprep_sample_kernel:
// every workgroup builds the fragments it samples with, workgroup 0 publishes)
template <int D>
__device__ __forceinline__ void qprep_slot(const float* __restrict__ q, int B, int b, int lane,
                                           const uint32_t* __restrict__ filt_in,
                                           float* __restrict__ qn, half8* __restrict__ qf,
                                           uint32_t* __restrict__ filt, float* __restrict__ eps,
                                           double store_eps, bool publish,
                                           uint32_t* __restrict__ filt_copy = nullptr,
                                           half8* __restrict__ qf_glob = nullptr) {
  const bool live = b < B;
  if (lane == 0) {
    // per-query payload filter (mask, value); padding / unfiltered queries match every row
    const uint32_t fm = (live && filt_in) ? filt_in[2 * b] : 0u;
    const uint32_t fv = (live && filt_in) ? filt_in[2 * b + 1] : 0u;
    if (publish) {
      filt[2 * b] = fm;
      filt[2 * b + 1] = fv;
    }
    if (filt_copy) {
      filt_copy[2 * b] = fm;
      filt_copy[2 * b + 1] = fv;
    }
  }
  double norm = 0.0;
  if (live) norm = sqrt(canon_sumsq<D>(q + (int64_t)b * D, lane));
  const int qt = b >> 4, c16 = b & 15;
  double dq2 = 0.0, hh2 = 0.0;   // ||h - qn||^2, ||h||^2 (lane partials)
  for (int c = lane; c < D / 8; c += 64) {
    half8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float y = live ? canon_scale(q[(int64_t)b * D + 8 * c + j], norm) : 0.0f;
      if (publish) qn[b * D + 8 * c + j] = y;
      h[j] = f32_to_f16(y);
      const double hd = (double)h[j], dd = hd - (double)y;
      dq2 = fma(dd, dd, dq2);
      hh2 = fma(hd, hd, hh2);
    }
    const int s = c >> 2, hh = c & 3;
    qf[(qt * steps<D>() + s) * 64 + hh * 16 + c16] = h;
    if (qf_glob) qf_glob[(qt * steps<D>() + s) * 64 + hh * 16 + c16] = h;
  }
  if (!publish) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    dq2 += __shfl_xor(dq2, d, 64);
    hh2 += __shfl_xor(hh2, d, 64);
  }
  if (lane == 0) {
    double e = kRowNorm * sqrt(dq2) + (double)D * 0x1p-23 * kRowNorm * sqrt(hh2) + 0x1p-23 +
               store_eps;
    e = e * (1.0 + 0x1p-10) + 0x1p-22;
    eps[b] = live ? (float)(e * (1.0 + 0x1p-20)) : 0.0f;   // rounded up past fp32's RNE
  }
}

template <int D>
__global__ __launch_bounds__(64) void qprep_kernel(const float* __restrict__ q, int B,
                                                   const uint32_t* __restrict__ filt_in,
                                                   float* __restrict__ qn,
                                                   half8* __restrict__ qfrag,
                                                   uint32_t* __restrict__ filt,
                                                   float* __restrict__ eps,
                                                   double store_eps = 0.0) {
  qprep_slot<D>(q, B, blockIdx.x, threadIdx.x, filt_in, qn, qfrag, filt, eps, store_eps, true);
}

}  // namespace ragmi
