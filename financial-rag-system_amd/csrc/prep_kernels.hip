// prep_kernels.hip — the storage layout of the in-HBM flat cosine index for gfx950 (MI355X)
// and the kernels that write into it: ingest (upsert_kernel) and query prep (qprep_*); then
// the scan copies of the rows (dim 384, fp16 storage): the int8 and the 6-bit layout, the int8
// query prep (qprep8_*) and the upper bound u_bound, the two copy formats (Copy8, Copy6) and the
// one quantiser over them (quantise_row / requant_kernel).
// First of the device headers index_search.hip includes; the scan, seed, certify, merge, large-k,
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
  const double norm = canon_norm(canon_sumsq<D>(x, lane));
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
// kRowNorm: device_common.hpp (the imports check it on the host)

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
  if (live) norm = canon_norm(canon_sumsq<D>(q + (int64_t)b * D, lane));
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

// ----------------------------------------------------------------------------------------
// int8 scan copy (D = 384, fp16 storage; DESIGN.md "int8 prescan"). A second image of the
// corpus for v_mfma_i32_16x16x64_i8, layout "tile16x64":
//     tile t, k-step s (64 dims), lane l = h*16 + r  ->  16 bytes  row 16t+r, dims 64s+16h..+15
//     byte offset = ((t*(D/64) + s)*64 + l)*16
// and per row its scale s_r and its measured error E_r = ||c16 - s_r c8||_2 (rounded up), in
// `meta` as [tile][32] floats: the tile's 16 scales, then its 16 errors. Both are pure
// functions of the stored fp16 row (quantise_row), rebuilt by requant_kernel after every write
// of `corpus`.
// ----------------------------------------------------------------------------------------
typedef int intx4 __attribute__((ext_vector_type(4)));

template <int D>
__host__ __device__ constexpr int steps8() { return D / 64; }

// byte offset of piece c (dims 8c .. 8c+7, 8 bytes) of row `row` in the tile16x64 layout
template <int D>
__device__ __forceinline__ int64_t tile8_byte(int64_t row, int c) {
  return (((row >> 4) * steps8<D>() + (c >> 3)) * 64 + ((c >> 1) & 3) * 16 + (row & 15)) * 16 +
         (c & 1) * 8;
}

// first float of row `row`'s scale in meta (its error: + 16)
__device__ __forceinline__ int64_t meta_slot(int64_t row) { return (row >> 4) * 32 + (row & 15); }

// ----------------------------------------------------------------------------------------
// 6-bit scan copy (D = 384, fp16 storage, the largest shards). A third image of
// the corpus: per row and dimension one integer v in [-31, 31] (six bits, two's complement),
// with the row's own scale s_r = max|c| / 31 and measured error E_r = ||c - s_r v||_2. The scan
// reads each value as the int8 4 v (its six bits are the byte's top six: no sign extension, no
// bias), so its meta (meta_slot, as the int8 copy's) holds s_r / 4, exact, and E_r.
// Layout "pair6": the unit is a PAIR of tiles (32 rows, 9216 B, nine 1-KiB wave loads). Lane
// l = h*16 + r of the wave owns row r and k-group h of both tiles: 36 dwords, dword g of lane l
// at byte
//     pair * 9216 + (g / 4) * 1024 + l * 16 + (g % 4) * 4,
// g = 18 u + 3 s + c for tile u of the pair, k-step s and part c < 3. The three dwords of
// (u, s) hold the lane's sixteen values of dims 64 s + 16 h .. + 15 — the k-map of the int8
// copy, so the int8 query fragments serve unchanged —: byte b of part c carries in its top six
// bits v of dim 4 c + b, and in its low two bits the bits 2c, 2c + 1 of v of dim 12 + b.
// unpack6 rebuilds the four A-fragment dwords (bytes 4 v) in nine bitwise ops.
// ----------------------------------------------------------------------------------------
constexpr int kPair6Bytes = 9216;

// dword index, within the lane's 36, of part c of k-step s of tile u of a pair
__host__ __device__ constexpr int pair6_dword(int u, int s, int c) { return 18 * u + 3 * s + c; }

// byte offset of dword g of fragment lane l of pair `pair`
__device__ __forceinline__ int64_t pair6_byte(int64_t pair, int g, int l) {
  return pair * kPair6Bytes + (g >> 2) * 1024 + l * 16 + (g & 3) * 4;
}

// the int8 A-fragment (sixteen values 4 v, one per byte) of three packed dwords
__device__ __forceinline__ intx4 unpack6(uint32_t p0, uint32_t p1, uint32_t p2) {
  const uint32_t x = ((p0 << 2) & 0x0c0c0c0cu) | ((p1 << 4) & 0x30303030u) |
                     ((p2 << 6) & 0xc0c0c0c0u);
  return intx4{(int)(p0 & 0xfcfcfcfcu), (int)(p1 & 0xfcfcfcfcu), (int)(p2 & 0xfcfcfcfcu), (int)x};
}

// ----------------------------------------------------------------------------------------
// int8 query prep, one wave per query slot, after qprep_slot: the normalised query y as two
// int8 planes, y ~ qh = sq * (254 hi + lo) with s1 = max|y| / 127, hi = rint(y / s1),
// sq = s1 / 254 and lo = rint((y - s1 hi) / sq) (|y - s1 hi| <= s1 / 2, so |lo| <= 127).
//   qfrag8 [2 query tiles][2 planes: hi, lo][D/64][64] x 16 bytes: B-operand fragments of
//          v_mfma_i32_16x16x64_i8, lane l -> query 16 qt + (l & 15), dims 64s + 16(l>>4) .. +15
//          (the corpus copy's k-map; integer accumulation is exact and order-free)
//   qp8    [32][4] floats: sq, A = ||y|| + F, C = kRowNorm F + slack, 0
//   eps8   [32] the certificate's eps for a pass that ranks by u (u_bound): u >= e already
//          holds, so eps only keeps select's fp32 comparisons conservative
// F = ||y - qh||_2 is measured in fp64 against the fp32 value of sq actually used, so it is
// the error of the represented query whatever the quantisation's own roundings were.
//
// Upper bound. With c the stored fp16 row, c8 / s_r / E_r its int8 copy, I = sum c8 (254 hi +
// lo) (exact in int32: |I| <= D 127 (254 127 + 127) < 2^31) and e = fp32(sum c y):
//   sum c y = sum (s_r c8 + (c - s_r c8)) (qh + (y - qh))
//           = s_r sq I + sum (c - s_r c8) qh + sum c (y - qh)
//          <= s_r sq I + E_r (||y|| + F) + ||c|| F                 (Cauchy-Schwarz, ||c|| <= kRowNorm)
// u_bound evaluates the right side in fp32 as fma(If, s_r sq, fma(E_r, A, C)) with If =
// fma(float(hi dot), 254, float(lo dot)): both dots are < 2^24 in magnitude (D 127^2 =
// 6.2e6), so their conversions are exact and If, which can exceed 2^24, carries one rounding
// (2^-24 relative). The product s_r sq and the two fmas add one each; every term is at most
// (||c|| + E_r)(||y|| + F) < 1.1 in magnitude, so the four roundings stay below 4 * 1.1 * 2^-24
// < 2^-21.7, and e's own fp32 rounding below 2^-24 * 1.01. The slack 2^-20 in C covers both
// (A and C themselves are rounded up from fp64).
//
// The 6-bit copy (c8 := v in [-31, 31], s_r = max|c| / 31, its own measured E_r) goes through
// the same inequality. Its scan multiplies the bytes 4 v and reads the scale s_r / 4: both
// factors of 4 are exact, so u is the u of (v, s_r) bit for bit. I6 = sum 4 v (254 hi + lo) is
// exact in int32 (|I6| <= 4 D 31 (254 127 + 127) = 1.55e9 < 2^31); both plane dots are at most
// 4 D 31 127 = 6.05e6 < 2^23, so u_bound6 forms 254 hi + lo with one 24-bit integer
// multiply-add and converts once: the same single rounding of the same exact integer as
// u_bound's fma of two exact conversions. E_r <= (s_r / 2) sqrt(D) = 0.317 max|c| <= 0.317
// ||c||, so every term is at most (||c|| + E_r)(||y|| + F) < 1.33 * 1.01 in magnitude: four
// roundings stay below 4 * 1.35 * 2^-24 < 2^-21.5, and with e's own 2^-24 * 1.01 below
// 2^-21.2. The slack 2^-20 covers it unchanged.
// ----------------------------------------------------------------------------------------
constexpr float kU8Slack = 0x1p-20f;

__device__ __forceinline__ float u_bound(int hi, int lo, float s_r, float e_r, float sq, float A,
                                         float C) {
  // fma_scalar: same values as fmaf, never paired into packed fp32 ops beside the MFMAs
  const float If = fma_scalar((float)hi, 254.0f, (float)lo);
  return fma_scalar(If, s_r * sq, fma_scalar(e_r, A, C));
}

// the 6-bit scan's form (hi, lo: the plane dots of the bytes 4 v; s_r: the stored s_r / 4)
__device__ __forceinline__ float u_bound6(int hi, int lo, float s_r, float e_r, float sq, float A,
                                          float C) {
  const float If = (float)(__mul24(hi, 254) + lo);
  return fma_scalar(If, s_r * sq, fma_scalar(e_r, A, C));
}

template <int D>
__device__ __forceinline__ void qprep8_slot(const float* __restrict__ q, int B, int b, int lane,
                                            char* __restrict__ qfrag8, float* __restrict__ qp8,
                                            float* __restrict__ eps8) {
  static_assert(D / 8 <= 64, "one piece per lane");
  const bool live = b < B;
  double norm = 0.0;
  if (live) norm = canon_norm(canon_sumsq<D>(q + (int64_t)b * D, lane));
  const bool has = lane < D / 8;
  float y[8];
  float m = 0.f;
  double y2 = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    y[j] = (live && has) ? canon_scale(q[(int64_t)b * D + 8 * lane + j], norm) : 0.0f;
    m = fmaxf(m, fabsf(y[j]));
    y2 = fma((double)y[j], (double)y[j], y2);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  const float s1 = m / 127.0f, sq = s1 / 254.0f;
  uint32_t wh[2] = {0u, 0u}, wl[2] = {0u, 0u};
  double f2 = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float hi = s1 > 0.f ? rintf(y[j] / s1) : 0.f;
    hi = fminf(fmaxf(hi, -127.f), 127.f);
    const double rho = (double)y[j] - (double)s1 * (double)hi;
    float lo = sq > 0.f ? rintf((float)(rho / (double)sq)) : 0.f;
    lo = fminf(fmaxf(lo, -127.f), 127.f);
    const double dd = (double)y[j] - (double)sq * (254.0 * (double)hi + (double)lo);
    f2 = fma(dd, dd, f2);
    wh[j >> 2] |= ((uint32_t)(int)hi & 0xffu) << (8 * (j & 3));
    wl[j >> 2] |= ((uint32_t)(int)lo & 0xffu) << (8 * (j & 3));
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    f2 += __shfl_xor(f2, d, 64);
    y2 += __shfl_xor(y2, d, 64);
  }
  if (has) {
    const int qt = b >> 4, c16 = b & 15, c = lane;
    const int lane_l = ((c >> 1) & 3) * 16 + c16;
    const int64_t o_hi = ((int64_t)((qt * 2 + 0) * steps8<D>() + (c >> 3)) * 64 + lane_l) * 16 +
                         (c & 1) * 8;
    const int64_t o_lo = ((int64_t)((qt * 2 + 1) * steps8<D>() + (c >> 3)) * 64 + lane_l) * 16 +
                         (c & 1) * 8;
    *reinterpret_cast<uint2*>(qfrag8 + o_hi) = uint2{wh[0], wh[1]};
    *reinterpret_cast<uint2*>(qfrag8 + o_lo) = uint2{wl[0], wl[1]};
  }
  if (lane == 0) {
    const double F = sqrt(f2) * (1.0 + 0x1p-20), Y = sqrt(y2) * (1.0 + 0x1p-20);
    qp8[4 * b + 0] = sq;
    qp8[4 * b + 1] = (float)((Y + F) * (1.0 + 0x1p-20));
    qp8[4 * b + 2] = (float)((kRowNorm * F + (double)kU8Slack) * (1.0 + 0x1p-20));
    qp8[4 * b + 3] = 0.f;
    eps8[b] = live ? kU8Slack : 0.0f;
  }
}

// qprep for a pass that scans the int8 copy: everything qprep_kernel writes (select rescoring,
// the tier-2 rescan and its fp16 bound `eps` read it), then the int8 planes
template <int D>
__global__ __launch_bounds__(64) void qprep8_kernel(const float* __restrict__ q, int B,
                                                    const uint32_t* __restrict__ filt_in,
                                                    float* __restrict__ qn,
                                                    half8* __restrict__ qfrag,
                                                    uint32_t* __restrict__ filt,
                                                    float* __restrict__ eps,
                                                    char* __restrict__ qfrag8,
                                                    float* __restrict__ qp8,
                                                    float* __restrict__ eps8) {
  qprep_slot<D>(q, B, blockIdx.x, threadIdx.x, filt_in, qn, qfrag, filt, eps, 0.0, true);
  qprep8_slot<D>(q, B, blockIdx.x, threadIdx.x, qfrag8, qp8, eps8);
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

// ----------------------------------------------------------------------------------------
// The two scan copy formats. A format states what differs between the copies and nothing else:
// the quantiser's range, the scale its scan reads, how a quantised row is stored, how a tile's
// upper bounds u are produced from memory (tile_u_at, defined in scan_kernels.hip beside the
// tile arithmetic it uses) and the form of the bound. Everything else — the quantiser, the
// rebuild, the seed sample, the diagnostic bounds — is written once over a format.
// ----------------------------------------------------------------------------------------
template <int D>
struct Query8;   // scan_kernels.hip: the int8 query batch of a wave

struct Copy8 {
  static constexpr int kQMax = 127;   // |byte| <= 127
  static __device__ __forceinline__ float stored_scale(float s) { return s; }
  // lane c < D/8 (`has`) holds the eight bytes of piece c of `row`
  template <int D>
  static __device__ __forceinline__ void store_row(char* __restrict__ data, int64_t row, int lane,
                                                   bool has, uint2 b) {
    if (has) *reinterpret_cast<uint2*>(data + tile8_byte<D>(row, lane)) = b;
  }
  static __device__ __forceinline__ float bound(int hi, int lo, float s_r, float e_r, float sq,
                                                float A, float C) {
    return u_bound(hi, lo, s_r, e_r, sq, A, C);
  }
  // u of tile t of the copy against the 32 queries, by one wave
  template <int D>
  static __device__ __forceinline__ void tile_u_at(const char* __restrict__ data,
                                                   const float* __restrict__ meta, int64_t t,
                                                   const Query8<D>& q, int lane, floatx4& u0,
                                                   floatx4& u1);
};

struct Copy6 {
  static constexpr int kQMax = 31;    // |v| <= 31
  // the scale of the bytes 4 v the scan multiplies (exact)
  static __device__ __forceinline__ float stored_scale(float s) { return 0.25f * s; }
  // b: the eight values as six-bit fields, one per byte. Pieces 2m, 2m + 1 are the sixteen dims
  // of one (k-step, k-group): the even lane packs both (every lane of the wave calls)
  template <int D>
  static __device__ __forceinline__ void store_row(char* __restrict__ data, int64_t row, int lane,
                                                   bool has, uint2 b) {
    static_assert(D == 384, "pair6 layout");
    const uint32_t o0 = __shfl_xor(b.x, 1, 64), o1 = __shfl_xor(b.y, 1, 64);
    if (has && (lane & 1) == 0) {
      const int ks = lane >> 3, kg = (lane >> 1) & 3;
      const int l = kg * 16 + (int)(row & 15), u = (int)(row >> 4) & 1;
      const uint32_t p[3] = {(b.x << 2) | (o1 & 0x03030303u), (b.y << 2) | ((o1 >> 2) & 0x03030303u),
                             (o0 << 2) | ((o1 >> 4) & 0x03030303u)};
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<uint32_t*>(data + pair6_byte(row >> 5, pair6_dword(u, ks, c), l)) = p[c];
    }
  }
  static __device__ __forceinline__ float bound(int hi, int lo, float s_r, float e_r, float sq,
                                                float A, float C) {
    return u_bound6(hi, lo, s_r, e_r, sq, A, C);
  }
  template <int D>
  static __device__ __forceinline__ void tile_u_at(const char* __restrict__ data,
                                                   const float* __restrict__ meta, int64_t t,
                                                   const Query8<D>& q, int lane, floatx4& u0,
                                                   floatx4& u1);
};

// The one quantiser of a stored row, by one wave: lane c < D/8 passes piece c (x: the fp16
// values widened, dims 8c .. 8c+7), other lanes zeros. Max-abs scale s = max|x| / kQMax, values
// v = rint(x / s) in [-kQMax, kQMax], returned as two's complement fields of the format's width,
// one per byte; err = ||x - s v||_2 measured in fp64 and rounded up to fp32. The zero row gives
// scale 0, v = 0, error 0. Every lane returns the same s and err.
template <typename Copy>
__device__ __forceinline__ uint2 quantise_row(const float (&x)[8], float& s, float& err) {
  constexpr float kMax = (float)Copy::kQMax;
  constexpr uint32_t kField = 2u * Copy::kQMax + 1u;   // 0xff, 0x3f
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(x[j]));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  s = m / kMax;
  uint32_t w[2] = {0u, 0u};
  double e2 = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = s > 0.f ? rintf(x[j] / s) : 0.f;
    v = fminf(fmaxf(v, -kMax), kMax);
    const double dd = (double)x[j] - (double)s * (double)v;
    e2 = fma(dd, dd, e2);
    w[j >> 2] |= ((uint32_t)(int)v & kField) << (8 * (j & 3));
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) e2 += __shfl_xor(e2, d, 64);
  // fp64 sum of <= D squares: relative error << 2^-40; 2^-20 covers it and the fp32 RNE
  err = e2 > 0.0 ? (float)(sqrt(e2) * (1.0 + 0x1p-20)) : 0.f;
  return uint2{w[0], w[1]};
}

// rows[i] (rows != nullptr) or row0 + i, i < n: the copy (`data`, `meta`) of the stored fp16 row
// in format Copy. One wave per row; launched after every kernel that writes `corpus`, on the
// same stream.
template <int D, typename Copy>
__global__ __launch_bounds__(64) void requant_kernel(const half8* __restrict__ corpus,
                                                     const int64_t* __restrict__ rows,
                                                     int64_t row0, int64_t n, int64_t cap_rows,
                                                     char* __restrict__ data,
                                                     float* __restrict__ meta) {
  static_assert(D / 8 <= 64, "one piece per lane");
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int lane = threadIdx.x;
  const int64_t row = rows ? rows[i] : row0 + i;
  if (row < 0 || row >= cap_rows) return;   // never read or write out of bounds
  float x[8];
  const bool has = lane < D / 8;
  half8 h = {};
  if (has) h = corpus[tile_slot<D>(row, lane)];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = has ? (float)h[j] : 0.f;
  float s, err;
  const uint2 b = quantise_row<Copy>(x, s, err);
  Copy::template store_row<D>(data, row, lane, has, b);
  if (lane == 0) {
    meta[meta_slot(row)] = Copy::stored_scale(s);
    meta[meta_slot(row) + 16] = err;
  }
}

}  // namespace ragmi
