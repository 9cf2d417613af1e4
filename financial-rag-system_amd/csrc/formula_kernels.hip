// formula_kernels.hip — formula queries (included by index_search.hip after reselect_kernels.hip,
// whose sort it shares): formula_rescore_kernel re-scores the distinct rows of a request's L exact
// candidate lists by a postfix program over their scores, payload keys and filter conditions
// (rag_formula_rescore). The blob's layout, the ops and E, the decay exponential,
// are the ones of include/ragmi.h ("Formula queries"), restated by ragmi.formula.pack_formula and
// tests/_formula_ref.py. One workgroup per request; it reads only its input arrays (no index).
//
// No reference counterpart: the reference sorts by similarity alone (main.py:232-237).
namespace ragmi {

constexpr int kFmlBlock = kRrfBlock;              // rrf_bitonic's block
constexpr int kFmlPer = kRrfMaxE / kFmlBlock;     // slots per thread at the limit
constexpr int kFmlMaxOps = RAG_FORMULA_MAX_OPS;
constexpr int kFmlMaxConds = RAG_FORMULA_MAX_CONDS;
constexpr int kFmlHdr = RAG_FORMULA_HDR_WORDS;
constexpr int kFmlOp = RAG_FORMULA_OP_WORDS;

// the candidates' key columns, [B][L][C] each; nullptr = not supplied
struct FormulaKeys {
  const int64_t* col[RAG_KEYS_MAX_COLS];
};

__device__ __forceinline__ const int64_t* formula_col(const FormulaKeys& keys, uint32_t c) {
  return c == 0 ? keys.col[0] : c == 1 ? keys.col[1] : c == 2 ? keys.col[2] : keys.col[3];
}

// E(a), the decay exponential of include/ragmi.h: multiplies and adds only, never contracted,
// so that a numpy restatement gives the same bits.
__device__ __forceinline__ double formula_exp(double a) {
#pragma clang fp contract(off)
  if (!(a <= 0.0)) return __builtin_nan("");
  if (a < -700.0) return 0.0;
  const double n = __builtin_rint(a * 1.4426950408889634);
  const double r = (a - n * 6.93147180369123816490e-01) - n * 1.90821492927058770002e-10;
  // 1 / i!, i = 13 .. 0: i! is exact in fp64, so each quotient is the correctly rounded one
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  // n lies in [-1010, 0]: 2^n is a normal double, the product exact
  return p * __longlong_as_double((long long)(1023 + (int)n) << 52);
}

// One condition program (a "Filter programs" record, staged in LDS) against a candidate's tag
// and keys. pool / pool_words: the condition blob in global memory, offsets from its first word;
// a word is read only when its index is < pool_words. A RANGE atom reads its column at `slot`
// only when the column was supplied.
__device__ __forceinline__ bool formula_cond(const uint32_t* rec, const uint32_t* __restrict__ pool,
                                             uint32_t pool_words, uint32_t tag,
                                             const FormulaKeys& keys, int64_t slot) {
  const int na = (int)min(rec[0], (uint32_t)RAG_FILTER_MAX_ATOMS);
  uint32_t idx = 0u;
  for (int a = 0; a < na; ++a) {                      // wave-uniform
    const uint32_t* d = rec + 9 + 4 * a;
    const uint32_t kind = d[0], p0 = d[1], p1 = d[2], p2 = d[3];
    uint32_t bit = 0u;
    if (kind == RAG_FILTER_ATOM_RANGE) {
      if (p0 < (uint32_t)RAG_KEYS_MAX_COLS && (uint64_t)p1 + 3 < pool_words) {
        const int64_t* kp = formula_col(keys, p0);
        if (kp) {
          const int64_t lo = (int64_t)(((uint64_t)pool[p1 + 1] << 32) | pool[p1]);
          const int64_t hi = (int64_t)(((uint64_t)pool[p1 + 3] << 32) | pool[p1 + 2]);
          const int64_t k = kp[slot];
          bit = (uint32_t)(k != RAG_KEY_ABSENT && lo <= k && k <= hi);
        }
      }
    } else if (kind == RAG_FILTER_ATOM_INSET) {
      const uint32_t code = (tag >> ((p0 & 1u) * 16u)) & 0xFFFFu;
      const uint64_t w = (uint64_t)p1 + (code >> 5);
      uint32_t bits = 0u;
      if (code < p2 && w < pool_words) bits = pool[w];
      bit = (bits >> (code & 31u)) & 1u;
    } else {                                          // MASKEQ (and any unknown kind)
      bit = (uint32_t)((tag & p0) == p1);
    }
    idx |= bit << a;
  }
  return ((rec[1 + (idx >> 5)] >> (idx & 31u)) & 1u) != 0u;
}

// ----------------------------------------------------------------------------------------
// formula_rescore_kernel: rrf_fuse_kernel's structure with a program in place of the sum.
//   1. the blob is checked and staged: the op records and the condition records in LDS (the
//      pool of the condition blob stays in global memory, L2-resident). Every thread walks the
//      staged ops once for the stack discipline and the indices (uniform, 64 LDS broadcasts at
//      most); a bad program evaluates nothing and sets RAG_FORMULA_BAD.
//   2. list ends, then the live entries as (row as uint64, e) in LDS, dead ones ~0; bitonic sort
//      by (row, e): the entries of a row are one run, its head the row's first entry in (list,
//      position) order.
//   3. the lane at a run's head evaluates the program. The op loop is the same for every lane
//      (wave-uniform; lanes that hold no head run it predicated off). The evaluation stack is
//      eight registers with the top at s0: a push shifts them down, a binary op shifts them up,
//      so every index is a compile-time one and nothing lives in scratch. SCORE walks the run
//      for the first entry of its list (the run is sorted by e = l * C + p); KEY and COND read
//      the tag and keys at the head's own entry. A head reads only its own run, so it may write
//      its result over its own s_aux slot at once; the other slots wait for the barrier.
//   4. the head's slot becomes (row, ~key) with key the order-preserving uint32 of the fp32 value
//      (sign bit flipped for positives, all bits for negatives), every other slot dead.
//   5. second bitonic sort by (~key, row) = (value descending, row ascending), then emit.
// Integer LDS atomics only (min for the list ends, add for the count of heads, or for the
// status), whose results do not depend on their order: the output is a pure function of the
// inputs. Every output element is written exactly once.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFmlBlock) void formula_rescore_kernel(
    const float* __restrict__ cand_s, const int64_t* __restrict__ cand_r,
    const uint32_t* __restrict__ cand_t, FormulaKeys keys, const int32_t* __restrict__ ncand,
    const uint32_t* __restrict__ prog, uint32_t words, int L, int C, int k,
    float* __restrict__ out_s, int64_t* __restrict__ out_r, int32_t* __restrict__ out_count,
    uint32_t* __restrict__ out_status) {
#pragma clang fp contract(off)
  __shared__ uint64_t s_row[kRrfMaxE];
  __shared__ uint32_t s_aux[kRrfMaxE];   // e, then ~key of the value
  __shared__ uint32_t s_ops[kFmlMaxOps * kFmlOp];
  __shared__ uint32_t s_cond[kFmlMaxConds * RAG_FILTER_REC_WORDS];
  __shared__ int s_n[kRrfMaxL];
  __shared__ int s_m;
  __shared__ uint32_t s_status;
  constexpr uint64_t kDead = ~0ull;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int E = L * C;               // <= kRrfMaxE
  int N = 2;
  while (N < E) N <<= 1;             // <= kRrfMaxE
  cand_s += b * E;
  cand_r += b * E;
  if (cand_t) cand_t += b * E;
#pragma unroll
  for (int c = 0; c < RAG_KEYS_MAX_COLS; ++c)
    if (keys.col[c]) keys.col[c] += b * E;

  // 1. the blob
  uint32_t n_ops = 0u, n_cond = 0u;
  bool bad = words < (uint32_t)kFmlHdr;
  if (!bad) {
    n_ops = prog[0];
    n_cond = prog[1];
    bad = n_ops > (uint32_t)kFmlMaxOps || n_cond > (uint32_t)kFmlMaxConds ||
          (uint64_t)kFmlHdr + (uint64_t)kFmlOp * n_ops +
                  (uint64_t)RAG_FILTER_REC_WORDS * n_cond > words;
  }
  if (bad) n_ops = n_cond = 0u;
  const uint32_t pool_at = (uint32_t)kFmlHdr + (uint32_t)kFmlOp * n_ops;   // <= words
  for (uint32_t i = tid; i < n_ops * kFmlOp; i += kFmlBlock) s_ops[i] = prog[kFmlHdr + i];
  for (uint32_t i = tid; i < n_cond * RAG_FILTER_REC_WORDS; i += kFmlBlock)
    s_cond[i] = prog[pool_at + i];
  if (tid < L) s_n[tid] = ncand ? min(C, max(0, ncand[b * L + tid])) : C;
  if (tid == 0) {
    s_m = 0;
    s_status = 0u;
  }
  __syncthreads();
  {
    int depth = 0;
    for (uint32_t o = 0; o < n_ops; ++o) {
      const uint32_t kind = s_ops[o * kFmlOp], arg = s_ops[o * kFmlOp + 1];
      int pops, pushes = 1;
      switch (kind) {
        case RAG_FORMULA_CONST: pops = 0; break;
        case RAG_FORMULA_SCORE: pops = 0; bad |= arg >= (uint32_t)L; break;
        case RAG_FORMULA_KEY:
          pops = 0;
          bad |= arg >= (uint32_t)RAG_KEYS_MAX_COLS || formula_col(keys, arg) == nullptr;
          break;
        case RAG_FORMULA_COND: pops = 0; bad |= arg >= n_cond || cand_t == nullptr; break;
        case RAG_FORMULA_NEG:
        case RAG_FORMULA_ABS: pops = 1; break;
        case RAG_FORMULA_ADD:
        case RAG_FORMULA_MUL:
        case RAG_FORMULA_DIV:
        case RAG_FORMULA_LIN:
        case RAG_FORMULA_EXP:
        case RAG_FORMULA_GAUSS: pops = 2; break;
        default: pops = 0; bad = true; break;
      }
      bad |= depth < pops;
      depth += pushes - pops;
      bad |= depth > RAG_FORMULA_MAX_STACK;
    }
    bad |= depth != 1;
  }
  if (bad) n_ops = 0u;               // nothing is evaluated: every value is 0.0
  n_ops = __builtin_amdgcn_readfirstlane(n_ops);
  const uint32_t* pool = prog + pool_at;
  const uint32_t pool_words = words - pool_at;

  // 2. the entries, sorted by (row, e)
  for (int e = tid; e < E; e += kFmlBlock) {
    const int l = e / C, p = e - l * C;
    if (cand_r[e] < 0) atomicMin(&s_n[l], p);   // a list ends at its first negative row
  }
  __syncthreads();
  for (int e = tid; e < N; e += kFmlBlock) {
    uint64_t r = kDead;
    if (e < E) {
      const int l = e / C, p = e - l * C;
      if (p < s_n[l]) r = (uint64_t)cand_r[e];
    }
    s_row[e] = r;
    s_aux[e] = (uint32_t)e;
  }
  __syncthreads();
  rrf_bitonic<true>(s_row, s_aux, N, tid);

  // 3. the heads evaluate
  uint32_t heads = 0u, status = bad ? RAG_FORMULA_BAD : 0u;
  for (int u = 0; u < kFmlPer; ++u) {
    const int i = tid + u * kFmlBlock;
    if (u * kFmlBlock >= N) break;               // uniform
    const uint64_t r = i < N ? s_row[i] : kDead;
    const bool head = i < N && r != kDead && (i == 0 || s_row[i - 1] != r);
    const int e0 = head ? (int)s_aux[i] : 0;     // the row's first entry
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
    uint32_t st = 0u;
    for (uint32_t o = 0; o < n_ops; ++o) {       // uniform
      const uint32_t* op = s_ops + o * kFmlOp;
      // the program is the same for every lane: scalar branches
      const uint32_t kind = __builtin_amdgcn_readfirstlane(op[0]);
      const uint32_t arg = __builtin_amdgcn_readfirstlane(op[1]);
      const uint32_t fl = __builtin_amdgcn_readfirstlane(op[2]);
      const double imm = __longlong_as_double((long long)(((uint64_t)op[5] << 32) | op[4]));
      double v = imm;
      int pops = 0;
      switch (kind) {                            // uniform
        case RAG_FORMULA_CONST: break;
        case RAG_FORMULA_SCORE: {
          bool found = false;
          if (head) {
            for (int j = i; j < N && s_row[j] == r; ++j) {
              const int e = (int)s_aux[j];
              const int l = e / C;
              if (l >= (int)arg) {               // ascending e: the first entry of list arg
                if (l == (int)arg) {
                  v = (double)cand_s[e];
                  found = true;
                }
                break;
              }
            }
            if (!found && !(fl & 1u)) {
              st |= RAG_FORMULA_MISSING;
              v = 0.0;
            }
          }
          break;
        }
        case RAG_FORMULA_KEY: {
          if (head) {
            const int64_t key = formula_col(keys, arg)[e0];
            if (key == RAG_KEY_ABSENT) {
              if (!(fl & 1u)) {
                st |= RAG_FORMULA_MISSING;
                v = 0.0;
              }
            } else {
              v = __longlong_as_double(key >= 0 ? key : key ^ 0x7FFFFFFFFFFFFFFFll);
              if (fl & 2u) v = v / 1e6;
            }
          }
          break;
        }
        case RAG_FORMULA_COND:
          v = head && formula_cond(s_cond + arg * RAG_FILTER_REC_WORDS, pool, pool_words,
                                   cand_t[e0], keys, e0)
                  ? 1.0
                  : 0.0;
          break;
        case RAG_FORMULA_NEG: pops = 1; v = -s0; break;
        case RAG_FORMULA_ABS: pops = 1; v = __builtin_fabs(s0); break;
        case RAG_FORMULA_ADD: pops = 2; v = s1 + s0; break;
        case RAG_FORMULA_MUL: pops = 2; v = s1 * s0; break;
        case RAG_FORMULA_DIV:
          pops = 2;
          if (s0 == 0.0) {
            if (!(fl & 1u)) {
              v = s1 / s0;
              if (head) st |= RAG_FORMULA_NONFINITE;
            }
          } else {
            v = s1 / s0;
          }
          break;
        case RAG_FORMULA_LIN: {
          pops = 2;
          const double t = 1.0 - imm * __builtin_fabs(s1 - s0);
          v = t > 0.0 ? t : 0.0;
          break;
        }
        case RAG_FORMULA_EXP: pops = 2; v = formula_exp(imm * __builtin_fabs(s1 - s0)); break;
        default: {                               // RAG_FORMULA_GAUSS: the walk above knows no other
          pops = 2;
          const double d = __builtin_fabs(s1 - s0);
          v = formula_exp(imm * (d * d));
          break;
        }
      }
      if (pops == 0) {                           // push
        s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0;
      } else if (pops == 2) {                    // two operands make one value
        s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
      }
      s0 = v;
    }
    if (head) {
      float f = (float)s0;                       // one rounding
      if (f == 0.0f) f = 0.0f;                   // -0.0 is +0.0
      if (!(__builtin_fabsf(f) < __builtin_inff())) st |= RAG_FORMULA_NONFINITE;
      const uint32_t fb = __float_as_uint(f);
      const uint32_t key = fb ^ ((fb >> 31) ? 0xFFFFFFFFu : 0x80000000u);   // ascending in f
      s_aux[i] = ~key;                           // its own run's first slot: no one else reads it
      heads |= 1u << u;
      status |= st;
    }
  }
  if (heads) atomicAdd(&s_m, __popc(heads));
  if (status) atomicOr(&s_status, status);
  __syncthreads();                   // every walk has read its run
  // 4. every other slot dies
#pragma unroll
  for (int u = 0; u < kFmlPer; ++u) {
    const int i = tid + u * kFmlBlock;
    if (i >= N || ((heads >> u) & 1u)) continue;
    s_row[i] = kDead;
    s_aux[i] = ~0u;
  }
  __syncthreads();
  // 5. by (value descending, row ascending)
  rrf_bitonic<false>(s_row, s_aux, N, tid);

  const int m = s_m;                 // distinct rows, <= E <= N
  for (int t = tid; t < k; t += kFmlBlock) {
    const bool live = t < m;
    float f = kNegInf;
    if (live) {
      const uint32_t key = ~s_aux[t];
      f = __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu));
    }
    out_s[b * k + t] = f;
    out_r[b * k + t] = live ? (int64_t)s_row[t] : -1;
  }
  if (tid == 0) {
    if (out_count) out_count[b] = m;
    out_status[b] = s_status;
  }
}

}  // namespace ragmi
