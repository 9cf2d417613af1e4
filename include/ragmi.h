/*
 * ragmi.h — C ABI of libragmi.so, the MI355X-native (gfx950) two-stage retrieval hot path.
 *
 * This is the drop-in boundary that replaces, for the reference
 * (pythonmailer/financial-rag-system, read-only at /root/reference):
 *   - the Qdrant server behind `QdrantClient.query_points` / `upsert` / `create_collection`
 *       main.py:92-95    get_qdrant()            -> rag_index_create
 *       main.py:215-239  retrieve_from_qdrant()  -> rag_index_search (one query per call, B=1)
 *       main2.py:160-163 retrieve_from_qdrant()  -> rag_index_search
 *       main2.py:281-295 batch_processor()       -> rag_index_search (B=32 in one call)
 *       ingest.py:86-96  ensure_collection()     -> rag_index_create (dim=384, COSINE)
 *       ingest.py:148-175 PointStruct + upsert   -> rag_index_upsert (row slots assigned by host)
 *       database.py:111-143 init_qdrant()        -> rag_index_create
 *   - the sentence-transformers encoders (see ragmi_bert.h).
 *
 * Conventions
 *   - All functions return 0 on success and a negative RAG_E* code on failure;
 *     rag_last_error() returns a thread-local message for the last failure on this thread.
 *   - "_dev" pointers are HIP device pointers (e.g. torch.Tensor.data_ptr() of a cuda tensor);
 *     "_host" pointers are host memory. Host buffers are caller-owned; device storage made by
 *     rag_index_create is handle-owned.
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); NULL = default stream.
 *     Device-pointer calls are asynchronous on `stream`; *_host calls are synchronous.
 *   - Handles are re-entrant: calls on one handle from several threads are serialised
 *     internally and each search uses its own workspace slot guarded by a HIP event, so
 *     concurrent searches on different streams are safe (main2.py runs up to 25 requests
 *     in flight through asyncio.to_thread, main2.py:52-53,218,228).
 *
 * Semantics (Qdrant COSINE collection, restated; see DESIGN.md §2 and oracle/scan_ref.c)
 *   - upsert: every vector is L2-normalised (canonical fp64 norm) to fp32,
 *     rounded to fp16 (RNE) and stored at its row slot; an existing slot is overwritten
 *     (md5 point ids make re-ingest idempotent, ingest.py:151-154).
 *   - search: the query is normalised the same way; score(row) = fp32(sum_k fp64(c_k)*fp64(q_k))
 *     with the canonical fp64 summation order (oracle/scan_ref.c); result = top-k rows by
 *     (score desc, row asc), optionally restricted per query to rows whose tag satisfies
 *     (tag & tag_mask) == tag_value (the payload `must` filter, main.py:218-236).
 *     Missing results (fewer than k matching rows) are reported as id -1, score -inf.
 *   - edges: a vector whose canonical sumsq is not finite, or is zero, normalises to the zero
 *     vector: fp32 +0.0 in every element, so fp16 0x0000. fp32 squares of dim <= 1024 elements
 *     cannot overflow fp64, so sumsq is non-finite exactly when some component is non-finite
 *     (inf or NaN). Finite inputs keep every bit. This holds for upserted vectors, queries and
 *     recommend examples alike. A zero query scores +0.0 against every row; the ranking is
 *     then row ascending. The imports (rag_index_import_rows[32]) write caller bits and so
 *     refuse, with RAG_EINVAL naming the first offending row and the index unchanged, a row
 *     with a non-finite element or with an fp64 L2 norm above 1.001, the row norm every
 *     exactness certificate assumes. Candidate scores handed in from outside (rag_index_mmr,
 *     rag_group_select, rag_fuse_rrf, rag_formula_rescore) are not checked.
 */
#ifndef RAGMI_H
#define RAGMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  RAG_OK = 0,
  RAG_EINVAL = -1,   /* bad argument */
  RAG_EHIP = -2,     /* HIP runtime error */
  RAG_ENOMEM = -3,   /* device allocation failed */
  RAG_ERANGE = -4,   /* row slot beyond capacity, k too large, ... */
};

/* Largest k a single search may ask for (the reference uses limit=15, main.py:215).
 * Exactness is unconditional for every k <= RAG_MAX_K: the result is always the exact top-k
 * by (canonical score desc, row asc). The scan ranks rows by MFMA score (fp16 query, fp32
 * accumulation) and re-scores its approximate top-32 exactly; a per-query bound eps on
 * |MFMA score - exact score| (computed at query prep) certifies the result when the k-th
 * exact score exceeds the 32nd approximate score + eps. When it does not (near-duplicate
 * rows, k close to 32), every row whose MFMA score is >= (k-th exact score - eps) is
 * re-scored exactly, from the scan's per-wave lists when they provably hold all of them,
 * otherwise by a second pass over the shard (see rag_index_exactness_stats). */
#define RAG_MAX_K 32
/* Largest k of the large-k pass (round 5; Qdrant's query_points takes any `limit`,
 * main.py:215,232-237). RAG_MAX_K < k <= RAG_MAX_K_LARGE runs a separate exact pass per 32
 * queries: a sampled certified lower bound of each query's k-th best score, every row whose
 * MFMA score can reach it collected, all of those re-scored exactly, the k best by (score
 * desc, row asc) emitted — the same exact result and canonical scores as the k <= 32 path
 * (largek_kernels.hip, "Exact top-k for RAG_MAX_K < k"). rag_index_search_packed accepts k
 * up to this. rag_index_search itself takes ANY k >= 1: k > RAG_MAX_K_LARGE runs the full
 * exact pass (rag_index_search_full, round 6), and rag_merge_topk[_packed] merge any k (past
 * this by three stable radix sorts per query). */
#define RAG_MAX_K_LARGE 4096
/* Queries handled per scan pass; larger batches run ceil(B/32) passes. */
#define RAG_QUERY_TILE 32

typedef struct rag_index rag_index_t;

/* Last error message of the calling thread ("" if none). */
const char* rag_last_error(void);
/* Library version string. */
const char* rag_version(void);

/* Create an empty flat index of `dim`-dimensional vectors (dim % 32 == 0; 384 and 1024 are
 * built) with room for `capacity_rows` rows on HIP device `device`.
 * Replaces QdrantClient.create_collection(vectors_config=VectorParams(size, COSINE)),
 * ingest.py:86-96. */
int rag_index_create(int dim, int64_t capacity_rows, int device, rag_index_t** out);

/* Vector storage of an index. RAG_STORE_FP16: the normalised rows rounded to fp16 (RNE) —
 * the scan's operand, 2 B per element; scores are exact on the fp16 rows. RAG_STORE_FP32
 * (Qdrant's default Float32 datatype: VectorParams without `datatype`, database.py:124-130,
 * ingest.py:89-95): the normalised fp32 rows are kept as well (4 B more per element) and the
 * exact scores read them — score(row) = fp32(sum_k fp64(y_k) fp64(q_k)) over the fp32 row y,
 * ranking identical to an fp32 store — while the scan still streams the fp16 copy (the
 * certified select's error bound grows by ||fp16(y) - y|| <= 2^-11 ||y||). */
enum { RAG_STORE_FP16 = 0, RAG_STORE_FP32 = 1 };
/* Flag OR-ed into rag_index_create_ex's `storage` (and rag_encoder_create_ex's `flags`): the
 * process then honours the RAGMI_* environment knobs that switch kernels for A/B measurements
 * (scan / rescan grids, seed sample, GEMM and attention variants). Without it every knob reads
 * as its production default and a set knob is reported once on stderr. Diagnostic only:
 * several knobs trade the worst-case latency or the certificate's fallback for timing. */
#define RAG_CREATE_DIAGNOSTIC 0x100
/* The value the library uses for the integer knob `name` (a RAGMI_* variable): the variable's
 * value when it is set and diagnostics are on, else `dflt` (reporting an ignored variable
 * once on stderr). Runs the same code path as every knob site; for tests. */
int rag_knob_probe(const char* name, int dflt);
/* 1 in a diagnostic build of the library (-DRAGMI_DIAG_BUILD, out of tree: `python
 * ragmi/_build.py OUT.so -DRAGMI_DIAG_BUILD`), whose rag_bench_scan / rag_bert_attention also
 * carry the measured timing probes and kernel variants; 0 in the production libragmi.so
 * (rag_bench_scan variants 0 / 7, rag_bert_attention -1 / 42 / 10 only). */
int rag_diagnostic_build(void);
/* rag_index_create with an explicit storage (rag_index_create = RAG_STORE_FP16). */
int rag_index_create_ex(int dim, int64_t capacity_rows, int device, int storage,
                        rag_index_t** out);
/* RAG_STORE_FP16 / RAG_STORE_FP32 of an index (-1 for NULL). */
int rag_index_storage(const rag_index_t* index);
int rag_index_destroy(rag_index_t* index);

/* Grow capacity (keeps contents). */
int rag_index_reserve(rag_index_t* index, int64_t capacity_rows);
int64_t rag_index_capacity(const rag_index_t* index);
int64_t rag_index_count(const rag_index_t* index);
int rag_index_dim(const rag_index_t* index);

/* Write n vectors (fp32 [n][dim], device) into the row slots rows_dev[i] (int64, device);
 * tags_dev (uint32 [n], device) may be NULL (tag 0). `new_count` is the number of valid rows
 * after this upsert (rows >= new_count are ignored by search). Replaces qdrant.upsert,
 * ingest.py:171-175. */
int rag_index_upsert(rag_index_t* index, const float* vecs_dev, const int64_t* rows_dev,
                     const uint32_t* tags_dev, int64_t n, int64_t new_count, void* stream);
/* Same, host pointers, synchronous. */
int rag_index_upsert_host(rag_index_t* index, const float* vecs_host, const int64_t* rows_host,
                          const uint32_t* tags_host, int64_t n, int64_t new_count);

/* Top-k search of B queries (fp32 [B][dim], device). Outputs: out_scores_dev fp32 [B][k],
 * out_ids_dev int64 [B][k] (row + id_offset, or -1). filters_dev is NULL (no filter) or
 * uint32 [B][2] = (tag_mask, tag_value) per query: row r qualifies for query b iff
 * (tag[r] & tag_mask) == tag_value ((0,0) = every row). One scan serves a whole micro-batch
 * whose requests filter on different tickers (main2.py:228 per request).
 * Replaces QdrantClient.query_points, main.py:232-237. */
int rag_index_search(rag_index_t* index, const float* queries_dev, int B, int k,
                     const uint32_t* filters_dev, int64_t id_offset,
                     float* out_scores_dev, int64_t* out_ids_dev, void* stream);
/* rag_index_search by the full exact pass, for any k >= 1: per query every row is scored
 * exactly (the canonical fp64 order), the (score, row) pairs are radix-sorted (stable, score
 * descending, so ties stay row-ascending) and the first k emitted, -1 / -inf past the
 * matching rows. The same result as rag_index_search at every k; ~ms per query at 10M rows.
 * rag_index_search takes it for k > RAG_MAX_K_LARGE; callers take it to re-answer a query a
 * large-k pass left unanswered (rag_index_unanswered). No reference counterpart beyond
 * query_points(limit) itself (main.py:232-237). */
int rag_index_search_full(rag_index_t* index, const float* queries_dev, int B, int k,
                          const uint32_t* filters_dev, int64_t id_offset,
                          float* out_scores_dev, int64_t* out_ids_dev, void* stream);
/* Same, host pointers (filters_host may be NULL), synchronous. */
int rag_index_search_host(rag_index_t* index, const float* queries_host, int B, int k,
                          const uint32_t* filters_host, int64_t id_offset,
                          float* out_scores_host, int64_t* out_ids_host);

/* Multi-GPU exchange form of rag_index_search: the result is written as ONE array
 * out_packed [B][k][2] int32 = (fp32 score bits, global row id = local row + id_offset; -1
 * where fewer than k rows match), so the per-shard lists travel in a single all-gather.
 * Global row ids must stay below 2^31. */
int rag_index_search_packed(rag_index_t* index, const float* queries_dev, int B, int k,
                            const uint32_t* filters_dev, int64_t id_offset, int32_t* out_packed_dev,
                            void* stream);

/* Copy stored rows [row0, row0+n) out as row-major fp16 bits ([n][dim] uint16, host). */
int rag_index_export_rows(rag_index_t* index, int64_t row0, int64_t n, uint16_t* out_host);
/* Load already-stored rows back (persistence): row-major fp16 bits [n][dim] (host) are
 * written to rows [row0, row0+n) unchanged (no renormalisation), tags (host, may be NULL)
 * likewise; `new_count` = valid rows afterwards. Synchronous. Checked on the host before
 * anything is copied: a row with a non-finite element (fp16: all exponent bits set) or an fp64
 * L2 norm above 1.001 is refused with RAG_EINVAL, the message naming the first such row, and
 * the index stays unchanged ("edges" above). rag_index_import_rows32 checks alike. */
int rag_index_import_rows(rag_index_t* index, int64_t row0, int64_t n, const uint16_t* rows_host,
                          const uint32_t* tags_host, int64_t new_count);
/* fp32 storage: copy the stored fp32 rows [row0, row0+n) out ([n][dim] float, host), and
 * load saved fp32 rows back (their fp16 scan copy is re-derived by the same RNE rounding, so
 * a reloaded index is bit-identical). rag_index_import_rows is refused on fp32 storage. */
int rag_index_export_rows32(rag_index_t* index, int64_t row0, int64_t n, float* out_host);
int rag_index_import_rows32(rag_index_t* index, int64_t row0, int64_t n, const float* rows_host,
                            const uint32_t* tags_host, int64_t new_count);
/* Copy stored tags of rows [row0, row0+n) to host. */
int rag_index_export_tags(rag_index_t* index, int64_t row0, int64_t n, uint32_t* out_host);

/* Row removal (QdrantClient.delete; the reference itself only upserts, ingest.py:171-175, and
 * leaves deletion to the Qdrant server it talks to). A deleted row is physically removed: a
 * surviving row from the tail is moved into its slot and the count shrinks, so the index stays
 * dense and every search kernel runs unchanged. Removal rule (ragmi.index.plan_removal, the
 * one every layer follows): with D the distinct deleted rows and n1 = count - |D|, the holes
 * D ∩ [0, n1) ascending receive the survivors of [n1, count) ascending, pair by pair; no other
 * row moves; the new count is n1. All four calls are asynchronous on `stream`, take the
 * handle's lock and never dereference a row index outside [0, capacity): such a pair is
 * skipped.
 *
 * rag_index_select_rows: the rows r < count with (tag[r] & tag_mask) == tag_value, ascending,
 * into out_rows_dev (int64, device) — at most `cap` of them, the first `cap` matches, nothing
 * past out_rows_dev[cap - 1] — and the total number of matches into *out_n_dev (int64,
 * device), also when it exceeds `cap`. cap = 0 with out_rows_dev NULL is a pure count; (0, 0)
 * selects every row. The order of the output is deterministic (count / prefix sum / emit). */
int rag_index_select_rows(rag_index_t* index, uint32_t tag_mask, uint32_t tag_value,
                          int64_t* out_rows_dev, int64_t cap, int64_t* out_n_dev, void* stream);
/* Copy every stored form of row src_rows_dev[i] into slot dst_rows_dev[i] (int64 [n], device):
 * the fp16 tile16 pieces, the fp32 row of an fp32-storage index, the tag and the key of every
 * key column ("Key columns" below), bit for bit (no renormalisation), one read and one write per
 * byte; then count = new_count.
 * Precondition: the src and dst sets are disjoint (a row is never both read and written). */
int rag_index_move_rows(rag_index_t* index, const int64_t* src_rows_dev,
                        const int64_t* dst_rows_dev, int64_t n, int64_t new_count, void* stream);
/* The same copy through a packed row-major staging form, for moves between the shards of a set:
 * [n][dim] fp16 bits, [n][dim] fp32, [n] tags (device). gather reads rows rows_dev[i] (at any
 * slot below capacity, the count is not consulted or changed) into staging row i; scatter
 * writes staging row i to slot rows_dev[i] (distinct slots) and sets count = new_count. The
 * f32 pointer is required exactly when storage is RAG_STORE_FP32 (NULL otherwise); the fp16
 * and tag pointers always. The indexed, device-side counterparts of rag_index_export_rows /
 * rag_index_import_rows. */
int rag_index_gather_rows(rag_index_t* index, const int64_t* rows_dev, int64_t n,
                          uint16_t* out_f16_dev, float* out_f32_dev, uint32_t* out_tags_dev,
                          void* stream);
int rag_index_scatter_rows(rag_index_t* index, const int64_t* rows_dev, int64_t n,
                           const uint16_t* in_f16_dev, const float* in_f32_dev,
                           const uint32_t* in_tags_dev, int64_t new_count, void* stream);

/* MMR (maximal marginal relevance): re-select k diverse hits from each query's exact top-C
 * candidate list (rag_index_search at k = C: cand_scores_dev fp32 [B][C], cand_rows_dev int64
 * [B][C] rows of THIS index, -1 = none). The candidates of query b are the first n_b entries,
 * n_b = min(ncand_dev[b] (NULL = C), the leading entries whose row lies in [0, capacity)): a
 * row outside that range counts as absent, ends the list and is never dereferenced; rows are
 * read at any slot below capacity, as rag_index_gather_rows reads them. Step 0 selects
 * candidate 0. After selecting s, maxsim[j] = max(maxsim[j], sim(s, j)) in fp32 for every
 * unselected j (from -inf), sim(s, j) being the canonical exact score of stored row r_j against
 * the stored row r_s as an fp32 vector (fp16 storage: the halves widened) — the arithmetic of
 * every exact score here, fp64 fma in the canonical order and one rounding to fp32. Step t >= 1
 * selects the unselected j with the largest
 *     val[j] = (double)(1.0f - div) * (double)score[j] - (double)div * (double)maxsim[j],
 * div = diversity_dev[b] (fp32, in [0, 1]: the caller's check), ties to the smallest j. It
 * stops after k picks or n_b. Outputs in selection order, [B][k]: the candidate's score,
 * its row, and (out_pos_dev, may be NULL) its position j in the list; -inf / -1 / -1 past the
 * last pick. Diversity 0 returns the first k candidates unchanged; the first k' picks of a run
 * at k are the run at k'. 1 <= C <= RAG_MMR_MAX_CANDIDATES, k >= 1, B >= 0; argument errors
 * are refused on the host before any HIP call. Asynchronous on `stream`. Qdrant's counterpart
 * is NearestQuery(nearest, mmr=Mmr(diversity, candidates_limit)); the reference never asks for
 * it, and parity with Qdrant's own MMR arithmetic is unpinned. */
#define RAG_MMR_MAX_CANDIDATES 1024
int rag_index_mmr(rag_index_t* index, const float* cand_scores_dev, const int64_t* cand_rows_dev,
                  int B, int C, int k, const float* diversity_dev, const int32_t* ncand_dev,
                  float* out_scores_dev, int64_t* out_ids_dev, int32_t* out_pos_dev, void* stream);

/* Grouped search (Qdrant's query_points_groups(group_by, limit = G, group_size = S)): the G best
 * groups of rows sharing a key, each with its S best hits. The key of row r is
 * tag[r] & key_mask, key_mask being the 16 tag bits of the group_by field; key 0 (field absent)
 * belongs to no group. Definition, for one query with filter (mask, value): the ranked list is
 * every row r < count that passes the filter and has key(r) != 0, ordered by (canonical exact
 * score desc, row asc) — rag_index_search's order and scores. Walk it in order: a row whose key
 * was not seen yet opens the next group while fewer than G are open; a row of an open group with
 * fewer than S hits is appended to it; every other row is skipped. Result: the groups in opening
 * order (by best hit), each with its hits in list order. The ladder that makes this exact from
 * candidate lists (ragmi.groups) is host logic over these two calls and
 * rag_index_search. The reference never groups (it over-fetches a flat top-15, main.py:215), and
 * parity with a Qdrant server's own grouped search, which is best-effort, is unpinned.
 *
 * rag_index_gather_tags: out_tags_dev[i] = tag[rows_dev[i]] (int64 [n] -> uint32 [n], device)
 * for rows in [0, capacity), 0 otherwise: a row index outside that range is never dereferenced.
 * Asynchronous on `stream`, under the handle's lock.
 *
 * rag_group_select: the walk above over candidate lists — cand_scores_dev fp32 [B][C],
 * cand_rows_dev int64 [B][C] (-1 = none), cand_tags_dev uint32 [B][C] (rag_index_gather_tags of
 * the rows). Index-free like rag_merge_topk: it reads only its input arrays and runs on the
 * calling thread's current device. The candidates of query b are the first n_b entries, n_b =
 * min(ncand_dev[b] (NULL = C; clamped to [0, C]), the leading entries with row >= 0). Outputs,
 * every element written by the launch: out_keys_dev uint32 [B][G], the groups' keys in opening
 * order, 0 past the last group; out_fill_dev int32 [B][G], hits per group; out_scores_dev fp32
 * [B][G][S] (-inf padding), out_rows_dev int64 [B][G][S] (-1 padding) and out_pos_dev int32
 * [B][G][S] (the hit's position j in its list, -1 padding; may be NULL); out_count_dev int32
 * [B][2] = (number of groups, n_b). Deterministic, equal to the sequential walk. Limits, refused
 * on the host before any HIP call: 1 <= C <= RAG_GROUPS_MAX_CANDIDATES, 1 <= G <= RAG_GROUPS_MAX,
 * S >= 1, G * S <= RAG_GROUPS_MAX_CELLS (RAG_ERANGE); key_mask != 0, B >= 0, non-NULL pointers
 * (RAG_EINVAL); B = 0 launches nothing. Asynchronous on `stream`. */
#define RAG_GROUPS_MAX_CANDIDATES 4096 /* = RAG_MAX_K_LARGE */
#define RAG_GROUPS_MAX 1024
#define RAG_GROUPS_MAX_CELLS 4096
int rag_index_gather_tags(rag_index_t* index, const int64_t* rows_dev, int64_t n,
                          uint32_t* out_tags_dev, void* stream);
int rag_group_select(const float* cand_scores_dev, const int64_t* cand_rows_dev,
                     const uint32_t* cand_tags_dev, const int32_t* ncand_dev, int B, int C,
                     uint32_t key_mask, int G, int S, uint32_t* out_keys_dev, int32_t* out_fill_dev,
                     float* out_scores_dev, int64_t* out_rows_dev, int32_t* out_pos_dev,
                     int32_t* out_count_dev, void* stream);

/* Fusion queries (Qdrant's query_points(prefetch = [Prefetch(...), ...], query =
 * FusionQuery(Fusion.RRF))): the L candidate lists of a request fused by reciprocal rank.
 * Index-free like rag_group_select: it reads only its input arrays (cand_rows_dev int64
 * [B][L][C], -1 = none; ncand_dev int32 [B][L] or NULL = C everywhere), runs on the calling
 * thread's current device and is asynchronous on `stream`.
 *
 * Entries. For request b and list l the entries are the first n_{b,l} positions, n_{b,l} =
 * min(ncand_dev[b][l] clamped to [0, C], the number of leading entries with row >= 0): a negative
 * row ends its list. Rows are opaque int64 ids, compared and copied, never dereferenced; they may
 * exceed 2^31 (global ids).
 *
 * Fused score. An entry at 0-based position p contributes c(p) = 1.0 / (double)(rrf_k + p), one
 * correctly rounded fp64 division. For a distinct row r, fused(r) = (float)(sum of c(p)) over
 * every entry holding r: the contributions are added in fp64 in (list ascending, position
 * ascending) order from 0.0, and the sum is rounded once to fp32. A row that appears twice in
 * one list (a search never produces that, a caller may) contributes twice.
 *
 * Result. The distinct rows ordered by (fused fp32 value descending, row ascending); the first k
 * go to out_scores_dev fp32 [B][k] and out_rows_dev int64 [B][k], -inf / -1 past the last
 * distinct row; out_count_dev int32 [B] (may be NULL) is the number of distinct rows, which may
 * exceed k. Every output element is written by the launch, and the result is a pure function of
 * the inputs (no floating-point atomics). So L = 1 returns the list unchanged with scores
 * (float)(1.0 / (rrf_k + p)), and the first k' outputs of a run at k are the run at k'.
 *
 * Limits, refused on the host before any HIP call: 1 <= L <= RAG_FUSION_MAX_LISTS, C >= 1,
 * L * C <= RAG_FUSION_MAX_ENTRIES (RAG_ERANGE); k >= 1, rrf_k >= 1, B >= 0, non-NULL
 * cand_rows_dev / out_scores_dev / out_rows_dev (RAG_EINVAL); B = 0 launches nothing. The
 * arithmetic is this project's definition, modelled on Qdrant's published RRF (reciprocal of
 * position plus a constant, default 2); the reference never fuses, and parity with a Qdrant
 * server's own fusion is unpinned. */
#define RAG_FUSION_MAX_LISTS 16
#define RAG_FUSION_MAX_ENTRIES 4096 /* L * C */
int rag_fuse_rrf(const int64_t* cand_rows_dev, const int32_t* ncand_dev, int B, int L, int C,
                 int k, int rrf_k, float* out_scores_dev, int64_t* out_rows_dev,
                 int32_t* out_count_dev, void* stream);

/* Formula queries (Qdrant's query_points(prefetch = [Prefetch(...), ...], query =
 * FormulaQuery(formula, defaults))): the candidates of a request's L exact lists re-scored by an
 * arithmetic formula over their scores, their payload keys and filter conditions. Index-free like
 * rag_fuse_rrf: it reads only its input arrays, runs on the calling thread's current device and
 * is asynchronous on `stream`. The arithmetic is this project's definition, modelled on Qdrant's
 * published formula expressions (sum, mult, div, neg, abs, lin / exp / gauss decay, conditions as
 * 1.0 / 0.0); the reference never re-scores, and parity with a Qdrant server's own arithmetic is
 * unpinned.
 *
 * Candidates. Lists and their ends are rag_fuse_rrf's: for request b and list l the entries are
 * the first n_{b,l} positions, n_{b,l} = min(ncand_dev[b][l] clamped to [0, C], the number of
 * leading entries with row >= 0). The candidates are the distinct rows of the live entries; rows
 * are opaque int64 ids. A row that occurs several times within one list contributes its first
 * occurrence; its tag and keys are read at the slot e = l * C + p of its first entry in (list,
 * position) order.
 *
 * Formula programs. A formula is a postfix program of at most RAG_FORMULA_MAX_OPS ops over an
 * evaluation stack of fp64 values, at most RAG_FORMULA_MAX_STACK deep, the same for every
 * candidate of the launch. The device blob (uint32 words, `words` of them):
 *   word 0    n, the op count;   word 1    U, the number of condition programs (<=
 *             RAG_FORMULA_MAX_CONDS)
 *   words [2 + 6 i, 8 + 6 i), i < n: op i = (kind, arg, flags, 0, imm low, imm high), imm one fp64
 *   words [2 + 6 n, words): when U > 0, a "Filter programs" blob of U programs (their INSET /
 *             RANGE offsets count from this blob's own first word)
 * Op kinds (x, y popped: y the top of the stack; every arithmetic step one IEEE fp64 operation,
 * never contracted into an fma):
 *   RAG_FORMULA_CONST   push imm
 *   RAG_FORMULA_SCORE   push (double)score of the candidate's entry in list arg; a candidate
 *                       absent from that list: imm when flags & 1, else status bit 0 and 0.0
 *   RAG_FORMULA_KEY     the key k of column arg (cand_keys[arg][b][e]): push the double whose
 *                       key it is ("Key columns"), divided by 1e6 when flags & 2 (a datetime
 *                       column: microseconds to seconds); k == RAG_KEY_ABSENT: imm when
 *                       flags & 1, else status bit 0 and 0.0
 *   RAG_FORMULA_COND    push 1.0 when (tag, keys) of the candidate passes condition program arg,
 *                       else 0.0; a RANGE atom on a column that was not supplied is false
 *   RAG_FORMULA_ADD     push x + y        RAG_FORMULA_MUL   push x * y
 *   RAG_FORMULA_NEG     push -y           RAG_FORMULA_ABS   push |y|
 *   RAG_FORMULA_DIV     push x / y; when y == 0.0: imm when flags & 1, else status bit 1
 *   RAG_FORMULA_LIN     d = |x - y|; t = 1.0 - imm * d; push t when t > 0.0, else 0.0
 *   RAG_FORMULA_EXP     d = |x - y|; push E(imm * d)
 *   RAG_FORMULA_GAUSS   d = |x - y|; push E(imm * (d * d))
 * (for the decays x is the variable, y the target and imm the coefficient lambda the host derives
 * from scale and midpoint). E, the decay exponential, for a <= 0: 0.0 when a < -700; otherwise
 * n = rint(a * 1.4426950408889634), r = (a - n * 6.93147180369123816490e-01) - n *
 * 1.90821492927058770002e-10, p = the degree-13 Taylor polynomial of e^r by Horner (coefficients
 * 1 / i! as correctly rounded doubles; each step one multiply, then one add), E = p * 2^n
 * (exact). E(a) is NaN for a > 0 or a NaN. Relative error against a correctly rounded exp over
 * [-700, 0]: at most 2.0 * 2^-53 (measured, 6M arguments).
 *
 * Value and result. After the last op the one value left is rounded once to fp32, -0.0 taken as
 * +0.0. The distinct rows ordered by (value descending, row ascending); the first k go to
 * out_scores_dev fp32 [B][k] and out_rows_dev int64 [B][k], -inf / -1 past the last distinct row;
 * out_count_dev int32 [B] (may be NULL) is the number of distinct rows. out_status_dev uint32 [B]:
 * bit 0 a variable without a value and without a default, bit 1 a division by zero without a
 * default or a final fp32 value that is not finite, bit 2 a bad program. For a request whose
 * status is non-zero the other outputs are written but unspecified. Every output element is
 * written by the launch; no floating-point atomics, so the result is a pure function of the
 * inputs, and the first k' outputs of a run at k are the run at k'.
 *
 * The blob is never trusted. It is bad (bit 2 for every request, no op evaluated) when words < 2,
 * n > RAG_FORMULA_MAX_OPS, U > RAG_FORMULA_MAX_CONDS, the op records or the U program records end
 * past `words`, a kind is unknown, the stack would drop below its operands or rise above
 * RAG_FORMULA_MAX_STACK, it does not end at depth 1, a SCORE names a list >= L, a KEY names a
 * column >= RAG_KEYS_MAX_COLS or one whose pointer is NULL, a COND names a program >= U or
 * cand_tags_dev is NULL. A condition program reads the blob as filter_view_kernel does: a word
 * only when its index is < words. So a malformed blob never reads or writes outside the blob,
 * the inputs and the outputs.
 *
 * cand_keys: a HOST array of RAG_KEYS_MAX_COLS device pointers (int64 [B][L][C] each, the keys
 * of the candidates' rows: rag_index_gather_keys), NULL = column not supplied; the array itself
 * may be NULL (no column). cand_tags_dev: uint32 [B][L][C] (rag_index_gather_tags) or NULL.
 * Limits and refusals are rag_fuse_rrf's, on the host before any HIP call: 1 <= L <=
 * RAG_FUSION_MAX_LISTS, C >= 1, L * C <= RAG_FUSION_MAX_ENTRIES (RAG_ERANGE); k >= 1, B >= 0,
 * words >= 2, non-NULL cand_scores_dev / cand_rows_dev / prog_dev / out_scores_dev /
 * out_rows_dev / out_status_dev (RAG_EINVAL); B = 0 launches nothing. */
#define RAG_FORMULA_MAX_OPS 64
#define RAG_FORMULA_MAX_STACK 8
#define RAG_FORMULA_MAX_CONDS 8
#define RAG_FORMULA_HDR_WORDS 2
#define RAG_FORMULA_OP_WORDS 6
enum {
  RAG_FORMULA_CONST = 0, RAG_FORMULA_SCORE = 1, RAG_FORMULA_KEY = 2, RAG_FORMULA_COND = 3,
  RAG_FORMULA_ADD = 4, RAG_FORMULA_MUL = 5, RAG_FORMULA_NEG = 6, RAG_FORMULA_ABS = 7,
  RAG_FORMULA_DIV = 8, RAG_FORMULA_LIN = 9, RAG_FORMULA_EXP = 10, RAG_FORMULA_GAUSS = 11,
};
#define RAG_FORMULA_MISSING 1u     /* status bit 0 */
#define RAG_FORMULA_NONFINITE 2u   /* status bit 1 */
#define RAG_FORMULA_BAD 4u         /* status bit 2 */
int rag_formula_rescore(const float* cand_scores_dev, const int64_t* cand_rows_dev,
                        const uint32_t* cand_tags_dev, const int64_t* const* cand_keys,
                        const int32_t* ncand_dev, const uint32_t* prog_dev, int64_t words, int B,
                        int L, int C, int k, float* out_scores_dev, int64_t* out_rows_dev,
                        int32_t* out_count_dev, uint32_t* out_status_dev, void* stream);

/* Merge n_lists per-shard result lists (each [B][k] sorted by (score desc, id asc), device;
 * laid out [n_lists][B][k]; padding: id -1) into the global top-k [B][k] (device) by (score
 * desc, id asc), padding -inf / -1 past the valid entries. Any k >= 1 (k > RAG_MAX_K_LARGE:
 * stream-ordered scratch of ~36 B per entry). Used after the RCCL all-gather of per-shard
 * results. */
int rag_merge_topk(const float* in_scores_dev, const int64_t* in_ids_dev, int n_lists, int B,
                   int k, float* out_scores_dev, int64_t* out_ids_dev, void* stream);
/* Same merge over the packed exchange form ([n_lists][B][k][2] int32, see
 * rag_index_search_packed) gathered from all shards. */
int rag_merge_topk_packed(const int32_t* in_packed_dev, int n_lists, int B, int k,
                          float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* The same merge over n_lists SEPARATE packed lists (each int32 [B][k][2] of shard-local rows,
 * see rag_index_search_packed): `lists` is a host array of n_lists device pointers, and a valid
 * local row r of list l becomes the global id r * id_mul + id_add_host[l] (int64) before the
 * merge by (score desc, id asc) — gather, id remap and merge in one launch; the pointer table
 * and the offsets travel in the kernel arguments, nothing is uploaded. out_empty_dev (uint8
 * [n_lists][B], may be NULL) receives 1 where list l holds no entry for query b (its first id
 * is -1), else 0. 1 <= n_lists <= RAG_MAX_SHARDS, 1 <= k <= RAG_MAX_K_LARGE. The merge of
 * rag_shardset_search; no reference counterpart (the reference's Qdrant is one node). */
#define RAG_MAX_SHARDS 64
int rag_merge_topk_gather(const int32_t* const* lists, int n_lists, int B, int k, int64_t id_mul,
                          const int64_t* id_add_host, float* out_scores_dev, int64_t* out_ids_dev,
                          uint8_t* out_empty_dev, void* stream);

/* Shard set: n_shards flat indexes (same dim and storage; on any devices, several may share
 * one) searched as ONE index from one process — a Qdrant collection spanning the GPUs of a
 * node behind the same query_points (main.py:232-237). Placement is striped: global row g
 * lives on shard g % n_shards at local row g / n_shards, so a collection that grows by upsert
 * (ingest.py:171-175, no total known in advance) fills every shard evenly, and local order is
 * global order: each shard's exact top-k by (score desc, local row asc) is its exact top-k in
 * global rows, and the merged list equals the unsharded index's bit for bit. The set borrows
 * the shard handles: the caller upserts into them (rag_index_upsert at the local rows), keeps
 * them alive while the set lives and destroys them afterwards. */
typedef struct rag_shardset rag_shardset_t;
int rag_shardset_create(rag_index_t* const* shards, int n_shards, rag_shardset_t** out);
int rag_shardset_destroy(rag_shardset_t* set);
/* rag_index_search over the set: out_scores_dev fp32 [B][k], out_ids_dev int64 [B][k] in
 * global rows (-1 / -inf past the matching rows). Asynchronous on `stream`, a stream of the
 * merge device (shard 0's), where queries, filters and outputs live. Every shard searches on a
 * stream of its own behind `stream` (one event out, one event back per shard); a shard on
 * another device gets the queries and filters by hipMemcpyPeerAsync and its packed list is
 * copied back the same way (no kernel reads another GPU's memory); then one
 * rag_merge_topk_gather launch on `stream`. k > RAG_MAX_K_LARGE, or flags & RAG_SHARDSET_FULL
 * (every shard answers by rag_index_search_full): unpacked per-shard lists, an id-remap kernel
 * and rag_merge_topk. out_empty_dev (uint8 [n_shards][B], may be NULL): 1 where shard s
 * returned nothing for query b — no matching row there, or a large-k pass that left the query
 * unanswered (rag_index_unanswered on the shard tells which; re-run such queries with
 * RAG_SHARDSET_FULL). Re-entrant like an index: searches from several threads on several
 * streams are safe (per-search buffers in event-guarded slots). The calling thread's current
 * HIP device is restored on return. */
#define RAG_SHARDSET_FULL 1
int rag_shardset_search(rag_shardset_t* set, const float* queries_dev, int B, int k,
                        const uint32_t* filters_dev, int flags, float* out_scores_dev,
                        int64_t* out_ids_dev, uint8_t* out_empty_dev, void* stream);

/* Filter programs (the filter algebra: should, must_not, min_should, MatchAny, MatchExcept,
 * is-empty, nested filters; ragmi.filters compiles a Qdrant Filter into one). A program has at
 * most RAG_FILTER_MAX_ATOMS atoms and a 256-bit truth table over them: a row passes iff bit
 * idx of the table is set, idx = sum over atoms i of atom_i(tag) << i. Atom kinds:
 *   RAG_FILTER_ATOM_MASKEQ (p0 = mask, p1 = value):  (tag & mask) == value
 *   RAG_FILTER_ATOM_INSET  (p0 = field f, p1 = bitmap word offset, p2 = bitmap length in bits):
 *       with code = (tag >> 16 f) & 0xFFFF: code < p2 and bit code of the bitmap is set
 *       (bit b of a bitmap is bit b % 32 of its word b / 32).
 * The device blob for U programs (uint32 words, `words` of them):
 *   words [s * 41, (s + 1) * 41), s < U: program s's record —
 *       [0]       atom count (read clamped to RAG_FILTER_MAX_ATOMS)
 *       [1..8]    the truth table, bit idx = bit idx % 32 of word 1 + idx / 32
 *       [9 + 4 i .. 12 + 4 i], i < 8: atom i = (kind, p0, p1, p2); unused atoms are zero
 *   words [41 U, words): the bitmap pool; an INSET atom's p1 is a word offset from the blob's
 *       start.
 *   RAG_FILTER_ATOM_RANGE  (p0 = key column, p1 = word offset of the bounds, p2 = 0):
 *       with key = keys[p0][row] (the index's key columns, below): key != RAG_KEY_ABSENT and
 *       lo <= key <= hi as signed 64-bit integers. The bounds are 4 words of the pool, at p1:
 *       lo low, lo high, hi low, hi high. An absent key is in no range.
 * The blob is never trusted: a bitmap word is read only when its index is < words (a code whose
 * word lies outside is "not a member"), and a RANGE atom is false, with neither its bounds nor a
 * key read, when p0 >= the index's number of key columns or p1 + 3 >= words; so a malformed
 * blob gives wrong bits, never a read outside the blob or a column. An index WITHOUT key columns
 * runs the kernel of the releases before RANGE existed, to which kind 2 is an unknown kind, read
 * as MASKEQ like every unknown kind: create the columns (rag_index_keys_create) before sending
 * RANGE atoms.
 *
 * rag_index_filter_view: out_view_dev[r] (uint32 [capacity], 16-byte aligned, device) = sum
 * over s < n_programs of pass_s(tag[r]) << s for r < count, 0 for count <= r < capacity; nothing
 * past out_view_dev[capacity - 1] is written. One streaming launch: 4 B read and 4 B written per
 * row, plus 8 B read per row for every key column that a RANGE atom of the blob names (each such
 * column is read once, however many atoms name it).
 * rag_index_search_view: rag_index_search over that view instead of the stored tags, under one
 * hold of the handle's lock: filter_view_kernel runs once on `stream` ahead of the first pass
 * into a view column the handle keeps per stream (4 B per row of capacity, allocated on a
 * stream's first view call, freed with the handle), and every pass of the call reads that
 * view. filters_dev [B][2] are ordinary
 * (mask, value) pairs over the VIEW's bits: (1 << s, 1 << s) asks for program s, (0, 0) for
 * every row; NULL = no query filters. flags: RAG_SEARCH_FULL forces the full exact pass.
 * out_packed_dev non-NULL: the packed form of rag_index_search_packed (k <= RAG_MAX_K_LARGE,
 * global rows below 2^31) and the two other outputs are ignored; NULL: out_scores_dev and
 * out_ids_dev as rag_index_search writes them.
 * rag_index_select_rows_view: rag_index_select_rows of the rows passing ONE program (the blob's
 * first record).
 * rag_shardset_search_view: rag_shardset_search with the view search on every shard; the blob
 * travels to a shard on another device as the filters do.
 * Argument errors (NULL blob, n_programs outside [1, RAG_FILTER_MAX_PROGRAMS], words < 41 *
 * n_programs, the k / packed rules of the plain calls) are refused before any HIP call. All four
 * are asynchronous on `stream`. */
#define RAG_FILTER_MAX_ATOMS 8
#define RAG_FILTER_MAX_PROGRAMS 32
#define RAG_FILTER_REC_WORDS 41
#define RAG_FILTER_ATOM_MASKEQ 0
#define RAG_FILTER_ATOM_INSET 1
#define RAG_FILTER_ATOM_RANGE 2
#define RAG_SEARCH_FULL 1
int rag_index_filter_view(rag_index_t* index, const uint32_t* progs_dev, int64_t words,
                          int n_programs, uint32_t* out_view_dev, void* stream);
int rag_index_search_view(rag_index_t* index, const float* queries_dev, int B, int k,
                          const uint32_t* progs_dev, int64_t words, int n_programs,
                          const uint32_t* filters_dev, int64_t id_offset, int flags,
                          float* out_scores_dev, int64_t* out_ids_dev, int32_t* out_packed_dev,
                          void* stream);
int rag_index_select_rows_view(rag_index_t* index, const uint32_t* progs_dev, int64_t words,
                               int64_t* out_rows_dev, int64_t cap, int64_t* out_n_dev,
                               void* stream);
int rag_shardset_search_view(rag_shardset_t* set, const float* queries_dev, int B, int k,
                             const uint32_t* progs_dev, int64_t words, int n_programs,
                             const uint32_t* filters_dev, int flags, float* out_scores_dev,
                             int64_t* out_ids_dev, uint8_t* out_empty_dev, void* stream);

/* Recommend queries ("more like these points, less like those": Qdrant's RecommendQuery /
 * client.recommend). One request has P positive and N negative examples,
 * 0 <= P, N <= RAG_RECO_MAX_SIDE, each a vector of the index's dim (pos_dev [n_pos][dim],
 * neg_dev [n_neg][dim], fp32, device; the caller resolves point ids to stored rows with
 * rag_index_gather_rows). Every example goes through the canonical query normalisation into
 * x_i (fp32), exactly as a search query does; e_i(r) is the canonical exact score of stored row
 * r against x_i — the arithmetic of every exact score of this library, never another dot
 * product. A zero-vector example normalises to the zero query: e_i(r) = 0 for every row, and it
 * adds the zero vector to AVERAGE's mean.
 *   RAG_RECO_BEST (P + N >= 1): mp = max over the positives of e_i(r) in fp32 (-inf when P = 0),
 *     mn the same over the negatives (-inf when N = 0); sig(x) = 0.5 (x / (1 + |x|) + 1) in fp64
 *     on the fp32 value, rounded once to fp32; score = sig(mp) if mp > mn, else -sig(mn).
 *   RAG_RECO_SUM (P + N >= 1): score = sum over positives of e_i - sum over negatives of e_j,
 *     accumulated in fp64 in example order, positives first, rounded once to fp32.
 *   RAG_RECO_AVERAGE (P >= 1): v = a_pos when N = 0, else a_pos + (a_pos - a_neg), a_* the mean
 *     of the side's x_i; per component accumulated in fp64 in example order, divided, combined
 *     and rounded once to fp32. v is then the query of the ordinary exact search (every route
 *     of rag_index_search, scan copies included): the scores are rag_index_search's for v.
 * Result: the k best rows passing the filter by (score desc, row asc), -inf / -1 past the
 * matching rows — rag_index_search's order and padding; ids are id_offset + row. The example
 * points themselves are NOT excluded here: the host layer asks for k + m and drops them.
 * The BEST form is Qdrant's scaled-fast-sigmoid scoring restated from memory of its source:
 * parity with a Qdrant server's own arithmetic is unpinned (as for MMR and formulas). Results
 * are exact with respect to the contract above.
 *
 * rag_index_recommend: one request, asynchronous on `stream`, under the handle's lock.
 * progs_dev NULL (words = n_programs = 0): the filter is over the stored tags; else over the
 * blob's filter view (rag_index_search_view's rules). filter_dev: one (mask, value) pair [2] or
 * NULL. BEST and SUM with k <= RAG_MAX_K_LARGE take the hot pass — one MFMA stream of the fp16
 * rows whatever P + N: certified bounds [L, U] of every row's score, a sampled threshold,
 * candidates (at most 16384 kept) scored exactly; a request with more than 16384 rows within
 * its bounds of the k-th best after the last round is left unanswered (-inf / -1, counted in
 * rag_index_unanswered): re-run it with RAG_SEARCH_FULL. flags RAG_SEARCH_FULL, or
 * k > RAG_MAX_K_LARGE: the full pass (every row scored exactly, sorted), which always answers.
 * Both give the same lists bit for bit.
 * rag_index_reco_bounds: diagnostic; out_lo_dev[i] <= exact score of rows_dev[i] <= out_hi_dev[i]
 * as the hot pass computes them (BEST or SUM), (-inf, +inf) for a row outside [0, count).
 * rag_index_reco_vector: diagnostic; AVERAGE's v (fp32 [dim], device).
 * rag_index_reco_stats: out[0] hot passes and out[1] full passes since creation, out[2] the
 * candidates the last hot pass counted in its last round, out[3] the rounds it ran;
 * synchronises the device.
 * Argument errors are refused before any HIP call: a NULL pointer where one is needed, a side
 * above RAG_RECO_MAX_SIDE, P = 0 for AVERAGE, P + N = 0, an unknown strategy, k < 1, unknown
 * flags, the program rules of rag_index_search_view. */
#define RAG_RECO_AVERAGE 0
#define RAG_RECO_BEST 1
#define RAG_RECO_SUM 2
#define RAG_RECO_MAX_SIDE 16
int rag_index_recommend(rag_index_t* index, const float* pos_dev, int n_pos,
                        const float* neg_dev, int n_neg, int strategy, int k,
                        const uint32_t* progs_dev, int64_t words, int n_programs,
                        const uint32_t* filter_dev /* [2] or NULL */, int64_t id_offset,
                        int flags, float* out_scores_dev, int64_t* out_ids_dev, void* stream);
int rag_index_reco_bounds(rag_index_t* index, const float* pos_dev, int n_pos,
                          const float* neg_dev, int n_neg, int strategy,
                          const int64_t* rows_dev, int64_t n,
                          float* out_lo_dev, float* out_hi_dev, void* stream);
int rag_index_reco_vector(rag_index_t* index, const float* pos_dev, int n_pos,
                          const float* neg_dev, int n_neg, float* out_v_dev, void* stream);
int rag_index_reco_stats(rag_index_t* index, int64_t out[4]);

/* Discovery queries (Qdrant's DiscoverQuery — "nearest to this target, but on the positive side
 * of these example pairs" —, ContextQuery — the pairs alone — and client.discover; DESIGN.md
 * R20). A request has n pairs (positive_i, negative_i) and optionally a target, each a vector of
 * the index's dim (target_dev [dim], pos_dev / neg_dev [n_pairs][dim], fp32, device; the caller
 * resolves point ids to stored rows with rag_index_gather_rows). Every example goes through the
 * canonical query normalisation, exactly as a search query does, so a zero or non-finite example
 * is the zero query; e_x(r) is the canonical exact score (fp32) of stored row r against example
 * x — the arithmetic of every exact score of this library, never another dot product.
 *   Discover (target given, 0 <= n <= RAG_DISCOVER_MAX_PAIRS):
 *     rank(r) = sum_i sgn(e_pi(r) - e_ni(r)), compared on the fp32 values: each term +1, 0 or -1;
 *     score = fp32(rank + sig(e_t(r))), sig(x) = 0.5 (x / (1 + |x|) + 1) in fp64 on the fp32
 *     value (recommend's sig before its rounding), the add in fp64: one rounding in all.
 *     n = 0 is allowed: the order is then the nearest search's for the target, except that rows
 *     whose scores sig's rounding merges order by row.
 *   Context (target NULL, 1 <= n <= RAG_CONTEXT_MAX_PAIRS):
 *     d_i = (double)e_pi - (double)e_ni - 2^-23, m_i = min(d_i, 0), l_i = m_i / (1 + |m_i|);
 *     score = fp32(sum_i l_i), accumulated in fp64 in pair order, one rounding. Scores are <= 0;
 *     a score is 0 exactly when every pair has e_p - e_n >= 2^-23.
 *   Both map -0 to +0.
 * Result: the k best rows passing the filter by (score desc, row asc), -inf / -1 past the
 * matching rows — rag_index_search's order and padding; ids are id_offset + row. Example points
 * are NOT excluded here: the host layer asks for k + m and drops them.
 * Both forms are Qdrant's scoring restated from memory of its source:
 * parity with a Qdrant server's own arithmetic is unpinned (as for recommend, MMR and formulas).
 * Results are exact with respect to the contract above.
 *
 * rag_index_discover: one request, asynchronous on `stream`, under the handle's lock; target_dev
 * NULL makes it a context search. Filters as for rag_index_recommend: progs_dev NULL (words =
 * n_programs = 0) for the stored tags, else the blob's filter view; filter_dev one (mask, value)
 * pair [2] or NULL. k <= RAG_MAX_K_LARGE takes the hot pass — one MFMA stream of the fp16 rows
 * whatever n: pair i's positive in query slot i and its negative in slot 16 + i (the target in
 * slot 15: hence the limits), certified bounds [L, U] of every row's score, a sampled threshold,
 * candidates (at most 16384 kept) scored exactly. A request with more than 16384 rows within its
 * bounds of the k-th best — a context search with few pairs, whose best score 0 a large part of
 * the corpus shares; a discover request with a zero target — is left unanswered (-inf / -1,
 * counted in rag_index_unanswered), after one round where the tie is exact: re-run it with
 * RAG_SEARCH_FULL. flags RAG_SEARCH_FULL, or k > RAG_MAX_K_LARGE: the full pass (every row scored
 * exactly, sorted), which always answers. Both give the same lists bit for bit.
 * rag_index_discover_bounds: diagnostic; out_lo_dev[i] <= exact score of rows_dev[i] <=
 * out_hi_dev[i] as the hot pass computes them, (-inf, +inf) for a row outside [0, count).
 * rag_index_discover_stats: out[0] hot passes and out[1] full passes since creation, out[2] the
 * candidates the last hot pass counted in its last round, out[3] the rounds it ran; synchronises
 * the device. Counters of their own: rag_index_reco_stats does not move.
 * Argument errors are refused before any HIP call: a NULL side with n_pairs > 0, n_pairs above
 * the limit for the kind, a context search with n_pairs = 0, k < 1, unknown flags, the program
 * rules of rag_index_search_view. */
#define RAG_DISCOVER_MAX_PAIRS 15
#define RAG_CONTEXT_MAX_PAIRS 16
int rag_index_discover(rag_index_t* index, const float* target_dev /* [dim] or NULL: context */,
                       const float* pos_dev, const float* neg_dev, int n_pairs, int k,
                       const uint32_t* progs_dev, int64_t words, int n_programs,
                       const uint32_t* filter_dev /* [2] or NULL */, int64_t id_offset, int flags,
                       float* out_scores_dev, int64_t* out_ids_dev, void* stream);
int rag_index_discover_bounds(rag_index_t* index, const float* target_dev, const float* pos_dev,
                              const float* neg_dev, int n_pairs, const int64_t* rows_dev,
                              int64_t n, float* out_lo_dev, float* out_hi_dev, void* stream);
int rag_index_discover_stats(rag_index_t* index, int64_t out[4]);

/* Key columns (range and datetime filters: the numeric payload fields of a collection, in HBM).
 * An index holds 0 to RAG_KEYS_MAX_COLS columns, each int64 [capacity] (8 B per row, the tag
 * array's extent: a multiple of 16 rows). A column holds KEYS: for a double x, -0.0 taken as
 * +0.0, with b its IEEE-754 bits as int64, key(x) = b if b >= 0, else b ^ 0x7FFFFFFFFFFFFFFF,
 * so that a signed compare of keys is the numeric compare of the doubles (ragmi.filters.key_of).
 * RAG_KEY_ABSENT = INT64_MIN is "no value"; no double maps to it (key(-inf) =
 * 0x800FFFFFFFFFFFFF). The RANGE atom of a filter program compares them ("Filter programs").
 *
 * rag_index_keys_create: make the index hold n_cols columns (1..RAG_KEYS_MAX_COLS; RAG_ERANGE
 * outside). The number only ever grows: fewer than the index has is a no-op. New columns are
 * filled with RAG_KEY_ABSENT, existing ones keep their content. Synchronises the device.
 * rag_index_keys_cols: the number of columns (-1 for NULL).
 * rag_index_write_keys: keys[col][rows_dev[i]] = keys_dev[i], i < n (int64, device). A row
 * outside [0, capacity) is skipped and never dereferenced; the rows must be distinct.
 * rag_index_gather_keys: out_keys_dev[i] = keys[col][rows_dev[i]], RAG_KEY_ABSENT for a row
 * outside [0, capacity) (never dereferenced) — rag_index_gather_tags for a key column.
 * Both are asynchronous on `stream`; col outside [0, columns) is RAG_ERANGE.
 *
 * The keys are a stored form of the row: rag_index_move_rows moves every column's key with the
 * row (a kernel of its own on the same stream under the same hold of the lock, launched only
 * when the index has columns), rag_index_reserve regrows the columns (old rows keep their keys,
 * new rows hold RAG_KEY_ABSENT), rag_index_destroy frees them. rag_index_upsert, the imports,
 * rag_index_gather_rows and rag_index_scatter_rows do NOT touch them: the host layer writes
 * every column of every row it upserts, and carries the keys of rows it moves between indexes
 * (gather_keys / write_keys). Row invariant: the keys of rows >= count are unspecified (a
 * delete leaves stale values in the tail); nothing exposes them, the filter view being 0 for
 * those rows. No reference counterpart: the reference leaves range conditions to the Qdrant
 * server and sends none itself. */
#define RAG_KEYS_MAX_COLS 4
#define RAG_KEY_ABSENT INT64_MIN
int rag_index_keys_create(rag_index_t* index, int n_cols);
int rag_index_keys_cols(const rag_index_t* index);
int rag_index_write_keys(rag_index_t* index, int col, const int64_t* rows_dev,
                         const int64_t* keys_dev, int64_t n, void* stream);
int rag_index_gather_keys(rag_index_t* index, int col, const int64_t* rows_dev, int64_t n,
                          int64_t* out_keys_dev, void* stream);

/* Sparse vectors (a named sparse vector beside the dense one: Qdrant's sparse_vectors_config,
 * SparseVector queries and hybrid prefetches). An index holds 0 or 1 sparse
 * column of S slots per row, S a multiple of 16 in [16, RAG_SPARSE_MAX_SLOTS], fixed when the
 * column is created: terms uint16 [capacity][S] and values fp32 [capacity][S]. A stored row
 * holds its nonzero entries in ascending term order, no term twice, every value finite, terms in
 * [0, 65535); the remaining slots hold RAG_SPARSE_TERM_NONE with value 0. The callers keep these
 * rules (ragmi.collection refuses what breaks them); the kernels read a row up to its first empty
 * slot. Deviations from Qdrant, all refused by the host layer and never truncated: indices are
 * below 65535 (Qdrant: uint32), a point holds at most S nonzeros, a query at most
 * RAG_SPARSE_MAX_QUERY_NNZ, a collection one sparse name, and shard sets hold none.
 *
 * Score. score(q, r) = the sum, over the slots of r in stored order whose term occurs in q, of
 * (double)val_r * (double)w_q, accumulated in fp64 in that order and rounded once to fp32, -0.0
 * taken as +0.0. Both factors are fp32, so every product is exact in fp64 and a fused
 * multiply-add gives the bits of a multiply and an add: a numpy loop reproduces the score bit
 * for bit. A row is eligible when it is < count, passes the filter and shares at least one term
 * with the query; a row without a shared term is no hit even when k exceeds the matches
 * (Qdrant's sparse semantics), so a point without a sparse vector is never one. Result: the k
 * best eligible rows by (score desc, row asc), -inf / -1 past them — rag_index_search's order
 * and padding; ids are id_offset + row.
 *
 * rag_index_sparse_create: make the index hold the column; a second call with the same `slots`
 * is a no-op, another slot count RAG_EINVAL. New rows are empty. Synchronises the device.
 * rag_index_sparse_slots: S, or 0 without a column (and for NULL).
 * rag_index_sparse_write: row rows_dev[i] = (terms_dev, vals_dev)[i] (uint16 / fp32 [n][S], the
 * slot layout above; distinct rows). A row outside [0, capacity) is skipped, never dereferenced.
 * rag_index_sparse_gather: the stored rows back, an empty row for a row outside [0, capacity).
 * rag_index_sparse_df: out_df_dev[t] (int64 [65535], device; zeroed by the call) = the rows
 * < count that hold term t. One streaming pass over the terms, integer atomics only: the same
 * bits on every run.
 * rag_index_sparse_search: B queries, padded: q_terms_dev uint16 [B][64] ascending, q_vals_dev
 * fp32 [B][64], q_nnz_dev int32 [B] (read clamped to [0, 64]; a term >= 65535 matches nothing).
 * Filters follow rag_index_search / rag_index_search_view: progs_dev NULL (words = n_programs =
 * 0): filters_dev [B][2] (or NULL) over the stored tags; else over the blob's filter view.
 * k <= RAG_MAX_K_LARGE takes the hot pass — up to 32 queries share one stream of the sparse
 * rows: their distinct terms form a bitmap and a weight table in LDS, a sample of 16-row tiles
 * gives each query a threshold that every top-k row reaches (the k-th largest tile maximum),
 * the rows at or above it are collected with their scores (at most 16384 kept) and the k best
 * emitted. A query with more than 16384 rows at or above its last threshold is left unanswered
 * (-inf / -1, counted in rag_index_unanswered), and so is every query of a pass (32 consecutive
 * queries) whose distinct terms exceed RAG_SPARSE_MAX_UNION: the host layer groups queries so
 * that none does, and re-runs an unanswered query with RAG_SEARCH_FULL. flags RAG_SEARCH_FULL,
 * or k > RAG_MAX_K_LARGE: the full pass, one query at a time (every row scored, the stable sort
 * and emit of rag_index_search_full), which always answers. Both give the same lists bit for bit.
 * write, gather, df and search are asynchronous on `stream`, under the handle's lock; every
 * argument error (a NULL pointer, no column, k < 1, unknown flags, the program rules of
 * rag_index_search_view) is refused on the host before any HIP call.
 *
 * The sparse row is a stored form of the row, as a key is: rag_index_move_rows moves it with the
 * dense row (a kernel of its own on the same stream under the same hold of the lock, launched
 * only when the column exists), rag_index_reserve regrows the column (old rows kept, new rows
 * empty), rag_index_destroy frees it. rag_index_upsert, the imports, rag_index_gather_rows and
 * rag_index_scatter_rows do NOT touch it: the host layer writes the sparse row of every point it
 * upserts, an empty one when the point has none. Rows at or past the count are unspecified and
 * never eligible. No reference counterpart: the reference retrieves by one dense vector. */
#define RAG_SPARSE_TERM_NONE 0xFFFFu
#define RAG_SPARSE_MAX_SLOTS 512
#define RAG_SPARSE_MAX_QUERY_NNZ 64
#define RAG_SPARSE_MAX_UNION 512
int rag_index_sparse_create(rag_index_t* index, int slots);
int rag_index_sparse_slots(const rag_index_t* index);
int rag_index_sparse_write(rag_index_t* index, const int64_t* rows_dev, const uint16_t* terms_dev,
                           const float* vals_dev, int64_t n, void* stream);
int rag_index_sparse_gather(rag_index_t* index, const int64_t* rows_dev, int64_t n,
                            uint16_t* out_terms_dev, float* out_vals_dev, void* stream);
int rag_index_sparse_df(rag_index_t* index, int64_t* out_df_dev, void* stream);
int rag_index_sparse_search(rag_index_t* index, const uint16_t* q_terms_dev,
                            const float* q_vals_dev, const int32_t* q_nnz_dev, int B, int k,
                            const uint32_t* progs_dev, int64_t words, int n_programs,
                            const uint32_t* filter_dev, int64_t id_offset, int flags,
                            float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* Payload queries (QdrantClient.scroll, order_by, facet): ranking and counting over the tag and
 * key columns, with no vector in play. All three take a filter the way
 * rag_index_select_rows_view does: progs_dev == NULL means every row < count; otherwise ONE
 * program (the blob's first record, the blob checked as every *_view call checks it) is
 * evaluated into the view column the handle keeps for `stream`, and bit 0 of it is read. Rows at
 * or past the count are never eligible, whatever their (unspecified) keys and tags hold, and no
 * row outside [0, capacity) is dereferenced. Every argument is checked on the host before any
 * HIP call; all three are asynchronous on `stream`.
 *
 * rag_index_order_rows: the `limit` best eligible rows of key column `col`. A row is eligible
 * when it is < count, passes the program, its key is not RAG_KEY_ABSENT and lo <= key <= hi
 * (signed 64-bit, both inclusive). The order is (key ascending, row ascending), or with
 * RAG_ORDER_DESC in `flags` (key descending, row ascending). out_keys_dev / out_rows_dev (int64
 * [limit], device) receive the list; out_n_dev (int64 [2], device): [0] the entries written,
 * min(limit, eligible), [1] the eligible rows. Entries past the written ones hold row -1 and key
 * RAG_KEY_ABSENT; nothing past entry limit - 1 is written. 1 <= limit <= RAG_ORDER_MAX and
 * 0 <= col < columns, else RAG_ERANGE; a NULL output is RAG_EINVAL. The result is a pure
 * function of the columns: the same bits on every run (a radix select of the limit-th key whose
 * atomics add integer counts only, an ordered emit, a sort of the list in LDS). Each of its 10
 * streaming passes reads 8 B per row of keys, and 4 B per row of view under a program.
 *
 * rag_index_facet_counts: out_counts_dev (int64 [n_codes + 1], device; zeroed by the call)
 * [c] = the eligible rows whose code of tag field `field`, (tag >> 16 field) & 0xFFFF, equals c,
 * 0 <= c <= n_codes. A stored code above n_codes is not counted and indexes nothing. field is 0
 * or 1 and 0 <= n_codes <= 65535, else RAG_ERANGE. Exact for every n_codes (bins in LDS up to
 * 8192 of them, in global memory above). One streaming pass: 4 B per row of tags, and 4 B per
 * row of view under a program.
 *
 * rag_index_select_rows_from: rag_index_select_rows_view restricted to rows >= row0 (with
 * progs_dev == NULL: every such row), *out_n_dev counting the matches at or after row0.
 * row0 < 0 is RAG_EINVAL; row0 >= count selects nothing. Reads only the chunks from row0's on.
 * No reference counterpart: the reference never scrolls, orders or facets. */
#define RAG_ORDER_MAX 4096
#define RAG_ORDER_DESC 1
int rag_index_order_rows(rag_index_t* index, const uint32_t* progs_dev, int64_t words, int col,
                         int flags, int64_t lo, int64_t hi, int limit, int64_t* out_keys_dev,
                         int64_t* out_rows_dev, int64_t* out_n_dev, void* stream);
int rag_index_facet_counts(rag_index_t* index, const uint32_t* progs_dev, int64_t words, int field,
                           int n_codes, int64_t* out_counts_dev, void* stream);
int rag_index_select_rows_from(rag_index_t* index, const uint32_t* progs_dev, int64_t words,
                               int64_t row0, int64_t* out_rows_dev, int64_t cap,
                               int64_t* out_n_dev, void* stream);

/* Exactness bookkeeping (tests, bench): tier1 / tier2 = number of queries, since the index
 * was created, whose top-k was certified by the list re-scoring fallback / needed the second
 * pass over the shard (all other queries passed the error-bound check directly).
 * last_tiers (host, may be NULL when n_last == 0) receives, for the first n_last queries of
 * the most recent search PASS, 0 / 1 / 2 = the path that certified them (3 = marked for the
 * second pass but left unanswered, see rag_index_unanswered; -1 past the pass's
 * query count). Scope: a pass is one scan of <= 32 queries (<= 128 on the D = 1024 wide
 * scan); a search of more queries runs several passes and only its last one is reported, and
 * the state is per handle, so searches issued concurrently on several streams overwrite each
 * other's record (the tier1 / tier2 totals are exact in every case). Synchronises the device. */
int rag_index_exactness_stats(rag_index_t* index, int64_t* tier1, int64_t* tier2,
                              int32_t* last_tiers, int n_last);

/* Number of queries, since the index was created, that received NO result (-1 ids; their
 * last_tiers entry reads 3): k <= RAG_MAX_K passes whose second pass was skipped
 * (RAGMI_RESCAN_WG=0, honoured only under RAG_CREATE_DIAGNOSTIC), and large-k passes
 * (RAG_MAX_K < k <= RAG_MAX_K_LARGE) where more than 16384 rows tie within the MFMA error band
 * of a query's k-th best after the last collection round — possible in production (thousands
 * of identical chunks). Re-answer such queries with rag_index_search_full (the QdrantClient
 * front end does). Synchronises the device. */
int rag_index_unanswered(rag_index_t* index, int64_t* n);

/* Scan order across streams. serial = 1: each search pass's scan launch waits for the
 * previous pass's scan, whichever stream that ran on (one HIP event per handle), so passes
 * issued on several streams overlap their query prep, seed sampling and select with another
 * pass's scan while the HBM-bound scans themselves run one at a time (measured effective with
 * 2 streams; with 4 the traced scans still overlap). serial = 2: every pass hands
 * its scan to the handle's own scan stream and waits for it before select (two event hops
 * per pass; strictly one scan at a time). serial = 0 (default): passes on different streams
 * are unordered. No reference counterpart: the reference issues one HTTP search per query
 * (main.py:232-237); this is serving-loop plumbing for main2.py:281-295's batch processor
 * with several batches in flight. */
int rag_index_set_scan_order(rag_index_t* index, int serial);

/* int8 prescan (dim 384, RAG_STORE_FP16 only). Such an index keeps, beside its fp16 rows, an
 * int8 copy of them with a scale and a measured quantisation error per row: memory is
 * 3 B + 8 B / dim per element instead of 2 B (+50 %: 3.9 GB more at 10M x 384), rebuilt on the
 * device by every call that writes rows (upsert, import, move, scatter, reserve). A pass with
 * k <= RAG_MAX_K may stream that copy (half the bytes) ranking rows by an UPPER BOUND of their
 * exact score; select then rescores the listed rows on the fp16 rows and certifies the exact
 * top-k as it does after the fp16 scan: returned ids and scores are the same in every mode,
 * bit for bit. The wider error band makes the list re-scoring fallback (tier 1 of
 * rag_index_exactness_stats) common, which is why the default is by size:
 *   RAG_PRESCAN_OFF      always the fp16 scan
 *   RAG_PRESCAN_AUTO     (default) the int8 prescan for passes (filtered ones included) over
 *                        at least RAG_PRESCAN_MIN_ROWS rows, else the fp16 scan; the 6-bit
 *                        prescan (below) from RAG_PRESCAN6_MIN_ROWS rows
 *   RAG_PRESCAN_ALWAYS   the int8 prescan for every k <= RAG_MAX_K pass
 *   RAG_PRESCAN_ALWAYS6  the 6-bit prescan for every k <= RAG_MAX_K pass
 * Indexes without the copy (dim 1024, fp32 storage) accept any mode and stay on the fp16 scan.
 * No reference counterpart (Qdrant's scalar quantisation with rescoring is approximate; this
 * one is certified exact).
 *
 * 6-bit prescan. The largest shards keep a third image: one integer in [-31, 31] per element
 * (six bits, 288 B per row) with its own scale and measured error per row, +296 B per row
 * (+38 % of the fp16 rows: 2.96 GB more at 10M x 384). A pass over it reads 0.755x the int8
 * pass's bytes and ranks by the same kind of upper bound; the certificate band is about four
 * times wider, so every query of such a pass takes tier 1 (about 200 rescored rows at 10M
 * rows). The copy exists only where it is used: in an index whose capacity is at least
 * RAG_PRESCAN6_MIN_ROWS (at creation or after rag_index_reserve), or once
 * RAG_PRESCAN_ALWAYS6 is set, which builds it from the stored rows. It is rebuilt with the
 * int8 copy by every call that writes rows, and on import. */
enum {
  RAG_PRESCAN_OFF = 0,
  RAG_PRESCAN_AUTO = 1,
  RAG_PRESCAN_ALWAYS = 2,
  RAG_PRESCAN_ALWAYS6 = 3
};
#define RAG_PRESCAN_MIN_ROWS 500000
#define RAG_PRESCAN6_MIN_ROWS 4000000
/* The routing rule itself (the library calls this; no device involved): 1 when a pass of `k`
 * over `count` rows of a (dim, storage) index in `mode` streams a prescan copy (either). */
#define RAG_PRESCAN_ROUTES(mode, dim, storage, k, count)                                   \
  ((dim) == 384 && (storage) == RAG_STORE_FP16 && (k) >= 1 && (k) <= RAG_MAX_K &&          \
   ((mode) == RAG_PRESCAN_ALWAYS || (mode) == RAG_PRESCAN_ALWAYS6 ||                       \
    ((mode) == RAG_PRESCAN_AUTO && (count) >= RAG_PRESCAN_MIN_ROWS)))
/* 1 when that pass streams the 6-bit copy, given that the index keeps one (else the int8 copy
 * serves it): RAG_PRESCAN_ALWAYS6, or auto from RAG_PRESCAN6_MIN_ROWS rows.
 * RAG_PRESCAN_ALWAYS stays the int8 prescan. */
#define RAG_PRESCAN6_ROUTES(mode, dim, storage, k, count)                                  \
  ((dim) == 384 && (storage) == RAG_STORE_FP16 && (k) >= 1 && (k) <= RAG_MAX_K &&          \
   ((mode) == RAG_PRESCAN_ALWAYS6 ||                                                       \
    ((mode) == RAG_PRESCAN_AUTO && (count) >= RAG_PRESCAN6_MIN_ROWS)))
int rag_index_set_prescan(rag_index_t* index, int mode);
/* The mode set (-1 for NULL). */
int rag_index_prescan(const rag_index_t* index);
/* *n = the search passes since creation that streamed a prescan copy (scan_kernel_i8 or
 * scan_kernel_i6): what tells a pass of the prescan from one of the fp16 scan, whose results
 * are the same. A search of B queries with k <= RAG_MAX_K that routes to the prescan adds
 * ceil(B / RAG_QUERY_TILE); every other pass adds nothing. Host state only, no device work. */
int rag_index_prescan_passes(rag_index_t* index, int64_t* n);
/* *n = those of them that streamed the 6-bit copy (scan_kernel_i6). */
int rag_index_prescan6_passes(rag_index_t* index, int64_t* n);
/* Diagnostic view of the certificate's premise: out_u_dev[b * n + i] = the prescan's upper
 * bound u of stored row rows_dev[i] against query b (q_dev: B <= 32 queries, as for a search),
 * computed from the stored copy by the device function the prescan itself uses (of the copy
 * a k = 1 pass of the index streams in its current mode; the int8 one where none); -inf for a
 * row outside [0, count). u >= the exact score of every pair is what the certificate rests
 * on. RAG_EINVAL for an index without the copy. Synchronous. */
int rag_index_prescan_bounds(rag_index_t* index, const float* q_dev, int B,
                             const int64_t* rows_dev, int64_t n, float* out_u_dev);
/* Spatial partition of the batches in flight (serving option): a HIP stream restricted to CU
 * share `part` of `parts` (contiguous CU ids, hipExtStreamCreateWithCUMask). Searches issued
 * on such a stream size their scan grids to the stream's CUs (one scan workgroup per CU), so
 * `parts` batches in flight on `parts` partition streams scan side by side on disjoint CUs.
 * Results are identical on any stream. Destroy with rag_stream_destroy. (The reference has no
 * counterpart: Qdrant serves concurrent searches from one server process, main2.py:281-295.) */
int rag_stream_create_cu_partition(int device, int part, int parts, void** stream);
/* The same with an explicit CU mask (`words` 32-bit words, bit i = CU id i as
 * hipExtStreamCreateWithCUMask numbers them). On MI355X bit i is a CU of XCD i % 8, and an
 * XCD whose bits are all clear runs on ALL its CUs, so the mask must enable at least one CU
 * of every XCD (else RAG_EINVAL); likewise rag_stream_create_cu_partition takes at most
 * n_cu / 8 parts. Round 6. */
int rag_stream_create_cu_mask(int device, const uint32_t* mask, int words, void** stream);
int rag_stream_destroy(void* stream);
/* Diagnostic build only (else RAG_EINVAL): n_wg one-wave workgroups on `stream`, each writing
 * its (XCC_ID, HW_ID) hardware registers to out_dev[2 * wg .. +1] — where a CU mask's
 * workgroups actually run. */
int rag_diag_cu_probe(void* stream, int n_wg, int32_t* out_dev);

/* Kernel timing hook for bench.py: average device time (ms) of `rag_index_search` scan-kernel
 * launches measured with HIP events on the launch stream. enable = 0 off; enable = n > 0 records
 * an event pair around every n-th scan launch (each record costs a few us of device idle
 * time, so bench.py samples instead of timing every pass). */
int rag_profile_enable(rag_index_t* index, int enable);
int rag_profile_scan_ms(rag_index_t* index, double* total_ms, int64_t* launches);
/* The same event pairs as intervals: start_ms[i] / end_ms[i] of the i-th recorded launch,
 * relative to the first recorded launch's start (cap entries at most; *launches = how many
 * were recorded), then clears them like rag_profile_scan_ms. With several batches in flight
 * the launches of different streams overlap in time; bench.py takes the union of these
 * intervals as the time the scan kernel occupied the device. */
int rag_profile_scan_intervals(rag_index_t* index, double* start_ms, double* end_ms, int64_t cap,
                               int64_t* launches);

/* Diagnostic: average device ms of `reps` launches of scan variant `variant` on the current
 * corpus with the first min(B,32) queries (dim 384 only). Variants: 0 production (seeded
 * thresholds), 1 unseeded, 2 contiguous per-wave tile ranges, 3 MFMA without top-k,
 * 4 loads only, 5 without non-temporal loads, 6 without the load sched-barrier, 7 production
 * with every seed at +inf (top-k compares only), 8 the VALU ablation: v_dot2_f32_f16 instead
 * of MFMA over a row-group-major copy of the corpus, same top-k; 9 / 10 / 11 the dynamic tile
 * queue with chunks of 2 / 1 / 4 tiles, 12 dynamic (2) loads only, 13 / 14 static production
 * / loads only (9-14 time every launch on its own event pair), 15 production without the
 * end-of-scan sort of pending-only queries (timing probe), 16 production with the round-1
 * end-of-scan sort (A/B). dim 1024: variants 0-4 of
 * the wide (33-128 query) scan. The production library accepts variants 0 and 7 only (dim
 * 1024: 0); the others are compiled into the diagnostic build (rag_diagnostic_build). */
int rag_bench_scan(rag_index_t* index, const float* queries_dev, int B, int variant, int reps,
                   double* avg_ms);

#ifdef __cplusplus
}
#endif

#endif /* RAGMI_H */
