"""numpy restatement of the MMR re-selection (rag_index_mmr; include/ragmi.h), built
on the CPU oracle: oracle_scan.search gives the exact candidates, oracle_scan.rescore the
canonical row-to-row similarity, the greedy choice is float64 `val` and np.argmax (the first
maximum: ties to the smallest position). TEST HELPER ONLY, shared by test_mmr_cpu.py and
test_mmr_gpu.py; also the seed-7 corpus of near-duplicate groups both use.
"""
import numpy as np

import oracle_scan as O

N_GROUPS, GROUP_ROWS, N_IDENTICAL, N_ROWS = 12, 9, 4, 3001


def grouped_corpus(D: int):
    """The seed-7 corpus: 12 groups of 9 rows (4 identical to the group's centre, 5 at 0.02
    noise) plus 2893 random rows, permuted; 3001 rows, not a multiple of the 16-row tile.
    Returns (x fp32 [3001, D], query fp32 [D], group [3001]: the row's group or -1)."""
    rng = np.random.default_rng(7)
    centres = rng.standard_normal((N_GROUPS, D)).astype(np.float32)
    rows, label = [], []
    for g in range(N_GROUPS):
        for r in range(GROUP_ROWS):
            if r < N_IDENTICAL:
                rows.append(centres[g].copy())
            else:
                rows.append((centres[g] + 0.02 * rng.standard_normal(D)).astype(np.float32))
            label.append(g)
    n_rand = N_ROWS - N_GROUPS * GROUP_ROWS
    rand = rng.standard_normal((n_rand, D)).astype(np.float32)
    x = np.concatenate([np.stack(rows), rand])
    label = np.asarray(label + [-1] * n_rand)
    perm = rng.permutation(N_ROWS)
    query = (centres.sum(axis=0) + 0.3 * rng.standard_normal(D)).astype(np.float32)
    return np.ascontiguousarray(x[perm]), query, label[perm]


def encode(x, storage: str):
    """The stored form of input rows x: fp16 bits (uint16) or the normalised fp32 rows."""
    return O.encode_rows(x) if storage == "fp16" else O.encode_rows32(x)


def stored_f32(corpus, row: int):
    """Stored row `row` as the fp32 vector the similarity reads: the halves widened, or the
    fp32 row."""
    c = corpus[row]
    return np.ascontiguousarray(c.view(np.float16).astype(np.float32) if c.dtype == np.uint16
                                else c)


def mmr(corpus, cand_s, cand_r, k: int, diversity, ncand=None, stats=None):
    """MMR over candidate lists cand_s fp32 [B, C] / cand_r int64 [B, C] (-1 = none), as pinned:
    n_b = min(ncand[b], leading valid entries); step 0 picks position 0; after picking s,
    maxsim[j] = max(maxsim[j], sim(s, j)) in fp32 over the unselected j; step t >= 1 picks the
    first maximum of val[j] = float64(fp32(1 - div)) * rel[j] - float64(div) * maxsim[j]. Returns
    (scores [B, k], rows [B, k], positions [B, k]), -inf / -1 / -1 past the last pick.
    stats["ties"] counts the steps whose maximum was shared by several candidates."""
    cand_s = np.asarray(cand_s, np.float32)
    cand_r = np.asarray(cand_r, np.int64)
    B, C = cand_r.shape
    div_a = np.broadcast_to(np.asarray(diversity, np.float32), (B,))
    nc_a = np.full(B, C) if ncand is None else np.broadcast_to(np.asarray(ncand), (B,))
    out_s = np.full((B, k), -np.inf, np.float32)
    out_r = np.full((B, k), -1, np.int64)
    out_p = np.full((B, k), -1, np.int32)
    for b in range(B):
        bad = np.nonzero((cand_r[b] < 0) | (cand_r[b] >= corpus.shape[0]))[0]
        n = int(min(max(int(nc_a[b]), 0), C, bad[0] if bad.size else C))
        if n == 0:
            continue
        rows = np.ascontiguousarray(cand_r[b, :n])
        rel = cand_s[b, :n]
        div = np.float32(div_a[b])
        lam = np.float32(np.float32(1.0) - div)
        maxsim = np.full(n, -np.inf, np.float32)
        free = np.ones(n, bool)
        s = 0
        for t in range(min(k, n)):
            out_s[b, t], out_r[b, t], out_p[b, t] = rel[s], rows[s], s
            free[s] = False
            if t + 1 == min(k, n):
                break
            sim = O.rescore(corpus, stored_f32(corpus, rows[s])[None], rows[None])[0]
            maxsim[free] = np.maximum(maxsim[free], sim[free])
            val = np.full(n, -np.inf, np.float64)
            val[free] = np.float64(lam) * rel[free].astype(np.float64) \
                - np.float64(div) * maxsim[free].astype(np.float64)
            s = int(np.argmax(val))
            if stats is not None and int((val == val[s]).sum()) > 1:
                stats["ties"] = stats.get("ties", 0) + 1
    return out_s, out_r, out_p


def search_mmr(corpus, queries, k: int, diversity, candidates, tags=None, filters=None,
               stats=None):
    """oracle_scan.search at C = max(candidates) per query (its own filter (mask, value) from
    `filters` [B, 2] when given), then mmr with ncand = candidates. Returns mmr's triple and the
    candidate lists (cand_s, cand_r)."""
    queries = np.ascontiguousarray(queries, np.float32)
    B = queries.shape[0]
    nc = np.broadcast_to(np.asarray(candidates, np.int64), (B,))
    C = int(nc.max())
    cs = np.empty((B, C), np.float32)
    cr = np.empty((B, C), np.int64)
    for b in range(B):
        if filters is None:
            cs[b], cr[b] = [a[0] for a in O.search(corpus, queries[b:b + 1], C)]
        else:
            cs[b], cr[b] = [a[0] for a in O.search(
                corpus, queries[b:b + 1], C, tags=tags, mask=int(filters[b][0]),
                value=int(filters[b][1]), use_filter=True)]
    return mmr(corpus, cs, cr, k, diversity, nc, stats) + (cs, cr)
