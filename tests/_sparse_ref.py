"""numpy restatement of sparse vectors (rag_index_sparse_*; include/ragmi.h "Sparse vectors",
DESIGN.md R19): the slot layout, the score, eligibility, the result order and padding, document
frequency, the IDF weights, bm25_document, and the corpora the GPU tests search. Nothing here
imports ragmi: it is the independent statement the product is compared against, bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

NONE = 0xFFFF            # RAG_SPARSE_TERM_NONE
TERMS = 65535            # terms lie in [0, TERMS)
QUERY_NNZ = 64           # RAG_SPARSE_MAX_QUERY_NNZ


# ---------------------------------------------------------------- layout
def pack(vectors, S: int):
    """[(indices, values), ...] -> (terms uint16 [n, S], vals fp32 [n, S], nnz int32 [n]) in the
    stored layout: explicit zeros dropped, ascending terms, NONE / 0 padding."""
    n = len(vectors)
    terms = np.full((n, S), NONE, np.uint16)
    vals = np.zeros((n, S), np.float32)
    nnz = np.zeros(n, np.int32)
    for i, (idx, val) in enumerate(vectors):
        idx = np.asarray(idx, np.int64).reshape(-1)
        val = np.asarray(val, np.float32).reshape(-1)
        keep = val != 0
        idx, val = idx[keep], val[keep]
        order = np.argsort(idx, kind="stable")
        assert len(idx) <= S and len(set(idx.tolist())) == len(idx)
        terms[i, :len(idx)] = idx[order]
        vals[i, :len(idx)] = val[order]
        nnz[i] = len(idx)
    return terms, vals, nnz


# ---------------------------------------------------------------- score
def scores(terms, vals, q_idx, q_val):
    """(score fp32 [n], overlap bool [n]) of every stored row against one query: the fp64 sum,
    in slot order, of (double)val * (double)w over the slots whose term the query holds, rounded
    once to fp32, -0.0 taken as +0.0."""
    w = np.zeros(TERMS + 1, np.float64)
    has = np.zeros(TERMS + 1, bool)
    w[np.asarray(q_idx, np.int64)] = np.asarray(q_val, np.float32).astype(np.float64)
    has[np.asarray(q_idx, np.int64)] = True
    has[NONE] = False
    t = terms.astype(np.int64)
    hit = has[t]                                            # [n, S]
    prod = np.where(hit, vals.astype(np.float64) * w[t], 0.0)
    # a left-to-right fp64 accumulation in slot order (adding 0.0 for a miss changes nothing:
    # the running sum is never -0.0, it starts at +0.0)
    acc = np.add.accumulate(prod, axis=1)[:, -1] if terms.shape[1] else np.zeros(len(terms))
    s = acc.astype(np.float32)
    s[s == 0] = np.float32(0.0)
    return s, hit.any(axis=1)


def score_loop(row_terms, row_vals, q_idx, q_val) -> np.float32:
    """The same score of one row as a plain Python loop (the contract read literally)."""
    w = {int(t): float(np.float32(v)) for t, v in zip(q_idx, q_val)}
    acc = 0.0
    for t, v in zip(row_terms.tolist(), row_vals.tolist()):
        if t != NONE and t in w:
            acc = acc + float(np.float32(v)) * w[t]        # the product is exact in fp64
    s = np.float32(acc)
    return np.float32(0.0) if s == 0 else s


def topk(terms, vals, count: int, q_idx, q_val, k: int, passing=None, id_offset: int = 0):
    """(scores fp32 [k], ids int64 [k]): the k best eligible rows by (score desc, row asc), -inf /
    -1 past them. Eligible: below the count, passing (bool [count] or None) and sharing a term."""
    s, ov = scores(terms[:count], vals[:count], q_idx, q_val)
    ok = ov if passing is None else ov & np.asarray(passing, bool)[:count]
    rows = np.nonzero(ok)[0]
    order = np.lexsort((rows, -s[rows].astype(np.float64)))[:k]
    out_s = np.full(k, -np.inf, np.float32)
    out_i = np.full(k, -1, np.int64)
    out_s[:len(order)] = s[rows[order]]
    out_i[:len(order)] = rows[order] + id_offset
    return out_s, out_i


def search(terms, vals, count, queries, k, passing=None):
    """topk of every query [(indices, values), ...]; passing: per query bool [count] or None."""
    res = [topk(terms, vals, count, qi, qv, k, None if passing is None else passing[j])
           for j, (qi, qv) in enumerate(queries)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ---------------------------------------------------------------- df, IDF, BM25
def df(terms, count: int) -> np.ndarray:
    t = terms[:count].reshape(-1).astype(np.int64)
    return np.bincount(t[t != NONE], minlength=TERMS)[:TERMS].astype(np.int64)


def idf_weights(q_idx, q_val, df_all, n_docs: int) -> np.ndarray:
    """w' = float32(float64(w) * ln(1 + (N - df + 0.5) / (df + 0.5)))."""
    out = []
    for t, w in zip(q_idx, q_val):
        d = float(df_all[int(t)])
        out.append(np.float32(float(np.float32(w)) * math.log(1.0 + (n_docs - d + 0.5) / (d + 0.5))))
    return np.asarray(out, np.float32)


SPECIAL = (0, 100, 101, 102, 103)    # [PAD] [UNK] [CLS] [SEP] [MASK] of the BERT vocabulary


def bm25_document(token_ids, S: int = 128, k1: float = 1.2, b: float = 0.75,
                  avg_len: float = 256.0):
    """(indices, values): tf * (k1 + 1) / (tf + k1 * (1 - b + b * len / avg_len)) per distinct
    term in fp64, rounded to fp32; special tokens and [UNK] dropped (len counts the kept tokens);
    more than S terms: the S largest values, ties to the lower term."""
    ids = [int(t) for t in token_ids if int(t) not in SPECIAL]
    n = len(ids)
    tf: dict = {}
    for t in ids:
        tf[t] = tf.get(t, 0) + 1
    items = [(t, np.float32(c * (k1 + 1.0) / (c + k1 * (1.0 - b + b * n / avg_len))))
             for t, c in tf.items()]
    items.sort(key=lambda x: (-float(x[1]), x[0]))
    items = sorted(items[:S])
    return [t for t, _ in items], [v for _, v in items]


# ---------------------------------------------------------------- corpora
def zipf_rows(rng, n: int, S: int, mean_nnz: int, vocab: int = TERMS, negative: float = 0.1):
    """n sparse rows [(indices, values)] with terms from a Zipf-like distribution over
    [0, vocab): term = floor(vocab * u^3) makes low ids frequent; values in (0.1, 3), a share
    `negative` of them negated."""
    rows = []
    for _ in range(n):
        m = int(min(S, max(1, rng.poisson(mean_nnz))))
        t = np.unique((vocab * rng.random(2 * m) ** 3).astype(np.int64))
        t = rng.permutation(t)[:m]
        v = (0.1 + 2.9 * rng.random(len(t))).astype(np.float32)
        v[rng.random(len(t)) < negative] *= -1
        rows.append((np.sort(t), v[np.argsort(t, kind="stable")]))
    return rows


def corpus(n: int, S: int, seed: int = 0, mean_nnz: int | None = None):
    """The search corpus: n Zipf rows with every forced case written over fixed rows —
    row 0 empty, row 1 one nonzero, row 2 exactly S nonzeros, rows 3 / 4 holding terms 0 and
    65534, a block of 40 identical rows straddling row 16 k boundaries (exact ties across a
    tile boundary) from row 1000 on (from n // 3 on in a small corpus). Returns (rows, terms,
    vals, nnz)."""
    rng = np.random.default_rng(seed)
    mean = mean_nnz if mean_nnz is not None else max(2, (3 * S) // 4)
    rows = zipf_rows(rng, n, S, mean)
    rows[0] = (np.zeros(0, np.int64), np.zeros(0, np.float32))
    rows[1] = (np.asarray([7]), np.asarray([1.5], np.float32))
    full = np.sort(rng.choice(5000, S, replace=False))
    rows[2] = (full, (0.5 + rng.random(S)).astype(np.float32))
    rows[3] = (np.asarray([0, 7, 65534]), np.asarray([2.0, -1.0, 0.25], np.float32))
    rows[4] = (np.asarray([0, 65534]), np.asarray([-0.5, 4.0], np.float32))
    tie0 = min(1000, n // 3) + 5                       # 40 rows from here cross 16-row tiles
    tie = (np.asarray([3, 7, 11, 500]), np.asarray([1.0, 0.5, -0.25, 2.0], np.float32))
    for r in range(tie0, tie0 + 40):
        rows[r] = tie
    terms, vals, nnz = pack(rows, S)
    return rows, terms, vals, nnz


def identical_corpus(n: int = 20000, S: int = 16):
    """n identical rows: more rows at the k-th best score than a hot pass keeps."""
    rows = [(np.asarray([5, 9]), np.asarray([1.0, 2.0], np.float32))] * n
    return (rows,) + pack(rows, S)


def queries(rng, rows, B: int, nnz: int):
    """B queries of `nnz` distinct terms each, drawn from the terms of random corpus rows (so
    they overlap) topped up with Zipf terms; weights in (0.2, 2), a few negative."""
    out = []
    for _ in range(B):
        pool = np.concatenate([rows[int(rng.integers(len(rows)))][0] for _ in range(4)] +
                              [(TERMS * rng.random(2 * nnz) ** 3).astype(np.int64)])
        t = np.unique(pool)
        t = np.sort(rng.permutation(t)[:nnz])
        w = (0.2 + 1.8 * rng.random(len(t))).astype(np.float32)
        w[rng.random(len(t)) < 0.1] *= -1
        out.append((t, w))
    return out


# ---------------------------------------------------------------- retrieval quality
RARE_TERM = 40000


def quality_case(seed: int = 3, n: int = 2000, dim: int = 384, S: int = 16):
    """A corpus where the dense vector cannot find what the sparse one names: n points with
    random dense vectors and a few common sparse terms each; 12 of them also hold RARE_TERM.
    Their dense vectors are drawn like the rest and the dense query is unrelated to them.
    Returns (x fp32 [n, dim], q fp32 [dim], sparse rows, the 12 rows ascending, the sparse
    query (indices, values))."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    rows = zipf_rows(rng, n, S, 6, vocab=1000, negative=0.0)
    rare = np.sort(rng.choice(n, 12, replace=False))
    for j, r in enumerate(rare.tolist()):
        t, v = rows[r]
        t, v = t[:S - 1], v[:S - 1]
        rows[r] = (np.append(t, RARE_TERM), np.append(v, np.float32(1.0 + 0.125 * j)))
    return x, q, rows, rare, (np.asarray([RARE_TERM]), np.asarray([1.0], np.float32))
