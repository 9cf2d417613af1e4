"""Sparse vectors on the host: the stored slot layout, the refusals that keep it, BM25-style
document and query vectors from WordPiece ids, and the IDF query weights.

The device side is rag_index_sparse_* (include/ragmi.h "Sparse vectors"): a row
of S slots holds its nonzero entries in ascending term order, then SPARSE_TERM_NONE / 0.0. The
terms are WordPiece ids (30,522 of them in the BERT vocabulary the encoder uses), so nothing
beyond the encoder's own vocab.txt is needed to make sparse vectors. Host code over numpy arrays.
"""
from __future__ import annotations

import math

import numpy as np

from . import qdrant_models as models
from .index import SPARSE_MAX_QUERY_NNZ, SPARSE_TERM_NONE, SPARSE_TERMS

# [PAD] [UNK] [CLS] [SEP] [MASK] of the BERT WordPiece vocabulary: no content, never a term
SPECIAL_TOKENS = frozenset((0, 100, 101, 102, 103))


def entries(vector, who: str):
    """(indices int64 [m], values fp32 [m]) of a SparseVector (or an object / dict with `indices`
    and `values`), explicit zeros dropped, ascending by index — or ValueError naming `who`: the
    two lists must pair up, an index must be an integer in [0, 65535) (Qdrant takes uint32: a
    documented deviation), a value finite, and no index may repeat (as Qdrant refuses)."""
    if isinstance(vector, dict):
        idx, val = vector.get("indices"), vector.get("values")
    else:
        idx, val = getattr(vector, "indices", None), getattr(vector, "values", None)
    if idx is None or val is None:
        raise ValueError(f"{who}: a sparse vector is SparseVector(indices=[...], values=[...])")
    raw = np.asarray(idx).reshape(-1)
    if raw.size and raw.dtype.kind not in "iu":
        raise ValueError(f"{who}: sparse indices must be integers")
    idx = raw.astype(np.int64)
    val64 = np.asarray(val, np.float64).reshape(-1)
    if idx.shape != val64.shape:
        raise ValueError(f"{who}: {idx.size} sparse indices for {val64.size} values")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= SPARSE_TERMS):
        bad = int(idx[(idx < 0) | (idx >= SPARSE_TERMS)][0])
        raise ValueError(f"{who}: sparse index {bad} outside [0, {SPARSE_TERMS}) (terms are "
                         "16-bit here; Qdrant's are uint32)")
    with np.errstate(over="ignore"):
        val = val64.astype(np.float32)
    if not np.isfinite(val).all():
        raise ValueError(f"{who}: a sparse value is not finite (inf or NaN, or beyond fp32)")
    if np.unique(idx).size != idx.size:
        raise ValueError(f"{who}: a sparse index repeats")
    keep = val != 0
    idx, val = idx[keep], val[keep]
    order = np.argsort(idx, kind="stable")
    return idx[order], val[order]


def pack_rows(vectors: list, slots: int, names=None, what: str = "point"):
    """Sparse vectors (SparseVector or None = empty) as padded rows in the stored layout: (terms
    uint16 [n, slots], vals fp32 [n, slots], nnz int32 [n]). ValueError (entries', or more than
    `slots` nonzeros) names `what` and names[i], else the position i."""
    n = len(vectors)
    terms = np.full((n, slots), SPARSE_TERM_NONE, np.uint16)
    vals = np.zeros((n, slots), np.float32)
    nnz = np.zeros(n, np.int32)
    for i, v in enumerate(vectors):
        if v is None:
            continue
        who = f"{what} {names[i]!r}" if names is not None else f"{what} at position {i}"
        idx, val = entries(v, who)
        if idx.size > slots:
            raise ValueError(f"{who}: {idx.size} nonzeros, at most {slots} fit a sparse "
                             + ("query" if slots == SPARSE_MAX_QUERY_NNZ and what != "point"
                                else "row (sparse_slots)"))
        terms[i, :idx.size] = idx
        vals[i, :idx.size] = val
        nnz[i] = idx.size
    return terms, vals, nnz


def unpack_row(terms, vals) -> models.SparseVector:
    """One stored row (uint16 / int16 bits and fp32 [slots]) as a SparseVector."""
    t = np.asarray(terms).reshape(-1).view(np.uint16) if np.asarray(terms).dtype == np.int16 \
        else np.asarray(terms, np.uint16).reshape(-1)
    keep = t != SPARSE_TERM_NONE
    return models.SparseVector(indices=t[keep].astype(np.int64).tolist(),
                               values=np.asarray(vals, np.float32).reshape(-1)[keep].tolist())


def idf_weights(indices, values, df, n_docs: int) -> np.ndarray:
    """Modifier.IDF on the host: w' = float32(float64(w) * ln(1 + (N - df + 0.5) / (df + 0.5))),
    df the document frequency of the term (rag_index_sparse_df) and N the points with a non-empty
    sparse row. This restates Qdrant's IDF formula from memory of its source; parity with a
    Qdrant server's own arithmetic is unpinned (as for MMR and formulas). The device never takes
    a logarithm."""
    out = np.empty(len(indices), np.float32)
    for j, (t, w) in enumerate(zip(indices, values)):
        d = float(df[int(t)])
        out[j] = np.float32(float(np.float32(w)) *
                            math.log(1.0 + (float(n_docs) - d + 0.5) / (d + 0.5)))
    return out


def _content(token_ids) -> list:
    return [int(t) for t in np.asarray(token_ids).reshape(-1).tolist()
            if int(t) not in SPECIAL_TOKENS]


def bm25_document(token_ids, k1: float = 1.2, b: float = 0.75, avg_len: float = 256.0,
                  slots: int = 128) -> models.SparseVector:
    """The BM25 term-frequency vector of one text from its WordPiece ids (one sequence of
    WordPiece.encode_packed's output): the special tokens and [UNK] are dropped, len is the
    number of tokens kept, and the distinct term t with count tf weighs
    tf * (k1 + 1) / (tf + k1 * (1 - b + b * len / avg_len)), computed in fp64 and rounded to
    fp32. More than `slots` distinct terms: the `slots` largest values are kept, ties going to the
    lower term. The IDF half of BM25 is the collection's (Modifier.IDF)."""
    ids = _content(token_ids)
    tf: dict = {}
    for t in ids:
        tf[t] = tf.get(t, 0) + 1
    norm = k1 * (1.0 - b + b * len(ids) / avg_len)
    items = [(t, np.float32(c * (k1 + 1.0) / (c + norm))) for t, c in tf.items()]
    if len(items) > slots:
        items.sort(key=lambda x: (-float(x[1]), x[0]))
        items = items[:slots]
    items.sort()
    return models.SparseVector(indices=[t for t, _ in items], values=[float(v) for _, v in items])


def bm25_query(token_ids) -> models.SparseVector:
    """The query side: the distinct content terms, each weighted 1.0, ascending."""
    terms = sorted(set(_content(token_ids)))
    return models.SparseVector(indices=terms, values=[1.0] * len(terms))


def sequences(ids, cu) -> list:
    """WordPiece.encode_packed's (ids, cu_seqlens) split into one id array per text."""
    return [np.asarray(ids[int(cu[i]):int(cu[i + 1])]) for i in range(len(cu) - 1)]
