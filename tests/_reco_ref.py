"""numpy restatement of recommend queries (rag_index_recommend; include/ragmi.h "Recommend
queries"), built on the CPU oracle: oracle_scan.normalize gives the examples x_i,
oracle_scan.rescore the canonical exact scores e_i(r) over all rows; the combine is fp32 max,
fp64 sig / sum / mean with one rounding, and np.lexsort for (score desc, row asc). TEST HELPER
ONLY, shared by test_recommend_cpu.py and test_recommend_gpu.py; the corpus and the storage
forms are _mmr_ref's.
"""
import numpy as np

import oracle_scan as O
from _mmr_ref import encode, grouped_corpus, stored_f32  # noqa: F401  (re-exported)

AVERAGE, BEST, SUM = "average_vector", "best_score", "sum_scores"
MAX_SIDE = 16


def example(corpus, x):
    """An example as the vector the contract treats it as: an int is a stored row's id (its
    stored form as fp32), anything else the caller's vector."""
    if isinstance(x, (int, np.integer)):
        return stored_f32(corpus, int(x))
    return np.ascontiguousarray(x, np.float32)


def examples(corpus, side) -> np.ndarray:
    """x_i fp32 [n, D]: the side's examples through the canonical normalisation (an example with
    a non-finite component, or the zero vector, is the zero vector: it scores +0.0 everywhere)."""
    d = corpus.shape[1]
    if side is None or len(side) == 0:
        return np.empty((0, d), np.float32)
    return O.normalize(np.stack([example(corpus, x) for x in side]))


def exact(corpus, xs) -> np.ndarray:
    """e_i(r) fp32 [n, rows]: the canonical exact score of every stored row against x_i."""
    n = corpus.shape[0]
    if xs.shape[0] == 0:
        return np.empty((0, n), np.float32)
    rows = np.broadcast_to(np.arange(n, dtype=np.int64), (xs.shape[0], n))
    return O.rescore(corpus, xs, np.ascontiguousarray(rows))


def sig(x) -> np.ndarray:
    """0.5 (x / (1 + |x|) + 1) in fp64 on the fp32 value, rounded once to fp32."""
    xd = np.asarray(x, np.float32).astype(np.float64)
    return (0.5 * (xd / (1.0 + np.abs(xd)) + 1.0)).astype(np.float32)


def best_of(mp, mn) -> np.ndarray:
    """F(mp, mn) = sig(mp) if mp > mn else -sig(mn), elementwise on fp32 (a side's -inf: that
    side is empty; never both)."""
    mp = np.asarray(mp, np.float32)
    mn = np.asarray(mn, np.float32)
    pos = mp > mn
    arg = np.where(pos, mp, mn)
    s = sig(arg)
    return np.where(pos, s, -s).astype(np.float32)


def scores(corpus, pos, neg, strategy, stats=None) -> np.ndarray:
    """The exact combined score fp32 [rows] of every stored row (BEST or SUM)."""
    ep, en = exact(corpus, examples(corpus, pos)), exact(corpus, examples(corpus, neg))
    n = corpus.shape[0]
    assert ep.shape[0] <= MAX_SIDE and en.shape[0] <= MAX_SIDE and ep.shape[0] + en.shape[0] >= 1
    if strategy == BEST:
        mp = ep.max(axis=0) if ep.shape[0] else np.full(n, -np.inf, np.float32)
        mn = en.max(axis=0) if en.shape[0] else np.full(n, -np.inf, np.float32)
        if stats is not None:
            stats["pos_branch"] = int((mp > mn).sum())
            stats["neg_branch"] = int((~(mp > mn)).sum())
        s = best_of(mp, mn)
    else:
        assert strategy == SUM
        acc = np.zeros(n, np.float64)
        for e in ep:                                  # example order, positives first
            acc = acc + e.astype(np.float64)
        for e in en:
            acc = acc - e.astype(np.float64)
        s = acc.astype(np.float32)
    return s + np.float32(0.0)                        # -0 -> +0: one key for both


def top_k(s, k: int, passing=None, stats=None):
    """(scores [k], rows [k]) of the k best passing rows by (score desc, row asc), -inf / -1
    padding. stats["ties"]: pairs of equal neighbouring scores among the returned rows."""
    rows = np.arange(s.shape[0], dtype=np.int64)
    if passing is not None:
        rows = rows[np.asarray(passing, bool)]
    sc = s[rows]
    order = np.lexsort((rows, -sc.astype(np.float64)))[:k]
    out_s = np.full(k, -np.inf, np.float32)
    out_r = np.full(k, -1, np.int64)
    out_s[:order.size], out_r[:order.size] = sc[order], rows[order]
    if stats is not None:
        stats["ties"] = stats.get("ties", 0) + int((np.diff(sc[order]) == 0).sum())
    return out_s, out_r


def recommend(corpus, pos, neg, strategy, k: int, passing=None, stats=None):
    """rag_index_recommend for BEST / SUM: (scores [k], rows [k])."""
    return top_k(scores(corpus, pos, neg, strategy, stats), k, passing, stats)


def average_vector(corpus, pos, neg) -> np.ndarray:
    """AVERAGE_VECTOR's target v fp32 [D]: a_pos, or a_pos + (a_pos - a_neg); the means
    accumulated per component in fp64 in example order, one rounding."""
    xp, xn = examples(corpus, pos), examples(corpus, neg)
    assert xp.shape[0] >= 1

    def mean(xs):
        acc = np.zeros(xs.shape[1], np.float64)
        for x in xs:
            acc = acc + x.astype(np.float64)
        return acc / np.float64(xs.shape[0])

    ap = mean(xp)
    v = ap if xn.shape[0] == 0 else ap + (ap - mean(xn))
    return v.astype(np.float32)
