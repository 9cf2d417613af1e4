"""numpy restatement of discovery and context queries (rag_index_discover; include/ragmi.h
"Discovery queries"), built on the CPU oracle through _reco_ref: `examples` gives the
canonically normalised examples, `exact` the canonical exact scores e_x(r) over all rows, `top_k`
the (score desc, row asc) selection. The combine is this file's: fp32 comparisons for the signs,
fp64 sig / loss with ONE rounding at the end. TEST HELPER ONLY, shared by test_discover_cpu.py and
test_discover_gpu.py.
"""
import numpy as np

from _reco_ref import (encode, exact, examples, grouped_corpus, sig,  # noqa: F401
                       stored_f32, top_k)

DISCOVER_MAX_PAIRS, CONTEXT_MAX_PAIRS = 15, 16
SHIFT = np.float64(2.0 ** -23)


def sig64(x) -> np.ndarray:
    """recommend's sig before its rounding: 0.5 (x / (1 + |x|) + 1) in fp64 on the fp32 value.
    _reco_ref.sig is its fp32 rounding."""
    xd = np.asarray(x, np.float32).astype(np.float64)
    return 0.5 * (xd / (1.0 + np.abs(xd)) + 1.0)


def loss(d) -> np.ndarray:
    """l = m / (1 + |m|), m = min(d, 0), in fp64."""
    m = np.minimum(np.asarray(d, np.float64), 0.0)
    return m / (1.0 + np.abs(m))


def pair_scores(corpus, pairs):
    """(e_p, e_n) fp32 [n, rows] each: the exact scores of every row against the pairs' sides."""
    pos, neg = [p for p, _ in pairs], [n for _, n in pairs]
    return exact(corpus, examples(corpus, pos)), exact(corpus, examples(corpus, neg))


def ranks(corpus, pairs, stats=None) -> np.ndarray:
    """rank(r) = sum_i sgn(e_pi - e_ni) on the fp32 values, as fp64 integers [rows]."""
    ep, en = pair_scores(corpus, pairs)
    sgn = (ep > en).astype(np.int64) - (ep < en).astype(np.int64)
    if stats is not None:
        stats["plus"] = stats.get("plus", 0) + int((sgn > 0).sum())
        stats["minus"] = stats.get("minus", 0) + int((sgn < 0).sum())
        stats["zero"] = stats.get("zero", 0) + int((sgn == 0).sum())
    return sgn.sum(axis=0).astype(np.float64) if len(pairs) else np.zeros(corpus.shape[0])


def discover_scores(corpus, target, pairs, stats=None) -> np.ndarray:
    """fp32(rank + sig(e_t)) [rows]: the add in fp64, one rounding."""
    assert 0 <= len(pairs) <= DISCOVER_MAX_PAIRS
    et = exact(corpus, examples(corpus, [target]))[0]
    s = (ranks(corpus, pairs, stats) + sig64(et)).astype(np.float32)
    return s + np.float32(0.0)


def context_scores(corpus, pairs, stats=None) -> np.ndarray:
    """fp32(sum_i l_i) [rows], l_i the loss of d_i = e_pi - e_ni - 2^-23, accumulated in fp64 in
    pair order, one rounding."""
    assert 1 <= len(pairs) <= CONTEXT_MAX_PAIRS
    ep, en = pair_scores(corpus, pairs)
    acc = np.zeros(corpus.shape[0], np.float64)
    for p, n in zip(ep, en):                                  # pair order
        d = p.astype(np.float64) - n.astype(np.float64) - SHIFT
        if stats is not None:
            stats["plus"] = stats.get("plus", 0) + int((d >= 0).sum())
            stats["minus"] = stats.get("minus", 0) + int((d < 0).sum())
        acc = acc + loss(d)
    return acc.astype(np.float32) + np.float32(0.0)           # -0 -> +0


def scores(corpus, target, pairs, stats=None) -> np.ndarray:
    """The exact score of every stored row: a discover request with a target, a context request
    with None."""
    if target is None:
        return context_scores(corpus, pairs, stats)
    return discover_scores(corpus, target, pairs, stats)


def discover(corpus, target, pairs, k: int, passing=None, stats=None):
    """rag_index_discover: (scores [k], rows [k])."""
    return top_k(scores(corpus, target, pairs, stats), k, passing, stats)
