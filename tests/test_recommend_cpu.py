"""CPU tests of recommend queries: the RecommendStrategy / RecommendInput / RecommendQuery models
and their defaults, every refusal of recommend_params and of the routes, QdrantClient's routing
over a stand-in index, the numpy restatement's own properties, rag_index_recommend's argument
refusals (no device), and the header / binding / docs."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import _reco_ref as R
import _stubs as S


# ------------------------------------------------------------------ 1. models and defaults
def test_models_and_defaults():
    from ragmi import qdrant_models as m
    from ragmi.index import RECO_MAX_SIDE, reco_strategy
    from ragmi.qdrant import RECOMMEND, recommend_params, route_of
    assert [s.value for s in m.RecommendStrategy] == ["average_vector", "best_score", "sum_scores"]
    assert m.RecommendInput() == m.RecommendInput(positive=None, negative=None, strategy=None)
    q = m.RecommendQuery(recommend=m.RecommendInput(positive=[7]))
    assert route_of(q) == RECOMMEND and route_of(q, prefetch=[m.Prefetch()]) == RECOMMEND
    assert RECO_MAX_SIDE == 16
    assert [reco_strategy(s) for s in (None, m.RecommendStrategy.AVERAGE_VECTOR, "best_score",
                                       m.RecommendStrategy.SUM_SCORES, 1)] == [0, 0, 1, 2, 1]
    assert recommend_params(q, 10) == ([7], [], 0)
    v = [0.0, 1.0]
    q = m.RecommendQuery(m.RecommendInput([7, v], ["6f1ed002ab5595859014ebf0951522d9"],
                                          m.RecommendStrategy.BEST_SCORE))
    assert recommend_params(q, np.int64(3)) == ([7, v], ["6f1ed002ab5595859014ebf0951522d9"], 1)
    only_neg = m.RecommendInput(negative=[1], strategy="sum_scores")
    assert recommend_params(m.RecommendQuery(only_neg), 1) == ([], [1], 2)


def test_recommend_params_refusals():
    from ragmi import qdrant_models as m
    from ragmi.qdrant import recommend_params

    def bad(match, limit=10, **kw):
        with pytest.raises(ValueError, match=match):
            recommend_params(m.RecommendQuery(m.RecommendInput(**kw)), limit)

    bad("at most 16 positive", positive=list(range(17)))
    bad("at most 16 negative", positive=[1], negative=list(range(17)))
    bad("at least one")
    bad("at least one", positive=[], negative=[])
    bad("needs a positive", negative=[1])
    bad("needs a positive", negative=[1], strategy=m.RecommendStrategy.AVERAGE_VECTOR)
    bad("unknown recommend strategy", positive=[1], strategy="dbsf")
    bad("unknown recommend strategy", positive=[1], strategy=7)
    bad("must be a list", positive="abc")
    bad("must be a list", positive=[1], negative=5)
    for limit in (None, 2.0, "3", True):
        bad("int limit", limit=limit, positive=[1])
    with pytest.raises(ValueError, match="RecommendQuery"):
        recommend_params([0.0, 1.0], 10)
    with pytest.raises(ValueError, match="RecommendInput"):
        recommend_params(m.RecommendQuery(recommend=[1, 2]), 10)


def test_header_binding_and_docs_name_the_calls():
    from ragmi import _lib
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("rag_index_recommend", 16), ("rag_index_reco_bounds", 11),
                         ("rag_index_reco_vector", 7), ("rag_index_reco_stats", 2)):
        assert re.search(r"^int %s\(rag_index_t\* index," % name, code, re.M)
        assert len(_lib.INDEX_API[name][1]) == n_args
    for line in ("#define RAG_RECO_AVERAGE 0", "#define RAG_RECO_BEST 1",
                 "#define RAG_RECO_SUM 2", "#define RAG_RECO_MAX_SIDE 16"):
        assert re.search("^%s$" % line, code, re.M)
    assert "parity with a Qdrant server's own arithmetic is unpinned" in " ".join(hdr.split())
    assert "zero-vector example" in hdr
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "rag_index_recommend" in doc and "RecommendQuery" in doc
    assert "recommend over a shard set is not built" in " ".join(doc.split())


# ------------------------------------------------------------------ 2. the restatement itself
@pytest.fixture(scope="module")
def seed7():
    x, q, group = R.grouped_corpus(384)
    return R.encode(x, "fp16"), q, group


def test_ref_one_positive_ranks_as_plain_search(seed7):
    import oracle_scan as O
    enc, q, _ = seed7
    s, r = O.search(enc, q[None], 20)
    for strategy in (R.BEST, R.SUM):
        assert np.array_equal(R.recommend(enc, [q], [], strategy, 20)[1], r[0])
    # SUM with one positive IS the exact score; BEST is sig of it
    assert np.array_equal(R.recommend(enc, [q], [], R.SUM, 20)[0].view(np.uint32),
                          s[0].view(np.uint32))
    assert np.array_equal(R.recommend(enc, [q], [], R.BEST, 20)[0], R.sig(s[0]))
    # AVERAGE with one positive: v is the normalised query, so search(v) is search(q)
    v = R.average_vector(enc, [q], [])
    assert np.array_equal(v, O.normalize(q[None])[0])
    assert np.array_equal(O.search(enc, v[None], 20)[1], r)


def test_ref_negative_equal_to_a_row(seed7):
    enc, q, _ = seed7
    row = 1234
    s = R.scores(enc, [q], [row], R.BEST)
    e_self = R.exact(enc, R.examples(enc, [row]))[0, row]
    assert abs(float(e_self) - 1.0) < 1e-3                    # a stored row against itself
    assert s[row] == -R.sig(e_self) and abs(float(s[row]) + 0.75) < 1e-3   # -sig(1) = -0.75
    stats = {}
    R.recommend(enc, [q], [row], R.BEST, 3001, stats=stats)
    assert stats["pos_branch"] > 0 and stats["neg_branch"] > 0


def test_ref_F_is_monotone():
    grid = np.concatenate([np.linspace(-1.0, 1.0, 81, dtype=np.float32),
                           np.float32([-1e-7, 0.0, 1e-7, 0.25, np.nextafter(np.float32(0.25), 1)])])
    grid = np.unique(grid)
    mp, mn = np.meshgrid(grid, grid, indexing="ij")           # includes mp == mn
    F = R.best_of(mp, mn)
    assert (np.diff(F, axis=0) >= 0).all()                    # non-decreasing in mp
    assert (np.diff(F, axis=1) <= 0).all()                    # non-increasing in mn
    assert (F[mp > mn] >= 0).all() and (F[mp <= mn] <= 0).all()
    ninf = np.full_like(grid, -np.inf)
    assert np.array_equal(R.best_of(grid, ninf), R.sig(grid))            # N = 0
    assert np.array_equal(R.best_of(ninf, grid), -R.sig(grid))           # P = 0
    assert (np.diff(R.sig(grid)) >= 0).all()


def test_ref_sum_and_average_arithmetic(seed7):
    enc, q, _ = seed7
    rng = np.random.default_rng(3)
    pos = [q, 17, rng.standard_normal(384).astype(np.float32)]
    neg = [99, rng.standard_normal(384).astype(np.float32)]
    ep, en = R.exact(enc, R.examples(enc, pos)), R.exact(enc, R.examples(enc, neg))
    want = (((ep[0].astype(np.float64) + ep[1]) + ep[2]) - en[0]) - en[1]
    assert np.array_equal(R.scores(enc, pos, neg, R.SUM), want.astype(np.float32))
    xp, xn = R.examples(enc, pos).astype(np.float64), R.examples(enc, neg).astype(np.float64)
    ap, an = ((xp[0] + xp[1]) + xp[2]) / 3.0, (xn[0] + xn[1]) / 2.0
    assert np.array_equal(R.average_vector(enc, pos, neg), (ap + (ap - an)).astype(np.float32))
    # a zero-vector example normalises to the zero query: it scores 0 against every row
    z = np.zeros(384, np.float32)
    assert not R.exact(enc, R.examples(enc, [z])).any()
    s, r = R.recommend(enc, [q], [], R.BEST, 8, passing=np.arange(3001) < 5)
    assert (r[:5] >= 0).all() and (r[5:] == -1).all() and np.isneginf(s[5:]).all()


# ------------------------------------------------------------------ 3. argument refusals
def test_recommend_argument_errors_need_no_device():
    from ragmi import _build, _lib
    _build.build()
    L = _lib.load()
    buf = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(buf)

    def call(P, N, strategy, k, pos=p, neg=p, progs=None, words=0, U=0, flags=0, out=p, h=None):
        return L.rag_index_recommend(h, pos, P, neg, N, strategy, k, progs, words, U, None, 0,
                                     flags, out, out, None)

    err = L.rag_last_error
    assert call(17, 0, 1, 5) != 0 and b"RAG_RECO_MAX_SIDE=16" in err()
    assert call(1, 17, 2, 5) != 0 and b"RAG_RECO_MAX_SIDE=16" in err()
    assert call(-1, 0, 1, 5) != 0
    assert call(0, 0, 1, 5) != 0 and b"at least one example" in err()
    assert call(0, 2, 0, 5) != 0 and b"RAG_RECO_AVERAGE needs a positive" in err()
    assert call(1, 0, 3, 5) != 0 and b"unknown strategy" in err()
    assert call(1, 0, -1, 5) != 0 and b"unknown strategy" in err()
    assert call(1, 0, 1, 0) != 0 and b"k must be >= 1" in err()
    assert call(1, 1, 1, 5, pos=None) != 0 and b"NULL example" in err()
    assert call(1, 1, 1, 5, neg=None) != 0 and b"NULL example" in err()
    assert call(1, 0, 1, 5, neg=None, out=None) != 0 and b"NULL output" in err()
    assert call(1, 0, 1, 5, flags=2) != 0 and b"unknown flags" in err()
    assert call(1, 0, 1, 5, progs=p, words=41, U=0) != 0 and b"n_programs" in err()
    assert call(1, 0, 1, 5, progs=p, words=3, U=1) != 0 and b"words" in err()
    assert call(1, 0, 1, 5, words=41, U=1) != 0 and b"programs is NULL" in err()
    assert call(1, 0, 1, 5, neg=None) != 0 and b"index is NULL" in err()

    def bounds(P, N, strategy, n, rows=p, out=p):
        return L.rag_index_reco_bounds(None, p, P, p, N, strategy, rows, n, out, out, None)

    assert bounds(17, 0, 1, 1) != 0 and b"RAG_RECO_MAX_SIDE=16" in err()
    assert bounds(1, 0, 0, 1) != 0 and b"RAG_RECO_BEST=1" in err()
    assert bounds(1, 0, 1, 1, rows=None) != 0 and b"NULL" in err()
    assert bounds(1, 0, 1, 1) != 0 and b"index is NULL" in err()
    assert L.rag_index_reco_vector(None, p, 0, p, 1, p, None) != 0 and b"positive" in err()
    assert L.rag_index_reco_vector(None, p, 1, p, 0, None, None) != 0 and b"NULL output" in err()
    assert L.rag_index_reco_stats(None, buf) != 0


# ------------------------------------------------------------------ 4. QdrantClient routing
class _StubIndex:
    """FlatIndex stand-in: recommend records what it was asked and returns rows 0..k-1 with
    falling scores; gather_rows returns row r as the fp32 vector [r, 0, 0, 0]."""
    device = None
    storage = "fp32"

    def __init__(self, count):
        self.count = count
        self.calls = []

    def search(self, q, k, filters=None, full=False, rescue=False):
        import torch
        B = len(q)
        self.calls.append(("search", B, k, None if filters is None else filters.tolist()))
        return (torch.linspace(0.9, 0.1, k).repeat(B, 1),
                torch.arange(k, dtype=torch.int64).repeat(B, 1))

    def unanswered(self):
        return 0

    def gather_rows(self, rows):
        import torch
        rows = np.asarray(rows, np.int64)
        self.calls.append(("gather_rows", rows.tolist()))
        f32 = torch.zeros((len(rows), 4))
        f32[:, 0] = torch.as_tensor(rows, dtype=torch.float32)
        return None, f32, None

    def recommend(self, pos, neg, strategy, k, filters=None, programs=None, rescue=False):
        import torch
        side = lambda t: None if t is None else np.asarray(t).tolist()  # noqa: E731
        self.calls.append(("recommend", side(pos), side(neg), strategy, k, filters,
                           programs is not None, rescue))
        return torch.linspace(0.9, 0.1, k), torch.arange(k, dtype=torch.int64)


def stub_client(count=40):
    return S.stub_client(S.stub_collection(
        _StubIndex(count), dim=4, ids=range(100, 100 + count),
        payloads=[{"ticker": "AMD" if r % 2 else "AAPL", "n": r} for r in range(count)]))


def _rq(positive=None, negative=None, strategy=None):
    from ragmi import qdrant_models as m
    return m.RecommendQuery(m.RecommendInput(positive, negative, strategy))


def test_recommend_route_resolves_ids_and_drops_the_examples():
    from ragmi import qdrant_models as m
    client, col = stub_client()
    v = [0.0, 1.0, 0.0, 0.0]
    amd = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    r = client.query_points("t", _rq([101, v, 103], [102], m.RecommendStrategy.BEST_SCORE),
                            limit=5, query_filter=amd)
    assert col.coalescer.requests == 0 and col.coalescer.batches == 0
    # ids 101, 103, 102 are rows 1, 3, 2: gathered, then limit + 3 hits asked for, under rescue
    assert col.index.calls == [
        ("gather_rows", [1, 3]), ("gather_rows", [2]),
        ("recommend", [[1.0, 0, 0, 0], v, [3.0, 0, 0, 0]], [[2.0, 0, 0, 0]], 1, 8, (0xFFFF, 2),
         False, True)]
    # rows 1, 2, 3 dropped out of 0..7, cut to 5
    assert [p.id for p in r.points] == [100, 104, 105, 106, 107]
    assert r.points[0].payload == {"ticker": "AAPL", "n": 0}
    assert r.points[0].score == pytest.approx(0.9)
    col.index.calls.clear()
    # the legacy spelling; duplicates of one id count once; vectors alone: nothing gathered
    pts = client.recommend("t", positive=[101, 101], limit=3, with_payload=False)
    assert col.index.calls[-1][3:5] == (0, 4)
    assert [p.id for p in pts] == [100, 102, 103] and pts[0].payload is None
    col.index.calls.clear()
    pts = client.recommend("t", positive=[v], negative=[np.asarray(v, np.float32)],
                           strategy="sum_scores", limit=50)
    assert col.index.calls == [("recommend", [v], [v], 2, 40, None, False, True)]   # k <= count
    assert len(pts) == 40


def test_recommend_route_refusals_and_empty_answers():
    from ragmi import qdrant_models as m
    client, col = stub_client()
    v = [0.0, 1.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="example point 999 is not in collection"):
        client.query_points("t", _rq([999]), limit=5)
    with pytest.raises(ValueError, match="prefetched candidates"):
        client.query_points("t", _rq([101]), limit=5, prefetch=[m.Prefetch(query=v)])
    with pytest.raises(ValueError, match="RecommendQuery inside a Prefetch"):
        client.query_points("t", m.FusionQuery(m.Fusion.RRF), limit=5,
                            prefetch=[m.Prefetch(query=_rq([101]))])
    with pytest.raises(ValueError, match="grouped"):
        client.query_points_groups("t", _rq([101]), group_by="ticker")
    with pytest.raises(ValueError, match="using"):
        client.query_points("t", _rq([101]), limit=5, using="title")
    with pytest.raises(ValueError, match="lookup_from"):
        client.recommend("t", positive=[101], lookup_from="other")
    with pytest.raises(ValueError, match="at most 16"):
        client.recommend("t", positive=list(range(100, 117)))
    with pytest.raises(ValueError, match="needs a positive"):
        client.recommend("t", negative=[101])
    with pytest.raises(ValueError, match="int limit"):
        client.query_points("t", _rq([101]), limit=None)
    assert col.index.calls == []                               # refused before any index call
    never = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="NONE"))])
    assert client.query_points("t", _rq([101]), limit=5, query_filter=never).points == []
    assert client.query_points("t", _rq([101]), limit=0).points == []
    assert col.index.calls == []                               # ... and no launch for these
    empty, ecol = stub_client(count=0)
    assert empty.query_points("t", _rq([v]), limit=5).points == []
    assert ecol.index.calls == []


def test_mixed_batch_routes_recommend_one_pass_each_in_order():
    from ragmi import qdrant_models as m
    client, col = stub_client()
    v = [0.0, 1.0, 0.0, 0.0]
    reqs = [m.QueryRequest(query=v, limit=7),
            m.QueryRequest(query=_rq([105], None, "best_score"), limit=2),
            m.QueryRequest(query=v, limit=3, with_payload=False),
            m.QueryRequest(query=_rq([v], [106], m.RecommendStrategy.SUM_SCORES), limit=4,
                           with_payload=False)]
    out = client.query_batch_points("t", reqs)
    assert [len(r.points) for r in out] == [7, 2, 3, 4]
    reco = [c for c in col.index.calls if c[0] == "recommend"]
    assert [(c[3], c[4]) for c in reco] == [(1, 3), (2, 5)]    # one pass each, in request order
    assert [c for c in col.index.calls if c[0] == "search"] == [("search", 2, 7, None)]
    assert col.coalescer.requests == 0
    assert out[3].points[0].payload is None and out[1].points[0].payload is not None
    assert 105 not in [p.id for p in out[1].points] and 106 not in [p.id for p in out[3].points]


def test_shard_set_collection_refuses():
    from ragmi.collection import Collection
    from ragmi.shardset import ShardSet
    assert not hasattr(ShardSet, "recommend")                  # how a Collection tells

    class StubSet:
        device, storage, count = None, "fp32", 4

    col = Collection("t", 4, None, index=StubSet())
    with pytest.raises(NotImplementedError, match="recommend over a shard set is not built"):
        col.search_recommend([([[0.0, 1.0, 0.0, 0.0]], [], 1, (0, 0), 5)])


def test_rag_similar_chunks(monkeypatch):
    from ragmi import qdrant_models as m
    from ragmi import rag
    seen = []

    class Fake:
        def query_points(self, **kw):
            seen.append(kw)
            return m.QueryResponse()

    monkeypatch.setattr(rag, "_testing", lambda: False)
    monkeypatch.setattr(rag, "get_qdrant", lambda: Fake())
    rag.similar_chunks(["a" * 32, "b" * 32], not_like=["c" * 32], ticker="amd", limit=4)
    assert seen[-1]["query"] == m.RecommendQuery(m.RecommendInput(
        ["a" * 32, "b" * 32], ["c" * 32], m.RecommendStrategy.BEST_SCORE))
    assert seen[-1]["limit"] == 4
    assert seen[-1]["query_filter"] == m.Filter(must=[m.FieldCondition(
        key="ticker", match=m.MatchValue(value="AMD"))])
    rag.similar_chunks([5])
    assert seen[-1]["query_filter"] is None and seen[-1]["limit"] == rag.RETRIEVE_LIMIT
