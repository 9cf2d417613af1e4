"""CPU tests of discovery and context queries: the numpy restatement's own
properties, the model classes, route_of / discover_params on every accepted spelling, every
refusal of the route, the C ABI's argument refusals (reached without a device, as recommend's
are) and the routing through QdrantClient over a stub index.

The four test_ref_* tests check tests/_discover_ref.py against the oracle alone: they state what
the restatement means and pass without the feature; they are no evidence for it. Every other test
here, and every GPU test, needs the feature."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import _discover_ref as R
import _stubs as S


# ------------------------------------------------------------------ 1. the restatement itself
@pytest.fixture(scope="module")
def seed7():
    x, q, group = R.grouped_corpus(384)
    return R.encode(x, "fp16"), q, group


def _vec(rng):
    return rng.standard_normal(384).astype(np.float32)


def test_ref_discover_scores_lie_in_rank_plus_unit_interval(seed7):
    enc, q, _ = seed7
    rng = np.random.default_rng(1)
    pairs = [(17, _vec(rng)), (_vec(rng), 99), (_vec(rng), _vec(rng))]
    stats = {}
    s = R.discover_scores(enc, q, pairs, stats)
    rank = R.ranks(enc, pairs)
    assert stats["plus"] > 0 and stats["minus"] > 0
    assert set(np.unique(rank)) <= {-3.0, -1.0, 1.0, 3.0, -2.0, 0.0, 2.0}
    frac = s.astype(np.float64) - rank
    assert (frac >= 0.0).all() and (frac <= 1.0).all()
    # the fraction is sig of the target's exact score, up to the one fp32 rounding of the sum
    et = R.exact(enc, R.examples(enc, [q]))[0]
    assert np.abs(frac - R.sig(et)).max() <= 2.0 ** -22
    assert np.array_equal(s, (rank + R.sig64(et)).astype(np.float32))


def test_ref_equal_pair_adds_nothing_to_ranks_and_a_constant_to_context(seed7):
    enc, q, _ = seed7
    rng = np.random.default_rng(2)
    same = _vec(rng)
    base = [(5, _vec(rng))]
    stats = {}
    assert np.array_equal(R.ranks(enc, base + [(same, same)], stats), R.ranks(enc, base))
    assert stats["zero"] == enc.shape[0]                        # the sign-0 branch, every row
    assert np.array_equal(R.discover_scores(enc, q, base + [(same, same)]),
                          R.discover_scores(enc, q, base))
    # context: d = -2^-23 for every row, so the pair alone scores l(-2^-23) everywhere
    l0 = R.loss(-R.SHIFT)
    only = R.context_scores(enc, [(same, same)])
    assert np.array_equal(only, np.full(enc.shape[0], np.float32(l0)))
    assert -2.0 ** -23 < l0 < -2.0 ** -23 * (1 - 2.0 ** -22)    # -2^-23 / (1 + 2^-23)
    ep, en = R.pair_scores(enc, base)
    want = R.loss(ep[0].astype(np.float64) - en[0] - R.SHIFT) + l0
    assert np.array_equal(R.context_scores(enc, base + [(same, same)]), want.astype(np.float32))


def test_ref_context_scores_are_at_most_zero(seed7):
    enc, _, _ = seed7
    rng = np.random.default_rng(3)
    pairs = [(_vec(rng), _vec(rng)) for _ in range(4)] + [(1500, 7)]
    s = R.context_scores(enc, pairs)
    assert (s <= 0).all() and (s > -len(pairs)).all()
    assert not np.signbit(s[s == 0]).any()                      # -0 -> +0
    ep, en = R.pair_scores(enc, pairs)
    ok = ((ep.astype(np.float64) - en - R.SHIFT) >= 0).all(axis=0)
    assert np.array_equal(s == 0, ok) and 0 < ok.sum() < len(s)  # 0 exactly when every pair holds
    # the loss: 0 for d >= 0, increasing and 1-Lipschitz below
    d = np.linspace(-2.0, 1.0, 3001)
    lo = R.loss(d)
    assert (lo[d >= 0] == 0).all() and (np.diff(lo) >= 0).all()
    assert (np.diff(lo) <= np.diff(d) * (1 + 1e-12)).all()


def test_ref_no_pairs_orders_as_the_nearest_search(seed7):
    import oracle_scan as O
    enc, q, _ = seed7
    s = R.discover_scores(enc, q, [])
    et = R.exact(enc, R.examples(enc, [q]))[0]
    assert np.array_equal(s, R.sig(et))                         # rank 0: sig's own rounding
    # the nearest search's order, except where sig's rounding merges neighbouring scores
    near = O.search(enc, q[None], 3001)[1][0]
    assert (np.diff(s[near]) <= 0).all()
    got = R.discover(enc, q, [], 20)[1]
    assert set(got[:5]) == set(near[:5])
    # sig is monotone, so a strictly better discover score is a strictly better exact score
    order = np.argsort(-s, kind="stable")
    assert (np.diff(et[order])[np.diff(s[order]) < 0] < 0).all()


# ------------------------------------------------------------------ 2. models, routes, parameters
def test_models_routes_and_params():
    from ragmi import qdrant_models as m
    from ragmi.qdrant import DISCOVER, discover_params, route_of
    v, w = [0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]
    one = m.ContextPair(positive=5, negative=w)
    assert m.DiscoverInput(target=v).context is None
    dq = m.DiscoverQuery(discover=m.DiscoverInput(target=v, context=[one, m.ContextPair(7, 8)]))
    assert route_of(dq) == DISCOVER and route_of(dq, prefetch=[m.Prefetch(query=v)]) == DISCOVER
    assert discover_params(dq, 10) == (v, [(5, w), (7, 8)])
    # one pair or a list, with and without a target; no context at all with a target
    assert discover_params(m.DiscoverQuery(m.DiscoverInput(v, one)), 3) == (v, [(5, w)])
    assert discover_params(m.DiscoverQuery(m.DiscoverInput(11)), 3) == (11, [])
    assert discover_params(m.DiscoverQuery(m.DiscoverInput(v, [])), 3) == (v, [])
    cq = m.ContextQuery(context=one)
    assert route_of(cq) == DISCOVER and discover_params(cq, 1) == (None, [(5, w)])
    assert discover_params(m.ContextQuery(context=[one] * 16), 1)[1] == [(5, w)] * 16
    assert discover_params(m.DiscoverQuery(m.DiscoverInput(v, [one] * 15)), 1)[1] == [(5, w)] * 15
    assert route_of(v) != DISCOVER and route_of(m.RecommendQuery(m.RecommendInput([1]))) != DISCOVER


def test_discover_params_refusals():
    from ragmi import qdrant_models as m
    from ragmi.qdrant import discover_params
    v = [0.0, 1.0, 0.0, 0.0]
    one = m.ContextPair(positive=5, negative=6)
    for query, limit, match in (
            (m.DiscoverQuery(m.DiscoverInput(v, [one] * 16)), 5, "at most 15 context pairs"),
            (m.ContextQuery([one] * 17), 5, "at most 16 context pairs"),
            (m.ContextQuery([]), 5, "ContextQuery without pairs is not built"),
            (m.ContextQuery(None), 5, "ContextQuery without pairs is not built"),
            (m.DiscoverQuery(m.DiscoverInput(None, [one])), 5, "needs a target"),
            (m.DiscoverQuery(discover=[1, 2]), 5, "DiscoverInput"),
            (m.ContextQuery([one, (5, 6)]), 5, r"context\[1\] is not a ContextPair"),
            (m.ContextQuery([m.ContextPair(5, None)]), 5, "a positive and a negative"),
            (m.ContextQuery("abc"), 5, "ContextPair or a list"),
            (m.ContextQuery(one), None, "int limit"),
            (m.ContextQuery(one), True, "int limit"),
            (v, 5, "DiscoverQuery or a ContextQuery")):
        with pytest.raises(ValueError, match=match):
            discover_params(query, limit)


def test_header_binding_and_docs_name_the_calls():
    from ragmi import _lib
    from ragmi import index as I
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("rag_index_discover", 15), ("rag_index_discover_bounds", 10),
                         ("rag_index_discover_stats", 2)):
        assert re.search(r"^int %s\(rag_index_t\* index," % name, code, re.M)
        assert len(_lib.INDEX_API[name][1]) == n_args
    for line in ("#define RAG_DISCOVER_MAX_PAIRS 15", "#define RAG_CONTEXT_MAX_PAIRS 16"):
        assert re.search("^%s$" % line, code, re.M)
    assert (I.DISCOVER_MAX_PAIRS, I.CONTEXT_MAX_PAIRS) == (15, 16)
    flat = " ".join(hdr.split())
    assert "Discovery queries" in hdr
    assert flat.count("parity with a Qdrant server's own arithmetic is unpinned") >= 2
    doc = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    assert "rag_index_discover" in doc and "DiscoverQuery" in doc and "ContextQuery" in doc
    assert "discover over a shard set is not built" in doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "R20" in design and "rag_index_discover" in design


# ------------------------------------------------------------------ 3. argument refusals
def test_discover_argument_errors_need_no_device():
    from ragmi import _build, _lib
    _build.build()
    L = _lib.load()
    buf = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(buf)

    def call(n, k, target=p, pos=p, neg=p, progs=None, words=0, U=0, flags=0, out=p, h=None):
        return L.rag_index_discover(h, target, pos, neg, n, k, progs, words, U, None, 0, flags,
                                    out, out, None)

    err = L.rag_last_error
    assert call(16, 5) != 0 and b"RAG_DISCOVER_MAX_PAIRS=15" in err()
    assert call(17, 5, target=None) != 0 and b"RAG_CONTEXT_MAX_PAIRS=16" in err()
    assert call(-1, 5) != 0 and call(-1, 5, target=None) != 0
    assert call(0, 5, target=None) != 0 and b"needs a pair" in err()
    assert call(1, 5, pos=None) != 0 and b"NULL pair" in err()
    assert call(1, 5, neg=None) != 0 and b"NULL pair" in err()
    assert call(2, 5, target=None, neg=None) != 0 and b"NULL pair" in err()
    assert call(1, 0) != 0 and b"k must be >= 1" in err()
    assert call(1, 5, out=None) != 0 and b"NULL output" in err()
    assert call(1, 5, flags=2) != 0 and b"unknown flags" in err()
    assert call(1, 5, progs=p, words=41, U=0) != 0 and b"n_programs" in err()
    assert call(1, 5, progs=p, words=3, U=1) != 0 and b"words" in err()
    assert call(1, 5, words=41, U=1) != 0 and b"programs is NULL" in err()
    # every argument in order: what is left is the missing index
    assert call(15, 5) != 0 and b"index is NULL" in err()
    assert call(16, 5, target=None) != 0 and b"index is NULL" in err()
    assert call(0, 5, pos=None, neg=None) != 0 and b"index is NULL" in err()   # n = 0: no pairs

    def bounds(n, rows_n, target=p, rows=p, out=p):
        return L.rag_index_discover_bounds(None, target, p, p, n, rows, rows_n, out, out, None)

    assert bounds(16, 1) != 0 and b"RAG_DISCOVER_MAX_PAIRS=15" in err()
    assert bounds(0, 1, target=None) != 0 and b"needs a pair" in err()
    assert bounds(1, 1, rows=None) != 0 and b"NULL" in err()
    assert bounds(1, 1) != 0 and b"index is NULL" in err()
    assert L.rag_index_discover_stats(None, buf) != 0


# ------------------------------------------------------------------ 4. QdrantClient routing
class _StubIndex:
    """FlatIndex stand-in: discover records what it was asked and returns rows 0..k-1 with
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

    def discover(self, target, pos, neg, k, filters=None, programs=None, rescue=False):
        import torch
        arr = lambda t: None if t is None else np.asarray(t).tolist()  # noqa: E731
        self.calls.append(("discover", arr(target), arr(pos), arr(neg), k, filters,
                           programs is not None, rescue))
        return torch.linspace(0.9, 0.1, k), torch.arange(k, dtype=torch.int64)


def stub_client(count=40):
    return S.stub_client(S.stub_collection(
        _StubIndex(count), dim=4, ids=range(100, 100 + count),
        payloads=[{"ticker": "AMD" if r % 2 else "AAPL", "n": r} for r in range(count)]))


def _dq(target, *pairs):
    from ragmi import qdrant_models as m
    return m.DiscoverQuery(m.DiscoverInput(target, [m.ContextPair(p, n) for p, n in pairs]))


def _cq(*pairs):
    from ragmi import qdrant_models as m
    return m.ContextQuery([m.ContextPair(p, n) for p, n in pairs])


def test_discover_route_resolves_ids_and_drops_the_examples():
    from ragmi import qdrant_models as m
    client, col = stub_client()
    v = [0.0, 1.0, 0.0, 0.0]
    amd = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    r = client.query_points("t", _dq(v, (101, 103), (v, 102)), limit=5, query_filter=amd)
    assert col.coalescer.requests == 0 and col.coalescer.batches == 0
    # ids 101, 103, 102 are rows 1, 3, 2: gathered once, then limit + 3 hits asked for, under rescue
    assert col.index.calls == [
        ("gather_rows", [1, 3, 2]),
        ("discover", v, [[1.0, 0, 0, 0], v], [[3.0, 0, 0, 0], [2.0, 0, 0, 0]], 8, (0xFFFF, 2),
         False, True)]
    assert [p.id for p in r.points] == [100, 104, 105, 106, 107]   # rows 1, 2, 3 dropped, cut to 5
    assert r.points[0].payload == {"ticker": "AAPL", "n": 0}
    col.index.calls.clear()
    # a target by id, no pairs; the legacy spelling
    pts = client.discover("t", target=104, limit=3, with_payload=False)
    assert col.index.calls == [("gather_rows", [4]),
                               ("discover", [4.0, 0, 0, 0], None, None, 4, None, False, True)]
    assert [p.id for p in pts] == [100, 101, 102] and pts[0].payload is None
    col.index.calls.clear()
    # no target: a context query; one pair as ContextQuery takes it; k <= count
    pts = client.discover("t", context=m.ContextPair(positive=v, negative=101), limit=50)
    assert col.index.calls == [("gather_rows", [1]),
                               ("discover", None, [v], [[1.0, 0, 0, 0]], 40, None, False, True)]
    assert len(pts) == 39 and 101 not in [p.id for p in pts]
    col.index.calls.clear()
    pts = client.query_points("t", _cq((v, v)), limit=2).points
    assert col.index.calls == [("discover", None, [v], [v], 2, None, False, True)]
    assert [p.id for p in pts] == [100, 101]


def test_discover_route_refusals_and_empty_answers():
    from ragmi import qdrant_models as m
    client, col = stub_client()
    v = [0.0, 1.0, 0.0, 0.0]
    sp = m.SparseVector(indices=[1], values=[1.0])
    with pytest.raises(ValueError, match="discover: example point 999 is not in collection"):
        client.query_points("t", _dq(999), limit=5)
    for q in (_dq(v, (101, 102)), _cq((101, 102))):
        name = type(q).__name__
        with pytest.raises(ValueError, match=f"{name} over prefetched candidates"):
            client.query_points("t", q, limit=5, prefetch=[m.Prefetch(query=v)])
        with pytest.raises(ValueError, match=f"{name} inside a Prefetch is not built"):
            client.query_points("t", m.FusionQuery(m.Fusion.RRF), limit=5,
                                prefetch=[m.Prefetch(query=q)])
        with pytest.raises(ValueError, match=f"grouped query cannot be a {name}"):
            client.query_points_groups("t", q, group_by="ticker")
        with pytest.raises(ValueError, match=f"{name} with using"):
            client.query_points("t", q, limit=5, using="title")
        with pytest.raises(ValueError, match=f"{name} with lookup_from"):
            client.query_points("t", q, limit=5, lookup_from="other")
        with pytest.raises(ValueError, match="int limit"):
            client.query_points("t", q, limit=None)
    with pytest.raises(ValueError, match="lookup_from"):
        client.discover("t", target=101, lookup_from="other")
    with pytest.raises(ValueError, match="SparseVector examples is not built"):
        client.discover("t", target=sp)
    with pytest.raises(ValueError, match="SparseVector examples is not built"):
        client.discover("t", context=[m.ContextPair(101, sp)])
    with pytest.raises(ValueError, match="at most 15 context pairs"):
        client.discover("t", target=v, context=[m.ContextPair(101, 102)] * 16)
    with pytest.raises(ValueError, match="at most 16 context pairs"):
        client.discover("t", context=[m.ContextPair(101, 102)] * 17)
    with pytest.raises(ValueError, match="ContextQuery without pairs is not built"):
        client.discover("t")
    with pytest.raises(ValueError, match="ContextQuery without pairs is not built"):
        client.query_points("t", m.ContextQuery(context=[]), limit=5)
    assert col.index.calls == []                               # refused before any index call
    never = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="NONE"))])
    assert client.query_points("t", _dq(101), limit=5, query_filter=never).points == []
    assert client.query_points("t", _cq((101, v)), limit=0).points == []
    assert col.index.calls == []                               # ... and no launch for these
    empty, ecol = stub_client(count=0)
    assert empty.query_points("t", _dq(v), limit=5).points == []
    assert ecol.index.calls == []


def test_mixed_batch_routes_discover_one_pass_each_in_order():
    from ragmi import qdrant_models as m
    client, col = stub_client()
    v = [0.0, 1.0, 0.0, 0.0]
    reqs = [m.QueryRequest(query=v, limit=7),
            m.QueryRequest(query=_dq(v, (105, v)), limit=2),
            m.QueryRequest(query=v, limit=3, with_payload=False),
            m.QueryRequest(query=_cq((v, 106), (v, v)), limit=4, with_payload=False)]
    out = client.query_batch_points("t", reqs)
    assert [len(r.points) for r in out] == [7, 2, 3, 4]
    disc = [c for c in col.index.calls if c[0] == "discover"]
    # one pass each, in request order: (has a target, pairs, k)
    assert [(c[1] is not None, len(c[2]), c[4]) for c in disc] == [(True, 1, 3), (False, 2, 5)]
    assert [c for c in col.index.calls if c[0] == "search"] == [("search", 2, 7, None)]
    assert col.coalescer.requests == 0
    assert out[3].points[0].payload is None and out[1].points[0].payload is not None
    assert 105 not in [p.id for p in out[1].points] and 106 not in [p.id for p in out[3].points]


def test_shard_set_collection_refuses():
    from ragmi.collection import Collection
    from ragmi.shardset import ShardSet
    assert not hasattr(ShardSet, "discover")                   # how a Collection tells

    class StubSet:
        device, storage, count = None, "fp32", 4

    col = Collection("t", 4, None, index=StubSet())
    with pytest.raises(NotImplementedError, match="discover over a shard set is not built"):
        col.search_discover([([0.0, 1.0, 0.0, 0.0], [], (0, 0), 5)])


def test_flat_index_refuses_bad_sides_before_the_library():
    """FlatIndex._discover_sides is host logic over tensors: run it on the CPU device."""
    import torch
    from ragmi.index import FlatIndex
    idx = FlatIndex.__new__(FlatIndex)
    idx.device, idx.dim = torch.device("cpu"), 4
    v = np.zeros((1, 4), np.float32)
    t, p, n, P = idx._discover_sides(v[0], np.repeat(v, 3, 0), np.repeat(v, 3, 0))
    assert t.shape == (4,) and p.shape == (3, 4) and n.shape == (3, 4) and P == 3
    assert idx._discover_sides(v[0], None, None)[1:] == (None, None, 0)
    for args, match in (((v[0], np.repeat(v, 2, 0), v), "2 positives and 1 negatives"),
                        ((v[0], np.repeat(v, 16, 0), np.repeat(v, 16, 0)), "at most 15"),
                        ((None, np.repeat(v, 17, 0), np.repeat(v, 17, 0)), "at most 16"),
                        ((None, None, None), "needs at least one pair"),
                        ((np.zeros(5, np.float32), None, None), "target must be"),
                        ((v[0], np.zeros((1, 5), np.float32), v), "must be")):
        with pytest.raises(ValueError, match=match):
            idx._discover_sides(*args)


def test_rag_retrieve_steered(monkeypatch):
    from ragmi import qdrant_models as m
    from ragmi import rag
    seen = []

    class Fake:
        def query_points(self, **kw):
            seen.append(kw)
            return m.QueryResponse()

    monkeypatch.setattr(rag, "_testing", lambda: False)
    monkeypatch.setattr(rag, "get_qdrant", lambda: Fake())
    qv = [0.1, 0.2]
    rag.retrieve_steered(qv, [("a" * 32, "b" * 32), ("c" * 32, "d" * 32)], ticker="amd", limit=4)
    assert seen[-1]["query"] == m.DiscoverQuery(m.DiscoverInput(
        qv, [m.ContextPair("a" * 32, "b" * 32), m.ContextPair("c" * 32, "d" * 32)]))
    assert seen[-1]["limit"] == 4
    assert seen[-1]["query_filter"] == m.Filter(must=[m.FieldCondition(
        key="ticker", match=m.MatchValue(value="AMD"))])
    rag.retrieve_steered(qv, [])
    assert seen[-1]["query_filter"] is None and seen[-1]["limit"] == rag.RETRIEVE_LIMIT
    assert seen[-1]["query"].discover.context == []

    class Broken:
        def query_points(self, **kw):
            raise RuntimeError("down")

    monkeypatch.setattr(rag, "get_qdrant", lambda: Broken())
    assert rag.retrieve_steered(qv, [(1, 2)]).points == []
