"""CPU tests of MMR search: the Mmr / NearestQuery models and their defaults, the numpy
restatement's own properties on the seed-7 corpus of near-duplicate groups, rag_index_mmr's
argument refusals (no device), and QdrantClient's routing of MMR requests over a stand-in
index."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import _mmr_ref as R
import _stubs as S


# ------------------------------------------------------------------ 1. models and defaults
def test_models_and_defaults():
    from ragmi import qdrant_models as m
    from ragmi.index import MMR_MAX_CANDIDATES
    from ragmi.qdrant import mmr_params, nearest_of
    assert m.Mmr() == m.Mmr(diversity=None, candidates_limit=None)
    assert m.NearestQuery(nearest=[1.0]).mmr is None
    v = [0.0, 1.0]
    assert nearest_of(v) == (v, None)
    assert nearest_of(m.NearestQuery(nearest=v)) == (v, None)
    mm = m.Mmr(diversity=0.25, candidates_limit=40)
    assert nearest_of(m.NearestQuery(nearest=v, mmr=mm)) == (v, mm)
    assert MMR_MAX_CANDIDATES == 1024
    assert mmr_params(m.Mmr(), 10) == (0.5, 100)              # diversity 0.5, max(limit, 100)
    assert mmr_params(m.Mmr(), 250) == (0.5, 250)
    assert mmr_params(m.Mmr(0.0, 7), 10) == (0.0, 7)
    assert mmr_params(m.Mmr(1.0, 1024), np.int64(3)) == (1.0, 1024)
    for bad in (m.Mmr(diversity=-0.01), m.Mmr(diversity=1.5), m.Mmr(diversity=float("nan")),
                m.Mmr(candidates_limit=0), m.Mmr(candidates_limit=2.5)):
        with pytest.raises(ValueError):
            mmr_params(bad, 10)
    with pytest.raises(ValueError, match="1024"):
        mmr_params(m.Mmr(candidates_limit=1025), 10)
    with pytest.raises(ValueError, match="1024"):
        mmr_params(m.Mmr(), 2000)                             # the default would pass the cap
    for limit in (None, 2.0, "3", True):
        with pytest.raises(ValueError, match="int limit"):
            mmr_params(m.Mmr(), limit)


def test_header_binding_and_docs_name_the_call():
    from ragmi import _lib
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"^int rag_index_mmr\(rag_index_t\* index,", code, re.M)
    assert re.search(r"^#define RAG_MMR_MAX_CANDIDATES 1024$", code, re.M)
    assert len(_lib.INDEX_API["rag_index_mmr"][1]) == 12
    assert "rag_index_mmr" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "candidates_limit" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ------------------------------------------------------------------ 2. the restatement itself
@pytest.fixture(scope="module")
def seed7():
    x, q, group = R.grouped_corpus(384)
    return R.encode(x, "fp16"), q, group


def test_corpus_layout():
    x, q, group = R.grouped_corpus(384)
    assert x.shape == (3001, 384) and x.dtype == np.float32 and q.shape == (384,)
    assert 3001 % 16 != 0
    for g in range(12):
        rows = np.nonzero(group == g)[0]
        assert len(rows) == 9
        same = [r for r in rows if sum(np.array_equal(x[r], x[o]) for o in rows) == 4]
        assert len(same) == 4                                  # 4 identical, 5 noisy
    assert (group == -1).sum() == 2893


def test_ref_diversity_zero_is_the_top_k(seed7):
    enc, q, _ = seed7
    s, r, p, cs, cr = R.search_mmr(enc, q[None], 12, 0.0, 100)
    assert np.array_equal(r, cr[:, :12]) and np.array_equal(s.view(np.uint32),
                                                            cs[:, :12].view(np.uint32))
    assert p.tolist() == [list(range(12))]


def test_ref_prefix_property(seed7):
    enc, q, _ = seed7
    for div in (0.3, 0.5, 1.0):
        s12, r12, p12, _, _ = R.search_mmr(enc, q[None], 12, div, 100)
        s5, r5, p5, _, _ = R.search_mmr(enc, q[None], 5, div, 100)
        assert np.array_equal(r12[:, :5], r5) and np.array_equal(s12[:, :5], s5)
        assert np.array_equal(p12[:, :5], p5)


def test_ref_mmr_spreads_over_the_groups(seed7):
    enc, q, group = seed7
    stats = {}
    _, r, _, _, cr = R.search_mmr(enc, np.stack([q, q]), 12, [0.0, 0.5], 100, stats=stats)
    assert len(set(group[r[0]].tolist())) == 2                 # plain top-12: two groups
    assert sorted(group[r[1]].tolist()) == list(range(12))     # MMR at 0.5: all twelve
    assert stats["ties"] > 0                                   # identical rows tie exactly


def test_ref_similarity_is_symmetric_and_padding(seed7):
    import oracle_scan as O
    enc, q, _ = seed7
    _, cr = O.search(enc, q[None], 20)
    rows = cr[0]
    sim = np.stack([O.rescore(enc, R.stored_f32(enc, r)[None], rows[None])[0] for r in rows])
    assert np.array_equal(sim.view(np.uint32), sim.T.view(np.uint32))
    cs = np.linspace(0.9, 0.5, 20, dtype=np.float32)[None]
    s, r, p = R.mmr(enc, cs, cr, 6, 0.5, ncand=[4])
    assert (r[0, 4:] == -1).all() and np.isneginf(s[0, 4:]).all() and (p[0, 4:] == -1).all()
    assert sorted(p[0, :4].tolist()) == [0, 1, 2, 3]
    broken = cr.copy()
    broken[0, 2] = -1                                          # the list ends at its first -1
    assert R.mmr(enc, cs, broken, 6, 0.5)[2][0].tolist()[2:] == [-1] * 4


# ------------------------------------------------------------------ 3. argument refusals
def test_mmr_argument_errors_need_no_device():
    from ragmi import _build, _lib
    _build.build()
    L = _lib.load()
    buf = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(buf)

    def call(h, B, C, k, ptr=p):
        return L.rag_index_mmr(h, ptr, ptr, B, C, k, ptr, None, ptr, ptr, None, None)

    assert call(None, 1, 0, 1) != 0 and b"RAG_MMR_MAX_CANDIDATES" in L.rag_last_error()
    assert call(None, 1, 1025, 1) != 0 and b"1024" in L.rag_last_error()
    assert call(None, 1, -3, 1) != 0
    assert call(None, 1, 8, 0) != 0 and b"k must be" in L.rag_last_error()
    assert call(None, -1, 8, 1) != 0 and b"B must be" in L.rag_last_error()
    assert call(None, 1, 8, 1) != 0 and b"NULL" in L.rag_last_error()
    assert call(None, 1, 8, 1, None) != 0 and b"NULL" in L.rag_last_error()


# ------------------------------------------------------------------ 4. QdrantClient routing
class _StubIndex:
    """FlatIndex stand-in: search returns rows 0..k-1 with falling scores, mmr records what it
    was asked and returns the first k candidates."""
    device = None

    def __init__(self, count):
        self.count = count
        self.calls = []

    def search(self, q, k, filters=None, full=False, rescue=False):
        import torch
        B = len(q)
        self.calls.append(("search", B, k, None if filters is None else filters.tolist()))
        ids = torch.arange(k, dtype=torch.int64).repeat(B, 1)
        s = torch.linspace(0.9, 0.1, k).repeat(B, 1)
        return s, ids

    def unanswered(self):
        return 0

    def mmr(self, s, ids, k, diversity, ncand):
        self.calls.append(("mmr", tuple(s.shape), k, np.asarray(diversity).tolist(),
                           np.asarray(ncand).tolist()))
        return s[:, :k].clone(), ids[:, :k].clone()


def stub_client(count=40):
    return S.stub_client(S.stub_collection(
        _StubIndex(count), dim=4, ids=range(100, 100 + count),
        payloads=[{"ticker": "AMD" if r % 2 else "AAPL", "n": r} for r in range(count)]))


def test_nearest_query_without_mmr_is_the_plain_path():
    from ragmi import qdrant_models as m
    client, col = stub_client()
    v = [0.0, 1.0, 0.0, 0.0]
    plain = client.query_points("t", v, limit=5)
    assert col.coalescer.requests == 1
    same = client.query_points("t", m.NearestQuery(nearest=v), limit=5)
    assert col.coalescer.requests == 2                         # rode the coalescer too
    assert [p.id for p in same.points] == [p.id for p in plain.points] == [100, 101, 102, 103, 104]
    assert col.index.calls == [("search", 1, 5, None)] * 2     # no mmr call
    out = client.query_batch_points("t", [m.QueryRequest(query=m.NearestQuery(nearest=v), limit=3),
                                          m.QueryRequest(query=v, limit=2)])
    assert [len(r.points) for r in out] == [3, 2]
    assert col.index.calls[-1] == ("search", 2, 3, None)


def test_mmr_query_bypasses_the_coalescer_and_clamps():
    from ragmi import qdrant_models as m
    client, col = stub_client(count=40)
    v = [0.0, 1.0, 0.0, 0.0]
    amd = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    r = client.query_points("t", m.NearestQuery(nearest=v, mmr=m.Mmr()), limit=10,
                            query_filter=amd)
    assert col.coalescer.requests == 0 and col.coalescer.batches == 0
    # default candidates max(10, 100) = 100, clamped to the 40 points; default diversity 0.5
    assert col.index.calls == [("search", 1, 40, [[0xFFFF, 2]]),
                               ("mmr", (1, 40), 10, [0.5], [40])]
    assert [p.id for p in r.points] == list(range(100, 110))
    assert r.points[0].payload == {"ticker": "AAPL", "n": 0}
    assert r.points[0].score == pytest.approx(0.9)
    col.index.calls.clear()
    r = client.query_points("t", m.NearestQuery(nearest=v, mmr=m.Mmr(0.25, 6)), limit=10,
                            with_payload=False)
    assert col.index.calls == [("search", 1, 6, None), ("mmr", (1, 6), 6, [0.25], [6])]
    assert len(r.points) == 6 and r.points[0].payload is None
    with pytest.raises(ValueError, match="1024"):
        client.query_points("t", m.NearestQuery(nearest=v, mmr=m.Mmr(0.5, 4096)), limit=10)
    with pytest.raises(ValueError):
        client.query_points("t", m.NearestQuery(nearest=v, mmr=m.Mmr(1.5)), limit=10)
    with pytest.raises(ValueError):
        client.query_points("t", m.NearestQuery(nearest=v, mmr=m.Mmr()), limit=None)
    assert client.query_points("t", m.NearestQuery(nearest=v, mmr=m.Mmr()), limit=0).points == []
    never = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="NONE"))])
    assert client.query_points("t", m.NearestQuery(nearest=v, mmr=m.Mmr()), limit=5,
                               query_filter=never).points == []
    assert col.coalescer.requests == 0


def test_mixed_batch_is_one_search_and_one_mmr_launch():
    from ragmi import qdrant_models as m
    client, col = stub_client(count=40)
    v = [0.0, 1.0, 0.0, 0.0]
    amd = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    never = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="NONE"))])
    reqs = [m.QueryRequest(query=v, limit=7),                                          # plain
            m.QueryRequest(query=m.NearestQuery(nearest=v, mmr=m.Mmr(0.5, 30)), limit=10,
                           filter=amd),
            m.QueryRequest(query=m.NearestQuery(nearest=v, mmr=m.Mmr(0.75)), limit=3),  # 100 -> 40
            m.QueryRequest(query=m.NearestQuery(nearest=v, mmr=m.Mmr()), limit=4, filter=never),
            m.QueryRequest(query=m.NearestQuery(nearest=v), limit=2, with_payload=False)]
    out = client.query_batch_points("t", reqs)
    # the request whose filter can match nothing takes no part; C = the batch maximum; plain
    # requests ride at diversity 0 with their own limit as candidate count
    assert col.index.calls == [
        ("search", 4, 40, [[0, 0], [0xFFFF, 2], [0, 0], [0, 0]]),
        ("mmr", (4, 40), 10, [0.0, 0.5, 0.75, 0.0], [7, 30, 40, 2])]
    assert [len(r.points) for r in out] == [7, 10, 3, 0, 2]
    assert out[4].points[0].payload is None and out[0].points[0].payload is not None
    assert col.coalescer.requests == 0
    # a plain limit past the cap cannot ride: the plain requests are searched on their own
    col.index.calls.clear()
    col.index.count = 5000
    col.row_ids = list(range(5000))
    col.payloads = [None] * 5000
    col.versions = [1] * 5000
    out = client.query_batch_points("t", [m.QueryRequest(query=v, limit=2000), reqs[1]])
    assert [c[:3] for c in col.index.calls] == [("search", 1, 2000), ("search", 1, 30),
                                                ("mmr", (1, 30), 10)]
    assert [len(r.points) for r in out] == [2000, 10]


def test_rag_retrieval_keywords(monkeypatch):
    from ragmi import qdrant_models as m
    from ragmi import rag
    seen = []

    class Fake:
        def query_points(self, **kw):
            seen.append(kw)
            return m.QueryResponse()

        def query_batch_points(self, name, reqs):
            seen.append(reqs)
            return [m.QueryResponse() for _ in reqs]

    monkeypatch.setattr(rag, "_testing", lambda: False)
    monkeypatch.setattr(rag, "get_qdrant", lambda: Fake())
    v = [0.0] * 384
    rag.retrieve_from_qdrant(v, "amd")
    assert seen[-1]["query"] is v                               # today's call exactly
    rag.retrieve_from_qdrant(v, "amd", limit=15, diversity=0.4)
    assert seen[-1]["query"] == m.NearestQuery(nearest=v, mmr=m.Mmr(0.4, None))
    rag.retrieve_from_qdrant(v, "amd", candidates=64)
    assert seen[-1]["query"] == m.NearestQuery(nearest=v, mmr=m.Mmr(None, 64))
    rag.retrieve_batch([v, v], ["amd", "aapl"])
    assert all(r.query is v for r in seen[-1])
    rag.retrieve_batch([v, v], ["amd", "aapl"], diversity=0.5, candidates=100)
    assert all(r.query == m.NearestQuery(nearest=v, mmr=m.Mmr(0.5, 100)) for r in seen[-1])
    with pytest.raises(TypeError):
        rag.retrieve_from_qdrant(v, "amd", None, 15, 0.5)       # keyword-only
