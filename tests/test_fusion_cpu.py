"""CPU tests of fusion queries: the Qdrant models, fusion_params' acceptances and refusals (each
message names its cause), rag_fuse_rrf's argument refusals through ctypes (no device), the
restatement's properties (tests/_fusion_ref.py), and the client's routing checks that need no
search."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

import _fusion_ref as F

RAG_EINVAL, RAG_ERANGE = -1, -4
V = [0.0, 1.0, 0.0, 0.0]


# ------------------------------------------------------------------ 1. models
def test_models_construct():
    from ragmi import qdrant_models as m
    assert m.Fusion.RRF.value == "rrf" and m.Fusion.DBSF.value == "dbsf"
    assert m.FusionQuery(fusion=m.Fusion.RRF).fusion is m.Fusion.RRF
    assert m.Rrf().k is None and m.Rrf(k=60).k == 60
    assert m.RrfQuery(rrf=m.Rrf(k=60)).rrf.k == 60
    p = m.Prefetch(query=V)
    assert (p.query, p.filter, p.limit, p.prefetch) == (V, None, 10, None)
    f = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    assert m.Prefetch(query=V, filter=f, limit=50).filter is f
    r = m.QueryRequest(query=V)
    assert r.prefetch is None and (r.filter, r.limit, r.with_payload) == (None, 10, True)
    r = m.QueryRequest(query=m.FusionQuery(fusion=m.Fusion.RRF), prefetch=[p], limit=3)
    assert r.prefetch == [p]


# ------------------------------------------------------------------ 2. fusion_params
def test_fusion_params_accepts():
    from ragmi import qdrant_models as m
    from ragmi.index import FUSION_MAX_ENTRIES, FUSION_MAX_LISTS
    from ragmi.qdrant import fusion_params, is_fusion
    assert (FUSION_MAX_LISTS, FUSION_MAX_ENTRIES) == (16, 4096)
    rrf = m.FusionQuery(fusion=m.Fusion.RRF)
    f = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    w = [1.0, 0.0, 0.0, 0.0]
    k, pres = fusion_params(rrf, [m.Prefetch(query=V, limit=50, filter=f),
                                  m.Prefetch(query=m.NearestQuery(nearest=w), limit=7)], 15)
    assert k == 2 and pres == [(V, f, 50), (w, None, 7)]
    # a single Prefetch is a list of one; "rrf" the string is the enum's value
    assert fusion_params(m.FusionQuery(fusion="rrf"), m.Prefetch(query=V), 15) == \
        (2, [(V, None, 10)])
    assert fusion_params(m.RrfQuery(rrf=m.Rrf(k=60)), [m.Prefetch(query=V)], 1)[0] == 60
    assert fusion_params(m.RrfQuery(rrf=m.Rrf()), [m.Prefetch(query=V)], 1)[0] == 2
    assert fusion_params(rrf, [m.Prefetch(query=V)] * 16, np.int64(5))[0] == 2
    assert fusion_params(rrf, [m.Prefetch(query=V, limit=0)], 0)[1] == [(V, None, 0)]
    assert is_fusion(rrf) and is_fusion(m.RrfQuery(rrf=m.Rrf())) and not is_fusion(V)
    assert not is_fusion(m.NearestQuery(nearest=V))


def test_fusion_params_refuses_and_names_the_cause():
    from ragmi import qdrant_models as m
    from ragmi.qdrant import fusion_params
    rrf = m.FusionQuery(fusion=m.Fusion.RRF)
    one = [m.Prefetch(query=V)]
    f = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    cases = (
        ((m.FusionQuery(fusion=m.Fusion.DBSF), one, 5), "DBSF"),
        ((rrf, None, 5), "needs prefetches"),
        ((rrf, [], 5), "needs prefetches"),
        ((V, one, 5), "re-scoring prefetched candidates"),
        ((m.NearestQuery(nearest=V), one, 5), "re-scoring prefetched candidates"),
        ((None, one, 5), "re-scoring prefetched candidates"),
        ((rrf, [m.Prefetch(query=V, prefetch=m.Prefetch(query=V))], 5), "nested"),
        ((rrf, [m.Prefetch(query=V), m.Prefetch()], 5), r"prefetch\[1\] needs a query"),
        ((rrf, [m.Prefetch(query=m.NearestQuery(nearest=V, mmr=m.Mmr()))], 5), "MMR"),
        ((rrf, [m.Prefetch(query=V)] * 17, 5), "at most 16"),
        ((m.RrfQuery(rrf=m.Rrf(k=0)), one, 5), "Rrf.k"),
        ((m.RrfQuery(rrf=m.Rrf(k=2.0)), one, 5), "Rrf.k"),
        ((m.RrfQuery(rrf=m.Rrf(k=True)), one, 5), "Rrf.k"),
        ((rrf, one, 5.0), "int limit"),
        ((rrf, one, None), "int limit"),
        ((rrf, [m.Prefetch(query=V, limit="3")], 5), r"prefetch\[0\] needs an int limit"),
        ((rrf, [V], 5), "not a Prefetch"),
    )
    for args, word in cases:
        with pytest.raises(ValueError, match=word):
            fusion_params(*args)
    with pytest.raises(ValueError, match="belongs on each Prefetch"):
        fusion_params(rrf, one, 5, f)


# ------------------------------------------------------------------ 3. argument refusals
def test_argument_errors_need_no_device():
    from ragmi import _build, _lib
    _build.build()
    L = _lib.load()
    assert len(_lib.INDEX_API["rag_fuse_rrf"][1]) == 11
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)

    def call(B=1, L_=2, C=4, k=3, rrf_k=2, rows=p, out_s=p, out_r=p):
        return L.rag_fuse_rrf(rows, None, B, L_, C, k, rrf_k, out_s, out_r, None, None)

    for kw, code, word in (({"L_": 0}, RAG_ERANGE, b"L must be"), ({"L_": 17}, RAG_ERANGE, b"16"),
                           ({"L_": -1}, RAG_ERANGE, b"L must be"),
                           ({"C": 0}, RAG_ERANGE, b"C must be"),
                           ({"L_": 1, "C": 4097}, RAG_ERANGE, b"L * C"),
                           ({"L_": 16, "C": 257}, RAG_ERANGE, b"4096"),
                           ({"L_": 16, "C": 1 << 30}, RAG_ERANGE, b"L * C"),
                           ({"k": 0}, RAG_EINVAL, b"k must be"),
                           ({"rrf_k": 0}, RAG_EINVAL, b"rrf_k must be"),
                           ({"B": -1}, RAG_EINVAL, b"B must be"),
                           ({"rows": None}, RAG_EINVAL, b"NULL"),
                           ({"out_s": None}, RAG_EINVAL, b"NULL"),
                           ({"out_r": None}, RAG_EINVAL, b"NULL")):
        assert call(**kw) == code and word in L.rag_last_error(), kw
    assert call(B=0, rows=None, out_s=None, out_r=None) == 0               # launches nothing
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    for line in ("#define RAG_FUSION_MAX_LISTS 16", "#define RAG_FUSION_MAX_ENTRIES 4096",
                 "int rag_fuse_rrf("):
        assert line in hdr
    assert "rag_fuse_rrf" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_fuse_rrf_checks_before_any_launch():
    import torch
    from ragmi.index import fuse_rrf
    rows = torch.zeros((1, 2, 4), dtype=torch.int64)
    for bad, kw in ((rows.to(torch.int32), {}), (rows[0], {}), (rows, {"k": 0}),
                    (rows, {"rrf_k": 0}), (torch.zeros((1, 17, 1), dtype=torch.int64), {}),
                    (torch.zeros((1, 16, 257), dtype=torch.int64), {}),
                    (torch.zeros((1, 2, 0), dtype=torch.int64), {}),
                    (rows, {"ncand": np.zeros((2, 2))})):
        with pytest.raises(ValueError):
            fuse_rrf(bad, **{"k": 3, **kw})


# ------------------------------------------------------------------ 4. the restatement
def test_one_list_is_returned_unchanged():
    rng = np.random.default_rng(0)
    rows = rng.permutation(1000)[:40].reshape(2, 1, 20).astype(np.int64) + (1 << 40)
    for rrf_k in (1, 2, 60):
        s, r, count = F.rrf(rows, None, 25, rrf_k)
        assert np.array_equal(r[:, :20], rows[:, 0]) and (r[:, 20:] == -1).all()
        want = np.array([np.float32(1.0 / (rrf_k + p)) for p in range(20)], np.float32)
        assert np.array_equal(F.bits(s[:, :20]), F.bits(np.stack([want, want])))
        assert np.isneginf(s[:, 20:]).all() and count.tolist() == [20, 20]


def test_two_rows_tie_and_the_smaller_row_leads():
    # rrf_k = 2: A at (list 0 pos 0, list 1 pos 1), B at (list 0 pos 1, list 1 pos 0)
    for a, b in ((7, 9), (9, 7)):
        s, r, count = F.rrf(np.array([[[a, b, 5], [b, a, -1]]]), None, 6)
        assert r[0].tolist() == [min(a, b), max(a, b), 5, -1, -1, -1] and count[0] == 3
        assert F.bits(s[0, :1]) == F.bits(s[0, 1:2]) == F.bits(np.float32(1 / 2 + 1 / 3))
        assert s[0, 2] == np.float32(0.25)


def test_prefix_property_and_lengths():
    rng = np.random.default_rng(1)
    rows = rng.integers(0, 60, (4, 3, 30)).astype(np.int64)
    rows[1, 2, 11] = -1
    ncand = np.array([[30, 30, 30], [30, 7, 30], [0, 0, 0], [40, -2, 1]])
    assert F.list_lengths(rows, ncand).tolist() == [[30, 30, 30], [30, 7, 11], [0, 0, 0],
                                                     [30, 0, 1]]
    full = F.rrf(rows, ncand, 90)
    assert full[2][2] == 0 and (full[1][2] == -1).all() and np.isneginf(full[0][2]).all()
    for k in (1, 5, 33):
        s, r, count = F.rrf(rows, ncand, k)
        assert np.array_equal(r, full[1][:, :k]) and np.array_equal(count, full[2])
        assert np.array_equal(F.bits(s), F.bits(full[0][:, :k]))
    for b in range(4):
        live = full[0][b, :full[2][b]]
        assert (np.diff(live) <= 0).all()
        assert len(set(full[1][b, :full[2][b]].tolist())) == full[2][b]


def test_a_row_twice_in_one_list_counts_twice():
    s, r, count = F.rrf(np.array([[[4, 8, 4]]]), None, 3)
    assert r[0].tolist() == [4, 8, -1] and count[0] == 2
    assert F.bits(s[0, 0]) == F.bits(np.float32(1.0 / 2 + 1.0 / 4))
    assert F.bits(s[0, 1]) == F.bits(np.float32(1.0 / 3))


def test_corpus_gives_overlap_and_a_tie():
    x, Q, tickers = F.fusion_corpus()                  # asserts its own properties
    assert x.shape == (F.N_ROWS, F.DIM) and Q.shape == (3, F.DIM) and set(tickers) == set(F.TICKERS)


# ------------------------------------------------------------------ 5. routing, no search
def test_client_refusals_and_rag_arguments(monkeypatch):
    from test_groups_cpu import stub_client
    from ragmi import qdrant_models as m
    from ragmi import rag
    client, col = stub_client()
    rrf = m.FusionQuery(fusion=m.Fusion.RRF)
    one = [m.Prefetch(query=V)]
    f = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    with pytest.raises(ValueError, match="belongs on each Prefetch"):
        client.query_points("t", rrf, prefetch=one, query_filter=f)
    with pytest.raises(ValueError, match="re-scoring"):
        client.query_points("t", V, prefetch=one)
    with pytest.raises(ValueError, match="needs prefetches"):
        client.query_points("t", rrf)
    with pytest.raises(ValueError, match="DBSF"):
        client.query_batch_points("t", [m.QueryRequest(query=V), m.QueryRequest(
            query=m.FusionQuery(fusion=m.Fusion.DBSF), prefetch=one)])
    with pytest.raises(ValueError, match="grouped query over prefetched"):
        client.query_points_groups("t", rrf, group_by="ticker", prefetch=one)
    with pytest.raises(ValueError, match="grouped query over prefetched"):
        client.query_points_groups("t", V, group_by="ticker", prefetch=one)
    assert col.index.calls == [] and col.coalescer.requests == 0
    # limit < 1 and never-matching filters answer [] without a search
    never = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="NONE"))])
    assert client.query_points("t", rrf, prefetch=one, limit=0).points == []
    assert client.query_points("t", rrf, prefetch=[m.Prefetch(query=V, filter=never),
                                                   m.Prefetch(query=V, limit=0)]).points == []
    assert col.index.calls == [] and col.coalescer.requests == 0
    col.index.count = 5000
    with pytest.raises(ValueError, match="4800.*4096"):                    # 16 x 300 entries
        client.query_points("t", rrf, prefetch=[m.Prefetch(query=V, limit=300)] * 16)
    col.index.count = 40
    assert col.index.calls == []
    # rag: rewrites with MMR arguments are refused before any client exists
    monkeypatch.setenv("TESTING", "False")
    with pytest.raises(ValueError, match="rewrites"):
        rag.retrieve_from_qdrant(V, "AMD", rewrites=[V], diversity=0.5)
    with pytest.raises(ValueError, match="rewrites"):
        rag.retrieve_batch([V], ["AMD"], rewrites=[[V]], candidates=100)
    q, pre = rag._fusion(V, [V, V], rag._filter("amd", "10-k"), 15, None, None, None)
    assert q == rrf and len(pre) == 3 and all(p.limit == 50 and p.filter == rag._filter(
        "AMD", "10-K") for p in pre)
    q, pre = rag._fusion(V, [], None, 80, 60, None, None)
    assert q == m.RrfQuery(rrf=m.Rrf(k=60)) and [p.limit for p in pre] == [80]
