"""CPU tests of sparse vectors (include/ragmi.h "Sparse vectors"): every host-side
refusal, bm25_document / bm25_query against hand-computed values, vector-dict parsing, route
selection, the pass grouping, Collection over a stand-in index (an overwrite without a sparse
entry writes an empty row, a delete moves the sparse rows with the host maps, a collection
without a sparse config never calls a sparse method), the store round trip, the declared ABI,
and the restatement tests/_sparse_ref.py against itself."""
import json
import math
import os
import re

import numpy as np
import pytest

import _sparse_ref as R
import _stubs as S
from ragmi import qdrant_models as m
from ragmi.qdrant_models import SparseVector          # the parent commit fails here


def sv(idx, val):
    return SparseVector(indices=list(idx), values=list(val))


# ------------------------------------------------------------------ 1. the restatement itself
def test_reference_vectorised_score_is_the_literal_loop():
    rows, terms, vals, nnz = R.corpus(400, 16, seed=2)
    rng = np.random.default_rng(0)
    assert nnz[0] == 0 and nnz[1] == 1 and nnz[2] == 16
    assert terms[3, 0] == 0 and terms[4, 1] == 65534 and (vals < 0).any()
    for qi, qv in R.queries(rng, rows, 6, 8) + [(np.asarray([0, 65534]), np.asarray([1.0, -2.0]))]:
        s, ov = R.scores(terms, vals, qi, qv)
        for r in range(400):
            assert s[r].tobytes() == R.score_loop(terms[r], vals[r], qi, qv).tobytes()
            assert ov[r] == bool(set(terms[r][:nnz[r]].tolist()) & set(np.asarray(qi).tolist()))
    s, i = R.topk(terms, vals, 400, [7], [1.0], 400)
    n_hit = int((i >= 0).sum())
    assert 41 <= n_hit < 400 and (i[n_hit:] == -1).all() and np.isneginf(s[n_hit:]).all()
    assert (np.diff(s[:n_hit]) <= 0).all()
    tie = np.nonzero(s[:n_hit] == np.float32(0.5))[0]       # the 40 identical rows, row ascending
    assert len(tie) >= 40 and (np.diff(i[tie]) > 0).all()


def test_reference_quality_case_holds_for_the_seed():
    """The retrieval-quality check of the GPU suite, verified with the references alone: the
    dense top-12 holds none of the 12 rare-term points, the hybrid top-24 holds all of them."""
    import _fusion_ref as F
    import oracle_scan as O
    x, q, rows, rare, (qi, qv) = R.quality_case()
    _, dense = O.search(O.encode_rows(x), q[None, :], 50)
    assert not set(dense[0][:12].tolist()) & set(rare.tolist())
    terms, vals, _ = R.pack(rows, 16)
    _, sparse = R.topk(terms, vals, len(rows), qi, qv, 50)
    assert sorted(sparse[sparse >= 0].tolist()) == rare.tolist()
    cand = np.stack([dense[0], sparse])[None]
    fused = F.rrf(cand, None, 24)
    assert set(rare.tolist()) <= set(fused[1][0].tolist())


# ------------------------------------------------------------------ 2. host-side refusals
def test_entries_refusals_name_the_point():
    from ragmi.sparse import entries, pack_rows
    i, v = entries(sv([9, 3, 5], [1.0, 0.0, -2.0]), "p")
    assert i.tolist() == [5, 9] and v.tolist() == [-2.0, 1.0]          # zeros dropped, ascending
    for bad, pat in ((sv([65535], [1.0]), r"index 65535 outside \[0, 65535\)"),
                     (sv([-1], [1.0]), "index -1 outside"),
                     (sv([1 << 20], [1.0]), "outside"),
                     (sv([1, 2], [1.0, float("nan")]), "not finite"),
                     (sv([1], [float("inf")]), "not finite"),
                     (sv([1], [1e39]), "not finite"),
                     (sv([4, 4], [1.0, 2.0]), "repeats"),
                     (sv([4, 5], [1.0]), "2 sparse indices for 1 values"),
                     (sv([1.5], [1.0]), "integers"),
                     ([1.0, 2.0], "SparseVector")):
        with pytest.raises(ValueError, match=pat) as e:
            pack_rows([None, bad], 16, ["a", "b7"], "upsert: the sparse vector of point")
        assert "'b7'" in str(e.value)
    with pytest.raises(ValueError, match="17 nonzeros, at most 16") as e:
        pack_rows([sv(range(17), [1.0] * 17)], 16, ["big"])
    assert "'big'" in str(e.value)
    t, v, n = pack_rows([sv(range(17), [0.0] + [1.0] * 16), None], 16, ["z", "e"])   # zero dropped
    assert n.tolist() == [16, 0] and t[1].tolist() == [0xFFFF] * 16 and not v[1].any()
    assert t[0].tolist() == list(range(1, 17)) and t.dtype == np.uint16 and v.dtype == np.float32


def test_create_collection_refusals():
    from ragmi.qdrant import sparse_config
    P = m.SparseVectorParams
    assert sparse_config(None, 128) is None and sparse_config({}, 128) is None
    assert sparse_config({"bm25": P()}, 128) == ("bm25", False, 128)
    assert sparse_config({"s": P(modifier=m.Modifier.IDF)}, 32) == ("s", True, 32)
    assert sparse_config({"s": P(index=m.SparseIndexParams(on_disk=True,
                                                            datatype="float32"))}, 16)[1] is False
    with pytest.raises(NotImplementedError, match="one sparse vector"):
        sparse_config({"a": P(), "b": P()}, 128)
    with pytest.raises(ValueError, match='other than ""'):
        sparse_config({"": P()}, 128)
    with pytest.raises(NotImplementedError, match="float16"):
        sparse_config({"a": P(index=m.SparseIndexParams(datatype="float16"))}, 128)
    for slots in (0, 8, 24, 520, 1024):
        with pytest.raises(ValueError, match="multiple of 16"):
            Collection_("t", sparse=("bm25", False, slots))


def test_shard_set_refuses_a_sparse_vector():
    from ragmi.shardset import ShardSet
    with pytest.raises(NotImplementedError, match="sparse vectors over a shard set are not built"):
        ShardSet.sparse_create(object.__new__(ShardSet), 128)


# ------------------------------------------------------------------ 3. BM25
def test_bm25_document_and_query_by_hand():
    from ragmi.sparse import bm25_document, bm25_query, sequences
    ids = [101, 2054, 2003, 2054, 100, 7592, 102, 0, 0]       # [CLS] a b a [UNK] c [SEP] [PAD]x2
    d = bm25_document(ids)
    n = 4                                                     # a, b, a, c
    norm = 1.2 * (1 - 0.75 + 0.75 * n / 256.0)
    want = {2003: 1 * 2.2 / (1 + norm), 2054: 2 * 2.2 / (2 + norm), 7592: 1 * 2.2 / (1 + norm)}
    assert d.indices == [2003, 2054, 7592]
    assert [np.float32(v).tobytes() for v in d.values] == \
        [np.float32(want[t]).tobytes() for t in d.indices]
    assert d.values[1] == float(np.float32(4.4 / (2 + 1.2 * (0.25 + 0.75 * 4 / 256))))
    d2 = bm25_document(ids, k1=2.0, b=0.0, avg_len=10.0)
    assert d2.values[1] == float(np.float32(2 * 3.0 / (2 + 2.0)))
    ri, rv = R.bm25_document(ids)
    assert ri == d.indices and [float(v) for v in rv] == d.values
    q = bm25_query(ids)
    assert q.indices == [2003, 2054, 7592] and q.values == [1.0, 1.0, 1.0]
    assert bm25_document([101, 102]).indices == [] and bm25_query([]).indices == []
    # more distinct terms than slots: the largest values stay, ties to the lower term
    many = [1000 + i for i in range(20)] + [1005, 1005, 1019]
    d3 = bm25_document(many, slots=16)
    assert len(d3.indices) == 16 and 1005 in d3.indices and 1019 in d3.indices
    assert d3.indices == sorted(d3.indices)
    assert set(d3.indices) == {1005, 1019} | set(range(1000, 1015)) - {1005}
    ri, rv = R.bm25_document(many, S=16)
    assert ri == d3.indices and [float(v) for v in rv] == d3.values
    seqs = sequences(np.arange(10), np.asarray([0, 4, 4, 10]))
    assert [s.tolist() for s in seqs] == [[0, 1, 2, 3], [], [4, 5, 6, 7, 8, 9]]


def test_idf_weights_by_hand():
    from ragmi.sparse import idf_weights
    df = np.zeros(65535, np.int64)
    df[5], df[9] = 3, 100
    w = idf_weights([5, 9, 11], np.asarray([1.0, 2.0, 0.5], np.float32), df, 100)
    want = [np.float32(1.0 * math.log(1 + 97.5 / 3.5)), np.float32(2.0 * math.log(1 + 0.5 / 100.5)),
            np.float32(0.5 * math.log(1 + 100.5 / 0.5))]
    assert w.dtype == np.float32 and [x.tobytes() for x in w] == [x.tobytes() for x in want]
    assert [x.tobytes() for x in R.idf_weights([5, 9, 11], [1.0, 2.0, 0.5], df, 100)] == \
        [x.tobytes() for x in want]


# ------------------------------------------------------------------ 4. parsing and routes
class _SpIndex:
    """Index stand-in (the `index=` protocol) that keeps tags and the sparse column in numpy and
    records every sparse call."""
    device = None
    storage = "fp16"
    rescued = 0

    def __init__(self, dim=2, capacity=16, device=None, storage="fp16"):
        self.dim = dim
        self.rows = np.zeros((capacity, dim), np.uint16)
        self.tag = np.zeros(capacity, np.uint32)
        self.count = 0
        self.slots = 0
        self.terms = self.vals = None
        self.calls = []

    @property
    def capacity(self):
        return len(self.tag)

    def reserve(self, cap):
        if cap > self.capacity:
            grow = cap - self.capacity
            self.rows = np.concatenate([self.rows, np.zeros((grow, self.dim), np.uint16)])
            self.tag = np.concatenate([self.tag, np.zeros(grow, np.uint32)])
            if self.slots:
                self.terms = np.concatenate([self.terms, np.full((grow, self.slots), 0xFFFF, np.uint16)])
                self.vals = np.concatenate([self.vals, np.zeros((grow, self.slots), np.float32)])

    def upsert(self, vectors, rows, tags=None, new_count=None):
        self.tag[rows] = tags
        self.rows[rows, 0] = 0x3C00
        self.count = new_count

    def sparse_create(self, slots=128):
        self.calls.append(("sparse_create", slots))
        self.slots = slots
        self.terms = np.full((self.capacity, slots), 0xFFFF, np.uint16)
        self.vals = np.zeros((self.capacity, slots), np.float32)

    def sparse_slots(self):
        return self.slots

    def sparse_write(self, rows, terms, vals):
        self.calls.append(("sparse_write", np.asarray(rows).tolist()))
        self.terms[np.asarray(rows)] = np.asarray(terms).view(np.uint16)
        self.vals[np.asarray(rows)] = vals

    def sparse_gather(self, rows):
        import torch
        self.calls.append(("sparse_gather", np.asarray(rows).tolist()))
        r = np.asarray(rows)
        return (torch.from_numpy(self.terms[r].view(np.int16).copy()),
                torch.from_numpy(self.vals[r].copy()))

    def sparse_df(self):
        import torch
        self.calls.append(("sparse_df",))
        return torch.from_numpy(R.df(self.terms, self.count))

    def sparse_search(self, q_terms, q_vals, q_nnz, k, filters=None, rescue=False, programs=None):
        import torch
        self.calls.append(("sparse_search", len(q_nnz), k))
        self.last_query = (np.array(q_terms), np.array(q_vals), np.array(q_nnz))
        qs = [(q_terms[b][:q_nnz[b]], q_vals[b][:q_nnz[b]]) for b in range(len(q_nnz))]
        passing = None
        if filters is not None:
            passing = [(self.tag[:self.count] & f[0]) == f[1] for f in np.asarray(filters)]
        s, i = R.search(self.terms, self.vals, self.count, qs, k, passing)
        return torch.from_numpy(s), torch.from_numpy(i)

    def remove_rows(self, rows):
        from ragmi.index import plan_removal
        src, dst, n1 = plan_removal(self.count, rows)
        for a in (self.rows, self.tag) + ((self.terms, self.vals) if self.slots else ()):
            a[dst] = a[src]
        self.count = n1
        return src, dst, n1

    def export_rows(self, row0=0, n=None):
        return self.rows[row0:row0 + n].copy()

    def export_tags(self, row0=0, n=None):
        return self.tag[row0:row0 + n].copy()

    def import_rows(self, a, row0=0, tags=None, new_count=None):
        a = np.asarray(a)
        self.rows[row0:row0 + len(a)] = a.view(np.uint16) if a.dtype == np.float16 else a
        self.tag[row0:row0 + len(a)] = tags
        self.count = new_count

    def close(self):
        pass


class _NoStream:
    def synchronize(self):
        pass


@pytest.fixture
def no_stream(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _NoStream())


def Collection_(name="t", sparse=("bm25", False, 16), index=None):
    from ragmi.collection import Collection
    return Collection(name, 2, None, index=index if index is not None else _SpIndex(),
                      sparse=sparse)


def sparse_calls(idx):
    return [c for c in idx.calls if c[0].startswith("sparse")]


def test_vector_dict_parsing(no_stream):
    from ragmi.qdrant import split_vectors
    col = Collection_()
    a, b = sv([1], [1.0]), sv([2, 3], [1.0, 2.0])
    assert split_vectors(col, [1, 2], [[1.0, 0.0], [0.0, 1.0]]) == ([[1.0, 0.0], [0.0, 1.0]], None)
    arr = np.ones((2, 2), np.float32)
    assert split_vectors(col, [1, 2], arr)[0] is arr and split_vectors(col, [1, 2], arr)[1] is None
    d, s = split_vectors(col, [1, 2, 3], [{"": [1.0, 0.0], "bm25": a}, [0.0, 1.0],
                                          {"": [1.0, 1.0], "bm25": None}])
    assert d == [[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]] and s == [a, None, None]
    d, s = split_vectors(col, [1, 2], {"": [[1.0, 0.0], [0.0, 1.0]], "bm25": [a, b]})
    assert d == [[1.0, 0.0], [0.0, 1.0]] and s == [a, b]
    assert split_vectors(col, [1], {"": [[1.0, 0.0]]}) == ([[1.0, 0.0]], None)
    with pytest.raises(ValueError, match="'title' is not a vector of collection 't'") as e:
        split_vectors(col, [7], [{"": [1.0, 0.0], "title": a}])
    assert "point 7" in str(e.value)
    with pytest.raises(ValueError, match='the dense vector \\(the "" entry\\) is required'):
        split_vectors(col, [7], [{"bm25": a}])
    with pytest.raises(ValueError, match="1 sparse vectors for 2 ids"):
        split_vectors(col, [1, 2], {"": [[1.0, 0.0], [0.0, 1.0]], "bm25": [a]})
    plain = Collection_(sparse=None)
    with pytest.raises(ValueError, match="'bm25' is not a vector.*no sparse vector"):
        split_vectors(plain, [1], [{"": [1.0, 0.0], "bm25": a}])
    # through the client: dicts, a Batch, and a plain list into the same collection
    client, _ = S.stub_client(col)
    client.upsert("t", [m.PointStruct(id=1, vector={"": [1.0, 0.0], "bm25": a}),
                        m.PointStruct(id=2, vector=[0.0, 1.0])])
    client.upsert("t", m.Batch(ids=[3], vectors={"": [[1.0, 1.0]], "bm25": [b]}))
    idx = col.index
    assert idx.terms[0, :2].tolist() == [1, 0xFFFF] and idx.terms[1, 0] == 0xFFFF
    assert idx.terms[2, :3].tolist() == [2, 3, 0xFFFF] and col.sparse_len == [1, 0, 2]
    with pytest.raises(ValueError, match="sparse index 70000 outside") as e:
        client.upsert("t", [m.PointStruct(id=9, vector={"": [1.0, 0.0], "bm25": sv([70000], [1.0])})])
    assert "9" in str(e.value) and len(col.row_ids) == 3                # nothing was written


def test_route_selection_and_query_refusals(no_stream):
    from ragmi import qdrant as Q
    q = sv([1, 2], [1.0, 1.0])
    assert Q.route_of(q) == Q.SPARSE and Q.route_of(m.NearestQuery(nearest=q)) == Q.SPARSE
    assert Q.route_of(q, [m.Prefetch(query=[1.0, 0.0])]) == Q.SPARSE    # refused on that route
    assert Q.route_of([1.0, 0.0]) == Q.PLAIN
    assert Q.route_of(m.FusionQuery(fusion=m.Fusion.RRF), [m.Prefetch(query=q, using="bm25")]) \
        == Q.FUSION
    col = Collection_()
    client, _ = S.stub_client(col)
    client.upsert("t", [m.PointStruct(id=i, vector={"": [1.0, 0.0], "bm25": sv([i, 50], [1.0, 2.0])},
                                      payload={"ticker": "AMD" if i % 2 else "NVDA"})
                        for i in range(1, 7)])
    got = client.query_points("t", query=q, using="bm25", limit=10)
    assert [p.id for p in got.points] == [1, 2] and got.points[0].score == 1.0
    assert [c for c in sparse_calls(col.index) if c[0] == "sparse_search"] == [("sparse_search", 1, 6)]
    # one request routes once; a batch of sparse requests is one sparse search
    col.index.calls.clear()
    res = client.query_batch_points("t", [
        m.QueryRequest(query=sv([50], [1.0]), using="bm25", limit=2),
        m.QueryRequest(query=sv([3], [1.0]), using="bm25", limit=5,
                       filter=m.Filter(must=[m.FieldCondition(key="ticker",
                                                              match=m.MatchValue(value="AMD"))]))])
    assert [p.id for p in res[0].points] == [1, 2] and [p.id for p in res[1].points] == [3]
    assert [c for c in col.index.calls if c[0] == "sparse_search"] == [("sparse_search", 2, 5)]
    for kwargs, pat in (
            (dict(query=q), "needs using='bm25'"),
            (dict(query=q, using="title"), "using='title' is not a vector.*'bm25'"),
            (dict(query=[1.0, 0.0], using="bm25"), "using='bm25' with a dense query vector"),
            (dict(query=[1.0, 0.0], using="bm25", limit=100), "with a dense query vector"),
            (dict(query=sv(range(65), [1.0] * 65), using="bm25"), "65 entries.*at most 64"),
            (dict(query=sv([1, 1], [1.0, 1.0]), using="bm25"), "repeats"),
            (dict(query=sv([65535], [1.0]), using="bm25"), "outside"),
            (dict(query=q, using="bm25", prefetch=[m.Prefetch(query=[1.0, 0.0])]),
             "sparse query over prefetched candidates"),
            (dict(query=m.NearestQuery(nearest=q, mmr=m.Mmr(diversity=0.5)), using="bm25"),
             "MMR query .* over a sparse vector is not built"),
            (dict(query=m.FormulaQuery(formula="$score"),
                  prefetch=[m.Prefetch(query=q, using="bm25")]),
             "sparse prefetch inside a formula query is not built"),
            (dict(query=m.FusionQuery(fusion=m.Fusion.RRF),
                  prefetch=[m.Prefetch(query=[1.0, 0.0], using="bm25")]),
             "using='bm25' names a sparse vector, but the query is a dense vector"),
            (dict(query=m.FusionQuery(fusion=m.Fusion.RRF), prefetch=[m.Prefetch(query=q)]),
             "needs using='bm25'"),
            (dict(query=m.RecommendQuery(recommend=m.RecommendInput(positive=[q]))),
             "SparseVector examples is not built")):
        with pytest.raises(ValueError, match=pat):
            client.query_points("t", **kwargs)
    with pytest.raises(ValueError, match="grouped query cannot be a SparseVector"):
        client.query_points_groups("t", query=q, group_by="ticker")
    plain = Collection_("p", sparse=None)
    client._collections["p"] = plain
    with pytest.raises(ValueError, match="collection 'p' has no sparse vector"):
        client.query_points("p", query=q, using="bm25")
    assert sparse_calls(plain.index) == []


def test_sparse_groups_split_by_count_and_union():
    from ragmi.index import sparse_groups
    qs = [(np.arange(8) + 8 * b, np.ones(8, np.float32)) for b in range(70)]
    t, _, n = R.pack(qs, 64)
    assert sparse_groups(t, n) == [(0, 32), (32, 64), (64, 70)]
    wide = [(np.arange(64) + 64 * b, np.ones(64, np.float32)) for b in range(20)]
    t, _, n = R.pack(wide, 64)
    assert sparse_groups(t, n) == [(0, 8), (8, 16), (16, 20)]                # 8 x 64 = 512
    same = [(np.arange(64), np.ones(64, np.float32))] * 40
    t, _, n = R.pack(same, 64)
    assert sparse_groups(t, n) == [(0, 32), (32, 40)]
    assert sparse_groups(t[:0], n[:0]) == []
    t, _, n = R.pack(wide[:8] + [(np.asarray([9999]), np.ones(1, np.float32))], 64)
    assert sparse_groups(t, n) == [(0, 8), (8, 9)]


# ------------------------------------------------------------------ 5. Collection over a stand-in
def test_overwrite_without_a_sparse_entry_writes_an_empty_row(no_stream):
    col = Collection_()
    idx = col.index
    assert idx.calls == [("sparse_create", 16)]
    v = np.ones((3, 2), np.float32)
    col.upsert([10, 11, 12], v, None, [sv([5, 2], [1.0, 2.0]), None, sv([9], [3.0])])
    assert idx.terms[0, :3].tolist() == [2, 5, 0xFFFF] and idx.vals[0, :2].tolist() == [2.0, 1.0]
    assert idx.terms[1].tolist() == [0xFFFF] * 16 and col.sparse_len == [2, 0, 1]
    col.upsert([10], v[:1], None)                          # Qdrant's upsert replaces the point
    assert idx.terms[0].tolist() == [0xFFFF] * 16 and not idx.vals[0].any()
    assert col.sparse_len == [0, 0, 1]
    assert [c for c in sparse_calls(idx) if c[0] == "sparse_write"] == \
        [("sparse_write", [0, 1, 2]), ("sparse_write", [0])]
    # growth past the capacity: the column follows
    col.upsert(list(range(100, 130)), np.ones((30, 2), np.float32), None,
               [sv([i], [1.0]) for i in range(30)])
    assert idx.capacity >= 33 and len(idx.terms) == idx.capacity and idx.terms[32, 0] == 29


def test_delete_moves_the_sparse_rows_with_the_host_maps(no_stream):
    col = Collection_(sparse=("bm25", True, 16))
    col.upsert(list(range(10)), np.ones((10, 2), np.float32), None,
               [sv([i, 100], [1.0, 1.0]) if i % 3 else None for i in range(10)])
    df, n_docs = col.sparse_stats()
    assert n_docs == 6 and df[100] == 6 and df[4] == 1
    assert col.sparse_stats()[0] is df                      # cached
    col.delete([1, 2, 9])
    assert col.index.count == 7 and len(col.sparse_len) == 7
    for pid, r in col.id_to_row.items():
        want = [pid, 100] if pid % 3 else []
        got = col.index.terms[r]
        assert got[got != 0xFFFF].tolist() == want and col.sparse_len[r] == len(want)
    df2, n2 = col.sparse_stats()                            # a delete invalidates the cache
    assert n2 == 4 and df2[100] == 4 and df2 is not df
    col.upsert([50], np.ones((1, 2), np.float32), None, [sv([100], [1.0])])
    assert col.sparse_stats()[1] == 5                       # and so does an upsert
    # Modifier.IDF: the query weights are multiplied on the host
    hits = col.search_sparse([(sv([100, 4], [1.0, 2.0]), "bm25", (0, 0), 10)])[0]
    _, qv, qn = col.index.last_query
    want = R.idf_weights([4, 100], [2.0, 1.0], col.sparse_stats()[0], 5)
    assert qn.tolist() == [2] and qv[0, :2].tobytes() == want.tobytes()
    assert hits[0][0] == col.id_to_row[4] and len(hits) == 5


def test_a_collection_without_a_sparse_config_never_calls_a_sparse_method(no_stream):
    from ragmi.collection import Collection
    idx = _SpIndex()
    col = Collection("t", 2, None, index=idx)
    client, _ = S.stub_client(col)
    client.upsert("t", [m.PointStruct(id=i, vector=[1.0, 0.0], payload={"ticker": "AMD"})
                        for i in range(5)])
    client.delete("t", [1])
    assert client.retrieve("t", [0], with_vectors=True)[0].vector == [1.0, 0.0]
    assert sparse_calls(idx) == [] and col.sparse_name is None
    with pytest.raises(ValueError, match="has no sparse vector"):
        col.upsert([7], np.ones((1, 2), np.float32), None, [sv([1], [1.0])])


def test_retrieve_with_vectors_names_both(no_stream):
    col = Collection_()
    client, _ = S.stub_client(col)
    client.upsert("t", [m.PointStruct(id=1, vector={"": [1.0, 0.0], "bm25": sv([7, 3], [0.5, 2.0])}),
                        m.PointStruct(id=2, vector=[1.0, 0.0])])
    a, b = client.retrieve("t", [1, 2], with_vectors=True)
    assert a.vector == {"": [1.0, 0.0], "bm25": sv([3, 7], [2.0, 0.5])}
    assert b.vector == {"": [1.0, 0.0], "bm25": sv([], [])}


def test_store_round_trip(tmp_path, no_stream, monkeypatch):
    from ragmi import collection, store
    col = Collection_("h", sparse=("bm25", True, 32))
    col.upsert(list(range(6)), np.ones((6, 2), np.float32), [{"ticker": "AMD"}] * 6,
               [sv([i, 40 + i], [1.0, -2.5]) if i != 3 else None for i in range(6)])
    store.save_collection(col, str(tmp_path / "h"))
    cj = json.load(open(tmp_path / "h" / "collection.json"))
    assert cj["sparse"] == {"name": "bm25", "modifier": "idf", "slots": 32}
    meta = json.load(open(tmp_path / "h" / "shard" / "meta.json"))
    assert meta["version"] == store.VERSION == 1
    t = np.load(tmp_path / "h" / "shard" / "sparse.terms.u16.npy")
    v = np.load(tmp_path / "h" / "shard" / "sparse.vals.f32.npy")
    assert t.dtype == np.uint16 and t.shape == (6, 32) and v.dtype == np.float32
    monkeypatch.setattr(collection, "FlatIndex",
                        lambda dim, capacity, device, storage: _SpIndex(dim, capacity))
    back = store.load_collection(str(tmp_path / "h"))
    assert (back.sparse_name, back.sparse_idf, back.sparse_slots) == ("bm25", True, 32)
    assert back.sparse_len == col.sparse_len == [2, 2, 2, 0, 2, 2]
    np.testing.assert_array_equal(back.index.terms[:6], col.index.terms[:6])
    np.testing.assert_array_equal(back.index.vals[:6], col.index.vals[:6])
    # a saved row that is not in the stored layout is refused, naming the row
    t2 = np.lib.format.open_memmap(str(tmp_path / "h" / "shard" / "sparse.terms.u16.npy"), mode="r+")
    t2[4, 0], t2[4, 1] = t2[4, 1], t2[4, 0]
    t2.flush()
    del t2
    with pytest.raises(ValueError, match="sparse row 4 is not in the stored layout"):
        store.load_collection(str(tmp_path / "h"))
    # a collection without a sparse vector saves and loads as before
    plain = Collection_("p", sparse=None)
    plain.upsert([1, 2], np.ones((2, 2), np.float32), [{"ticker": "AMD"}, None])
    store.save_collection(plain, str(tmp_path / "p"))
    assert sorted(json.load(open(tmp_path / "p" / "collection.json"))) == \
        ["codebooks", "dim", "distance", "name", "op", "storage", "tag_fields"]
    assert sorted(os.listdir(tmp_path / "p" / "shard")) == ["meta.json", "tags.u32.npy",
                                                            "vectors.f16.npy"]
    again = store.load_collection(str(tmp_path / "p"))
    assert again.sparse_name is None and sparse_calls(again.index) == sparse_calls(plain.index) == []


def test_hybrid_fusion_over_a_stand_in(no_stream):
    """search_fusion places dense and sparse prefetches into one row tensor; the sparse list is
    cut by ncand to its real hits."""
    import torch

    from ragmi import collection
    col = Collection_()
    idx = col.index
    idx.search = lambda q, k, filters=None, rescue=False, **kw: (
        torch.zeros((len(q), k)), torch.arange(k).repeat(len(q), 1))
    col.upsert(list(range(8)), np.ones((8, 2), np.float32), None,
               [sv([i % 2, 9], [1.0, float(i)]) for i in range(8)])
    seen = {}

    def fake_fuse(rows, k, rrf_k, ncand):
        seen["rows"], seen["ncand"] = rows.clone(), np.array(ncand)
        return torch.zeros((rows.shape[0], k)), torch.full((rows.shape[0], k), -1)
    collection.fuse_rrf, keep = fake_fuse, collection.fuse_rrf
    try:
        client, _ = S.stub_client(col)
        client.query_points("t", query=m.FusionQuery(fusion=m.Fusion.RRF), limit=4, prefetch=[
            m.Prefetch(query=[1.0, 0.0], limit=5),
            m.Prefetch(query=sv([1], [1.0]), using="bm25", limit=6)])
    finally:
        collection.fuse_rrf = keep
    assert seen["rows"].shape == (1, 2, 6) and seen["ncand"].tolist() == [[5, 4]]
    assert seen["rows"][0, 0].tolist() == [0, 1, 2, 3, 4, 5]
    assert seen["rows"][0, 1].tolist() == [1, 3, 5, 7, -1, -1]


def test_rag_layer_defaults_are_todays_calls(monkeypatch):
    from ragmi import rag
    made = {}

    class _Q:
        def collection_exists(self, name):
            return False

        def create_collection(self, **kw):
            made.update(kw)
    rag.ensure_collection(_Q())
    assert sorted(made) == ["collection_name", "vectors_config"]
    rag.ensure_collection(_Q(), hybrid=True)
    assert made["sparse_vectors_config"] == {"bm25": m.SparseVectorParams(modifier=m.Modifier.IDF)}
    pts = rag.chunk_points("amd", "10-k", "f", ["a b"], [[0.0] * 384], ingested_at="t")
    assert pts[0].vector == [0.0] * 384
    monkeypatch.setattr(rag, "sparse_texts", lambda texts, kind: [sv([7], [1.0]) for _ in texts])
    pts = rag.chunk_points("amd", "10-k", "f", ["a b"], [[0.0] * 384], ingested_at="t", sparse=True)
    assert pts[0].vector == {"": [0.0] * 384, "bm25": sv([7], [1.0])}
    q, pre = rag._fusion([1.0], [], None, 15, None, None, None)
    assert len(pre) == 1 and pre[0].using is None
    q, pre = rag._fusion([1.0], [[2.0]], "F", 15, None, None, None, sparse=sv([7], [1.0]))
    assert [p.using for p in pre] == [None, None, "bm25"] and pre[2].limit == 50
    assert pre[2].filter == "F" and isinstance(q, m.FusionQuery)


# ------------------------------------------------------------------ 6. the ABI
def test_abi_is_declared_and_bound():
    from conftest import ROOT
    from ragmi import _lib, index
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    for name, n_args in (("rag_index_sparse_create", 2), ("rag_index_sparse_slots", 1),
                         ("rag_index_sparse_write", 6), ("rag_index_sparse_gather", 6),
                         ("rag_index_sparse_df", 3), ("rag_index_sparse_search", 15)):
        decl = re.search(rf"int {name}\(([^;]*)\);", hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.INDEX_API[name][1]) == n_args, name
    for macro, value in (("RAG_SPARSE_TERM_NONE", index.SPARSE_TERM_NONE),
                         ("RAG_SPARSE_MAX_SLOTS", index.SPARSE_MAX_SLOTS),
                         ("RAG_SPARSE_MAX_QUERY_NNZ", index.SPARSE_MAX_QUERY_NNZ),
                         ("RAG_SPARSE_MAX_UNION", index.SPARSE_MAX_UNION)):
        got = re.search(rf"#define {macro} (\w+)", hdr).group(1)
        assert int(got.rstrip("u"), 0) == value, macro
    assert R.NONE == index.SPARSE_TERM_NONE and R.TERMS == index.SPARSE_TERMS
    assert R.QUERY_NNZ == index.SPARSE_MAX_QUERY_NNZ
    # the LDS budget of the scorer: two workgroups in a CU's 160 KB
    lds = 4 * (2048 + 1024 + index.SPARSE_MAX_UNION + 32 * index.SPARSE_MAX_UNION)
    assert 2 * lds <= 160 * 1024
