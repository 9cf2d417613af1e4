"""GPU tests of sparse vectors (rag_index_sparse_* / sparse_kernels.hip, FlatIndex.sparse_*,
Collection.search_sparse and the hybrid prefetches of search_fusion behind QdrantClient; DESIGN.md
R19): ids and scores bit-equal to the restatement tests/_sparse_ref.py on both passes, over
corpora with a tile tail and a real threshold, under filters, after row moves, and through the
client."""
import numpy as np
import pytest
import torch

import _fusion_ref as F
import _sparse_ref as R
import oracle_scan as O
from ragmi import qdrant_models as m
from ragmi.qdrant_models import SparseVector          # the parent commit fails here

pytestmark = pytest.mark.gpu

DIM = 384


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    s, i = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got)
    assert np.array_equal(i, want[1])
    assert np.array_equal(bits(s), bits(want[0]))


def sv(q):
    return SparseVector(indices=np.asarray(q[0]).tolist(), values=np.asarray(q[1]).tolist())


class Corpus:
    """A sparse corpus in a FlatIndex (dense rows random, tags 1..4) and its reference arrays."""

    def __init__(self, gpu, n, S, seed, rows=None):
        from ragmi.index import FlatIndex
        if rows is None:
            self.rows, self.terms, self.vals, self.nnz = R.corpus(n, S, seed)
        else:
            self.rows = rows
            self.terms, self.vals, self.nnz = R.pack(rows, S)
        rng = np.random.default_rng(seed + 100)
        self.n, self.S = n, S
        self.tags = (rng.integers(0, 4, n) + 1).astype(np.uint32)
        self.idx = FlatIndex(DIM, n, gpu, storage="fp16")
        x = rng.standard_normal((n, DIM)).astype(np.float32)
        self.idx.upsert(x, np.arange(n), self.tags, new_count=n)
        self.idx.sparse_create(S)
        self.idx.sparse_write(np.arange(n), self.terms, self.vals)

    def search(self, qs, k, **kw):
        qt, qv, qn = R.pack(qs, 64)
        out = self.idx.sparse_search(qt, qv, qn, k, **kw)
        torch.cuda.synchronize()
        return out

    def want(self, qs, k, passing=None):
        return R.search(self.terms, self.vals, self.n, qs, k, passing)


@pytest.fixture(scope="module")
def small128(gpu):
    c = Corpus(gpu, 3001, 128, 1)
    yield c
    c.idx.close()


@pytest.fixture(scope="module")
def small16(gpu):
    c = Corpus(gpu, 3001, 16, 2)
    yield c
    c.idx.close()


@pytest.fixture(scope="module")
def big128(gpu):
    c = Corpus(gpu, 50009, 128, 3)
    yield c
    c.idx.close()


# ------------------------------------------------------------------ 1. storage
@pytest.mark.parametrize("which", ["small128", "small16"])
def test_gather_returns_what_write_wrote_and_df_is_bincount(which, request):
    c = request.getfixturevalue(which)
    rows = np.asarray([0, 1, 2, 3, 4, 1007, c.n - 1, c.n + 10 ** 6, -1])
    t, v = c.idx.sparse_gather(rows)
    t, v = t.cpu().numpy().view(np.uint16), v.cpu().numpy()
    assert np.array_equal(t[:7], c.terms[rows[:7]]) and np.array_equal(bits(v[:7]), bits(c.vals[rows[:7]]))
    assert (t[7:] == R.NONE).all() and not v[7:].any()        # outside [0, capacity): empty rows
    t, v = c.idx.sparse_gather(np.arange(c.n))
    assert np.array_equal(t.cpu().numpy().view(np.uint16), c.terms)
    assert c.idx.sparse_slots() == c.S
    df = c.idx.sparse_df().cpu().numpy()
    t_all = c.terms.reshape(-1).astype(np.int64)
    assert np.array_equal(df, np.bincount(t_all[t_all != R.NONE], minlength=65535)[:65535])
    assert df[0] >= 2 and df[65534] >= 2 and np.array_equal(df, c.idx.sparse_df().cpu().numpy())


def test_argument_errors_are_refused(gpu, small16):
    from ragmi._lib import RagmiError
    from ragmi.index import FlatIndex
    plain = FlatIndex(DIM, 64, gpu)
    assert plain.sparse_slots() == 0
    with pytest.raises(ValueError, match="no sparse column"):
        plain.sparse_search(*R.pack([([1], [1.0])], 64), 5)
    with pytest.raises(RagmiError, match="no sparse column"):
        plain.sparse_df()
    for slots in (0, 8, 24, 528):
        with pytest.raises(RagmiError, match="multiple of 16"):
            plain.sparse_create(slots)
    plain.sparse_create(32)
    plain.sparse_create(32)                                   # the same slot count: a no-op
    with pytest.raises(RagmiError, match="another slot count"):
        plain.sparse_create(16)
    with pytest.raises(ValueError, match=r"\[n, 32\]"):
        plain.sparse_write([0], np.zeros((1, 16), np.uint16), np.zeros((1, 16), np.float32))
    plain.close()
    qt, qv, qn = R.pack([([1], [1.0])], 64)
    with pytest.raises(ValueError, match="k must be >= 1"):
        small16.idx.sparse_search(qt, qv, qn, 0)
    with pytest.raises(ValueError, match="padded to"):
        small16.idx.sparse_search(qt[:, :32], qv[:, :32], qn, 5)
    with pytest.raises(ValueError, match="0 to 64 nonzeros"):
        small16.idx.sparse_search(qt, qv, np.asarray([65]), 5)


# ------------------------------------------------------------------ 2. both passes against the restatement
BATCHES = {"B1": (1, 1), "B32": (32, 8), "B33": (33, 64)}    # B queries of nnz terms


@pytest.mark.parametrize("k", [1, 15, 200, 4097])
@pytest.mark.parametrize("batch", ["B1", "B32", "B33"])
@pytest.mark.parametrize("which", ["small128", "small16"])
def test_search_equals_the_reference_on_both_passes(which, batch, k, request):
    """B = 33 queries of 64 terms: two passes by count and, their union exceeding the cap, more
    by union. k = 4097 is above the hot limit (the full pass either way) and above the
    eligible rows of every query (the padding), as any k is for the query no row overlaps."""
    c = request.getfixturevalue(which)
    B, nnz = BATCHES[batch]
    rng = np.random.default_rng(10 * k + B)
    qs = R.queries(rng, c.rows, B, nnz)
    if batch == "B32":
        qs[0] = (np.asarray([0, 65534]), np.asarray([1.0, -2.0], np.float32))
        qs[1] = (np.asarray([3, 7, 11, 500]), np.asarray([1.0, 1.0, 1.0, 1.0], np.float32))  # the ties
        free = np.setdiff1d(np.arange(60000, 65534), c.terms)[:1]       # a term no row holds
        qs[2] = (free, np.asarray([1.0], np.float32))
    want = c.want(qs, k)
    if batch == "B32":
        assert (want[1][2] == -1).all() and (want[1][:2, 0] >= 0).all()
        assert (want[1][:2, -1] >= 0).all() == (k <= 200)               # k = 4097: the padding
    un0 = c.idx.unanswered()
    hot = c.search(qs, k)
    same(hot, want)
    full = c.search(qs, k, full=True)
    same(full, want)
    assert np.array_equal(bits(hot[0].cpu().numpy()), bits(full[0].cpu().numpy()))
    assert c.idx.unanswered() == un0


@pytest.mark.parametrize("batch,k", [("B32", 15), ("B33", 200), ("B1", 4096)])
def test_search_over_a_real_threshold(big128, batch, k):
    """50,009 rows: the sample is a fraction of the tiles and the threshold cuts most rows."""
    B, nnz = BATCHES[batch]
    qs = R.queries(np.random.default_rng(k), big128.rows, B, max(nnz, 4))
    want = big128.want(qs, k)
    same(big128.search(qs, k), want)
    same(big128.search(qs[:4], k, full=True), (want[0][:4], want[1][:4]))


def test_a_union_above_the_cap_splits_into_passes(small128, monkeypatch):
    from ragmi import index
    rng = np.random.default_rng(77)
    qs = R.queries(rng, small128.rows, 32, 64)
    qt, _, qn = R.pack(qs, 64)
    groups = index.sparse_groups(qt, qn)
    assert len(groups) > 1 and len(np.unique(qt[qt != R.NONE])) > index.SPARSE_MAX_UNION
    want = small128.want(qs, 15)
    same(small128.search(qs, 15), want)
    # one pass handed more terms than its table holds answers nothing and says so
    monkeypatch.setattr(index, "sparse_groups", lambda t, n: [(0, len(n))])
    un0 = small128.idx.unanswered()
    s, i = small128.search(qs, 15)
    assert (i.cpu().numpy() == -1).all() and np.isneginf(s.cpu().numpy()).all()
    assert small128.idx.unanswered() == un0 + 32
    same(small128.search(qs, 15, rescue=True), want)          # ... and the rescue re-answers it


# ------------------------------------------------------------------ 3. filters
def test_tag_filters_a_view_program_and_a_filter_that_matches_nothing(small128):
    from ragmi.filters import FilterProgram, pack_view
    c = small128
    rng = np.random.default_rng(5)
    qs = R.queries(rng, c.rows, 32, 8)
    tag = rng.integers(1, 5, 32).astype(np.uint32)
    tag[5] = 9                                                # no row holds tag 9
    filt = np.stack([np.full(32, 0xFFFF, np.uint32), tag], axis=1)
    filt[7] = (0, 0)                                          # every row
    passing = [(c.tags & f[0]) == f[1] for f in filt]
    want = c.want(qs, 15, passing)
    assert (want[1][5] == -1).all()
    same(c.search(qs, 15, filters=filt), want)
    same(c.search(qs, 15, filters=filt, full=True), want)
    # a filter view: program 0 = tag in {1, 2} (two MASKEQ atoms, either), program 1 = tag 3
    either = FilterProgram((("maskeq", 0xFFFF, 1), ("maskeq", 0xFFFF, 2)), 0b1110)
    blob = pack_view([either, FilterProgram.maskeq(0xFFFF, 3)])
    use = np.asarray([(1, 1) if j % 3 == 0 else (2, 2) if j % 3 == 1 else (0, 0)
                      for j in range(32)], np.uint32)
    passing = [np.isin(c.tags, (1, 2)) if j % 3 == 0 else c.tags == 3 if j % 3 == 1 else
               np.ones(c.n, bool) for j in range(32)]
    want = c.want(qs, 40, passing)
    same(c.search(qs, 40, filters=use, programs=blob), want)
    same(c.search(qs, 40, filters=use, programs=blob, full=True), want)


# ------------------------------------------------------------------ 4. more ties than a pass keeps
def test_identical_rows_are_left_unanswered_and_rescued(gpu):
    rows, terms, vals, nnz = R.identical_corpus()
    c = Corpus(gpu, len(rows), 16, 4, rows=rows)
    try:
        qs = [(np.asarray([5, 9]), np.asarray([1.0, 0.5], np.float32)),
              (np.asarray([77]), np.asarray([1.0], np.float32))]
        un0 = c.idx.unanswered()
        s, i = c.search(qs, 10)
        assert (i.cpu().numpy() == -1).all() and c.idx.unanswered() == un0 + 1   # 77: no overlap
        want = c.want(qs, 10)
        assert want[1][0].tolist() == list(range(10)) and (want[1][1] == -1).all()
        r0 = c.idx.rescued
        same(c.search(qs, 10, rescue=True), want)
        assert c.idx.rescued == r0 + 2 and c.idx.unanswered() == un0 + 2
        same(c.search(qs, 10, full=True), want)
    finally:
        c.idx.close()


# ------------------------------------------------------------------ 5. the sparse row moves with its row
def test_search_after_remove_rows_and_reserve(gpu):
    from ragmi.index import plan_removal
    c = Corpus(gpu, 3001, 16, 6)
    try:
        rng = np.random.default_rng(8)
        qs = R.queries(rng, c.rows, 32, 8)
        gone = np.unique(np.concatenate([rng.choice(3001, 400, replace=False), [0, 2, 3000, 2990]]))
        src, dst, n1 = plan_removal(3001, gone)
        c.idx.remove_rows(gone)
        terms, vals = c.terms.copy(), c.vals.copy()
        terms[dst], vals[dst] = terms[src], vals[src]
        assert c.idx.count == n1 == 3001 - len(gone)
        want = R.search(terms, vals, n1, qs, 15)
        same(c.search(qs, 15), want)
        same(c.search(qs, 15, full=True), want)
        c.idx.reserve(8000)                                  # old rows kept, new rows empty
        assert c.idx.capacity >= 8000
        same(c.search(qs, 15), want)
        t, v = c.idx.sparse_gather(np.asarray([n1 - 1, 4000, 7999]))
        t = t.cpu().numpy().view(np.uint16)
        assert np.array_equal(t[0], terms[n1 - 1]) and (t[1:] == R.NONE).all()
        assert not v.cpu().numpy()[1:].any()
        assert np.array_equal(c.idx.sparse_df().cpu().numpy(), R.df(terms, n1))
    finally:
        c.idx.close()


# ------------------------------------------------------------------ 6. through QdrantClient
@pytest.fixture(scope="module")
def hybrid(gpu):
    """A 2,000-point Modifier.IDF collection (fp16 dense rows, 16 sparse slots, tickers A / B):
    the retrieval-quality corpus. Point ids are the rows."""
    from ragmi.qdrant import QdrantClient
    x, q, rows, rare, sq = R.quality_case()
    client = QdrantClient(device=gpu, coalesce=False)
    client.create_collection("h", m.VectorParams(size=DIM, distance=m.Distance.COSINE,
                                                 datatype=m.Datatype.FLOAT16),
                             sparse_vectors_config={"bm25": m.SparseVectorParams(
                                 modifier=m.Modifier.IDF)}, sparse_slots=16, capacity=2048)
    pts = [m.PointStruct(id=i, vector={"": x[i].tolist(), "bm25": sv(rows[i])},
                         payload={"ticker": "A" if i % 2 else "B"}) for i in range(len(rows))]
    for i in range(0, len(pts), 500):
        client.upsert("h", pts[i:i + 500])
    terms, vals, nnz = R.pack(rows, 16)
    yield client, x, q, rows, rare, sq, terms, vals, nnz
    client.close()


def idf_query(qi, qv, terms, nnz):
    return np.asarray(qi), R.idf_weights(qi, qv, R.df(terms, len(terms)), int((nnz > 0).sum()))


def test_client_sparse_queries_under_idf(hybrid):
    client, x, q, rows, rare, sq, terms, vals, nnz = hybrid
    n = len(rows)
    qs = R.queries(np.random.default_rng(1), rows, 6, 5) + [sq]
    got = client.query_points("h", query=sv(qs[0]), using="bm25", limit=20)
    want = R.topk(terms, vals, n, *idf_query(*qs[0], terms, nnz), 20)
    hits = int((want[1] >= 0).sum())
    assert [p.id for p in got.points] == want[1][:hits].tolist()
    assert np.array_equal(bits([p.score for p in got.points]), bits(want[0][:hits]))
    assert got.points[0].payload["ticker"] in ("A", "B")
    flt = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="A"))])
    either = m.Filter(should=[m.FieldCondition(key="ticker", match=m.MatchValue(value="A")),
                              m.FieldCondition(key="ticker", match=m.MatchValue(value="B"))])
    reqs = [m.QueryRequest(query=sv(qv), using="bm25", limit=5 + j,
                           filter=flt if j % 3 == 0 else either if j % 3 == 1 else None)
            for j, qv in enumerate(qs)]
    res = client.query_batch_points("h", reqs)
    odd = np.arange(n) % 2 == 1
    for j, (r, qv) in enumerate(zip(res, qs)):
        want = R.topk(terms, vals, n, *idf_query(*qv, terms, nnz), 5 + j,
                      odd if j % 3 == 0 else None)
        hits = int((want[1] >= 0).sum())
        assert [p.id for p in r.points] == want[1][:hits].tolist(), j
        assert np.array_equal(bits([p.score for p in r.points]), bits(want[0][:hits])), j
    rec = client.retrieve("h", [int(rare[0]), 5], with_vectors=True)
    assert rec[0].vector["bm25"] == SparseVector(
        indices=terms[rare[0]][:nnz[rare[0]]].astype(int).tolist(),
        values=vals[rare[0]][:nnz[rare[0]]].astype(float).tolist())
    assert rec[0].vector["bm25"].indices[-1] == R.RARE_TERM and len(rec[1].vector[""]) == DIM


def test_hybrid_fusion_equals_the_reference_and_finds_the_rare_term(hybrid):
    client, x, q, rows, rare, sq, terms, vals, nnz = hybrid
    n = len(rows)
    enc = O.encode_rows(x)
    dense_only = client.query_points("h", query=q.tolist(), limit=12)
    assert not {p.id for p in dense_only.points} & set(rare.tolist())
    pre = [m.Prefetch(query=q.tolist(), limit=50),
           m.Prefetch(query=sv(sq), using="bm25", limit=50)]
    got = client.query_points("h", query=m.FusionQuery(fusion=m.Fusion.RRF), prefetch=pre, limit=24)
    assert set(rare.tolist()) <= {p.id for p in got.points}
    _, dense = O.search(enc, q[None, :], 50)
    _, sparse = R.topk(terms, vals, n, *idf_query(*sq, terms, nnz), 50)
    want = F.rrf(np.stack([dense[0], sparse])[None], None, 24)
    assert [p.id for p in got.points] == want[1][0].tolist()
    assert np.array_equal(bits([p.score for p in got.points]), bits(want[0][0]))
    # a batch: several sparse prefetches ride one sparse search, under a filter and a cut
    qs = R.queries(np.random.default_rng(4), rows, 3, 4)
    flt = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="B"))])
    reqs = [m.QueryRequest(query=m.RrfQuery(rrf=m.Rrf(k=60)), limit=10, prefetch=[
        m.Prefetch(query=x[7 * j + 1].tolist(), filter=flt, limit=20),
        m.Prefetch(query=sv(qv), using="bm25", filter=flt, limit=8)]) for j, qv in enumerate(qs)]
    even = np.arange(n) % 2 == 0
    for j, (r, qv) in enumerate(zip(client.query_batch_points("h", reqs), qs)):
        ds, di = O.search(enc[even], x[7 * j + 1][None, :], 20)
        di = np.nonzero(even)[0][di[0]]
        _, sp = R.topk(terms, vals, n, *idf_query(*qv, terms, nnz), 8, even)
        cand = np.full((1, 2, 20), -1, np.int64)
        cand[0, 0], cand[0, 1, :8] = di, sp
        want = F.rrf(cand, None, 10, rrf_k=60)
        k = int((want[1][0] >= 0).sum())
        assert [p.id for p in r.points] == want[1][0][:k].tolist(), j
        assert np.array_equal(bits([p.score for p in r.points]), bits(want[0][0][:k])), j


def test_save_and_load_give_the_same_hits(hybrid, gpu, tmp_path):
    from ragmi.qdrant import QdrantClient
    client, x, q, rows, rare, sq, terms, vals, nnz = hybrid
    client.save(str(tmp_path))
    back = QdrantClient(device=gpu, path=str(tmp_path), coalesce=False)
    try:
        qs = R.queries(np.random.default_rng(9), rows, 4, 6) + [sq]
        for qv in qs:
            a = client.query_points("h", query=sv(qv), using="bm25", limit=30).points
            b = back.query_points("h", query=sv(qv), using="bm25", limit=30).points
            assert [(p.id, p.score) for p in a] == [(p.id, p.score) for p in b] and a
        pre = [m.Prefetch(query=q.tolist(), limit=50), m.Prefetch(query=sv(sq), using="bm25", limit=50)]
        a, b = (c.query_points("h", query=m.FusionQuery(fusion=m.Fusion.RRF), prefetch=pre,
                               limit=24).points for c in (client, back))
        assert [(p.id, p.score) for p in a] == [(p.id, p.score) for p in b]
        col = back._col("h")
        assert (col.sparse_name, col.sparse_idf, col.sparse_slots) == ("bm25", True, 16)
        assert col.sparse_len == nnz.tolist()
    finally:
        back.path = None
        back.close()


def test_delete_and_overwrite_through_the_client(gpu):
    """A delete moves sparse rows on the device with the host maps; an overwrite without a sparse
    entry empties the row; df follows both (the IDF cache is invalidated)."""
    from ragmi.qdrant import QdrantClient
    rng = np.random.default_rng(12)
    rows = R.zipf_rows(rng, 300, 16, 6, vocab=200, negative=0.0)
    x = rng.standard_normal((300, DIM)).astype(np.float32)
    client = QdrantClient(device=gpu, coalesce=False)
    try:
        client.create_collection("d", m.VectorParams(size=DIM, distance=m.Distance.COSINE),
                                 sparse_vectors_config={"s": m.SparseVectorParams(
                                     modifier=m.Modifier.IDF)}, sparse_slots=16, capacity=64)
        client.upsert("d", [m.PointStruct(id=1000 + i, vector={"": x[i].tolist(), "s": sv(rows[i])})
                            for i in range(300)])
        client.delete("d", [1000 + i for i in range(0, 300, 7)])
        client.upsert("d", [m.PointStruct(id=1001, vector=x[1].tolist())])      # loses its sparse row
        col = client._col("d")
        live = {pid: rows[pid - 1000] for pid in col.row_ids}
        live[1001] = (np.zeros(0, np.int64), np.zeros(0, np.float32))
        order = [live[pid] for pid in col.row_ids]
        terms, vals, nnz = R.pack(order, 16)
        assert col.sparse_len == nnz.tolist()
        for qv in R.queries(rng, rows, 5, 4):
            got = client.query_points("d", query=sv(qv), using="s", limit=25).points
            want = R.topk(terms, vals, len(order), *idf_query(*qv, terms, nnz), 25)
            hits = int((want[1] >= 0).sum())
            assert [p.id for p in got] == [col.row_ids[r] for r in want[1][:hits]]
            assert np.array_equal(bits([p.score for p in got]), bits(want[0][:hits]))
    finally:
        client.close()


def test_a_plain_collection_holds_no_sparse_column(gpu):
    from ragmi.qdrant import QdrantClient
    client = QdrantClient(device=gpu, coalesce=False)
    try:
        client.create_collection("p", m.VectorParams(size=DIM, distance=m.Distance.COSINE))
        client.upsert("p", [m.PointStruct(id=i, vector=np.eye(DIM, dtype=np.float32)[i].tolist())
                            for i in range(4)])
        client.delete("p", [0])
        assert client._col("p").index.sparse_slots() == 0
        with pytest.raises(ValueError, match="has no sparse vector"):
            client.query_points("p", query=SparseVector(indices=[1], values=[1.0]), using="bm25")
    finally:
        client.close()
