"""GPU tests of MMR search (rag_index_mmr / mmr_kernel, FlatIndex.search_mmr, ShardSet.mmr and
QdrantClient's NearestQuery path): ids, scores and positions bit for bit against the numpy
restatement tests/_mmr_ref.py on the seed-7 corpus of near-duplicate groups (3001 rows: the
tile tail; 4 identical rows per group: exact `val` ties)."""
import functools

import numpy as np
import pytest
import torch

import _mmr_ref as R

pytestmark = pytest.mark.gpu

DIVS = (0.0, 0.3, 0.5, 0.8, 1.0)


@functools.lru_cache(maxsize=None)
def corpus(D):
    return R.grouped_corpus(D)


@functools.lru_cache(maxsize=None)
def stored(D, storage):
    return R.encode(corpus(D)[0], storage)


_indexes = {}


def index_of(gpu, D, storage):
    """One FlatIndex per (D, storage) for the module; tag 2 on five rows, 1 elsewhere."""
    from ragmi.index import FlatIndex
    key = (D, storage)
    if key not in _indexes:
        x = corpus(D)[0]
        idx = FlatIndex(D, len(x), gpu, storage=storage)
        idx.upsert(x, np.arange(len(x)), row_tags(), new_count=len(x))
        _indexes[key] = idx
    return _indexes[key]


def row_tags():
    tags = np.ones(R.N_ROWS, np.uint32)
    tags[[5, 16, 17, 1500, 3000]] = 2
    return tags


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    """(scores, rows[, positions]) device tensors against the restatement, bit for bit."""
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        g = g.cpu().numpy()
        if g.dtype == np.float32:
            assert np.array_equal(bits(g), bits(w))
        else:
            assert np.array_equal(g, w)


# ------------------------------------------------------------------ 1. bit-exact vs the restatement
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
@pytest.mark.parametrize("D", [384, 1024])
def test_mmr_matches_the_restatement(gpu, D, storage):
    idx = index_of(gpu, D, storage)
    enc = stored(D, storage)
    q = np.stack([corpus(D)[1]] * 5)
    # C = 100 (the large-k route; 12 rounds of 8 candidates and a ragged 4), k = 12
    stats = {}
    want = R.search_mmr(enc, q, 12, DIVS, 100, stats=stats)
    assert stats["ties"] > 0                     # identical rows: exact val ties, smaller j wins
    cs, cr = idx.search(q, 100)
    same((cs, cr), want[3:])
    same(idx.mmr(cs, cr, 12, DIVS, with_pos=True), want[:3])
    same(idx.search_mmr(q, 12, DIVS, 100), want[:2])
    group = corpus(D)[2]
    assert len(set(group[want[1][0]].tolist())) == 2 and \
        sorted(group[want[1][2]].tolist()) == list(range(12))     # what MMR is for
    # per-query candidate counts: padding past 8 and 1 picks
    ncand = (100, 37, 8, 100, 1)
    want_n = R.mmr(enc, want[3], want[4], 12, DIVS, ncand)
    assert (want_n[1][2, 8:] == -1).all() and (want_n[1][4, 1:] == -1).all()
    same(idx.mmr(cs, cr, 12, DIVS, ncand, with_pos=True), want_n)
    same(idx.search_mmr(q, 12, DIVS, ncand), want_n[:2])
    # C = 20 (the scan route), k = 20: the list is exhausted, every candidate picked once
    want20 = R.search_mmr(enc, q, 20, DIVS, 20)
    assert all(sorted(p) == list(range(20)) for p in want20[2].tolist())
    c20 = idx.search(q, 20)
    same(c20, want20[3:])
    same(idx.mmr(*c20, 20, DIVS, with_pos=True), want20[:3])
    # C = 1, k = 3: one pick, then padding
    want1 = R.search_mmr(enc, q, 3, DIVS, 1)
    same(idx.mmr(*idx.search(q, 1), 3, DIVS, with_pos=True), want1[:3])
    assert want1[2].tolist() == [[0, -1, -1]] * 5


def test_more_candidates_and_picks_than_threads(gpu):
    """C = 600 and k = 600 pass the workgroup's 512 threads: the list set-up and the padding
    take a second trip, every candidate is picked once, and ncand = 20 pads 580 slots."""
    idx = index_of(gpu, 384, "fp16")
    q = np.stack([corpus(384)[1]] * 2)
    want = R.search_mmr(stored(384, "fp16"), q, 600, (0.5, 0.7), (600, 20))
    assert sorted(want[2][0].tolist()) == list(range(600))
    assert (want[2][1, 20:] == -1).all() and sorted(want[2][1, :20].tolist()) == list(range(20))
    cs, cr = idx.search(q, 600)
    same((cs, cr), want[3:])
    same(idx.mmr(cs, cr, 600, (0.5, 0.7), (600, 20), with_pos=True), want[:3])


def test_rows_outside_capacity_end_the_list(gpu):
    idx = index_of(gpu, 384, "fp16")
    enc = stored(384, "fp16")
    q = corpus(384)[1][None]
    cs, cr = idx.search(q, 20)
    torch.cuda.synchronize()
    cr = cr.clone()
    cr[0, 9] = idx.capacity                      # absent: never dereferenced, ends the list
    cr[0, 12] = -1
    want = R.mmr(enc, cs.cpu().numpy(), np.where(np.arange(20) == 9, -1, cr.cpu().numpy()),
                 12, 0.5)
    assert (want[1][0, :9] >= 0).all() and (want[1][0, 9:] == -1).all()
    same(idx.mmr(cs, cr, 12, 0.5, with_pos=True), want)
    with pytest.raises(ValueError):
        idx.mmr(cs, cr, 12, 1.5)
    with pytest.raises(ValueError):
        idx.search_mmr(q, 5, 0.5, 2000)


# ------------------------------------------------------------------ 2. diversity 0, padding
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
def test_diversity_zero_is_search_and_filter_padding(gpu, storage):
    idx = index_of(gpu, 384, storage)
    q = np.stack([corpus(384)[1], corpus(384)[0][7] + 0.1])
    for k, C in ((12, 100), (20, 20), (32, 64)):
        s, i = idx.search(q, k)
        same(idx.search_mmr(q, k, 0.0, C), (s.cpu().numpy(), i.cpu().numpy()))
    # a filter that leaves 5 rows: 5 hits, then -1 / -inf
    filt = np.array([[0xFFFF, 2], [0xFFFF, 2]], np.uint32)
    want = R.search_mmr(stored(384, storage), q, 12, [0.5, 0.9], 100, tags=row_tags(),
                        filters=filt)
    assert sorted(want[1][0, :5].tolist()) == [5, 16, 17, 1500, 3000]
    assert (want[1][:, 5:] == -1).all() and np.isneginf(want[0][:, 5:]).all()
    same(idx.search_mmr(q, 12, [0.5, 0.9], 100, filters=filt), want[:2])


# ------------------------------------------------------------------ 3. prefix property
@pytest.mark.parametrize("D,storage", [(384, "fp32"), (1024, "fp16")])
def test_prefix_property(gpu, D, storage):
    idx = index_of(gpu, D, storage)
    q = np.stack([corpus(D)[1]] * 5)
    s12, i12 = idx.search_mmr(q, 12, DIVS, 100)
    s5, i5 = idx.search_mmr(q, 5, DIVS, 100)
    torch.cuda.synchronize()
    assert torch.equal(i12[:, :5], i5) and torch.equal(s12[:, :5], s5)


# ------------------------------------------------------------------ 4. QdrantClient parity
TICKERS = ("AMD", "AAPL", "MSFT")


def payload_of(i):
    return {"ticker": TICKERS[i % 3], "document_type": "10-K", "n": int(i)}


def make_client(gpu, devices=None):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    x = corpus(384)[0]
    c = QdrantClient(device=gpu, devices=devices)
    c.create_collection("t", m.VectorParams(size=384, distance=m.Distance.COSINE),
                        capacity=len(x))
    c.upsert("t", m.Batch(ids=list(range(len(x))), vectors=x,
                          payloads=[payload_of(i) for i in range(len(x))]))
    return c


def ticker_filter(t):
    from ragmi import qdrant_models as m
    return m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value=t))])


def expected_points(enc, ids_of_row, q, limit, mmr, ticker):
    """[(id, score, payload)] the client must report: the restatement (or the plain oracle
    search when `mmr` is None) over stored rows `enc`, whose row r holds point ids_of_row[r]."""
    import oracle_scan as O
    ids_of_row = np.asarray(ids_of_row)
    tags = (ids_of_row % 3 + 1).astype(np.uint32)
    filt = None if ticker is None else [(0xFFFF, TICKERS.index(ticker) + 1)]
    if mmr is None:
        s, r = O.search(enc, q[None], limit, tags=tags, mask=filt[0][0] if filt else 0,
                        value=filt[0][1] if filt else 0, use_filter=filt is not None)
    else:
        div, cand = mmr
        s, r = R.search_mmr(enc, q[None], limit, div, min(cand, len(enc)), tags=tags,
                            filters=filt)[:2]
    return [(int(ids_of_row[row]), float(sc), payload_of(ids_of_row[row]))
            for sc, row in zip(s[0], r[0]) if row >= 0]


def reported(resp):
    return [(p.id, p.score, p.payload) for p in resp.points]


def batch_requests(q):
    from ragmi import qdrant_models as m
    spec = [(7, None, None), (10, (0.5, 50), "AMD"), (12, (0.8, None), None),
            (40, None, "AMD"), (20, (1.0, 20), None)]
    reqs = [m.QueryRequest(
        query=q if mm is None else m.NearestQuery(
            nearest=q.tolist(), mmr=m.Mmr(diversity=mm[0], candidates_limit=mm[1])),
        limit=limit, filter=None if t is None else ticker_filter(t)) for limit, mm, t in spec]
    return spec, reqs


def test_client_parity_single_and_sharded(gpu):
    from ragmi import qdrant_models as m
    enc = stored(384, "fp32")                    # VectorParams' default datatype
    q = corpus(384)[1]
    ids = np.arange(len(enc))
    single = make_client(gpu)
    sharded = make_client(gpu, devices=[gpu.index] * 3)
    try:
        want = expected_points(enc, ids, q, 10, (0.5, 50), "AMD")
        assert len(want) == 10
        for c in (single, sharded):
            got = c.query_points("t", m.NearestQuery(nearest=q, mmr=m.Mmr(0.5, 50)), limit=10,
                                 query_filter=ticker_filter("AMD"))
            assert reported(got) == want
        # defaults: diversity 0.5, candidates max(limit, 100)
        want = expected_points(enc, ids, q, 12, (0.5, 100), None)
        assert len({p["n"] for _, _, p in want}) == 12
        for c in (single, sharded):
            assert reported(c.query_points("t", m.NearestQuery(nearest=q, mmr=m.Mmr()),
                                           limit=12)) == want
        spec, reqs = batch_requests(q)
        outs = [c.query_batch_points("t", reqs) for c in (single, sharded)]
        for j, (limit, mm, t) in enumerate(spec):
            want = expected_points(enc, ids, q, limit,
                                   None if mm is None else (mm[0], mm[1] or 100), t)
            assert len(want) == limit
            assert reported(outs[0][j]) == want and reported(outs[1][j]) == want
    finally:
        single.close()
        sharded.close()


# ------------------------------------------------------------------ 5. after a delete
def test_mmr_after_deleting_a_group(gpu):
    from ragmi import qdrant_models as m
    enc = stored(384, "fp32")
    q = corpus(384)[1]
    group = corpus(384)[2]
    gone = np.nonzero(group == 0)[0].tolist()
    for devices in (None, [gpu.index] * 3):
        c = make_client(gpu, devices)
        try:
            c.delete("t", gone)
            col = c._col("t")
            ids_of_row = np.asarray(col.row_ids)
            assert len(ids_of_row) == len(enc) - 9 and (ids_of_row[:2900] != np.arange(2900)).any()
            after = np.ascontiguousarray(enc[ids_of_row])        # rows moved bit for bit
            want = expected_points(after, ids_of_row, q, 12, (0.5, 100), None)
            got = c.query_points("t", m.NearestQuery(nearest=q, mmr=m.Mmr(0.5, 100)), limit=12)
            assert reported(got) == want
            assert set(range(1, 12)) <= set(group[[i for i, _, _ in want]].tolist())
            want = expected_points(after, ids_of_row, q, 10, (0.7, 60), "MSFT")
            got = c.query_points("t", m.NearestQuery(nearest=q, mmr=m.Mmr(0.7, 60)), limit=10,
                                 query_filter=ticker_filter("MSFT"))
            assert reported(got) == want and all(p["ticker"] == "MSFT" for _, _, p in want)
        finally:
            c.close()
