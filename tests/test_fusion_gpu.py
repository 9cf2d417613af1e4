"""GPU tests of fusion queries (rag_fuse_rrf / rrf_fuse_kernel, ragmi.index.fuse_rrf,
Collection.search_fusion behind QdrantClient.query_points / query_batch_points, ragmi.rag's
rewrites): fused scores bit-equal (as uint32), rows and counts equal to the restatement
tests/_fusion_ref.py — on synthetic int64 lists, on FlatIndex lists of the 3001-row corpus, and
through the client against the restatement applied to separate query_points calls."""
import numpy as np
import pytest
import torch

import _fusion_ref as F
import _mmr_ref as M
import oracle_scan as O

pytestmark = pytest.mark.gpu


def fused(gpu, rows, k, rrf_k=2, ncand=None):
    """fuse_rrf over host lists, back on the host: (scores, rows, count)."""
    from ragmi.index import fuse_rrf
    s, r, c = fuse_rrf(torch.as_tensor(rows, device=gpu), k, rrf_k, ncand, with_count=True)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy()


def same(got, want):
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(F.bits(got[0]), F.bits(want[0]))


# ------------------------------------------------------------------ 1. the kernel, synthetic lists
def test_one_pick_then_padding(gpu):
    rows = np.array([[[5]]], np.int64)
    got = fused(gpu, rows, 3)
    same(got, F.rrf(rows, None, 3))
    assert got[1].tolist() == [[5, -1, -1]] and got[2].tolist() == [1]
    assert got[0][0, 0] == np.float32(0.5) and np.isneginf(got[0][0, 1:]).all()
    # no count asked for; an empty list
    from ragmi.index import fuse_rrf
    s, r = fuse_rrf(torch.as_tensor([[[-1]]], device=gpu), 3)
    assert r.cpu().tolist() == [[-1, -1, -1]] and np.isneginf(s.cpu().numpy()).all()


def test_exact_tie_goes_to_the_smaller_row(gpu):
    rows = np.array([[[7, 9, 5], [9, 7, -1]], [[9, 7, 5], [7, 9, 3]]], np.int64)
    got = fused(gpu, rows, 6)
    same(got, F.rrf(rows, None, 6))
    assert got[1][0].tolist() == [7, 9, 5, -1, -1, -1]
    assert F.bits(got[0][0, 0]) == F.bits(got[0][0, 1])
    assert got[1][1].tolist() == [7, 9, 3, 5, -1, -1]      # 3 and 5 tie at 1 / 4 as well


def test_ragged_lists_and_a_cut(gpu):
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 400, (3, 3, 100)).astype(np.int64)
    rows[1, 0, 50] = -1                                     # ends its list mid-way
    ncand = np.array([[100, 37, 0], [100, 1, 100], [0, 0, 0]], np.int32)
    want = F.rrf(rows, ncand, 15)
    assert F.list_lengths(rows, ncand)[1].tolist() == [50, 1, 100] and want[2][2] == 0
    same(fused(gpu, rows, 15, ncand=ncand), want)
    same(fused(gpu, rows, 15, ncand=torch.as_tensor(ncand, device=gpu)), want)
    same(fused(gpu, rows, 15), F.rrf(rows, None, 15))
    # clamped counts: above C and below 0
    odd = np.array([[150, -4, 100]] * 3, np.int32)
    same(fused(gpu, rows, 40, ncand=odd), F.rrf(rows, odd, 40))
    for rrf_k in (1, 60, 2**31 - 1):
        same(fused(gpu, rows, 15, rrf_k, ncand), F.rrf(rows, ncand, 15, rrf_k))


def test_the_full_4096_entries(gpu):
    rng = np.random.default_rng(3)
    rows = np.empty((2, 16, 256), np.int64)
    rows[0] = rng.permutation(1 << 20)[:4096].reshape(16, 256)          # all distinct
    rows[1] = np.stack([rng.permutation(300)[:256] for _ in range(16)])  # heavily overlapping
    want = F.rrf(rows, None, 4096)
    assert want[2].tolist() == [4096, 300]
    got = fused(gpu, rows, 4096)
    same(got, want)
    # the prefix property, and determinism: a second launch gives equal bytes
    again = fused(gpu, rows, 4096)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    short = fused(gpu, rows, 15)
    assert np.array_equal(short[1], got[1][:, :15])
    assert np.array_equal(F.bits(short[0]), F.bits(got[0][:, :15]))


def test_lists_and_k_past_the_block(gpu):
    rng = np.random.default_rng(4)
    rows = rng.integers(0, 1500, (2, 4, 600)).astype(np.int64)
    rows[1] = np.stack([rng.permutation(5000)[:600] for _ in range(4)])
    ncand = np.array([[600, 513, 512, 1], [600, 600, 600, 600]], np.int32)
    same(fused(gpu, rows, 700, ncand=ncand), F.rrf(rows, ncand, 700))
    same(fused(gpu, rows, 5000), F.rrf(rows, None, 5000))   # k past L * C: padding only


def test_rows_around_2_to_the_40_and_a_duplicate(gpu):
    rng = np.random.default_rng(5)
    rows = (1 << 40) + rng.integers(-40, 40, (2, 3, 30)).astype(np.int64)
    rows[0, 1, :4] = [2**62, 0, 2**63 - 1, 2**31]
    rows[1, 0, 5] = rows[1, 0, 2]                           # the same row twice in one list
    want = F.rrf(rows, None, 90)
    same(fused(gpu, rows, 90), want)
    dup = np.array([[[4, 8, 4]]], np.int64)
    got = fused(gpu, dup, 3)
    same(got, F.rrf(dup, None, 3))
    assert got[1].tolist() == [[4, 8, -1]]
    assert F.bits(got[0][0, 0]) == F.bits(np.float32(1.0 / 2 + 1.0 / 4))


def test_many_requests_and_none(gpu):
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 50, (33, 3, 20)).astype(np.int64)
    ncand = rng.integers(0, 21, (33, 3)).astype(np.int32)
    same(fused(gpu, rows, 15, ncand=ncand), F.rrf(rows, ncand, 15))
    s, r, c = fused(gpu, np.empty((0, 3, 20), np.int64), 15)
    assert s.shape == (0, 15) and r.shape == (0, 15) and c.shape == (0,)
    assert s.dtype == np.float32 and r.dtype == np.int64 and c.dtype == np.int32


# ------------------------------------------------------------------ 2. through the index
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
def test_index_lists_fuse_as_the_restatement(gpu, storage):
    from ragmi.index import FlatIndex, fuse_rrf
    x, Q, _ = F.fusion_corpus()
    enc = M.encode(x, storage)
    ref_s, ref_r = O.search(enc, Q, F.LIST_LEN)
    idx = FlatIndex(F.DIM, len(x), gpu, storage=storage)
    try:
        idx.upsert(x, np.arange(len(x)), new_count=len(x))
        s, r = idx.search(Q, F.LIST_LEN)
        torch.cuda.synchronize()
        assert np.array_equal(r.cpu().numpy(), ref_r)
        assert np.array_equal(F.bits(s.cpu().numpy()), F.bits(ref_s))
        ncand = np.array([[50, 20, 35]], np.int32)
        for nc in (None, ncand):
            fs, fr, fc = fuse_rrf(r.reshape(1, 3, F.LIST_LEN), 15, ncand=nc, with_count=True)
            torch.cuda.synchronize()
            same((fs.cpu().numpy(), fr.cpu().numpy(), fc.cpu().numpy()),
                 F.rrf(ref_r[None], nc, 15))
    finally:
        idx.close()


# ------------------------------------------------------------------ 3. the client
def b32(x) -> int:
    return int(np.float32(x).view(np.uint32))


def payload_of(i, tickers):
    return {"ticker": tickers[i], "n": i}


def make_client(gpu, devices=None):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    x, _, tickers = F.fusion_corpus()
    c = QdrantClient(device=gpu, devices=devices)
    c.create_collection("t", m.VectorParams(size=F.DIM, distance=m.Distance.COSINE),
                        capacity=len(x))
    c.upsert("t", m.Batch(ids=list(range(len(x))), vectors=x,
                          payloads=[payload_of(i, tickers) for i in range(len(x))]))
    return c


@pytest.fixture(scope="module")
def client(gpu):
    c = make_client(gpu)
    yield c
    c.close()


def ticker(match):
    from ragmi import qdrant_models as m
    return m.Filter(must=[m.FieldCondition(key="ticker", match=match)])


def prefetches(variants=(0, 1, 2)):
    """Three prefetches of different limits: a MatchValue filter, a MatchAny filter (the
    program route), no filter; plus one on a never-ingested value (an empty list)."""
    from ragmi import qdrant_models as m
    Q = F.fusion_corpus()[1]
    a, b, c = variants
    return [m.Prefetch(query=Q[a].tolist(), limit=50, filter=ticker(m.MatchValue(value="AAA"))),
            m.Prefetch(query=m.NearestQuery(nearest=Q[b]), limit=20,
                       filter=ticker(m.MatchAny(any=["AAA", "BBB"]))),
            m.Prefetch(query=torch.as_tensor(Q[c]), limit=35),
            m.Prefetch(query=Q[a], limit=50, filter=ticker(m.MatchValue(value="ZZZ")))]


def expected(client, pres, limit, rrf_k=2, with_payload=True):
    """[(id, fused score bits, payload)]: the restatement over one query_points call per
    prefetch (ids are the rows' own numbers in this collection)."""
    tickers = F.fusion_corpus()[2]
    C = max(p.limit for p in pres)
    rows = np.full((1, len(pres), C), -1, np.int64)
    for l, p in enumerate(pres):
        pts = client.query_points("t", p.query, limit=p.limit, query_filter=p.filter).points
        rows[0, l, :len(pts)] = [pt.id for pt in pts]
    s, r, count = F.rrf(rows, None, limit, rrf_k)
    n = min(limit, int(count[0]))
    return [(int(r[0, t]), b32(s[0, t]),
             payload_of(int(r[0, t]), tickers) if with_payload else None) for t in range(n)]


def reported(res):
    return [(p.id, b32(p.score), p.payload) for p in res.points]


def test_client_fuses_as_separate_calls_would(gpu, client):
    from ragmi import qdrant_models as m
    rrf = m.FusionQuery(fusion=m.Fusion.RRF)
    pres = prefetches()
    want = expected(client, pres, 15)
    assert len(want) == 15
    col = client._col("t")
    rides = col.coalescer.requests
    got = client.query_points("t", rrf, prefetch=pres, limit=15)
    assert col.coalescer.requests == rides                   # a fusion request never coalesces
    assert isinstance(got, m.QueryResponse) and isinstance(got.points[0], m.ScoredPoint)
    assert reported(got) == want
    assert reported(client.query_points("t", rrf, prefetch=pres, limit=200)) == \
        expected(client, pres, 200)                          # past the distinct rows: no padding
    bare = client.query_points("t", rrf, prefetch=pres, limit=15, with_payload=False,
                               with_vectors=True)
    assert reported(bare) == expected(client, pres, 15, with_payload=False)
    assert len(bare.points[0].vector) == F.DIM
    # a single Prefetch is a list of one: the list itself, at scores 1 / (2 + p)
    one = client.query_points("t", rrf, prefetch=pres[0], limit=5)
    assert reported(one) == expected(client, pres[:1], 5)
    assert [p.score for p in one.points] == [float(np.float32(1.0 / (2 + p))) for p in range(5)]
    # Rrf(k=60) changes the scores as the restatement says
    k60 = client.query_points("t", m.RrfQuery(rrf=m.Rrf(k=60)), prefetch=pres, limit=15)
    assert reported(k60) == expected(client, pres, 15, rrf_k=60) and reported(k60) != want
    # only empty lists
    assert client.query_points("t", rrf, prefetch=pres[3:], limit=15).points == []


def test_batch_mixes_fusion_plain_and_mmr(gpu, client):
    from ragmi import qdrant_models as m
    Q = F.fusion_corpus()[1]
    rrf = m.FusionQuery(fusion=m.Fusion.RRF)
    reqs = [m.QueryRequest(query=rrf, prefetch=prefetches(), limit=15),
            m.QueryRequest(query=Q[1].tolist(), limit=7, filter=ticker(m.MatchValue(value="BBB"))),
            m.QueryRequest(query=m.RrfQuery(rrf=m.Rrf(k=60)), prefetch=prefetches((2, 0, 1))[:2],
                           limit=30, with_payload=False),
            m.QueryRequest(query=m.NearestQuery(nearest=Q[2].tolist(),
                                                mmr=m.Mmr(diversity=0.5, candidates_limit=40)),
                           limit=10),
            m.QueryRequest(query=rrf, prefetch=prefetches((1, 2, 0))[1:], limit=4)]
    got = client.query_batch_points("t", reqs)
    assert len(got) == len(reqs)
    for r, g in zip(reqs, got):
        alone = client.query_points("t", r.query, limit=r.limit, query_filter=r.filter,
                                    with_payload=r.with_payload, prefetch=r.prefetch)
        assert reported(g) == reported(alone) and len(g.points) == r.limit
    assert reported(got[0]) == expected(client, reqs[0].prefetch, 15)
    assert reported(got[2]) == expected(client, reqs[2].prefetch, 30, 60, with_payload=False)
    assert reported(got[4]) == expected(client, reqs[4].prefetch, 4)
    only = client.query_batch_points("t", [reqs[4], reqs[0]])
    assert [reported(g) for g in only] == [reported(got[4]), reported(got[0])]


def test_three_logical_shards_return_the_same_points(gpu, client):
    from ragmi import qdrant_models as m
    rrf = m.FusionQuery(fusion=m.Fusion.RRF)
    sharded = make_client(gpu, devices=[gpu.index] * 3)
    try:
        for q, lim in ((rrf, 15), (m.RrfQuery(rrf=m.Rrf(k=60)), 120)):
            a = client.query_points("t", q, prefetch=prefetches(), limit=lim)
            b = sharded.query_points("t", q, prefetch=prefetches(), limit=lim)
            assert reported(a) == reported(b) and len(a.points) > 0
    finally:
        sharded.close()


def test_rag_rewrites(gpu, client, monkeypatch):
    from ragmi import qdrant_models as m
    from ragmi import rag
    Q = F.fusion_corpus()[1]
    monkeypatch.setenv("TESTING", "False")
    monkeypatch.setattr(rag, "COLLECTION_NAME", "t")
    monkeypatch.setattr(rag, "get_qdrant", lambda: client)
    flt = rag._filter("aaa")
    pres = [m.Prefetch(query=v, filter=flt, limit=50) for v in Q]
    want = client.query_points("t", m.FusionQuery(fusion=m.Fusion.RRF), prefetch=pres, limit=15)
    got = rag.retrieve_from_qdrant(Q[0], "aaa", rewrites=[Q[1], Q[2]])
    assert reported(got) == reported(want) == expected(client, pres, 15)
    assert all(p.payload["ticker"] == "AAA" for p in got.points)
    k60 = rag.retrieve_from_qdrant(Q[0], "aaa", rewrites=[Q[1], Q[2]], rrf_k=60, limit=60)
    assert reported(k60) == expected(
        client, [m.Prefetch(query=v, filter=flt, limit=60) for v in Q], 60, 60)
    # rewrites=None is today's call
    plain = client.query_points("t", Q[0], limit=15, query_filter=flt)
    assert reported(rag.retrieve_from_qdrant(Q[0], "aaa")) == reported(plain)
    assert reported(rag.retrieve_from_qdrant(Q[0], "aaa", rewrites=None)) == reported(plain)
    both = rag.retrieve_batch([Q[0], Q[1]], ["aaa", ["aaa", "bbb"]], rewrites=[[Q[1], Q[2]], []])
    assert reported(both[0]) == reported(want)
    any_flt = rag._filter(["aaa", "bbb"])
    assert reported(both[1]) == expected(
        client, [m.Prefetch(query=Q[1], filter=any_flt, limit=50)], 15)
    today = rag.retrieve_batch([Q[0], Q[1]], ["aaa", "bbb"])
    assert reported(today[0]) == reported(plain) and len(today[1].points) == 15
