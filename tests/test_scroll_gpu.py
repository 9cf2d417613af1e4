"""GPU tests of QdrantClient.scroll, the OrderByQuery route and rag_index_select_rows_from
(DESIGN.md §R16): a 12293-point collection (three select chunks plus 5) with md5 and int ids,
paged to the end with and without filters; ordered scrolls on a datetime field against the
lexsort of (key_of(payload), row); the batch route. Exact throughout."""
import datetime as dt
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 12293
UTC = dt.timezone.utc
T0 = dt.datetime(2024, 3, 1, tzinfo=UTC)
TICKERS = [f"T{i:02d}" for i in range(9)]


def point_id(i):
    i = int(i)
    return hashlib.md5(f"doc-{i}".encode()).hexdigest() if i % 2 else i


def payload_of(i):
    i = int(i)
    p = {"ticker": TICKERS[(i * 5) % 9], "document_type": ("10-K", "10-Q", "8-K")[i % 3]}
    if i % 7:            # every seventh point lacks the field; seconds repeat, so keys tie
        p["ingested_at"] = (T0 + dt.timedelta(seconds=(i * 37) % 500)).isoformat()
    return p


@pytest.fixture(scope="module")
def served(gpu):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    client = QdrantClient(device=gpu)
    client.create_collection("docs", m.VectorParams(size=384, distance=m.Distance.COSINE),
                             capacity=N, payload_range_fields={"ingested_at": "datetime"})
    vec = np.random.default_rng(3).standard_normal((N, 384)).astype(np.float32)
    for r0 in range(0, N, 4000):
        ids = [point_id(i) for i in range(r0, min(N, r0 + 4000))]
        client.upsert("docs", m.Batch(ids=ids, vectors=vec[r0:r0 + len(ids)],
                                      payloads=[payload_of(i) for i in range(r0, r0 + len(ids))]))
    yield client, client._col("docs"), vec
    client.close()


def must(key, value):
    from ragmi import qdrant_models as m
    return m.Filter(must=[m.FieldCondition(key=key, match=m.MatchValue(value=value))])


def canon(i):
    from ragmi.collection import _norm_id
    return _norm_id(point_id(i))


def page_through(client, limit, flt=None):
    ids, sizes, offset = [], [], None
    while True:
        recs, offset = client.scroll("docs", scroll_filter=flt, limit=limit, offset=offset)
        ids += [r.id for r in recs]
        sizes.append(len(recs))
        if offset is None:
            return ids, sizes


def test_select_rows_from_matches_numpy(served):
    from ragmi.filters import FilterProgram, eval_view_np, pack_view
    _, col, _ = served
    idx = col.index
    tags = idx.export_tags(0, N)
    blob = pack_view([FilterProgram.maskeq(0xFFFF, 3)])
    passing = np.nonzero(eval_view_np(blob, tags, 1) & 1)[0]
    for row0 in (0, 1, 4095, 4096, 4097, 8192, N - 5, N - 1, N, N + 100):
        for programs, want in ((None, np.arange(N)), (blob, passing)):
            want = want[want >= row0]
            for cap in (None, 0, 7, 4097):
                rows, total = idx.select_rows_from(row0, programs, cap=cap)
                assert total == want.size
                np.testing.assert_array_equal(rows.cpu().numpy(),
                                              want if cap is None else want[:cap])
    # the calls it generalises are unchanged
    rows, total = idx.select_rows_view(blob)
    np.testing.assert_array_equal(rows.cpu().numpy(), passing)
    rows, total = idx.select_rows(0xFFFF, 3)
    np.testing.assert_array_equal(rows.cpu().numpy(), passing)
    st = torch.cuda.current_stream(idx.device).cuda_stream
    n = torch.zeros(1, dtype=torch.int64, device=idx.device)
    assert idx._L.rag_index_select_rows_from(idx._h, None, 0, -1, None, 0, n.data_ptr(), st) == -1


def test_scroll_round_trip(served):
    client, col, _ = served
    every = [canon(i) for i in range(N)]
    ids, sizes = page_through(client, 4096)                 # limit + 1 at every chunk border
    assert ids == every and sizes == [4096, 4096, 4096, 5]
    ids, sizes = page_through(client, 12288)                # a page that ends at the last row
    assert ids == every and sizes == [12288, 5]
    recs, nxt = client.scroll("docs", limit=N)              # ... exactly
    assert len(recs) == N and nxt is None
    recs, nxt = client.scroll("docs", limit=5, offset=canon(N - 5))
    assert [r.id for r in recs] == every[-5:] and nxt is None
    # md5 ids are accepted as given and reported back in canonical form; payloads ride along
    recs, nxt = client.scroll("docs", limit=3, offset=point_id(4097))
    assert [r.id for r in recs] == every[4097:4100] and nxt == every[4100]
    assert [r.payload for r in recs] == [payload_of(i) for i in range(4097, 4100)]
    for flt, keep in ((must("ticker", "T03"), lambda i: (i * 5) % 9 == 3),
                      (_not_10k(), lambda i: i % 3 != 0)):
        want = [canon(i) for i in range(N) if keep(i)]
        for limit in (1000, 4096):
            ids, sizes = page_through(client, limit, flt)
            assert ids == want and len(set(ids)) == len(ids)
            assert sizes == [limit] * (len(want) // limit) + [len(want) % limit]
    recs, _ = client.scroll("docs", limit=2, with_payload=False, with_vectors=True)
    assert recs[0].payload is None and len(recs[0].vector) == 384


def _not_10k():
    from ragmi import qdrant_models as m
    return m.Filter(must_not=[m.FieldCondition(key="document_type",
                                               match=m.MatchValue(value="10-K"))])


def want_ordered(col, desc, keep=lambda i: True, lo=None, hi=None):
    """Rows by the lexsort of (key_of(payload), row) over the points that hold the field."""
    rows = np.array([i for i in range(N) if i % 7 and keep(i)], np.int64)
    keys = np.array([col.ranges.key_of("ingested_at", payload_of(i)["ingested_at"])
                     for i in rows], np.int64)
    ok = np.ones(rows.shape, bool)
    if lo is not None:
        ok &= keys >= lo
    if hi is not None:
        ok &= keys <= hi
    rows, keys = rows[ok], keys[ok]
    return rows[np.lexsort((rows, -keys if desc else keys))]


def test_ordered_scroll_on_a_datetime_field(served):
    from ragmi import qdrant_models as m
    client, col, _ = served
    for desc in (False, True):
        order = m.OrderBy("ingested_at", m.Direction.DESC if desc else m.Direction.ASC)
        for limit in (15, 4096):
            recs, nxt = client.scroll("docs", limit=limit, order_by=order)
            want = want_ordered(col, desc)[:limit]
            assert nxt is None and [r.id for r in recs] == [canon(i) for i in want]
            assert [r.order_value for r in recs] == [payload_of(i)["ingested_at"] for i in want]
        recs, _ = client.scroll("docs", scroll_filter=must("ticker", "T03"), limit=50,
                                order_by=order)
        want = want_ordered(col, desc, lambda i: (i * 5) % 9 == 3)[:50]
        assert [r.id for r in recs] == [canon(i) for i in want]
        # start_from, inclusive, as a string and as a datetime
        cut = T0 + dt.timedelta(seconds=250)
        key = col.ranges.key_of("ingested_at", cut)
        want = want_ordered(col, desc, lo=None if desc else key, hi=key if desc else None)[:300]
        assert payload_of(int(want[0]))["ingested_at"] == cut.isoformat()        # inclusive
        for start in (cut.isoformat(), cut):
            recs, _ = client.scroll("docs", limit=300, order_by=m.OrderBy(
                "ingested_at", order.direction, start_from=start))
            assert [r.id for r in recs] == [canon(i) for i in want]
    recs, _ = client.scroll("docs", limit=5, order_by="ingested_at")            # a bare name
    assert [r.id for r in recs] == [canon(i) for i in want_ordered(col, False)[:5]]


def test_order_by_query_and_batch(served):
    from ragmi import qdrant_models as m
    client, col, vec = served
    order = m.OrderBy("ingested_at", m.Direction.DESC)
    recs, _ = client.scroll("docs", scroll_filter=_not_10k(), limit=40, order_by=order)
    res = client.query_points("docs", query=m.OrderByQuery(order), query_filter=_not_10k(),
                              limit=40)
    assert [p.id for p in res.points] == [r.id for r in recs]
    assert all(p.score == 0.0 and p.order_value == r.order_value and p.payload == r.payload
               for p, r in zip(res.points, recs))
    # a batch mixing order requests with plain ones: each answer in its slot
    reqs = [m.QueryRequest(query=vec[17].tolist(), limit=3),
            m.QueryRequest(query=m.OrderByQuery(order), filter=_not_10k(), limit=40),
            m.QueryRequest(query=vec[4100].tolist(), limit=2, filter=must("ticker", "T07")),
            m.QueryRequest(query=m.OrderByQuery("ingested_at"), limit=5)]
    out = client.query_batch_points("docs", reqs)
    assert out[0].points[0].id == canon(17) and len(out[0].points) == 3
    assert [p.id for p in out[1].points] == [r.id for r in recs]
    assert out[2].points[0].id == canon(4100) and len(out[2].points) == 2
    assert all(p.payload["ticker"] == "T07" for p in out[2].points)
    assert [p.id for p in out[3].points] == [canon(i) for i in want_ordered(col, False)[:5]]
    assert all(p.order_value is None for p in out[0].points + out[2].points)


def test_scroll_after_a_delete(served):
    """Storage order after a delete: tail rows sit in the holes, and paging still visits every
    remaining point exactly once. Runs last: it changes the collection."""
    from ragmi import qdrant_models as m
    client, col, _ = served
    gone = [point_id(i) for i in range(0, 600, 2)]
    client.delete("docs", m.PointIdsList(points=gone))
    left = {canon(i) for i in range(N)} - {canon(i) for i in range(0, 600, 2)}
    ids, _ = page_through(client, 4096)
    assert ids == col.row_ids and set(ids) == left and len(ids) == len(left)
    recs, _ = client.scroll("docs", limit=15, order_by="ingested_at")
    rows = np.arange(len(col.row_ids))
    keys = np.array([col.ranges.keys(p)[0] for p in col.payloads], np.int64)
    from ragmi.filters import KEY_ABSENT
    ok = keys != KEY_ABSENT
    want = rows[ok][np.lexsort((rows[ok], keys[ok]))][:15]
    assert [r.id for r in recs] == [col.row_ids[r] for r in want]
