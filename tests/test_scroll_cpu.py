"""CPU tests of scroll, order_by and facet: the models and their defaults, the
ORDER route, every refusal with its message, the numpy restatements of the two kernels against
hand-written cases, and a Collection over a protocol fake built on those restatements driven
through scroll, both routes of query_points and facet. No device code runs here."""
import datetime as dt
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

UTC = dt.timezone.utc


# ------------------------------------------------------------------ models and route
def test_models_and_defaults():
    from ragmi import qdrant_models as m
    assert m.Direction.ASC.value == "asc" and m.Direction.DESC.value == "desc"
    ob = m.OrderBy(key="ingested_at")
    assert ob.direction is None and ob.start_from is None
    assert m.OrderByQuery(order_by="x").order_by == "x"
    assert m.OrderByQuery(order_by=ob).order_by is ob
    hit = m.FacetValueHit(value="AAPL", count=3)
    assert (hit.value, hit.count) == ("AAPL", 3)
    assert m.FacetResponse().hits == []
    assert m.ScoredPoint(id=1, version=0, score=0.0).order_value is None
    assert m.Record(id=1).order_value is None


def test_route_of_order_by_query():
    from ragmi import qdrant as q
    m = q.models
    assert q.ORDER == "order"
    assert q.route_of(m.OrderByQuery(order_by="year")) == q.ORDER
    # with a prefetch it still goes to ORDER, to be refused there
    assert q.route_of(m.OrderByQuery(order_by="year"), prefetch=[m.Prefetch(query=[0.0])]) == q.ORDER
    assert q.route_of([0.0, 1.0]) == q.PLAIN
    assert q.route_of(m.FormulaQuery(formula=1.0)) == q.FORMULA


def test_header_declares_the_three_calls():
    text = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    for name in ("rag_index_order_rows", "rag_index_facet_counts", "rag_index_select_rows_from"):
        assert re.search(rf"^int {name}\(", text, re.M), name
    assert re.search(r"^#define RAG_ORDER_MAX 4096$", text, re.M)
    assert re.search(r"^#define RAG_ORDER_DESC 1$", text, re.M)
    from ragmi import _lib, index
    assert index.ORDER_MAX == 4096 and index.ORDER_DESC == 1
    assert {"rag_index_order_rows", "rag_index_facet_counts",
            "rag_index_select_rows_from"} <= set(_lib.INDEX_API)


# ------------------------------------------------------------------ the numpy restatements
def test_order_rows_np_hand_cases():
    from ragmi.filters import KEY_ABSENT
    from ragmi.index import order_rows_np
    A = KEY_ABSENT
    keys = np.array([5, 3, A, 3, 9, -7, 3, 5], np.int64)
    k, r, n = order_rows_np(keys, 4)
    assert (k.tolist(), r.tolist(), n) == ([-7, 3, 3, 3], [5, 1, 3, 6], 7)
    k, r, n = order_rows_np(keys, 4, desc=True)                 # key desc, row ASC among ties
    assert (k.tolist(), r.tolist(), n) == ([9, 5, 5, 3], [4, 0, 7, 1], 7)
    k, r, n = order_rows_np(keys, 100)
    assert (r.tolist(), n) == ([5, 1, 3, 6, 0, 7, 4], 7)         # the absent key is left out
    k, r, n = order_rows_np(keys, 10, lo=3, hi=5)                 # both bounds inclusive
    assert (k.tolist(), r.tolist(), n) == ([3, 3, 3, 5, 5], [1, 3, 6, 0, 7], 5)
    assert order_rows_np(keys, 10, lo=6, hi=5)[2] == 0            # lo > hi: empty
    passing = np.array([1, 0, 1, 1, 0, 1, 1, 1], bool)
    k, r, n = order_rows_np(keys, 3, passing=passing)
    assert (k.tolist(), r.tolist(), n) == ([-7, 3, 3], [5, 3, 6], 5)
    # the extremes of int64 order correctly in both directions
    ext = np.array([np.iinfo(np.int64).max, A + 1, 0], np.int64)
    assert order_rows_np(ext, 3)[1].tolist() == [1, 2, 0]
    assert order_rows_np(ext, 3, desc=True)[1].tolist() == [0, 2, 1]
    assert order_rows_np(np.empty(0, np.int64), 5) [2] == 0


def test_facet_counts_np_hand_cases():
    from ragmi.index import facet_counts_np
    tags = np.array([1, 2, 2, 0, 3 | (1 << 16), 2 | (2 << 16), 7], np.uint32)
    assert facet_counts_np(tags, 0, 3).tolist() == [1, 1, 3, 1]        # code 7 > n_codes: dropped
    assert facet_counts_np(tags, 0, 7).tolist() == [1, 1, 3, 1, 0, 0, 0, 1]
    assert facet_counts_np(tags, 1, 2).tolist() == [5, 1, 1]
    assert facet_counts_np(tags, 0, 0).tolist() == [1]
    passing = np.array([1, 1, 0, 0, 1, 1, 1], bool)
    assert facet_counts_np(tags, 0, 3, passing).tolist() == [0, 1, 2, 1]
    assert facet_counts_np(np.empty(0, np.uint32), 1, 4).tolist() == [0] * 5


# ------------------------------------------------------------------ a protocol fake
class FakeIndex:
    """The slice of the index protocol the payload queries use, over host arrays and the numpy
    restatements (eval_view_np, order_rows_np, facet_counts_np). Counts its launches."""
    storage = "fp32"
    device = torch.device("cpu")

    def __init__(self):
        self.tags = np.zeros(0, np.uint32)
        self.keys = np.zeros((0, 0), np.int64)
        self.count = 0
        self.calls = []

    capacity = 1 << 20

    def reserve(self, capacity):
        pass

    def keys_create(self, n_cols):
        from ragmi.filters import KEY_ABSENT
        grown = np.full((n_cols, self.keys.shape[1]), KEY_ABSENT, np.int64)
        grown[:self.keys.shape[0]] = self.keys
        self.keys = grown

    def upsert(self, vectors, rows, tags=None, new_count=None):
        from ragmi.filters import KEY_ABSENT
        if new_count > self.count:
            self.tags = np.concatenate([self.tags, np.zeros(new_count - self.count, np.uint32)])
            pad = np.full((self.keys.shape[0], new_count - self.count), KEY_ABSENT, np.int64)
            self.keys = np.concatenate([self.keys, pad], axis=1)
            self.count = new_count
        self.tags[rows] = tags

    def write_keys(self, col, rows, keys):
        self.keys[col, rows] = keys

    def _passing(self, programs):
        from ragmi.filters import eval_view_np
        if programs is None:
            return None
        return (eval_view_np(programs, self.tags, 1, keys=self.keys) & 1).astype(bool)

    def select_rows_from(self, row0, programs=None, cap=None):
        self.calls.append(("select_rows_from", row0, cap))
        ok = self._passing(programs)
        rows = np.arange(self.count) if ok is None else np.nonzero(ok)[0]
        rows = rows[rows >= row0].astype(np.int64)
        return torch.from_numpy(rows[:cap]), int(rows.size)

    def order_rows(self, col, limit, desc=False, lo=None, hi=None, programs=None):
        from ragmi.index import order_rows_np
        self.calls.append(("order_rows", col, limit, desc, lo, hi))
        k, r, n = order_rows_np(self.keys[col], limit, desc, lo, hi, self._passing(programs))
        return torch.from_numpy(k), torch.from_numpy(r), n

    def facet_counts(self, field, n_codes, programs=None):
        from ragmi.index import facet_counts_np
        self.calls.append(("facet_counts", field, n_codes))
        return torch.from_numpy(facet_counts_np(self.tags, field, n_codes,
                                                self._passing(programs)))


TICKERS = ["AAPL", "MSFT", "NVDA"]
T0 = dt.datetime(2024, 1, 1, tzinfo=UTC)


def payload_of(i):
    p = {"ticker": TICKERS[i % 3], "document_type": "10-K" if i % 2 else "10-Q"}
    if i % 5:                                        # every fifth point lacks both range fields
        p["ingested_at"] = (T0 + dt.timedelta(hours=(i * 7) % 11)).isoformat()
        p["year"] = 2000 + (i * 3) % 4
    return p


@pytest.fixture()
def served():
    from ragmi.collection import Collection
    from ragmi.qdrant import QdrantClient
    fake = FakeIndex()
    col = Collection("docs", 4, None, index=fake,
                     range_fields={"ingested_at": "datetime", "year": "number"})
    n = 23
    col.upsert(list(range(100, 100 + n)), np.zeros((n, 4), np.float32),
               [payload_of(i) for i in range(n)])
    client = QdrantClient()
    client._collections[col.name] = col
    fake.calls.clear()
    return client, col, fake


def must(key, value):
    from ragmi import qdrant_models as m
    return m.Filter(must=[m.FieldCondition(key=key, match=m.MatchValue(value=value))])


def test_scroll_pages_to_the_end(served):
    client, col, fake = served
    seen, offset, pages = [], None, 0
    while True:
        recs, offset = client.scroll("docs", limit=5, offset=offset)
        seen += [r.id for r in recs]
        pages += 1
        if offset is None:
            break
    assert seen == list(range(100, 123)) and pages == 5          # 5 + 5 + 5 + 5 + 3
    assert fake.calls[0] == ("select_rows_from", 0, 6)           # limit + 1 rows, one call
    assert len(fake.calls) == pages
    # under a filter, and under a general filter (a program)
    from ragmi import qdrant_models as m
    for flt, want in ((must("ticker", "MSFT"), [100 + i for i in range(23) if i % 3 == 1]),
                      (m.Filter(must_not=[m.FieldCondition(key="ticker",
                                                           match=m.MatchValue(value="MSFT"))]),
                       [100 + i for i in range(23) if i % 3 != 1])):
        got, offset = [], None
        while True:
            recs, offset = client.scroll("docs", scroll_filter=flt, limit=4, offset=offset)
            assert all(r.payload == payload_of(r.id - 100) for r in recs)
            got += [r.id for r in recs]
            if offset is None:
                break
        assert got == want
    # a page that ends exactly at the last point has no next offset
    recs, offset = client.scroll("docs", limit=23)
    assert len(recs) == 23 and offset is None
    recs, offset = client.scroll("docs", limit=22)
    assert len(recs) == 22 and offset == 122
    recs, _ = client.scroll("docs", limit=2, with_payload=False)
    assert [r.payload for r in recs] == [None, None] and recs[0].order_value is None


def test_scroll_nothing_to_launch(served):
    client, col, fake = served
    assert client.scroll("docs", scroll_filter=must("ticker", "TSLA")) == ([], None)
    assert client.scroll("docs", limit=0) == ([], None)
    assert client.scroll("docs", limit=0, order_by="year") == ([], None)
    assert client.scroll("docs", scroll_filter=must("ticker", "TSLA"), order_by="year") == ([], None)
    assert fake.calls == []


def want_order(field, desc, keep=lambda i: True):
    """ids by (value, row), rows without the field left out; a stable sort keeps rows ascending."""
    rows = [i for i in range(23) if i % 5 and keep(i)]
    return [100 + i for i in sorted(rows, key=lambda i: payload_of(i)[field], reverse=desc)]


def test_scroll_order_by(served):
    from ragmi import qdrant_models as m
    client, col, fake = served
    recs, nxt = client.scroll("docs", limit=50, order_by="year")
    assert nxt is None
    assert [r.id for r in recs] == want_order("year", False)
    assert [r.order_value for r in recs] == [payload_of(r.id - 100)["year"] for r in recs]
    recs, _ = client.scroll("docs", limit=6, order_by=m.OrderBy("ingested_at", m.Direction.DESC))
    assert [r.id for r in recs] == want_order("ingested_at", True)[:6]
    assert all(r.order_value == payload_of(r.id - 100)["ingested_at"] for r in recs)
    # the direction as a plain string, under a filter
    recs, _ = client.scroll("docs", scroll_filter=must("ticker", "NVDA"), limit=50,
                            order_by=m.OrderBy("year", "desc"))
    assert [r.id for r in recs] == want_order("year", True, lambda i: i % 3 == 2)
    # start_from is inclusive on its side: a string and a datetime, ascending and descending
    cut = T0 + dt.timedelta(hours=5)
    for start in (cut.isoformat(), cut):
        recs, _ = client.scroll("docs", limit=50, order_by=m.OrderBy("ingested_at", None, start))
        assert [r.id for r in recs] == want_order(
            "ingested_at", False, lambda i: (i * 7) % 11 >= 5)
        recs, _ = client.scroll("docs", limit=50,
                                order_by=m.OrderBy("ingested_at", m.Direction.DESC, start))
        assert [r.id for r in recs] == want_order(
            "ingested_at", True, lambda i: (i * 7) % 11 <= 5)
    recs, _ = client.scroll("docs", limit=50, order_by=m.OrderBy("year", start_from=2002))
    assert [r.id for r in recs] == want_order("year", False, lambda i: (i * 3) % 4 >= 2)


def test_query_points_order_by_query(served):
    from ragmi import qdrant_models as m
    client, col, fake = served
    res = client.query_points("docs", query=m.OrderByQuery("year"), limit=7)
    assert [p.id for p in res.points] == want_order("year", False)[:7]
    assert all(p.score == 0.0 and p.order_value == payload_of(p.id - 100)["year"]
               and p.payload == payload_of(p.id - 100) for p in res.points)
    assert [c[0] for c in fake.calls] == ["order_rows"]          # never the coalescer's search
    res = client.query_points("docs", query=m.OrderByQuery(m.OrderBy("year", m.Direction.DESC)),
                              query_filter=must("document_type", "10-K"), limit=50,
                              with_payload=False)
    assert [p.id for p in res.points] == want_order("year", True, lambda i: i % 2 == 1)
    assert all(p.payload is None and p.order_value is not None for p in res.points)
    # a batch of order requests only: each in its slot, one order_rows per request
    fake.calls.clear()
    out = client.query_batch_points("docs", [
        m.QueryRequest(query=m.OrderByQuery("year"), limit=3),
        m.QueryRequest(query=m.OrderByQuery(m.OrderBy("ingested_at", "desc")), limit=4,
                       filter=must("ticker", "AAPL"))])
    assert [p.id for p in out[0].points] == want_order("year", False)[:3]
    assert [p.id for p in out[1].points] == want_order("ingested_at", True,
                                                       lambda i: i % 3 == 0)[:4]
    assert [c[0] for c in fake.calls] == ["order_rows", "order_rows"]


def test_facet(served):
    from ragmi import qdrant_models as m
    client, col, fake = served
    res = client.facet("docs", "ticker")
    assert isinstance(res, m.FacetResponse)
    assert [(h.value, h.count) for h in res.hits] == [("AAPL", 8), ("MSFT", 8), ("NVDA", 7)]
    assert fake.calls == [("facet_counts", 0, 3)]                # one call, n_codes = codebook
    res = client.facet("docs", "document_type", facet_filter=must("ticker", "AAPL"))
    assert [(h.value, h.count) for h in res.hits] == [("10-K", 4), ("10-Q", 4)]   # tie: value asc
    res = client.facet("docs", "ticker", limit=1,
                       facet_filter=m.Filter(must=[m.FieldCondition(
                           key="year", range=m.Range(gte=2003))]))
    want = sorted(((t, sum(1 for i in range(23) if i % 5 and (i * 3) % 4 == 3
                           and TICKERS[i % 3] == t)) for t in TICKERS), key=lambda h: (-h[1], h[0]))
    assert [(h.value, h.count) for h in res.hits] == [w for w in want if w[1]][:1]
    assert sum(h.count for h in client.facet("docs", "ticker").hits) == \
        client.count("docs").count
    assert client.facet("docs", "ticker", facet_filter=must("ticker", "TSLA")).hits == []
    assert client.facet("docs", "ticker", limit=0).hits == []
    # a value seen only in a filter gets no code; a code nothing holds any more is dropped
    col.upsert([100], np.zeros((1, 4), np.float32), [{"ticker": "MSFT"}])
    assert [(h.value, h.count) for h in client.facet("docs", "ticker").hits] == \
        [("MSFT", 9), ("AAPL", 7), ("NVDA", 7)]


def test_facet_values_that_do_not_compare(served):
    client, col, fake = served
    col.upsert([500, 501], np.zeros((2, 4), np.float32), [{"ticker": 7}, {"ticker": "7A"}])
    hits = client.facet("docs", "ticker", limit=10).hits
    assert [(h.value, h.count) for h in hits] == \
        [("AAPL", 8), ("MSFT", 8), ("NVDA", 7), (7, 1), ("7A", 1)]


# ------------------------------------------------------------------ refusals
def test_refusals(served):
    from ragmi import qdrant_models as m
    client, col, fake = served
    with pytest.raises(ValueError, match="offset cannot be used together with order_by"):
        client.scroll("docs", offset=100, order_by="year")
    with pytest.raises(ValueError, match="create_payload_index"):
        client.scroll("docs", order_by="revenue")
    with pytest.raises(ValueError, match="create_payload_index"):
        client.scroll("docs", order_by="ticker")                 # a keyword field
    with pytest.raises(ValueError, match="at most 4096"):
        client.scroll("docs", limit=4097, order_by="year")
    with pytest.raises(ValueError, match="at most 4096"):
        client.query_points("docs", query=m.OrderByQuery("year"), limit=5000)
    for field, bad in (("year", "2003"), ("year", True), ("ingested_at", 17),
                       ("ingested_at", "yesterday")):
        with pytest.raises(ValueError, match="start_from"):
            client.scroll("docs", order_by=m.OrderBy(field, start_from=bad))
    with pytest.raises(ValueError, match="Direction"):
        client.scroll("docs", order_by=m.OrderBy("year", "sideways"))
    with pytest.raises(ValueError, match="999.*not the id of a point"):
        client.scroll("docs", offset=999)
    with pytest.raises(NotImplementedError, match=r"payload_tag_fields=\('ticker', 'document_type'\)"):
        client.facet("docs", "year")
    with pytest.raises(ValueError, match="not built"):
        client.query_points("docs", query=m.OrderByQuery("year"),
                            prefetch=[m.Prefetch(query=[0.0] * 4)])
    with pytest.raises(ValueError, match="not built"):
        client.query_points("docs", query=m.FusionQuery(m.Fusion.RRF),
                            prefetch=[m.Prefetch(query=m.OrderByQuery("year"))])
    with pytest.raises(ValueError, match="not built"):
        client.query_batch_points("docs", [m.QueryRequest(
            query=m.OrderByQuery("year"), prefetch=[m.Prefetch(query=[0.0] * 4)])])
    assert fake.calls == []                                      # every refusal before a launch


def test_index_level_argument_checks():
    """FlatIndex / ShardSet refuse a bad limit, n_codes or row0 before touching the library."""
    from ragmi.index import FlatIndex
    from ragmi.shardset import ShardSet
    idx = FlatIndex.__new__(FlatIndex)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match=r"\[1, 4096\]"):
            FlatIndex.order_rows(idx, 0, bad)
    for bad in (-1, 65536):
        with pytest.raises(ValueError, match="65535"):
            FlatIndex.facet_counts(idx, 0, bad)
    with pytest.raises(ValueError, match="row0"):
        FlatIndex.select_rows_from(idx, -1)
    with pytest.raises(ValueError, match="row0"):
        ShardSet.select_rows_from(ShardSet.__new__(ShardSet), -1)
