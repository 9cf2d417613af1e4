"""GPU test that every route of the query front end answers a request the same way: one
query_batch_points call holding plain requests (scan, large-k pass, full pass), filtered
requests (legacy `must`, general, never-ingested value), limit 0, MMR requests and fusion
requests returns, id for id and score bit for bit, what each request gets when sent alone
through query_points — on one FlatIndex and on a two-shard ShardSet, whose answers are equal to
each other. A grouped query and a filtered count are compared between the two as well."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D = 6000, 384
TICKERS = ["AAPL", "MSFT", "NVDA", "AMZN", "GOOG", "META", "TSLA", "AMD"]
DOCS = ["10-K", "10-Q", "8-K"]


def _requests(m, q):
    def must(**kv):
        return m.Filter(must=[m.FieldCondition(key=k, match=m.MatchValue(value=v))
                              for k, v in kv.items()])
    general = m.Filter(
        must_not=[m.FieldCondition(key="document_type", match=m.MatchValue(value="8-K"))],
        must=[m.FieldCondition(key="ticker", match=m.MatchAny(any=["AAPL", "NVDA", "AMD"]))])
    return [
        m.QueryRequest(query=q[0], limit=5),
        m.QueryRequest(query=q[1], limit=40),
        m.QueryRequest(query=q[2], limit=5000),
        m.QueryRequest(query=q[3], limit=15, filter=must(ticker="MSFT", document_type="10-Q")),
        m.QueryRequest(query=q[4], limit=15, filter=general),
        m.QueryRequest(query=q[5], limit=15, filter=must(ticker="NEVER")),
        m.QueryRequest(query=q[6], limit=0),
        m.QueryRequest(query=m.NearestQuery(nearest=q[7], mmr=m.Mmr(diversity=0.3,
                                                                     candidates_limit=60)),
                       limit=10),
        m.QueryRequest(query=m.NearestQuery(nearest=q[8], mmr=m.Mmr(diversity=0.8,
                                                                     candidates_limit=200)),
                       limit=12, filter=general),
        m.QueryRequest(query=m.FusionQuery(fusion=m.Fusion.RRF), limit=10, prefetch=[
            m.Prefetch(query=q[9], filter=must(ticker="GOOG"), limit=20),
            m.Prefetch(query=q[10], filter=general, limit=30)]),
        m.QueryRequest(query=m.RrfQuery(rrf=m.Rrf(k=7)), limit=8, prefetch=[
            m.Prefetch(query=q[11], limit=25),
            m.Prefetch(query=q[9], filter=must(document_type="10-K"), limit=10)]),
    ]


def _triples(points):
    return [(p.id, np.float32(p.score).tobytes(), p.payload) for p in points]


@pytest.fixture(scope="module")
def clients(gpu):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, D)).astype(np.float32)
    payloads = [{"ticker": TICKERS[i % 8], "document_type": DOCS[(i // 8) % 3],
                 "text": f"chunk {i}"} for i in range(N)]
    q = x[rng.choice(N, 12)] + 0.05 * rng.standard_normal((12, D)).astype(np.float32)
    made = []
    for devices in (None, [0, 0]):
        cl = QdrantClient(url="http://unused", device=gpu, devices=devices)
        cl.create_collection("c", m.VectorParams(size=D, distance=m.Distance.COSINE),
                             capacity=N)
        cl.upsert("c", m.Batch(ids=list(range(N)), vectors=x, payloads=payloads))
        made.append(cl)
    yield made[0], made[1], q
    for cl in made:
        cl.close()


def test_batch_equals_each_request_alone_on_one_index_and_two_shards(clients):
    from ragmi import qdrant_models as m
    one, two, q = clients
    reqs = _requests(m, q)
    answers = []
    for cl in (one, two):
        batch = cl.query_batch_points("c", reqs)
        assert len(batch) == len(reqs)
        for r, got in zip(reqs, batch):
            alone = cl.query_points("c", query=r.query, limit=r.limit, query_filter=r.filter,
                                    prefetch=r.prefetch)
            assert _triples(got.points) == _triples(alone.points)
        answers.append([_triples(b.points) for b in batch])
    assert answers[0] == answers[1]
    sizes = [len(a) for a in answers[0]]
    assert sizes == [5, 40, 5000, 15, 15, 0, 0, 10, 12, 10, 8]


def test_groups_and_filtered_count_equal_on_one_index_and_two_shards(clients):
    from ragmi import qdrant_models as m
    one, two, q = clients
    flt = m.Filter(must=[m.FieldCondition(key="document_type", match=m.MatchValue(value="10-Q"))])
    general = m.Filter(
        must_not=[m.FieldCondition(key="document_type", match=m.MatchValue(value="8-K"))],
        must=[m.FieldCondition(key="ticker", match=m.MatchAny(any=["AAPL", "NVDA", "AMD"]))])
    found = [[(g.id, _triples(g.hits)) for g in
              cl.query_points_groups("c", query=q[0], group_by="ticker", limit=4, group_size=3,
                                     query_filter=flt).groups] for cl in (one, two)]
    assert found[0] == found[1]
    assert len(found[0]) == 4 and all(len(h) == 3 for _, h in found[0])
    # 3 of 8 tickers, 2 of 3 document types, every (ticker, type) cell holding N / 24 points
    counts = [cl.count("c", count_filter=general).count for cl in (one, two)]
    assert counts == [N * 6 // 24] * 2
    assert [cl.count("c", count_filter=flt).count for cl in (one, two)] == [N // 3] * 2
