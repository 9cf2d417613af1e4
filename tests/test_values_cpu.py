"""CPU tests of the front end's value check (ragmi.collection.require_finite; DESIGN.md "Values
at the edges"): a vector with a non-finite component is refused with ValueError before any index
call, the message naming the point id (upsert) or the position (queries, prefetches, recommend
examples), on every route that takes a caller's vector. Finite extremes pass. Collections over
stand-in indexes (_stubs); no GPU."""
import numpy as np
import pytest

import _stubs as S
import _values_ref as V

D = 4
GOOD = [0.0, 1.0, 0.0, 0.0]
BAD = {"+inf": [0.0, float("inf"), 0.0, 0.0], "-inf": [0.0, 1.0, float("-inf"), 0.0],
       "nan": [float("nan"), 1.0, 0.0, 0.0], "fp32 overflow": [0.0, 1e39, 0.0, 0.0]}
MSG = "non-finite component"


class _StubIndex:
    """FlatIndex stand-in: every call is recorded; search / recommend return rows 0..k-1 with
    falling scores, mmr the first k candidates, gather_rows row r as [r, 0, 0, 0]."""
    device = None
    storage = "fp32"
    capacity = 1000

    def __init__(self, count):
        self.count = count
        self.calls = []

    def upsert(self, vectors, rows, tags, new_count):
        self.calls.append(("upsert", np.asarray(vectors).tolist(), np.asarray(rows).tolist()))
        self.count = new_count

    def search(self, q, k, filters=None, full=False, rescue=False):
        import torch
        self.calls.append(("search", len(q), k))
        return (torch.linspace(0.9, 0.1, k).repeat(len(q), 1),
                torch.arange(k, dtype=torch.int64).repeat(len(q), 1))

    def unanswered(self):
        return 0

    def mmr(self, s, ids, k, diversity, ncand):
        self.calls.append(("mmr", k))
        return s[:, :k].clone(), ids[:, :k].clone()

    def gather_rows(self, rows):
        import torch
        f32 = torch.zeros((len(rows), D))
        f32[:, 0] = torch.as_tensor(np.asarray(rows), dtype=torch.float32)
        return None, f32, None

    def recommend(self, pos, neg, strategy, k, filters=None, programs=None, rescue=False):
        import torch
        self.calls.append(("recommend", k))
        return torch.linspace(0.9, 0.1, k), torch.arange(k, dtype=torch.int64)


def stub_client(count=40):
    return S.stub_client(S.stub_collection(
        _StubIndex(count), dim=D, ids=range(100, 100 + count),
        payloads=[{"ticker": "AMD" if r % 2 else "AAPL", "n": r} for r in range(count)]))


# ------------------------------------------------------------------------------- 1. the helper
def test_require_finite_names_the_first_bad_vector():
    import torch
    from ragmi.collection import require_finite, stack_queries
    ok = np.zeros((5, D), np.float32)
    require_finite(ok, "query")
    require_finite(torch.from_numpy(ok), "query")
    require_finite(np.zeros((0, D), np.float32), "query")
    for name, bad in BAD.items():
        x = ok.copy()
        with np.errstate(over="ignore"):
            x[3] = np.asarray(bad, np.float32)
            x[4] = np.asarray(bad, np.float32)
        for batch in (x, torch.from_numpy(x)):
            with pytest.raises(ValueError, match=f"query at position 3 holds a {MSG}"):
                require_finite(batch, "query")
            with pytest.raises(ValueError, match=f"the vector of point 'd' holds a {MSG}"):
                require_finite(batch, "the vector of point", ["a", "b", "c", "d", "e"])
        with pytest.raises(ValueError, match=f"query at position 1 holds a {MSG}"):
            stack_queries([GOOD, bad, GOOD], D)
        with pytest.raises(ValueError, match=f"query at position 0 holds a {MSG}"):
            stack_queries([torch.tensor(bad)], D, one=True, host=True)
        with pytest.raises(ValueError, match=f"query at position 2 holds a {MSG}"):
            stack_queries([GOOD, torch.tensor(GOOD), bad], D)
    with pytest.raises(ValueError, match="must be one 4-dim vector"):      # the shape check first
        stack_queries([[float("nan")] * 3], D, one=True)


def test_finite_extremes_pass():
    """fp32 subnormals, FLT_MAX, -0.0, one-hot: every finite vector is let through unchanged."""
    from ragmi.collection import stack_queries
    x = V.specials(V.FINITE, 384, 5)
    got = stack_queries(list(x), 384)
    np.testing.assert_array_equal(got.view(np.uint32), x.view(np.uint32))
    client, col = stub_client(count=0)
    fine = np.float32([[V.FLT_MAX, -V.FLT_MAX, 1e-45, -0.0], [0, 0, 0, 0], [1e-42, 0, 0, 3e36]])
    client.upsert("t", [_point(i, v.tolist()) for i, v in enumerate(fine)])
    assert [c[0] for c in col.index.calls] == ["upsert"] and col.index.count == 3
    np.testing.assert_array_equal(np.float32(col.index.calls[0][1]).view(np.uint32),
                                  fine.view(np.uint32))
    assert len(client.query_points("t", fine[0].tolist(), limit=2).points) == 2


# --------------------------------------------------------------------------------- 2. upsert
def _point(pid, vec, payload=None):
    from ragmi import qdrant_models as m
    return m.PointStruct(id=pid, vector=vec, payload=payload or {"ticker": "AMD"})


@pytest.mark.parametrize("name", list(BAD))
def test_upsert_refuses_and_names_the_point_id(name):
    from ragmi import qdrant_models as m
    client, col = stub_client(count=0)
    with pytest.raises(ValueError, match=f"upsert: the vector of point 7 holds a {MSG}"):
        client.upsert("t", [_point(5, GOOD), _point(7, BAD[name]), _point(9, BAD[name])])
    uid = "0123456789abcdef0123456789abcdef"
    with pytest.raises(ValueError, match=f"point '{uid}' holds a {MSG}"):
        client.upsert("t", m.Batch(ids=[1, uid], vectors=[GOOD, BAD[name]],
                                   payloads=[None, None]))
    # nothing reached the index and no point exists
    assert col.index.calls == [] and col.index.count == 0
    assert col.row_ids == [] and col.id_to_row == {} and col.payloads == []


# -------------------------------------------------------------------------------- 3. queries
@pytest.mark.parametrize("name", list(BAD))
def test_every_query_route_refuses_and_names_the_position(name):
    from ragmi import qdrant_models as m
    bad = BAD[name]
    client, col = stub_client()
    q0 = f"query at position 0 holds a {MSG}"
    # search / query_points: through the coalescer, and (limit past the scan's k) on its own
    with pytest.raises(ValueError, match=q0):
        client.query_points("t", bad, limit=5)
    with pytest.raises(ValueError, match=q0):
        client.query_points("t", bad, limit=100)
    with pytest.raises(ValueError, match=q0):
        client.query_points("t", np.asarray(bad, np.float64), limit=5, with_vectors=True)
    with pytest.raises(ValueError, match=q0):
        client.query_points("t", m.NearestQuery(nearest=bad), limit=5)
    with pytest.raises(ValueError, match=q0):
        client.search("t", bad, limit=5)
    with pytest.raises(ValueError, match=f"query at position 2 holds a {MSG}"):
        client.query_batch_points("t", [m.QueryRequest(query=GOOD, limit=3),
                                        m.QueryRequest(query=GOOD, limit=3),
                                        m.QueryRequest(query=bad, limit=3)])
    # grouped
    with pytest.raises(ValueError, match=q0):
        client.query_points_groups("t", bad, group_by="ticker", limit=2, group_size=2)
    # MMR: alone and in a batch the plain requests ride
    with pytest.raises(ValueError, match=q0):
        client.query_points("t", m.NearestQuery(nearest=bad, mmr=m.Mmr(0.5, 10)), limit=5)
    with pytest.raises(ValueError, match=f"query at position 1 holds a {MSG}"):
        client.query_batch_points("t", [
            m.QueryRequest(query=m.NearestQuery(nearest=GOOD, mmr=m.Mmr(0.5, 10)), limit=5),
            m.QueryRequest(query=bad, limit=3)])
    # fusion and formula prefetches, also those that would not be searched (limit 0)
    rrf = m.FusionQuery(fusion=m.Fusion.RRF)
    fq = m.FormulaQuery(formula=m.SumExpression(sum=["$score[0]", "$score[1]"]))
    for query, route in ((rrf, "fusion"), (fq, "formula")):
        msg = f"{route}: request 0, the query of prefetch 1 holds a {MSG}"
        with pytest.raises(ValueError, match=msg):
            client.query_points("t", query, limit=5, prefetch=[m.Prefetch(query=GOOD, limit=8),
                                                               m.Prefetch(query=bad, limit=8)])
        with pytest.raises(ValueError, match=msg):
            client.query_points("t", query, limit=5, prefetch=[m.Prefetch(query=GOOD, limit=8),
                                                               m.Prefetch(query=bad, limit=0)])
        with pytest.raises(ValueError, match=f"{route}: request 1, the query of prefetch 0"):
            client.query_batch_points("t", [
                m.QueryRequest(query=query, limit=5, prefetch=[m.Prefetch(query=GOOD, limit=8),
                                                               m.Prefetch(query=GOOD, limit=8)]),
                m.QueryRequest(query=query, limit=5, prefetch=[m.Prefetch(query=bad, limit=8),
                                                               m.Prefetch(query=GOOD, limit=8)])])
    # recommend examples: ids are stored rows, vectors are the caller's
    reco = lambda pos, neg: m.RecommendQuery(m.RecommendInput(pos, neg,     # noqa: E731
                                                              m.RecommendStrategy.BEST_SCORE))
    with pytest.raises(ValueError, match=f"recommend: positive example 1 holds a {MSG}"):
        client.query_points("t", reco([101, bad, GOOD], [102]), limit=5)
    with pytest.raises(ValueError, match=f"recommend: negative example 2 holds a {MSG}"):
        client.query_points("t", reco([GOOD], [102, GOOD, bad]), limit=5)
    with pytest.raises(ValueError, match=f"recommend: positive example 0 holds a {MSG}"):
        client.recommend("t", positive=[bad], limit=0)         # whatever the limit
    with pytest.raises(ValueError, match=f"recommend: negative example 0 holds a {MSG}"):
        client.recommend("t", positive=[101], negative=[np.asarray(bad, np.float32)],
                         strategy="sum_scores")
    # refused before any index call, and nothing rode the coalescer
    assert col.index.calls == [] and col.coalescer.batches == 0
    # the same requests with finite vectors are answered (fusion and formula fuse on the device)
    assert len(client.query_points("t", GOOD, limit=5).points) == 5
    assert len(client.query_points("t", reco([101, GOOD], [102]), limit=5).points) == 5
    assert len(client.query_points("t", m.NearestQuery(nearest=GOOD, mmr=m.Mmr(0.5, 10)),
                                   limit=5).points) == 5
