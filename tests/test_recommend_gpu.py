"""GPU tests of recommend queries (rag_index_recommend / reco_kernels.hip, FlatIndex.recommend,
Collection.search_recommend and QdrantClient's RecommendQuery route): ids and scores bit for bit
against the numpy restatement tests/_reco_ref.py — on the seed-7 corpus of near-duplicate groups
(3001 rows: the tile tail; 4 identical rows per group: exact ties), on a 50,009-row corpus whose
threshold comes from a true sample, on a corpus of 20,000 identical rows the hot pass must leave
unanswered, and through the client."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import _reco_ref as R

pytestmark = pytest.mark.gpu

CAP = 16384                                  # kLkCap: candidates the hot pass keeps
SIDES = ((1, 0), (3, 2), (16, 16), (0, 2))
KS = (1, 15, 33, 100, 200)                   # 200 > the 188 tile maxima: T = -inf


@functools.lru_cache(maxsize=None)
def corpus(D):
    return R.grouped_corpus(D)


@functools.lru_cache(maxsize=None)
def stored(D, storage):
    return R.encode(corpus(D)[0], storage)


def row_tags():
    tags = np.ones(len(corpus(384)[0]), np.uint32)
    tags[[5, 16, 17, 1500, 3000]] = 2
    return tags


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


@functools.lru_cache(maxsize=None)
def sides(D, P, N):
    """The examples of case (P, N): ids (ints: stored rows) and vectors mixed, the query of the
    corpus first among the positives, a stored row of a group first among the negatives."""
    x, q, group = corpus(D)
    rng = np.random.default_rng(100 * P + N)
    in_groups = np.nonzero(group >= 0)[0]
    pos = [q] if P else []
    while len(pos) < P:
        pos.append(int(rng.choice(in_groups)) if len(pos) % 2 else
                   rng.standard_normal(D).astype(np.float32))
    neg = [int(in_groups[0])] if N else []
    while len(neg) < N:
        neg.append(int(rng.integers(0, len(x))) if len(neg) % 2 == 0 else
                   rng.standard_normal(D).astype(np.float32))
    return tuple(pos), tuple(neg)


def on_device(idx, side):
    """A side as FlatIndex.recommend takes it: ids resolved to their stored rows on the device
    (gather_rows, as Collection.search_recommend does), vectors as they are."""
    if not side:
        return None
    rows = [x for x in side if isinstance(x, int)]
    f16, f32, _ = idx.gather_rows(np.asarray(rows, np.int64)) if rows else (None, None, None)
    got = iter(f32 if f32 is not None else
               f16.view(torch.float16).float() if rows else ())
    return torch.stack([next(got) if isinstance(x, int) else
                        torch.as_tensor(x, device=idx.device) for x in side])


@functools.lru_cache(maxsize=None)
def ref_scores(D, storage, P, N, strategy):
    stats = {}
    s = R.scores(stored(D, storage), *sides(D, P, N), strategy, stats)
    return s, stats


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    torch.cuda.synchronize()
    s, r = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(r, want[1])
    assert np.array_equal(bits(s), bits(want[0]))


# ------------------------------------------------------------------ 1. bit-exact vs the restatement
@pytest.mark.parametrize("strategy", [R.BEST, R.SUM])
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
@pytest.mark.parametrize("D", [384, 1024])
def test_recommend_matches_the_restatement(gpu, D, storage, strategy):
    idx = index_of(gpu, D, storage)
    ties = 0
    for P, N in SIDES:
        s, stats = ref_scores(D, storage, P, N, strategy)
        if strategy == R.BEST and P and N:
            assert stats["pos_branch"] > 0 and stats["neg_branch"] > 0
        pos, neg = (on_device(idx, side) for side in sides(D, P, N))
        for k in KS:
            tstats = {}
            want = R.top_k(s, k, stats=tstats)
            ties += tstats["ties"] if P else 0
            before, un = idx.reco_stats(), idx.unanswered()
            same(idx.recommend(pos, neg, strategy, k), want)
            after = idx.reco_stats()
            assert (after.hot, after.full) == (before.hot + 1, before.full)
            assert idx.unanswered() == un and after.rounds == 1
            if k <= 33:
                assert 0 < after.candidates < len(s)           # the threshold prunes
            else:
                assert after.candidates <= len(s)
            if k == 200:
                assert after.candidates == len(s)              # T = -inf: every row
            same(idx.recommend(pos, neg, strategy, k, full=True), want)
            assert idx.reco_stats()[:2] == (after.hot, after.full + 1)
    assert ties > 0                                            # identical rows tie exactly


@pytest.mark.parametrize("storage", ["fp16", "fp32"])
@pytest.mark.parametrize("D", [384, 1024])
def test_average_vector_is_the_plain_search_of_v(gpu, D, storage):
    import oracle_scan as O
    idx = index_of(gpu, D, storage)
    enc = stored(D, storage)
    for P, N in ((1, 0), (3, 2), (16, 16)):
        pos_h, neg_h = sides(D, P, N)
        v = R.average_vector(enc, pos_h, neg_h)
        pos, neg = on_device(idx, pos_h), on_device(idx, neg_h)
        got_v = idx.reco_vector(pos, neg)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got_v.cpu().numpy()), bits(v))
        before = idx.reco_stats()
        for k in (15, 100):
            want = idx.search(v[None], k)
            got = idx.recommend(pos, neg, None, k)
            same(got, (want[0][0].cpu().numpy(), want[1][0].cpu().numpy()))
            ws, wr = O.search(enc, v[None], k)
            same(got, (ws[0], wr[0]))
        pair = idx.recommend(pos, neg, "average_vector", 8, filters=(0xFFFF, 2))
        ws, wr = O.search(enc, v[None], 8, tags=row_tags(), mask=0xFFFF, value=2, use_filter=True)
        same(pair, (ws[0], wr[0]))
        assert idx.reco_stats()[:2] == before[:2]              # a search, not a recommend pass


# ------------------------------------------------------------------ 2. filters
@pytest.mark.parametrize("strategy", [R.BEST, R.SUM])
@pytest.mark.parametrize("D,storage", [(384, "fp16"), (1024, "fp32")])
def test_filters(gpu, D, storage, strategy):
    from ragmi.filters import FilterProgram, pack_view
    idx = index_of(gpu, D, storage)
    s, _ = ref_scores(D, storage, 3, 2, strategy)
    pos, neg = (on_device(idx, side) for side in sides(D, 3, 2))
    tags = row_tags()
    five = R.top_k(s, 8, passing=tags == 2)
    assert (five[1][:5] >= 0).all() and (five[1][5:] == -1).all()
    blob = pack_view([FilterProgram.maskeq(0xFFFF, 2)])
    for full in (False, True):
        same(idx.recommend(pos, neg, strategy, 8, filters=(0xFFFF, 2), full=full), five)
        same(idx.recommend(pos, neg, strategy, 8, filters=(1, 1), programs=blob, full=full), five)
        none = idx.recommend(pos, neg, strategy, 8, filters=(0xFFFF, 3), full=full)
        same(none, (np.full(8, -np.inf, np.float32), np.full(8, -1, np.int64)))
        most = R.top_k(s, 40, passing=tags == 1)
        same(idx.recommend(pos, neg, strategy, 40, filters=(0xFFFF, 1), full=full), most)
    assert idx.unanswered() == 0


# ------------------------------------------------------------------ 3. a true sample
@functools.lru_cache(maxsize=None)
def sampling_corpus():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((50009, 384)).astype(np.float32)
    tags = (1 + rng.integers(0, 7, len(x))).astype(np.uint32)
    return x, tags, R.encode(x, "fp16")


def test_sampled_threshold(gpu):
    """50,009 rows = 3,126 tiles; k = 15 samples 97 of them, so T is a real threshold."""
    from ragmi.index import FlatIndex
    x, tags, enc = sampling_corpus()
    idx = FlatIndex(384, len(x), gpu, storage="fp16")
    idx.upsert(x, np.arange(len(x)), tags, new_count=len(x))
    rng = np.random.default_rng(6)
    vec = lambda: rng.standard_normal(384).astype(np.float32)  # noqa: E731
    for strategy, pos_h, neg_h in ((R.BEST, (vec(), 40001, vec()), (123, vec())),
                                   (R.SUM, (vec(), 7), (vec(),))):
        s = R.scores(enc, pos_h, neg_h, strategy)
        pos, neg = on_device(idx, pos_h), on_device(idx, neg_h)
        for flt, passing in ((None, None), ((0xFFFF, 3), tags == 3)):
            want = R.top_k(s, 15, passing)
            # on the CPU: far fewer rows than the cap lie near the k-th score
            near = int((s[passing if passing is not None else slice(None)]
                        >= want[0][14] - np.float32(1e-2)).sum())
            assert near < CAP // 8
            before = idx.reco_stats()
            same(idx.recommend(pos, neg, strategy, 15, filters=flt), want)
            after = idx.reco_stats()
            assert (after.hot, after.full) == (before.hot + 1, before.full)
            assert 15 <= after.candidates < CAP and after.rounds == 1
            same(idx.recommend(pos, neg, strategy, 15, filters=flt, full=True), want)
    assert idx.unanswered() == 0
    idx.close()


# ------------------------------------------------------------------ 4. the certificate
@pytest.mark.parametrize("strategy", [R.BEST, R.SUM])
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
@pytest.mark.parametrize("D", [384, 1024])
def test_bounds_hold_for_every_row(gpu, D, storage, strategy):
    idx = index_of(gpu, D, storage)
    s, _ = ref_scores(D, storage, 16, 16, strategy)
    pos, neg = (on_device(idx, side) for side in sides(D, 16, 16))
    lo, hi = idx.reco_bounds(pos, neg, strategy, np.arange(len(s)))
    torch.cuda.synchronize()
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    print(f"reco_bounds D={D} {storage} {strategy}: max hi-lo = {float((hi - lo).max()):.6g}")
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    assert (lo <= s).all() and (s <= hi).all()
    out = idx.reco_bounds(pos, neg, strategy, np.asarray([-1, len(s), 5]))
    torch.cuda.synchronize()
    assert out[0].cpu().tolist()[:2] == [-np.inf] * 2 and out[1].cpu().tolist()[:2] == [np.inf] * 2
    assert out[0][2].item() == lo[5] and out[1][2].item() == hi[5]


# ------------------------------------------------------------------ 5. massive ties
def test_massive_ties_are_unanswered_then_rescued(gpu):
    """1,000 random rows, then 20,000 identical ones: more than kLkCap rows tie at the top, no
    threshold can separate them, the hot pass must say so and the full pass must answer."""
    from ragmi.collection import Collection
    rng = np.random.default_rng(9)
    one = rng.standard_normal(384).astype(np.float32)
    x = np.concatenate([rng.standard_normal((1000, 384)).astype(np.float32),
                        np.broadcast_to(one, (20000, 384))])
    col = Collection("ties", 384, gpu, capacity=len(x), storage="fp16")
    col.upsert(list(range(len(x))), x, None)
    enc = R.encode(x, "fp16")
    pos_h = (one, rng.standard_normal(384).astype(np.float32))
    neg_h = (rng.standard_normal(384).astype(np.float32),)
    for strategy in (R.BEST, R.SUM):
        want = R.recommend(enc, pos_h, neg_h, strategy, 15)
        assert want[1].tolist() == list(range(1000, 1015))     # the tied block's lowest rows
        un, rescued = col.index.unanswered(), col.rescued
        s, r = col.index.recommend(np.stack(pos_h), np.stack(neg_h), strategy, 15)
        torch.cuda.synchronize()
        assert (r.cpu().numpy() == -1).all() and torch.isneginf(s).all()
        assert col.index.unanswered() == un + 1
        assert col.index.reco_stats().candidates > CAP
        code = {R.BEST: 1, R.SUM: 2}[strategy]
        hits = col.search_recommend([(list(pos_h), list(neg_h), code, (0, 0), 15)])[0]
        assert [h[0] for h in hits] == want[1].tolist()
        assert np.array_equal(bits([h[1] for h in hits]), bits(want[0]))
        assert col.index.unanswered() == un + 2 and col.rescued == rescued + 1
    col.index.close()


# ------------------------------------------------------------------ 6. through the client
def test_client_recommend(gpu):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    rng = np.random.default_rng(21)
    n = 200
    x = rng.standard_normal((n, 384)).astype(np.float32)
    ids = [hashlib.md5(str(i).encode()).hexdigest() for i in range(n)]
    canon = [str(__import__("uuid").UUID(i)) for i in ids]
    client = QdrantClient(device=gpu)
    client.create_collection("c", m.VectorParams(size=384, distance=m.Distance.COSINE))
    client.upsert("c", [m.PointStruct(id=ids[i], vector=x[i].tolist(),
                                      payload={"ticker": "AMD" if i % 2 else "AAPL", "n": i})
                        for i in range(n)])
    enc = R.encode(x, "fp32")
    pos_rows, neg_rows, extra = [n - 1, 17], [40], x[3] + x[9]

    def expect(limit, passing=None):
        s, r = R.recommend(enc, pos_rows + [extra], neg_rows, R.BEST, limit + 3, passing)
        keep = [j for j in range(limit + 3) if r[j] >= 0 and r[j] not in pos_rows + neg_rows]
        return [canon[r[j]] for j in keep[:limit]], s[keep[:limit]]

    query = m.RecommendQuery(m.RecommendInput(
        positive=[ids[n - 1], ids[17], extra.tolist()], negative=[ids[40]],
        strategy=m.RecommendStrategy.BEST_SCORE))
    want_ids, want_s = expect(10)
    got = client.query_points("c", query, limit=10).points
    assert [p.id for p in got] == want_ids and len(got) == 10
    assert np.array_equal(bits([p.score for p in got]), bits(want_s))
    assert not {canon[r] for r in pos_rows + neg_rows} & {p.id for p in got}
    assert got[0].payload["n"] == canon.index(got[0].id) and got[0].vector is None
    legacy = client.recommend("c", positive=[ids[n - 1], ids[17], extra.tolist()],
                              negative=[ids[40]], strategy="best_score", limit=10,
                              with_payload=False, with_vectors=True)
    assert [p.id for p in legacy] == want_ids
    assert legacy[0].payload is None and len(legacy[0].vector) == 384
    amd = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    f_ids, f_s = expect(10, passing=np.arange(n) % 2 == 1)
    got = client.query_points("c", query, limit=10, query_filter=amd).points
    assert [p.id for p in got] == f_ids and np.array_equal(bits([p.score for p in got]), bits(f_s))
    anyof = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchAny(any=["AMD", "X"]))])
    got = client.query_points("c", query, limit=10, query_filter=anyof).points
    assert [p.id for p in got] == f_ids                        # a FilterProgram, through a view
    # average_vector (the default) and sum_scores through the same route
    for strategy in (None, "sum_scores"):
        pts = client.recommend("c", positive=[ids[5], ids[6]], negative=[ids[7]],
                               strategy=strategy, limit=12)
        assert len(pts) == 12 and not {canon[5], canon[6], canon[7]} & {p.id for p in pts}
    # a delete that moves an example's row (the last row fills the hole): same ids
    gone = next(i for i in range(n - 1) if canon[i] not in want_ids
                and i not in pos_rows + neg_rows)
    client.delete("c", [ids[gone]])
    col = client._col("c")
    assert col.id_to_row[canon[n - 1]] == gone                 # the example moved
    assert [p.id for p in client.query_points("c", query, limit=10).points] == want_ids
    with pytest.raises(ValueError, match="is not in collection"):
        client.recommend("c", positive=[ids[gone]])
    client.close()
    sharded = QdrantClient(device=gpu, devices=[0, 0])
    sharded.create_collection("c", m.VectorParams(size=384, distance=m.Distance.COSINE))
    sharded.upsert("c", [m.PointStruct(id=i, vector=x[i].tolist()) for i in range(8)])
    with pytest.raises(NotImplementedError, match="recommend over a shard set is not built"):
        sharded.recommend("c", positive=[1])
    sharded.close()
