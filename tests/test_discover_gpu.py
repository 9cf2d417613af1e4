"""GPU tests of discovery and context queries (rag_index_discover / discover_kernels.hip,
FlatIndex.discover, Collection.search_discover and QdrantClient's DiscoverQuery / ContextQuery
route): ids and scores bit for bit against the numpy restatement tests/_discover_ref.py — on the
seed-7 corpus of near-duplicate groups (3001 rows: the tile tail; 4 identical rows per group:
exact ties), on a 50,009-row corpus whose threshold comes from a true sample and on which a
one-pair context search and a zero-target discover request saturate (more than 16384 rows tied at
the top: left unanswered after ONE round, re-answered by the full pass), and through the client.

Measured on the MI355X (test_bounds_hold_for_every_row's print), the largest hi - lo over the
3001 rows, D = 384 / 1024: context n = 16 0.0116 / 0.0165 (fp16 storage), 0.0420 / 0.0484 (fp32);
context n = 1 0.0006 / 0.0009 and 0.0029 / 0.0033. Discover n = 1: 2.0002-2.0008 on the 15-87 rows
whose pair is uncertain (the 2-wide step of a sign: expected), at most 0.0008 elsewhere. Discover
n = 15 holds the positive == negative pair, so every row has the step: 6.0-10.0, i.e. 3 to 5
uncertain pairs in the widest row."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import _discover_ref as R

pytestmark = pytest.mark.gpu

CAP = 16384                                  # kLkCap: candidates the hot pass keeps
CASES = (("discover", 0), ("discover", 1), ("discover", 3), ("discover", 15),
         ("context", 1), ("context", 3), ("context", 16))
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
    """One FlatIndex per (D, storage) for the module; tag 2 on five rows, 1 elsewhere. One
    recommend request runs on it first, so rag_index_reco_stats has live counters to keep."""
    from ragmi.index import FlatIndex
    key = (D, storage)
    if key not in _indexes:
        x, q, _ = corpus(D)
        idx = FlatIndex(D, len(x), gpu, storage=storage)
        idx.upsert(x, np.arange(len(x)), row_tags(), new_count=len(x))
        idx.recommend(q[None], None, "best_score", 15)
        _indexes[key] = idx
    return _indexes[key]


@functools.lru_cache(maxsize=None)
def request(D, kind, n):
    """(target or None, pairs) of case (kind, n): ids (ints: stored rows) and vectors mixed. The
    target is the corpus's query. Pair 0's positive is a stored row of a duplicate group; for
    n >= 3 pair 1 has positive == negative (the sign-0 branch: every row uncertain) and pair 2 a
    stored row as its negative."""
    x, q, group = corpus(D)
    rng = np.random.default_rng(1000 * (kind == "context") + n)
    in_groups = np.nonzero(group >= 0)[0]
    vec = lambda: rng.standard_normal(D).astype(np.float32)  # noqa: E731
    pairs = []
    for i in range(n):
        if i == 0:
            pairs.append((int(rng.choice(in_groups)), vec()))
        elif i == 1 and n >= 3:
            same = vec()
            pairs.append((same, same))
        elif i % 2 == 0:
            pairs.append((vec(), int(rng.integers(0, len(x)))))
        else:
            pairs.append((q + 0.5 * vec(), vec()))
    return (q if kind == "discover" else None), tuple(pairs)


def on_device(idx, vecs):
    """Examples as FlatIndex.discover takes them: ids resolved to their stored rows on the
    device (gather_rows, as Collection.search_discover does), vectors as they are."""
    if not vecs:
        return None
    rows = [x for x in vecs if isinstance(x, int)]
    f16, f32, _ = idx.gather_rows(np.asarray(rows, np.int64)) if rows else (None, None, None)
    got = iter(f32 if f32 is not None else
               f16.view(torch.float16).float() if rows else ())
    return torch.stack([next(got) if isinstance(x, int) else
                        torch.as_tensor(x, device=idx.device) for x in vecs])


def args_of(idx, target, pairs):
    return (None if target is None else torch.as_tensor(target, device=idx.device),
            on_device(idx, [p for p, _ in pairs]), on_device(idx, [n for _, n in pairs]))


@functools.lru_cache(maxsize=None)
def ref_scores(D, storage, kind, n):
    stats = {}
    s = R.scores(stored(D, storage), *request(D, kind, n), stats)
    return s, stats


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    torch.cuda.synchronize()
    s, r = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(r, want[1])
    assert np.array_equal(bits(s), bits(want[0]))


# ------------------------------------------------------------------ 1. bit-exact vs the restatement
@pytest.mark.parametrize("kind", ["discover", "context"])
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
@pytest.mark.parametrize("D", [384, 1024])
def test_discover_matches_the_restatement(gpu, D, storage, kind):
    idx = index_of(gpu, D, storage)
    reco = idx.reco_stats()
    assert reco.hot == 1 and reco.candidates > 0
    ties = 0
    for knd, n in CASES:
        if knd != kind:
            continue
        s, stats = ref_scores(D, storage, kind, n)
        if n:
            assert stats["plus"] > 0 and stats["minus"] > 0     # both signs occur in the corpus
        if kind == "discover" and n >= 3:
            assert stats["zero"] >= len(s)                      # the equal pair: sign 0 everywhere
        t, pos, neg = args_of(idx, *request(D, kind, n))
        for k in KS:
            tstats = {}
            want = R.top_k(s, k, stats=tstats)
            ties += tstats["ties"]
            before, un = idx.discover_stats(), idx.unanswered()
            same(idx.discover(t, pos, neg, k), want)
            after = idx.discover_stats()
            assert (after.hot, after.full) == (before.hot + 1, before.full)
            assert idx.unanswered() == un and after.rounds == 1
            if k <= 33:
                assert 0 < after.candidates < len(s)            # the threshold prunes
            else:
                assert after.candidates <= len(s)
            if k == 200:
                assert after.candidates == len(s)               # T = -inf: every row
            same(idx.discover(t, pos, neg, k, full=True), want)
            assert idx.discover_stats()[:2] == (after.hot, after.full + 1)
    assert ties > 0                                             # identical rows tie exactly
    assert idx.reco_stats() == reco                             # counters of their own


# ------------------------------------------------------------------ 2. the certificate
@pytest.mark.parametrize("kind,n", [("discover", 15), ("context", 16), ("discover", 1),
                                    ("context", 1)])      # n = 1: no equal pair in the request
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
@pytest.mark.parametrize("D", [384, 1024])
def test_bounds_hold_for_every_row(gpu, D, storage, kind, n):
    idx = index_of(gpu, D, storage)
    s, _ = ref_scores(D, storage, kind, n)
    t, pos, neg = args_of(idx, *request(D, kind, n))
    lo, hi = idx.discover_bounds(t, pos, neg, np.arange(len(s)))
    torch.cuda.synchronize()
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    width = hi - lo
    print(f"discover_bounds D={D} {storage} {kind} n={n}: max hi-lo = {float(width.max()):.6g}, "
          f"rows wider than 0.5: {int((width > 0.5).sum())}, "
          f"max of the others = {float(width[width <= 0.5].max(initial=0.0)):.6g}")
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    assert (lo <= s).all() and (s <= hi).all()
    if kind == "context":
        assert (hi <= 0).all()
    out = idx.discover_bounds(t, pos, neg, np.asarray([-1, len(s), 5]))
    torch.cuda.synchronize()
    assert out[0].cpu().tolist()[:2] == [-np.inf] * 2 and out[1].cpu().tolist()[:2] == [np.inf] * 2
    assert out[0][2].item() == lo[5] and out[1][2].item() == hi[5]


# ------------------------------------------------------------------ 3. filters
@pytest.mark.parametrize("kind", ["discover", "context"])
@pytest.mark.parametrize("D,storage", [(384, "fp16"), (1024, "fp32")])
def test_filters(gpu, D, storage, kind):
    from ragmi.filters import FilterProgram, pack_view
    idx = index_of(gpu, D, storage)
    s, _ = ref_scores(D, storage, kind, 3)
    t, pos, neg = args_of(idx, *request(D, kind, 3))
    tags = row_tags()
    five = R.top_k(s, 8, passing=tags == 2)
    assert (five[1][:5] >= 0).all() and (five[1][5:] == -1).all()
    blob = pack_view([FilterProgram.maskeq(0xFFFF, 2)])
    un = idx.unanswered()
    for full in (False, True):
        same(idx.discover(t, pos, neg, 8, filters=(0xFFFF, 2), full=full), five)
        same(idx.discover(t, pos, neg, 8, filters=(1, 1), programs=blob, full=full), five)
        none = idx.discover(t, pos, neg, 8, filters=(0xFFFF, 3), full=full)
        same(none, (np.full(8, -np.inf, np.float32), np.full(8, -1, np.int64)))
        most = R.top_k(s, 40, passing=tags == 1)
        same(idx.discover(t, pos, neg, 40, filters=(0xFFFF, 1), full=full), most)
    assert idx.unanswered() == un


# ------------------------------------------------------------------ 4. a true sample, 5. saturation
@functools.lru_cache(maxsize=None)
def sampling_corpus():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((50009, 384)).astype(np.float32)
    tags = (1 + rng.integers(0, 7, len(x))).astype(np.uint32)
    return x, tags, R.encode(x, "fp16")


_big = {}


def big_index(gpu):
    from ragmi.index import FlatIndex
    if "idx" not in _big:
        x, tags, _ = sampling_corpus()
        idx = FlatIndex(384, len(x), gpu, storage="fp16")
        idx.upsert(x, np.arange(len(x)), tags, new_count=len(x))
        _big["idx"] = idx
    return _big["idx"]


def test_sampled_threshold(gpu):
    """50,009 rows = 3,126 tiles; k = 15 samples 97 of them, so T is a real threshold."""
    x, tags, enc = sampling_corpus()
    idx = big_index(gpu)
    rng = np.random.default_rng(6)
    vec = lambda: rng.standard_normal(384).astype(np.float32)  # noqa: E731
    target, pairs = vec(), ((vec(), 40001), (123, vec()), (vec(), vec()))
    s = R.scores(enc, target, pairs)
    t, pos, neg = args_of(idx, target, pairs)
    un = idx.unanswered()
    for flt, passing in ((None, None), ((0xFFFF, 3), tags == 3)):
        want = R.top_k(s, 15, passing)
        # on the CPU: far fewer rows than the cap lie near the k-th score
        near = int((s[passing if passing is not None else slice(None)]
                    >= want[0][14] - np.float32(1e-2)).sum())
        assert near < CAP // 8
        before = idx.discover_stats()
        same(idx.discover(t, pos, neg, 15, filters=flt), want)
        after = idx.discover_stats()
        assert (after.hot, after.full) == (before.hot + 1, before.full)
        assert 15 <= after.candidates < CAP // 4 and after.rounds == 1
        same(idx.discover(t, pos, neg, 15, filters=flt, full=True), want)
    assert idx.unanswered() == un


@pytest.mark.parametrize("kind", ["context", "discover"])
def test_saturated_requests_take_one_round_then_the_full_pass(gpu, kind):
    """(a) a context search with one pair: about half the corpus scores 0; (b) a discover
    request with one pair and a zero target: about half the corpus scores exactly 1.5. More
    than kLkCap rows tie at the k-th score, no threshold separates them: the hot pass must say
    so after ONE round, and the full pass must answer."""
    x, _, enc = sampling_corpus()
    idx = big_index(gpu)
    rng = np.random.default_rng(11)
    pairs = ((rng.standard_normal(384).astype(np.float32),
              rng.standard_normal(384).astype(np.float32)),)
    target = None if kind == "context" else np.zeros(384, np.float32)
    s = R.scores(enc, target, pairs)
    want = R.top_k(s, 15)
    tied = np.nonzero(s == want[0][14])[0]
    assert len(tied) > CAP and want[0][0] == want[0][14] == (0.0 if kind == "context" else 1.5)
    assert want[1].tolist() == tied[:15].tolist()               # the k lowest tied rows
    t, pos, neg = args_of(idx, target, pairs)
    before, un, rescued = idx.discover_stats(), idx.unanswered(), idx.rescued
    sc, r = idx.discover(t, pos, neg, 15)
    torch.cuda.synchronize()
    assert (r.cpu().numpy() == -1).all() and torch.isneginf(sc).all()
    after = idx.discover_stats()
    assert idx.unanswered() == un + 1
    assert after.rounds == 1 and after.candidates > CAP
    assert (after.hot, after.full) == (before.hot + 1, before.full)
    same(idx.discover(t, pos, neg, 15, rescue=True), want)
    last = idx.discover_stats()
    assert (last.hot, last.full) == (after.hot + 1, after.full + 1) and last.rounds == 1
    assert idx.unanswered() == un + 2 and idx.rescued == rescued + 1


# ------------------------------------------------------------------ 6. through the client
def test_client_discover(gpu):
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
    target, extra = x[3] + x[9], x[50] - x[60]
    pairs_rows = [(n - 1, 17), (extra, 40)]
    own = [n - 1, 17, 40]

    def expect(tgt, limit, passing=None):
        s, r = R.discover(enc, tgt, pairs_rows, limit + 3, passing)
        keep = [j for j in range(limit + 3) if r[j] >= 0 and r[j] not in own]
        return [canon[r[j]] for j in keep[:limit]], s[keep[:limit]]

    context = [m.ContextPair(positive=ids[n - 1], negative=ids[17]),
               m.ContextPair(positive=extra.tolist(), negative=ids[40])]
    query = m.DiscoverQuery(m.DiscoverInput(target=target.tolist(), context=context))
    want_ids, want_s = expect(target, 10)
    got = client.query_points("c", query, limit=10).points
    assert [p.id for p in got] == want_ids and len(got) == 10
    assert np.array_equal(bits([p.score for p in got]), bits(want_s))
    assert not {canon[r] for r in own} & {p.id for p in got}   # id examples never among the hits
    assert got[0].payload["n"] == canon.index(got[0].id) and got[0].vector is None
    legacy = client.discover("c", target=target.tolist(), context=context, limit=10,
                             with_payload=False, with_vectors=True)
    assert [p.id for p in legacy] == want_ids
    assert legacy[0].payload is None and len(legacy[0].vector) == 384
    amd = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    f_ids, f_s = expect(target, 10, passing=np.arange(n) % 2 == 1)
    got = client.query_points("c", query, limit=10, query_filter=amd).points
    assert [p.id for p in got] == f_ids and np.array_equal(bits([p.score for p in got]), bits(f_s))
    anyof = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchAny(any=["AMD", "X"]))])
    got = client.query_points("c", query, limit=10, query_filter=anyof).points
    assert [p.id for p in got] == f_ids                        # a FilterProgram, through a view
    # the context query: the same pairs, no target; and both in one batch, in order
    c_ids, c_s = expect(None, 12)
    cq = m.ContextQuery(context=context)
    got = client.query_points("c", cq, limit=12).points
    assert [p.id for p in got] == c_ids and np.array_equal(bits([p.score for p in got]), bits(c_s))
    assert [p.id for p in client.discover("c", context=context, limit=12)] == c_ids
    batch = client.query_batch_points("c", [m.QueryRequest(query=cq, limit=12),
                                            m.QueryRequest(query=query, limit=10, filter=amd)])
    assert [[p.id for p in r.points] for r in batch] == [c_ids, f_ids]
    # a target given by id is an example too: never among the hits
    pts = client.discover("c", target=ids[5], context=context, limit=12)
    assert len(pts) == 12 and not {canon[5], *(canon[r] for r in own)} & {p.id for p in pts}
    # a delete that moves an example's row (the last row fills the hole): same ids
    gone = next(i for i in range(n - 1) if canon[i] not in want_ids + c_ids and i not in own)
    client.delete("c", [ids[gone]])
    col = client._col("c")
    assert col.id_to_row[canon[n - 1]] == gone                 # the example moved
    assert [p.id for p in client.query_points("c", query, limit=10).points] == want_ids
    assert [p.id for p in client.query_points("c", cq, limit=12).points] == c_ids
    with pytest.raises(ValueError, match="is not in collection"):
        client.discover("c", target=ids[gone])
    client.close()
    sharded = QdrantClient(device=gpu, devices=[0, 0])
    sharded.create_collection("c", m.VectorParams(size=384, distance=m.Distance.COSINE))
    sharded.upsert("c", [m.PointStruct(id=i, vector=x[i].tolist()) for i in range(8)])
    with pytest.raises(NotImplementedError, match="discover over a shard set is not built"):
        sharded.discover("c", target=1)
    sharded.close()


def test_client_saturated_context_query_is_answered_by_the_full_pass(gpu):
    """A one-pair context query over 50,009 points: the hot pass cannot answer it (test above);
    the route rescues it on the full pass instead of returning nothing."""
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    x, _, _ = sampling_corpus()
    client = QdrantClient(device=gpu)
    client.create_collection("big", m.VectorParams(size=384, distance=m.Distance.COSINE))
    col = client._col("big")
    col.upsert(list(range(len(x))), x, None)
    enc = R.encode(x, col.index.storage)
    rng = np.random.default_rng(12)
    pos, neg = rng.standard_normal(384).astype(np.float32), 777
    s = R.scores(enc, None, [(pos, neg)])
    want = R.top_k(s, 11)
    assert int((s == 0).sum()) > CAP and (want[0][:11] == 0).all()
    keep = [int(r) for r in want[1] if r != 777][:10]
    before, rescued = col.index.discover_stats(), col.rescued
    got = client.query_points("big", m.ContextQuery(m.ContextPair(pos.tolist(), neg)),
                              limit=10).points
    assert [p.id for p in got] == keep and all(p.score == 0.0 for p in got)
    after = col.index.discover_stats()
    assert (after.hot, after.full) == (before.hot + 1, before.full + 1) and after.rounds == 1
    assert col.rescued == rescued + 1
    client.close()
