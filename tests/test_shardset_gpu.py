"""GPU tests of the shard set: rag_merge_topk_gather against its numpy restatement, ShardSet
against one FlatIndex on the same rows and against the oracle (ids and scores bit-equal), and
QdrantClient(devices=[...]) against QdrantClient() under the same calls. Logical shards share
GPU 0 (devices=[0, 0, ...]); the last test runs on two physical devices where there are two."""
import hashlib
import threading

import numpy as np
import pytest
import torch

import oracle_scan as O

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF


# ------------------------------------------------------------------ 1. the gather-merge kernel
def packed_lists(rng, n, B, k, n_scores=6):
    """n packed lists [B, k, 2] sorted by (score desc, local row asc), -1 padded: few distinct
    scores (ties across lists, the mapped id decides), random fill, some (list, query) pairs
    and, from three lists up, one whole list entirely -1."""
    vals = rng.standard_normal(n_scores).astype(np.float32)
    R = 2 * k + 8
    out = []
    for l in range(n):
        rows = rng.permuted(np.tile(np.arange(R, dtype=np.int32), (B, 1)), axis=1)[:, :k]
        sc = vals[rng.integers(0, n_scores, (B, k))]
        m = rng.integers(0, k + 1, B)
        m[rng.random(B) < 0.2] = 0
        if n >= 3 and l == n - 2:
            m[:] = 0
        if l == 0:
            m[0] = k                                  # one full list
        bad = np.arange(k)[None, :] >= m[:, None]
        order = np.lexsort((rows, -sc.astype(np.float64), bad), axis=-1)
        rows = np.take_along_axis(rows, order, -1)
        sc = np.take_along_axis(sc, order, -1)
        bad = np.take_along_axis(bad, order, -1)
        a = np.stack([sc.view(np.int32), rows], axis=-1)
        a[bad] = -1
        out.append(np.ascontiguousarray(a))
    return out


@pytest.mark.parametrize("k", [1, 15, 32, 33, 100, 4096])
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("n", [1, 2, 3, 8, 64])
def test_merge_topk_gather_bit_exact(gpu, n, B, k):
    from ragmi.shardset import gather_merge_np, merge_topk_gather
    rng = np.random.default_rng(n * 100003 + B * 1009 + k)
    lists = packed_lists(rng, n, B, k)
    add = list(range(n))
    dev = [torch.from_numpy(a).to(gpu) for a in lists]          # separate allocations
    s, i, e = merge_topk_gather(dev, k, n, add)
    torch.cuda.synchronize()
    s2, i2, e2 = gather_merge_np(lists, k, n, add)
    np.testing.assert_array_equal(i.cpu().numpy(), i2)
    np.testing.assert_array_equal(s.cpu().numpy().view(np.int32), s2.view(np.int32))
    np.testing.assert_array_equal(e.cpu().numpy(), e2)


def test_merge_topk_gather_general_id_map_and_stacked_merge(gpu):
    """id_mul = 1 with per-list offsets (contiguous ranges, ids past 2^31), and the same
    lists through rag_merge_topk_packed, which must agree where its int32 ids reach."""
    from ragmi.index import merge_topk_packed
    from ragmi.shardset import gather_merge_np, merge_topk_gather
    rng = np.random.default_rng(5)
    n, B, k = 3, 4, 40
    lists = packed_lists(rng, n, B, k)
    dev = [torch.from_numpy(a).to(gpu) for a in lists]
    for add in ([0, 1000, 2000], [0, 1 << 33, 1 << 34]):
        s, i, e = merge_topk_gather(dev, k, 1, add)
        torch.cuda.synchronize()
        s2, i2, e2 = gather_merge_np(lists, k, 1, add)
        np.testing.assert_array_equal(i.cpu().numpy(), i2)
        np.testing.assert_array_equal(s.cpu().numpy().view(np.int32), s2.view(np.int32))
    shifted = []
    for l, a in enumerate(lists):
        a = a.copy()
        a[..., 1] = np.where(a[..., 1] >= 0, a[..., 1] + 1000 * l, -1)
        shifted.append(torch.from_numpy(a).to(gpu))
    s3, i3 = merge_topk_packed(torch.stack(shifted), k)
    s2, i2, _ = gather_merge_np(lists, k, 1, [0, 1000, 2000])
    np.testing.assert_array_equal(i3.cpu().numpy(), i2)
    np.testing.assert_array_equal(s3.cpu().numpy().view(np.int32), s2.view(np.int32))


# ------------------------------------------------------------------ 2. ShardSet vs FlatIndex vs oracle
N_ROWS = 3001          # no multiple of any N; the last tile of 16 is partial
FILTERS = np.array([[ALL, 7], [ALL, 9], [0, 0], [ALL, 1], [0, 0]], np.uint32)


class Case:
    """Rows, queries, tags, and the single-index and oracle answers, computed once per
    (dim, storage) and shared by the tests (never modified)."""

    def __init__(self, gpu, dim, storage, n=N_ROWS):
        from ragmi.index import FlatIndex
        rng = np.random.default_rng(dim + n)
        self.dim, self.storage, self.n = dim, storage, n
        x = rng.standard_normal((n, dim)).astype(np.float32)
        x[100:140] = x[3]                                # ties that span the shards
        self.x = x
        self.q = np.concatenate([x[rng.choice(n, 4)] +
                                 0.05 * rng.standard_normal((4, dim)).astype(np.float32),
                                 x[3:4]]).astype(np.float32)
        # tag 7 only on rows = 1 (mod 24): on shard 1 alone for N = 2, 3, 8; tag 9 nowhere
        self.tags = np.ones(n, np.uint32)
        self.tags[1::24] = 7
        self.enc = O.encode_rows32(x) if storage == "fp32" else O.encode_rows(x)
        self.single = FlatIndex(dim, n, gpu, storage=storage)
        self.single.upsert(x, np.arange(n), self.tags, new_count=n)
        self._oracle, self._flat = {}, {}

    def oracle(self, k, filtered):
        key = (k, filtered)
        if key not in self._oracle:
            kk = min(k, self.n)
            if not filtered:
                s, i = O.search(self.enc, self.q, kk)
            else:
                parts = [O.search(self.enc, self.q[b:b + 1], kk, tags=self.tags, mask=int(m),
                                  value=int(v), use_filter=bool(m))
                         for b, (m, v) in enumerate(FILTERS)]
                s = np.concatenate([p[0] for p in parts])
                i = np.concatenate([p[1] for p in parts])
            pad = k - kk
            self._oracle[key] = (np.pad(s, ((0, 0), (0, pad)), constant_values=-np.inf),
                                 np.pad(i, ((0, 0), (0, pad)), constant_values=-1))
        return self._oracle[key]

    def flat(self, k, filtered):
        key = (k, filtered)
        if key not in self._flat:
            s, i = self.single.search(self.q, k, filters=FILTERS if filtered else None)
            torch.cuda.synchronize()
            self._flat[key] = (s.cpu().numpy(), i.cpu().numpy())
        return self._flat[key]


_cases = {}


def case(gpu, dim, storage, n=N_ROWS):
    key = (dim, storage, n)
    if key not in _cases:
        _cases[key] = Case(gpu, dim, storage, n)
    return _cases[key]


def make_set(c, devices):
    from ragmi.shardset import ShardSet
    ss = ShardSet(c.dim, devices, c.n, c.storage)
    ss.upsert(c.x, np.arange(c.n), c.tags, new_count=c.n)
    return ss


def check_set(ss, c, k, filtered, **kw):
    s, i = ss.search(c.q, k, filters=FILTERS if filtered else None, **kw)
    torch.cuda.synchronize()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    for name, (s2, i2) in (("flat", c.flat(k, filtered)), ("oracle", c.oracle(k, filtered))):
        np.testing.assert_array_equal(i, i2, err_msg=f"ids vs {name}, k={k}")
        np.testing.assert_array_equal(s.view(np.int32), s2.view(np.int32),
                                      err_msg=f"scores vs {name}, k={k}")
    return s, i


@pytest.mark.parametrize("storage", ["fp16", "fp32"])
@pytest.mark.parametrize("n_shards", [1, 2, 3, 8])
def test_shardset_equals_single_index_and_oracle(gpu, n_shards, storage):
    c = case(gpu, 384, storage)
    ss = make_set(c, [gpu.index] * n_shards)
    assert ss.count == c.n and [sh.count for sh in ss.shards] == \
        [len(range(s, c.n, n_shards)) for s in range(n_shards)]
    for k in (15, 32, 100):
        check_set(ss, c, k, False)
        s, i = check_set(ss, c, k, True)
        assert (i[0] >= 0).sum() == min(k, len(range(1, c.n, 24))) and (i[1] == -1).all()
    # the tied rows 3, 100..139 lead the last query in row order, across shards
    _, i = check_set(ss, c, 32, False)
    assert i[4].tolist() == [3] + list(range(100, 131))
    ss.close()


def test_shardset_dim_1024(gpu):
    c = case(gpu, 1024, "fp16")
    ss = make_set(c, [gpu.index] * 3)
    for k in (15, 100):
        check_set(ss, c, k, False)
    check_set(ss, c, 15, True)
    ss.close()


def test_shardset_any_k_and_full_pass(gpu):
    """k = 5000 over 7000 rows (unpacked lists, the id-remap kernel, rag_merge_topk), and
    full=True at k <= 4096 (RAG_SHARDSET_FULL)."""
    c = case(gpu, 384, "fp16", 7000)
    ss = make_set(c, [gpu.index] * 3)
    check_set(ss, c, 5000, False)
    check_set(ss, c, 5000, True)
    check_set(ss, c, 15, True, full=True)
    check_set(ss, c, 100, False, full=True)
    ss.close()


# ------------------------------------------------------------------ 3. small and growing sets
def both(gpu, dim=384, storage="fp16", capacity=16, n_shards=3):
    from ragmi.index import FlatIndex
    from ragmi.shardset import ShardSet
    return (ShardSet(dim, [gpu.index] * n_shards, capacity, storage),
            FlatIndex(dim, capacity, gpu, storage=storage))


def same_search(ss, flat, q, k):
    a = ss.search(q, k)
    b = flat.search(q, k)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a[1].cpu().numpy(), b[1].cpu().numpy())
    np.testing.assert_array_equal(a[0].cpu().numpy().view(np.int32),
                                  b[0].cpu().numpy().view(np.int32))
    return a[1].cpu().numpy()


def test_small_sets(gpu):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, 384)).astype(np.float32)
    q = rng.standard_normal((3, 384)).astype(np.float32)
    ss, flat = both(gpu)
    i = ss.search(q, 15)[1]                                  # an empty set
    torch.cuda.synchronize()
    assert (i.cpu().numpy() == -1).all() and ss.count == 0
    for idx in (ss, flat):
        idx.upsert(x[:2], np.arange(2), new_count=2)         # 2 rows over 3 shards: one is empty
    assert [sh.count for sh in ss.shards] == [1, 1, 0]
    i = same_search(ss, flat, q, 15)
    assert ((i >= 0).sum(axis=1) == 2).all()
    for idx in (ss, flat):
        idx.upsert(x[2:], np.arange(2, 5), new_count=5)      # 5 rows over 3 shards
    assert [sh.count for sh in ss.shards] == [2, 2, 1]
    i = same_search(ss, flat, q, 15)
    assert ((i >= 0).sum(axis=1) == 5).all()
    same_search(ss, flat, q, 3)
    ss.close()
    flat.close()


@pytest.mark.parametrize("storage", ["fp16", "fp32"])
def test_growth_overwrites_and_export(gpu, storage):
    rng = np.random.default_rng(4)
    ss, flat = both(gpu, storage=storage, capacity=16)
    q = rng.standard_normal((4, 384)).astype(np.float32)
    count = 0
    for step, m in enumerate((7, 1000, 333)):
        x = rng.standard_normal((m, 384)).astype(np.float32)
        rows = np.arange(count, count + m)
        if count:                                            # overwrites on different shards
            over = rng.choice(count, min(count, 5), replace=False)
            rows = np.concatenate([rows, over])
            x = np.concatenate([x, rng.standard_normal((len(over), 384)).astype(np.float32)])
        tags = rng.integers(0, 4, len(rows)).astype(np.uint32)
        count += m
        for idx in (ss, flat):
            if count > idx.capacity:
                idx.reserve(count)
            idx.upsert(x, rows, tags, new_count=count)
        assert ss.count == flat.count == count and ss.capacity >= count
        same_search(ss, flat, q, 15)
        same_search(ss, flat, q, 100)
    np.testing.assert_array_equal(ss.export_rows(), flat.export_rows())
    np.testing.assert_array_equal(ss.export_rows(5, 700), flat.export_rows(5, 700))
    np.testing.assert_array_equal(ss.export_tags(), flat.export_tags())
    np.testing.assert_array_equal(ss.export_tags(11, 2), flat.export_tags(11, 2))
    if storage == "fp32":
        np.testing.assert_array_equal(ss.export_rows32(1, 999), flat.export_rows32(1, 999))
    ss.close()
    flat.close()


# ------------------------------------------------------------------ 4. QdrantClient(devices=...)
def md5_id(i):
    return hashlib.md5(f"doc-{i}".encode()).hexdigest()


def ingest(c, m, x, tickers, lo, hi, note):
    c.upsert("t", [m.PointStruct(id=md5_id(i), vector=x[i].tolist(),
                                 payload={"ticker": tickers[i % len(tickers)], "n": i,
                                          "note": note}) for i in range(lo, hi)])


def points(res):
    return [(p.id, p.score, p.payload, p.version) for p in res.points]


def test_qdrant_client_sharded_equals_single(gpu):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    rng = np.random.default_rng(6)
    n, dim = 400, 384
    x = rng.standard_normal((n + 50, dim)).astype(np.float32)
    tickers = ["AAPL", "MSFT", "NVDA", "AMD", "TSLA"]
    a = QdrantClient(device=gpu, devices=[gpu.index] * 3)
    b = QdrantClient(device=gpu)
    for c in (a, b):
        c.create_collection("t", m.VectorParams(size=dim, distance=m.Distance.COSINE))
        ingest(c, m, x, tickers, 0, 250, "first")
        ingest(c, m, x, tickers, 200, n, "second")           # re-ingest 200..249: same ids
        x2 = x.copy()
        x2[10:20] = x[n:n + 10]                              # last write wins, new vectors
        ingest(c, m, x2, tickers, 10, 20, "third")
    from ragmi.shardset import ShardSet
    assert isinstance(a._col("t").index, ShardSet) and not isinstance(b._col("t").index, ShardSet)
    assert a.count("t").count == b.count("t").count == n
    q = x[5] + 0.1 * rng.standard_normal(dim).astype(np.float32)
    flt = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    for kw in (dict(limit=15), dict(limit=15, query_filter=flt), dict(limit=100),
               dict(limit=1000, query_filter=flt)):
        pa, pb = points(a.query_points("t", query=q, **kw)), points(b.query_points("t", query=q, **kw))
        assert pa == pb and len(pa) > 0
    reqs = [m.QueryRequest(query=x2[j].tolist(), limit=5 + j,
                           filter=flt if j % 2 else None, with_payload=True) for j in range(6)]
    ra, rb = a.query_batch_points("t", reqs), b.query_batch_points("t", reqs)
    assert [points(r) for r in ra] == [points(r) for r in rb]
    ids = [md5_id(i) for i in (0, 15, 249, 399)]
    va = a.retrieve("t", ids, with_vectors=True)
    vb = b.retrieve("t", ids, with_vectors=True)
    assert [(r.id, r.payload, r.vector) for r in va] == [(r.id, r.payload, r.vector) for r in vb]
    assert va[1].payload["note"] == "third"
    a.close()
    b.close()


# ------------------------------------------------------------------ 5. one shard unanswered
def test_unanswered_shard_is_rescued(gpu):
    """20,000 copies of one row, all on shard 0 of 3: more than the 16,384 a large-k round
    keeps, so shard 0 leaves the query unanswered and hands the merge an all -1 list. The set
    sees the flag and re-answers on the full exact pass."""
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    rng = np.random.default_rng(8)
    n, dim = 66_000, 384
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[0:60_000:3] = x[0]
    c = QdrantClient(device=gpu, devices=[gpu.index] * 3)
    c.create_collection("t", m.VectorParams(size=dim, distance=m.Distance.COSINE,
                                            datatype="float16"), capacity=n)
    c.upsert("t", m.Batch(ids=list(range(n)), vectors=x, payloads=None))
    res = c.query_points("t", query=x[0], limit=100)
    s2, i2 = O.search(O.encode_rows(x), x[:1], 100)
    assert i2[0].tolist() == list(range(0, 300, 3))
    assert [p.id for p in res.points] == i2[0].tolist()
    assert [p.score for p in res.points] == s2[0].tolist()
    assert c._col("t").rescued == 1
    c.close()


# ------------------------------------------------------------------ 6. persistence
def test_persistence_across_shard_counts(gpu, tmp_path):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    rng = np.random.default_rng(10)
    n, dim = 500, 384
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = x[7] + 0.1 * rng.standard_normal(dim).astype(np.float32)
    flt = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="B"))])

    def ask(c):
        return [points(c.query_points("t", query=q, limit=k, query_filter=f))
                for k in (15, 100) for f in (None, flt)]

    def fill(c):
        c.create_collection("t", m.VectorParams(size=dim, distance=m.Distance.COSINE))
        c.upsert("t", m.Batch(ids=list(range(n)), vectors=x,
                              payloads=[{"ticker": "AB"[i % 2], "n": i} for i in range(n)]))

    for first, others in (([gpu.index] * 3, (None, [gpu.index] * 2)),
                          (None, ([gpu.index] * 3, [gpu.index] * 2))):
        path = str(tmp_path / f"from_{len(first) if first else 1}")
        c = QdrantClient(device=gpu, devices=first, path=path)
        fill(c)
        want = ask(c)
        c.close()                                            # saves
        for devs in others:
            d = QdrantClient(device=gpu, devices=devs, path=path)
            assert d.count("t").count == n
            assert ask(d) == want
            d.path = None                                    # do not write back
            d.close()


# ------------------------------------------------------------------ 7. concurrency
def test_two_threads_two_streams(gpu):
    c = case(gpu, 384, "fp16")
    ss = make_set(c, [gpu.index] * 3)
    qs = [torch.from_numpy(c.q).to(gpu), torch.from_numpy(c.q[::-1].copy()).to(gpu)]
    ks = [15, 100]
    want = []
    for q, k in zip(qs, ks):
        s, i = ss.search(q, k)
        torch.cuda.synchronize()
        want.append((s.cpu().numpy(), i.cpu().numpy()))
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
    got, errs = [[], []], []

    def work(t):
        try:
            with torch.cuda.stream(streams[t]):
                for _ in range(8):
                    s, i = ss.search(qs[t], ks[t])
                    got[t].append((s, i))
                streams[t].synchronize()
        except BaseException as e:          # surfaces in the main thread
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for t in range(2):
        for s, i in got[t]:
            np.testing.assert_array_equal(i.cpu().numpy(), want[t][1])
            np.testing.assert_array_equal(s.cpu().numpy(), want[t][0])
    ss.close()


def test_coalescer_over_sharded_collection(gpu):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    rng = np.random.default_rng(12)
    n, dim = 600, 384
    x = rng.standard_normal((n, dim)).astype(np.float32)
    c = QdrantClient(device=gpu, devices=[gpu.index] * 3, coalesce_window_s=0.002)
    c.create_collection("t", m.VectorParams(size=dim, distance=m.Distance.COSINE))
    c.upsert("t", m.Batch(ids=list(range(n)), vectors=x, payloads=None))
    qs = x[:12] + 0.1 * rng.standard_normal((12, dim)).astype(np.float32)
    want = [points(c.query_points("t", query=q, limit=15)) for q in qs]
    got, errs = [None] * 12, []

    def work(j):
        try:
            got[j] = points(c.query_points("t", query=qs[j], limit=15))
        except BaseException as e:
            errs.append(e)

    th = [threading.Thread(target=work, args=(j,)) for j in range(12)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert got == want
    co = c._col("t").coalescer
    assert co.requests == 24 and co.batches <= 24
    c.close()


# ------------------------------------------------------------------ 8. two physical devices
def test_two_physical_devices(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("one HIP device visible")
    c = case(gpu, 384, "fp16")
    before = torch.cuda.current_device()
    ss = make_set(c, [0, 1])
    assert ss.shards[1].device.index == 1
    for k in (15, 32, 100):
        check_set(ss, c, k, False)
        check_set(ss, c, k, True)
    assert torch.cuda.current_device() == before
    ss.close()
