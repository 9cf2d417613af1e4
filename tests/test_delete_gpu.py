"""GPU tests of point deletion: rag_index_select_rows against np.nonzero, remove_rows against
the numpy application of the removal plan (bit for bit), search after a removal against a
freshly loaded index and the oracle, ShardSet.remove_rows against one FlatIndex, and
QdrantClient.delete against clients that never held the deleted points. Logical shards share
GPU 0 (devices=[0, 0, ...]); the last sharded case also runs on two devices where there are
two."""
import hashlib
import threading
import time
import uuid

import numpy as np
import pytest
import torch

import oracle_scan as O

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
N_ROWS = 3001          # no multiple of 16 or of any N: the last tile is partial


def dev_rows(gpu, n, dim=384):
    v = torch.zeros((n, dim), dtype=torch.float32, device=gpu)
    if n:
        v[:, 0] = 1.0
    return v


# ------------------------------------------------------------------ 1. select_rows
# one tag array serves every density through (mask, value): bit 0 a random half, bit 1 every
# 24th row, bit 2 every row; bits 8.. random, so the mask has something to mask
DENSITY = {"none": (4, 0), "all": (0, 0), "all_masked": (4, 4), "every24": (2, 2),
           "half": (1, 1), "half_and_every24": (3, 3)}
_select = {}


def select_case(gpu, n):
    if n not in _select:
        from ragmi.index import FlatIndex
        rng = np.random.default_rng(n)
        tags = (rng.integers(0, 2, n).astype(np.uint32) | np.uint32(4) |
                (rng.integers(0, 1 << 24, n).astype(np.uint32) << np.uint32(8)))
        tags[::24] |= np.uint32(2)
        idx = FlatIndex(384, n, gpu)
        if n:
            idx.upsert(dev_rows(gpu, n), np.arange(n), tags, new_count=n)
        _select[n] = (idx, tags)
    return _select[n]


@pytest.mark.parametrize("density", list(DENSITY))
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, N_ROWS, 4096, 4097, 200_003])
def test_select_rows_equals_nonzero(gpu, n, density):
    idx, tags = select_case(gpu, n)
    mask, value = DENSITY[density]
    want = np.nonzero((tags & np.uint32(mask)) == np.uint32(value))[0].astype(np.int64)
    rows, total = idx.select_rows(mask, value)
    assert total == len(want)
    np.testing.assert_array_equal(rows.cpu().numpy(), want)
    assert idx.select_rows(mask, value, cap=0)[1] == len(want)          # the pure count
    # a cap below the match count: the first cap rows, the full total, nothing past cap
    for cap in {1, len(want) // 2, len(want) - 1} - {0, -1}:
        if cap >= len(want):
            continue
        out = torch.full((cap + 64,), -7, dtype=torch.int64, device=gpu)
        rows, total = idx.select_rows(mask, value, cap=cap, out=out)
        assert total == len(want) and rows.numel() == cap
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:cap], want[:cap])
        assert (got[cap:] == -7).all()


def test_select_rows_follows_the_count(gpu):
    """Rows at or past count never match, whatever their (stale) tags say."""
    idx, tags = select_case(gpu, N_ROWS)
    from ragmi.index import FlatIndex
    other = FlatIndex(384, N_ROWS, gpu)
    other.upsert(dev_rows(gpu, N_ROWS), np.arange(N_ROWS), tags, new_count=N_ROWS)
    for count in (2999, 2992, 17, 0):
        other.set_count(count)
        rows, total = other.select_rows(1, 1)
        want = np.nonzero((tags[:count] & 1) == 1)[0]
        assert total == len(want)
        np.testing.assert_array_equal(rows.cpu().numpy(), want)
    other.close()


def test_row_call_argument_errors(gpu):
    from ragmi import _lib
    from ragmi.index import FlatIndex
    L = _lib.load()
    idx = FlatIndex(384, 32, gpu, storage="fp32")
    buf = torch.zeros(64 * 384, dtype=torch.float32, device=gpu)
    p = buf.data_ptr()
    assert L.rag_index_move_rows(idx._h, None, p, 3, 0, None) == -1          # RAG_EINVAL
    assert L.rag_index_move_rows(idx._h, p, None, 3, 0, None) == -1
    assert L.rag_index_move_rows(idx._h, p, p, -1, 0, None) == -1
    assert L.rag_index_move_rows(idx._h, p, p, 1, 33, None) == -4            # RAG_ERANGE
    assert L.rag_index_gather_rows(idx._h, None, 2, p, p, p, None) == -1
    assert L.rag_index_gather_rows(idx._h, p, 2, p, None, p, None) == -1     # fp32 needs f32
    assert L.rag_index_scatter_rows(idx._h, p, 2, p, None, p, 2, None) == -1
    assert L.rag_index_scatter_rows(idx._h, p, 2, None, p, p, 2, None) == -1
    assert L.rag_index_select_rows(idx._h, 0, 0, None, 4, p, None) == -1     # cap without rows
    assert L.rag_index_select_rows(idx._h, 0, 0, p, 4, None, None) == -1
    idx16 = FlatIndex(384, 32, gpu)
    assert L.rag_index_gather_rows(idx16._h, p, 2, p, p, p, None) == -1      # fp16 takes no f32
    assert idx.count == 0
    idx.close()
    idx16.close()


# ------------------------------------------------------------------ 2. the shared case
FILTERS = np.array([[ALL, 7], [ALL, 9], [0, 0], [ALL, 1], [0, 0], [0, 0], [ALL, 1]], np.uint32)
N1_SEARCH = 2100       # count after the "search" delete set: 131 tiles and 4 rows


class Case:
    """Rows, tags, queries and the stored forms of one (dim, storage), exported once from an
    index that is never modified; each test loads copies of it."""

    def __init__(self, gpu, dim, storage):
        from ragmi.index import FlatIndex
        rng = np.random.default_rng(dim + 7)
        n = N_ROWS
        self.gpu, self.dim, self.storage, self.n = gpu, dim, storage, n
        x = rng.standard_normal((n, dim)).astype(np.float32)
        x[100:140] = x[3]                              # a block of identical rows (ties)
        self.x = x
        # tag 7 on rows = 1 (mod 24), tag 1 elsewhere; the high half a second field
        self.tags = np.ones(n, np.uint32)
        self.tags[1::24] = 7
        base = FlatIndex(dim, n, gpu, storage=storage)
        base.upsert(x, np.arange(n), self.tags, new_count=n)
        self.rows16 = base.export_rows()
        self.rows32 = base.export_rows32() if storage == "fp32" else None
        np.testing.assert_array_equal(base.export_tags(), self.tags)
        base.close()
        self.sets = self.delete_sets(rng)
        # queries: a deleted row whose old slot (2101) lies past the new count in the new
        # partial last tile, the moved last row, a deleted row deep in the tail, the
        # duplicated block, perturbed survivors
        self.q = np.concatenate([x[[2101, 3000, 2900, 3]],
                                 x[[5, 1500, 49]] + 0.05 * rng.standard_normal(
                                     (3, dim)).astype(np.float32)]).astype(np.float32)
        self._expected, self._answers = {}, {}

    def delete_sets(self, rng):
        n = self.n
        # "search": 901 rows, so N1_SEARCH remain: 2100..2110 (stale bytes stay in the last,
        # partial tile of the shrunken index), 2900, half of the duplicated block, the rest
        # random; rows 3000 (moved into a hole) and 3 survive
        fixed = list(range(2100, 2111)) + [2900] + list(range(100, 120))
        pool = np.setdiff1d(np.arange(n), fixed + [3000, 3] + list(range(120, 140)))
        search = np.concatenate([fixed, rng.choice(pool, n - N1_SEARCH - len(fixed),
                                                   replace=False)])
        return {"last": np.array([n - 1]), "row0": np.array([0]),
                "block": np.arange(10, 41),
                "random30": rng.choice(n, (3 * n) // 10, replace=False),
                "random70": rng.choice(n, (7 * n) // 10, replace=False),
                "one_tag": np.nonzero(self.tags == 7)[0],
                "every": np.arange(n), "search": search}

    def load(self, index, rows16=None, rows32=None, tags=None):
        """The stored rows (default: all of the case's) into an empty index, bit for bit."""
        rows16 = self.rows16 if rows16 is None else rows16
        rows32 = self.rows32 if rows32 is None else rows32
        tags = self.tags if tags is None else tags
        m = len(tags)
        if m == 0:
            return index
        if self.storage == "fp32":
            index.import_rows32(rows32, 0, tags, new_count=m)
        else:
            index.import_rows(rows16, 0, tags, new_count=m)
        return index

    def flat(self):
        from ragmi.index import FlatIndex
        return self.load(FlatIndex(self.dim, self.n, self.gpu, storage=self.storage))

    def expected(self, name):
        """(rows16, rows32 or None, tags, n1): the numpy application of the plan."""
        if name not in self._expected:
            from ragmi.index import plan_removal
            src, dst, n1 = plan_removal(self.n, self.sets[name])

            def apply(a):
                if a is None:
                    return None
                a = a.copy()
                a[dst] = a[src]
                return np.ascontiguousarray(a[:n1])

            self._expected[name] = (apply(self.rows16), apply(self.rows32), apply(self.tags), n1)
        return self._expected[name]

    def answers(self, name, k, filtered):
        """Search results on the expected rows: the oracle's, and a fresh index's (loaded by
        import_rows / import_rows32), which must already agree."""
        key = (name, k, filtered)
        if key not in self._answers:
            from ragmi.index import FlatIndex
            r16, r32, tags, n1 = self.expected(name)
            stored = r32 if self.storage == "fp32" else r16
            kk = min(k, n1)
            if not filtered:
                s, i = O.search(stored, self.q, kk)
            else:
                parts = [O.search(stored, self.q[b:b + 1], kk, tags=tags, mask=int(m),
                                  value=int(v), use_filter=bool(m))
                         for b, (m, v) in enumerate(FILTERS)]
                s = np.concatenate([p[0] for p in parts])
                i = np.concatenate([p[1] for p in parts])
            s = np.pad(s, ((0, 0), (0, k - kk)), constant_values=-np.inf)
            i = np.pad(i, ((0, 0), (0, k - kk)), constant_values=-1)
            fresh = self.load(FlatIndex(self.dim, n1, self.gpu, storage=self.storage),
                              r16, r32, tags)
            same_answers(fresh, self, k, filtered, (s, i), "oracle")
            fresh.close()
            self._answers[key] = (s, i)
        return self._answers[key]


def same_answers(index, c, k, filtered, want, what):
    s, i = index.search(c.q, k, filters=FILTERS if filtered else None)
    torch.cuda.synchronize()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    np.testing.assert_array_equal(i, want[1], err_msg=f"ids vs {what}, k={k}")
    np.testing.assert_array_equal(s.view(np.int32), want[0].view(np.int32),
                                  err_msg=f"scores vs {what}, k={k}")
    return s, i


_cases = {}


def case(gpu, dim, storage):
    if (dim, storage) not in _cases:
        _cases[(dim, storage)] = Case(gpu, dim, storage)
    return _cases[(dim, storage)]


def same_stored(index, c, name):
    r16, r32, tags, n1 = c.expected(name)
    assert index.count == n1
    if n1 == 0:
        return
    np.testing.assert_array_equal(index.export_rows(0, n1), r16)
    np.testing.assert_array_equal(index.export_tags(0, n1), tags)
    if r32 is not None:
        np.testing.assert_array_equal(index.export_rows32(0, n1).view(np.uint32),
                                      r32.view(np.uint32))


CONFIGS = [(384, "fp16"), (384, "fp32"), (1024, "fp16"), (1024, "fp32")]


# ------------------------------------------------------------------ 3. remove_rows, bit for bit
@pytest.mark.parametrize("name", ["last", "row0", "block", "random30", "random70", "one_tag",
                                  "search"])
@pytest.mark.parametrize("dim,storage", CONFIGS)
def test_remove_rows_bit_for_bit(gpu, dim, storage, name):
    from ragmi.index import plan_removal
    c = case(gpu, dim, storage)
    idx = c.flat()
    rows = c.sets[name]
    if name == "one_tag":                                 # the rows come from the device
        sel, total = idx.select_rows(ALL, 7)
        np.testing.assert_array_equal(sel.cpu().numpy(), rows)
        rows = sel.cpu().numpy()
    src, dst, n1 = idx.remove_rows(np.concatenate([rows, rows[:5]]))      # duplicates collapse
    want = plan_removal(c.n, rows)
    assert n1 == want[2] == c.n - len(rows)
    np.testing.assert_array_equal(src, want[0])
    np.testing.assert_array_equal(dst, want[1])
    same_stored(idx, c, name)
    if name == "one_tag":
        assert idx.select_rows(ALL, 7)[1] == 0 and idx.select_rows(ALL, 1)[1] == n1
    idx.close()


@pytest.mark.parametrize("dim,storage", CONFIGS)
def test_remove_every_row_then_refill(gpu, dim, storage):
    c = case(gpu, dim, storage)
    idx = c.flat()
    src, dst, n1 = idx.remove_rows(c.sets["every"])
    assert (len(src), len(dst), n1, idx.count) == (0, 0, 0, 0)
    s, i = idx.search(c.q, 15)
    torch.cuda.synchronize()
    assert (i.cpu().numpy() == -1).all()                  # the old bytes are all past count
    rng = np.random.default_rng(3)
    m = 50
    y = rng.standard_normal((m, dim)).astype(np.float32)
    y[7] = c.x[2101]
    tags = np.full(m, 5, np.uint32)
    idx.upsert(y, np.arange(m), tags, new_count=m)
    enc = O.encode_rows32(y) if storage == "fp32" else O.encode_rows(y)
    for k in (15, 40):
        kk = min(k, m)
        s2, i2 = O.search(enc, c.q, kk)
        s, i = idx.search(c.q, k)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(i.cpu().numpy()[:, :kk], i2)
        np.testing.assert_array_equal(s.cpu().numpy()[:, :kk].view(np.int32), s2.view(np.int32))
        assert (i.cpu().numpy()[:, kk:] == -1).all()
    assert int(i[0, 0]) == 7
    idx.close()


def test_move_gather_scatter_directly(gpu):
    """The three copies on their own: gather equals export, scatter into another index equals
    import, and a pair whose row index lies outside [0, capacity) is skipped."""
    from ragmi.index import FlatIndex
    for dim, storage in ((384, "fp32"), (1024, "fp16")):
        c = case(gpu, dim, storage)
        idx = c.flat()
        rng = np.random.default_rng(11)
        rows = np.concatenate([np.arange(2990, 3001), rng.choice(2990, 200, replace=False)])
        f16, f32, tags = idx.gather_rows(rows)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(f16.cpu().numpy().view(np.uint16), c.rows16[rows])
        np.testing.assert_array_equal(tags.cpu().numpy().view(np.uint32), c.tags[rows])
        if storage == "fp32":
            np.testing.assert_array_equal(f32.cpu().numpy().view(np.uint32),
                                          c.rows32[rows].view(np.uint32))
        else:
            assert f32 is None
        other = FlatIndex(dim, 512, gpu, storage=storage)
        slots = rng.permutation(300)[:len(rows)]
        other.scatter_rows(slots, f16, f32, tags, new_count=300)
        assert other.count == 300
        got = other.export_rows(0, 300)
        np.testing.assert_array_equal(got[slots], c.rows16[rows])
        untouched = np.setdiff1d(np.arange(300), slots)
        assert not got[untouched].any()
        np.testing.assert_array_equal(other.export_tags(0, 300)[slots], c.tags[rows])
        if storage == "fp32":
            np.testing.assert_array_equal(other.export_rows32(0, 300)[slots].view(np.uint32),
                                          c.rows32[rows].view(np.uint32))
        # pairs with a row index of -1 or of the capacity itself are skipped
        cap = other.capacity
        before = other.export_rows(0, 300)
        other.move_rows([int(slots[0]), cap, -1, int(slots[1])], [cap, int(slots[2]), int(slots[3]),
                                                               int(untouched[0])], 300)
        after = other.export_rows(0, 300)
        before[untouched[0]] = before[slots[1]]
        np.testing.assert_array_equal(after, before)
        other.close()
        idx.close()


# ------------------------------------------------------------------ 4. search after removal
@pytest.mark.parametrize("dim,storage", CONFIGS)
def test_search_after_removal(gpu, dim, storage):
    c = case(gpu, dim, storage)
    idx = c.flat()
    idx.remove_rows(c.sets["search"])
    n1 = c.expected("search")[3]
    assert n1 == N1_SEARCH and n1 % 16
    for k in (15, 32, 100, 5000):
        for filtered in (False, True):
            s, i = same_answers(idx, c, k, filtered, c.answers("search", k, filtered),
                                "fresh index and oracle")
            assert i.max() < n1                            # nothing from past the new count
    s, i = same_answers(idx, c, 32, False, c.answers("search", 32, False), "oracle")
    # the deleted rows' queries find no copy of themselves; the moved last row is found once
    assert s[0, 0] < 0.9 and s[2, 0] < 0.9
    assert s[1, 0] > 0.999 and s[1, 1] < 0.9
    # the duplicated block lost rows 100..119: row 3, then the 20 survivors wherever they are
    tied = np.nonzero((c.expected("search")[0] == c.expected("search")[0][3]).all(axis=1))[0]
    assert len(tied) == 21 and i[3, :21].tolist() == tied.tolist()
    idx.close()


# ------------------------------------------------------------------ 5. ShardSet.remove_rows
def check_shardset(gpu, dim, storage, devices, names):
    from ragmi.shardset import ShardSet, shard_count
    c = case(gpu, dim, storage)
    for name in names:
        ss = c.load(ShardSet(dim, devices, c.n, storage))
        assert ss.count == c.n
        rows, total = ss.select_rows(ALL, 7)
        np.testing.assert_array_equal(rows.cpu().numpy(), np.nonzero(c.tags == 7)[0])
        assert total == rows.numel() and ss.select_rows(ALL, 7, cap=10)[0].numel() == 10
        src, dst, n1 = ss.remove_rows(c.sets[name])
        assert ss.count == n1 == c.expected(name)[3]
        assert [sh.count for sh in ss.shards] == \
            [shard_count(n1, s, ss.n) for s in range(ss.n)]
        same_stored(ss, c, name)                          # = the single index, test 3
        if n1:
            for k, filtered in ((15, False), (32, True), (100, False), (100, True)):
                same_answers(ss, c, k, filtered, c.answers(name, k, filtered), "single index")
        ss.close()


@pytest.mark.parametrize("storage", ["fp16", "fp32"])
@pytest.mark.parametrize("n_shards", [2, 3, 8])
def test_shardset_remove_rows(gpu, n_shards, storage):
    check_shardset(gpu, 384, storage, [gpu.index] * n_shards, ["search", "random70", "row0"])


def test_shardset_remove_rows_dim_1024_and_small_sets(gpu):
    check_shardset(gpu, 1024, "fp32", [gpu.index] * 3, ["search", "last", "every"])


def test_shardset_remove_rows_two_physical_devices(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("one HIP device visible")
    before = torch.cuda.current_device()
    check_shardset(gpu, 384, "fp32", [0, 1], ["search", "random70"])
    assert torch.cuda.current_device() == before


# ------------------------------------------------------------------ 6. QdrantClient.delete
TICKERS = ["AAPL", "MSFT", "NVDA", "AMD", "TSLA"]
DOCS = ["10-K", "10-Q", "8-K"]


def md5_id(i):
    return hashlib.md5(f"doc-{i}".encode()).hexdigest()


def payload_of(i, note):
    return {"ticker": TICKERS[i % 5], "document_type": DOCS[i % 3], "n": i, "note": note}


def points(res, version=True):
    return [(p.id, p.score, p.payload) + ((p.version,) if version else ()) for p in res.points]


def must(**kw):
    from ragmi import qdrant_models as m
    return m.Filter(must=[m.FieldCondition(key=k, match=m.MatchValue(value=v))
                          for k, v in kw.items()])


def run_sequence(c, x, x2):
    """The call sequence of the parity test; returns the model {n: (vector, payload)} of what
    must be left."""
    from ragmi import qdrant_models as m
    n = 400
    c.create_collection("t", m.VectorParams(size=x.shape[1], distance=m.Distance.COSINE))
    c.upsert("t", [m.PointStruct(id=md5_id(i), vector=x[i].tolist(), payload=payload_of(i, "a"))
                   for i in range(n)])                                               # 1
    alive = {i: (x[i], payload_of(i, "a")) for i in range(n)}
    gone = [0, 7, 7, 399, 250, 16, 33]
    r = c.delete("t", [md5_id(i) for i in gone] + [md5_id(5000), 123456])             # 2
    assert r.status == m.UpdateStatus.COMPLETED
    for i in gone:
        alive.pop(i, None)
    assert c.count("t").count == len(alive) == n - 6
    c.delete("t", m.FilterSelector(filter=must(ticker="AMD")))                        # 3
    alive = {i: v for i, v in alive.items() if i % 5 != 3}
    c.delete("t", must(ticker="MSFT", document_type="8-K"))                           # 4
    alive = {i: v for i, v in alive.items() if not (i % 5 == 1 and i % 3 == 2)}
    before = c.count("t").count
    c.delete("t", m.FilterSelector(filter=must(ticker="NEVER")))                      # 5
    c.delete("t", m.PointIdsList(points=[]))
    assert c.count("t").count == before == len(alive)
    col = c._col("t")
    moved = [i for i in alive if col.id_to_row[str(uuid.UUID(md5_id(i)))] != i]
    assert moved, "the sequence must have moved some point"
    over = moved[:3] + [4]
    c.upsert("t", [m.PointStruct(id=md5_id(i), vector=x2[i].tolist(),
                                 payload=payload_of(i, "b")) for i in over])          # 6
    for i in over:
        alive[i] = (x2[i], payload_of(i, "b"))
    c.upsert("t", [m.PointStruct(id=md5_id(i), vector=x[i].tolist(), payload=payload_of(i, "c"))
                   for i in range(n, n + 40)])                                        # 7
    alive.update({i: (x[i], payload_of(i, "c")) for i in range(n, n + 40)})
    return alive, over


def ask(c, q, x2, version=True):
    from ragmi import qdrant_models as m
    out = []
    for kw in (dict(limit=15), dict(limit=15, query_filter=must(ticker="AAPL")),
               dict(limit=100), dict(limit=1000, query_filter=must(ticker="TSLA",
                                                                   document_type="10-K")),
               dict(limit=10, query_filter=must(ticker="AMD")), dict(limit=5000)):
        for qq in q:
            out.append(points(c.query_points("t", query=qq, **kw), version))
    reqs = [m.QueryRequest(query=x2[j].tolist(), limit=5 + j,
                           filter=must(ticker="NVDA") if j % 2 else None, with_payload=True)
            for j in range(6)]
    out += [points(r, version) for r in c.query_batch_points("t", reqs)]
    out.append(c.count("t").count)
    out += [c.count("t", count_filter=must(ticker=t)).count for t in TICKERS + ["NEVER"]]
    out.append(c.count("t", count_filter=must(ticker="MSFT", document_type="10-K")).count)
    return out


def test_qdrant_client_delete_parity(gpu, tmp_path):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient, UnsupportedFilter
    rng = np.random.default_rng(21)
    dim = 384
    x = rng.standard_normal((440, dim)).astype(np.float32)
    x2 = rng.standard_normal((440, dim)).astype(np.float32)
    q = [x[5] + 0.1 * rng.standard_normal(dim).astype(np.float32), x[7], x2[4]]
    path = str(tmp_path / "store")
    a = QdrantClient(device=gpu, path=path)
    alive, over = run_sequence(a, x, x2)
    col = a._col("t")
    canon = {str(uuid.UUID(md5_id(i))): i for i in alive}
    assert sorted(col.row_ids) == sorted(canon) and a.count("t").count == len(alive)
    with pytest.raises(UnsupportedFilter):
        a.delete("t", m.Filter(must_not=[m.FieldCondition(key="ticker",
                                                          match=m.MatchValue(value="AMD"))]))
    want_v = ask(a, q, x2)
    want = ask(a, q, x2, version=False)
    assert all(p[2]["n"] in alive and p[2] == alive[p[2]["n"]][1]
               for res in want[:-8] for p in res)
    assert len(want[0]) == 15 and len(want[15]) == len(alive)
    # every AMD point was deleted in step 3; step 7 ingested 8 new ones (403, 408, ..., 438)
    assert sorted(p[2]["n"] for p in want[12]) == list(range(403, 440, 5))
    assert want[-8] == len(alive) and want[-4] == 8 and want[-2] == 0      # AMD, NEVER
    assert want[-7] == len([i for i in alive if i % 5 == 0])
    # deleted ids are gone, moved and overwritten ids answer with their own payloads
    assert a.retrieve("t", [md5_id(i) for i in (0, 7, 399, 3, 8)]) == []
    probe = over + [i for i in alive if col.id_to_row[str(uuid.UUID(md5_id(i)))] != i][:5]
    got = a.retrieve("t", [md5_id(i) for i in probe], with_vectors=True)
    assert [r.payload for r in got] == [alive[i][1] for i in probe]
    enc = O.encode_rows32(np.stack([alive[i][0] for i in probe]))
    np.testing.assert_array_equal(np.asarray([r.vector for r in got], np.float32), enc)
    # sharded clients under the same calls: everything equal, versions too
    for n_shards in (2, 3):
        b = QdrantClient(device=gpu, devices=[gpu.index] * n_shards)
        run_sequence(b, x, x2)
        assert b._col("t").row_ids == col.row_ids
        assert ask(b, q, x2) == want_v
        b.close()
    # a client that never held the deleted points: the survivors in a's final row order
    f = QdrantClient(device=gpu)
    f.create_collection("t", m.VectorParams(size=dim, distance=m.Distance.COSINE))
    order = [canon[pid] for pid in col.row_ids]
    f.upsert("t", [m.PointStruct(id=md5_id(i), vector=alive[i][0].tolist(), payload=alive[i][1])
                   for i in order])
    assert ask(f, q, x2, version=False) == want
    f.close()
    # persistence: the index stayed dense, the shard format is unchanged
    a.close()                                                              # saves
    for devs in (None, [gpu.index] * 3):
        d = QdrantClient(device=gpu, devices=devs, path=path)
        assert ask(d, q, x2) == want_v
        d.path = None
        d.close()


# ------------------------------------------------------------------ 7. searches during deletes
def test_queries_during_deletes(gpu):
    """Coalesced query_points from several threads while one thread deletes and re-upserts
    batches: every returned point carries its own payload and its own exact score, and no
    search that started after a delete had returned (and ended before the re-upsert began)
    returns a deleted id."""
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    rng = np.random.default_rng(31)
    n, dim, n_q, n_threads = 600, 384, 8, 4
    x = rng.standard_normal((n, dim)).astype(np.float32)
    qs = x[rng.choice(n, n_q)] + 0.3 * rng.standard_normal((n_q, dim)).astype(np.float32)
    # the exact score of every id for every query (fp32 storage): a point's score does not
    # depend on the row it sits in
    s_all, i_all = O.search(O.encode_rows32(x), qs, n)
    score = np.empty((n_q, n), np.float32)
    np.put_along_axis(score, i_all, s_all, axis=1)
    c = QdrantClient(device=gpu, coalesce_window_s=0.0005)
    c.create_collection("t", m.VectorParams(size=dim, distance=m.Distance.COSINE))

    def pts(ids):
        return [m.PointStruct(id=int(i), vector=x[i].tolist(),
                              payload={"ticker": TICKERS[i % 5], "n": int(i)}) for i in ids]

    c.upsert("t", pts(range(n)))
    batches = [rng.choice(n, 40, replace=False) for _ in range(30)]
    absent = []                    # (id, delete returned, re-upsert began)
    done = threading.Event()
    errs, seen = [], []

    def deleter():
        try:
            held = []              # (ids, time their delete returned)
            for b in batches:
                live = [int(i) for i in b if all(int(i) not in h[0] for h in held)]
                c.delete("t", live if len(held) % 2 else m.PointIdsList(points=live))
                held.append((live, time.perf_counter()))
                if len(held) == 2:                        # re-upsert the older batch
                    ids, t_del = held.pop(0)
                    t_up = time.perf_counter()
                    absent.extend((i, t_del, t_up) for i in ids)
                    c.upsert("t", pts(ids))
            absent.extend((i, held[0][1], float("inf")) for i in held[0][0])   # never back
            c.delete("t", must(ticker="TSLA"))
            t_del = time.perf_counter()
            absent.extend((i, t_del, float("inf")) for i in range(n) if i % 5 == 4)
        except BaseException as e:
            errs.append(e)
        finally:
            done.set()

    def searcher(t):
        try:
            j = t
            for it in range(2000):
                last = done.is_set()                      # one more round after the deleter
                flt = must(ticker=TICKERS[j % 5]) if j % 3 == 0 else None
                t0 = time.perf_counter()
                res = c.query_points("t", query=qs[j % n_q], limit=10, query_filter=flt)
                seen.append((j % n_q, flt is not None and TICKERS[j % 5], t0,
                             time.perf_counter(), [(p.id, p.score, p.payload) for p in res.points]))
                j += n_threads
                if last:
                    break
        except BaseException as e:
            errs.append(e)

    th = [threading.Thread(target=searcher, args=(t,)) for t in range(n_threads)]
    th.append(threading.Thread(target=deleter))
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert len(seen) >= n_threads and any(len(p) for *_, p in seen)
    gaps = {}
    for i, a, b in absent:
        gaps.setdefault(i, []).append((a, b))
    for jq, ticker, t0, t1, found in seen:
        assert len({pid for pid, _, _ in found}) == len(found)
        for pid, sc, payload in found:
            assert payload["n"] == pid and payload["ticker"] == TICKERS[pid % 5]
            assert not ticker or payload["ticker"] == ticker
            assert np.float32(sc) == score[jq, pid], (pid, sc, score[jq, pid])
            for a, b in gaps.get(pid, ()):
                assert not (a <= t0 and t1 <= b), f"id {pid} returned while deleted"
        assert [s for _, s, _ in found] == sorted((s for _, s, _ in found), reverse=True)
    # afterwards: the collection is what the calls left, and searches agree with a fresh client
    left = [i for i in range(n) if not any(b == float("inf") for a, b in gaps.get(i, ()))]
    assert c.count("t").count == len(left) and sorted(c._col("t").row_ids) == left
    f = QdrantClient(device=gpu)
    f.create_collection("t", m.VectorParams(size=dim, distance=m.Distance.COSINE))
    f.upsert("t", pts(c._col("t").row_ids))
    for j in range(n_q):
        assert [(p.id, p.score, p.payload) for p in c.query_points("t", query=qs[j], limit=15).points] \
            == [(p.id, p.score, p.payload) for p in f.query_points("t", query=qs[j], limit=15).points]
    f.close()
    c.close()
