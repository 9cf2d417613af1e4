"""GPU tests of range and datetime filters: filter_view_kernel with key columns
against its numpy restatement bit for bit, the key columns' write / gather / reserve / create,
the view search against the exact oracle over the same view, and the client routes (one index
and three logical shards: query, count, batch, MMR, groups, fusion, deletes, overwrites, growth,
create_payload_index, save / load, rag) against brute force over a plain evaluator that never
sees a key (_range_ref). Nothing here carries a tolerance.

No GPU test feeds the kernel a malformed blob: its two RANGE guards (a column at or past the
index's columns, bounds ending past the blob) are covered by the numpy restatement
(tests/test_range_cpu.py::test_blob_layout_and_guards), which the kernel is held equal to on
well-formed blobs here."""
import datetime as dt

import numpy as np
import pytest
import torch

import oracle_scan as O
from _range_ref import matches_range

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
N_ROWS = 3001          # no multiple of 16: the last tile is partial
TICKERS = [f"T{i:02d}" for i in range(12)]
TYPES = ["10-K", "10-Q", "8-K"]
KINDS = {"fiscal_year": "number", "ingested_at": "datetime", "revenue": "number",
         "pages": "number"}
UTC = dt.timezone.utc


def P(atoms, table):
    from ragmi.filters import FilterProgram
    return FilterProgram(tuple(atoms), table)


# ------------------------------------------------------------------ 1. the kernel
KEY_POOL = 12          # distinct key values per column, so that bounds hit stored values
_kernel = {}


def key_values(n_cols):
    from ragmi.filters import KEY_ABSENT, key_of_float
    vals = [-np.inf, -1e300, -2.5, -5e-324, 0.0, 5e-324, 1.0, float(np.nextafter(1.0, 2)),
            2.0 ** 53, 1e300, np.inf]
    return np.array([[key_of_float(v + c if abs(v) < 10 else v) for v in vals] + [KEY_ABSENT]
                     for c in range(n_cols)], np.int64)


def kernel_case(gpu, count, n_cols):
    """An index of `count` rows (capacity well past it) with random tags and `n_cols` key
    columns of random keys (some absent)."""
    if (count, n_cols) not in _kernel:
        from ragmi.index import FlatIndex
        rng = np.random.default_rng(count + n_cols)
        tags = (rng.integers(0, 50, count).astype(np.uint32) |
                (rng.integers(0, 20, count).astype(np.uint32) << np.uint32(16)))
        vals = key_values(n_cols)
        keys = np.stack([vals[c][rng.integers(0, KEY_POOL, count)] for c in range(n_cols)])
        idx = FlatIndex(384, count + 37, gpu, "fp16")
        v = torch.zeros((count, 384), dtype=torch.float32, device=gpu)
        v[:, 0] = 1.0
        idx.upsert(v, np.arange(count), tags, new_count=count)
        idx.keys_create(n_cols)
        assert idx.keys_cols() == n_cols
        for c in range(n_cols):
            idx.write_keys(c, np.arange(count), keys[c])
        _kernel[(count, n_cols)] = (idx, tags, keys)
    return _kernel[(count, n_cols)]


def random_program(rng, n_atoms, n_cols):
    vals = key_values(n_cols)
    atoms = []
    while len(atoms) < n_atoms:
        kind = int(rng.integers(0, 4))
        f = int(rng.integers(0, 2))
        hi = (50, 20)[f]
        if kind == 0:
            a = ("maskeq", 0xFFFF << (16 * f), int(rng.integers(0, hi)) << (16 * f))
        elif kind == 1:
            bm = int.from_bytes(rng.bytes((hi + 8) // 8), "little") & ((1 << hi) - 1)
            a = ("inset", f, bm, hi)
        else:
            c = int(rng.integers(0, n_cols))
            lo, hi = sorted(int(x) for x in vals[c][rng.integers(0, KEY_POOL - 1, 2)])
            a = ("range", c, lo + int(rng.integers(0, 2)), hi - int(rng.integers(0, 2)))
            if a[2] > a[3]:
                continue
        if a not in atoms:
            atoms.append(a)
    table = int.from_bytes(rng.bytes(32), "little") & ((1 << (1 << n_atoms)) - 1)
    return P(atoms, table)


def check_view(idx, tags, keys, blob, n_programs=None):
    from ragmi.filters import eval_view_np
    cap = idx.capacity
    assert cap % 16 == 0 and cap > idx.count
    out = torch.full((cap + 64,), CANARY, dtype=torch.int32, device=idx.device)
    got = idx.filter_view(blob, n_programs=n_programs, out=out)
    torch.cuda.synchronize()
    full = out.cpu().numpy().view(np.uint32)
    n = idx.count
    want = np.zeros(cap, np.uint32)
    want[:n] = eval_view_np(blob, tags[:n], n_programs, keys=keys[:, :n])
    np.testing.assert_array_equal(full[:cap], want)
    assert (full[cap:] == CANARY).all()                    # nothing past the column
    assert got.shape == (cap,)
    return want[:n]


@pytest.mark.parametrize("U", [1, 32])
@pytest.mark.parametrize("n_cols", [1, 4])
@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, 1025, 70_001])
def test_filter_view_with_keys_equals_numpy(gpu, count, n_cols, U):
    from ragmi.filters import pack_view
    idx, tags, keys = kernel_case(gpu, count, n_cols)
    rng = np.random.default_rng(1000 * U + 10 * count + n_cols)
    sizes = [8, 1, 3] + [int(x) for x in rng.integers(0, 9, 32)]
    progs = [random_program(rng, n, n_cols) for n in sizes[:U]]
    while not any(a[0] == "range" for a in progs[0].atoms):
        progs[0] = random_program(rng, 8, n_cols)
    if U > 3:
        progs[1] = P([("range", n_cols - 1, int(keys[-1].max()) + 1, (1 << 63) - 1)], 0b10)  # none
        progs[3] = P([("maskeq", 0, 0)], 0b10)                                  # a tag-only program
    assert any(a[0] == "range" for p in progs for a in p.atoms)
    want = check_view(idx, tags, keys, pack_view(progs))
    if count > 1000:
        assert len(np.unique(want)) > 1
        if U > 3:
            assert not (want & 2).any() and (want & 8).all()


def test_rows_past_the_count_read_zero_over_stale_keys(gpu):
    """Keys (and tags) written up to row 1025, then the count set down to 600: rows at and past
    it read 0 though their stale keys would pass; and the full-interval atom."""
    from ragmi.filters import KEY_MAX, KEY_MIN, pack_view
    idx, tags, keys = kernel_case(gpu, 1025, 4)
    present = P([("range", 2, KEY_MIN, KEY_MAX)], 0b10)
    blob = pack_view([present, P([("range", 2, KEY_MIN, KEY_MAX)], 0b01)])
    full = check_view(idx, tags, keys, blob)
    assert (full[600:] & 1).any() and (full[600:] & 2).any()
    try:
        idx.set_count(600)
        cut = check_view(idx, tags, keys, blob)
        np.testing.assert_array_equal(cut, full[:600])
        idx.set_count(598)                                  # inside a lane's 4 rows
        np.testing.assert_array_equal(check_view(idx, tags, keys, blob), full[:598])
    finally:
        idx.set_count(1025)


def test_bounds_read_from_global_memory(gpu):
    """A bitmap pool above 32 KiB: only the records are staged in LDS, and the RANGE bounds, as
    the bitmaps, come from global memory."""
    from ragmi.filters import pack_view, view_programs
    idx, tags, keys = kernel_case(gpu, 70_001, 4)
    rng = np.random.default_rng(9)
    codes = 40_000
    vals = key_values(4)
    progs = []
    for s in range(8):
        bm = int.from_bytes(rng.bytes(codes // 8 + 1), "little") & ((1 << codes) - 1)
        c = s % 4
        progs.append(P([("inset", 0, bm, codes), ("range", c, int(vals[c][2]), int(vals[c][8])),
                        ("range", (c + 1) % 4, int(vals[(c + 1) % 4][5]), (1 << 63) - 1)],
                       int(rng.integers(1, 255))))
    blob = pack_view(progs)
    assert len(blob) > 8192 and view_programs(blob) == 8            # kFvLdsWords
    want = check_view(idx, tags, keys, blob)
    assert len(np.unique(want)) > 8
    small = pack_view([P([a for a in p.atoms if a[0] == "range"], 0b0110) for p in progs])
    assert len(small) <= 8192
    check_view(idx, tags, keys, small)


# ------------------------------------------------------------------ 2. the key columns
def test_write_gather_reserve_create(gpu):
    from ragmi.filters import KEY_ABSENT
    from ragmi.index import FlatIndex
    rng = np.random.default_rng(3)
    idx = FlatIndex(384, 1000, gpu, "fp16")
    try:
        cap = idx.capacity
        assert idx.keys_cols() == 0
        idx.keys_create(1)
        every = torch.arange(cap, device=gpu)
        assert (idx.gather_keys(0, every) == KEY_ABSENT).all()          # a new column is absent
        rows = rng.choice(cap, 700, replace=False)                     # duplicate-free
        vals = rng.integers(-(1 << 63) + 1, (1 << 63) - 1, 700, dtype=np.int64)
        idx.write_keys(0, rows, vals)
        want = np.full(cap, KEY_ABSENT, np.int64)
        want[rows] = vals
        np.testing.assert_array_equal(idx.gather_keys(0, every).cpu().numpy(), want)
        probe = np.array([[rows[0], cap, -1], [cap + 5, rows[1], 1 << 40]], np.int64)
        got = idx.gather_keys(0, probe).cpu().numpy()
        assert got.shape == (2, 3)
        assert got.tolist() == [[vals[0], KEY_ABSENT, KEY_ABSENT], [KEY_ABSENT, vals[1], KEY_ABSENT]]
        idx.write_keys(0, np.array([cap, -7, 1 << 40]), np.array([1, 2, 3]))     # skipped
        np.testing.assert_array_equal(idx.gather_keys(0, every).cpu().numpy(), want)
        idx.keys_create(3)                                  # 1 -> 3 keeps column 0
        idx.keys_create(2)                                  # the number only grows
        assert idx.keys_cols() == 3
        np.testing.assert_array_equal(idx.gather_keys(0, every).cpu().numpy(), want)
        assert (idx.gather_keys(2, every) == KEY_ABSENT).all()
        idx.write_keys(2, rows[:10], vals[:10] // 2)
        idx.reserve(3 * cap)                                # old keys kept, new rows absent
        cap2 = idx.capacity
        assert cap2 >= 3 * cap
        got = idx.gather_keys(0, torch.arange(cap2, device=gpu)).cpu().numpy()
        np.testing.assert_array_equal(got[:cap], want)
        assert (got[cap:] == KEY_ABSENT).all()
        got2 = idx.gather_keys(2, torch.arange(cap2, device=gpu)).cpu().numpy()
        assert got2[rows[:10]].tolist() == (vals[:10] // 2).tolist()
        assert (np.delete(got2, rows[:10]) == KEY_ABSENT).all()
        # move_rows carries every column
        idx.set_count(cap)
        idx.move_rows(rows[:5], np.setdiff1d(np.arange(cap), rows)[:5], cap)
        dst = np.setdiff1d(np.arange(cap), rows)[:5]
        assert idx.gather_keys(0, dst).cpu().numpy().tolist() == vals[:5].tolist()
        assert idx.gather_keys(2, dst).cpu().numpy().tolist() == (vals[:5] // 2).tolist()
        assert (idx.gather_keys(1, dst) == KEY_ABSENT).all()
        from ragmi._lib import RagmiError
        for bad in (lambda: idx.keys_create(5), lambda: idx.keys_create(0),
                    lambda: idx.write_keys(3, [0], [0]), lambda: idx.gather_keys(-1, [0])):
            with pytest.raises(RagmiError):
                bad()
    finally:
        idx.close()


# ------------------------------------------------------------------ 3. search over the view
def corpus_payloads(rng, n):
    """12 tickers x 3 types and four range fields, each absent (missing, or a value its kind
    does not take) for some points; exactly rows 7, 700, 1500, 2222, 3000 hold fiscal_year
    2025.5."""
    t0 = dt.datetime(2023, 1, 1, tzinfo=UTC)
    pay = []
    for r in range(n):
        p = {"ticker": TICKERS[rng.integers(0, 12)], "document_type": TYPES[rng.integers(0, 3)],
             "n": r}
        if rng.random() < 0.06:
            del p["ticker"]
        u = rng.random()
        if u < 0.7:
            p["fiscal_year"] = int(rng.integers(2018, 2025))
        elif u < 0.8:
            p["fiscal_year"] = float(rng.integers(2018, 2025)) + 0.25
        elif u < 0.85:
            p["fiscal_year"] = ["FY2021", None, [2021], True][rng.integers(0, 4)]
        if rng.random() < 0.85:
            d = t0 + dt.timedelta(minutes=int(rng.integers(0, 2 * 365 * 24 * 60)))
            p["ingested_at"] = [d.isoformat(), d.strftime("%Y-%m-%dT%H:%M:%SZ"),
                                d.astimezone(dt.timezone(dt.timedelta(hours=9))).isoformat(),
                                d.date().isoformat()][rng.integers(0, 4)]
        if rng.random() < 0.75:
            p["revenue"] = float(rng.choice([-2.5e9, -1.0, -0.0, 0.0, 1.0, 3.25e9])) * \
                float(rng.integers(1, 4))
        if rng.random() < 0.75:
            p["pages"] = int(rng.integers(-3, 60))
        pay.append(p)
    for r in (7, 700, 1500, 2222, 3000):
        pay[r] = dict(pay[r], fiscal_year=2025.5)
    return pay


def named_filters():
    from ragmi import qdrant_models as m
    fc = m.FieldCondition
    year = lambda **kw: fc("fiscal_year", range=m.Range(**kw))
    at = lambda **kw: fc("ingested_at", range=m.DatetimeRange(**kw))
    return {
        "since": m.Filter(must=[at(gte="2024-01-01T00:00:00Z")]),
        "years": m.Filter(must=[year(gte=2021, lte=2023)]),
        "ticker_window": m.Filter(must=[fc("ticker", m.MatchAny(any=["T03", "T04", "T05"])),
                                        at(gte="2023-06-01", lt=dt.datetime(2024, 6, 1, 9, tzinfo=dt.timezone(dt.timedelta(hours=9))))]),
        "not_old": m.Filter(must_not=[year(lt=2021), fc("document_type", m.MatchValue("8-K"))]),
        "should_mix": m.Filter(should=[fc("revenue", range={"gt": 0}), fc("ticker", m.MatchValue("T01"))],
                               must_not=[fc("pages", range=m.Range(gte=30))]),
        "min_should": m.Filter(min_should=m.MinShould(
            [year(gt=2022), fc("pages", range=m.Range(lte=0)), fc("revenue", range=m.Range(lt=0.0)),
             m.IsEmptyCondition(m.PayloadField("ingested_at")),
             fc("document_type", m.MatchValue("10-K"))], 2)),
        "no_year": m.Filter(must=[m.IsEmptyCondition(m.PayloadField("fiscal_year"))],
                            should=[m.Filter(must=[fc("revenue", range=m.Range(gte=0.0, lte=0.0))]),
                                    at(lt="2023-03-01")]),
        "few": m.Filter(must=[year(gte=2025.5, lte=2025.5)]),
        "none": m.Filter(must=[year(gt=9999)]),
    }


_corpus = {}


def corpus(dim):
    """Rows, payloads, tags, keys, queries and the programs of one dim, computed once: 3001 rows
    with a 64-row near-duplicate cluster, 40 queries, the first eight aimed at the cluster."""
    if dim not in _corpus:
        from ragmi.filters import PayloadRanges, compile_program, eval_view_np, pack_view
        from ragmi.qdrant import PayloadTags
        rng = np.random.default_rng(dim + 1)
        x = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
        base = rng.standard_normal((1, dim)).astype(np.float32)
        dup = np.sort(rng.choice(N_ROWS, 64, replace=False))
        x[dup] = base + 1e-5 * rng.standard_normal((64, dim)).astype(np.float32)
        pay = corpus_payloads(rng, N_ROWS)
        pt, pr = PayloadTags(), PayloadRanges(KINDS)
        tags = np.array([pt.tag(p) for p in pay], np.uint32)
        keys = np.array([pr.keys(p) for p in pay], np.int64).T.copy()
        B = 40
        q = rng.standard_normal((B, dim)).astype(np.float32)
        q[:8] = base + 0.02 * rng.standard_normal((8, dim)).astype(np.float32)
        flts = named_filters()
        progs = [compile_program(pt, f, pr) for f in flts.values()]
        blob = pack_view(progs)
        view = eval_view_np(blob, tags, keys=keys)
        for s, f in enumerate(flts.values()):                   # the view is the plain evaluator's
            want = np.array([matches_range(f, p, KINDS) for p in pay])
            np.testing.assert_array_equal((view >> s) & 1, want)
            assert 50 < want.sum() < N_ROWS - 50 or s >= 7
        assert int(((view >> 7) & 1).sum()) == 5 and not ((view >> 8) & 1).any()
        slot = np.arange(B) % 10            # slot 9: (0, 0), every row
        filt = np.array([[0, 0] if s == 9 else [1 << s, 1 << s] for s in slot], np.uint32)
        _corpus[dim] = dict(x=x, pay=pay, pt=pt, pr=pr, tags=tags, keys=keys, q=q, flts=flts,
                            progs=progs, blob=blob, view=view, slot=slot, filt=filt, dup=dup,
                            oracle={})
    return _corpus[dim]


def oracle_lists(c, storage, k):
    if (storage, k) not in c["oracle"]:
        rows = O.encode_rows(c["x"]) if storage == "fp16" else O.encode_rows32(c["x"])
        B = len(c["q"])
        s = np.empty((B, k), np.float32)
        i = np.empty((B, k), np.int64)
        for slot in range(10):
            sel = np.nonzero(c["slot"] == slot)[0]
            m = 0 if slot == 9 else 1 << slot
            s[sel], i[sel] = O.search(rows, c["q"][sel], k, tags=c["view"], mask=m, value=m,
                                      use_filter=True)
        c["oracle"][(storage, k)] = (s, i)
    return c["oracle"][(storage, k)]


_index = {}


def view_index(gpu, dim, storage):
    if (dim, storage) not in _index:
        from ragmi.index import FlatIndex
        c = corpus(dim)
        idx = FlatIndex(dim, N_ROWS, gpu, storage)
        idx.upsert(c["x"], np.arange(N_ROWS), c["tags"], new_count=N_ROWS)
        idx.keys_create(4)
        for col in range(4):
            idx.write_keys(col, np.arange(N_ROWS), c["keys"][col])
        _index[(dim, storage)] = idx
    return _index[(dim, storage)]


@pytest.mark.parametrize("dim,storage,how", [
    (384, "fp16", "k15"), (384, "fp16", "k100"), (384, "fp16", "full"),
    (384, "fp32", "k15"), (384, "fp32", "k100"), (384, "fp32", "full"), (1024, "fp16", "k15")])
def test_range_view_search_equals_oracle(gpu, dim, storage, how):
    """The scan, the large-k pass and the forced full pass over a view with RANGE atoms: ids and
    scores bit-equal to the oracle over the numpy view; a program matching fewer than k rows and
    one matching none; cluster queries inside the MFMA error band."""
    c = corpus(dim)
    idx = view_index(gpu, dim, storage)
    k = 100 if how == "k100" else 15
    s, i = idx.search(c["q"], k, filters=c["filt"], programs=c["blob"], full=how == "full")
    torch.cuda.synchronize()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    s2, i2 = oracle_lists(c, storage, k)
    np.testing.assert_array_equal(i, i2)
    np.testing.assert_array_equal(s, s2)
    assert (i[c["slot"] == 8] == -1).all()                          # matches none
    few = i[c["slot"] == 7]
    assert ((few >= 0).sum(axis=1) == 5).all() and (few[:, 5:] == -1).all()   # padding
    assert np.isin(i[9], c["dup"]).any() or np.isin(i[0], c["dup"]).any()
    assert idx.unanswered() == 0
    rows, total = idx.select_rows_view(c["blob"])                   # the blob's first program
    want = np.nonzero(c["view"] & 1)[0]
    assert total == len(want) and rows.cpu().numpy().tolist() == want.tolist()


# ------------------------------------------------------------------ 4. the client
_clients = {}


def make_client(gpu, devices, ids, range_fields=KINDS, capacity=N_ROWS, name="c"):
    """A 384-d collection (fp32 storage, the client's default) holding corpus points `ids`, in
    that row order."""
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    c = corpus(384)
    cl = QdrantClient(device=gpu, devices=devices)
    cl.create_collection(name, m.VectorParams(size=384, distance=m.Distance.COSINE),
                         capacity=capacity, payload_range_fields=range_fields)
    ids = list(ids)
    if ids:
        cl.upsert(name, m.Batch(ids=ids, vectors=c["x"][ids], payloads=[c["pay"][i] for i in ids]))
    return cl


def client(gpu, devices=None):
    key = None if devices is None else tuple(devices)
    if key not in _clients:
        _clients[key] = make_client(gpu, devices, range(N_ROWS))
    return _clients[key]


def brute_hits(cl, q, flt, k, name="c", x=None):
    """Exact top-k over the points the plain evaluator lets through, from the collection's
    current rows: [(id, score)]."""
    col = cl._col(name)
    x = corpus(384)["x"][np.asarray(col.row_ids)] if x is None else x
    ok = np.array([flt is None or matches_range(flt, p, KINDS) for p in col.payloads], np.uint32)
    s, i = O.search(O.encode_rows32(x), np.asarray(q, np.float32).reshape(1, -1), k, tags=ok,
                    mask=1, value=1, use_filter=True)
    return [(col.row_ids[r], sc) for r, sc in zip(i[0].tolist(), s[0].tolist()) if r >= 0]


def hits_of(resp):
    return [(p.id, np.float32(p.score)) for p in resp.points]


def same(resp, want):
    got = hits_of(resp)
    assert [h[0] for h in got] == [h[0] for h in want]
    assert [h[1] for h in got] == [np.float32(h[1]) for h in want]


def test_client_routes_equal_brute_force(gpu):
    from ragmi import qdrant_models as m
    c = corpus(384)
    flts, pay = c["flts"], c["pay"]
    one, three = client(gpu), client(gpu, [0, 0, 0])
    for name, flt in flts.items():
        want_n = sum(matches_range(flt, p, KINDS) for p in pay)
        assert one.count("c", count_filter=flt).count == want_n, name
        assert three.count("c", count_filter=flt).count == want_n, name
    for cl in (one, three):
        for j, (name, limit) in enumerate([("since", 10), ("years", 100), ("not_old", 5000),
                                           ("ticker_window", 10), ("should_mix", 100),
                                           ("min_should", 5000), ("no_year", 10), ("few", 10),
                                           ("none", 100)]):
            r = cl.query_points("c", query=c["q"][j], limit=limit, query_filter=flts[name])
            same(r, brute_hits(cl, c["q"][j], flts[name], min(limit, N_ROWS)))
            assert all(p.payload == pay[p.id] for p in r.points)
            assert bool(r.points) == (name != "none")
    legacy = m.Filter(must=[m.FieldCondition("ticker", m.MatchValue("T04"))])
    tag_only = m.Filter(must_not=[m.FieldCondition("document_type", m.MatchValue("8-K"))])
    mmr0 = m.NearestQuery(nearest=c["q"][3].tolist(), mmr=m.Mmr(diversity=0.0, candidates_limit=12))
    mmr5 = m.NearestQuery(nearest=c["q"][1].tolist(), mmr=m.Mmr(diversity=0.5, candidates_limit=40))
    reqs = [m.QueryRequest(query=c["q"][0].tolist(), filter=legacy, limit=10),
            m.QueryRequest(query=c["q"][1].tolist(), filter=tag_only, limit=10),
            m.QueryRequest(query=c["q"][2].tolist(), filter=flts["since"], limit=7),
            m.QueryRequest(query=mmr0, filter=flts["years"], limit=12),
            m.QueryRequest(query=mmr5, filter=flts["ticker_window"], limit=10),
            m.QueryRequest(query=c["q"][4].tolist(), filter=flts["since"], limit=3),
            m.QueryRequest(query=c["q"][5].tolist(), filter=flts["few"], limit=10),
            m.QueryRequest(query=c["q"][6].tolist(), filter=None, limit=5)]
    plain = [r for r in reqs if not isinstance(r.query, m.NearestQuery)]
    for cl in (one, three):
        for batch in (plain, reqs):
            out = cl.query_batch_points("c", batch)
            for r, resp in zip(batch, out):
                vec, mmr = (r.query.nearest, r.query.mmr) if isinstance(r.query, m.NearestQuery) \
                    else (r.query, None)
                if mmr is None or mmr.diversity == 0.0:     # diversity 0: the plain top-k
                    same(resp, brute_hits(cl, vec, r.filter, r.limit))
                solo = cl.query_points("c", query=r.query, limit=r.limit, query_filter=r.filter)
                assert hits_of(resp) == hits_of(solo)
                assert [p.payload for p in resp.points] == [p.payload for p in solo.points]
    a = one.query_batch_points("c", reqs)
    b = three.query_batch_points("c", reqs)
    assert [hits_of(x) for x in a] == [hits_of(x) for x in b]
    picked = hits_of(a[4])
    assert len(picked) == 10
    assert all(matches_range(flts["ticker_window"], pay[i], KINDS) for i, _ in picked)


def test_groups_and_fusion_equal_a_collection_of_the_matching_points(gpu):
    """A fusion request with a DatetimeRange on a prefetch, and a grouped request, against the
    same request over a collection that holds only the matching points (in the same row
    order). The grouped request carries a legacy document_type filter, the only kind it takes:
    query_points_groups composes (mask, value) pairs and refuses every general filter, a range
    included, as before; what is checked is that groups still work over an index that holds key
    columns."""
    from ragmi import qdrant_models as m
    from ragmi.qdrant import UnsupportedFilter
    c = corpus(384)
    since = c["flts"]["since"]
    keep = [i for i, p in enumerate(c["pay"]) if matches_range(since, p, KINDS)]
    for devices in (None, [0, 0, 0]):
        cl = client(gpu, devices)
        only = make_client(gpu, devices, keep)
        try:
            pre = lambda f: [m.Prefetch(query=c["q"][0].tolist(), filter=f, limit=40),
                             m.Prefetch(query=c["q"][9].tolist(), filter=f, limit=25)]
            got = cl.query_points("c", prefetch=pre(since), query=m.FusionQuery(fusion=m.Fusion.RRF),
                                  limit=30)
            want = only.query_points("c", prefetch=pre(None), query=m.FusionQuery(fusion=m.Fusion.RRF),
                                     limit=30)
            assert hits_of(got) == hits_of(want) and len(got.points) == 30
            assert [p.payload for p in got.points] == [p.payload for p in want.points]
            # groups on an index with key columns: the tags still gather, under a legacy filter
            typ = m.Filter(must=[m.FieldCondition("document_type", m.MatchValue("10-K"))])
            k10 = [i for i, p in enumerate(c["pay"]) if p.get("document_type") == "10-K"]
            only10 = make_client(gpu, devices, k10)
            try:
                g = cl.query_points_groups("c", query=c["q"][1].tolist(), group_by="ticker",
                                           limit=4, group_size=3, query_filter=typ)
                w = only10.query_points_groups("c", query=c["q"][1].tolist(), group_by="ticker",
                                               limit=4, group_size=3)
                assert [(x.id, [(p.id, p.score) for p in x.hits]) for x in g.groups] == \
                    [(x.id, [(p.id, p.score) for p in x.hits]) for x in w.groups]
                assert len(g.groups) == 4
            finally:
                only10.close()
            with pytest.raises(UnsupportedFilter, match="query_points_groups takes only"):
                cl.query_points_groups("c", query=c["q"][1].tolist(), group_by="ticker",
                                       query_filter=since)
        finally:
            only.close()


# ------------------------------------------------------------------ 5. keys follow their rows
def check_against_survivors(gpu, cl, devices, names=("since", "years", "not_old", "no_year", "few")):
    """Every range query and count of `cl` equals that of a fresh collection built from its
    surviving points in its current row order; every live row's keys are its payload's."""
    c = corpus(384)
    col = cl._col("c")
    fresh = make_client(gpu, devices, col.row_ids)
    try:
        assert fresh._col("c").payloads == col.payloads
        for j, name in enumerate(names):
            flt = c["flts"][name]
            want_n = sum(matches_range(flt, p, KINDS) for p in col.payloads)
            assert cl.count("c", count_filter=flt).count == want_n == \
                fresh.count("c", count_filter=flt).count, name
            for limit in (10, 64):
                r = cl.query_points("c", query=c["q"][j], limit=limit, query_filter=flt)
                assert hits_of(r) == hits_of(fresh.query_points("c", query=c["q"][j], limit=limit,
                                                                query_filter=flt)), name
                same(r, brute_hits(cl, c["q"][j], flt, limit))
                assert len(r.points) == min(limit, want_n)
    finally:
        fresh.close()
    n = len(col.row_ids)
    want = np.array([col.ranges.keys(p) for p in col.payloads], np.int64)
    for k in range(4):
        got = col.index.gather_keys(k, np.arange(n)).cpu().numpy()
        np.testing.assert_array_equal(got, want[:, k])


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one", "three"])
def test_keys_follow_rows_through_deletes_overwrites_and_growth(gpu, devices):
    from ragmi import qdrant_models as m
    c = corpus(384)
    rng = np.random.default_rng(11)
    ids = list(range(1200))
    cl = make_client(gpu, devices, ids[:200], capacity=64)          # grows past its capacity
    try:
        cl.upsert("c", m.Batch(ids=ids[200:], vectors=c["x"][ids[200:]],
                               payloads=[c["pay"][i] for i in ids[200:]]))
        col = cl._col("c")
        assert col.index.capacity >= 1200 and col.index.keys_cols() == 4
        check_against_survivors(gpu, cl, devices, ("since", "years"))
        cl.delete("c", rng.choice(1200, 300, replace=False).tolist())        # scattered
        check_against_survivors(gpu, cl, devices)
        tail = col.row_ids[-150:]                                            # a contiguous tail
        cl.delete("c", m.PointIdsList(points=list(tail)))
        check_against_survivors(gpu, cl, devices, ("years", "few"))
        cl.delete("c", m.FilterSelector(filter=m.Filter(
            must=[m.FieldCondition("ticker", m.MatchValue("T02"))])))       # a legacy filter
        assert all(p.get("ticker") != "T02" for p in col.payloads) and len(col.payloads) < 750
        check_against_survivors(gpu, cl, devices)
        # an overwrite that changes the value moves the point across a bound; one without the
        # field drops it from every range
        years = c["flts"]["years"]
        inside = next(i for i, p in zip(col.row_ids, col.payloads)
                      if matches_range(years, p, KINDS) and i not in set(c["dup"].tolist()))
        n_in = cl.count("c", count_filter=years).count
        n_empty = cl.count("c", count_filter=m.Filter(
            must=[m.IsEmptyCondition(m.PayloadField("fiscal_year"))])).count
        q = c["x"][inside]
        top = cl.query_points("c", query=q, limit=1, query_filter=years).points[0]
        assert top.id == inside
        cl.upsert("c", [m.PointStruct(id=inside, vector=q, payload=dict(c["pay"][inside],
                                                                        fiscal_year=2030))])
        assert cl.count("c", count_filter=years).count == n_in - 1
        assert cl.query_points("c", query=q, limit=1, query_filter=years).points[0].id != inside
        far = m.Filter(must=[m.FieldCondition("fiscal_year", range=m.Range(gt=2029))])
        assert [p.id for p in cl.query_points("c", query=q, limit=5, query_filter=far).points] == [inside]
        cl.upsert("c", [m.PointStruct(id=inside, vector=q, payload={"ticker": "T00", "n": inside})])
        assert cl.count("c", count_filter=far).count == 0
        assert cl.count("c", count_filter=m.Filter(
            must=[m.IsEmptyCondition(m.PayloadField("fiscal_year"))])).count == n_empty + 1
        for k in range(4):
            assert int(col.index.gather_keys(k, [col.id_to_row[inside]])[0]) == -(1 << 63)
        with pytest.raises(NotImplementedError, match="Collection.delete takes only"):
            cl.delete("c", m.FilterSelector(filter=years))
    finally:
        cl.close()


# ------------------------------------------------------------------ 6. create_payload_index
@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one", "three"])
def test_create_payload_index_on_a_populated_collection(gpu, devices):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import UnsupportedFilter
    c = corpus(384)
    flts = c["flts"]
    late = make_client(gpu, devices, range(N_ROWS), range_fields=None)
    born = client(gpu, devices)
    try:
        with pytest.raises(UnsupportedFilter, match="range"):
            late.query_points("c", query=c["q"][0], limit=5, query_filter=flts["since"])
        T = m.PayloadSchemaType
        for field, schema in (("fiscal_year", T.INTEGER), ("ingested_at", T.DATETIME),
                              ("revenue", T.FLOAT), ("pages", "integer")):
            assert late.create_payload_index("c", field, schema).status == m.UpdateStatus.COMPLETED
        late.create_payload_index("c", "revenue", T.FLOAT)                   # idempotent
        late.create_payload_index("c", "ticker", T.KEYWORD)
        assert late._col("c").index.keys_cols() == 4
        with pytest.raises(ValueError, match="at most 4"):
            late.create_payload_index("c", "fifth", T.FLOAT)
        for j, name in enumerate(flts):
            assert late.count("c", count_filter=flts[name]).count == \
                born.count("c", count_filter=flts[name]).count, name
            a = late.query_points("c", query=c["q"][j], limit=20, query_filter=flts[name])
            b = born.query_points("c", query=c["q"][j], limit=20, query_filter=flts[name])
            assert hits_of(a) == hits_of(b) and [p.payload for p in a.points] == [p.payload for p in b.points]
    finally:
        late.close()


# ------------------------------------------------------------------ 7. save / load
@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one", "three"])
def test_answers_survive_save_and_load(gpu, devices, tmp_path):
    from ragmi.qdrant import QdrantClient
    c = corpus(384)
    flts = c["flts"]
    cl = client(gpu, devices)
    cl.save(str(tmp_path))
    back = QdrantClient(device=gpu, devices=devices, path=str(tmp_path))
    try:
        col = back._col("c")
        assert col.ranges.as_dict() == KINDS and col.index.keys_cols() == 4
        for j, name in enumerate(flts):
            assert back.count("c", count_filter=flts[name]).count == \
                cl.count("c", count_filter=flts[name]).count, name
            a = back.query_points("c", query=c["q"][j], limit=50, query_filter=flts[name])
            b = cl.query_points("c", query=c["q"][j], limit=50, query_filter=flts[name])
            assert hits_of(a) == hits_of(b)
    finally:
        back.path = None             # close() would save again
        back.close()


# ------------------------------------------------------------------ 8. rag
def test_retrieve_from_qdrant_takes_an_ingest_window(gpu, monkeypatch):
    from ragmi import qdrant_models as m
    from ragmi import rag
    from ragmi.qdrant import QdrantClient
    c = corpus(384)
    cl = QdrantClient(device=gpu)
    rag.ensure_collection(cl)
    cl.create_payload_index(rag.COLLECTION_NAME, "ingested_at", m.PayloadSchemaType.DATETIME)
    pay = [dict(p, ticker="AAPL" if r % 2 else "MSFT") for r, p in enumerate(c["pay"][:600])]
    cl.upsert(rag.COLLECTION_NAME, m.Batch(ids=list(range(600)), vectors=c["x"][:600], payloads=pay))
    monkeypatch.setenv("TESTING", "False")
    monkeypatch.setattr(rag, "get_qdrant", lambda: cl)
    q = c["q"][9]
    since, until = "2023-09-01T00:00:00Z", dt.datetime(2024, 9, 1, tzinfo=UTC)
    flt = m.Filter(must=[m.FieldCondition("ticker", m.MatchValue("AAPL")),
                         m.FieldCondition("ingested_at", range=m.DatetimeRange(gte=since, lt=until))])
    for kw, f in (({"ingested_since": since, "ingested_until": until}, flt),
                  ({"ingested_since": since}, m.Filter(must=[flt.must[0], m.FieldCondition(
                      "ingested_at", range=m.DatetimeRange(gte=since))]))):
        got = rag.retrieve_from_qdrant(q, "aapl", limit=15, **kw)
        ok = np.array([matches_range(f, p, KINDS) for p in pay], np.uint32)
        assert 15 < ok.sum() < 300
        s, i = O.search(O.encode_rows32(c["x"][:600]), q.reshape(1, -1), 15, tags=ok, mask=1,
                        value=1, use_filter=True)
        assert [p.id for p in got.points] == i[0].tolist() and len(got.points) == 15
        assert [np.float32(p.score) for p in got.points] == s[0].tolist()
    plain = rag.retrieve_from_qdrant(q, "aapl", limit=15)               # today's call
    assert [p.id for p in plain.points] != [p.id for p in got.points] and len(plain.points) == 15
    cl.close()
