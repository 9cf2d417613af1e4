"""GPU tests of the filter algebra: filter_view_kernel against its numpy
restatement bit for bit (vector tail, padding, both bitmap routes, the blob guards), the view
search against the exact oracle over the same view, a program equal to a legacy filter against
the legacy call, and the client routes (deletes, shard set, batch, MMR, coalescer, rag)
against brute force over the payloads. Nothing here carries a tolerance."""
import threading

import numpy as np
import pytest
import torch

import oracle_scan as O
from _filters_ref import matches

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
N_ROWS = 3001          # no multiple of 16: the last tile is partial
TICKERS = [f"T{i:02d}" for i in range(12)]
TYPES = ["10-K", "10-Q", "8-K"]


def P(atoms, table):
    from ragmi.filters import FilterProgram
    return FilterProgram(tuple(atoms), table)


# ------------------------------------------------------------------ 1. the kernel
_kernel = {}


def kernel_case(gpu, count, codes0=50, codes1=20):
    """An index of `count` rows (capacity well past it) whose tags hold random codes."""
    key = (count, codes0)
    if key not in _kernel:
        from ragmi.index import FlatIndex
        rng = np.random.default_rng(count)
        tags = (rng.integers(0, codes0, count).astype(np.uint32) |
                (rng.integers(0, codes1, count).astype(np.uint32) << np.uint32(16)))
        idx = FlatIndex(384, count + 37, gpu, "fp16")
        v = torch.zeros((count, 384), dtype=torch.float32, device=gpu)
        v[:, 0] = 1.0
        idx.upsert(v, np.arange(count), tags, new_count=count)
        _kernel[key] = (idx, tags)
    return _kernel[key]


def random_program(rng, n_atoms, codes0=50, codes1=20):
    atoms = []
    while len(atoms) < n_atoms:
        f = int(rng.integers(0, 2))
        hi = (codes0, codes1)[f]
        if rng.integers(0, 2):
            a = ("maskeq", 0xFFFF << (16 * f), int(rng.integers(0, hi)) << (16 * f))
        else:
            bm = int.from_bytes(rng.bytes((hi + 8) // 8), "little") & ((1 << hi) - 1)
            a = ("inset", f, bm, hi)
        if a not in atoms:
            atoms.append(a)
    table = int.from_bytes(rng.bytes(32), "little") & ((1 << (1 << n_atoms)) - 1)
    return P(atoms, table)


def view_programs_for(rng, U):
    """Constant programs (0 atoms, false and true), 1 atom and 8 atoms first, then random."""
    sizes = [8, 0, 1, 0] + [int(x) for x in rng.integers(0, 9, 32)]
    progs = [random_program(rng, n) for n in sizes[:U]]
    if U > 3:
        progs[1] = P((), 0)            # constant false
        progs[3] = P((), 1)            # constant true
    return progs


def check_view(idx, tags, blob, n_programs=None):
    from ragmi.filters import eval_view_np
    cap = idx.capacity
    assert cap % 16 == 0 and cap > idx.count
    out = torch.full((cap + 64,), CANARY, dtype=torch.int32, device=idx.device)
    got = idx.filter_view(blob, n_programs=n_programs, out=out)
    torch.cuda.synchronize()
    full = out.cpu().numpy().view(np.uint32)
    want = np.zeros(cap, np.uint32)
    want[:len(tags)] = eval_view_np(blob, tags, n_programs)
    np.testing.assert_array_equal(full[:cap], want)
    assert (full[cap:] == CANARY).all()                    # nothing past the column
    assert got.shape == (cap,)
    return want[:len(tags)]


@pytest.mark.parametrize("U", [1, 7, 32])
@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, 1025, 70_001])
def test_filter_view_equals_numpy(gpu, count, U):
    from ragmi.filters import pack_view
    idx, tags = kernel_case(gpu, count)
    progs = view_programs_for(np.random.default_rng(100 * U + count % 97), U)
    want = check_view(idx, tags, pack_view(progs))
    if count > 1000:
        assert len(np.unique(want)) > 1
        if U > 3:                      # constant false bit 1, constant true bit 3
            assert not (want & 2).any() and (want & 8).all()


def test_filter_view_large_bitmaps_and_guards(gpu):
    """Bitmaps over 40 000 codes: one (the blob fits the LDS budget) and eight (it does not:
    the global-memory route); a code past the bitmap's length; bitmap offsets that point past
    the blob are answered "not a member" without the read being issued."""
    from ragmi.filters import REC_WORDS, pack_view, view_programs
    codes = 40_000
    idx, tags = kernel_case(gpu, 70_001, codes0=50_000)     # codes up to 49 999 > the bitmaps
    assert (tags & 0xFFFF).max() >= codes
    rng = np.random.default_rng(5)
    big = [P([("inset", 0, int.from_bytes(rng.bytes(codes // 8 + 1), "little") & ((1 << codes) - 1),
               codes), ("maskeq", 0xFFFF0000, 3 << 16)], 0b0110) for _ in range(8)]
    one = pack_view(big[:1])
    eight = pack_view(big)
    assert len(one) <= 8192 < len(eight)                     # kFvLdsWords: both routes
    assert view_programs(one) == 1 and view_programs(eight) == 8
    for blob in (one, eight):
        want = check_view(idx, tags, blob)
        past = (tags & 0xFFFF) >= codes
        # past the length: not a member, so only the MASKEQ atom decides (table 0b0110: xor)
        np.testing.assert_array_equal((want & 1)[past], ((tags >> 16) == 3)[past])
        assert 0 < (want & 1).sum() < len(tags)
        U = 1 if blob is one else 8
        for off in (len(blob) - 3, len(blob), 0x7FFFFFFF, 0xFFFFFFFF):
            bad = blob.copy()
            bad[11] = off                                     # program 0, atom 0: word offset
            w = check_view(idx, tags, bad, n_programs=U)
            if off >= len(blob):
                np.testing.assert_array_equal(w & 1, ((tags >> 16) == 3).astype(np.uint32))
    bad = eight.copy()
    bad[0] = 0xFFFFFFFF                                       # atom count: clamped to 8
    bad[REC_WORDS + 9] = 77                                   # an unknown atom kind
    check_view(idx, tags, bad, n_programs=8)


# ------------------------------------------------------------------ 2. search over the view
def corpus_payloads(rng, n):
    """12 tickers x 3 types; some points lack a field (or hold a list there: absent); rows
    7, 700, 1500, 2222, 3000 lack both, and only they."""
    pay = []
    for r in range(n):
        p = {"ticker": TICKERS[rng.integers(0, 12)], "document_type": TYPES[rng.integers(0, 3)],
             "n": r}
        u = rng.random()
        if u < 0.05:
            del p["ticker"]
        elif u < 0.08:
            p["ticker"] = ["T00", "T01"]
        elif u < 0.13:
            p["document_type"] = None
        pay.append(p)
    for r in (7, 700, 1500, 2222, 3000):
        pay[r] = {"n": r}
    return pay


def named_filters():
    from ragmi import qdrant_models as m
    fc = m.FieldCondition
    tick = lambda *t: fc("ticker", m.MatchAny(any=list(t)))
    return {
        "any_of": m.Filter(must=[tick("T00", "T03", "T07", "NEVER")]),
        "must_not": m.Filter(must_not=[fc("document_type", m.MatchValue("8-K"))]),
        "any_but": m.Filter(must=[tick("T01", "T02", "T03", "T04")],
                            must_not=[fc("document_type", m.MatchValue("10-Q"))]),
        "should_must": m.Filter(must=[fc("ticker", m.MatchExcept(except_=["T05", "T06"]))],
                                should=[fc("document_type", m.MatchValue("10-K")),
                                        fc("document_type", m.MatchValue("10-Q"))]),
        "nested": m.Filter(should=[m.Filter(must=[tick("T08"), fc("document_type", m.MatchValue("8-K"))]),
                                   m.Filter(must=[tick("T09", "T10")],
                                            must_not=[m.Filter(must=[fc("document_type", m.MatchValue("10-K"))])])]),
        "min_should": m.Filter(min_should=m.MinShould(
            [tick("T00", "T01", "T02"), fc("document_type", m.MatchValue("10-K")),
             m.IsEmptyCondition(m.PayloadField("document_type")), tick("T02", "T11")], 2)),
        "is_empty": m.Filter(must=[m.IsEmptyCondition(m.PayloadField("ticker"))]),
        "few": m.Filter(must=[m.IsEmptyCondition(m.PayloadField("ticker")),
                              m.IsEmptyCondition(m.PayloadField("document_type"))]),
    }


_corpus = {}


def corpus(dim):
    """Rows, payloads, tags, queries and the programs of one dim, computed once: 3001 rows
    with a 64-row near-duplicate cluster, 40 queries (128 at D = 1024), the first eight
    aimed at the cluster."""
    if dim not in _corpus:
        from ragmi.filters import compile_program, eval_view_np, pack_view
        from ragmi.qdrant import PayloadTags
        rng = np.random.default_rng(dim)
        x = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
        base = rng.standard_normal((1, dim)).astype(np.float32)
        dup = np.sort(rng.choice(N_ROWS, 64, replace=False))
        x[dup] = base + 1e-5 * rng.standard_normal((64, dim)).astype(np.float32)
        pay = corpus_payloads(rng, N_ROWS)
        pt = PayloadTags()
        tags = np.array([pt.tag(p) for p in pay], np.uint32)
        B = 40 if dim == 384 else 128
        q = rng.standard_normal((B, dim)).astype(np.float32)
        q[:8] = base + 0.02 * rng.standard_normal((8, dim)).astype(np.float32)
        flts = named_filters()
        progs = [compile_program(pt, f) for f in flts.values()]
        progs.append(P([("maskeq", 0xFFFF, 1)], 0))            # matches no row
        blob = pack_view(progs)
        view = eval_view_np(blob, tags)
        for s, f in enumerate(flts.values()):                   # the view is the plain evaluator's
            want = np.array([matches(f, p) for p in pay])
            np.testing.assert_array_equal((view >> s) & 1, want)
        assert int(((view >> 7) & 1).sum()) == 5 and not ((view >> 8) & 1).any()
        # query j asks for program j % 10, slot 9 meaning (0, 0): every row
        slot = np.arange(B) % 10
        filt = np.array([[0, 0] if s == 9 else [1 << s, 1 << s] for s in slot], np.uint32)
        _corpus[dim] = dict(x=x, pay=pay, pt=pt, tags=tags, q=q, flts=flts, progs=progs,
                            blob=blob, view=view, slot=slot, filt=filt, dup=dup, oracle={})
    return _corpus[dim]


def oracle_lists(c, storage, k):
    """The exact lists over the numpy view, one oracle call per view bit, shared by the k = 15
    and the forced-full case."""
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
        _index[(dim, storage)] = idx
    return _index[(dim, storage)]


@pytest.mark.parametrize("how", ["k15", "k100", "full"])
@pytest.mark.parametrize("storage", ["fp16", "fp32"])
@pytest.mark.parametrize("dim", [384, 1024])
def test_view_search_equals_oracle(gpu, dim, storage, how):
    """Two passes at D = 384 (B = 40), the 128-query wide pass at D = 1024; the scan, the
    large-k pass and the forced full pass; every filter shape, a filter matching fewer than k
    rows and one matching none; cluster queries inside the MFMA error band."""
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
    assert np.isin(i[0], c["dup"]).any()                            # the cluster is in play
    assert idx.unanswered() == 0


@pytest.mark.parametrize("k", [15, 100])
def test_program_equal_to_a_legacy_filter_gives_the_legacy_tensors(gpu, k):
    from ragmi.filters import FilterProgram, pack_view
    c = corpus(384)
    idx = view_index(gpu, 384, "fp16")
    pt = c["pt"]
    pairs = []
    for j in range(len(c["q"])):
        t = pt.codes[0][TICKERS[(j // 4) % 12]]
        d = pt.codes[1][TYPES[(j // 4) % 3]] << 16
        pairs.append([(0xFFFF, t), (0xFFFF0000, d), (0xFFFFFFFF, t | d), (0, 0)][j % 4])
    legacy = np.array(pairs, np.uint32)
    distinct = sorted(set(p for p in pairs if p != (0, 0)))
    assert 16 < len(distinct) <= 32
    blob = pack_view([FilterProgram.maskeq(m, v) for m, v in distinct])
    over_view = np.array([[0, 0] if p == (0, 0) else [1 << distinct.index(p)] * 2 for p in pairs],
                         np.uint32)
    s1, i1 = idx.search(c["q"], k, filters=legacy)
    s2, i2 = idx.search(c["q"], k, filters=over_view, programs=blob)
    p1 = idx.search_packed(c["q"], k, filters=legacy)
    p2 = idx.search_packed(c["q"], k, filters=over_view, programs=blob)
    torch.cuda.synchronize()
    assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert torch.equal(p1, p2)
    assert int((i1 >= 0).sum()) > 0
    rows, total = idx.select_rows_view(blob)                        # the blob's first program
    want = np.nonzero((c["tags"] & np.uint32(distinct[0][0])) == np.uint32(distinct[0][1]))[0]
    assert total == len(want) and rows.cpu().numpy().tolist() == want.tolist()
    assert idx.select_rows_view(blob, cap=3)[0].cpu().numpy().tolist() == want[:3].tolist()
    assert idx.select_rows_view(blob, cap=0)[1] == total


# ------------------------------------------------------------------ 3. the client
_clients = {}


def client(gpu, devices=None, own=None):
    """A 384-d collection of the corpus (fp32 storage, the client's default), on one index or
    on three logical shards of GPU 0; `own`: a client of the caller's own, to change."""
    key = (own, None if devices is None else tuple(devices))
    if key not in _clients:
        from ragmi import qdrant_models as m
        from ragmi.qdrant import QdrantClient
        c = corpus(384)
        cl = QdrantClient(device=gpu, devices=devices)
        cl.create_collection("c", m.VectorParams(size=384, distance=m.Distance.COSINE),
                             capacity=N_ROWS)
        cl.upsert("c", m.Batch(ids=list(range(N_ROWS)), vectors=c["x"], payloads=c["pay"]))
        _clients[key] = cl
    return _clients[key]


def brute_hits(cl, q, flt, k):
    """Exact top-k over the points the plain evaluator lets through, from the collection's
    current rows: [(id, score)]."""
    col = cl._col("c")
    x = corpus(384)["x"][np.asarray(col.row_ids)]
    ok = np.array([flt is None or matches(flt, p) for p in col.payloads], np.uint32)
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
    """query_points at the three k ranges, query_batch_points mixing legacy, general and MMR
    requests, count: one index and three shards, hit for hit, payloads included."""
    from ragmi import qdrant_models as m
    c = corpus(384)
    flts = c["flts"]
    legacy = m.Filter(must=[m.FieldCondition("ticker", m.MatchValue("T04"))])
    one, three = client(gpu), client(gpu, [0, 0, 0])
    pay = c["pay"]
    for name, flt in flts.items():
        want_n = sum(matches(flt, p) for p in pay)
        assert one.count("c", count_filter=flt).count == want_n, name
        assert three.count("c", count_filter=flt).count == want_n, name
    for cl in (one, three):
        for j, (name, limit) in enumerate([("any_but", 10), ("nested", 100), ("min_should", 5000),
                                           ("few", 10), ("is_empty", 33)]):
            r = cl.query_points("c", query=c["q"][j], limit=limit, query_filter=flts[name])
            want = brute_hits(cl, c["q"][j], flts[name], min(limit, N_ROWS))
            same(r, want)
            assert all(p.payload == pay[p.id] for p in r.points) and r.points
        assert cl.query_points("c", query=c["q"][0], limit=5, query_filter=m.Filter(
            must=[m.FieldCondition("ticker", m.MatchAny(any=["NEVER"]))])).points == []
    mmr0 = m.NearestQuery(nearest=c["q"][3].tolist(), mmr=m.Mmr(diversity=0.0, candidates_limit=12))
    mmr5 = m.NearestQuery(nearest=c["q"][1].tolist(), mmr=m.Mmr(diversity=0.5, candidates_limit=40))
    reqs = [m.QueryRequest(query=c["q"][0].tolist(), filter=legacy, limit=10),
            m.QueryRequest(query=c["q"][1].tolist(), filter=flts["any_but"], limit=10),
            m.QueryRequest(query=c["q"][2].tolist(), filter=None, limit=7),
            m.QueryRequest(query=mmr0, filter=flts["should_must"], limit=12),
            m.QueryRequest(query=mmr5, filter=flts["any_but"], limit=10),
            m.QueryRequest(query=c["q"][4].tolist(), filter=flts["any_but"], limit=3),
            m.QueryRequest(query=c["q"][5].tolist(), filter=flts["few"], limit=10)]
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
    assert len(picked) == 10 and all(matches(flts["any_but"], pay[i]) for i, _ in picked)
    assert picked != hits_of(one.query_points("c", query=c["q"][1].tolist(), limit=10,
                                              query_filter=flts["any_but"]))   # MMR re-selected


def test_concurrent_query_points_ride_the_coalescer(gpu):
    """8 threads, mixed legacy / general / no filters through the coalescer: every answer is
    its solo answer."""
    from ragmi import qdrant_models as m
    c = corpus(384)
    cl = client(gpu)
    legacy = m.Filter(must=[m.FieldCondition("ticker", m.MatchValue("T04"))])
    menu = [legacy, None] + list(c["flts"].values())
    jobs = [(c["q"][j % len(c["q"])], menu[j % len(menu)], 5 + j % 11) for j in range(48)]
    solo = [hits_of(cl.query_points("c", query=q, limit=k, query_filter=f)) for q, f, k in jobs]
    col = cl._col("c")
    before = (col.coalescer.requests, col.coalescer.batches)
    got = [None] * len(jobs)
    errs = []
    gate = threading.Barrier(8)

    def work(t):
        try:
            gate.wait()
            for j in range(t, len(jobs), 8):
                q, f, k = jobs[j]
                got[j] = hits_of(cl.query_points("c", query=q, limit=k, query_filter=f))
        except BaseException as e:             # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert got == solo
    assert col.coalescer.requests - before[0] == len(jobs)
    assert col.coalescer.batches - before[1] <= len(jobs)


def test_retrieve_from_qdrant_takes_ticker_lists(gpu, monkeypatch):
    from ragmi import qdrant_models as m
    from ragmi import rag
    from ragmi.qdrant import QdrantClient
    c = corpus(384)
    cl = QdrantClient(device=gpu)
    cl.create_collection(rag.COLLECTION_NAME, m.VectorParams(size=384, distance=m.Distance.COSINE))
    pay = [dict(p, ticker=p["ticker"].replace("T0", "AAPL").replace("T1", "MSFT"))
           if isinstance(p.get("ticker"), str) else p for p in c["pay"][:600]]
    cl.upsert(rag.COLLECTION_NAME, m.Batch(ids=list(range(600)), vectors=c["x"][:600], payloads=pay))
    monkeypatch.setenv("TESTING", "False")
    monkeypatch.setattr(rag, "get_qdrant", lambda: cl)
    q = c["q"][9]
    got = rag.retrieve_from_qdrant(q, ["aapl0", "msft1"], document_type=("10-k", "8-k"), limit=15)
    flt = m.Filter(must=[m.FieldCondition("ticker", m.MatchAny(any=["AAPL0", "MSFT1"])),
                         m.FieldCondition("document_type", m.MatchAny(any=["10-K", "8-K"]))])
    col = cl._col(rag.COLLECTION_NAME)
    ok = np.array([matches(flt, p) for p in col.payloads], np.uint32)
    s, i = O.search(O.encode_rows32(c["x"][:600]), q.reshape(1, -1), 15, tags=ok, mask=1, value=1,
                    use_filter=True)
    assert [p.id for p in got.points] == i[0].tolist() and len(got.points) == 15
    assert [np.float32(p.score) for p in got.points] == s[0].tolist()
    assert {p.payload["ticker"] for p in got.points} <= {"AAPL0", "MSFT1"}
    one = rag.retrieve_from_qdrant(q, "aapl0", limit=15)            # a string: as before
    assert one.points and {p.payload["ticker"] for p in one.points} == {"AAPL0"}
    batch = rag.retrieve_batch([q, q], [["aapl0", "msft1"], "aapl0"], [("10-k", "8-k"), None])
    assert [p.id for p in batch[0].points] == [p.id for p in got.points]
    assert [p.id for p in batch[1].points] == [p.id for p in one.points]
    cl.close()


def test_general_filters_after_deletes(gpu):
    """Delete by ids and by a legacy filter (rows move), then general-filter searches and
    counts: brute force over the surviving payloads."""
    from ragmi import qdrant_models as m
    c = corpus(384)
    flts = c["flts"]
    rng = np.random.default_rng(11)
    gone = rng.choice(N_ROWS, 400, replace=False).tolist()
    t02 = m.Filter(must=[m.FieldCondition("ticker", m.MatchValue("T02")),
                         m.FieldCondition("document_type", m.MatchValue("10-K"))])
    alive = [p for p in c["pay"] if p["n"] not in set(gone) and not matches(t02, p)]
    for cl in (client(gpu, None, "deletes"), client(gpu, [0, 0, 0], "deletes")):
        cl.delete("c", gone)
        cl.delete("c", m.FilterSelector(filter=t02))
        col = cl._col("c")
        assert len(col.payloads) == len(alive) < N_ROWS - 400
        for j, name in enumerate(flts):
            want_n = sum(matches(flts[name], p) for p in alive)
            assert cl.count("c", count_filter=flts[name]).count == want_n, name
            for limit in (10, 64):
                r = cl.query_points("c", query=c["q"][j], limit=limit, query_filter=flts[name])
                same(r, brute_hits(cl, c["q"][j], flts[name], limit))
                assert all(p.payload == c["pay"][p.id] for p in r.points)
                assert len(r.points) == min(limit, want_n)
