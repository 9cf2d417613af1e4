"""GPU tests of rag_index_facet_counts and QdrantClient.facet against
np.bincount over the exported tags, exactly. The kernel keeps its bins in LDS up to 8192 of them
(n_codes <= 8191) and in global memory above: codebooks of 3, 8191, 8192 and 20000 values put one
size on each side of that switch and one well inside each path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY = -0x5A5A5A5A5A5A5A5B
N_ROWS = 20011                       # no multiple of 16, five facet steps of 4096 rows less 469
_cases = {}


def K(x):
    from ragmi.filters import key_of_float
    return key_of_float(float(x))


def build(gpu, n_codes, index=None, count=N_ROWS):
    """`count` rows whose field-0 codes cover 0 (absent) .. n_codes and whose field-1 codes cover
    0 .. 3, one key column of small integers."""
    from ragmi.index import FlatIndex
    rng = np.random.default_rng(n_codes)
    c0 = rng.integers(0, n_codes + 1, count).astype(np.uint32)
    c0[:min(count, n_codes + 1)] = np.arange(min(count, n_codes + 1))      # every code occurs
    c0[-1] = n_codes                                                      # the last row's too
    tags = c0 | (rng.integers(0, 4, count).astype(np.uint32) << np.uint32(16))
    idx = FlatIndex(384, count + 21, gpu, "fp16") if index is None else index
    v = torch.zeros((count, 384), dtype=torch.float32, device=gpu)
    v[:, 0] = 1.0
    idx.reserve(count + 21)
    idx.upsert(v, np.arange(count), tags, new_count=count)
    idx.keys_create(1)
    idx.write_keys(0, np.arange(count), np.array([K(x) for x in rng.integers(0, 10, count)]))
    return idx


def case(gpu, n_codes):
    if n_codes not in _cases:
        _cases[n_codes] = build(gpu, n_codes)
    return _cases[n_codes]


def exported(idx):
    n = idx.count
    keys = idx.gather_keys(0, torch.arange(n, device=idx.device)).cpu().numpy()[None, :]
    return idx.export_tags(0, n), keys


def ref_counts(tags, field, n_codes, passing=None):
    code = ((tags >> np.uint32(16 * field)) & np.uint32(0xFFFF)).astype(np.int64)
    ok = code <= n_codes
    if passing is not None:
        ok &= passing
    return np.bincount(code[ok], minlength=n_codes + 1).astype(np.int64)


def raw_facet(idx, field, n_codes, blob=None):
    """The ABI call into a buffer with one guard element after the n_codes + 1 counts."""
    dev = idx.device
    out = torch.full((max(n_codes, 0) + 2,), CANARY, dtype=torch.int64, device=dev)
    p = None if blob is None else torch.from_numpy(
        np.ascontiguousarray(blob, np.uint32).view(np.int32)).to(dev)
    rc = idx._L.rag_index_facet_counts(
        idx._h, None if p is None else p.data_ptr(), 0 if p is None else p.numel(), field,
        n_codes, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def check(idx, field, n_codes, program=None, data=None):
    from ragmi.filters import eval_view_np, pack_view
    tags, keys = data if data is not None else exported(idx)
    blob = None if program is None else pack_view([program])
    passing = None if blob is None else (eval_view_np(blob, tags, 1, keys=keys) & 1).astype(bool)
    want = ref_counts(tags, field, n_codes, passing)
    rc, got = raw_facet(idx, field, n_codes, blob)
    assert rc == 0
    np.testing.assert_array_equal(got[:n_codes + 1], want)
    assert got[n_codes + 1] == CANARY                        # the word after the output
    np.testing.assert_array_equal(idx.facet_counts(field, n_codes, blob).cpu().numpy(), want)
    return want


@pytest.mark.parametrize("n_codes", (3, 8191, 8192, 20000))
def test_codebook_sizes_and_fields(gpu, n_codes):
    idx = case(gpu, n_codes)
    data = exported(idx)
    want = check(idx, 0, n_codes, data=data)
    assert want.sum() == N_ROWS and (want > 0).all()
    want = check(idx, 1, 3, data=data)
    assert want.sum() == N_ROWS
    # rows lacking the field sit in bin 0, which the client drops; the bins of the other field
    # are not mixed in
    assert want[0] == int(((data[0] >> np.uint32(16)) == 0).sum())


@pytest.mark.parametrize("n_codes", (3, 8191, 8192, 20000))
def test_stale_codes_are_ignored(gpu, n_codes):
    """n_codes smaller than the largest stored code: the surplus codes are not counted and index
    nothing, on both paths (8191 -> 100 stays in LDS, 20000 -> 8192 stays global)."""
    idx = case(gpu, n_codes)
    data = exported(idx)
    for smaller in sorted({0, 1, n_codes // 2, n_codes - 1}):
        want = check(idx, 0, smaller, data=data)
        assert want.sum() < N_ROWS
    check(idx, 1, 2, data=data)
    check(idx, 1, 0, data=data)


@pytest.mark.parametrize("n_codes", (3, 20000))
def test_filters_and_deletes(gpu, n_codes):
    from ragmi.filters import FilterProgram
    idx = build(gpu, n_codes)
    data = exported(idx)
    programs = (FilterProgram.maskeq(0xFFFF0000, 2 << 16),                 # a legacy pair
                FilterProgram((("range", 0, K(3), K(6)),), 0b10),
                FilterProgram((("maskeq", 0xFFFF0000, 1 << 16), ("range", 0, K(0), K(4))), 0b0111),
                FilterProgram.maskeq(0, 0))
    for program in programs:
        check(idx, 0, n_codes, program, data)
        check(idx, 1, 3, program, data)
    idx.remove_rows(np.arange(1, N_ROWS, 3))               # tail rows move into the holes
    torch.cuda.synchronize()
    after = exported(idx)
    assert after[0].shape[0] == idx.count < N_ROWS
    for program in (None,) + programs[:2]:
        check(idx, 0, n_codes, program, after)
    idx.close()


def test_empty_index_and_refusals(gpu):
    from ragmi.filters import FilterProgram, pack_view
    from ragmi.index import FlatIndex
    idx = FlatIndex(384, 64, gpu, "fp16")
    assert idx.count == 0
    for n_codes in (0, 5, 9000):
        rc, got = raw_facet(idx, 0, n_codes)
        assert rc == 0 and (got[:n_codes + 1] == 0).all() and got[n_codes + 1] == CANARY
    rc, got = raw_facet(idx, 1, 5, pack_view([FilterProgram.maskeq(0, 0)]))
    assert rc == 0 and (got[:6] == 0).all()
    EINVAL, ERANGE = -1, -4
    for field, n_codes, code in ((2, 5, ERANGE), (-1, 5, ERANGE), (0, -1, ERANGE),
                                 (0, 65536, ERANGE)):
        rc, got = raw_facet(idx, field, n_codes)
        assert rc == code and (got == CANARY).all()
    st = torch.cuda.current_stream(gpu).cuda_stream
    assert idx._L.rag_index_facet_counts(idx._h, None, 0, 0, 5, None, st) == EINVAL
    rc, got = raw_facet(idx, 0, 5, pack_view([FilterProgram.maskeq(0, 0)])[:40])
    assert rc == EINVAL and (got == CANARY).all()
    idx.close()


@pytest.mark.parametrize("n_codes", (3, 20000))
def test_shard_set_equals_single_index(gpu, n_codes):
    from ragmi.filters import FilterProgram, pack_view
    from ragmi.shardset import ShardSet
    one = case(gpu, n_codes)
    sset = build(gpu, n_codes, index=ShardSet(384, devices=[0, 0, 0], capacity=N_ROWS + 21))
    blob = pack_view([FilterProgram((("range", 0, K(2), K(7)),), 0b10)])
    for field, nc in ((0, n_codes), (1, 3), (0, n_codes // 2)):
        for programs in (None, blob):
            np.testing.assert_array_equal(sset.facet_counts(field, nc, programs).cpu().numpy(),
                                          one.facet_counts(field, nc, programs).cpu().numpy())
    sset.close()


def test_client_facet(gpu):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    client = QdrantClient(device=gpu)
    client.create_collection("docs", m.VectorParams(size=384, distance=m.Distance.COSINE),
                             payload_range_fields={"year": "number"})
    n = 1003
    rng = np.random.default_rng(5)
    tick = rng.choice(["AAPL", "MSFT", "NVDA", "AMD", "TSM"], n, p=[0.4, 0.2, 0.2, 0.1, 0.1])
    tick[:6] = ["ZZ", "ZZ", "YY", "YY", "XX", "XX"]              # ties: value ascending
    types = rng.choice(["10-K", "10-Q", "8-K"], n)
    vec = rng.standard_normal((n, 384)).astype(np.float32)
    pay = [{"ticker": str(t), "document_type": str(d), "year": 2000 + i % 7}
           for i, (t, d) in enumerate(zip(tick, types))]
    client.upsert("docs", m.Batch(ids=list(range(n)), vectors=vec, payloads=pay))

    def want(keep, key="ticker"):
        c = {}
        for p in pay:
            if keep(p):
                c[p[key]] = c.get(p[key], 0) + 1
        return sorted(c.items(), key=lambda h: (-h[1], h[0]))

    def got(**kw):
        return [(h.value, h.count) for h in client.facet("docs", **kw).hits]

    assert got(key="ticker", limit=100) == want(lambda p: True)
    assert got(key="ticker") == want(lambda p: True)[:10]
    assert got(key="ticker", limit=3) == want(lambda p: True)[:3]
    assert got(key="ticker", limit=100)[-3:] == [("XX", 2), ("YY", 2), ("ZZ", 2)]
    k10 = m.Filter(must=[m.FieldCondition(key="document_type", match=m.MatchValue(value="10-K"))])
    assert got(key="ticker", facet_filter=k10, limit=100) == want(lambda p: p["document_type"] == "10-K")
    rng_f = m.Filter(must=[m.FieldCondition(key="year", range=m.Range(gte=2003))],
                     must_not=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AAPL"))])
    keep = lambda p: p["year"] >= 2003 and p["ticker"] != "AAPL"
    assert got(key="document_type", facet_filter=rng_f) == want(keep, "document_type")
    # every point has the field: the counts add up to count(filter)
    assert sum(c for _, c in got(key="ticker", facet_filter=rng_f, limit=100)) == \
        client.count("docs", count_filter=rng_f).count == sum(map(keep, pay))
    # after a delete; a value no point holds any more is dropped
    client.delete("docs", m.PointIdsList(points=[4, 5] + list(range(100, 400))))
    pay[:] = [p for i, p in enumerate(pay) if i not in (4, 5) and not 100 <= i < 400]
    assert got(key="ticker", limit=100) == want(lambda p: True)
    assert "XX" not in dict(got(key="ticker", limit=100))
    client.close()
