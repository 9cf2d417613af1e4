"""GPU tests of rag_index_order_rows at dim 384: the radix select, the ordered
emit and the LDS sort against np.lexsort over the exported keys, exactly — keys, rows, both
counts, the padding of the list and the words after it — and every case twice with equal bits.
Row counts 1, 17, 4096 and 12293: the last is three select chunks plus 5, so the tail chunk, the
16-row padding of the columns and rows past the count are all in play. Nothing here carries a
tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = (1, 17, 4096, 12293)
LIMITS = (1, 15, 4096)
CANARY = -0x5A5A5A5A5A5A5A5B
GUARD = 8
_cases = {}


def K(x):
    from ragmi.filters import key_of_float
    return key_of_float(float(x))


def draw_keys(dist, count, rng):
    """One key column of `count` keys, KEY_ABSENT nowhere unless the distribution says so."""
    from ragmi.filters import KEY_ABSENT
    if dist == "ties":                    # 7 distinct values: ties across every cut
        vals = np.array([K(v) for v in (-3.5, -1.0, 0.0, 2.0, 2.5, 1e9, 1e300)], np.int64)
        return vals[rng.integers(0, 7, count)]
    if dist == "one_second":              # microsecond timestamps inside one second
        base = 1_718_000_000_000_000
        return np.array([K(base + int(u)) for u in rng.integers(0, 1_000_000, count)], np.int64)
    if dist == "low_byte":                # raw keys sharing their upper 56 bits
        return (K(1.718e15) & ~0xFF) + rng.integers(0, 256, count).astype(np.int64)
    if dist == "sign":                    # +-x: doubles that differ only in the sign bit
        xs = np.array([1.0, 2.0 ** -1022, 1e300])[rng.integers(0, 3, count)]
        return np.array([K(s * x) for s, x in zip(rng.choice([-1.0, 1.0], count), xs)], np.int64)
    if dist == "edges":
        vals = [-np.inf, np.inf, -0.0, 0.0, 1e-308, -1e-308, 2 ** 53 + 1, -(2 ** 53 + 1),
                2 ** 63, 5e-324]
        assert K(-0.0) == K(0.0)
        return np.array([K(vals[i]) for i in rng.integers(0, len(vals), count)], np.int64)
    if dist == "all_absent":
        return np.full(count, KEY_ABSENT, np.int64)
    if dist == "half_absent":
        k = draw_keys("ties", count, rng)
        k[rng.random(count) < 0.5] = KEY_ABSENT
        return k
    raise KeyError(dist)


def build(gpu, count, dist, index=None):
    """An index of `count` rows, capacity past it, random tags, column 0 drawn from `dist` and
    column 1 small integers (what the RANGE program of another column compares)."""
    from ragmi.index import FlatIndex
    rng = np.random.default_rng(count * 31 + sum(map(ord, dist)))
    tags = (rng.integers(0, 5, count).astype(np.uint32) |
            (rng.integers(0, 3, count).astype(np.uint32) << np.uint32(16)))
    keys = np.stack([draw_keys(dist, count, rng),
                     np.array([K(v) for v in rng.integers(0, 10, count)], np.int64)])
    idx = FlatIndex(384, count + 37, gpu, "fp16") if index is None else index
    v = torch.zeros((count, 384), dtype=torch.float32, device=gpu)
    v[:, 0] = 1.0
    idx.reserve(count + 37)
    idx.upsert(v, np.arange(count), tags, new_count=count)
    idx.keys_create(2)
    for c in range(2):
        idx.write_keys(c, np.arange(count), keys[c])
    return idx


def case(gpu, count, dist):
    if (count, dist) not in _cases:
        _cases[(count, dist)] = build(gpu, count, dist)
    return _cases[(count, dist)]


def exported(idx):
    """(tags uint32 [count], keys int64 [2, count]) as the index holds them now."""
    n = idx.count
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros((2, 0), np.int64)
    rows = torch.arange(n, device=idx.device)
    keys = np.stack([idx.gather_keys(c, rows).cpu().numpy() for c in range(2)])
    return idx.export_tags(0, n), keys


def ref_order(keys, limit, desc, lo, hi, passing):
    from ragmi.filters import KEY_ABSENT
    ok = (keys != KEY_ABSENT) & (keys >= lo) & (keys <= hi)
    if passing is not None:
        ok &= passing
    rows = np.nonzero(ok)[0].astype(np.int64)
    kk = keys[rows]
    order = np.lexsort((rows, ~kk if desc else kk))[:limit]     # ~k reverses int64 exactly
    return kk[order], rows[order], int(rows.size)


def raw_order(idx, col, limit, desc, lo, hi, blob):
    """rag_index_order_rows over ctypes into buffers with guard words: (rc, keys [limit +
    GUARD], rows [limit + GUARD], n [2 + GUARD]) as host arrays."""
    dev = idx.device
    room = max(limit, 0) + GUARD
    keys = torch.full((room,), CANARY, dtype=torch.int64, device=dev)
    rows = torch.full((room,), CANARY, dtype=torch.int64, device=dev)
    n = torch.full((2 + GUARD,), CANARY, dtype=torch.int64, device=dev)
    p = None if blob is None else torch.from_numpy(
        np.ascontiguousarray(blob, np.uint32).view(np.int32)).to(dev)
    rc = idx._L.rag_index_order_rows(
        idx._h, None if p is None else p.data_ptr(), 0 if p is None else p.numel(), col,
        1 if desc else 0, lo, hi, limit, keys.data_ptr(), rows.data_ptr(), n.data_ptr(),
        torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc, keys.cpu().numpy(), rows.cpu().numpy(), n.cpu().numpy()


def check(idx, limit, desc=False, lo=None, hi=None, program=None, col=0, data=None):
    """One call, twice: equal bits, and equal to the reference. Returns (rows, eligible)."""
    from ragmi.filters import KEY_ABSENT, KEY_MAX, KEY_MIN, eval_view_np, pack_view
    tags, keys = data if data is not None else exported(idx)
    lo = KEY_MIN if lo is None else lo
    hi = KEY_MAX if hi is None else hi
    blob = None if program is None else pack_view([program])
    passing = None
    if blob is not None:                                         # an emptied index: no rows
        passing = ((eval_view_np(blob, tags, 1, keys=keys) & 1).astype(bool) if tags.size
                   else np.zeros(0, bool))
    want_k, want_r, want_n = ref_order(keys[col], limit, desc, lo, hi, passing)
    a = raw_order(idx, col, limit, desc, lo, hi, blob)
    b = raw_order(idx, col, limit, desc, lo, hi, blob)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)                      # the same bits on every run
    rc, got_k, got_r, got_n = a
    assert rc == 0
    w = len(want_r)
    assert got_n[:2].tolist() == [w, want_n] and w == min(limit, want_n)
    np.testing.assert_array_equal(got_r[:w], want_r)
    np.testing.assert_array_equal(got_k[:w], want_k)
    assert (got_r[w:limit] == -1).all() and (got_k[w:limit] == KEY_ABSENT).all()   # padding
    for arr, used in ((got_k, limit), (got_r, limit), (got_n, 2)):
        assert (arr[used:] == CANARY).all()                      # nothing past the outputs
    # the Python method returns the same list, cut to what was written
    k, r, n = idx.order_rows(col, limit, desc, lo, hi, blob)
    assert n == want_n
    np.testing.assert_array_equal(r.cpu().numpy(), want_r)
    np.testing.assert_array_equal(k.cpu().numpy(), want_k)
    return want_r, want_n


@pytest.mark.parametrize("count", COUNTS)
def test_ties_across_the_cut(gpu, count):
    idx = case(gpu, count, "ties")
    data = exported(idx)
    for desc in (False, True):
        for limit in LIMITS:
            check(idx, limit, desc, data=data)
        # a limit above the number of eligible rows: one of the 7 values, about a seventh
        _, n = check(idx, 4096, desc, lo=K(2.0), hi=K(2.0), data=data)
        assert n < 4096


@pytest.mark.parametrize("dist", ("one_second", "low_byte", "sign", "edges"))
@pytest.mark.parametrize("count", COUNTS)
def test_adversarial_digits(gpu, count, dist):
    idx = case(gpu, count, dist)
    data = exported(idx)
    for desc in (False, True):
        for limit in LIMITS:
            check(idx, limit, desc, data=data)


@pytest.mark.parametrize("count", COUNTS)
def test_absent_keys(gpu, count):
    from ragmi.filters import KEY_ABSENT
    idx = case(gpu, count, "all_absent")
    for desc in (False, True):
        rows, n = check(idx, 15, desc)
        assert n == 0 and rows.size == 0
    idx = case(gpu, count, "half_absent")
    data = exported(idx)
    for desc in (False, True):
        for limit in (15, 4096):
            rows, _ = check(idx, limit, desc, data=data)
            assert (data[1][0][rows] != KEY_ABSENT).all()


@pytest.mark.parametrize("count", COUNTS)
def test_bounds_are_inclusive(gpu, count):
    idx = case(gpu, count, "ties")
    data = exported(idx)
    present = np.unique(data[1][0])
    for desc in (False, True):
        check(idx, 4096, desc, lo=K(-1.0), hi=K(2.5), data=data)       # both ends stored values
        check(idx, 15, desc, lo=K(-1.0) + 1, hi=K(2.5) - 1, data=data)  # just inside: both drop
        check(idx, 15, desc, lo=int(present[0]), hi=int(present[0]), data=data)
        rows, n = check(idx, 15, desc, lo=K(2.0), hi=K(0.0), data=data)  # lo > hi
        assert n == 0


@pytest.mark.parametrize("count", COUNTS)
def test_filter_programs(gpu, count):
    from ragmi.filters import FilterProgram
    idx = case(gpu, count, "ties")
    data = exported(idx)
    programs = (FilterProgram.maskeq(0xFFFF, 2),                          # MASKEQ
                FilterProgram((("range", 1, K(3), K(6)),), 0b10),        # RANGE on ANOTHER column
                FilterProgram((("maskeq", 0xFFFF0000, 1 << 16), ("range", 1, K(0), K(4))), 0b0110),
                FilterProgram.maskeq(0, 0))                               # the (0, 0) filter
    for program in programs:
        for desc in (False, True):
            for limit in (15, 4096):
                check(idx, limit, desc, program=program, data=data)
    check(idx, 15, program=programs[1], lo=K(-1.0), hi=K(2.0), data=data)


@pytest.mark.parametrize("count", COUNTS)
def test_after_a_delete(gpu, count):
    idx = build(gpu, count, "one_second")
    before = exported(idx)
    idx.remove_rows(np.arange(0, count, 3))                # tail rows move into the holes
    torch.cuda.synchronize()
    after = exported(idx)
    assert idx.count == count - len(range(0, count, 3)) == after[0].shape[0]
    if count > 4:
        assert not np.array_equal(after[1][0], before[1][0][:idx.count])     # rows did move
    from ragmi.filters import FilterProgram
    for desc in (False, True):
        for limit in (1, 15, 4096):
            check(idx, limit, desc, data=after)
        check(idx, 15, desc, program=FilterProgram.maskeq(0xFFFF, 1), data=after)
    idx.close()


@pytest.mark.parametrize("count", (17, 12293))
@pytest.mark.parametrize("dist", ("ties", "half_absent"))
def test_shard_set_equals_single_index(gpu, count, dist):
    from ragmi.filters import FilterProgram, pack_view
    from ragmi.shardset import ShardSet
    one = case(gpu, count, dist)
    sset = build(gpu, count, dist, index=ShardSet(384, devices=[0, 0, 0], capacity=count + 37))
    blob = pack_view([FilterProgram((("range", 1, K(2), K(7)),), 0b10)])
    for desc in (False, True):
        for limit in LIMITS:
            for programs, lo, hi in ((None, None, None), (blob, None, None),
                                     (None, K(-1.0), K(2.0))):
                k1, r1, n1 = one.order_rows(0, limit, desc, lo, hi, programs)
                k3, r3, n3 = sset.order_rows(0, limit, desc, lo, hi, programs)
                assert n1 == n3
                np.testing.assert_array_equal(r3.cpu().numpy(), r1.cpu().numpy())
                np.testing.assert_array_equal(k3.cpu().numpy(), k1.cpu().numpy())
    sset.close()


def test_abi_refusals_write_nothing(gpu):
    from ragmi.filters import KEY_MAX, KEY_MIN, FilterProgram, pack_view
    idx = case(gpu, 17, "ties")
    L, h = idx._L, idx._h
    blob = pack_view([FilterProgram.maskeq(0, 0)])
    EINVAL, ERANGE = -1, -4
    for col, limit, blob_, code, word in ((0, 0, None, ERANGE, b"limit"),
                                          (0, 4097, None, ERANGE, b"limit"),
                                          (-1, 15, None, ERANGE, b"column"),
                                          (2, 15, None, ERANGE, b"column"),      # col = columns
                                          (0, 15, blob[:40], EINVAL, b"41")):
        rc, k, r, n = raw_order(idx, col, limit, False, KEY_MIN, KEY_MAX, blob_)
        assert rc == code and word in L.rag_last_error(), (col, limit)
        assert (k == CANARY).all() and (r == CANARY).all() and (n == CANARY).all()
    st = torch.cuda.current_stream(gpu).cuda_stream
    buf = torch.full((32,), CANARY, dtype=torch.int64, device=gpu)
    for nulls in ((0,), (1,), (2,), (0, 1, 2)):
        ptrs = [None if i in nulls else buf.data_ptr() for i in range(3)]
        assert L.rag_index_order_rows(h, None, 0, 0, 0, KEY_MIN, KEY_MAX, 15, *ptrs, st) == -1
        assert b"NULL" in L.rag_last_error()
    assert L.rag_index_order_rows(None, None, 0, 0, 0, KEY_MIN, KEY_MAX, 15, buf.data_ptr(),
                                  buf.data_ptr(), buf.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == CANARY).all()


def test_blob_with_offsets_past_its_end(gpu):
    """An untrusted blob behaves as rag_index_filter_view documents: an INSET bitmap or RANGE
    bounds lying past the blob read as false, and the call answers over exactly that view."""
    from ragmi.filters import (ATOM_INSET, ATOM_RANGE, KEY_MAX, KEY_MIN, REC_WORDS, eval_view_np)
    idx = case(gpu, 4096, "ties")
    tags, keys = exported(idx)
    for kind, table in ((ATOM_INSET, 0b10), (ATOM_INSET, 0b01), (ATOM_RANGE, 0b10),
                        (ATOM_RANGE, 0b01)):
        blob = np.zeros(REC_WORDS + 2, np.uint32)
        blob[0], blob[1] = 1, table
        blob[9:13] = (kind, 0, 10_000 if kind == ATOM_INSET else REC_WORDS, 64)
        passing = (eval_view_np(blob, tags, 1, keys=keys) & 1).astype(bool)
        assert passing.all() == (table == 0b01) and passing.any() == (table == 0b01)
        want_k, want_r, want_n = ref_order(keys[0], 15, False, KEY_MIN, KEY_MAX, passing)
        rc, k, r, n = raw_order(idx, 0, 15, False, KEY_MIN, KEY_MAX, blob)
        assert rc == 0 and n[:2].tolist() == [len(want_r), want_n]
        np.testing.assert_array_equal(r[:len(want_r)], want_r)
        np.testing.assert_array_equal(k[:len(want_k)], want_k)
