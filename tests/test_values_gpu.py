"""GPU tests of vectors at the edges of the value space (DESIGN.md "Values at the edges"), on
every search route: a vector whose canonical sumsq is not finite (some component is inf or NaN),
or is zero, is stored and searched as the zero vector; finite extremes (fp32 subnormals, 1e-30
and 3e36 scales, +-FLT_MAX components, -0.0, one-hot rows, elements around fp16's subnormal
boundary) keep the canonical arithmetic; the imports refuse what a ragmi index cannot have stored.

One world per (D, storage): Gaussian rows (3017 = 189 tiles, an odd count with a partial last
tile; 9000 where the large-k pass is wanted) with one special row (_values_ref) in every eighth
tile, one whole tile of non-finite rows, one whole tile of zero rows and a NaN row last. The
queries: 8 Gaussian, 8 near planted rows, a zero query, one each with +inf, -inf and NaN, one each
scaled 1e-42 and 3e36, a one-hot one; for searches 17 more (a second pass), the last with a NaN.
Every comparison is on bits against oracle_scan and the restatements; nothing carries a tolerance.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _prescan6_ref as R6
import _reco_ref as RR
import _values_ref as V
import oracle_scan as O
import test_prescan6_gpu as P6
import test_prescan_routes_gpu as PR
from test_prescan_routes_gpu import bits, lists, same, unpacked

pytestmark = pytest.mark.gpu

N, N_LARGE = 3017, 9000
OFFSET = PR.OFFSET
ALL = 0xFFFFFFFF
BAD_TILE, ZERO_TILE = 50, 101
KINDS = V.NONFINITE + V.FINITE
ZERO_LIKE = [16, 17, 18, 19]          # of the 23 queries: zero, +inf, -inf, NaN
WORLDS = [(384, "fp16"), (384, "fp32"), (1024, "fp16"), (1024, "fp32")]
world_params = pytest.mark.parametrize("D,storage", WORLDS)


@functools.lru_cache(maxsize=None)
def world(D, n=N):
    rng = np.random.default_rng(1000 * D + n)
    x = rng.standard_normal((n, D)).astype(np.float32)
    kind = {}                                    # row -> kind of the special rows
    for j, t in enumerate(range(0, -(-n // 16), 8)):
        kind[min(16 * t + (5 * j) % 16, n - 1)] = KINDS[j % len(KINDS)]
    for r in range(16):
        kind[16 * BAD_TILE + r] = V.NONFINITE[r % len(V.NONFINITE)]
    kind[n - 1] = "nan"                          # the last row, in the partial tile
    for r, name in kind.items():
        x[r] = V.special(name, D, rng)
    x[16 * ZERO_TILE:16 * ZERO_TILE + 16] = 0
    bad = np.array(sorted(r for r, name in kind.items() if name in V.NONFINITE))
    assert len(bad) >= 16 + 5 and set(kind.values()) == set(KINDS)
    np.testing.assert_array_equal(np.nonzero(~np.isfinite(x).all(axis=1))[0], bad)
    tags = rng.integers(1, 4, n).astype(np.uint32)

    noise = lambda m: (0.05 / np.sqrt(D)) * rng.standard_normal((m, D))      # noqa: E731
    q = rng.standard_normal((23, D)).astype(np.float32)
    near = [min(r for r, name in kind.items() if name == want)
            for want in ("sub", "huge", "fltmax", "fltmax_one", "negzero", "onehot_p", "straddle")]
    near.append(3)
    q[8:16] = (V.plain_normalize(x[near]) + noise(8)).astype(np.float32)
    q[16] = 0
    q[17, 5], q[18, 7], q[19, D - 1] = np.inf, -np.inf, np.nan
    q[20] = (q[20].astype(np.float64) * 1e-42).astype(np.float32)
    q[21] *= np.float32(3e36)
    q[22] = 0
    q[22, 11] = 1.0
    q40 = np.concatenate([q, rng.standard_normal((17, D)).astype(np.float32)])
    q40[39, 0] = np.nan
    enc16, enc32 = O.encode_rows(x), O.encode_rows32(x)
    return dict(x=x, kind=kind, bad=bad, near=np.array(near), tags=tags, q=q, q40=q40,
                zero_like40=ZERO_LIKE + [39], enc16=enc16, enc32=enc32)


def stored(c, storage):
    return c["enc32"] if storage == "fp32" else c["enc16"]


@functools.lru_cache(maxsize=None)
def oracle(D, storage, n, B, k, filt=None):
    """The oracle's lists of the world's first B queries (40: q40), cached: (score bits, ids).
    filt: None, "legacy" or "view" (filters below)."""
    c = world(D, n)
    q = c["q40"][:B] if B > 23 else c["q"][:B]
    if filt is None:
        return PR.oracle(stored(c, storage), q, k)
    f, column = filters(D, n, B)[filt][:2]
    return PR.oracle(stored(c, storage), q, k, column, f)


@functools.lru_cache(maxsize=None)
def filters(D, n, B):
    """legacy: per-query (mask, value) over the tags 1..3, with (0, 0) and a value no row has;
    view: programs tag == 1, tag == 2, tag == 9 over the view's bits."""
    from ragmi.filters import FilterProgram, eval_view_np, pack_view
    tags = world(D, n)["tags"]
    legacy = np.array([[0xFFFF, 1 + j % 3] for j in range(B)], np.uint32)
    legacy[0], legacy[1] = (0, 0), (ALL, 9)
    blob = pack_view([FilterProgram.maskeq(ALL, v) for v in (1, 2, 9)])
    vf = np.array([[1 << ((j + 1) % 3)] * 2 for j in range(B)], np.uint32)
    return {"legacy": (legacy, tags, None), "view": (vf, eval_view_np(blob, tags), blob)}


_indexes = {}


def index_of(gpu, D, storage, n=N):
    """One FlatIndex per (D, storage, n) for the module, filled by the device-pointer upsert."""
    from ragmi.index import FlatIndex
    key = (D, storage, n)
    if key not in _indexes:
        c = world(D, n)
        idx = FlatIndex(D, n, gpu, storage=storage)
        idx.upsert(c["x"], np.arange(n, dtype=np.int64), c["tags"], new_count=n)
        _indexes[key] = idx
    return _indexes[key]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for idx in _indexes.values():
        idx.close()
    _indexes.clear()


def in_modes(idx, D, storage, run, n_searches, B):
    """run() once; on an index that keeps the scan copies (D = 384, fp16) under prescan modes 0,
    2 and 3 with equal results (test_prescan6_gpu.three_modes), left in auto mode."""
    if (D, storage) != (384, "fp16"):
        return run()
    try:
        return P6.three_modes(idx, run, n_searches, B)
    finally:
        idx.set_prescan(1)


def assert_stored(idx, x, storage):
    """The stored rows are the oracle's encoding of x; no stored element is NaN or inf."""
    got16 = idx.export_rows()
    np.testing.assert_array_equal(got16, O.encode_rows(x))
    assert ((got16 & 0x7c00) != 0x7c00).all()
    if storage == "fp32":
        got32 = idx.export_rows32()
        np.testing.assert_array_equal(got32.view(np.uint32), O.encode_rows32(x).view(np.uint32))
        assert ((got32.view(np.uint32) & 0x7f800000) != 0x7f800000).all()
    return got16


# ------------------------------------------------------------------------------ 1. stored rows
@world_params
def test_stored_rows(gpu, D, storage):
    """upsert from a device pointer and rag_index_upsert_host store the oracle's rows; the
    non-finite rows and the zero tile are all-zero bits in both stored forms."""
    from ragmi import _lib
    from ragmi.index import FlatIndex
    c = world(D)
    x, n = c["x"], N
    np.testing.assert_array_equal(c["enc16"], V.plain_store(x, "fp16"))      # the oracle's own pin
    np.testing.assert_array_equal(c["enc32"].view(np.uint32),
                                  V.plain_store(x, "fp32").view(np.uint32))
    dev = index_of(gpu, D, storage)
    host = FlatIndex(D, n, gpu, storage=storage)
    try:
        rows = np.arange(n, dtype=np.int64)
        _lib.check(host._L.rag_index_upsert_host(
            host._h, x.ctypes.data_as(_lib.c_f32p), rows.ctypes.data_as(_lib.c_i64p),
            c["tags"].ctypes.data_as(_lib.c_u32p), n, n))
        for idx in (dev, host):
            assert idx.count == n
            got16 = assert_stored(idx, x, storage)
            zero = np.concatenate([c["bad"], np.arange(16 * ZERO_TILE, 16 * ZERO_TILE + 16)])
            assert not got16[zero].any()
            if storage == "fp32":
                assert not idx.export_rows32().view(np.uint32)[zero].any()
            np.testing.assert_array_equal(idx.export_tags(), c["tags"])
    finally:
        host.close()


# ---------------------------------------------------------------------------------- 2. k <= 32
@pytest.mark.parametrize("k", [1, 15, 32])
@world_params
def test_search(gpu, D, storage, k):
    c = world(D)
    idx = index_of(gpu, D, storage)
    q, B = c["q40"], 40
    un = idx.unanswered()
    got = in_modes(idx, D, storage, lambda: lists(idx.search(q, k)), 1, B)
    same(got, oracle(D, storage, N, B, k))
    assert idx.unanswered() == un
    assert not np.isnan(got[0].view(np.float32)).any()
    zl = c["zero_like40"]
    np.testing.assert_array_equal(got[1][zl], np.broadcast_to(np.arange(k), (len(zl), k)))
    np.testing.assert_array_equal(got[0][zl], np.zeros((len(zl), k), np.int32))
    # the queries planted near special rows find them first
    np.testing.assert_array_equal(got[1][8:16, 0], c["near"])


# --------------------------------------------------------------------------- 3. prescan bounds
@pytest.mark.parametrize("mode", [2, 3])
def test_prescan_bounds(gpu, mode):
    """u of every row against the 23 queries: finite, >= the exact score, and the restatement's
    bit for bit; on the zero and the non-finite rows (s = 0, E = 0) it is the query's C."""
    D, storage = 384, "fp16"
    c = world(D)
    idx = index_of(gpu, D, storage)
    rows = np.arange(N, dtype=np.int64)
    try:
        idx.set_prescan(mode)
        u = idx.prescan_bounds(c["q"], rows).cpu().numpy()
    finally:
        idx.set_prescan(1)
    check_bounds(u, c["enc16"], c["q"], mode)
    planes = R6.query_planes(O.normalize(c["q"]))
    zero = np.concatenate([c["bad"], np.arange(16 * ZERO_TILE, 16 * ZERO_TILE + 16)])
    np.testing.assert_array_equal(bits(u[:, zero]),
                                  bits(np.broadcast_to(planes[4][:, None], (23, len(zero)))))


def check_bounds(u, enc, q, mode):
    n = enc.shape[0]
    rows = np.broadcast_to(np.arange(n, dtype=np.int64), (len(q), n)).copy()
    e = O.rescore(enc, O.normalize(q), rows)
    assert np.isfinite(u).all() and np.isfinite(e).all() and (u >= e).all()
    rows32 = enc.view(np.float16).astype(np.float32)
    planes = R6.query_planes(O.normalize(q))
    want = R6.upper_bounds(*R6.quantise_rows6(rows32), *planes) if mode == 3 else \
        P6._upper_bounds8(rows32, *planes)
    np.testing.assert_array_equal(bits(u), bits(want))


# ----------------------------------------------------------------------------- 4. other routes
@world_params
def test_legacy_filter_view_and_packed(gpu, D, storage):
    idx = index_of(gpu, D, storage)
    q, B, k = world(D)["q40"], 40, 15
    f = filters(D, N, B)
    (legacy, _, _), (vf, _, blob) = f["legacy"], f["view"]
    un = idx.unanswered()

    def run():
        return (lists(idx.search(q, k, filters=legacy)),
                lists(idx.search(q, k, filters=vf, programs=blob)),
                unpacked(idx.search_packed(q, k, filters=legacy, id_offset=OFFSET)))
    l, v, p = in_modes(idx, D, storage, run, 3, B)
    want = oracle(D, storage, N, B, k, "legacy")
    same(l, want)
    same(v, oracle(D, storage, N, B, k, "view"))
    same(p, (want[0], np.where(want[1] >= 0, want[1] + OFFSET, -1)))
    assert idx.unanswered() == un
    assert (l[1][1] == -1).all() and (v[1][1] == -1).all()          # a tag no row carries
    for got in (l, v, p):
        assert not np.isnan(got[0].view(np.float32)).any()


@world_params
def test_large_k_and_full_pass(gpu, D, storage):
    """k = 100 over 9000 rows: the large-k pass equals the oracle; a zero-like query, every row
    tied at +0.0, is either answered with the oracle's list or left unanswered (all -1,
    unanswered() advanced by one), which of the two is asserted; the full pass answers all."""
    c = world(D, N_LARGE)
    idx = index_of(gpu, D, storage, N_LARGE)
    q, k = c["q"], 100
    want = oracle(D, storage, N_LARGE, 23, k)
    un = idx.unanswered()
    got = lists(idx.search(q, k))
    left = [j for j in ZERO_LIKE if (got[1][j] == -1).all()]
    print(f"zero-like queries left unanswered by the large-k pass: {left}")
    assert idx.unanswered() == un + len(left)
    answered = [j for j in range(23) if j not in left]
    same((got[0][answered], got[1][answered]), (want[0][answered], want[1][answered]))
    np.testing.assert_array_equal(want[1][ZERO_LIKE], np.broadcast_to(np.arange(k), (4, k)))
    un = idx.unanswered()
    same(lists(idx.search(q, k, full=True)), want)
    assert idx.unanswered() == un
    rescued = idx.rescued
    same(lists(idx.search(q, k, rescue=True)), want)                 # the front end's route
    assert idx.rescued == rescued + len(left)


@world_params
def test_two_shard_set(gpu, D, storage):
    from ragmi.shardset import ShardSet
    c = world(D)
    q, B, k = c["q40"], 40, 15
    legacy = filters(D, N, B)["legacy"][0]
    sset = ShardSet(D, [gpu.index] * 2, N, storage)
    try:
        sset.upsert(c["x"], np.arange(N), c["tags"], new_count=N)
        np.testing.assert_array_equal(sset.export_rows(), c["enc16"])
        same(lists(sset.search(q, k)), oracle(D, storage, N, B, k))
        same(lists(sset.search(q, k, filters=legacy)), oracle(D, storage, N, B, k, "legacy"))
        assert all(s.unanswered() == 0 for s in sset.shards)
    finally:
        sset.close()


def reco_sides(c):
    """positives: a Gaussian vector, a NaN vector, a query near a planted row; negatives: a
    +inf vector, a stored row's input vector."""
    q, x = c["q"], c["x"]
    return (q[0], q[19], q[9]), (q[17], x[40])


@pytest.mark.parametrize("strategy", [RR.BEST, RR.SUM])
@world_params
def test_recommend_with_nonfinite_examples(gpu, D, storage, strategy):
    c = world(D)
    idx = index_of(gpu, D, storage)
    pos, neg = reco_sides(c)
    s = RR.scores(stored(c, storage), pos, neg, strategy)
    assert np.isfinite(s).all()
    if strategy == RR.BEST:        # a zero-vector example is not an absent one: it scores 0
        assert not np.array_equal(s, RR.scores(stored(c, storage), (pos[0], pos[2]), neg[1:],
                                               strategy))
    un = idx.unanswered()
    for k in (15, 100):
        want = RR.top_k(s, k)
        for full in (False, True):
            gs, gi = idx.recommend(np.stack(pos), np.stack(neg), strategy, k, full=full)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(gi.cpu().numpy(), want[1])
            np.testing.assert_array_equal(bits(gs.cpu().numpy()), bits(want[0]))
    assert idx.unanswered() == un


@world_params
def test_average_vector_with_nonfinite_examples(gpu, D, storage):
    """A non-finite example adds the zero vector to its side's mean; positives that are all
    non-finite give the zero target: rows 0 .. k-1 at +0.0."""
    c = world(D)
    idx = index_of(gpu, D, storage)
    enc = stored(c, storage)
    pos, neg = reco_sides(c)
    k = 15
    for p, n in ((pos, neg), (pos[:2], ()), ((c["q"][19], c["q"][18]), ())):
        v = RR.average_vector(enc, p, n)
        assert np.isfinite(v).all()
        got_v = idx.reco_vector(np.stack(p), np.stack(n) if n else None)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(got_v.cpu().numpy()), bits(v))
        gs, gi = idx.recommend(np.stack(p), np.stack(n) if n else None, None, k)
        ws, wi = O.search(enc, v[None], k)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(gi.cpu().numpy(), wi[0])
        np.testing.assert_array_equal(bits(gs.cpu().numpy()), bits(ws[0]))
    assert not v.any() and np.array_equal(wi[0], np.arange(k)) and not bits(ws).any()


# ------------------------------------------------------------- 5. upsert over an existing row
@world_params
def test_upsert_over_an_existing_row(gpu, D, storage):
    """A good row overwritten by a non-finite vector, then non-finite rows by good vectors:
    after each step the exports and a k = 15 search are the oracle's; at D = 384 fp16 under
    mode 3 the int8 and the 6-bit copies follow (the bounds of the rows written and of their
    tiles' other rows are the restatements')."""
    from ragmi.index import FlatIndex
    c = world(D)
    x, q, k = c["x"].copy(), c["q"], 15
    copies = (D, storage) == (384, "fp16")
    good = np.array([100, 101, 16 * 60 + 15], np.int64)                 # Gaussian rows
    was_bad = np.array([c["bad"][0], 16 * BAD_TILE + 3, N - 1], np.int64)
    rng = np.random.default_rng(9)
    idx = FlatIndex(D, N, gpu, storage=storage)
    try:
        idx.upsert(x, np.arange(N, dtype=np.int64), c["tags"], new_count=N)
        if copies:
            idx.set_prescan(3)

        def check(written):
            enc16 = assert_stored(idx, x, storage)
            enc = idx.export_rows32() if storage == "fp32" else enc16
            got = in_modes(idx, D, storage, lambda: lists(idx.search(q, k)), 1, len(q))
            same(got, PR.oracle(enc, q, k))
            if copies:
                near = np.unique(np.concatenate([16 * (written // 16) + j for j in range(16)]))
                near = near[near < N]
                for mode in (2, 3):
                    idx.set_prescan(mode)
                    u = idx.prescan_bounds(q, near).cpu().numpy()
                    check_bounds(u, enc16[near], q, mode)
                idx.set_prescan(3)
            return got

        check(good)
        x[good] = V.specials(("nan", "pinf", "inf_nan"), D, 7)
        idx.upsert(x[good], good, np.full(3, 2, np.uint32))
        assert not idx.export_rows()[good].any()
        check(good)
        fresh = rng.standard_normal((6, D)).astype(np.float32)
        fresh[:3] = q[:3] + np.float32(0.01) * fresh[:3]                   # found by queries 0..2
        rows = np.concatenate([was_bad, good])
        x[rows] = fresh
        idx.upsert(fresh, rows, np.full(6, 3, np.uint32))
        got = check(rows)
        np.testing.assert_array_equal(got[1][:3, 0], was_bad)
        assert idx.unanswered() == 0
    finally:
        idx.close()


# ------------------------------------------------------------------------- 6. imports refuse
RAG_EINVAL = -1


def _bad_imports(D, storage):
    """name -> three rows to import whose middle one the index cannot have stored"""
    f16 = storage == "fp16"
    base = np.zeros((3, D), np.float32)
    base[0, 1] = base[2, 2] = 1.0
    out = {}

    def case(name, row=None, bits16=None, at=3):
        a = base.copy()
        if row is not None:
            a[1] = row
        a = a.astype(np.float16).view(np.uint16) if f16 else a
        if bits16 is not None:
            a[1, at] = bits16
        out[name] = a
    if f16:
        for name, b in (("+inf", 0x7c00), ("-inf", 0xfc00), ("nan", 0x7e00)):
            case(name, base[0], b)
    else:
        for name, v in (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan)):
            row = base[0].copy()
            row[3] = v
            case(name, row)
    row = np.zeros(D, np.float32)
    row[4] = 1.5
    case("norm 1.5", row)
    target = 1.001 * (1 + 2.0 ** -10)
    row = np.zeros(D, np.float32)
    row[0], row[D - 1] = 1.0, np.sqrt(target * target - 1.0)
    case("norm 1.001 (1 + 2^-10)", row)
    stored_row = out["norm 1.001 (1 + 2^-10)"][1]
    v = (stored_row.view(np.float16) if f16 else stored_row).astype(np.float64)
    nrm = np.sqrt((v * v).sum())
    assert nrm > 1.001 and abs(nrm - target) < 4e-6        # fp16 rounding of the small element
    return out


@world_params
def test_imports_refuse_what_no_index_stored(gpu, D, storage):
    from ragmi import _lib
    from ragmi.index import FlatIndex
    c = world(D)
    q, k = c["q"], 15
    src = index_of(gpu, D, storage)
    f16 = storage == "fp16"
    rows = src.export_rows() if f16 else src.export_rows32()
    idx = FlatIndex(D, N, gpu, storage=storage)
    imp = idx.import_rows if f16 else idx.import_rows32
    fn = idx._L.rag_index_import_rows if f16 else idx._L.rag_index_import_rows32
    ptr = _lib.c_u16p if f16 else _lib.c_f32p
    try:
        imp(rows, 0, c["tags"], new_count=N)           # everything export returns imports fine
        assert idx.count == N
        assert_stored(idx, c["x"], storage)
        before = lists(idx.search(q, k))
        same(before, oracle(D, storage, N, 23, k))
        for name, a in _bad_imports(D, storage).items():
            a = np.ascontiguousarray(a)
            torch.cuda.synchronize()
            rc = fn(idx._h, 10, 3, a.ctypes.data_as(ptr), None, N)
            msg = idx._L.rag_last_error().decode()
            print(f"{name}: {rc} {msg}")
            assert rc == RAG_EINVAL, name
            assert "row 11 " in msg, (name, msg)       # the first offending row: 10 + 1
            assert ("non-finite" in msg) == (name in ("+inf", "-inf", "nan")), msg
            with pytest.raises(_lib.RagmiError, match="row 11 "):
                imp(a, 10)
            assert idx.count == N
        assert_stored(idx, c["x"], storage)            # nothing was written
        np.testing.assert_array_equal(idx.export_tags(), c["tags"])
        same(lists(idx.search(q, k)), before)
        # norm exactly 1, the zero row, and the largest fp16 step below kRowNorm import fine
        fine = np.zeros((3, D), np.float32)
        fine[0, 7] = -1.0
        fine[2, 0] = 1.0 + 2.0 ** -10
        fine = fine.astype(np.float16).view(np.uint16) if f16 else fine
        imp(fine, 10)
        got = (idx.export_rows if f16 else idx.export_rows32)(10, 3)
        np.testing.assert_array_equal(got.view(np.uint16 if f16 else np.uint32),
                                      fine.view(np.uint16 if f16 else np.uint32))
    finally:
        idx.close()
