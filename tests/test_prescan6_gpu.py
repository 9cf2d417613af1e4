"""GPU tests of the 6-bit prescan (rag_index_set_prescan mode 3): a k <= 32 pass
streams the 6-bit copy of the rows, ranks them by an upper bound u of their exact score, and
select certifies the exact top-k from the fp16 rows.

Every result is compared bit for bit with oracle_scan and with mode 0 on the same index
(`three_modes`); prescan6_passes() stays unmoved under modes 0 and 2 and advances by
ceil(B / 32) per search under mode 3. Nothing here carries a tolerance. The harness, the
3017-row corpus (189 tiles: the last pair has a spare tile, the last tile is partial), its tags,
views and queries are test_prescan_routes_gpu's.
"""
import numpy as np
import pytest
import torch

import _prescan6_ref as R
import oracle_scan as O
import test_prescan_routes_gpu as PR
import test_select_band_gpu as SB
from test_prescan_routes_gpu import bits, lists, oracle, passes, same, unpacked

pytestmark = pytest.mark.gpu
D = 384
OFFSET = PR.OFFSET


def three_modes(idx, run, n_searches, B):
    """run() under modes 0, 2 and 3: equal results; the 6-bit counter moves under mode 3 only,
    by n_searches * ceil(B / 32). Returns the mode-3 result; the index is left in mode 3."""
    p6 = idx.prescan6_passes()
    idx.set_prescan(0)
    r0 = run()
    idx.set_prescan(2)
    r2 = run()
    assert idx.prescan6_passes() == p6
    idx.set_prescan(3)
    p = idx.prescan_passes()
    r3 = run()
    assert idx.prescan6_passes() - p6 == n_searches * passes(B)
    assert idx.prescan_passes() - p == n_searches * passes(B)
    same(r0, r3)
    same(r2, r3)
    return r3


@pytest.fixture(scope="module")
def idx0(gpu):
    c = PR.world()
    idx = PR.make_index(gpu, c["x"], c["tags"])
    idx.set_prescan(3)          # below the threshold: builds the copy from the stored rows
    yield idx
    idx.close()


# ---------------------------------------------------------------------------------- 1. premise
def test_upper_bound_holds_and_equals_the_restatement(gpu):
    """test_prescan_gpu's 4101-row adversarial set x 32 queries under mode 3: min(u - e) > 0,
    and u is the numpy restatement's bit for bit"""
    from ragmi.index import FlatIndex
    rng = np.random.default_rng(1)
    n = 4101
    x = rng.standard_normal((n, D)).astype(np.float32)
    r = 3000
    for j in range(16):
        x[r] = 0
        x[r, (37 * j) % D] = 1.0 if j % 2 else -1.0
        r += 1
    for j in range(64):
        v = 0.02 * rng.standard_normal(D)
        v[rng.integers(D)] = 0.9
        x[r] = v
        r += 1
    for j in range(8):
        x[r] = (1.0 if j % 2 else -1.0) * (j + 1)
        r += 1
    x[r] = 0
    r += 1
    x[r:r + 100] *= 1e-4
    r += 100
    x[r:r + 100] *= 1e4
    r += 100
    x[r:r + 40] = x[5]
    q = np.zeros((32, D), np.float32)
    q[:8] = rng.standard_normal((8, D))
    q[8:16] = x[rng.choice(3000, 8, replace=False)] + \
        0.05 * rng.standard_normal((8, D)).astype(np.float32)
    q[16, 11] = 1.0
    q[18] = -x[123]
    q[19:] = rng.standard_normal((13, D))
    idx = FlatIndex(dim=D, capacity=n, device=gpu)
    idx.upsert(x, np.arange(n, dtype=np.int64), None, new_count=n)
    rows = np.arange(n, dtype=np.int64)
    u8 = idx.prescan_bounds(q, rows).cpu().numpy()          # auto mode, small: the int8 bound
    idx.set_prescan(3)
    u = idx.prescan_bounds(q, rows).cpu().numpy()
    enc = idx.export_rows()
    e = O.rescore(enc, O.normalize(q), np.broadcast_to(rows, (32, n)).copy())
    gap = u.astype(np.float64) - e.astype(np.float64)
    print(f"min(u - e) = {gap.min():.3e}; mean(u - e) random x random = "
          f"{gap[:8, :3000].mean():.5f} (int8 copy: {(u8 - e)[:8, :3000].mean():.5f})")
    assert np.isfinite(u).all() and gap.min() > 0
    assert (u8 != u).any()                                  # the other copy's bound
    c = enc.view(np.float16).astype(np.float32)
    want = R.upper_bounds(*R.quantise_rows6(c), *R.query_planes(O.normalize(q)))
    np.testing.assert_array_equal(bits(u), bits(want))
    out = idx.prescan_bounds(q[:3], np.array([-1, n, 10**9], np.int64)).cpu().numpy()
    assert np.isneginf(out).all()
    idx.close()


# ------------------------------------------------------------------------------ 2. tiny indexes
@pytest.mark.parametrize("k", PR.KS)
@pytest.mark.parametrize("B", [1, 32, 33, 70])
def test_plain_search(gpu, idx0, B, k):
    c = PR.world()
    q = c["q"][:B]
    got = three_modes(idx0, lambda: lists(idx0.search(q, k)), 1, B)
    same(got, oracle(c["enc"], q, k))


# a load batch of the scan is one pair of tiles: 32 rows
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65])
def test_tiny_indexes(gpu, n):
    rng = np.random.default_rng(100 + n)
    x = rng.standard_normal((n, D)).astype(np.float32)
    q = rng.standard_normal((33, D)).astype(np.float32)
    if n:
        q[:4] = x[rng.choice(n, 4)] + 0.05 * rng.standard_normal((4, D)).astype(np.float32)
    idx = PR.make_index(gpu, x)
    enc = O.encode_rows(x) if n else np.zeros((0, D), np.uint16)
    for k in (1, 15, 32):                               # k > n: padded with -1
        got = three_modes(idx, lambda: lists(idx.search(q, k)), 1, 33)
        if n:
            same(got, oracle(enc, q, k))
        assert ((got[1] >= 0).sum(axis=1) == min(k, n)).all()
    idx.close()


# ------------------------------------------------------------------------------ 3. other routes
@pytest.mark.parametrize("k", PR.KS)
def test_legacy_filter_view_and_packed(gpu, idx0, k):
    c = PR.world()
    B = 40
    q = c["q"][:B]
    legacy = PR.tag_filters(B, c["pt"])
    slot, vf = PR.view_filt(B, c["U"])

    def run():
        return (lists(idx0.search(q, k, filters=legacy)),
                lists(idx0.search(q, k, filters=vf, programs=c["blob"])),
                unpacked(idx0.search_packed(q, k, filters=legacy, id_offset=OFFSET)))
    l, v, p = three_modes(idx0, run, 3, B)
    same(l, oracle(c["enc"], q, k, c["tags"], legacy))
    same(v, oracle(c["enc"], q, k, c["view"], vf))        # should / must_not / MatchAny programs
    same(p, oracle(c["enc"], q, k, c["tags"], legacy, OFFSET))
    assert (v[1][slot == 8] == -1).all() and idx0.unanswered() == 0


def test_range_atom(gpu):
    c = PR.range_world(1)
    idx = PR.make_index(gpu, c["x"], c["tags"], c["keys"])
    q, filt, k = c["q"], c["filt"], 15
    got = three_modes(idx, lambda: lists(idx.search(q, k, filters=filt, programs=c["blob"])),
                      1, len(q))
    same(got, oracle(O.encode_rows(c["x"]), q, k, c["view"], filt))
    idx.close()


def test_scan_order_2_and_a_partitioned_stream(gpu, idx0):
    from ragmi.index import PartitionStreams
    c = PR.world()
    k = 15
    jobs = [c["q"][:32], c["q"][32:64], c["q"][16:48], c["q"][38:70]]
    want = [oracle(c["enc"], q, k) for q in jobs]
    cur = torch.cuda.current_stream(gpu)
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]

    def on(ss):
        outs = []
        for j, q in enumerate(jobs):
            ss[j % len(ss)].wait_stream(cur)
            with torch.cuda.stream(ss[j % len(ss)]):
                outs.append(idx0.search(q, k))
        return [lists(o) for o in outs]
    try:
        idx0.set_scan_order(2)
        same(three_modes(idx0, lambda: on(streams), len(jobs), 32), want)
    finally:
        idx0.set_scan_order(0)
    parts = PartitionStreams(gpu, 4)
    try:
        same(three_modes(idx0, lambda: on(parts.streams), len(jobs), 32), want)
    finally:
        parts.close()


# ------------------------------------------------------------------------------------ 4. tiers
def _tiers(gpu, x, q, k=15):
    idx = PR.make_index(gpu, x)
    got = three_modes(idx, lambda: lists(idx.search(q, k)), 1, len(q))
    _, t2, tiers = idx.exactness_stats(len(q))
    same(got, oracle(O.encode_rows(x), q, k))
    u = idx.prescan_bounds(q, np.arange(len(x), dtype=np.int64)).cpu().numpy()
    idx.close()
    return got, tiers, t2, u


def test_tier1_over_several_chunks(gpu):
    """300 near-duplicates at random rows of 24 000, drawn from the tiles the seed sample does
    not read (test_select_band_gpu's rule for its tier-1 geometries: with 32 sampled tiles
    holding a duplicate the seed itself stands inside the cluster, above L, and the verdict is
    tier 2 whatever the scan — observed here with unrestricted positions: tiers 2 for all eight
    near queries). Every near query's band holds all 300: three gather chunks of 128 lists."""
    rng = np.random.default_rng(300)
    x, q, rows = SB._cluster(rng, 24_000, D, 300, 8, 4, rows=SB._unsampled_rows(rng, 24_000, 300))
    got, tiers, _, u = _tiers(gpu, x, q)
    e15 = got[0][:, 14].view(np.float32)
    band = (u >= e15[:, None]).sum(axis=1)
    print(f"band rows per query: {band}; tiers {tiers}")
    assert (band[:8] >= 200).all() and (tiers[:8] == 1).all(), (band, tiers)


def test_contiguous_duplicates_fullness_verdict(gpu):
    """64 contiguous near-duplicates sit in two waves' lists: a full list inside the band"""
    x, q, _ = SB._cluster(np.random.default_rng(64), 24_000, D, 64, 8, 4,
                          rows=np.arange(8000, 8064))
    _, tiers, _, _ = _tiers(gpu, x, q)
    assert (tiers[:8] == 2).all(), tiers


def test_saturated_corpus_takes_tier_2(gpu):
    rng = np.random.default_rng(43)
    n = SB.SAT_N
    base = rng.standard_normal((1, D)).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    x[::2] = base + 1e-5 * rng.standard_normal((n // 2, D)).astype(np.float32)
    q = np.concatenate([base + 0.02 * rng.standard_normal((3, D)).astype(np.float32),
                        rng.standard_normal((2, D)).astype(np.float32)])
    _, tiers, t2, _ = _tiers(gpu, x, q)
    assert (tiers[:3] == 2).all() and t2 >= 3, tiers


def test_identical_rows_come_out_lowest_row_first(gpu):
    rng = np.random.default_rng(40)
    x = rng.standard_normal((5000, D)).astype(np.float32)
    rows = np.sort(rng.choice(5000, 40, replace=False))
    x[rows] = x[rows[0]]
    q = x[rows[:1]] + 0.01 * rng.standard_normal((4, D)).astype(np.float32)
    got, _, _, _ = _tiers(gpu, x, q, k=32)
    for ids in got[1]:
        assert len(set(ids.tolist())) == 32                       # no id twice
        np.testing.assert_array_equal(ids, rows[:32])             # equal scores: row ascending


# ------------------------------------------------------------------- 5. the copy follows the rows
def test_copy_follows_the_rows(gpu):
    from ragmi.index import FlatIndex, PRESCAN6_MIN_ROWS
    rng = np.random.default_rng(4)
    n, k = 3000, 15
    x = rng.standard_normal((n, D)).astype(np.float32)
    fresh = rng.standard_normal((64, D)).astype(np.float32)
    q = np.concatenate([x[:8] + 0.05 * rng.standard_normal((8, D)).astype(np.float32),
                        fresh[:8] + 0.05 * rng.standard_normal((8, D)).astype(np.float32),
                        rng.standard_normal((16, D)).astype(np.float32)])
    idx = FlatIndex(dim=D, capacity=n, device=gpu)
    idx.upsert(x, np.arange(n, dtype=np.int64), None, new_count=n)
    assert n < PRESCAN6_MIN_ROWS
    lists(idx.search(q, k))                   # auto mode below the threshold: never the 6-bit scan
    idx.set_prescan(2)
    lists(idx.search(q, k))
    assert idx.prescan6_passes() == 0

    def check():
        got = three_modes(idx, lambda: lists(idx.search(q, k)), 1, 32)
        enc = idx.export_rows()
        same(got, oracle(enc, q, k))
        rows = np.arange(idx.count, dtype=np.int64)
        u = idx.prescan_bounds(q, rows).cpu().numpy()
        c = enc.view(np.float16).astype(np.float32)
        want = R.upper_bounds(*R.quantise_rows6(c), *R.query_planes(O.normalize(q)))
        np.testing.assert_array_equal(bits(u), bits(want))
    check()                                   # mode 3 set below the threshold built the copy
    idx.upsert(fresh[:32], np.arange(0, 64, 2, dtype=np.int64), np.full(32, 9, np.uint32))
    check()
    idx.remove_rows(np.array([0, 1, 17, 500, 2000, idx.count - 1], np.int64))
    check()
    idx.reserve(3 * n)
    check()
    c0 = idx.count
    idx.upsert(fresh[32:], np.arange(c0, c0 + 32, dtype=np.int64), np.full(32, 3, np.uint32))
    check()
    idx.close()


def _upper_bounds8(c, hi, lo, sq, A, C):
    """The int8 copy's u [b, n] restated as _prescan6_ref restates the 6-bit one (prep_kernels.hip
    quantise_row over Copy8, u_bound): bytes v = rint(c / s) in [-127, 127] with s = max|c| / 127,
    E = ||c - s v||_2 rounded up; I = 254 (v . hi) + v . lo rounded to fp32 once (u_bound's fma of
    two exact conversions), then the same two fp32 fmas."""
    c = np.asarray(c, R.f32)
    s = (np.abs(c).max(axis=1) / R.f32(127)).astype(R.f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(s[:, None] > 0, np.rint((c / s[:, None]).astype(R.f32)), R.f32(0))
    v = np.clip(v, -127, 127)
    d = c.astype(np.float64) - s.astype(np.float64)[:, None] * v.astype(np.float64)
    e2 = (d * d).sum(axis=1)
    E = np.where(e2 > 0, np.sqrt(e2) * R.UP, 0.0).astype(R.f32)
    v = v.astype(np.int64)
    I8 = 254 * (hi @ v.T) + lo @ v.T                         # exact integers [b, n]
    assert np.abs(I8).max(initial=0) < 2 ** 31
    If = I8.astype(R.f32)
    scale = (s[None, :] * sq[:, None]).astype(R.f32)
    tail = R._fma32(np.broadcast_to(E[None, :], If.shape), np.broadcast_to(A[:, None], If.shape),
                    np.broadcast_to(C[:, None], If.shape))
    return R._fma32(If, scale, tail)


def test_copy_at_the_threshold_capacity(gpu):
    """The 6-bit copy's threshold paths: started inside reserve() when the capacity reaches
    PRESCAN6_MIN_ROWS (index A), kept from creation at that capacity and grown by a later
    reserve() (index B). 3017 rows, 189 tiles: the last pair of the copy has a spare half. After
    every step the mode-3 bounds of all rows are the restatement's bit for bit and a k = 15
    search is the oracle's under modes 0, 2 and 3; at the end the grown int8 copy's bounds are
    its restatement's too."""
    from ragmi.index import FlatIndex, PRESCAN6_MIN_ROWS
    c = PR.world()
    x, q, k = c["x"], c["q"][:32], 15
    n = len(x)
    assert n == 3017 and n < PRESCAN6_MIN_ROWS
    planes = R.query_planes(O.normalize(q))

    def check(idx):
        got = three_modes(idx, lambda: lists(idx.search(q, k)), 1, 32)
        enc = idx.export_rows()
        same(got, oracle(enc, q, k))
        u = idx.prescan_bounds(q, np.arange(idx.count, dtype=np.int64)).cpu().numpy()
        rows = enc.view(np.float16).astype(np.float32)
        want = R.upper_bounds(*R.quantise_rows6(rows), *planes)
        np.testing.assert_array_equal(bits(u), bits(want))
        return rows, enc

    a = FlatIndex(dim=D, capacity=n, device=gpu)
    a.upsert(x, np.arange(n, dtype=np.int64), None, new_count=n)
    a.reserve(PRESCAN6_MIN_ROWS)              # the copy starts here, from the rows just moved
    a.set_prescan(3)
    check(a)
    a.close()

    b = FlatIndex(dim=D, capacity=PRESCAN6_MIN_ROWS, device=gpu)   # the copy exists from creation
    b.upsert(x, np.arange(n, dtype=np.int64), None, new_count=n)
    b.set_prescan(3)
    check(b)
    b.reserve(PRESCAN6_MIN_ROWS + 48)         # grows an existing copy from an odd tile count
    fresh = np.random.default_rng(5).standard_normal((32, D)).astype(np.float32)
    b.upsert(fresh, np.arange(n, n + 32, dtype=np.int64), np.full(32, 3, np.uint32))
    assert b.count == n + 32
    rows, enc = check(b)
    b.set_prescan(2)                          # the grown int8 copy
    u8 = b.prescan_bounds(q, np.arange(b.count, dtype=np.int64)).cpu().numpy()
    np.testing.assert_array_equal(bits(u8), bits(_upper_bounds8(rows, *planes)))
    e = O.rescore(enc, O.normalize(q), np.broadcast_to(np.arange(b.count), (32, b.count)).copy())
    assert np.isfinite(u8).all() and (u8 >= e).all()
    b.close()
