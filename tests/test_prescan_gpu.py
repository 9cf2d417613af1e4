"""GPU tests of the int8 prescan (rag_index_set_prescan; DESIGN.md "int8 prescan"): a k <= 32
pass streams the int8 copy of the rows, ranks them by an upper bound u of their exact score,
and select certifies the exact top-k from the fp16 rows. Checked here: the premise itself
(u >= e for every row x query pair, through rag_index_prescan_bounds), bit-exact results
against the C oracle, the fallback tiers under the wider band, that the copy follows every
write of the rows, the auto routing by shard size, and streams. Mode 2 (always) unless stated.
"""
import numpy as np
import pytest
import torch

import oracle_scan as O

pytestmark = pytest.mark.gpu
D = 384


def _index(gpu, x, tags=None, mode=2, capacity=None):
    from ragmi.index import FlatIndex
    idx = FlatIndex(dim=x.shape[1], capacity=capacity or x.shape[0], device=gpu)
    idx.upsert(x, np.arange(x.shape[0], dtype=np.int64), tags, new_count=x.shape[0])
    idx.set_prescan(mode)
    return idx


def _search(idx, q, k, filters=None):
    s, i = idx.search(q, k, filters=filters)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _oracle(enc, q, k, tags=None, filt=None):
    if filt is None:
        return O.search(enc, q, k)
    s = np.empty((len(q), k), np.float32)
    i = np.empty((len(q), k), np.int64)
    for j in range(len(q)):
        sj, ij = O.search(enc, q[j:j + 1], k, tags=tags, mask=int(filt[j, 0]),
                          value=int(filt[j, 1]), use_filter=True)
        s[j], i[j] = sj[0], ij[0]
    return s, i


def _same_in_both_modes(idx, q, k, filters=None, tags=None):
    """mode-2 search == mode-0 search bit for bit == the oracle on the exported rows"""
    idx.set_prescan(2)
    s2, i2 = _search(idx, q, k, filters)
    idx.set_prescan(0)
    s0, i0 = _search(idx, q, k, filters)
    idx.set_prescan(2)
    np.testing.assert_array_equal(i2, i0)
    np.testing.assert_array_equal(s2, s0)
    so, io = _oracle(idx.export_rows(), q, k, tags, filters)
    np.testing.assert_array_equal(i2, io)
    np.testing.assert_array_equal(s2, so)


# ---------------------------------------------------------------------------------- 1. premise
def test_upper_bound_holds_for_every_pair(gpu):
    rng = np.random.default_rng(1)
    n = 4101                                   # 257 tiles, the last one partial
    x = rng.standard_normal((n, D)).astype(np.float32)
    n_rand = 3000                              # rows [0, 3000) stay random
    r = n_rand
    for j in range(16):                        # one-hot rows
        x[r] = 0
        x[r, (37 * j) % D] = 1.0 if j % 2 else -1.0
        r += 1
    for j in range(64):                        # one component 0.9 plus noise
        v = 0.02 * rng.standard_normal(D)
        v[rng.integers(D)] = 0.9
        x[r] = v
        r += 1
    for j in range(8):                         # equal components
        x[r] = (1.0 if j % 2 else -1.0) * (j + 1)
        r += 1
    x[r] = 0                                   # a zero row
    zero_row = r
    r += 1
    x[r:r + 100] *= 1e-4                       # scaled before normalisation
    r += 100
    x[r:r + 100] *= 1e4
    r += 100
    x[r:r + 40] = x[5]                         # exact duplicates
    r += 40
    assert r <= n
    q = np.zeros((32, D), np.float32)
    q[:8] = rng.standard_normal((8, D))
    src = rng.choice(n_rand, 8, replace=False)
    q[8:16] = x[src] + 0.05 * rng.standard_normal((8, D)).astype(np.float32)
    q[16, 11] = 1.0                            # one-hot
    # q[17] stays zero
    q[18] = -x[123]                            # the negative of a row
    q[19:] = rng.standard_normal((13, D))      # padding up to B = 32
    idx = _index(gpu, x)
    rows = np.arange(n, dtype=np.int64)
    u = idx.prescan_bounds(q, rows).cpu().numpy()
    enc = idx.export_rows()
    e = O.rescore(enc, O.normalize(q), np.broadcast_to(rows, (32, n)).copy())
    gap = u.astype(np.float64) - e.astype(np.float64)
    worst = np.unravel_index(np.argmin(gap), gap.shape)
    mean_gap = float(gap[:8, :n_rand].mean())
    print(f"min(u - e) = {gap.min():.3e} at (query, row) {worst}; "
          f"mean(u - e) random x random = {mean_gap:.5f}; zero row u max = {u[:, zero_row].max():.3e}")
    assert np.isfinite(u).all()
    assert (u >= e).all(), (gap.min(), worst)
    # the half-step worst case s_r sqrt(D) / 2 averages 0.0125 on such rows; a bound built on
    # it (or inflated otherwise) would pass u >= e and make the band useless
    assert mean_gap < 0.0125, mean_gap
    # rows outside the index: never dereferenced, -inf
    out = idx.prescan_bounds(q[:3], np.array([-1, n, 10**9], np.int64)).cpu().numpy()
    assert np.isneginf(out).all()
    idx.close()


# ---------------------------------------------------------------------------- 2. exact results
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(2)
    n = 3000
    x = rng.standard_normal((n, D)).astype(np.float32)
    tags = rng.integers(1, 9, n).astype(np.uint32)
    tags[:5] = 77                                        # a tag only 5 rows carry
    q = np.concatenate([x[rng.choice(n, 16, replace=False)] +
                        0.05 * rng.standard_normal((16, D)).astype(np.float32),
                        rng.standard_normal((16, D)).astype(np.float32)])
    return x, tags, q, O.encode_rows(x)


@pytest.mark.parametrize("k", [1, 15, 32])
@pytest.mark.parametrize("n,b", [(3000, 32), (2999, 32), (3000, 1)])
def test_results_are_bit_exact(gpu, small, n, b, k):
    x, tags, q, enc = small
    idx = _index(gpu, x[:n], tags[:n])
    s, i = _search(idx, q[:b], k)
    so, io = O.search(enc[:n], q[:b], k)
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(s, so)
    # per-query tag filters: common tags, one that fewer than k rows carry, one that none does
    filt = np.array([[0xffffffff, 1 + (j % 8)] for j in range(b)], np.uint32)
    filt[0] = (0xffffffff, 77)
    if b > 1:
        filt[1] = (0xffffffff, 999)
        filt[2] = (0, 0)
    s, i = _search(idx, q[:b], k, filters=filt)
    so, io = _oracle(enc[:n], q[:b], k, tags[:n], filt)
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(s, so)
    if b > 1:
        assert (i[1] == -1).all()
    idx.close()


# ------------------------------------------------------------ 3. fallback tiers, wide band
@pytest.mark.parametrize("contiguous", [False, True])
def test_near_duplicate_cluster(gpu, contiguous):
    """test_exactness_gpu's cluster corpus: 160 near-duplicates of one row"""
    rng = np.random.default_rng(40 + int(contiguous))
    n, n_dup, b, k = 24_000, 160, 12, 15
    base = rng.standard_normal((1, D)).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    rows = (np.arange(n // 3, n // 3 + n_dup) if contiguous
            else np.sort(rng.choice(n, n_dup, replace=False)))
    x[rows] = base + 1e-5 * rng.standard_normal((n_dup, D)).astype(np.float32)
    q = np.concatenate([base + 0.02 * rng.standard_normal((b - 4, D)).astype(np.float32),
                        rng.standard_normal((4, D)).astype(np.float32)])
    idx = _index(gpu, x)
    s, i = _search(idx, q, k)
    _, _, tiers = idx.exactness_stats(b)
    so, io = O.search(O.encode_rows(x), q, k)
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(s, so)
    assert (tiers[: b - 4] >= 1).all(), tiers
    idx.close()


def test_saturated_cluster_takes_second_pass(gpu):
    """every other row a near-duplicate: every wave's list is full inside the band, so only the
    fp16 rescan (tier 2) can certify, with its own fp16 floor"""
    rng = np.random.default_rng(43)
    n = 200_000
    base = rng.standard_normal((1, D)).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    x[::2] = base + 1e-5 * rng.standard_normal((n // 2, D)).astype(np.float32)
    q = np.concatenate([base + 0.02 * rng.standard_normal((3, D)).astype(np.float32),
                        rng.standard_normal((2, D)).astype(np.float32)])
    idx = _index(gpu, x)
    s, i = _search(idx, q, 15)
    _, t2, tiers = idx.exactness_stats(5)
    so, io = O.search(idx.export_rows(), q, 15)
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(s, so)
    assert (tiers[:3] == 2).all() and t2 >= 3, tiers
    idx.close()


# ------------------------------------------------------- 4. the copy follows every mutation
def test_copy_follows_every_mutation(gpu):
    from ragmi.index import FlatIndex
    rng = np.random.default_rng(4)
    n, k = 3000, 15
    x = rng.standard_normal((n, D)).astype(np.float32)
    tags = rng.integers(1, 5, n).astype(np.uint32)
    fresh = rng.standard_normal((64, D)).astype(np.float32)
    q = np.concatenate([x[:8] + 0.05 * rng.standard_normal((8, D)).astype(np.float32),
                        fresh[:8] + 0.05 * rng.standard_normal((8, D)).astype(np.float32),
                        rng.standard_normal((16, D)).astype(np.float32)])
    idx = _index(gpu, x, tags)
    _same_in_both_modes(idx, q, k)
    # overwrite by upsert: rows the planted queries point at change
    idx.upsert(fresh[:32], np.arange(0, 64, 2, dtype=np.int64), np.full(32, 9, np.uint32))
    _same_in_both_modes(idx, q, k)
    # move_rows: the tail into the first slots
    idx.move_rows(np.arange(n - 20, n, dtype=np.int64), np.arange(100, 120, dtype=np.int64),
                  n - 20)
    _same_in_both_modes(idx, q, k)
    # remove_rows (deletion: survivors from the tail take the holes)
    idx.remove_rows(np.array([0, 1, 17, 500, 2000, idx.count - 1], np.int64))
    _same_in_both_modes(idx, q, k)
    # scatter_rows: gathered rows written back over other slots
    g16, g32, gt = idx.gather_rows(np.arange(200, 232, dtype=np.int64))
    idx.scatter_rows(np.arange(1000, 1032, dtype=np.int64), g16, g32, gt, idx.count)
    _same_in_both_modes(idx, q, k)
    # a reserve that grows capacity, then rows upserted into the new space
    idx.reserve(3 * n)
    _same_in_both_modes(idx, q, k)
    c = idx.count
    idx.upsert(fresh[32:], np.arange(c, c + 32, dtype=np.int64), np.full(32, 3, np.uint32))
    _same_in_both_modes(idx, q, k)
    # import_rows into a fresh index
    enc, tg = idx.export_rows(), idx.export_tags()
    idx2 = FlatIndex(dim=D, capacity=enc.shape[0], device=gpu)
    idx2.import_rows(enc, 0, tg, new_count=enc.shape[0])
    _same_in_both_modes(idx2, q, k)
    filt = np.array([[0xffffffff, 1 + (j % 4)] for j in range(32)], np.uint32)
    _same_in_both_modes(idx2, q, k, filters=filt, tags=tg)
    idx2.close()
    idx.close()


# --------------------------------------------------------------------------- 5. auto routing
def test_auto_mode_keeps_small_shards_on_fp16(gpu):
    rng = np.random.default_rng(5)
    n, b = 100_000, 32
    x = rng.standard_normal((n, D)).astype(np.float32)
    q = np.concatenate([x[rng.choice(n, 16, replace=False)] +
                        0.05 * rng.standard_normal((16, D)).astype(np.float32),
                        rng.standard_normal((16, D)).astype(np.float32)])
    idx = _index(gpu, x, mode=1)
    assert idx.prescan() == 1
    s1, i1 = _search(idx, q, 15)
    t1, t2, tiers = idx.exactness_stats(b)
    assert (tiers == 0).all() and t1 == 0 and t2 == 0, tiers     # the fp16 path, as before
    idx.set_prescan(2)
    s2, i2 = _search(idx, q, 15)
    np.testing.assert_array_equal(i1, i2)
    np.testing.assert_array_equal(s1, s2)
    idx.close()


def test_auto_mode_above_the_threshold(gpu):
    from ragmi.index import FlatIndex, PRESCAN_MIN_ROWS
    n, b, k = PRESCAN_MIN_ROWS + 48, 32, 15
    g = torch.Generator(device=gpu).manual_seed(6)
    idx = FlatIndex(dim=D, capacity=n, device=gpu)
    step = 1 << 18
    planted = None
    for r0 in range(0, n, step):
        m = min(step, n - r0)
        v = torch.randn((m, D), generator=g, device=gpu)
        if planted is None:
            planted = v[:16].clone()
        rows = torch.arange(r0, r0 + m, device=gpu)
        idx.upsert(v, rows, (rows % 7 + 1).to(torch.int32), new_count=r0 + m)
    q = torch.cat([planted + 0.05 * torch.randn((16, D), generator=g, device=gpu),
                   torch.randn((16, D), generator=g, device=gpu)])
    assert idx.prescan() == 1
    t1a, t2a, _ = idx.exactness_stats()
    s1, i1 = _search(idx, q, k)
    t1b, t2b, tiers = idx.exactness_stats(b)
    filt = np.array([[0xffffffff, 1 + (j % 7)] for j in range(b)], np.uint32)
    s1f, i1f = _search(idx, q, k, filters=filt)     # filtered passes route alike
    _, t2f, _ = idx.exactness_stats()
    idx.set_prescan(0)
    s0f, i0f = _search(idx, q, k, filters=filt)
    t1b2, t2b2, _ = idx.exactness_stats()
    s0, i0 = _search(idx, q, k)
    t1c, t2c, tiers0 = idx.exactness_stats(b)
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(i1f, i0f)
    np.testing.assert_array_equal(s1f, s0f)
    assert ((i1f % 7 + 1) == filt[:, 1:2]).all()
    print(f"auto at {n} rows: tier-1 {t1b - t1a}/{b}, tier-2 {t2b - t2a}; filtered tier-2 "
          f"{t2f - t2b}; fp16: tier-1 {t1c - t1b2}, tier-2 {t2c - t2b2}")
    assert (tiers0 == 0).all()                  # the fp16 path certifies random data directly
    assert t2b == t2a                           # and the prescan never needs the second pass
    # certify the batch as bench.py's verify_exact does: every row at or above the worst
    # returned exact score, rescored and ordered
    enc = idx.export_rows()
    qn = O.normalize(q.cpu().numpy())
    floor = O.rescore(enc, qn, i1).min(axis=1)
    cand = O.candidates_above(enc, qn, floor)
    for j in range(b):
        ids, sc = cand[j]
        order = np.lexsort((ids, -sc.astype(np.float64)))[:k]
        np.testing.assert_array_equal(ids[order], i1[j])
        np.testing.assert_array_equal(sc[order], s1[j])
    idx.close()


# -------------------------------------------------------------------------------- 6. streams
def test_streams_match_the_default_stream(gpu):
    from ragmi.index import PartitionStreams
    rng = np.random.default_rng(7)
    n, k = 60_000, 15
    x = rng.standard_normal((n, D)).astype(np.float32)
    idx = _index(gpu, x)
    qs = [torch.from_numpy(x[rng.choice(n, 32)] + 0.05 * rng.standard_normal((32, D))
                           .astype(np.float32)).to(gpu) for _ in range(4)]
    ref = [idx.search(q, k) for q in qs]
    torch.cuda.synchronize()
    so, io = O.search(O.encode_rows(x), qs[0].cpu().numpy(), k)
    np.testing.assert_array_equal(ref[0][1].cpu().numpy(), io)
    np.testing.assert_array_equal(ref[0][0].cpu().numpy(), so)
    # two streams, serial scan order (the large-shard serving loop)
    idx.set_scan_order(True)
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
    cur = torch.cuda.current_stream(gpu)
    outs = []
    for j, q in enumerate(qs):
        streams[j % 2].wait_stream(cur)
        with torch.cuda.stream(streams[j % 2]):
            outs.append(idx.search(q, k))
    torch.cuda.synchronize()
    for (s0, i0), (s1, i1) in zip(ref, outs):
        assert torch.equal(i0, i1) and torch.equal(s0, s1)
    idx.set_scan_order(False)
    # CU-partitioned streams (the small-shard serving loop)
    parts = PartitionStreams(gpu, 4)
    try:
        outs = []
        for j, q in enumerate(qs):
            parts[j].wait_stream(cur)
            with torch.cuda.stream(parts[j]):
                outs.append(idx.search(q, k))
        torch.cuda.synchronize()
        for (s0, i0), (s1, i1) in zip(ref, outs):
            assert torch.equal(i0, i1) and torch.equal(s0, s1)
    finally:
        parts.close()
        idx.close()
