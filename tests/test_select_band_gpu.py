"""GPU tests of select's tier 1 as a band gather: when the check cannot
certify a query from the approximate top-32 A, the lists whose head reaches the floor L are
gathered in chunks of 32 lists, their entries >= L that are not in A go to a 1024-row band
buffer, are rescored 32 per round, and the result is the top-k of A and those rows. A full
list whose tail (lane 31 of the list's own load) is >= L hands the query to the rescan. Every
result here is compared bit for bit (ids and scores) with oracle_scan.search on the exported
rows. Built around near-duplicate clusters (base + 1e-5 noise), which put many rows inside the
band, under the int8 prescan (mode 2), whose wider band makes tier 1 the normal case, and on
the fp16 scan (mode 0).

The tier assertions (exactness_stats) state the verdict, a property of the scan's lists, of
the seed and of L, which the band gather does not change: this file, run once against the
build before the band gather, passed with the same tiers. What decides them here:
  * under the prescan the seed is a lower bound of the 32nd best UPPER BOUND u, the floor L
    lies below the k-th best EXACT score, so a cluster that 32 or more sample tiles see puts
    the seed above L and the query takes tier 2 before any list is read. launch_prep8 samples
    tile floor(j n_tiles / n_sample), j < n_sample = max(256, n_tiles / 128) (at most every
    tile): random positions of 300 or 1500 cluster rows in 24 000 take tier 2, and so does the
    saturated corpus at any size from 512 rows (32 tiles) up. The chunked route of tier 1 (more
    than 32 lists, more than 1024 band rows) is therefore reached with the cluster in tiles the
    sample skips ("unsampled"), and on the fp16 scan, whose seed and L are on one scale.
  * the prescan's waves take PAIRS of tiles: its lists cover 32 consecutive rows or more, so
    at n = 100, all near-duplicates, three lists are full inside the band (no seed: 7 sample
    tiles). That case and a 64-row contiguous cluster test the fullness check of the gather.

Cases that differ from a literal reading of their specification, because of arithmetic:
  * band sweep, n_dup = 20 at k = 1 and 15: the cluster is smaller than A, so its 20 rows
    stand a whole cluster-to-random gap above the 32nd candidate and the check certifies them
    (tier 0). Tier >= 1 is asserted where the k-th and the 32nd best row lie in the same
    band: n_dup >= 32, or k = 32.
  * band sweep, n_dup = 300: "more rows with u >= e_k than the band buffer holds" cannot hold
    for 300 rows and a 1024-row buffer. It is asserted at 1500, where it proves that more than
    32 lists qualified (a list holds 32 entries); at 300 the count is asserted to need more
    than four rescoring rounds. Both only mean tier 1 work where tier 1 ran (above): the
    unsampled and mode-0 cases assert tier == 1.
  * tiny grid n = 40: A holds 32 rows, not all 40, so "passes without tier 1" is asserted on
    random rows at k = 15 (the margin certifies), and an n = 24 near-duplicate corpus is added,
    where A does hold every row.
"""
import numpy as np
import pytest
import torch

import oracle_scan as O

pytestmark = pytest.mark.gpu
D = 384
BAND_ROWS = 32 * 32          # kBandLists x kKS of certify_kernels.hip
SAT_N = 512                  # the saturated corpus: smallest size at which 32 sample tiles exist


def _index(gpu, x, tags=None, mode=2, storage="fp16"):
    from ragmi.index import FlatIndex
    idx = FlatIndex(dim=x.shape[1], capacity=x.shape[0], device=gpu, storage=storage)
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


def _same(idx, q, k, enc=None, tags=None, filt=None):
    s, i = _search(idx, q, k, filt)
    so, io = _oracle(idx.export_rows() if enc is None else enc, q, k, tags, filt)
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(s, so)
    return s, i


def _cluster(rng, n, dim, n_dup, n_near, n_rand, rows=None):
    """n random rows with n_dup near-duplicates of one base row at `rows` (random positions by
    default); n_near queries near the base, n_rand random ones"""
    base = rng.standard_normal((1, dim)).astype(np.float32)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    if rows is None:
        rows = np.sort(rng.choice(n, n_dup, replace=False))
    x[rows] = base + 1e-5 * rng.standard_normal((n_dup, dim)).astype(np.float32)
    q = np.concatenate([base + 0.02 * rng.standard_normal((n_near, dim)).astype(np.float32),
                        rng.standard_normal((n_rand, dim)).astype(np.float32)])
    return x, q, rows


def _unsampled_rows(rng, n, n_dup):
    """n_dup random rows in tiles the prescan's seed sample does not read (launch_prep8)"""
    nt = (n + 15) // 16
    ns = min(nt, max(256, nt // 128), 4096)
    sampled = np.unique(np.arange(ns, dtype=np.int64) * nt // ns)
    free = np.setdiff1d(np.arange(nt), sampled)
    rows = (free[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)
    return np.sort(rng.choice(rows[rows < n], n_dup, replace=False))


@pytest.fixture(scope="module")
def cluster160():
    """24 000 rows, 160 near-duplicates, 32 queries (24 near the base); the stored fp16 rows"""
    x, q, rows = _cluster(np.random.default_rng(160), 24_000, D, 160, 24, 8)
    return x, q, rows, O.encode_rows(x)


# ---------------------------------------------------------------------- 1. band size sweep
SWEEP = [(2, "random", d) for d in (20, 33, 40, 64, 65, 300, 1500)] + \
        [(2, "unsampled", 300), (2, "unsampled", 1500), (0, "random", 300), (0, "random", 1500)]


@pytest.mark.parametrize("mode,where,n_dup", SWEEP)
def test_band_size_sweep(gpu, mode, where, n_dup):
    rng = np.random.default_rng(1000 + n_dup)
    n = 24_000
    rows = _unsampled_rows(rng, n, n_dup) if where == "unsampled" else None
    x, q, rows = _cluster(rng, n, D, n_dup, 8, 4, rows=rows)
    idx = _index(gpu, x, mode=mode)
    enc = idx.export_rows()
    for k in (1, 15, 32):
        _same(idx, q, k, enc)
        _, _, tiers = idx.exactness_stats(12)
        print(f"mode {mode} {where} n_dup {n_dup} k {k}: tiers {tiers.tolist()}")
        if n_dup >= 32 or k == 32:      # the k-th and the 32nd best row share the band
            assert (tiers[:8] >= 1).all(), tiers
        if where == "unsampled" or mode == 0:
            assert (tiers[:8] == 1).all(), tiers         # the chunked route of tier 1 ran
    if n_dup >= 300 and mode == 2:
        k = 15
        so, _ = O.search(enc, q[:8], k)
        u = idx.prescan_bounds(q[:8], np.arange(n, dtype=np.int64)).cpu().numpy()
        in_band = (u >= so[:, k - 1:k]).sum(axis=1)
        print(f"n_dup {n_dup}: rows with u >= e_k per near-base query {in_band.tolist()}")
        if n_dup == 1500:
            # every such row has u >= L and, under tier 1, sits in a list of <= 32 entries
            assert (in_band > BAND_ROWS).all(), in_band
        else:
            assert (in_band - 32 > 4 * 32).all(), in_band    # A aside: more than four rounds
    if mode == 0:
        # the cluster's exact scores span less than qprep's fp16 bound (the query's rounding
        # alone: half an fp16 ulp, 2^-12, of a score near 1): every cluster row is in the band
        e = O.rescore(enc, O.normalize(q[:8]), np.broadcast_to(rows, (8, n_dup)).copy())
        print(f"cluster exact score span {(e.max(axis=1) - e.min(axis=1)).max():.3e}")
        assert (e.max(axis=1) - e.min(axis=1) < 2.0 ** -13).all()
    idx.close()


# --------------------------------------------------------------------------- 2. exact ties
@pytest.mark.parametrize("k", [15, 32])
def test_exact_ties_lowest_rows_first(gpu, k):
    rng = np.random.default_rng(22)
    n = 5000
    x = rng.standard_normal((n, D)).astype(np.float32)
    copies = np.sort(rng.choice(n, 40, replace=False))
    x[copies] = x[copies[0]]
    q = x[copies[:1]].copy()
    idx = _index(gpu, x)
    s, i = _same(idx, q, k)
    _, _, tiers = idx.exactness_stats(1)
    print(f"exact ties k {k}: tier {tiers.tolist()}")
    assert tiers[0] == 1, tiers               # 8 copies outside A, found by the band gather
    np.testing.assert_array_equal(i[0], copies[:k])
    assert (s[0] == s[0, 0]).all()
    assert len(set(i[0].tolist())) == k
    idx.close()


# --------------------------------------------------------------------------- 3. tiny grids
@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("k", [1, 15, 32])
def test_tiny_all_near_duplicates(gpu, k, mode):
    """n = 100, seven tiles, 68 band rows outside A. fp16 scan: one tile per list, every list
    short, tier 1. Prescan: a pair of tiles per list, three full lists inside the band, which
    the gather must report (no seed at seven sample tiles): tier 2."""
    x, q, _ = _cluster(np.random.default_rng(3), 100, D, 100, 8, 4, rows=np.arange(100))
    idx = _index(gpu, x, mode=mode)
    _same(idx, q, k)
    _, _, tiers = idx.exactness_stats(12)
    print(f"n 100 k {k} mode {mode}: tiers {tiers.tolist()}")
    assert (tiers[:8] == (2 if mode == 2 else 1)).all(), tiers
    idx.close()


def test_tiny_certified_without_tier1(gpu):
    rng = np.random.default_rng(4)
    # n = 40 random rows, k = 15: the 15th and the 32nd of 40 scores lie far apart
    x = rng.standard_normal((40, D)).astype(np.float32)
    q = np.concatenate([x[:8] + 0.05 * rng.standard_normal((8, D)).astype(np.float32),
                        rng.standard_normal((4, D)).astype(np.float32)])
    idx = _index(gpu, x)
    _same(idx, q, 15)
    _, _, tiers = idx.exactness_stats(12)
    assert (tiers == 0).all(), tiers
    idx.close()
    # n = 24 near-duplicates: A holds every row
    x, q, _ = _cluster(rng, 24, D, 24, 8, 4, rows=np.arange(24))
    idx = _index(gpu, x)
    for k in (15, 32):
        s, i = _same(idx, q, k)
        _, _, tiers = idx.exactness_stats(12)
        assert (tiers == 0).all(), tiers
        assert (i[:, 24:] == -1).all()
    idx.close()


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("k", [15, 32])
def test_partial_last_tile(gpu, k, mode):
    rng = np.random.default_rng(5)
    n = 2999
    rows = np.sort(rng.choice(n - 8, 152, replace=False))
    rows = np.concatenate([rows, np.arange(n - 8, n)])       # the partial tile is in the cluster
    x, q, _ = _cluster(rng, n, D, 160, 8, 4, rows=rows)
    idx = _index(gpu, x, mode=mode)
    _same(idx, q, k)
    _, _, tiers = idx.exactness_stats(12)
    print(f"n 2999 k {k} mode {mode}: tiers {tiers.tolist()}")
    assert (tiers[:8] >= 1).all(), tiers
    if mode == 0:
        assert (tiers[:8] == 1).all(), tiers
    idx.close()


# --------------------------------------------------------- 4. a full list inside the band
def test_saturated_cluster_takes_second_pass(gpu):
    """test_prescan_gpu's saturated corpus (every other row a near-duplicate) at SAT_N rows"""
    rng = np.random.default_rng(43)
    n = SAT_N
    base = rng.standard_normal((1, D)).astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    x[::2] = base + 1e-5 * rng.standard_normal((n // 2, D)).astype(np.float32)
    q = np.concatenate([base + 0.02 * rng.standard_normal((3, D)).astype(np.float32),
                        rng.standard_normal((2, D)).astype(np.float32)])
    idx = _index(gpu, x)
    _same(idx, q, 15)
    _, t2, tiers = idx.exactness_stats(5)
    print(f"saturated n {n}: tiers {tiers.tolist()} t2 {t2}")
    assert (tiers[:3] == 2).all() and t2 >= 3, tiers
    idx.close()


def test_full_list_read_off_the_gather(gpu):
    """64 contiguous near-duplicates at a multiple of 32 in 24 000 rows: two prescan lists hold
    32 cluster rows each, full and wholly inside the band, while at most four sample tiles see
    the cluster (the seed stays at the random rows' level, below L). Only the tail on lane 31
    of the gathered list tells tier 2 from tier 1; the same 64 rows scattered (the sweep) take
    tier 1."""
    rng = np.random.default_rng(44)
    x, q, _ = _cluster(rng, 24_000, D, 64, 8, 4, rows=np.arange(8000, 8064))
    idx = _index(gpu, x)
    for k in (15, 32):
        t2a = idx.exactness_stats()[1]
        _same(idx, q, k)
        _, t2, tiers = idx.exactness_stats(12)
        print(f"contiguous 64 k {k}: tiers {tiers.tolist()} t2 {t2 - t2a}")
        assert (tiers[:8] == 2).all() and t2 - t2a >= 8, tiers
    idx.close()


# ------------------------------------------------- 5. the other instantiations of select
def test_fp16_scan_d384(gpu, cluster160):
    x, q, _, enc = cluster160
    idx = _index(gpu, x, mode=0)
    _same(idx, q[:28], 15, enc)
    _, _, tiers = idx.exactness_stats(28)
    print(f"mode 0 D 384: tiers {tiers.tolist()}")
    assert (tiers[:24] == 1).all(), tiers
    idx.close()


def test_d1024(gpu):
    x, q, _ = _cluster(np.random.default_rng(1024), 9_000, 1024, 160, 8, 4)
    idx = _index(gpu, x, mode=0)
    _same(idx, q, 15)
    _, _, tiers = idx.exactness_stats(12)
    print(f"D 1024: tiers {tiers.tolist()}")
    assert (tiers[:8] == 1).all(), tiers
    idx.close()


def test_fp32_storage(gpu, cluster160):
    x, q, _, _ = cluster160
    idx = _index(gpu, x, mode=0, storage="fp32")
    s, i = _search(idx, q[:12], 15)
    so, io = O.search(idx.export_rows32(), q[:12], 15)
    np.testing.assert_array_equal(i, io)
    np.testing.assert_array_equal(s, so)
    _, _, tiers = idx.exactness_stats(12)
    print(f"fp32 storage: tiers {tiers.tolist()}")
    assert (tiers[:12] == 1).all(), tiers
    idx.close()


# ------------------------------------------------------------------------------ 6. filtered
def test_filtered_band(gpu, cluster160):
    x, q, rows, enc = cluster160
    tags = np.random.default_rng(6).integers(1, 3, x.shape[0]).astype(np.uint32)
    tags[rows] = 1 + (np.arange(len(rows)) % 2)              # the cluster carries both values
    filt = np.array([[0xffffffff, (1, 2, 9)[j % 3]] for j in range(32)], np.uint32)
    idx = _index(gpu, x, tags)
    s, i = _same(idx, q, 15, enc, tags, filt)
    _, _, tiers = idx.exactness_stats(32)
    print(f"filtered: tiers {tiers.tolist()}")
    assert (i[2::3] == -1).all()                             # no row carries 9
    sel = np.arange(24)[np.arange(24) % 3 != 2]
    assert (tiers[sel] == 1).all(), tiers
    idx.close()


# -------------------------------------------------------------------------- 7. batch shapes
@pytest.mark.parametrize("b", [1, 32])
def test_batch_shapes(gpu, cluster160, b):
    x, q, _, enc = cluster160
    idx = _index(gpu, x)
    _same(idx, q[:b], 15, enc)
    _, _, tiers = idx.exactness_stats(b)
    assert (tiers[:min(b, 24)] == 1).all(), tiers
    idx.close()
