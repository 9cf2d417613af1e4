"""GPU tests of tier 1 spread over the chip after the 6-bit prescan: select's
head instantiation stops at the verdict and leaves a record per tier-1 query; band_kernel's grid
(S, B) gathers and rescores a query's qualifying lists in chunks of 32, slice s taking the chunks
s, s + S, ...; every slice publishes its 32 best band rows and a full-list flag and arrives at
the query's ticket, and the last arriver merges A with the S lists (or hands the query to tier 2).

Everything runs under set_prescan(3) on small indexes, and every result is compared bit for bit
with oracle_scan and with mode 0 on the same index (`both`). Nothing here carries a tolerance.
The harness is test_prescan_routes_gpu's, the cluster geometries are test_select_band_gpu's.

What decides the cases (reasoned from the kernels, not read off a run):
  * 24 000 rows are 750 tile pairs for the 6-bit scan's 1024 waves: a wave's list covers at most
    one pair, so the qualifying lists of a query are the distinct pairs that hold a row with
    u >= L, L = e_k - 2^-20 in fp32 (eps of a prescan pass is kU8Slack). u comes from
    prescan_bounds, e_k from the oracle: `n_lists_of`. With S = 4 slices and chunks of 32 lists,
    fewer than 4 chunks leave slices empty, 4..7 give every slice one or two, 8 or more give
    every slice several. Reasoned sizes: 5 duplicates leave the band to the random rows (about
    100 rows with u >= e_15 in 24 000, more for e_32), 40 duplicates are the whole band (40
    lists), 300 and 1500 fill 250 and 630 of the 750 pairs.
  * a cluster in tiles the seed sample skips keeps the seed below L (tier 1); one the sample
    sees puts the seed above L (tier 2 by the seed); 64 contiguous near-duplicates fill two
    lists inside the band, which only the slice that gathers them sees (tier 2 by fullness).
"""
import functools

import numpy as np
import pytest
import torch

import oracle_scan as O
import test_filters_gpu as TF
import test_select_band_gpu as SB
from test_prescan_routes_gpu import OFFSET, lists, make_index, oracle, same, unpacked

pytestmark = pytest.mark.gpu
D = 384
N = 24_000
SLICES = 4                    # kBandSlices of index_search.hip
CHUNK = 32                    # kBandLists
ALL = 0xFFFFFFFF
SLACK = np.float32(2.0 ** -20)


def both(idx, run):
    """run() under mode 0, then under mode 3 (left set): equal results; returns mode 3's"""
    idx.set_prescan(0)
    r0 = run()
    idx.set_prescan(3)
    p6 = idx.prescan6_passes()
    r3 = run()
    assert idx.prescan6_passes() > p6
    same(r0, r3)
    return r3


def n_lists_of(idx, q, e_k):
    """qualifying lists per query (mode 3 set): distinct tile pairs with a row of u >= L"""
    u = idx.prescan_bounds(q, np.arange(idx.count, dtype=np.int64)).cpu().numpy()
    L = e_k.astype(np.float32) - SLACK
    return np.array([len(np.unique(np.nonzero(u[j] >= L[j])[0] // 32)) for j in range(len(q))])


# ------------------------------------------------------------------- 1. chunk counts around S
@pytest.mark.parametrize("n_dup,want", [(5, ("fewer", "one")), (40, ("fewer", "fewer")),
                                        (300, ("several", "several")),
                                        (1500, ("several", "several"))])
def test_chunk_counts_around_the_slices(gpu, n_dup, want):
    rng = np.random.default_rng(7000 + n_dup)
    x, q, _ = SB._cluster(rng, N, D, n_dup, 8, 4, rows=SB._unsampled_rows(rng, N, n_dup))
    idx = make_index(gpu, x)
    enc = O.encode_rows(x)
    for k in (15, 32):
        got = both(idx, lambda: lists(idx.search(q, k)))
        _, _, tiers = idx.exactness_stats(len(q))
        same(got, oracle(enc, q, k))
        nl = n_lists_of(idx, q, got[0][:, k - 1].view(np.float32))
        chunks = -(-nl // CHUNK)
        print(f"n_dup {n_dup} k {k}: lists {nl.tolist()} chunks {chunks.tolist()} "
              f"tiers {tiers.tolist()}")
        assert (tiers[:8] == 1).all(), tiers
        cls = {"fewer": chunks < SLICES,
               "one": (chunks >= SLICES) & (chunks < 2 * SLICES),
               "several": chunks >= 2 * SLICES}[want[k == 32]]
        assert cls[:8].all(), (want, k, chunks)
    idx.close()


# ---------------------------------------------------------------------- 2. ties across slices
@pytest.mark.parametrize("k", [32, 15])
@pytest.mark.parametrize("where", ["random", "unsampled"])
def test_ties_across_slices(gpu, where, k):
    """40 identical rows: A holds 32 of them, the other 8 come back from the slices, and equal
    scores meet in the last arriver's merge: lowest row first, no id twice. At random rows of 5000
    most tiles are sampled (the seed may stand at the copies' own u: tier 1 or 2); at unsampled
    rows of 24 000 the verdict is tier 1 and the copies' ~40 lists are two chunks, two slices."""
    rng = np.random.default_rng(22)
    n = 5000 if where == "random" else N
    x = rng.standard_normal((n, D)).astype(np.float32)
    copies = (np.sort(rng.choice(n, 40, replace=False)) if where == "random"
              else SB._unsampled_rows(rng, n, 40))
    x[copies] = x[copies[0]]
    q = x[copies[:1]].copy()
    idx = make_index(gpu, x)
    s, i = both(idx, lambda: lists(idx.search(q, k)))
    _, _, tiers = idx.exactness_stats(1)
    same((s, i), oracle(O.encode_rows(x), q, k))
    print(f"ties {where} k {k}: tier {tiers.tolist()}")
    assert tiers[0] >= 1 and (where == "random" or tiers[0] == 1), tiers
    np.testing.assert_array_equal(i[0], copies[:k])
    assert (s[0] == s[0, 0]).all() and len(set(i[0].tolist())) == k
    idx.close()


# ------------------------------------------------------------- 3. fullness seen by one slice
def test_fullness_seen_by_one_slice(gpu):
    rng = np.random.default_rng(44)
    x, q, _ = SB._cluster(rng, N, D, 64, 8, 4, rows=np.arange(8000, 8064))
    idx = make_index(gpu, x)
    enc = O.encode_rows(x)
    idx.set_prescan(3)
    for k in (15, 32):
        t1a, t2a, _ = idx.exactness_stats()
        got = lists(idx.search(q, k))
        t1, t2, tiers = idx.exactness_stats(len(q))
        same(got, oracle(enc, q, k))
        print(f"contiguous 64 k {k}: tiers {tiers.tolist()} t1 +{t1 - t1a} t2 +{t2 - t2a}")
        assert (tiers[:8] == 2).all(), tiers
        # one tier-2 count per tier-2 query (not one per slice), and no tier-1 count for it
        assert t2 - t2a == int((tiers == 2).sum()) and t1 - t1a == int((tiers == 1).sum())
    idx.close()


# ------------------------------------------------------------------------ 4..7: one mixed index
@functools.lru_cache(maxsize=None)
def world():
    """24 000 rows with three near-duplicate clusters: U (300 rows in tiles the seed sample
    skips: tier 1), V (300 rows at random positions, which the sample sees: tier 2 by the seed)
    and F (64 contiguous rows: tier 2 by fullness); 20 rows carry tag 7, the others tag 1.
    70 queries: [0, 8) near U, [8, 16) near V, [16, 24) near F, [24, 32) random, then the same
    kinds in turn."""
    from ragmi.filters import eval_view_np, pack_view
    rng = np.random.default_rng(17)
    x = rng.standard_normal((N, D)).astype(np.float32)
    base = rng.standard_normal((3, D)).astype(np.float32)
    f_rows = np.arange(8000, 8064)
    u_rows = SB._unsampled_rows(rng, N, 300)
    u_rows = u_rows[(u_rows < 7968) | (u_rows >= 8096)]
    v_rows = np.setdiff1d(np.sort(rng.choice(N, 300, replace=False)),
                          np.concatenate([u_rows, np.arange(7968, 8096)]))
    for b, rows in enumerate((u_rows, v_rows, f_rows)):
        x[rows] = base[b] + 1e-5 * rng.standard_normal((len(rows), D)).astype(np.float32)
    tags = np.ones(N, np.uint32)
    few = np.setdiff1d(rng.choice(N, 40, replace=False),
                       np.concatenate([u_rows, v_rows, f_rows]))[:20]
    tags[few] = 7
    kind = np.concatenate([np.repeat(np.arange(4), 8), np.arange(38) % 4])
    q = rng.standard_normal((70, D)).astype(np.float32)
    near = kind < 3
    q[near] = base[kind[near]] + 0.02 * rng.standard_normal((int(near.sum()), D)).astype(np.float32)
    blob = pack_view([TF.P([("maskeq", ALL, 7)], 0b10), TF.P([("maskeq", ALL, 1)], 0b10)])
    return dict(x=x, q=q, kind=kind, tags=tags, enc=O.encode_rows(x), blob=blob,
                view=eval_view_np(blob, tags))


@pytest.fixture(scope="module")
def idx0(gpu):
    c = world()
    idx = make_index(gpu, c["x"], c["tags"])
    idx.set_prescan(3)
    yield idx
    idx.close()


@functools.lru_cache(maxsize=None)
def want_plain(k):
    c = world()
    return oracle(c["enc"], c["q"], k)


def mixed_filters(kind, view):
    """random queries ask for the 20 rows of tag 7 (fewer than 32 rows: tier 0), the others for
    every row; as legacy (mask, value) pairs or as bits of the view (program 0: tag 7)"""
    if view:
        return np.array([[1, 1] if t == 3 else [0, 0] for t in kind], np.uint32)
    return np.array([[ALL, 7] if t == 3 else [0, 0] for t in kind], np.uint32)


WANT_TIER = np.array([1, 2, 2, 0])      # by query kind, under mixed_filters


@pytest.mark.parametrize("view", [False, True])
def test_mixed_pass(gpu, idx0, view):
    c = world()
    q, kind = c["q"][:32], c["kind"][:32]
    filt = mixed_filters(kind, view)
    progs = c["blob"] if view else None
    k = 15
    t1a, t2a, _ = idx0.exactness_stats()
    got = lists(idx0.search(q, k, filters=filt, programs=progs))
    t1, t2, tiers = idx0.exactness_stats(32)
    print(f"mixed pass view {view}: tiers {tiers.tolist()}")
    same(got, oracle(c["enc"], q, k, c["view"] if view else c["tags"], filt))
    np.testing.assert_array_equal(tiers, WANT_TIER[kind])
    assert (t1 - t1a, t2 - t2a) == (8, 16)
    idx0.set_prescan(0)
    try:
        same(lists(idx0.search(q, k, filters=filt, programs=progs)), got)
    finally:
        idx0.set_prescan(3)


def test_rearming_over_twenty_searches(gpu, idx0):
    """two batches with different tier mixes alternate on one workspace: the tickets are
    re-armed and every record rewritten by each pass, so every result equals its first"""
    c = world()
    k = 15
    order = [np.arange(32), np.concatenate([np.arange(24, 32), np.arange(8, 24)[::-1],
                                            np.arange(32, 40)])]
    outs = [idx0.search(c["q"][order[j % 2]], k, filters=mixed_filters(c["kind"][order[j % 2]], False))
            for j in range(20)]
    got = [lists(o) for o in outs]
    for j in range(2):
        o = order[j]
        same(got[j], oracle(c["enc"], c["q"][o], k, c["tags"], mixed_filters(c["kind"][o], False)))
    for j in range(2, 20):
        same(got[j], got[j % 2])


def test_four_streams_four_workspaces(gpu, idx0):
    c = world()
    k = 15
    jobs = [c["q"][:32], c["q"][32:64], c["q"][16:48], c["q"][38:70]] * 3
    single = [lists(idx0.search(q, k)) for q in jobs[:4]]
    for j, s in enumerate([(0, 32), (32, 64), (16, 48), (38, 70)]):
        same(single[j], tuple(a[s[0]:s[1]] for a in want_plain(k)))
    cur = torch.cuda.current_stream(gpu)
    streams = [torch.cuda.Stream(gpu) for _ in range(4)]
    outs = []
    for j, q in enumerate(jobs):
        s = streams[(j + j // 4) % 4]          # a job meets another stream in every round
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            outs.append(idx0.search(q, k))
    for j, o in enumerate(outs):
        same(lists(o), single[j % 4])


@pytest.mark.parametrize("k", [1, 15, 32])
@pytest.mark.parametrize("B", [1, 6, 32, 70])
def test_shapes(gpu, idx0, B, k):
    """B = 70 is three passes, the last with 6 queries; plain, packed with an id offset, and the
    FILTER instantiation through a legacy filter and through a view"""
    c = world()
    q, kind = c["q"][:B], c["kind"][:B]
    ws, wi = (a[:B] for a in want_plain(k))
    same(lists(idx0.search(q, k)), (ws, wi))
    same(unpacked(idx0.search_packed(q, k, id_offset=OFFSET)),
         (ws, np.where(wi >= 0, wi + OFFSET, -1)))
    if k == 15 or B == 70:
        legacy, vf = mixed_filters(kind, False), mixed_filters(kind, True)
        same(lists(idx0.search(q, k, filters=legacy)), oracle(c["enc"], q, k, c["tags"], legacy))
        same(unpacked(idx0.search_packed(q, k, filters=vf, id_offset=OFFSET, programs=c["blob"])),
             oracle(c["enc"], q, k, c["view"], vf, OFFSET))
    if B == 70 and k == 15:
        idx0.set_prescan(0)
        try:
            same(lists(idx0.search(q, k)), (ws, wi))
        finally:
            idx0.set_prescan(3)
