"""GPU tests of every search route over the int8 prescan (DESIGN.md "int8 prescan"): dim 384,
fp16 storage, the routes that end in search_locked beside the plain FlatIndex.search — the
packed exchange form with an id offset, searches of several passes, filter views, RANGE atoms on
key columns, the fallback tiers under a filter, tiny indexes, scan order 2, the MMR / grouped /
fusion compositions, the shard set and the QdrantClient front end.

Every route runs through `both_modes`: once under prescan mode 0 (the fp16 scan) and once under
mode 2 (the int8 prescan at any size) on the same index, or on every shard of a set, which
asserts
  (a) equal ids, and equal scores as int32 bit patterns, in both modes,
  (b) prescan_passes() unchanged by the mode-0 run,
and returns the mode-2 result with each handle's counter move, of which every test asserts
  (c) exactly ceil(B / 32) per k <= 32 search (per shard for a set; more than zero for the
      front end, whose pass count is its own matter), and
  (d) equality with the CPU reference of the route (oracle_scan, tests/_*_ref.py,
      ragmi.shardset.gather_merge_np).
Nothing here carries a tolerance.

The default corpus: 3017 rows = 189 tiles, an odd count (the prescan's last pair has a spare
tile and a clipped tag descriptor) with a partial last tile; tags and payloads from
test_filters_gpu (12 tickers x 3 document types, five rows without either: tag 0); 70 queries,
alternately 16 planted (a row plus 0.05 noise) and 16 random ones.
"""
import datetime as dt
import functools

import numpy as np
import pytest
import torch

import _fusion_ref as F
import _groups_ref as R
import _mmr_ref as M
import oracle_scan as O
import test_filters_gpu as TF
import test_range_gpu as TR
import test_select_band_gpu as SB
from _filters_ref import matches
from _range_ref import matches_range

pytestmark = pytest.mark.gpu

D = 384
N = 3017
OFFSET = 5_000_000
ALL = 0xFFFFFFFF
FIVE = (ALL, 0)                  # the five rows without ticker and document type
NONE = (ALL, 0x7FFF7FFF)         # a tag no row carries
KS = [1, 15, 32]


# ------------------------------------------------------------------------------ the harness
def passes(B: int) -> int:
    """search passes of one k <= 32 search of B queries"""
    return -(-B // 32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def fbits(v) -> int:
    """the bit pattern of one fp32 score"""
    return int(np.float32(v).view(np.int32))


def lists(out):
    """(scores, ids) cuda tensors -> (score bits int32, ids int64) host arrays"""
    s, i = out
    torch.cuda.synchronize()
    return s.view(torch.int32).cpu().numpy(), i.cpu().numpy()


def unpacked(p):
    """a packed result int32 [B, k, 2] -> (score bits, ids int64) host arrays"""
    torch.cuda.synchronize()
    p = p.cpu().numpy()
    return np.ascontiguousarray(p[..., 0]), p[..., 1].astype(np.int64)


def same(a, b):
    if isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype, (a.dtype, getattr(b, "dtype", None))
        np.testing.assert_array_equal(a, b)
    elif isinstance(a, (list, tuple)) and any(isinstance(x, (np.ndarray, list, tuple)) for x in a):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same(x, y)
    else:
        assert a == b


def both_modes(handles, run):
    """`run()` under prescan mode 0, then under mode 2, on FlatIndex `handles`. Asserts (a) and
    (b); returns (the mode-2 result, each handle's prescan_passes() move under mode 2). The
    handles are left in auto mode."""
    try:
        for h in handles:
            h.set_prescan(0)
        before = [h.prescan_passes() for h in handles]
        r0 = run()
        assert [h.prescan_passes() for h in handles] == before               # (b)
        for h in handles:
            h.set_prescan(2)
        r2 = run()
        moved = [h.prescan_passes() - n for h, n in zip(handles, before)]
    finally:
        for h in handles:
            h.set_prescan(1)
    same(r0, r2)                                                             # (a)
    return r2, moved


def oracle(enc, q, k, column=None, filt=None, offset=0):
    """oracle_scan.search per distinct (mask, value) of `filt` [B, 2] over tag or view column
    `column`: (score bits, ids + offset with -1 padding)."""
    q = np.ascontiguousarray(q, np.float32)
    if filt is None:
        s, i = O.search(enc, q, k)
    else:
        filt = np.asarray(filt, np.uint32).reshape(len(q), 2)
        s = np.empty((len(q), k), np.float32)
        i = np.empty((len(q), k), np.int64)
        for m, v in sorted({(int(a), int(b)) for a, b in filt}):
            sel = np.nonzero((filt[:, 0] == m) & (filt[:, 1] == v))[0]
            s[sel], i[sel] = O.search(enc, q[sel], k, tags=column, mask=m, value=v,
                                      use_filter=True)
    return bits(s), np.where(i >= 0, i + offset, -1)


def make_index(gpu, x, tags=None, keys=None):
    from ragmi.index import FlatIndex
    n = len(x)
    idx = FlatIndex(D, max(n, 16), gpu, "fp16")
    if n:
        idx.upsert(x, np.arange(n, dtype=np.int64), tags, new_count=n)
    if keys is not None:
        idx.keys_create(len(keys))
        for c, col in enumerate(keys):
            idx.write_keys(c, np.arange(n), col)
    assert idx.prescan() == 1 and idx.prescan_passes() == 0
    return idx


def view_filt(B, U):
    """query j asks for program bit j % (U + 1); slot U: (0, 0), every row"""
    slot = np.arange(B) % (U + 1)
    return slot, np.array([[0, 0] if s == U else [1 << s, 1 << s] for s in slot], np.uint32)


# ------------------------------------------------------------------------- the default corpus
@functools.lru_cache(maxsize=None)
def world():
    from ragmi.filters import compile_program, eval_view_np, pack_view
    from ragmi.qdrant import PayloadTags
    rng = np.random.default_rng(N)
    x = rng.standard_normal((N, D)).astype(np.float32)
    pay = TF.corpus_payloads(rng, N)
    pt = PayloadTags()
    tags = np.array([pt.tag(p) for p in pay], np.uint32)
    assert int((tags == 0).sum()) == 5
    q = rng.standard_normal((70, D)).astype(np.float32)
    planted = (np.arange(70) // 16) % 2 == 0
    q[planted] = x[rng.choice(N, int(planted.sum()), replace=False)] + \
        0.05 * rng.standard_normal((int(planted.sum()), D)).astype(np.float32)
    flts = TF.named_filters()
    progs = [compile_program(pt, f) for f in flts.values()] + [TF.P([("maskeq", 0xFFFF, 1)], 0)]
    blob = pack_view(progs)
    view = eval_view_np(blob, tags)
    for s, f in enumerate(flts.values()):            # the view is the plain evaluator's
        np.testing.assert_array_equal((view >> s) & 1, np.array([matches(f, p) for p in pay]))
    assert int(((view >> 7) & 1).sum()) == 5 and not ((view >> 8) & 1).any()
    return dict(x=x, pay=pay, pt=pt, tags=tags, q=q, enc=O.encode_rows(x), blob=blob, view=view,
                U=len(progs))


def tag_filters(B, pt):
    """Per-query legacy filters that differ between a pass and the next one (query j and
    query j + 32 never ask alike): ticker codes, document types, both, the five-row tag, a tag no
    row carries, and (0, 0)."""
    f = np.empty((B, 2), np.uint32)
    for j in range(B):                 # the kind is j % 3, and (j + 32) % 3 != j % 3
        t = pt.codes[0][TF.TICKERS[(j // 3 + j // 32) % 12]]
        d = pt.codes[1][TF.TYPES[(j // 3) % 3]] << 16
        f[j] = [(0xFFFF, t), (0xFFFF0000, d), (ALL, t | d)][j % 3]
    f[0] = (0, 0)
    f[1] = FIVE
    if B > 2:
        f[2] = NONE
    if B > 32:
        f[32] = FIVE                   # the first query of the second pass
        f[B - 1] = NONE if B > 33 else FIVE
    return f


@pytest.fixture(scope="module")
def idx0(gpu):
    c = world()
    idx = make_index(gpu, c["x"], c["tags"])
    yield idx
    idx.close()


# ------------------------------------------------------------------------------ 1. packed form
@pytest.mark.parametrize("k", KS)
def test_packed_form_with_id_offset(gpu, idx0, k):
    c = world()
    q = c["q"][:32]
    for filt in (None, tag_filters(32, c["pt"])):
        def run():
            p1 = idx0.search_packed(q, k, filters=filt, id_offset=OFFSET)
            p2 = idx0.search_packed(q, k, filters=filt, id_offset=OFFSET)
            torch.cuda.synchronize()
            assert torch.equal(p1, p2)               # a second identical call: the same tensor
            return unpacked(p1)
        got, moved = both_modes([idx0], run)
        assert moved == [2 * passes(32)]                                     # (c)
        same(got, oracle(c["enc"], q, k, c["tags"], filt, OFFSET))           # (d)
        if filt is not None:
            ids = got[1]
            assert ((ids[1] >= OFFSET).sum() == min(k, 5)) and (ids[1, 5:] == -1).all()
            assert (ids[2] == -1).all()
            assert (ids[ids >= 0] >= OFFSET).all()


# -------------------------------------------------------------------------- 2. several passes
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B", [33, 70])
def test_several_passes_with_filters_that_differ_between_them(gpu, idx0, B, k):
    c = world()
    q = c["q"][:B]
    filt = tag_filters(B, c["pt"])
    assert not (filt[:B - 32] == filt[32:B]).all(axis=1).any()

    def run():
        return (lists(idx0.search(q, k, filters=filt)),
                unpacked(idx0.search_packed(q, k, filters=filt, id_offset=OFFSET)))
    (got, got_p), moved = both_modes([idx0], run)
    assert moved == [2 * passes(B)]                                          # (c)
    same(got, oracle(c["enc"], q, k, c["tags"], filt))                       # (d)
    same(got_p, oracle(c["enc"], q, k, c["tags"], filt, OFFSET))
    assert (got[1][32] >= 0).sum() == min(k, 5)


# ------------------------------------------------------------------------------ 3. filter views
@pytest.mark.parametrize("k", KS)
def test_filter_views(gpu, idx0, k):
    """general programs (should, must_not, MatchAny, MatchExcept, is-empty, min_should, one
    matching five rows, one matching none), B = 40: two passes"""
    c = world()
    B = 40
    q = c["q"][:B]
    slot, filt = view_filt(B, c["U"])

    def run():
        return (lists(idx0.search(q, k, filters=filt, programs=c["blob"])),
                unpacked(idx0.search_packed(q, k, filters=filt, id_offset=OFFSET,
                                            programs=c["blob"])))
    (got, got_p), moved = both_modes([idx0], run)
    assert moved == [2 * passes(B)]                                          # (c)
    same(got, oracle(c["enc"], q, k, c["view"], filt))                       # (d)
    same(got_p, oracle(c["enc"], q, k, c["view"], filt, OFFSET))
    ids = got[1]
    assert (ids[slot == 8] == -1).all()                                      # matches none
    assert ((ids[slot == 7] >= 0).sum(axis=1) == min(k, 5)).all()            # padding past five
    assert idx0.unanswered() == 0


@pytest.mark.parametrize("k", KS)
def test_program_equal_to_a_legacy_filter_gives_the_legacy_tensors(gpu, idx0, k):
    from ragmi.filters import FilterProgram, pack_view
    c = world()
    B = 40
    q = c["q"][:B]
    legacy = tag_filters(B, c["pt"])
    pairs = [tuple(int(v) for v in p) for p in legacy]
    distinct = sorted(set(p for p in pairs if p != (0, 0)))
    assert 16 < len(distinct) <= 32
    blob = pack_view([FilterProgram.maskeq(m, v) for m, v in distinct])
    over_view = np.array([[0, 0] if p == (0, 0) else [1 << distinct.index(p)] * 2 for p in pairs],
                         np.uint32)

    def run():
        return (lists(idx0.search(q, k, filters=legacy)),
                lists(idx0.search(q, k, filters=over_view, programs=blob)),
                unpacked(idx0.search_packed(q, k, filters=legacy)),
                unpacked(idx0.search_packed(q, k, filters=over_view, programs=blob)))
    (l1, l2, p1, p2), moved = both_modes([idx0], run)
    assert moved == [4 * passes(B)]                                          # (c)
    same(l1, l2)
    same(p1, p2)
    same(l1, p1)
    same(l1, oracle(c["enc"], q, k, c["tags"], legacy))                      # (d)


# ------------------------------------------------------------------------------ 4. range views
@functools.lru_cache(maxsize=None)
def range_world(n_cols):
    """test_range_gpu's corpus (3001 rows, 40 queries, the first eight at a 64-row cluster).
    Four key columns: its own programs, view and query filters. One column (fiscal_year): seven
    programs of RANGE atoms (closed, half-open, empty interval, is-empty, five rows, no row)
    mixed with tag atoms, each held equal to _range_ref on the payloads."""
    from ragmi import qdrant_models as m
    from ragmi.filters import PayloadRanges, compile_program, eval_view_np, pack_view
    c = TR.corpus(384)
    if n_cols == 4:
        return dict(c, U=9, kinds=TR.KINDS)
    kinds = {"fiscal_year": "number"}
    pt, pr = c["pt"], PayloadRanges(kinds)
    fc = m.FieldCondition
    year = lambda **kw: fc("fiscal_year", range=m.Range(**kw))
    no_year = m.IsEmptyCondition(m.PayloadField("fiscal_year"))
    flts = [
        m.Filter(must=[year(gte=2021, lte=2023)]),                                        # closed
        m.Filter(must=[year(gte=2022), fc("ticker", m.MatchAny(any=["T01", "T02", "T03", "T04"]))]),
        m.Filter(must_not=[year(lt=2021), fc("document_type", m.MatchValue("8-K"))]),      # half-open
        m.Filter(must=[no_year], should=[fc("document_type", m.MatchValue("10-K")),
                                         fc("ticker", m.MatchValue("T05"))]),              # is-empty
        m.Filter(must=[year(gte=2025.5, lte=2025.5)]),                                     # five rows
        m.Filter(must=[year(gt=9999)]),                                                    # no row
    ]
    progs = [compile_program(pt, f, pr) for f in flts]
    # an empty interval (lo > hi) as the kernel meets it, OR a ticker: the ticker's rows alone
    t3 = pt.codes[0]["T03"]
    lo = pr.interval("fiscal_year", m.Range(gte=2023))[1]
    hi = pr.interval("fiscal_year", m.Range(lte=2020))[2]
    assert lo > hi
    progs.append(TR.P([("range", 0, lo, hi), ("maskeq", 0xFFFF, t3)], 0b1110))
    flts.append(m.Filter(must=[fc("ticker", m.MatchValue("T03"))]))
    blob = pack_view(progs)
    keys = c["keys"][:1]
    view = eval_view_np(blob, c["tags"], keys=keys)
    for s, f in enumerate(flts):
        want = np.array([matches_range(f, p, kinds) for p in c["pay"]])
        np.testing.assert_array_equal((view >> s) & 1, want)
    assert int(((view >> 4) & 1).sum()) == 5 and not ((view >> 5) & 1).any()
    slot, filt = view_filt(40, len(progs))
    return dict(c, keys=keys, blob=blob, view=view, slot=slot, filt=filt, U=len(progs),
                kinds=kinds, oracle={})


@pytest.fixture(scope="module")
def range_indexes(gpu):
    made = {}

    def get(n_cols):
        if n_cols not in made:
            c = range_world(n_cols)
            made[n_cols] = make_index(gpu, c["x"], c["tags"], c["keys"])
            assert made[n_cols].keys_cols() == n_cols
        return made[n_cols]
    yield get
    for idx in made.values():
        idx.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n_cols", [1, 4])
def test_range_views(gpu, range_indexes, n_cols, k):
    c = range_world(n_cols)
    idx = range_indexes(n_cols)
    q, filt, slot = c["q"], c["filt"], c["slot"]
    B = len(q)

    def run():
        return (lists(idx.search(q, k, filters=filt, programs=c["blob"])),
                unpacked(idx.search_packed(q, k, filters=filt, id_offset=OFFSET,
                                           programs=c["blob"])))
    (got, got_p), moved = both_modes([idx], run)
    assert moved == [2 * passes(B)]                                          # (c)
    if n_cols == 4:
        s, i = TR.oracle_lists(c, "fp16", k)
        want = (bits(s), i)
    else:
        want = oracle(O.encode_rows(c["x"]), q, k, c["view"], filt)
    same(got, want)                                                          # (d)
    same(got_p, (want[0], np.where(want[1] >= 0, want[1] + OFFSET, -1)))
    none, five = (8, 7) if n_cols == 4 else (5, 4)
    assert (got[1][slot == none] == -1).all()
    assert ((got[1][slot == five] >= 0).sum(axis=1) == min(k, 5)).all()
    assert idx.unanswered() == 0


# ----------------------------------------------------- 5. fallback tiers under a view, packed
def tier_case(name):
    """(x, queries, n_near, tags): test_select_band_gpu's near-duplicate geometries with a tag
    that splits the cluster between the values 1 and 2"""
    if name == "dup100":                 # 100 rows, all near-duplicates
        x, q, rows = SB._cluster(np.random.default_rng(3), 100, D, 100, 8, 4, rows=np.arange(100))
        n_near = 8
    elif name == "saturated":            # every other row of SAT_N a near-duplicate
        rng = np.random.default_rng(43)
        n = SB.SAT_N
        base = rng.standard_normal((1, D)).astype(np.float32)
        x = rng.standard_normal((n, D)).astype(np.float32)
        rows = np.arange(0, n, 2)
        x[rows] = base + 1e-5 * rng.standard_normal((n // 2, D)).astype(np.float32)
        q = np.concatenate([base + 0.02 * rng.standard_normal((6, D)).astype(np.float32),
                            rng.standard_normal((2, D)).astype(np.float32)])
        n_near = 6
    else:                                # 160 near-duplicates at random rows of 24 000
        x, q, rows = SB._cluster(np.random.default_rng(160), 24_000, D, 160, 24, 8)
        n_near = 24
    tags = np.random.default_rng(6).integers(1, 3, len(x)).astype(np.uint32)
    tags[rows] = 1 + (np.arange(len(rows)) % 2)
    return x, q, n_near, tags


@pytest.mark.parametrize("name,tier", [("dup100", None), ("saturated", 2), ("cluster160", 1)])
def test_fallback_tiers_under_a_view_and_packed(gpu, name, tier):
    """k = 15, query j filtered on tag value (1, 2, 9)[j % 3] (no row carries 9): once as lists
    over a view whose programs are those three values, once packed with an id offset over the
    tags. The tiers of the cluster queries that ask for 1 or 2, under mode 2:
      saturated   SAT_N = 512 rows, 256 near-duplicates, 128 per value: every one of the 32
                  sample tiles sees four cluster rows of either value, the seed stands above
                  L: tier 2 (asserted).
      cluster160  24 000 rows, 160 near-duplicates, 80 per value: tier 1 (asserted), as
                  test_select_band_gpu::test_filtered_band found for the tag filter.
      dup100      100 rows, all near-duplicates, 50 per value: the k-th and the 32nd best row
                  share the band, so tier >= 1 (asserted). Observed: tier 1 in both runs — a
                  list of 32 rows holds 16 of either value, so no list is full, where the
                  unfiltered corpus takes tier 2 (test_select_band_gpu).
    Observed on an MI355X, view lists and tag packed alike: dup100 1, saturated 2, cluster160 1;
    the queries that ask for 9 and the random ones 0.
    So the file certifies a cluster query by tier 1 and one by tier 2 in a filtered and in a
    view run."""
    from ragmi.filters import FilterProgram, pack_view
    x, q, n_near, tags = tier_case(name)
    B, k = len(q), 15
    values = (1, 2, 9)
    tag_f = np.array([[ALL, values[j % 3]] for j in range(B)], np.uint32)
    view_f = np.array([[1 << (j % 3)] * 2 for j in range(B)], np.uint32)
    blob = pack_view([FilterProgram.maskeq(ALL, v) for v in values])
    cluster = np.array([j for j in range(n_near) if j % 3 != 2])
    idx = make_index(gpu, x, tags)
    try:
        want = oracle(idx.export_rows(), q, k, tags, tag_f)
        seen = {}
        for how in ("view lists", "tag packed"):
            if how == "view lists":
                run = lambda: lists(idx.search(q, k, filters=view_f, programs=blob))
            else:
                run = lambda: unpacked(idx.search_packed(q, k, filters=tag_f, id_offset=OFFSET))
            got, moved = both_modes([idx], run)
            tiers = idx.exactness_stats(B)[2]          # the last pass: the mode-2 run
            assert moved == [passes(B)]                                      # (c)
            off = OFFSET if how == "tag packed" else 0
            same(got, (want[0], np.where(want[1] >= 0, want[1] + off, -1)))  # (d)
            assert (got[1][2::3] == -1).all()
            print(f"{name} {how}: tiers {tiers.tolist()}")
            seen[how] = tiers[cluster]
            if tier is None:
                assert (tiers[cluster] >= 1).all(), tiers
            else:
                assert (tiers[cluster] == tier).all(), tiers
        np.testing.assert_array_equal(seen["view lists"], seen["tag packed"])
        assert idx.unanswered() == 0
    finally:
        idx.close()


# ------------------------------------------------------------------------------ 6. tiny indexes
@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 33])
def test_tiny_indexes(gpu, n, B):
    """k > n padding, waves with no pair, the empty index; a filter every row passes and one no
    row passes, through the tag compare"""
    rng = np.random.default_rng(100 + n)
    x = rng.standard_normal((n, D)).astype(np.float32)
    tags = np.full(n, 3, np.uint32)
    q = np.concatenate([x[:min(n, B) // 2] + 0.05, rng.standard_normal((B, D))])[:B]
    q = q.astype(np.float32)
    enc = O.encode_rows(x)
    every = np.array([[ALL, 3]] * B, np.uint32)
    nothing = np.array([[ALL, 4]] * B, np.uint32)
    idx = make_index(gpu, x, tags)
    try:
        assert idx.count == n
        for k in KS:
            for filt in (None, every, nothing):
                def run():
                    return (lists(idx.search(q, k, filters=filt)),
                            unpacked(idx.search_packed(q, k, filters=filt, id_offset=OFFSET)))
                (got, got_p), moved = both_modes([idx], run)
                assert moved == [2 * passes(B)]                              # (c)
                want = oracle(enc, q, k, tags, filt)
                same(got, want)                                              # (d)
                same(got_p, (want[0], np.where(want[1] >= 0, want[1] + OFFSET, -1)))
                m = 0 if filt is nothing else min(n, k)
                assert ((got[1] >= 0).sum(axis=1) == m).all() and (got[1][:, m:] == -1).all()
    finally:
        idx.close()


# ------------------------------------------------------------------------------ 7. scan order 2
@pytest.mark.parametrize("k", KS)
def test_scan_order_2_on_two_streams(gpu, idx0, k):
    c = world()
    filt = tag_filters(64, c["pt"])
    jobs = [(c["q"][:32], None), (c["q"][32:64], filt[32:64]), (c["q"][16:48], filt[:32]),
            (c["q"][38:70], None)]
    streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
    cur = torch.cuda.current_stream(gpu)

    def run():
        outs = []
        for j, (q, f) in enumerate(jobs):
            streams[j % 2].wait_stream(cur)
            with torch.cuda.stream(streams[j % 2]):
                outs.append(idx0.search(q, k, filters=f))
        return [lists(o) for o in outs]

    default, moved = both_modes([idx0], lambda: [lists(idx0.search(q, k, filters=f))
                                                 for q, f in jobs])
    assert moved == [len(jobs) * passes(32)]                                 # (c)
    try:
        idx0.set_scan_order(2)
        got, moved = both_modes([idx0], run)
    finally:
        idx0.set_scan_order(0)
    assert moved == [len(jobs) * passes(32)]                                 # (c)
    same(got, default)
    same(got, [oracle(c["enc"], q, k, c["tags"], f) for q, f in jobs])       # (d)


# ------------------------------------------------------------------------------ 8. compositions
@pytest.mark.parametrize("diversity", [0.3, 0.8])
def test_search_mmr(gpu, idx0, diversity):
    c = world()
    B, k, C = 32, 10, 32
    q = c["q"][:B]
    for filt in (None, tag_filters(B, c["pt"])):
        got, moved = both_modes([idx0], lambda: lists(idx0.search_mmr(q, k, diversity, C, filt)))
        assert moved == [passes(B)]                                          # (c)
        s, r, _, _, cr = M.search_mmr(c["enc"], q, k, diversity, C, c["tags"], filt)
        same(got, (bits(s), r))                                              # (d)
        if filt is None:
            assert not np.array_equal(r, cr[:, :k])    # the re-selection is not the plain top-k


def test_search_groups_rungs_3_and_4(gpu):
    """the grouped corpus of _mmr_ref / _groups_ref (3001 rows, 12 near-duplicate groups, 56
    ticker keys); candidates = 32, S = 3, G = 60 with widen = 16 (below the candidates: widening
    cannot help), so the missing keys are asked directly (rung 3) and the groups the list cut
    short are re-answered (rung 4); every search of the ladder has k <= 32"""
    from ragmi import groups
    x, _, group = M.grouped_corpus(D)
    enc = O.encode_rows(x)
    tags = R.row_tags(x, group)
    Q = R.queries(D)
    mask, G, S = R.TICKER_MASK, 60, 3
    every = sorted({int(t) & mask for t in tags} - {0})
    filt = np.array([[R.DOCTYPE_MASK, 2 << 16], [R.TICKER_MASK, 4], [0, 0],
                     [R.TICKER_MASK | R.DOCTYPE_MASK, (3 << 16) | 16], [R.DOCTYPE_MASK, 3 << 16]],
                    np.uint32)
    idx = make_index(gpu, x, tags)
    try:
        for f in (None, filt):
            possible = [every] * len(Q) if f is None else \
                [[int(v) & mask] if int(m) & mask else every for m, v in f]
            calls = []

            def search(q, k, flt):
                calls.append((len(q), int(k)))
                return idx.search(q, k, flt)

            def run():
                del calls[:]
                stats = {}
                res = groups.search_groups(idx, Q, f, mask, possible, G, S, 32, 16,
                                           search=search, stats=stats)
                return ([[(key, [(r, fbits(s)) for r, s in h]) for key, h in per]
                         for per in res], stats, list(calls))
            (got, stats, made), moved = both_modes([idx], run)
            assert all(k <= 32 for _, k in made) and len(made) == 3
            assert moved == [sum(passes(b) for b, _ in made)]                # (c)
            assert stats["per_key"] > 0 and stats["filled"] > 0 and stats["widened"] == 0
            want = R.search_groups(enc, Q, tags, f, mask, G, S)
            assert got == [[(key, [(r, fbits(s)) for r, s in h]) for key, h in per]
                           for per in want]                                  # (d)
    finally:
        idx.close()


def test_fuse_rrf_over_two_searches(gpu, idx0):
    from ragmi.index import fuse_rrf
    c = world()
    B, k = 16, 25
    qa = c["q"][:B]
    qb = (qa + 0.3 * np.random.default_rng(5).standard_normal((B, D))).astype(np.float32)
    ncand = np.array([[20, 30]] * B, np.int32)

    def run():
        rows = torch.full((B, 2, 30), -1, dtype=torch.int64, device=gpu)
        rows[:, 0, :20] = idx0.search(qa, 20)[1]
        rows[:, 1] = idx0.search(qb, 30)[1]
        s, r, n = fuse_rrf(rows, k, 2, ncand, with_count=True)
        torch.cuda.synchronize()
        return lists((s, r)) + (n.cpu().numpy(),)
    got, moved = both_modes([idx0], run)
    assert moved == [2 * passes(B)]                                          # (c)
    rows = np.full((B, 2, 30), -1, np.int64)
    rows[:, 0, :20] = O.search(c["enc"], qa, 20)[1]
    rows[:, 1] = O.search(c["enc"], qb, 30)[1]
    s, r, n = F.rrf(rows, ncand, k, 2)
    same(got, (bits(s), r, n))                                               # (d)
    assert (n < 50).any()                              # the two lists share rows


# ------------------------------------------------------------------------------ 9. shard set
@pytest.mark.parametrize("k", KS)
def test_shard_set(gpu, k):
    """three logical shards over the 3017 rows (1006 + 1006 + 1005), every shard in mode 2:
    lists under tag filters and under view programs equal the single index, the oracle and
    gather_merge_np over the shards' own packed lists; again after remove_rows (rows cross the
    shards) and after an upsert that overwrites 32 rows"""
    from ragmi.shardset import ShardSet, gather_merge_np
    c = world()
    B = 40
    q = c["q"][:B]
    x, tags = c["x"].copy(), c["tags"].copy()
    tfilt = tag_filters(B, c["pt"])
    _, vfilt = view_filt(B, c["U"])
    sset = ShardSet(D, [gpu.index] * 3, N, "fp16")
    one = make_index(gpu, x, tags)
    try:
        sset.upsert(x, np.arange(N), tags, new_count=N)
        assert [s.count for s in sset.shards] == [1006, 1006, 1005]

        def check():
            from ragmi.filters import eval_view_np
            enc = O.encode_rows(x)
            view = eval_view_np(c["blob"], tags)

            def run_set():
                return (lists(sset.search(q, k, filters=tfilt)),
                        lists(sset.search(q, k, filters=vfilt, programs=c["blob"])))
            got, moved = both_modes(sset.shards, run_set)
            assert moved == [2 * passes(B)] * 3                              # (c) every shard
            same(got, (oracle(enc, q, k, tags, tfilt), oracle(enc, q, k, view, vfilt)))   # (d)

            def run_one():
                return (lists(one.search(q, k, filters=tfilt)),
                        lists(one.search(q, k, filters=vfilt, programs=c["blob"])))
            single, moved = both_modes([one], run_one)
            assert moved == [2 * passes(B)]                                  # (c)
            same(got, single)
            # the shards' own packed lists, merged on the host
            parts, moved = both_modes(sset.shards, lambda: [
                unpacked(s.search_packed(q, k, filters=tfilt)) for s in sset.shards])
            assert moved == [passes(B)] * 3                                  # (c)
            packed = [np.stack([p[0], p[1].astype(np.int32)], axis=-1) for p in parts]
            s, i, _ = gather_merge_np(packed, k, 3, [0, 1, 2])
            same(got[0], (bits(s), i))

        check()
        rng = np.random.default_rng(50 + k)
        gone = np.concatenate([rng.choice(N - 60, 40, replace=False), np.arange(N - 25, N - 15)])
        src, dst, n1 = sset.remove_rows(gone)
        assert len(src) > 0 and ((src % 3) != (dst % 3)).any() and n1 == N - 50
        one.remove_rows(gone)
        x[dst], tags[dst] = x[src], tags[src]
        x, tags = x[:n1].copy(), tags[:n1].copy()
        check()
        rows = np.sort(rng.choice(n1, 32, replace=False))
        fresh = (c["q"][:32] + 0.01 * rng.standard_normal((32, D))).astype(np.float32)
        ftags = np.full(32, int(tags[rows[0]]), np.uint32)
        sset.upsert(fresh, rows, ftags)
        one.upsert(fresh, rows, ftags)
        x[rows], tags[rows] = fresh, ftags
        check()
    finally:
        sset.close()
        one.close()


# ------------------------------------------------------------------------------ 10. front end
FN = 6000
TICKERS = ["AAPL", "MSFT", "NVDA", "AMZN", "GOOG", "META", "TSLA", "AMD"]
DOCS = ["10-K", "10-Q", "8-K"]
FKINDS = {"fiscal_year": "number", "ingested_at": "datetime"}


@functools.lru_cache(maxsize=None)
def front_world():
    """test_routes_gpu's collection (6000 points, 8 tickers x 3 document types) with a number
    and a datetime range field, and a fourth document type that two points carry"""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((FN, D)).astype(np.float32)
    t0 = dt.datetime(2023, 1, 1, tzinfo=dt.timezone.utc)
    pay = [{"ticker": TICKERS[i % 8], "document_type": DOCS[(i // 8) % 3], "text": f"chunk {i}",
            "fiscal_year": 2018 + (i // 24) % 7,
            "ingested_at": (t0 + dt.timedelta(hours=5 * i)).isoformat()} for i in range(FN)]
    pay[FN - 2]["document_type"] = pay[FN - 1]["document_type"] = "S-1"
    q = x[rng.choice(FN - 2, 14, replace=False)] + \
        0.05 * rng.standard_normal((14, D)).astype(np.float32)
    return x, pay, q.tolist()


def front_requests(m, q):
    """test_routes_gpu's request list, cut so that every search has k <= 32, with a Range and a
    DatetimeRange request"""
    def must(**kv):
        return m.Filter(must=[m.FieldCondition(key=k, match=m.MatchValue(value=v))
                              for k, v in kv.items()])
    general = m.Filter(
        must_not=[m.FieldCondition(key="document_type", match=m.MatchValue(value="8-K"))],
        must=[m.FieldCondition(key="ticker", match=m.MatchAny(any=["AAPL", "NVDA", "AMD"]))])
    years = m.Filter(must=[m.FieldCondition("fiscal_year", range=m.Range(gte=2020, lt=2022)),
                           m.FieldCondition(key="ticker", match=m.MatchValue(value="GOOG"))])
    since = m.Filter(must=[m.FieldCondition("ingested_at", range=m.DatetimeRange(
        gte="2024-01-01T00:00:00Z", lt="2025-01-01T00:00:00+09:00"))],
        must_not=[m.FieldCondition(key="document_type", match=m.MatchValue(value="10-Q"))])
    return [
        m.QueryRequest(query=q[0], limit=5),
        m.QueryRequest(query=q[1], limit=32),
        m.QueryRequest(query=q[2], limit=15, filter=must(ticker="MSFT", document_type="10-Q")),
        m.QueryRequest(query=q[3], limit=15, filter=general),
        m.QueryRequest(query=q[4], limit=15, filter=must(ticker="NEVER")),
        m.QueryRequest(query=q[5], limit=0),
        m.QueryRequest(query=m.NearestQuery(nearest=q[6], mmr=m.Mmr(diversity=0.3,
                                                                     candidates_limit=32)),
                       limit=10),
        m.QueryRequest(query=m.NearestQuery(nearest=q[7], mmr=m.Mmr(diversity=0.8,
                                                                     candidates_limit=30)),
                       limit=12, filter=general),
        m.QueryRequest(query=m.FusionQuery(fusion=m.Fusion.RRF), limit=10, prefetch=[
            m.Prefetch(query=q[8], filter=must(ticker="GOOG"), limit=20),
            m.Prefetch(query=q[9], filter=general, limit=30)]),
        m.QueryRequest(query=m.RrfQuery(rrf=m.Rrf(k=7)), limit=8, prefetch=[
            m.Prefetch(query=q[10], limit=25),
            m.Prefetch(query=q[8], filter=must(document_type="10-K"), limit=10)]),
        m.QueryRequest(query=q[11], limit=15, filter=years),
        m.QueryRequest(query=q[12], limit=20, filter=since),
    ]


def brute_lists(enc, pay, vec, flt, k):
    """exact top-k rows and scores over the payloads the plain evaluator lets through"""
    ok = np.array([flt is None or matches_range(flt, p, FKINDS) for p in pay], np.uint32)
    s, i = O.search(enc, np.asarray(vec, np.float32).reshape(1, -1), k, tags=ok, mask=1, value=1,
                    use_filter=True)
    return s, i


def brute_answer(m, enc, ids, pay, r):
    """[(id, score bits, payload)] of request `r` by brute force over the collection's current
    rows (stored rows `enc`, their point ids and payloads): oracle_scan for the lists, _mmr_ref
    / _fusion_ref for the compositions"""
    n = len(ids)
    if r.prefetch is not None:
        pres = r.prefetch
        C = max(min(p.limit, n) for p in pres)
        rows = np.full((1, len(pres), C), -1, np.int64)
        for l, p in enumerate(pres):
            rows[0, l, :min(p.limit, n)] = brute_lists(enc, pay, p.query, p.filter,
                                                       min(p.limit, n))[1][0]
        rrf_k = 2 if isinstance(r.query, m.FusionQuery) else r.query.rrf.k
        s, i, _ = F.rrf(rows, np.array([[min(p.limit, n) for p in pres]]), r.limit, rrf_k)
    elif isinstance(r.query, m.NearestQuery):
        C = min(r.query.mmr.candidates_limit, n)
        cs, cr = brute_lists(enc, pay, r.query.nearest, r.filter, C)
        s, i, _ = M.mmr(enc, cs, cr, r.limit, r.query.mmr.diversity, [C])
    elif r.limit < 1:
        return []
    else:
        s, i = brute_lists(enc, pay, r.query, r.filter, min(r.limit, n))
    return [(int(ids[row]), fbits(sc), pay[row]) for row, sc in zip(i[0], s[0]) if row >= 0]


def brute_groups(enc, ids, pay, vec, group_by, G, S):
    """the definition of a grouped query: the walk over the whole ranked list"""
    s, i = O.search(enc, np.asarray(vec, np.float32).reshape(1, -1), len(ids))
    found = {}
    for row, sc in zip(i[0], s[0]):
        key = pay[row].get(group_by)
        if key is None or (key not in found and len(found) >= G):
            continue
        hits = found.setdefault(key, [])
        if len(hits) < S:
            hits.append((int(ids[row]), fbits(sc), pay[row]))
    return list(found.items())


def triples(points):
    return [(p.id, fbits(p.score), p.payload) for p in points]


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one", "two"])
def test_front_end_over_float16_collections(gpu, devices):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    x, pay, q = front_world()
    cl = QdrantClient(url="http://unused", device=gpu, devices=devices)
    try:
        cl.create_collection("c", m.VectorParams(size=D, distance=m.Distance.COSINE,
                                                 datatype="float16"),
                             capacity=FN, payload_range_fields=FKINDS)
        cl.upsert("c", m.Batch(ids=list(range(FN)), vectors=x, payloads=pay))
        col = cl._collections["c"]
        assert col.index.storage == "fp16"
        handles = [col.index] if devices is None else list(col.index.shards)
        reqs = front_requests(m, q)

        def run():
            batch = [triples(b.points) for b in cl.query_batch_points("c", reqs)]
            alone = [triples(cl.query_points("c", query=r.query, limit=r.limit,
                                             query_filter=r.filter, prefetch=r.prefetch).points)
                     for r in reqs]
            assert batch == alone
            return batch

        def run_groups():
            res = cl.query_points_groups("c", query=q[13], group_by="document_type", limit=4,
                                         group_size=3)
            return [(g.id, triples(g.hits)) for g in res.groups]

        def check():
            ids = np.asarray(col.row_ids)
            enc, rows_pay = O.encode_rows(x[ids]), col.payloads
            got, moved = both_modes(handles, run)
            assert all(n > 0 for n in moved), moved                          # (c)
            assert got == [brute_answer(m, enc, ids, rows_pay, r) for r in reqs]   # (d)
            assert [len(a) for a in got][4:6] == [0, 0] and all(got[j] for j in (0, 1, 2, 3, 6, 7, 8,
                                                                                 9, 10, 11))
            # the two S-1 points rank outside the first hundred: their group is asked directly,
            # one k = 3 search (rung 3 of the ladder)
            grp, moved = both_modes(handles, run_groups)
            assert all(n > 0 for n in moved), moved                          # (c)
            assert grp == brute_groups(enc, ids, rows_pay, q[13], "document_type", 4, 3)   # (d)
            assert [g for g, _ in grp][-1] == "S-1" and len(grp) == 4

        check()
        rng = np.random.default_rng(3)
        cl.delete("c", rng.choice(FN - 2, 100, replace=False).tolist())
        assert len(col.row_ids) == FN - 100
        check()
    finally:
        cl.close()
