"""GPU tests of grouped search (rag_index_gather_tags, rag_group_select / group_select_kernel,
ragmi.groups over FlatIndex and ShardSet, QdrantClient.query_points_groups): keys, fills, rows,
positions and counts equal and scores bit-equal to the numpy restatement tests/_groups_ref.py on
the 3001-row corpus of near-duplicate groups under the two-field tag recipe."""
import functools

import numpy as np
import pytest
import torch

import _groups_ref as R
import _mmr_ref as M

pytestmark = pytest.mark.gpu

MASKS = (R.TICKER_MASK, R.DOCTYPE_MASK)
GS = ((4, 3), (1, 1), (12, 1), (1, 40), (1024, 4))
CONFIGS = ((R.TICKER_MASK, 4, 3), (R.DOCTYPE_MASK, 3, 3), (R.TICKER_MASK, 60, 2))


@functools.lru_cache(maxsize=None)
def world(D, storage):
    """(stored rows, tags, queries, the whole ranked lists) — computed once per (D, storage)."""
    x, _, group = M.grouped_corpus(D)
    enc = M.encode(x, storage)
    tags = R.row_tags(x, group)
    Q = R.queries(D)
    return enc, tags, Q, R.ranked(enc, Q, tags)


_indexes = {}


def index_of(gpu, D, storage, shards=0):
    from ragmi.index import FlatIndex
    from ragmi.shardset import ShardSet
    key = (D, storage, shards)
    if key not in _indexes:
        x = M.grouped_corpus(D)[0]
        tags = world(D, storage)[1]
        idx = (ShardSet(D, [gpu.index] * shards, len(x), storage) if shards else
               FlatIndex(D, len(x), gpu, storage=storage))
        idx.upsert(x, np.arange(len(x)), tags, new_count=len(x))
        _indexes[key] = idx
    return _indexes[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_selection(sel, want):
    """A GroupSelection against the restatement's (keys, fill, scores, rows, pos, count)."""
    torch.cuda.synchronize()
    k, fill, s, r, p, count = want
    assert np.array_equal(sel.count.cpu().numpy(), count)
    assert np.array_equal(sel.keys.cpu().numpy().view(np.uint32), k)
    assert np.array_equal(sel.fill.cpu().numpy(), fill)
    assert np.array_equal(sel.rows.cpu().numpy(), r)
    assert np.array_equal(sel.pos.cpu().numpy(), p)
    assert np.array_equal(bits(sel.scores.cpu().numpy()), bits(s))


def possible(tags, key_mask, filters=None, B=R.N_QUERIES):
    every = sorted({int(t) & key_mask for t in tags} - {0})
    if filters is None:
        return [every] * B
    return [[int(v) & key_mask] if int(m) & key_mask else every for m, v in filters]


def hits_bits(res):
    return [[(k, [(r, int(np.float32(s).view(np.uint32))) for r, s in h]) for k, h in q]
            for q in res]


FILT = np.array([[R.DOCTYPE_MASK, 2 << 16], [R.TICKER_MASK, 4], [0, 0],
                 [R.TICKER_MASK | R.DOCTYPE_MASK, (3 << 16) | 16], [R.DOCTYPE_MASK, 3 << 16]],
                np.uint32)


# ------------------------------------------------------------------ 1. the select kernel
@pytest.mark.parametrize("D,storage", [(384, "fp16"), (1024, "fp32")])
def test_group_select_matches_the_restatement(gpu, D, storage):
    idx = index_of(gpu, D, storage)
    enc, tags, Q, (ref_s, ref_r) = world(D, storage)
    # gather_tags: the rows' tags, 0 outside [0, capacity), nothing dereferenced there
    rows = np.array([[0, 3000, -1, idx.capacity], [17, idx.capacity + 5, 1 << 40, -(1 << 40)]])
    got = idx.gather_tags(rows).cpu().numpy().view(np.uint32)
    ok = (rows >= 0) & (rows < len(tags))
    assert np.array_equal(got, np.where(ok, tags[np.where(ok, rows, 0)], 0))
    assert idx.gather_tags(np.empty((0, 4), np.int64)).shape == (0, 4)
    # C = 600 passes the workgroup's 512 threads: a second trip, a ragged ncand, one n_b = 0
    for C, ncand in ((100, None), (1, None), (600, (600, 513, 0, 37, 512))):
        cs, cr = idx.search(Q, C)
        torch.cuda.synchronize()
        assert np.array_equal(cr.cpu().numpy(), ref_r[:, :C])
        assert np.array_equal(bits(cs.cpu().numpy()), bits(ref_s[:, :C]))
        ct = tags[ref_r[:, :C]]
        for mask in MASKS:
            for G, S in GS:
                want = R.select(ref_s[:, :C], ref_r[:, :C], ct, ncand, mask, G, S)
                same_selection(idx.group_select(cs, cr, mask, G, S, ncand, with_pos=True), want)
        if C == 600:
            assert want[5][:, 1].tolist() == [600, 513, 0, 37, 512] and want[5][2, 0] == 0
        if C == 100:
            # a list cut by a -1 in the middle ends there; no positions asked for
            cut = cr.clone()
            cut[1, 40] = -1
            cut[3, 0] = -1
            cut_np = cut.cpu().numpy()
            want = R.select(ref_s[:, :C], cut_np, ct, None, R.TICKER_MASK, 4, 3)
            assert want[5][:, 1].tolist() == [100, 40, 100, 0, 100]
            sel = idx.group_select(cs, cut, R.TICKER_MASK, 4, 3)
            assert sel.pos is None
            same_selection(sel._replace(pos=torch.as_tensor(want[4])), want)
    with pytest.raises(ValueError):
        idx.group_select(cs, cr, 0, 4, 3)
    with pytest.raises(ValueError):
        idx.group_select(cs, cr, 0xFFFF, 1025, 1)
    with pytest.raises(ValueError):
        idx.group_select(cs, cr, 0xFFFF, 64, 65)


# ------------------------------------------------------------------ 2. the ladder on a FlatIndex
def test_ladder_equals_the_definition(gpu):
    from ragmi import groups
    idx = index_of(gpu, 384, "fp16")
    enc, tags, Q, lists = world(384, "fp16")
    R.assert_recipe_cases(enc, Q, tags, lists)     # the short lists, cut groups and ties below
    total = {"widened": 0, "per_key": 0, "filled": 0}
    for mask, G, S in CONFIGS:
        want = hits_bits(R.search_groups(enc, Q, tags, None, mask, G, S, lists))
        want_f = hits_bits(R.search_groups(enc, Q, tags, FILT, mask, G, S))
        for candidates in (8, 100):
            for widen in (16, None):
                stats = {}
                got = groups.search_groups(idx, Q, None, mask, possible(tags, mask), G, S,
                                           candidates, widen, stats=stats)
                assert hits_bits(got) == want, (mask, G, S, candidates, widen)
                got = groups.search_groups(idx, Q, FILT, mask, possible(tags, mask, FILT), G, S,
                                           candidates, widen, stats=stats)
                assert hits_bits(got) == want_f, (mask, G, S, candidates, widen)
                for name in total:
                    total[name] += stats[name]
                if (mask, G, candidates, widen) == (R.TICKER_MASK, 4, 8, 16):
                    assert stats["widened"] > 0 and stats["filled"] > 0
        if mask == R.TICKER_MASK and G == 4:
            assert [k for k, _ in want_f[1]] == [4] and [k for k, _ in want_f[3]] == [16]
            # a group cut short by the list at C = 8 is re-answered by a filtered search: its
            # first hits are the ones first found, bit for bit (canonical scores on every route)
            s8, r8 = idx.search(Q, 8)
            sel = idx.group_select(s8, r8, mask, G, S)
            torch.cuda.synchronize()
            keys, fill = sel.keys.cpu().numpy().view(np.uint32), sel.fill.cpu().numpy()
            hs, hr = sel.scores.cpu().numpy(), sel.rows.cpu().numpy()
            cut = 0
            for b in range(len(Q)):
                final = dict(want[b])
                for g in range(int(sel.count[b, 0])):
                    n = int(fill[b, g])
                    first = [(int(hr[b, g, i]), int(hs[b, g, i].view(np.uint32))) for i in range(n)]
                    assert final[int(keys[b, g])][:n] == first
                    cut += len(final[int(keys[b, g])]) > n
            assert cut > 0
    assert all(v > 0 for v in total.values()), total                   # every route ran
    assert groups.search_groups(idx, Q, None, R.TICKER_MASK, possible(tags, R.TICKER_MASK), 4, 3,
                                stats=total) == \
        groups.search_groups(idx, torch.as_tensor(Q, device=gpu), None, R.TICKER_MASK,
                             possible(tags, R.TICKER_MASK), 4, 3, 3001)


# ------------------------------------------------------------------ 3. shard set
def test_shardset_equals_the_flat_index(gpu):
    from ragmi import groups
    flat = index_of(gpu, 384, "fp16")
    sset = index_of(gpu, 384, "fp16", shards=3)
    enc, tags, Q, (ref_s, ref_r) = world(384, "fp16")
    rows = np.array([[0, 1, 2, 3000, -1, sset.capacity, 2999, 1 << 40]])
    assert torch.equal(sset.gather_tags(rows), flat.gather_tags(rows).to(sset.device))
    assert np.array_equal(sset.gather_tags(ref_r[:, :600]).cpu().numpy().view(np.uint32),
                          tags[ref_r[:, :600]])
    cs, cr = sset.search(Q, 600)
    ncand = (600, 513, 0, 37, 512)
    for mask in MASKS:
        for G, S in ((4, 3), (1024, 4)):
            a = sset.group_select(cs, cr, mask, G, S, ncand, with_pos=True)
            b = flat.group_select(cs, cr, mask, G, S, ncand, with_pos=True)
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            same_selection(a, R.select(ref_s[:, :600], ref_r[:, :600], tags[ref_r[:, :600]],
                                       ncand, mask, G, S))
    for mask, G, S in CONFIGS:
        want = hits_bits(R.search_groups(enc, Q, tags, FILT, mask, G, S))
        for candidates, widen in ((8, 16), (100, None)):
            got = [groups.search_groups(i, Q, FILT, mask, possible(tags, mask, FILT), G, S,
                                        candidates, widen) for i in (flat, sset)]
            assert got[0] == got[1] and hits_bits(got[1]) == want


# ------------------------------------------------------------------ 4. QdrantClient parity
def make_client(gpu, devices=None):
    from ragmi import qdrant_models as m
    from ragmi.qdrant import QdrantClient
    x = M.grouped_corpus(384)[0]
    tags = world(384, "fp32")[1]
    c = QdrantClient(device=gpu, devices=devices)
    c.create_collection("t", m.VectorParams(size=384, distance=m.Distance.COSINE),
                        capacity=len(x))
    c.upsert("t", m.Batch(ids=list(range(len(x))), vectors=x,
                          payloads=[R.payload_of(int(tags[i]), i) for i in range(len(x))]))
    return c


def field_filter(key, value):
    from ragmi import qdrant_models as m
    return m.Filter(must=[m.FieldCondition(key=key, match=m.MatchValue(value=value))])


def value_of(mask, key):
    return f"T{key:02d}" if mask == R.TICKER_MASK else R.DOC_TYPES[(key >> 16) - 1]


def expected_groups(enc, ids_of_row, q, mask, G, S, filt=None, with_payload=True):
    """[(group id, [(point id, score, payload)])] the client must report: the definition over
    stored rows `enc`, whose row r holds point ids_of_row[r] (its tag: the recipe's for that id)."""
    ids_of_row = np.asarray(ids_of_row)
    tags = world(384, "fp32")[1][ids_of_row]
    found = R.search_groups(enc, q[None], tags, None if filt is None else [filt], mask, G, S)[0]
    return [(value_of(mask, key),
             [(int(ids_of_row[r]), s, R.payload_of(int(tags[r]), ids_of_row[r]) if with_payload
               else None) for r, s in hits]) for key, hits in found]


def reported(res):
    return [(g.id, [(p.id, p.score, p.payload) for p in g.hits]) for g in res.groups]


def test_client_parity_single_and_sharded(gpu):
    from ragmi import qdrant_models as m
    enc, tags, Q, _ = world(384, "fp32")                 # VectorParams' default datatype
    ids = np.arange(len(enc))
    q = Q[0]
    single = make_client(gpu)
    sharded = make_client(gpu, devices=[gpu.index] * 3)
    try:
        by_ticker = expected_groups(enc, ids, q, R.TICKER_MASK, 10, 3)
        assert len(by_ticker) == 10 and by_ticker[0][0] == "T55" and len(by_ticker[0][1]) == 2
        k10 = expected_groups(enc, ids, q, R.TICKER_MASK, 6, 2, (R.DOCTYPE_MASK, 1 << 16))
        assert len(k10) == 6 and all(p["document_type"] == "10-K" for _, h in k10 for _, _, p in h)
        by_doc = expected_groups(enc, ids, q, R.DOCTYPE_MASK, 5, 4, (R.TICKER_MASK, 16))
        assert [len(h) for _, h in by_doc] == [2, 1] and {g for g, _ in by_doc} == {"10-Q", "8-K"}
        bare = expected_groups(enc, ids, q, R.TICKER_MASK, 10, 3, with_payload=False)
        for c in (single, sharded):
            assert reported(c.query_points_groups("t", q, group_by="ticker", limit=10,
                                                  group_size=3)) == by_ticker
            assert reported(c.query_points_groups(
                "t", m.NearestQuery(nearest=q.tolist()), group_by="ticker", limit=6, group_size=2,
                query_filter=field_filter("document_type", "10-K"))) == k10
            assert reported(c.query_points_groups(
                "t", torch.as_tensor(q), group_by="document_type", limit=5, group_size=4,
                query_filter=field_filter("ticker", "T16"))) == by_doc
            assert reported(c.query_points_groups("t", q, group_by="ticker", limit=10,
                                                  group_size=3, with_payload=False)) == bare
            legacy = c.search_groups("t", q, "ticker", limit=10, group_size=3)
            assert isinstance(legacy, m.GroupsResult) and reported(legacy) == by_ticker
            assert isinstance(legacy.groups[0], m.PointGroup) and legacy.groups[0].lookup is None
    finally:
        single.close()
        sharded.close()


# ------------------------------------------------------------------ 5. after a delete
def test_groups_after_deleting_keys(gpu):
    enc, tags, Q, _ = world(384, "fp32")
    q = Q[0]
    t16 = np.nonzero((tags & R.TICKER_MASK) == 16)[0]
    for devices in (None, [gpu.index] * 3):
        c = make_client(gpu, devices)
        try:
            c.delete("t", field_filter("document_type", "8-K"))       # one whole key's points
            c.delete("t", field_filter("ticker", "T55"))              # another whole key
            c.delete("t", [int(t16[0])])                              # part of a third
            col = c._col("t")
            ids_of_row = np.asarray(col.row_ids)
            assert 1900 < len(ids_of_row) < 2100 and (ids_of_row != np.arange(len(ids_of_row))).any()
            after = np.ascontiguousarray(enc[ids_of_row])             # rows moved bit for bit
            want = expected_groups(after, ids_of_row, q, R.DOCTYPE_MASK, 3, 3)
            assert [g for g, _ in want] and "8-K" not in [g for g, _ in want] and len(want) == 2
            assert "8-K" in col.tags.codes[1]                         # still a possible key
            got = c.query_points_groups("t", q, group_by="document_type", limit=3, group_size=3)
            assert reported(got) == want
            assert col.group_stats["per_key"] > 0                     # asked, and it has no rows
            want = expected_groups(after, ids_of_row, q, R.TICKER_MASK, 10, 3)
            assert "T55" not in [g for g, _ in want]
            assert int(t16[0]) not in [i for g, h in want if g == "T16" for i, _, _ in h]
            assert reported(c.query_points_groups("t", q, group_by="ticker", limit=10,
                                                  group_size=3)) == want
        finally:
            c.close()
