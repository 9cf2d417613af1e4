"""CPU tests of grouped search: the restated walk against a brute-force statement of the
kernel's parallel form, the exactness ladder (ragmi.groups) over a numpy stand-in index against
the definition, the two C calls' argument refusals (no device), PayloadTags.value_of, and
QdrantClient.query_points_groups' argument checks."""
import collections
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import ROOT

import _groups_ref as R
import _mmr_ref as M
import _stubs as S
import oracle_scan as O
from ragmi import groups

RAG_EINVAL, RAG_ERANGE = -1, -4
Sel = collections.namedtuple("Sel", "keys fill scores rows pos count")


# ------------------------------------------------------------------ 1. walk = parallel form
def parallel_form(rows, tags, ncand, key_mask, G, S):
    """The kernel's statement, by brute force: a candidate is a group's first if no earlier
    candidate has its key; the group index of a key is the number of earlier firsts; the rank of
    a candidate is the number of earlier candidates with its key; emit iff key != 0, group index
    < G and rank < S. Returns {(b, group, rank): position} and the (groups, n_b) counts."""
    B, C = rows.shape
    cells, counts = {}, []
    for b in range(B):
        bad = [j for j in range(C) if rows[b, j] < 0]
        n = min(C if ncand is None else min(max(int(ncand[b]), 0), C), bad[0] if bad else C)
        key = [int(tags[b, j]) & key_mask for j in range(n)]
        first = [key[j] != 0 and key[j] not in key[:j] for j in range(n)]
        for j in range(n):
            if key[j] == 0:
                continue
            f = key.index(key[j])
            g, rank = sum(first[:f]), key[:j].count(key[j])
            if g < G and rank < S:
                cells[(b, g, rank)] = j
        counts.append((min(sum(first), G), n))
    return cells, counts


@pytest.mark.parametrize("C,G,S,nkeys", [(1, 1, 1, 3), (37, 4, 3, 6), (64, 1, 1, 2), (50, 12, 1, 20),
                                        (90, 1, 40, 3), (200, 1024, 4, 70), (33, 5, 2, 0)])
def test_walk_equals_the_parallel_form(C, G, S, nkeys):
    rng = np.random.default_rng(C * 1000 + G)
    B = 6
    for key_mask, shift in ((R.TICKER_MASK, 0), (R.DOCTYPE_MASK, 16)):
        keys = rng.integers(0, nkeys + 1, (B, C)).astype(np.uint32)       # 0: no group
        other = rng.integers(0, 5, (B, C)).astype(np.uint32)              # the other field
        tags = (keys << shift) | (other << (16 - shift))
        rows = rng.permutation(B * C).reshape(B, C).astype(np.int64)
        scores = -np.sort(-rng.standard_normal((B, C)).astype(np.float32), axis=1)
        ncand = np.array([C, C // 2, 0, C + 5, -3, 1])                    # ragged, 0, clamped
        rows[3, C // 3] = -1                                              # a cut in the middle
        for nc in (None, ncand):
            k, fill, s, r, p, count = R.select(scores, rows, tags, nc, key_mask, G, S)
            cells, counts = parallel_form(rows, tags, nc, key_mask, G, S)
            assert count.tolist() == [list(c) for c in counts]
            want_p = np.full((B, G, S), -1, np.int32)
            for (b, g, rank), j in cells.items():
                want_p[b, g, rank] = j
            assert np.array_equal(p, want_p)
            assert np.array_equal(fill, (want_p >= 0).sum(axis=2))
            for b in range(B):
                for g in range(G):
                    j = want_p[b, g, 0]
                    assert k[b, g] == (int(tags[b, j]) & key_mask if j >= 0 else 0)
            ok = want_p >= 0
            bi = np.nonzero(ok)[0]
            assert np.array_equal(r[ok], rows[bi, want_p[ok]]) and (r[~ok] == -1).all()
            assert np.array_equal(s[ok].view(np.uint32), scores[bi, want_p[ok]].view(np.uint32))
            assert np.isneginf(s[~ok]).all()
    if nkeys == 0:
        assert count[:, 0].tolist() == [0] * B and (fill == 0).all()      # all keys 0


# ------------------------------------------------------------------ 2. the ladder, numpy index
class FakeIndex:
    """numpy stand-in: search is the oracle, group_select the restated walk."""

    def __init__(self, enc, tags):
        self.enc, self.tags, self.count = enc, np.asarray(tags, np.uint32), len(enc)
        self.calls = []

    def search(self, q, k, filters=None):
        q = np.ascontiguousarray(q, np.float32)
        self.calls.append((len(q), k))
        s = np.empty((len(q), k), np.float32)
        r = np.empty((len(q), k), np.int64)
        for b in range(len(q)):
            m, v = (0, 0) if filters is None else (int(filters[b][0]), int(filters[b][1]))
            s[b], r[b] = [a[0] for a in O.search(self.enc, q[b:b + 1], k, tags=self.tags, mask=m,
                                                 value=v, use_filter=True)]
        return s, r

    def group_select(self, s, r, key_mask, G, S, ncand=None, with_pos=False):
        tags = np.where(r >= 0, self.tags[np.maximum(r, 0)], 0)
        k, fill, os_, or_, op, count = R.select(s, r, tags, ncand, key_mask, G, S)
        return Sel(k, fill, os_, or_, op, count)


@pytest.fixture(scope="module")
def world():
    x, _, group = M.grouped_corpus(384)
    enc = M.encode(x, "fp16")
    tags = R.row_tags(x, group)
    Q = R.queries(384)
    return enc, tags, Q, R.ranked(enc, Q, tags)


def possible(tags, key_mask, filters=None, B=R.N_QUERIES):
    every = sorted({int(t) & key_mask for t in tags} - {0})
    if filters is None:
        return [every] * B
    return [[int(v) & key_mask] if int(m) & key_mask else every for m, v in filters]


def hits_bits(res):
    return [[(k, [(r, np.float32(s).view(np.uint32)) for r, s in h]) for k, h in q] for q in res]


def test_recipe_gives_every_case(world):
    """(a)-(e) of the corpus recipe, asserted on the reference alone."""
    enc, tags, Q, lists = world
    R.assert_recipe_cases(enc, Q, tags, lists)


@pytest.mark.parametrize("widen", [16, 3001])
@pytest.mark.parametrize("candidates", [1, 8, 100, 3001])
def test_ladder_gives_the_definition(world, candidates, widen):
    enc, tags, Q, lists = world
    idx = FakeIndex(enc, tags)
    for mask, G, S in ((R.TICKER_MASK, 4, 3), (R.DOCTYPE_MASK, 3, 3), (R.TICKER_MASK, 60, 2)):
        stats = {}
        got = groups.search_groups(idx, Q, None, mask, possible(tags, mask), G, S, candidates,
                                   widen, stats=stats)
        want = R.search_groups(enc, Q, tags, None, mask, G, S, lists)
        assert hits_bits(got) == hits_bits(want)
        if candidates == 3001:
            assert stats == {"widened": 0, "per_key": 0, "filled": 0}      # one search, final
        elif candidates <= 8 and mask == R.TICKER_MASK and G == 4:
            assert stats["widened"] > 0                                    # (a): 56 keys possible
            assert stats["filled"] > 0 or widen == 3001                    # (b), (c)
        elif candidates == 1 and mask == R.DOCTYPE_MASK:
            assert stats["per_key"] > 0 and stats["widened"] == 0          # 3 keys: asked directly
        elif G == 60 and candidates <= 100 and widen == 16:
            assert stats["per_key"] > 0                                    # widening cannot help
    # per-query filters: the other field, the grouped field itself (one group), none
    filt = np.array([[R.DOCTYPE_MASK, 2 << 16], [R.TICKER_MASK, 4], [0, 0],
                     [R.TICKER_MASK | R.DOCTYPE_MASK, (3 << 16) | 16], [R.DOCTYPE_MASK, 3 << 16]],
                    np.uint32)
    want = R.search_groups(enc, Q, tags, filt, R.TICKER_MASK, 4, 3)
    got = groups.search_groups(idx, Q, filt, R.TICKER_MASK, possible(tags, R.TICKER_MASK, filt),
                               4, 3, candidates, widen)
    assert hits_bits(got) == hits_bits(want)
    assert [k for k, _ in want[1]] == [4] and [k for k, _ in want[3]] == [16]


def test_ladder_batches_its_rungs(world):
    """One search per rung: C1, widen, the per-key queries, the under-full groups."""
    enc, tags, Q, _ = world
    idx = FakeIndex(enc, tags)
    stats = {}
    groups.search_groups(idx, Q, None, R.TICKER_MASK, possible(tags, R.TICKER_MASK), 4, 3, 8, 16,
                         stats=stats)
    assert [k for _, k in idx.calls] == [8, 16, 3, 3][:len(idx.calls)] and len(idx.calls) <= 4
    assert idx.calls[0] == (5, 8) and idx.calls[1] == (stats["widened"], 16)
    assert groups.default_candidates(10, 3) == 100 and groups.default_candidates(10, 15) == 300
    empty = FakeIndex(enc[:0], tags[:0])
    assert groups.search_groups(empty, Q, None, 0xFFFF, [[1]] * 5, 4, 3) == [[]] * 5


# ------------------------------------------------------------------ 3. argument refusals
def test_argument_errors_need_no_device():
    from ragmi import _build, _lib
    _build.build()
    L = _lib.load()
    assert {"rag_group_select", "rag_index_gather_tags"} <= set(_lib.INDEX_API)
    assert len(_lib.INDEX_API["rag_group_select"][1]) == 16
    assert len(_lib.INDEX_API["rag_index_gather_tags"][1]) == 5
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)

    def call(B=1, C=8, mask=0xFFFF, G=4, S=3, inp=p, out=p, count=p):
        return L.rag_group_select(inp, inp, inp, None, B, C, mask, G, S, out, out, out, out, None,
                                  count, None)

    for kw, code, word in (({"C": 0}, RAG_ERANGE, b"C must be"), ({"C": 4097}, RAG_ERANGE, b"4096"),
                           ({"C": -1}, RAG_ERANGE, b"C must be"),
                           ({"G": 0}, RAG_ERANGE, b"G must be"), ({"G": 1025}, RAG_ERANGE, b"1024"),
                           ({"S": 0}, RAG_ERANGE, b"S must be"),
                           ({"G": 1024, "S": 5}, RAG_ERANGE, b"G * S"),
                           ({"G": 1, "S": 4097}, RAG_ERANGE, b"G * S"),
                           ({"mask": 0}, RAG_EINVAL, b"key_mask"),
                           ({"B": -1}, RAG_EINVAL, b"B must be"),
                           ({"inp": None}, RAG_EINVAL, b"NULL"), ({"out": None}, RAG_EINVAL, b"NULL"),
                           ({"count": None}, RAG_EINVAL, b"NULL")):
        assert call(**kw) == code and word in L.rag_last_error(), kw
    assert call(B=0, inp=None, out=None, count=None) == 0                  # launches nothing
    assert L.rag_index_gather_tags(None, p, -1, p, None) == RAG_EINVAL and b"n must" in L.rag_last_error()
    assert L.rag_index_gather_tags(None, None, 4, p, None) == RAG_EINVAL and b"NULL rows" in L.rag_last_error()
    assert L.rag_index_gather_tags(None, p, 4, None, None) == RAG_EINVAL and b"NULL rows" in L.rag_last_error()
    assert L.rag_index_gather_tags(None, p, 4, p, None) == RAG_EINVAL and b"index is NULL" in L.rag_last_error()
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    for line in ("#define RAG_GROUPS_MAX_CANDIDATES 4096", "#define RAG_GROUPS_MAX 1024",
                 "int rag_group_select(", "int rag_index_gather_tags("):
        assert line in hdr
    assert "rag_group_select" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ------------------------------------------------------------------ 4. value_of
def test_value_of_round_trips_also_through_the_store():
    from ragmi.qdrant import PayloadTags
    t = PayloadTags()
    values = ["AMD", "AAPL", 7, "MSFT", ""]
    for v in values:
        t.tag({"ticker": v, "document_type": "10-K" if v == "AMD" else "10-Q"})
    t.tag({"ticker": ["a", "list"], "document_type": None})               # not coded
    for f, vals in ((0, values), (1, ["10-K", "10-Q"])):
        for v in vals:
            assert t.value_of(f, t.code(f, v, create=False)) == v
    for bad in (0, 6, -1):
        with pytest.raises(KeyError):
            t.value_of(0, bad)
    # the codebooks as ragmi.store writes and reads them (collection.json)
    saved = json.loads(json.dumps({"codebooks": [[[v, c] for v, c in b.items()] for b in t.codes]}))
    back = PayloadTags()
    for f_i, book in enumerate(saved["codebooks"]):
        back.codes[f_i] = {v: int(c) for v, c in book}
    for f in (0, 1):
        for v, c in t.codes[f].items():
            assert back.value_of(f, c) == v
    src = open(os.path.join(ROOT, "financial-rag-system_amd", "ragmi", "store.py")).read()
    assert '"codebooks": [[[v, c] for v, c in t.items()] for t in col.tags.codes]' in src
    assert "col.tags.codes[f_i] = {v: int(c) for v, c in book}" in src


# ------------------------------------------------------------------ 5. client argument checks
class _StubIndex:
    device = None

    def __init__(self, count):
        self.count = count
        self.calls = []

    def search(self, q, k, filters=None, full=False, rescue=False):
        import torch
        self.calls.append(("search", len(q), k))
        return (torch.linspace(0.9, 0.1, k).repeat(len(q), 1),
                torch.arange(k, dtype=torch.int64).repeat(len(q), 1))

    def unanswered(self):
        return 0

    def group_select(self, s, r, key_mask, G, S, ncand=None, with_pos=False):
        self.calls.append(("group_select", tuple(s.shape), key_mask, G, S))
        tags = np.asarray([[1 + (int(x) % 2) for x in row] for row in r.numpy()], np.uint32)
        return Sel(*R.select(s.numpy(), r.numpy(), tags, ncand, key_mask, G, S))


def stub_client(count=40):
    return S.stub_client(S.stub_collection(
        _StubIndex(count), dim=4, ids=range(100, 100 + count),
        payloads=[{"ticker": "AMD" if r % 2 else "AAPL", "n": r} for r in range(count)]))


def test_query_points_groups_argument_checks_and_routing():
    from ragmi import qdrant_models as m
    from ragmi.qdrant import UnsupportedFilter
    client, col = stub_client()
    v = [0.0, 1.0, 0.0, 0.0]
    with pytest.raises(UnsupportedFilter, match="payload_tag_fields"):
        client.query_points_groups("t", v, group_by="n")
    with pytest.raises(ValueError, match="group_by"):
        client.query_points_groups("t", v)
    with pytest.raises(ValueError, match="MMR"):
        client.query_points_groups("t", m.NearestQuery(nearest=v, mmr=m.Mmr()), group_by="ticker")
    with pytest.raises(NotImplementedError, match="with_lookup"):
        client.query_points_groups("t", v, group_by="ticker", with_lookup="other")
    big, big_col = stub_client(5000)
    with pytest.raises(ValueError, match="4096"):
        big.query_points_groups("t", v, group_by="ticker", limit=2, group_size=3000)
    assert big_col.index.calls == []
    assert col.index.calls == [] and col.coalescer.requests == 0
    res = client.query_points_groups("t", m.NearestQuery(nearest=v), group_by="ticker", limit=10,
                                     group_size=2)
    assert isinstance(res, m.GroupsResult) and col.coalescer.requests == 0
    # limit 10 clamps to the 2 tickers; candidates max(100, 2 * 2 * 2) clamps to the 40 points
    assert col.index.calls == [("search", 1, 40), ("group_select", (1, 40), 0xFFFF, 2, 2)]
    assert [g.id for g in res.groups] == ["AAPL", "AMD"]
    assert [[p.id for p in g.hits] for g in res.groups] == [[100, 102], [101, 103]]
    assert res.groups[0].hits[0].payload == {"ticker": "AAPL", "n": 0}
    assert res.groups[0] == m.PointGroup(hits=res.groups[0].hits, id="AAPL", lookup=None)
    legacy = client.search_groups("t", v, "ticker", limit=10, group_size=2, with_payload=False)
    assert [g.id for g in legacy.groups] == ["AAPL", "AMD"]
    assert all(p.payload is None for g in legacy.groups for p in g.hits)
    never = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="NONE"))])
    assert client.query_points_groups("t", v, group_by="ticker", query_filter=never).groups == []
    assert client.query_points_groups("t", v, group_by="ticker", limit=0).groups == []
