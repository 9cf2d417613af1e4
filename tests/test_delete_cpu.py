"""CPU tests of point deletion: the removal rule (plan_removal) against a plain list model, its
split over the shards of a set, the C ABI surface (header, bindings, argument errors that need
no device), the selector models, and Collection.delete's host bookkeeping over a stand-in
index."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import _stubs as S


# ------------------------------------------------------------------ 1. the removal rule
def model_removal(count, rows):
    """The rule restated over plain lists: (final list of original rows per slot, moves)."""
    D = set(int(r) for r in rows)
    n1 = count - len(D)
    holes = [r for r in range(n1) if r in D]
    movers = [r for r in range(n1, count) if r not in D]
    slots = list(range(count))
    for m, h in zip(movers, holes):
        slots[h] = m
    return slots[:n1], movers, holes, n1


def delete_sets(rng, count):
    """The named delete sets of the rule's corner cases, then random ones."""
    sets = [[]]
    if count:
        sets += [[count - 1], [0], list(range(count)),
                 rng.choice(count, count // 2 + 1, replace=False).tolist(),   # more than half
                 rng.choice(count, max(1, (7 * count) // 10), replace=False).tolist(),
                 rng.integers(0, count, 2 * count).tolist(),                   # duplicates
                 list(range(count // 3, count)),                               # a whole tail
                 list(range(0, count - count // 3))]                           # a whole head
        for _ in range(6):
            sets.append(rng.choice(count, rng.integers(0, count + 1), replace=False).tolist())
    return sets


def check_plan(count, rows):
    from ragmi.index import plan_removal
    src, dst, n1 = plan_removal(count, rows)
    final, movers, holes, n1_model = model_removal(count, rows)
    D = set(int(r) for r in rows)
    assert n1 == n1_model == count - len(D)
    assert src.dtype == dst.dtype == np.int64 and len(src) == len(dst) <= len(D)
    assert src.tolist() == movers and dst.tolist() == holes
    assert (np.diff(src) > 0).all() and (np.diff(dst) > 0).all()       # ascending, distinct
    assert (src >= n1).all() and (dst < n1).all() and (dst >= 0).all() and (src < count).all()
    assert not (set(src.tolist()) & D) and set(dst.tolist()) <= D
    # applying the moves to a list of the rows gives the model's result; survivors that are no
    # mover keep their slot
    slots = np.arange(count)
    slots[dst] = slots[src]
    assert slots[:n1].tolist() == final
    for r in range(n1):
        if r not in D:
            assert final[r] == r
    assert sorted(final) == sorted(set(range(count)) - D)
    if len(D) > count / 2 and count:
        assert any(r >= n1 for r in D)          # part of D lies in the tail: no hole there
    return src, dst, n1


def test_plan_removal_against_list_model():
    rng = np.random.default_rng(0)
    n_sets = 0
    for count in [0, 1, 2, 3, 15, 16, 17, 100, 3001] + rng.integers(1, 400, 12).tolist():
        for rows in delete_sets(rng, count):
            check_plan(count, rows)
            n_sets += 1
    assert n_sets > 200


def test_plan_removal_named_cases():
    from ragmi.index import plan_removal
    src, dst, n1 = plan_removal(10, [])
    assert (src.size, dst.size, n1) == (0, 0, 10)
    src, dst, n1 = plan_removal(10, [9])                    # the last row: nothing moves
    assert (src.size, dst.size, n1) == (0, 0, 9)
    src, dst, n1 = plan_removal(10, [0])                    # row 0: the last row takes its slot
    assert (src.tolist(), dst.tolist(), n1) == ([9], [0], 9)
    src, dst, n1 = plan_removal(10, range(10))              # every row
    assert (src.size, dst.size, n1) == (0, 0, 0)
    src, dst, n1 = plan_removal(10, [1, 8, 1, 3, 9, 8])     # duplicates collapse
    assert (src.tolist(), dst.tolist(), n1) == ([6, 7], [1, 3], 6)
    src, dst, n1 = plan_removal(10, [0, 1, 2, 3, 5, 7, 9])  # 7 of 10: holes 0..2, movers 4, 6, 8
    assert (src.tolist(), dst.tolist(), n1) == ([4, 6, 8], [0, 1, 2], 3)
    for bad in ([-1], [10], [3, 11]):
        with pytest.raises(IndexError):
            plan_removal(10, bad)


# ------------------------------------------------------------------ 2. the plan over shards
@pytest.mark.parametrize("n_shards", [1, 2, 3, 8])
def test_shard_moves_follow_the_stripes(n_shards):
    from ragmi.index import plan_removal
    from ragmi.shardset import local_of, shard_count, shard_moves, shard_of
    rng = np.random.default_rng(n_shards)
    for count in (0, 1, 7, 16, 100, 3001):
        for rows in delete_sets(rng, count):
            src, dst, n1 = plan_removal(count, rows)
            moves = shard_moves(src, dst, n_shards)
            # every pair appears once, under its (source shard, destination shard), in order
            want = {}
            for s, d in zip(src.tolist(), dst.tolist()):
                key = (shard_of(s, n_shards), shard_of(d, n_shards))
                a, b = want.setdefault(key, ([], []))
                a.append(local_of(s, n_shards))
                b.append(local_of(d, n_shards))
            assert set(moves) == set(want)
            for key, (ls, ld) in moves.items():
                assert ls.tolist() == want[key][0] and ld.tolist() == want[key][1]
                # sources lie at or past their shard's new count, destinations below theirs:
                # no pair reads a slot another pair writes
                assert (ls >= shard_count(n1, key[0], n_shards)).all()
                assert (ls < shard_count(count, key[0], n_shards)).all()
                assert (ld < shard_count(n1, key[1], n_shards)).all()
            assert sum(len(ls) for ls, _ in moves.values()) == len(src)
            assert sum(shard_count(n1, s, n_shards) for s in range(n_shards)) == n1
            # the rows each shard holds afterwards, from a model of the stripes
            slots = np.arange(count)
            slots[dst] = slots[src]
            for s in range(n_shards):
                assert len(slots[:n1][s::n_shards]) == shard_count(n1, s, n_shards)


# ------------------------------------------------------------------ 3. header, bindings, errors
NEW = ("rag_index_select_rows", "rag_index_move_rows", "rag_index_gather_rows",
       "rag_index_scatter_rows")


def test_header_declares_and_bindings_bind_the_four():
    from ragmi import _lib
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(rf"^int {name}\(rag_index_t\* index,", code, re.M), name
        assert name in _lib.INDEX_API
    assert "disjoint" in hdr                                     # move_rows' precondition
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integration


def test_argument_errors_need_no_device():
    from ragmi import _build, _lib
    _build.build()
    L = _lib.load()
    n = ctypes.c_int64()
    p = ctypes.addressof(n)
    assert L.rag_index_select_rows(None, 0, 0, None, 0, p, None) == -1
    assert b"NULL" in L.rag_last_error()
    assert L.rag_index_move_rows(None, p, p, 1, 0, None) == -1
    assert L.rag_index_move_rows(None, None, None, 0, 0, None) == -1
    assert L.rag_index_move_rows(None, p, p, 1, -1, None) == -1
    assert L.rag_index_gather_rows(None, p, 1, p, None, p, None) == -1
    assert L.rag_index_scatter_rows(None, p, 1, p, None, p, 1, None) == -1
    assert L.rag_index_scatter_rows(None, None, 1, None, None, None, 1, None) == -1
    assert b"NULL" in L.rag_last_error()


# ------------------------------------------------------------------ 4. selectors
def test_selector_models_round_trip():
    from ragmi import qdrant_models as m
    from ragmi.qdrant import _norm_id, parse_selector
    md5 = "0123456789abcdef0123456789abcdef"
    ids = [7, md5, 7]
    want = [7, _norm_id(md5), 7]
    assert parse_selector(ids) == ("ids", want)
    assert parse_selector(tuple(ids)) == ("ids", want)
    assert parse_selector(m.PointIdsList(points=ids)) == ("ids", want)
    assert parse_selector(m.PointIdsList(points=[])) == ("ids", [])
    flt = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    assert parse_selector(m.FilterSelector(filter=flt)) == ("filter", flt)
    assert parse_selector(flt) == ("filter", flt)
    assert m.FilterSelector(filter=flt).filter is flt and m.PointIdsList(points=ids).points == ids
    for bad in (m.FilterSelector(), "abc", 5, {"points": [1]}, None):
        with pytest.raises(ValueError):
            parse_selector(bad)
    with pytest.raises(ValueError):
        parse_selector([-1])                       # ids go through _norm_id
    with pytest.raises(ValueError):
        parse_selector(["not-a-uuid"])


# ------------------------------------------------------------------ 5. Collection.delete, host side
class _StubIndex:
    """FlatIndex stand-in holding one integer per row: remove_rows is the real plan applied to
    it, select_rows a numpy selection over the tags."""

    class _Rows:
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    device = None

    def __init__(self):
        self.val = np.empty(0, np.int64)
        self.tag = np.empty(0, np.uint32)
        self.capacity = 1 << 20
        self.selects = 0

    @property
    def count(self):
        return len(self.val)

    def upsert(self, vectors, rows, tags, new_count):
        grow = new_count - len(self.val)
        self.val = np.concatenate([self.val, np.zeros(grow, np.int64)])
        self.tag = np.concatenate([self.tag, np.zeros(grow, np.uint32)])
        self.val[rows] = np.asarray(vectors)[:, 0].astype(np.int64)
        self.tag[rows] = tags

    def select_rows(self, mask, value, cap=None):
        self.selects += 1
        rows = np.nonzero((self.tag & np.uint32(mask)) == np.uint32(value))[0].astype(np.int64)
        return self._Rows(rows if cap is None else rows[:cap]), len(rows)

    def remove_rows(self, rows):
        from ragmi.index import plan_removal
        src, dst, n1 = plan_removal(self.count, rows)
        self.val[dst] = self.val[src]
        self.tag[dst] = self.tag[src]
        self.val, self.tag = self.val[:n1], self.tag[:n1]
        return src, dst, n1


def stub_collection(monkeypatch):
    import torch

    class _NoStream:
        def synchronize(self):
            pass

    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _NoStream())
    return S.stub_collection(_StubIndex(), dim=2)


def consistent(col, alive):
    """Every map agrees: ids <-> rows, payloads and the index's own row values."""
    assert sorted(col.row_ids) == sorted(alive)
    assert len(col.row_ids) == len(col.payloads) == len(col.versions) == col.index.count
    assert len(col.id_to_row) == len(col.row_ids)
    for r, pid in enumerate(col.row_ids):
        assert col.id_to_row[pid] == r
        assert col.payloads[r]["n"] == pid and col.index.val[r] == pid
        assert col.index.tag[r] == col.tags.tag(col.payloads[r])


def test_collection_delete_keeps_the_host_maps_in_step(monkeypatch):
    from ragmi import qdrant_models as m
    col = stub_collection(monkeypatch)
    tick = ["AAPL", "MSFT", "AMD"]
    n = 50
    ids = list(range(n))
    col.upsert(ids, np.array([[i, 0] for i in ids], np.float32),
               [{"ticker": tick[i % 3], "document_type": "10-K" if i % 2 else "10-Q", "n": i}
                for i in ids])
    versions = dict(zip(col.row_ids, col.versions))
    alive = set(ids)
    op = col.delete([3, 3, 49, 1000, 17])                        # duplicates, an unknown id
    alive -= {3, 49, 17}
    assert op == 2
    consistent(col, alive)
    assert col.index.selects == 0                                # ids need no device select
    amd = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    assert col.count_matching(amd) == len([i for i in alive if i % 3 == 2])
    col.delete(m.FilterSelector(filter=amd))
    alive -= {i for i in ids if i % 3 == 2}
    consistent(col, alive)
    assert col.count_matching(amd) == 0
    both = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AAPL")),
                          m.FieldCondition(key="document_type", match=m.MatchValue(value="10-K"))])
    col.delete(both)
    alive -= {i for i in ids if i % 3 == 0 and i % 2}
    consistent(col, alive)
    before = (list(col.row_ids), col.index.selects)
    col.delete(m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="NONE"))]))
    col.delete(m.PointIdsList(points=[]))
    assert (list(col.row_ids), col.index.selects) == before      # nothing matched, no select
    assert all(col.versions[r] == versions[pid] for r, pid in enumerate(col.row_ids))
    from ragmi.qdrant import UnsupportedFilter
    with pytest.raises(UnsupportedFilter):
        col.delete(m.Filter(must_not=[m.FieldCondition(key="ticker",
                                                       match=m.MatchValue(value="AMD"))]))
    col.delete(m.Filter())                                       # no condition: every point
    consistent(col, set())
    col.upsert([5], np.array([[5, 0]], np.float32), [{"ticker": "AMD", "n": 5}])
    consistent(col, {5})
