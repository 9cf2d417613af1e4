"""CPU tests of the shard set's host side (ragmi.shardset): striped row placement, the
`devices` / RAGMI_DEVICES parsing, the numpy restatement of the gather-merge, and the C
argument errors, which are rejected before any HIP call."""
import ctypes

import numpy as np
import pytest

from ragmi import shardset as S


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_placement_round_trips(n):
    for count in range(51):
        g = np.arange(count, dtype=np.int64)
        sh, lo = S.shard_of(g, n), S.local_of(g, n)
        np.testing.assert_array_equal(S.global_of(lo, sh, n), g)
        counts = [S.shard_count(count, s, n) for s in range(n)]
        assert sum(counts) == count
        for s in range(n):
            mine = g[sh == s]
            assert counts[s] == len(mine)
            # local rows of a shard are 0 .. count-1 in global order (local order = global order)
            np.testing.assert_array_equal(lo[sh == s], np.arange(len(mine)))
            np.testing.assert_array_equal(S.global_of(np.arange(len(mine)), s, n), mine)
        # scalar forms agree
        for r in range(count):
            assert S.global_of(S.local_of(r, n), S.shard_of(r, n), n) == r


def test_parse_devices():
    assert S.parse_devices(None) is None
    assert S.parse_devices("") is None and S.parse_devices("  ") is None
    assert S.parse_devices("0,1,2,3") == [0, 1, 2, 3]
    assert S.parse_devices(" 2 , 0 ") == [2, 0]
    assert S.parse_devices([0, 0, 0]) == [0, 0, 0]
    assert S.parse_devices((1, np.int64(3))) == [1, 3]
    assert S.parse_devices("all", device_count=4) == [0, 1, 2, 3]
    assert S.parse_devices("ALL", device_count=1) == [0]
    for bad in ("0,x", "0;1", [], [-1], [0.5], [True], "-1", list(range(65))):
        with pytest.raises(ValueError):
            S.parse_devices(bad)
    with pytest.raises(ValueError):
        S.parse_devices("0,4", device_count=4)
    with pytest.raises(ValueError):
        S.parse_devices("all", device_count=0)


def test_rag_reads_ragmi_devices(monkeypatch):
    """get_qdrant() hands RAGMI_DEVICES to QdrantClient(devices=...), which parses it."""
    from ragmi import qdrant, rag
    seen = {}

    class Fake:
        def __init__(self, url=None, path=None, devices=None):
            seen.update(path=path, devices=S.parse_devices(devices, device_count=8))

    monkeypatch.setattr(qdrant, "QdrantClient", Fake)
    monkeypatch.delenv("TESTING", raising=False)
    monkeypatch.setattr(rag, "_testing", lambda: False)
    for env, want in (("0,1,2,3", [0, 1, 2, 3]), ("all", list(range(8))), ("", None)):
        rag.get_qdrant.cache_clear()
        monkeypatch.setenv("RAGMI_DEVICES", env)
        rag.get_qdrant()
        assert seen["devices"] == want
    rag.get_qdrant.cache_clear()
    monkeypatch.delenv("RAGMI_DEVICES")
    rag.get_qdrant()
    assert seen["devices"] is None
    rag.get_qdrant.cache_clear()


def random_lists(rng, n, B, k, n_scores=6):
    """n packed lists [B, k, 2], each sorted by (score desc, local row asc) with -1 padding;
    few distinct scores, so ties span lists and the mapped id decides; some lists empty."""
    scores = rng.standard_normal(n_scores).astype(np.float32)
    lists = []
    for l in range(n):
        a = np.full((B, k, 2), -1, np.int32)
        for b in range(B):
            m = int(rng.integers(0, k + 1)) if rng.random() > 0.2 else 0
            rows = np.sort(rng.choice(4 * k + 8, m, replace=False)).astype(np.int32)
            sc = scores[rng.integers(0, n_scores, m)]
            order = np.lexsort((rows, -sc.astype(np.float64)))
            a[b, :m, 0] = sc[order].view(np.int32)
            a[b, :m, 1] = rows[order]
        lists.append(a)
    return lists


@pytest.mark.parametrize("n,B,k", [(1, 1, 1), (2, 3, 15), (3, 2, 33), (8, 2, 100), (64, 1, 7)])
def test_gather_merge_np_against_brute_force(n, B, k):
    rng = np.random.default_rng(n * 1000 + k)
    lists = random_lists(rng, n, B, k)
    add = list(range(n))
    s, ids, empty = S.gather_merge_np(lists, k, n, add)
    for b in range(B):
        union = []
        for l, a in enumerate(lists):
            for bits, row in a[b]:
                if row >= 0:
                    union.append((-float(np.int32(bits).view(np.float32)), int(row) * n + add[l]))
            assert empty[l, b] == (a[b, 0, 1] < 0)
        union.sort()
        union = union[:k]
        assert ids[b, :len(union)].tolist() == [g for _, g in union]
        assert s[b, :len(union)].tolist() == [-x for x, _ in union]
        assert (ids[b, len(union):] == -1).all() and np.isneginf(s[b, len(union):]).all()
        assert len(set(g for _, g in union)) == len(union)     # striped ids never collide


def test_c_argument_errors_need_no_device():
    from ragmi import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    one = (_lib.c_vp * 1)(None)
    assert L.rag_shardset_create(None, 1, ctypes.byref(h)) == -1
    assert L.rag_shardset_create(one, 1, None) == -1
    assert L.rag_shardset_create(one, 0, ctypes.byref(h)) == -1
    assert L.rag_shardset_create(one, 65, ctypes.byref(h)) == -1
    assert b"RAG_MAX_SHARDS" in L.rag_last_error()
    assert L.rag_shardset_create(one, 1, ctypes.byref(h)) == -1       # a NULL shard handle
    assert b"NULL" in L.rag_last_error()
    assert L.rag_shardset_search(None, None, 1, 15, None, 0, None, None, None, None) == -1
    assert L.rag_shardset_destroy(None) == 0
    add = (ctypes.c_int64 * 1)(0)
    assert L.rag_merge_topk_gather(None, 1, 1, 15, 1, add, None, None, None, None) == -1
    assert L.rag_merge_topk_gather(one, 0, 1, 15, 1, add, None, None, None, None) == -1
    assert L.rag_merge_topk_gather(one, 65, 1, 15, 1, add, None, None, None, None) == -1
    assert L.rag_merge_topk_gather(one, 1, 1, 0, 1, add, None, None, None, None) == -1
    assert L.rag_merge_topk_gather(one, 1, 1, 15, 1, None, None, None, None, None) == -1
