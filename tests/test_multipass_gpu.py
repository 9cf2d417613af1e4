"""Searches of more queries than one pass holds, with per-query filters: the host loop cuts the
queries, the filters and every output form into passes (32 queries at dim 384, 128 at dim 1024)
and each pass must read and write its own slice. 70 filtered queries at dim 384 make passes of
32, 32 and 6 on the scan path (k = 5), the large-k path (k = 40), the full exact pass and the
packed exchange form with a global id offset; 150 unfiltered queries at dim 1024 make passes of
128 and 22. Ids and scores equal the oracle's (oracle/scan_ref.c) bit for bit, query by query.
"""
import functools

import numpy as np
import pytest
import torch

import oracle_scan as O

pytestmark = pytest.mark.gpu

N, DIM, B = 3000, 384, 70
ID_OFFSET = 1000


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(70)
    x = rng.standard_normal((N, DIM)).astype(np.float32)
    tags = rng.integers(1, 5, N).astype(np.uint32)              # 4 tag values
    q = rng.standard_normal((B, DIM)).astype(np.float32)
    filters = np.stack([np.full(B, 0xffffffff, np.uint32),
                        rng.integers(1, 5, B).astype(np.uint32)], axis=1)
    filters[[0, 31, 32, 45, 64, 69]] = 0                        # mask 0: no filter for these
    return x, tags, q, filters


@functools.lru_cache(maxsize=None)
def _reference(k):
    """The oracle's top-k, one call per query with that query's filter."""
    x, tags, q, filters = _data()
    x16 = O.encode_rows(x)
    s = np.empty((B, k), np.float32)
    i = np.empty((B, k), np.int64)
    for b, (mask, value) in enumerate(filters):
        sb, ib = O.search(x16, q[b:b + 1], k, tags=tags, mask=int(mask), value=int(value),
                          use_filter=mask != 0)
        s[b], i[b] = sb[0], ib[0]
    s.setflags(write=False)
    i.setflags(write=False)
    return s, i


@pytest.fixture(scope="module")
def index(gpu):
    from ragmi.index import FlatIndex
    x, tags, _, _ = _data()
    idx = FlatIndex(dim=DIM, capacity=N, device=gpu)
    idx.upsert(x, np.arange(N, dtype=np.int64), tags, new_count=N)
    yield idx
    idx.close()


@pytest.mark.parametrize("k,full", [(5, False), (40, False), (40, True)],
                         ids=["scan_k5", "large_k40", "full_k40"])
def test_filtered_queries_over_three_passes(index, k, full):
    _, _, q, filters = _data()
    s, i = index.search(q, k, filters=filters, full=full)
    torch.cuda.synchronize()
    want_s, want_i = _reference(k)
    np.testing.assert_array_equal(i.cpu().numpy(), want_i)
    np.testing.assert_array_equal(s.cpu().numpy().view(np.int32), want_s.view(np.int32))


def test_packed_with_id_offset_over_three_passes(index):
    _, _, q, filters = _data()
    p = index.search_packed(q, 5, filters=filters, id_offset=ID_OFFSET)
    torch.cuda.synchronize()
    p = p.cpu().numpy()                                         # [B, k, 2] (score bits, id)
    want_s, want_i = _reference(5)
    np.testing.assert_array_equal(p[..., 1].astype(np.int64),
                                  np.where(want_i >= 0, want_i + ID_OFFSET, -1))
    np.testing.assert_array_equal(p[..., 0], want_s.view(np.int32))


def test_wide_rows_unfiltered_over_two_passes(gpu):
    """dim 1024: one pass holds 128 queries (four groups of 32); 150 make passes of 128 and 22."""
    from ragmi.index import FlatIndex
    rng = np.random.default_rng(150)
    n, dim, b, k = 500, 1024, 150, 5
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((b, dim)).astype(np.float32)
    idx = FlatIndex(dim=dim, capacity=n, device=gpu)
    idx.upsert(x, np.arange(n, dtype=np.int64), None, new_count=n)
    s, i = idx.search(q, k)
    torch.cuda.synchronize()
    want_s, want_i = O.search(O.encode_rows(x), q, k)
    np.testing.assert_array_equal(i.cpu().numpy(), want_i)
    np.testing.assert_array_equal(s.cpu().numpy().view(np.int32), want_s.view(np.int32))
    idx.close()
