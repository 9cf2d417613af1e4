"""numpy / Python restatement of reciprocal rank fusion (rag_fuse_rrf; include/ragmi.h, DESIGN
§R10) and the seeded corpus its tests share. TEST HELPER ONLY, used by test_fusion_cpu.py and
test_fusion_gpu.py.

The arithmetic, as pinned: an entry at 0-based position p contributes 1.0 / (rrf_k + p) (one
fp64 division, Python floats); a row's contributions are added in (list ascending, position
ascending) order from 0.0 and the sum is rounded once to fp32 (np.float32); the distinct rows are
ordered by (fused fp32 value descending, row ascending).
"""
import functools

import numpy as np

import oracle_scan as O

N_ROWS, DIM, N_VARIANTS, LIST_LEN = 3001, 384, 3, 50
TICKERS = ("AAA", "BBB")


def list_lengths(cand_rows, ncand):
    """n[b][l] = min(ncand clamped to [0, C], the number of leading entries with row >= 0)."""
    cand_rows = np.asarray(cand_rows, np.int64)
    B, L, C = cand_rows.shape
    n = np.empty((B, L), np.int64)
    for b in range(B):
        for l in range(L):
            bad = np.nonzero(cand_rows[b, l] < 0)[0]
            lim = C if ncand is None else min(max(int(np.asarray(ncand)[b][l]), 0), C)
            n[b, l] = min(lim, int(bad[0]) if bad.size else C)
    return n


def rrf(cand_rows, ncand, k: int, rrf_k: int = 2):
    """Fusion of candidate lists cand_rows int64 [B, L, C] (-1 = none), ncand [B, L] or None.
    Returns (scores fp32 [B, k], rows int64 [B, k], count int32 [B]): -inf / -1 past the last
    distinct row; count = the number of distinct rows (may exceed k)."""
    cand_rows = np.asarray(cand_rows, np.int64)
    B, L, C = cand_rows.shape
    n = list_lengths(cand_rows, ncand)
    out_s = np.full((B, k), -np.inf, np.float32)
    out_r = np.full((B, k), -1, np.int64)
    count = np.zeros(B, np.int32)
    for b in range(B):
        total = {}
        for l in range(L):
            for p in range(int(n[b, l])):
                r = int(cand_rows[b, l, p])
                total[r] = total.get(r, 0.0) + 1.0 / float(rrf_k + p)
        fused = sorted(((np.float32(v), r) for r, v in total.items()),
                       key=lambda e: (-float(e[0]), e[1]))
        count[b] = len(fused)
        for t, (v, r) in enumerate(fused[:k]):
            out_s[b, t], out_r[b, t] = v, r
    return out_s, out_r, count


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def fusion_corpus():
    """The seed-11 corpus: 3001 rows (not a multiple of the 16-row tile), D = 384, tickers
    alternating between two values by row; three query variants (a question and two rewrites:
    the same direction under independent noise), whose top-50 lists overlap in part. Checked
    here, on the CPU oracle's lists over the fp16 stored rows: some rows are in all three
    lists, some in exactly one, and at least one pair of rows ties exactly in the fused score.
    Returns (x fp32 [3001, 384], Q fp32 [3, 384], ticker of each row)."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    base = x[rng.choice(N_ROWS, 40, replace=False)].sum(axis=0)
    Q = (base[None] + 4.0 * rng.standard_normal((N_VARIANTS, DIM))).astype(np.float32)
    tickers = [TICKERS[i % 2] for i in range(N_ROWS)]
    rows = np.stack([O.search(O.encode_rows(x), Q[v:v + 1], LIST_LEN)[1][0]
                     for v in range(N_VARIANTS)])
    seen = {}
    for v in range(N_VARIANTS):
        for r in rows[v]:
            seen[int(r)] = seen.get(int(r), 0) + 1
    assert sum(c == N_VARIANTS for c in seen.values()) >= 3, "no rows shared by all lists"
    assert sum(c == 1 for c in seen.values()) >= 3, "no rows in exactly one list"
    s, r, count = rrf(rows[None], None, N_VARIANTS * LIST_LEN)
    live = bits(s[0, :count[0]])
    assert count[0] == len(seen) and (live[1:] == live[:-1]).any(), "no exact fused tie"
    return x, Q, tickers
