"""numpy restatement of grouped search (rag_group_select, ragmi.groups; include/ragmi.h, DESIGN
§R8), built on the CPU oracle. `select` is the sequential walk over candidate lists; `search_groups`
is the definition itself: oracle_scan.search at k = every row, then the walk over the whole
ranked list — it never sees a candidate count, so it is independent of the ladder. TEST HELPER
ONLY, shared by test_groups_cpu.py and test_groups_gpu.py; also the tag recipe both use over
_mmr_ref.grouped_corpus (12 groups of near-duplicate rows among 3001).
"""
import numpy as np

import _mmr_ref as M
import oracle_scan as O

TICKER_MASK, DOCTYPE_MASK = 0xFFFF, 0xFFFF0000
RARE = 55                 # a ticker code held by two rows only
TIE = 56                  # TIE, TIE + 1: ticker codes of bit-identical rows
DOC_TYPES = ("10-K", "10-Q", "8-K")
N_QUERIES = 5


def row_tags(x, group, rare_group: int = 3, tie_group: int = 5):
    """The tag recipe over both fields, a pure function of the row number, of the row's
    near-duplicate group (`group[r]`, -1 = none; j = the row's rank among its group's rows) and
    of which rows of input x are copies of one another:
      ticker (low 16 bits)   grouped rows: code 1 + g, but 13 + g where j % 3 == 2, and absent
                             (0) where j == 4;
                             the rows j = 0, 1 of group `rare_group`: code RARE, two rows in all;
                             the identical rows of group `tie_group`: codes TIE and TIE + 1 in
                             turn, held by no other row — two groups whose best hits are
                             bit-identical rows, so the score tie decides their order by row;
                             other rows: 25 + r % 30, absent where r % 7 == 0
      document_type (high)   1 + r % 3, absent where r % 11 == 0."""
    group = np.asarray(group)
    n = len(group)
    tick = np.zeros(n, np.uint32)
    seen = {}
    for r in range(n):
        g = int(group[r])
        if g < 0:
            tick[r] = 0 if r % 7 == 0 else 25 + r % 30
            continue
        j = seen.get(g, 0)
        seen[g] = j + 1
        if g == rare_group and j < 2:
            tick[r] = RARE
        elif j == 4:
            tick[r] = 0
        else:
            tick[r] = 13 + g if j % 3 == 2 else 1 + g
    rows = np.nonzero(group == tie_group)[0]
    copies = [r for r in rows if sum(np.array_equal(x[r], x[o]) for o in rows) > 1]
    for i, r in enumerate(copies):
        tick[r] = TIE + i % 2
    r = np.arange(n)
    doc = np.where(r % 11 == 0, 0, 1 + r % 3).astype(np.uint32)
    return tick | (doc << 16)


def payload_of(tag: int, n: int):
    """The payload whose PayloadTags tag is `tag` when the values are first seen in code order."""
    p = {"n": int(n)}
    if tag & 0xFFFF:
        p["ticker"] = f"T{tag & 0xFFFF:02d}"
    if tag >> 16:
        p["document_type"] = DOC_TYPES[(tag >> 16) - 1]
    return p


def queries(D: int):
    """Five queries over grouped_corpus(D): its own query, two perturbations of it, and two near
    corpus rows."""
    x, q, _ = M.grouped_corpus(D)
    rng = np.random.default_rng(11)
    return np.stack([q, q + 0.5 * rng.standard_normal(D), q + 1.0 * rng.standard_normal(D),
                     x[5] + 0.1 * rng.standard_normal(D), x[1500]]).astype(np.float32)


def walk(scores, rows, tags, n: int, key_mask: int, G: int, S: int):
    """The sequential walk over the first n entries of one list: [[key, [positions]], ...]."""
    groups, at = [], {}
    for j in range(n):
        key = int(tags[j]) & key_mask
        if key == 0:
            continue
        if key not in at:
            if len(groups) >= G:
                continue
            at[key] = len(groups)
            groups.append([key, []])
        hits = groups[at[key]][1]
        if len(hits) < S:
            hits.append(j)
    return groups


def select(scores, rows, tags, ncand, key_mask: int, G: int, S: int):
    """rag_group_select restated: (keys uint32 [B, G], fill int32 [B, G], scores fp32 [B, G, S],
    rows int64 [B, G, S], positions int32 [B, G, S], count int32 [B, 2])."""
    scores = np.asarray(scores, np.float32)
    rows = np.asarray(rows, np.int64)
    tags = np.asarray(tags).astype(np.uint32)
    B, C = rows.shape
    nc = np.full(B, C) if ncand is None else np.broadcast_to(np.asarray(ncand), (B,))
    keys = np.zeros((B, G), np.uint32)
    fill = np.zeros((B, G), np.int32)
    out_s = np.full((B, G, S), -np.inf, np.float32)
    out_r = np.full((B, G, S), -1, np.int64)
    out_p = np.full((B, G, S), -1, np.int32)
    count = np.zeros((B, 2), np.int32)
    for b in range(B):
        bad = np.nonzero(rows[b] < 0)[0]
        n = int(min(max(int(nc[b]), 0), C, bad[0] if bad.size else C))
        found = walk(scores[b], rows[b], tags[b], n, key_mask, G, S)
        count[b] = (len(found), n)
        for g, (key, pos) in enumerate(found):
            keys[b, g], fill[b, g] = key, len(pos)
            out_s[b, g, :len(pos)] = scores[b, pos]
            out_r[b, g, :len(pos)] = rows[b, pos]
            out_p[b, g, :len(pos)] = pos
    return keys, fill, out_s, out_r, out_p, count


def ranked(enc, q, tags, filters=None):
    """The whole ranked lists: oracle_scan.search at k = every row, per query under its own
    filter (mask, value). (scores [B, N], rows [B, N]), -1 past the matching rows."""
    q = np.ascontiguousarray(q, np.float32)
    N = len(enc)
    s = np.empty((len(q), N), np.float32)
    r = np.empty((len(q), N), np.int64)
    for b in range(len(q)):
        m, v = (0, 0) if filters is None else (int(filters[b][0]), int(filters[b][1]))
        s[b], r[b] = [a[0] for a in O.search(enc, q[b:b + 1], N, tags=np.asarray(tags, np.uint32),
                                             mask=m, value=v, use_filter=True)]
    return s, r


def search_groups(enc, q, tags, filters, key_mask: int, G: int, S: int, lists=None):
    """The definition: the walk over every matching row in (score desc, row asc) order. Per
    query [(key, [(row, score), ...]), ...]. `lists`: ranked()'s result, to share it."""
    tags = np.asarray(tags).astype(np.uint32)
    s, r = lists if lists is not None else ranked(enc, q, tags, filters)
    out = []
    for b in range(len(r)):
        n = int((r[b] >= 0).sum())
        found = walk(s[b], r[b], tags[np.maximum(r[b], 0)], n, key_mask, G, S)
        out.append([(key, [(int(r[b, j]), float(s[b, j])) for j in pos]) for key, pos in found])
    return out


def assert_recipe_cases(enc, Q, tags, lists):
    """The cases the tests rest on, asserted on this reference alone (ticker field, G = 4,
    S = 3): (a) some query's first 8 candidates hold fewer than 4 keys; (b) some group selected
    there has fewer than S hits among them and more rows in the corpus; (c) the RARE key, two
    rows in all, is selected and under-full in the final result; (d) key-0 rows among the
    candidates; (e) two bit-identical rows under different keys are the best hits of two
    groups, so that their score tie decides the group order by row."""
    def f32bits(v):
        return np.float32(v).view(np.uint32)

    G, S, mask = 4, 3, TICKER_MASK
    s, r = lists
    full = search_groups(enc, Q, tags, None, mask, G, S, lists)
    keys8, fill8, _, _, _, count8 = select(s[:, :8], r[:, :8], tags[r[:, :8]], None, mask, G, S)
    assert (count8[:, 0] < G).any()                                                    # (a)
    total = {k: int(((tags & mask) == k).sum()) for q in full for k, _ in q}
    assert any(fill8[b, g] < S and total[int(keys8[b, g])] > fill8[b, g]
               for b in range(len(Q)) for g in range(int(count8[b, 0])))               # (b)
    assert total[RARE] == 2 < S and any(k == RARE and len(h) == 2 for q in full for k, h in q)  # (c)
    assert ((tags[r[:, :8]] & mask) == 0).any()                                        # (d)
    assert any(f32bits(a[1][0][1]) == f32bits(b[1][0][1]) and {a[0], b[0]} == {TIE, TIE + 1}
               and a[1][0][0] < b[1][0][0] and np.array_equal(enc[a[1][0][0]], enc[b[1][0][0]])
               for q in search_groups(enc, Q, tags, None, mask, 60, 2, lists)
               for a, b in zip(q, q[1:]))                                              # (e)
