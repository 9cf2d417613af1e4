"""Grouped search — the exactness ladder behind query_points_groups.

`group_select` (rag_group_select) walks a candidate list; a list of C candidates is only a
prefix of the ranked list the definition walks (include/ragmi.h), so a walk over it can stop
short: fewer than G groups opened, or an opened group with fewer than S hits while more of its
rows rank below the list's end. The ladder below closes both gaps with further exact searches,
so the result equals the walk over the WHOLE ranked list for every candidate setting.
`candidates` and `widen` are policy: they decide which rung answers, never what is answered.

Host logic over any object with `count`, `search(queries, k, filters)` and
`group_select(cand_scores, cand_rows, key_mask, G, S)`: FlatIndex, ShardSet, or a numpy
stand-in (tests). No reference counterpart: the reference over-fetches one flat top-15
(main.py:215, 232-237) and never groups.
"""
from __future__ import annotations

import numpy as np
import torch

from .index import MAX_K_LARGE, QUERY_TILE, hits_of


def default_candidates(G: int, S: int) -> int:
    """C1: what a flat over-fetch would ask for. 2 * G * S leaves room for key-0 rows and for
    groups deeper than S; 100 is the front end's MMR default, a list the large-k pass already
    serves at the cost of a search(k = 100)."""
    return max(100, 2 * G * S)


def _np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _take(x, idx):
    if isinstance(x, torch.Tensor):
        return x[torch.as_tensor(idx, dtype=torch.int64, device=x.device)]
    return x[np.asarray(idx, dtype=np.int64)]


def _rank_key(hit):
    return (-hit[1], hit[0])          # (score desc, row asc); hit = (row, score)


def search_groups(index, queries, filters, key_mask: int, keys_possible, G: int, S: int,
                  candidates: int | None = None, widen: int | None = None, search=None,
                  stats: dict | None = None):
    """Per query the G best groups under `key_mask`, each with its S best hits, exactly:
    [(key, [(row, score), ...]), ...] per query, groups by best hit, hits by (score desc, row
    asc). `queries` [B, dim]; `filters` None or [B, 2] uint32 (mask, value); `keys_possible[b]`:
    the keys (tag bits under key_mask) the query's filter allows — every code of the field, or
    the one the filter fixes. `search(queries, k, filters)` defaults to index.search (a caller
    passes its own to re-answer unanswered large-k queries). `stats` counts "widened" (queries
    re-searched at `widen`), "per_key" (filtered per-key queries sent) and "filled" (groups
    re-answered because the list cut them short).

    1. search at C1 = `candidates`, group_select. A query whose list holds every matching row
       (n_b < C, or C = count) is exhausted: its result is final.
    2. A non-exhausted query with fewer than min(G, |keys_possible|) groups is short. With at
       most RAG_QUERY_TILE keys still possible they are asked directly (3); otherwise the
       short queries are re-searched at `widen` and selected again.
    3. A query still short: one filtered search (mask | key_mask, value | key), k = S, per key
       not found yet, all in one batched call; the keys with a hit, ranked by their best hit,
       supply the missing groups, complete.
    4. Every selected group with fewer than S hits in a non-exhausted query is re-answered by
       the same kind of filtered query, all in one batched call; its hits replace the group's."""
    search = search or index.search
    key_mask = int(key_mask) & 0xFFFFFFFF
    count = int(index.count)
    B = len(keys_possible)
    if B == 0 or count == 0:
        return [[] for _ in range(B)]
    fl = (np.zeros((B, 2), np.uint32) if filters is None
          else np.asarray(_np(filters)).astype(np.uint32).reshape(B, 2))
    cap = min(count, MAX_K_LARGE)
    C1 = min(max(int(candidates if candidates is not None else default_candidates(G, S)), 1), cap)
    Cw = min(max(int(widen if widen is not None else MAX_K_LARGE), 1), cap)
    k_key = min(S, count)
    st = stats if stats is not None else {}
    for name in ("widened", "per_key", "filled"):
        st.setdefault(name, 0)

    groups = [[] for _ in range(B)]      # per query [key, [(row, score), ...], complete]
    exhausted = np.zeros(B, bool)

    def select(which, C):
        s, r = search(_take(queries, which) if len(which) != B else queries, C,
                      fl[which] if fl.any() else None)
        sel = index.group_select(s, r, key_mask, G, S)
        keys = _np(sel.keys).view(np.uint32)
        fill, cnt = _np(sel.fill), _np(sel.count)
        hs, hr = _np(sel.scores), _np(sel.rows)
        for j, b in enumerate(which):
            groups[b] = [[int(keys[j, g]),
                          [(int(hr[j, g, i]), float(hs[j, g, i])) for i in range(int(fill[j, g]))],
                          False] for g in range(int(cnt[j, 0]))]
            exhausted[b] = cnt[j, 1] < C or C == count

    def short(b):
        return not exhausted[b] and len(groups[b]) < min(G, len(keys_possible[b]))

    def ask(pairs):
        """One batched filtered search, k = S: the hits of each (query, key) pair."""
        if not pairs:
            return []
        which = [b for b, _ in pairs]
        f = fl[which].copy()
        f[:, 0] |= np.uint32(key_mask)
        f[:, 1] |= np.asarray([k for _, k in pairs], np.uint32)
        return hits_of(*search(_take(queries, which), k_key, f))

    select(list(range(B)), C1)                                            # 1
    wide = [b for b in range(B)
            if short(b) and len(keys_possible[b]) - len(groups[b]) > QUERY_TILE]
    if wide and Cw > C1:                                                  # 2
        st["widened"] += len(wide)
        select(wide, Cw)
    pairs = []                                                            # 3
    for b in range(B):
        if short(b):
            found = {g[0] for g in groups[b]}
            pairs += [(b, int(k)) for k in sorted(keys_possible[b]) if int(k) not in found]
    st["per_key"] += len(pairs)
    fresh = [[] for _ in range(B)]
    for (b, k), hits in zip(pairs, ask(pairs)):
        if hits:
            fresh[b].append([k, hits, True])
    for b in range(B):
        fresh[b].sort(key=lambda g: _rank_key(g[1][0]))
        groups[b] += fresh[b][:G - len(groups[b])]
    pairs = [(b, g[0]) for b in range(B) if not exhausted[b]             # 4
             for g in groups[b] if not g[2] and len(g[1]) < S]
    st["filled"] += len(pairs)
    answers = iter(ask(pairs))
    for b in range(B):
        if not exhausted[b]:
            for g in groups[b]:
                if not g[2] and len(g[1]) < S:
                    g[1] = next(answers)
    return [[(g[0], g[1]) for g in groups[b]] for b in range(B)]
