"""What an exact grouped search costs next to the flat over-fetch a caller would do instead.

ROWS (default 1M) x 384 fp16 rows on a FlatIndex, TICKERS (500) ticker codes in the low 16 tag
bits: row r belongs to ticker r % TICKERS and is 0.35 x its ticker's seeded Gaussian centre plus
unit Gaussian noise, so a query's nearest rows are partly its own ticker's and partly everyone's.
B = 32 queries (corpus rows plus noise), G = 10 groups of S = 3 hits, C1 = the ladder's default
(100). In one process, alternating batch by batch after WARMUP (20) batches of each:
  search         FlatIndex.search(k = C1) alone — the over-fetch, the code path the tree had
                 before grouped search
  group_select   gather_tags + rag_group_select over that search's lists (the new kernels alone)
  search_groups  ragmi.groups.search_groups: the whole ladder, host logic and read-backs included
each timed by a HIP event pair around the call, ITERS (100) batches of each. One JSON line with the
medians, the ranges and the route counters of one batch (queries widened, per-key queries sent,
groups re-answered), to stdout and appended to --out (default profiles/groups_timing.jsonl). The
further searches those rungs issue are timed the same way on their own (widen_search: the widened
queries at k = 4096; fill_search: one filtered k = S query per per-key or re-answered group), so the
difference to `search` can be told apart from the host's share.

The kernels' own times come from a separate run under a kernel trace, e.g.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o groups -- \
      python scripts/bench_groups.py --iters 20 --out /dev/null
(DIR/**/groups_kernel_stats.csv: the group_select_kernel and gather_tags_kernel rows)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "financial-rag-system_amd"))

from ragmi import groups  # noqa: E402
from ragmi.index import FlatIndex  # noqa: E402

D, B, G, S, KEY_MASK = 384, 32, 10, 3, 0xFFFF
CHUNK = 1 << 18


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(t):
    return [round(float(np.median(t)), 4), round(min(t), 4), round(max(t), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--tickers", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groups_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    idx = FlatIndex(D, args.rows, dev, storage="fp16")
    g = torch.Generator(device=dev)
    g.manual_seed(1000)
    centres = torch.randn((args.tickers, D), generator=g, device=dev)
    q = None
    for r0 in range(0, args.rows, CHUNK):
        n = min(CHUNK, args.rows - r0)
        rows = torch.arange(r0, r0 + n, device=dev)
        ticker = rows % args.tickers
        x = 0.35 * centres[ticker] + torch.randn((n, D), generator=g, device=dev)
        if q is None:
            q = x[:B] + 0.05 * torch.randn((B, D), generator=g, device=dev)
        idx.upsert(x, rows, (ticker + 1).to(torch.int32), new_count=r0 + n)
    torch.cuda.synchronize()
    C1 = min(groups.default_candidates(G, S), args.rows)
    possible = [[c + 1 for c in range(args.tickers)]] * B
    lists = idx.search(q, C1)

    def search():
        return idx.search(q, C1)

    def group_select():
        return idx.group_select(lists[0], lists[1], KEY_MASK, G, S)

    def search_groups(stats=None):
        return groups.search_groups(idx, q, None, KEY_MASK, possible, G, S, stats=stats)

    for _ in range(args.warmup):
        search()
        group_select()
        search_groups()
    torch.cuda.synchronize()
    routes = {}
    found = search_groups(routes)
    # the rungs one batch climbed, re-enacted as the searches they issue: `widened` queries at
    # k = RAG_MAX_K_LARGE, and one filtered k = S query per per-key / re-answered group
    n_w, n_f = routes["widened"], routes["per_key"] + routes["filled"]
    q_f = q.repeat(-(-max(n_f, 1) // B), 1)[:max(n_f, 1)]
    f_f = np.array([[KEY_MASK, 1 + i % args.tickers] for i in range(len(q_f))], np.uint32)
    k_w = min(4096, args.rows)

    def widen():
        return idx.search(q[:max(n_w, 1)], k_w)

    def fill():
        return idx.search(q_f, S, f_f)

    for _ in range(args.warmup):
        widen()
        fill()
    torch.cuda.synchronize()
    t_search, t_select, t_groups, t_widen, t_fill = [], [], [], [], []
    for _ in range(args.iters):
        t_search.append(event_ms(search))
        t_select.append(event_ms(group_select))
        t_groups.append(event_ms(search_groups))
        t_widen.append(event_ms(widen))
        t_fill.append(event_ms(fill))
    rec = {"bench": "groups", "rows": args.rows, "dim": D, "storage": "fp16", "tickers": args.tickers,
           "B": B, "G": G, "S": S, "C1": C1, "warmup": args.warmup, "iters": args.iters,
           "search_ms_median_min_max": spread(t_search),
           "group_select_ms_median_min_max": spread(t_select),
           "search_groups_ms_median_min_max": spread(t_groups),
           "routes_per_batch": routes,
           "widen_search_ms_median_min_max": spread(t_widen) if n_w else None,
           "fill_search_ms_median_min_max": spread(t_fill) if n_f else None,
           "groups_found": [len(f) for f in found],
           "hits_per_group_min": min(len(h) for f in found for _, h in f),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    idx.close()


if __name__ == "__main__":
    main()
