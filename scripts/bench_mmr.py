"""What MMR re-selection costs on top of the candidate search it follows.

ROWS (default 1M) x 384 fp16 seeded Gaussian rows on a FlatIndex; B = 32 queries (corpus rows
plus noise), C = 100 candidates, k = 15, diversity 0.5. In one process, alternating batch by
batch after WARMUP (20) batches of each:
  search      FlatIndex.search(k = C) alone — the candidate search, the code path the tree had
              before MMR
  search_mmr  FlatIndex.search_mmr(k, diversity, C): the same search, then rag_index_mmr
each timed by a HIP event pair around the call, ITERS (200) batches of each. One JSON line with
the medians, their difference and the difference per greedy step (k - 1 scoring steps), to
stdout and appended to --out (default profiles/mmr_timing.jsonl).

The MMR kernel's own time comes from a separate run under a kernel trace, e.g.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mmr -- \
      python scripts/bench_mmr.py --iters 50 --out /dev/null
(DIR/**/mmr_kernel_stats.csv: the mmr_kernel row)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "financial-rag-system_amd"))

from ragmi.index import FlatIndex  # noqa: E402

D, B, C, K, DIVERSITY = 384, 32, 100, 15, 0.5
CHUNK = 1 << 18


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    idx = FlatIndex(D, args.rows, dev, storage="fp16")
    g = torch.Generator(device=dev)
    g.manual_seed(1000)
    q = None
    for r0 in range(0, args.rows, CHUNK):
        n = min(CHUNK, args.rows - r0)
        x = torch.randn((n, D), generator=g, device=dev)
        if q is None:
            q = x[:B] + 0.05 * torch.randn((B, D), generator=g, device=dev)
        idx.upsert(x, torch.arange(r0, r0 + n, device=dev), new_count=r0 + n)
    torch.cuda.synchronize()

    def search():
        return idx.search(q, C)

    def search_mmr():
        return idx.search_mmr(q, K, DIVERSITY, C)

    for _ in range(args.warmup):
        search()
        search_mmr()
    torch.cuda.synchronize()
    t_search, t_mmr = [], []
    for _ in range(args.iters):
        t_search.append(event_ms(search))
        t_mmr.append(event_ms(search_mmr))
    s, m = float(np.median(t_search)), float(np.median(t_mmr))
    rec = {"bench": "mmr", "rows": args.rows, "dim": D, "storage": "fp16", "B": B, "C": C, "k": K,
           "diversity": DIVERSITY, "warmup": args.warmup, "iters": args.iters,
           "search_ms": round(s, 4), "search_mmr_ms": round(m, 4),
           "mmr_extra_ms": round(m - s, 4), "mmr_extra_us_per_step": round(1e3 * (m - s) / (K - 1), 2),
           "search_ms_min_max": [round(min(t_search), 4), round(max(t_search), 4)],
           "search_mmr_ms_min_max": [round(min(t_mmr), 4), round(max(t_mmr), 4)],
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
