"""One collection over several shards from one process: rag_shardset_search against the route
the tree offered before it, at the serving shape (B = 32, k = 15).

On one GPU: ROWS (default 10M) x 384 fp16 as SHARDS (default 8) logical shards.
  (a) shardset : ShardSet.search — fan-out over the shards' streams, one gather-merge launch
  (b) loop     : a Python loop of SHARDS search_packed(id_offset=...) calls on contiguous
                 shards, torch.stack, merge_topk_packed
Both and the single ROWS-row index must agree id for id (checked before timing). Each route
is warmed, then timed over REPEATS (5) windows of ITERS (200) searches, each window ended by a
device synchronise, the routes alternating inside this one process. One JSON line per route
with every window's ms per search; where two or more GPUs are visible, one more line for a
ShardSet over all of them (one shard per GPU). Lines go to stdout and to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "financial-rag-system_amd"))

from ragmi.index import FlatIndex, merge_topk_packed  # noqa: E402
from ragmi.shardset import ShardSet  # noqa: E402

D, B, K = 384, 32, 15
CHUNK = 1 << 20


def fill(targets, n, dev):
    """The same seeded rows into every target (global rows), chunk by chunk."""
    g = torch.Generator(device=dev)
    g.manual_seed(1000)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        x = torch.randn((m, D), generator=g, device=dev)
        for put in targets:
            put(x, r0, m)
    torch.cuda.synchronize()


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shardset_one_gpu.jsonl"))
    args = ap.parse_args()
    n = int(os.environ.get("ROWS", "10000000"))
    ns = int(os.environ.get("SHARDS", "8"))
    iters, repeats = int(os.environ.get("ITERS", "200")), int(os.environ.get("REPEATS", "5"))
    dev = torch.device("cuda", 0)
    single = FlatIndex(D, n, dev)
    ss = ShardSet(D, [0] * ns, n, "fp16")
    bounds = [n * s // ns for s in range(ns + 1)]
    parts = [FlatIndex(D, bounds[s + 1] - bounds[s], dev) for s in range(ns)]

    def put_parts(x, r0, m):
        for s, p in enumerate(parts):
            lo, hi = max(bounds[s], r0), min(bounds[s + 1], r0 + m)
            if lo < hi:
                p.upsert(x[lo - r0:hi - r0], np.arange(lo - bounds[s], hi - bounds[s]),
                         new_count=hi - bounds[s])

    fill([lambda x, r0, m: single.upsert(x, np.arange(r0, r0 + m), new_count=r0 + m),
          lambda x, r0, m: ss.upsert(x, np.arange(r0, r0 + m), new_count=r0 + m),
          put_parts], n, dev)
    rng = np.random.default_rng(3)
    q = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(dev)

    def route_set():
        return ss.search(q, K)

    def route_loop():
        packed = [p.search_packed(q, K, id_offset=bounds[s]) for s, p in enumerate(parts)]
        return merge_topk_packed(torch.stack(packed), K)

    ref = [t.cpu().numpy() for t in single.search(q, K)]
    for name, fn in (("shardset", route_set), ("loop", route_loop)):
        s, i = [t.cpu().numpy() for t in fn()]
        assert np.array_equal(i, ref[1]), f"{name}: ids differ from the single index"
        assert np.array_equal(s, ref[0]), f"{name}: scores differ from the single index"
    routes = {"shardset": route_set, "loop": route_loop}
    ms = {name: [] for name in routes}
    for fn in routes.values():
        window(fn, max(10, iters // 10))                     # warm
    for _ in range(repeats):
        for name, fn in routes.items():                      # alternating
            ms[name].append(round(window(fn, iters), 4))
    lines = [{"bench": "shardset_one_gpu", "route": name, "rows": n, "dim": D, "storage": "fp16",
              "logical_shards": ns, "B": B, "k": K, "iters_per_window": iters,
              "ms_per_search": v, "median_ms": float(np.median(v)),
              "agrees_with_single_index": True} for name, v in ms.items()]
    n_dev = torch.cuda.device_count()
    if n_dev >= 2:
        single.close()
        for p in parts:
            p.close()
        ss.close()
        ms_set = ShardSet(D, list(range(n_dev)), n, "fp16")
        fill([lambda x, r0, m: ms_set.upsert(x, np.arange(r0, r0 + m), new_count=r0 + m)], n, dev)
        s, i = [t.cpu().numpy() for t in ms_set.search(q, K)]
        assert np.array_equal(i, ref[1]) and np.array_equal(s, ref[0])
        window(lambda: ms_set.search(q, K), max(10, iters // 10))
        v = [round(window(lambda: ms_set.search(q, K), iters), 4) for _ in range(repeats)]
        lines.append({"bench": "shardset_multi_gpu", "route": "shardset", "rows": n, "dim": D,
                      "storage": "fp16", "devices": n_dev, "B": B, "k": K,
                      "iters_per_window": iters, "ms_per_search": v,
                      "median_ms": float(np.median(v)), "agrees_with_single_index": True})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
