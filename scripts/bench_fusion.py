"""What reciprocal rank fusion costs on top of the batched search that feeds it.

ROWS (default 1M) x 384 fp16 seeded Gaussian rows on a FlatIndex; B = 32 requests of L = 3
prefetches each (a corpus row plus noise, under three independent noises): 96 flattened queries,
C = 100 candidates per list, k = 15, rrf_k = 2. In one process, alternating batch by batch after
WARMUP (20) batches of each:
  search        FlatIndex.search(96 queries, k = C) alone — the code path the tree had before
                fusion
  search_fuse   the same search, the arrangement of its rows into [B, L, C] with per-list counts
                (the device ops of Collection.search_fusion) and fuse_rrf
each timed by a HIP event pair around the call, ITERS (200) batches of each. Also recorded, by a
host clock around work that ends with the results on the host (ITERS / 4 batches):
  separate_host three searches of 32 queries each, their rows copied to the host and fused there
                in numpy — what a caller had to do before fusion
  search_fuse_host  search_fuse with its [B, k] results copied to the host, for comparison
One JSON line with the medians and the difference, to stdout and appended to --out (default
profiles/fusion_timing.jsonl).

The fusion kernel's own time comes from a separate run under a kernel trace, e.g.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fusion -- \\
      python scripts/bench_fusion.py --iters 50 --out /dev/null
(DIR/**/fusion_kernel_stats.csv: the rrf_fuse_kernel row)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "financial-rag-system_amd"))

from ragmi.index import FlatIndex, fuse_rrf  # noqa: E402

D, B, L, C, K, RRF_K = 384, 32, 3, 100, 15, 2
CHUNK = 1 << 18


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t)


def host_fuse(rows):
    """RRF of rows int64 [B, L, C] on the host: the numpy a caller would write."""
    w = np.tile(1.0 / (RRF_K + np.arange(rows.shape[2], dtype=np.float64)), rows.shape[1])
    out = []
    for b in range(rows.shape[0]):
        u, inv = np.unique(rows[b].ravel(), return_inverse=True)
        sc = np.bincount(inv, weights=w).astype(np.float32)
        order = np.lexsort((u, -sc))[:K]
        out.append((u[order], sc[order]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    idx = FlatIndex(D, args.rows, dev, storage="fp16")
    g = torch.Generator(device=dev)
    g.manual_seed(1000)
    q = None
    for r0 in range(0, args.rows, CHUNK):
        n = min(CHUNK, args.rows - r0)
        x = torch.randn((n, D), generator=g, device=dev)
        if q is None:          # [B, L, D] -> the flattened batch, request-major
            q = (x[:B, None] + 0.5 * torch.randn((B, L, D), generator=g, device=dev))
            q = q.reshape(B * L, D).contiguous()
        idx.upsert(x, torch.arange(r0, r0 + n, device=dev), new_count=r0 + n)
    torch.cuda.synchronize()
    at = np.asarray([(b, l) for b in range(B) for l in range(L)], dtype=np.int64)
    ncand = np.full((B, L), min(C, args.rows), dtype=np.int32)

    def search():
        return idx.search(q, C)

    def search_fuse():
        _, ids = idx.search(q, C)
        rows = torch.full((B, L, C), -1, dtype=torch.int64, device=dev)
        rows[torch.from_numpy(at[:, 0]).to(dev), torch.from_numpy(at[:, 1]).to(dev)] = ids
        return fuse_rrf(rows, K, RRF_K, ncand)

    def search_fuse_host():
        s, r = search_fuse()
        return s.cpu().numpy(), r.cpu().numpy()

    def separate_host():
        rows = np.stack([idx.search(q[l::L], C)[1].cpu().numpy() for l in range(L)], axis=1)
        return host_fuse(rows)

    # the two routes agree before anything is timed
    s, r = search_fuse_host()
    for b, (hr, hs) in enumerate(separate_host()):
        assert np.array_equal(hr, r[b]) and np.array_equal(hs.view(np.uint32),
                                                           s[b].view(np.uint32))
    for _ in range(args.warmup):
        search()
        search_fuse()
    torch.cuda.synchronize()
    t_search, t_fuse, t_sep, t_fh = [], [], [], []
    for _ in range(args.iters):
        t_search.append(event_ms(search))
        t_fuse.append(event_ms(search_fuse))
    for _ in range(max(1, args.iters // 4)):
        t_sep.append(host_ms(separate_host))
        t_fh.append(host_ms(search_fuse_host))
    a, b = float(np.median(t_search)), float(np.median(t_fuse))
    rec = {"bench": "fusion", "rows": args.rows, "dim": D, "storage": "fp16", "B": B, "L": L,
           "C": C, "k": K, "rrf_k": RRF_K, "warmup": args.warmup, "iters": args.iters,
           "search_ms": round(a, 4), "search_fuse_ms": round(b, 4),
           "fuse_extra_ms": round(b - a, 4),
           "search_ms_min_max": [round(min(t_search), 4), round(max(t_search), 4)],
           "search_fuse_ms_min_max": [round(min(t_fuse), 4), round(max(t_fuse), 4)],
           "host_iters": len(t_sep),
           "separate_host_ms": round(float(np.median(t_sep)), 4),
           "separate_host_ms_min_max": [round(min(t_sep), 4), round(max(t_sep), 4)],
           "search_fuse_host_ms": round(float(np.median(t_fh)), 4),
           "search_fuse_host_ms_min_max": [round(min(t_fh), 4), round(max(t_fh), 4)],
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
