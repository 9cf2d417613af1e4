"""What a recommend request costs, against the two things a caller could do before it existed.

ROWS (default 1M) x 384 fp16 seeded Gaussian rows on a FlatIndex, 500 tickers in the tags; the
examples are corpus rows plus noise (positives) and fresh Gaussian vectors (negatives). In one
process, after WARMUP calls of each shape, ITERS timed calls of each (a HIP event pair around
the call), the shapes of one block alternating call by call; medians in ms:
  hot    FlatIndex.recommend(best_score | sum_scores) at (P, N) in (1,0), (3,2), (16,16), k in
         15, 100, unfiltered and under a one-ticker filter — the hot pass
  full   the same requests with full=True (FULL_ITERS calls): the new full pass
  largek FlatIndex.search(B = 32, k = 33): the large-k pass, one MFMA stream of the same rows with
         candidate collection — the floor the hot pass is shaped after
  exact  E x FlatIndex.search(B = 1, k, full=True), E = P + N: one full exact pass per example,
         what a caller had to run before combining 'ROWS' scores per example on the host (the
         host combine itself is not timed)
  avg    FlatIndex.recommend(average_vector) against the FlatIndex.search(B = 1, k) it reduces to
One JSON line per shape, to stdout and appended to --out (default profiles/reco_timing.jsonl).

Kernel times come from a separate run under a kernel trace, e.g.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o reco -- \\
      python scripts/bench_reco.py --iters 20 --out /dev/null
(DIR/**/reco_kernel_stats.csv: the reco_collect_kernel / reco_rescore_kernel rows)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "financial-rag-system_amd"))

from ragmi.index import FlatIndex  # noqa: E402

D, TICKERS = 384, 500
CHUNK = 1 << 18
SIDES = ((1, 0), (3, 2), (16, 16))
KS = (15, 100)
STRATEGIES = ("best_score", "sum_scores")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fns: dict, warmup: int, iters: int) -> dict:
    """name -> (median, min, max) ms of `iters` calls of each function, alternating call by call
    after `warmup` calls of each."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    for _ in range(iters):
        for name, f in fns.items():
            t[name].append(event_ms(f))
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--full-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reco_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    idx = FlatIndex(D, args.rows, dev, storage="fp16")
    g = torch.Generator(device=dev)
    g.manual_seed(1000)
    seeds = None
    for r0 in range(0, args.rows, CHUNK):
        n = min(CHUNK, args.rows - r0)
        x = torch.randn((n, D), generator=g, device=dev)
        if seeds is None:
            seeds = x[:32] + 0.05 * torch.randn((32, D), generator=g, device=dev)
        rows = torch.arange(r0, r0 + n, device=dev)
        idx.upsert(x, rows, (1 + rows % TICKERS).to(torch.int32), new_count=r0 + n)
    negs = torch.randn((16, D), generator=g, device=dev)
    torch.cuda.synchronize()
    one_ticker = (0xFFFF, 7)
    base = {"bench": "reco", "rows": args.rows, "dim": D, "storage": "fp16",
            "warmup": args.warmup, "iters": args.iters,
            "device": torch.cuda.get_device_name(0)}
    lines = []

    def emit(rec):
        line = json.dumps({**base, **rec})
        print(line, flush=True)
        lines.append(line)

    def ms(t):
        return {"ms": round(t[0], 4), "ms_min_max": [round(t[1], 4), round(t[2], 4)]}

    # the large-k yardstick, beside the (3,2) hot pass it is compared with
    t = timed({"largek": lambda: idx.search(seeds, 33),
               "hot": lambda: idx.recommend(seeds[:3], negs[:2], "best_score", 15)},
              args.warmup, args.iters)
    emit({"shape": "largek", "B": 32, "k": 33, **ms(t["largek"]),
          "hot_best_3_2_k15_ms": round(t["hot"][0], 4)})
    for P, N in SIDES:
        pos, neg = seeds[:P], (negs[:N] if N else None)
        for k in KS:
            for flt in (None, one_ticker):
                fns = {s: (lambda s=s: idx.recommend(pos, neg, s, k, filters=flt))
                       for s in STRATEGIES}
                t = timed(fns, args.warmup, args.iters)
                stats = {}
                for s in STRATEGIES:
                    fns[s]()
                    stats[s] = idx.reco_stats()
                for s in STRATEGIES:
                    emit({"shape": "hot", "strategy": s, "P": P, "N": N, "k": k,
                          "filtered": flt is not None, **ms(t[s]),
                          "candidates": stats[s].candidates, "rounds": stats[s].rounds})
        # the full pass and the per-example exact passes, unfiltered, k = 15
        E = P + N
        ex = torch.cat([pos, neg]) if N else pos

        def per_example():
            for e in range(E):
                idx.search(ex[e:e + 1], 15, full=True)

        fns = {s: (lambda s=s: idx.recommend(pos, neg, s, 15, full=True)) for s in STRATEGIES}
        fns["exact"] = per_example
        t = timed(fns, 1, args.full_iters)
        for s in STRATEGIES:
            emit({"shape": "full", "strategy": s, "P": P, "N": N, "k": 15, "filtered": False,
                  "iters": args.full_iters, **ms(t[s])})
        emit({"shape": "exact_per_example", "E": E, "k": 15, "iters": args.full_iters,
              **ms(t["exact"])})
        # average_vector against the plain search it reduces to
        v = idx.reco_vector(pos, neg)
        for k in KS:
            t = timed({"avg": lambda: idx.recommend(pos, neg, None, k),
                       "search": lambda: idx.search(v[None], k)}, args.warmup, args.iters)
            emit({"shape": "average", "P": P, "N": N, "k": k, **ms(t["avg"]),
                  "search_ms": round(t["search"][0], 4)})
    assert idx.unanswered() == 0
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    idx.close()


if __name__ == "__main__":
    main()
