"""What a discovery or context request costs, against recommend's hot pass at the same example
count and against what a caller could do before it existed.

ROWS (default 1M) x 384 fp16 seeded Gaussian rows on a FlatIndex, 500 tickers in the tags. The
target and the positives are corpus rows plus noise, the negatives fresh Gaussian vectors. In one
process, after WARMUP calls of each shape, ITERS timed calls of each (a HIP event pair around the
call), the shapes of one block alternating call by call; medians in ms:
  hot    FlatIndex.discover at discover n in 1, 3, 15 and context n in 3, 16, k in 15, 100,
         unfiltered and under a one-ticker filter — the hot pass; beside each, in the same block,
         FlatIndex.recommend(best_score) with the same E = 2 n (+ 1) examples: both stream the same
         fp16 rows once. Every shape is checked unsaturated from the stats (one round, at most
         16384 candidates, nothing unanswered). The context n = 3 request is the cyclic preference
         (a, b), (b, c), (c + 0.1 g, a): three independent random pairs would saturate (an eighth
         of the corpus scores 0), this cone holds about 2e-4 of it, and the rows within the
         bound's width of it stay below the candidate list's 16384 at 10M rows. (Pairs that
         contradict outright, (a, b) and (b, a), do NOT work: the best scores then sit at the
         cusp e_a = e_b where the corpus is dense, about 30,000 rows within the bounds at 10M,
         and the hot pass leaves the request unanswered after three rounds.)
  full   the same requests with full=True (FULL_ITERS calls), unfiltered, k = 15
  exact  E x FlatIndex.search(B = 1, k = 15, full=True): one full exact pass per example, what a
         caller had to run before combining E score arrays on the host (the combine is not timed)
  saturated  one context request with ONE pair (about half the corpus scores 0) under
         rescue=True: the hot attempt that leaves it unanswered plus the full pass that answers
One JSON line per shape, to stdout and appended to --out (default
profiles/discover_timing.jsonl). Run each row count as its own step under its own time limit:
  timeout -k 10 300 python scripts/bench_discover.py --rows 1000000 && \\
  timeout -k 10 600 python scripts/bench_discover.py --rows 10000000"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "financial-rag-system_amd"))

from ragmi.index import FlatIndex  # noqa: E402

D, TICKERS, CAP = 384, 500, 16384
CHUNK = 1 << 18
SHAPES = (("discover", 1), ("discover", 3), ("discover", 15), ("context", 3), ("context", 16))
KS = (15, 100)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discover_timing.jsonl"))
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
    base = {"bench": "discover", "rows": args.rows, "dim": D, "storage": "fp16",
            "warmup": args.warmup, "iters": args.iters,
            "device": torch.cuda.get_device_name(0)}
    lines = []

    def emit(rec):
        line = json.dumps({**base, **rec})
        print(line, flush=True)
        lines.append(line)

    def ms(t):
        return {"ms": round(t[0], 4), "ms_min_max": [round(t[1], 4), round(t[2], 4)]}

    for kind, n in SHAPES:
        target = seeds[31] if kind == "discover" else None
        pos, neg = seeds[:n].clone(), negs[:n].clone()
        if kind == "context" and n == 3:                    # a > b, b > c, c + 0.1 g > a
            pos[1], neg[1] = negs[0], negs[1]
            pos[2], neg[2] = negs[1] + 0.1 * negs[2], seeds[0]
        E = 2 * n + (kind == "discover")
        # recommend best_score at the same example count: ceil(E / 2) positives, the rest negatives
        rp, rn = seeds[:(E + 1) // 2], (negs[:E // 2] if E // 2 else None)
        for k in KS:
            for flt in (None, one_ticker):
                fns = {"hot": lambda: idx.discover(target, pos, neg, k, filters=flt),
                       "reco": lambda: idx.recommend(rp, rn, "best_score", k, filters=flt)}
                un = idx.unanswered()
                t = timed(fns, args.warmup, args.iters)
                fns["hot"]()
                st = idx.discover_stats()
                fns["reco"]()
                rst = idx.reco_stats()
                unsat = st.rounds == 1 and st.candidates <= CAP and idx.unanswered() == un
                assert unsat, (kind, n, k, flt, st)
                emit({"shape": "hot", "kind": kind, "n": n, "E": E, "k": k,
                      "filtered": flt is not None, **ms(t["hot"]), "candidates": st.candidates,
                      "rounds": st.rounds, "unsaturated": unsat,
                      "reco_best_same_E_ms": round(t["reco"][0], 4),
                      "reco_best_same_E_ms_min_max": [round(t["reco"][1], 4),
                                                      round(t["reco"][2], 4)],
                      "reco_candidates": rst.candidates})
        ex = torch.cat([pos, neg] + ([target[None]] if target is not None else []))

        def per_example():
            for e in range(E):
                idx.search(ex[e:e + 1], 15, full=True)

        t = timed({"full": lambda: idx.discover(target, pos, neg, 15, full=True),
                   "exact": per_example}, 1, args.full_iters)
        emit({"shape": "full", "kind": kind, "n": n, "E": E, "k": 15, "filtered": False,
              "iters": args.full_iters, **ms(t["full"])})
        emit({"shape": "exact_per_example", "kind": kind, "n": n, "E": E, "k": 15,
              "iters": args.full_iters, **ms(t["exact"])})
    # one saturated context request: the hot attempt, then the full pass (rescue)
    un, rescued = idx.unanswered(), idx.rescued
    t = timed({"sat": lambda: idx.discover(None, seeds[:1], negs[:1], 15, rescue=True),
               "hot_only": lambda: idx.discover(None, seeds[:1], negs[:1], 15)},
              1, args.full_iters)
    st = idx.discover_stats()
    calls = 1 + args.full_iters
    assert idx.rescued == rescued + calls and idx.unanswered() == un + 2 * calls
    emit({"shape": "saturated", "kind": "context", "n": 1, "E": 2, "k": 15,
          "iters": args.full_iters, **ms(t["sat"]), "hot_attempt_ms": round(t["hot_only"][0], 4),
          "candidates": st.candidates, "rounds": st.rounds})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    idx.close()


if __name__ == "__main__":
    main()
