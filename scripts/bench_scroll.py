"""What order_by, facet and a scroll page cost, next to the routes the index API offered before
them.

For each of --rows (default 1M and 10M) a FlatIndex of that many 384-dim fp16 rows carrying what
a collection with 500 tickers and one datetime field carries: ticker code 1 + (r * 7919) % 500
in the low 16 tag bits, 3 document types in the high 16, and key column 0 the key of a microsecond
timestamp drawn uniformly from a 30-day window. In one process, after WARMUP calls of each,
ITERS (>= 20) calls of each timed by a HIP event pair around the call, alternating:

  order_{15,4096}[_ticker]   FlatIndex.order_rows at limit 15 / 4096, unfiltered / under a
                             one-ticker MASKEQ program (1 row in 500 eligible)
  sort_{...}                 the same answer from the earlier API: select_rows_view of every match
                             (select_rows (0, 0) unfiltered), gather_keys, a stable torch.sort,
                             the first `limit` entries. Checked equal to order_rows once.
  facet[_range]              FlatIndex.facet_counts of the ticker field (n_codes = 500),
                             unfiltered / under a RANGE program that passes half the window
  bincount[_range]           select_rows_view + gather_tags + torch.bincount. Checked equal once.
  page                       one 4096-row select_rows_from page from the middle of the index
  page_from_start            select_rows (0, 0) with cap = middle + 4096: what reaching that page
                             took before
Both sides read their counts back as the methods do, so both include one stream synchronise.
The *_dev entries time the new calls through the C ABI alone (no read-back): device time, from
which the achieved bytes/s and the fraction of the 8 TB/s peak are taken, against the bytes each
call must stream —
  view build (under a program): 4 B/row of tags read + 4 B/row of view written, + 8 B/row per
                                RANGE column
  order_rows: 10 passes (8 digit histograms, count, emit) of 8 B/row of keys (+ 4 B/row of view)
  facet_counts: one pass of 4 B/row of tags (+ 4 B/row of view)
One JSON line per row count, to stdout and appended to --out (default
profiles/scroll_timing.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, TICKERS, TYPES = 384, 500, 3
CHUNK = 1 << 18
WINDOW_US = 30 * 86400 * 1_000_000
BASE_US = 1_718_000_000_000_000
PEAK = 8e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(t):
    return [round(float(np.median(t)), 4), round(min(t), 4), round(max(t), 4)]


def build(rows, dev):
    from ragmi.index import FlatIndex
    idx = FlatIndex(D, rows, dev, storage="fp16")
    idx.keys_create(1)
    g = torch.Generator(device=dev)
    g.manual_seed(1000)
    for r0 in range(0, rows, CHUNK):
        n = min(CHUNK, rows - r0)
        r = torch.arange(r0, r0 + n, device=dev)
        x = torch.randn((n, D), generator=g, device=dev)
        tags = ((r * 7919) % TICKERS + 1) | (((r // 7) % TYPES + 1) << 16)
        idx.upsert(x, r, tags.to(torch.int32), new_count=r0 + n)
        us = BASE_US + torch.randint(0, WINDOW_US, (n,), generator=g, device=dev)
        idx.write_keys(0, r, us.double().view(torch.int64))   # a positive double's key: its bits
    torch.cuda.synchronize()
    return idx


def measure(rows, args, dev):
    from ragmi.filters import FilterProgram, key_of_float, pack_view
    idx = build(rows, dev)
    L, h = idx._L, idx._h
    st = torch.cuda.current_stream(dev).cuda_stream
    as_dev = lambda blob: torch.from_numpy(blob.view(np.int32)).to(dev)
    ticker = as_dev(pack_view([FilterProgram.maskeq(0xFFFF, 17)]))
    half = as_dev(pack_view([FilterProgram(
        (("range", 0, key_of_float(float(BASE_US)),
          key_of_float(float(BASE_US + WINDOW_US // 2))),), 0b10)]))
    lo, hi = -(1 << 63) + 1, (1 << 63) - 1
    runs, checks = {}, []

    def sort_route(limit, blob):
        r = idx.select_rows(0, 0)[0] if blob is None else idx.select_rows_view(blob)[0]
        k = idx.gather_keys(0, r)
        o = torch.sort(k, stable=True).indices[:limit]        # r ascending: ties in row order
        return k[o], r[o]

    def bincount_route(blob):
        r = idx.select_rows(0, 0)[0] if blob is None else idx.select_rows_view(blob)[0]
        codes = idx.gather_tags(r) & 0xFFFF
        return torch.bincount(codes, minlength=TICKERS + 1)

    ok = torch.empty((4096,), dtype=torch.int64, device=dev)
    orr = torch.empty((4096,), dtype=torch.int64, device=dev)
    on = torch.empty((2,), dtype=torch.int64, device=dev)
    oc = torch.empty((TICKERS + 1,), dtype=torch.int64, device=dev)
    for limit in (15, 4096):
        for name, blob in (("", None), ("_ticker", ticker)):
            tag = f"{limit}{name}"
            runs[f"order_{tag}"] = lambda limit=limit, blob=blob: idx.order_rows(
                0, limit, programs=blob)
            runs[f"sort_{tag}"] = lambda limit=limit, blob=blob: sort_route(limit, blob)
            p, w = (None, 0) if blob is None else (blob.data_ptr(), blob.numel())
            runs[f"order_{tag}_dev"] = lambda limit=limit, p=p, w=w: L.rag_index_order_rows(
                h, p, w, 0, 0, lo, hi, limit, ok.data_ptr(), orr.data_ptr(), on.data_ptr(), st)
            checks.append((runs[f"order_{tag}"], runs[f"sort_{tag}"]))
    for name, blob in (("", None), ("_range", half)):
        runs[f"facet{name}"] = lambda blob=blob: idx.facet_counts(0, TICKERS, blob)
        runs[f"bincount{name}"] = lambda blob=blob: bincount_route(blob)
        p, w = (None, 0) if blob is None else (blob.data_ptr(), blob.numel())
        runs[f"facet{name}_dev"] = lambda p=p, w=w: L.rag_index_facet_counts(
            h, p, w, 0, TICKERS, oc.data_ptr(), st)
    mid = rows // 2
    runs["page"] = lambda: idx.select_rows_from(mid, None, cap=4096)
    runs["page_from_start"] = lambda: idx.select_rows(0, 0, cap=mid + 4096)[0][mid:]
    # the two routes give the same answer
    for new, old in checks:
        (k1, r1, _), (k2, r2) = new(), old()
        assert torch.equal(k1, k2) and torch.equal(r1, r2)
    for name in ("", "_range"):
        assert torch.equal(runs[f"facet{name}"](), runs[f"bincount{name}"]())
    assert torch.equal(runs["page"]()[0], runs["page_from_start"]())
    for _ in range(args.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.iters):
        for name, fn in runs.items():
            times[name].append(event_ms(fn))
    rec = {"bench": "scroll", "rows": rows, "dim": D, "tickers": TICKERS, "warmup": args.warmup,
           "iters": args.iters}
    rec.update({f"{name}_ms_median_min_max": spread(t) for name, t in times.items()})
    cap = idx.capacity
    view = {"_ticker": 8 * cap, "_range": 16 * cap, "": 0}
    stream = {}
    for limit in (15, 4096):
        for name in ("", "_ticker"):
            stream[f"order_{limit}{name}"] = view[name] + 10 * rows * (8 + (4 if name else 0))
    for name in ("", "_range"):
        stream[f"facet{name}"] = view[name] + rows * (4 + (4 if name else 0))
    for name, nbytes in stream.items():
        t = float(np.median(times[f"{name}_dev"])) * 1e-3
        rec[f"{name}_stream_MB"] = round(nbytes / 1e6, 1)
        rec[f"{name}_GBps"] = round(nbytes / t / 1e9, 1)
        rec[f"{name}_frac_of_8TBps"] = round(nbytes / t / PEAK, 4)
    rec["device"] = torch.cuda.get_device_name(0)
    idx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scroll_timing.jsonl"))
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be at least 20")
    sys.path.insert(0, os.path.join(ROOT, "financial-rag-system_amd"))
    dev = torch.device("cuda", 0)
    for rows in args.rows:
        line = json.dumps(measure(rows, args, dev))
        print(line, flush=True)
        if args.out and args.out != os.devnull:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
