"""Point deletion at the serving size: what a delete costs, against the only alternative the
tree offered before it (recreate_collection + upsert of the survivors from host memory).

ROWS (default 10M) x 384 fp16. Tickers are dealt per "filing" of 64 consecutive rows (one
filing's chunks are ingested together): ticker "A" gets ~1 % of the filings, "B" ~10 %, twenty
others share the rest. Part 1 works on a FlatIndex, part 2 on a QdrantClient collection.

Part 1, device times (HIP events around the calls, after warm-up, REPEATS (10) repeats each,
the median and the spread reported):
  select   rag_index_select_rows over the ROWS tags (4 B each), count only and with the rows
           emitted, for "A" and "B"
  move     rag_index_move_rows of the removal plan for "A" and for "B" (the same plan launched
           again moves the same bytes: sources and destinations are disjoint), bytes moved =
           rows * (768 + 4) read and as many written, against a device-to-device
           hipMemcpyAsync of the same byte count in the same process, the two alternating
Part 2, wall clock (host clock around work that ends in a device synchronise) and HIP events:
  delete   QdrantClient.delete by ticker filter, "A" then "B"
  rebuild  after each delete: recreate_collection + upsert of the survivors (ids, payloads and
           fp32 vectors held in host memory, in batches of BATCH (1M) points) in a second client
  scan     B = 32, k = 15 searches on the collection after both deletes and on the freshly
           rebuilt one (the same rows in the same order), WINDOWS (5) windows of ITERS (100)
           searches each, alternating
One JSON line per measurement, to stdout and appended to --out as it is taken."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "financial-rag-system_amd"))

from ragmi import qdrant_models as m  # noqa: E402
from ragmi.index import FlatIndex, plan_removal  # noqa: E402
from ragmi.qdrant import QdrantClient  # noqa: E402

D, B, K = 384, 32, 15
FILING = 64
OTHERS = 20
CHUNK = 1 << 20


def tickers_of(n, seed=7):
    """Ticker index per row: 0 = "A" (~1 % of the filings), 1 = "B" (~10 %), 2.. the others."""
    rng = np.random.default_rng(seed)
    n_f = -(-n // FILING)
    u = rng.random(n_f)
    t = 2 + rng.integers(0, OTHERS, n_f)
    t[u < 0.11] = 1
    t[u < 0.01] = 0
    return np.repeat(t, FILING)[:n].astype(np.int64)


def name_of(t):
    return "A" if t == 0 else "B" if t == 1 else f"T{t}"


def chunks(n, dev, seed=1000):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    for r0 in range(0, n, CHUNK):
        mm = min(CHUNK, n - r0)
        yield r0, mm, torch.randn((mm, D), generator=g, device=dev)


def timed(fn, repeats, warm=2):
    """Device ms of each of `repeats` calls of fn (an event pair around each), after warm-up."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
            "all_ms": [round(float(v), 4) for v in ms]}


class Out:
    def __init__(self, path):
        self.path = path
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        open(path, "w").close()

    def __call__(self, **rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(self.path, "a") as f:
            f.write(line + "\n")


def part1(n, dev, repeats, out):
    tick = tickers_of(n)
    tags = (tick + 1).astype(np.uint32)                   # the ticker's code, as PayloadTags deals
    idx = FlatIndex(D, n, dev)
    for r0, mm, x in chunks(n, dev):
        idx.upsert(x, torch.arange(r0, r0 + mm, device=dev), tags[r0:r0 + mm], new_count=r0 + mm)
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                   ctypes.c_void_p]
    stream = torch.cuda.current_stream(dev).cuda_stream
    for t in (0, 1):
        want = np.nonzero(tick == t)[0]
        rows, total = idx.select_rows(0xFFFF, t + 1)
        assert total == len(want) and np.array_equal(rows.cpu().numpy(), want)
        buf = torch.empty((total,), dtype=torch.int64, device=dev)
        cnt = timed(lambda: idx.select_rows(0xFFFF, t + 1, cap=0), repeats)
        emit = timed(lambda: idx.select_rows(0xFFFF, t + 1, cap=total, out=buf), repeats)
        for what, ms in (("count", cnt), ("emit", emit)):
            out(part="select", what=what, ticker=name_of(t), rows=n, matches=total,
                tag_bytes=4 * n, gb_per_s_of_tags=4 * n / np.median(ms) / 1e6,
                note="the call reads the total back, so each time includes that synchronise; "
                     "emit reads the tags twice (count, then emit) and writes 8 B per match",
                **stats(ms))
    for t in (0, 1):                                      # after every select: a move rewrites tags
        want = np.nonzero(tick == t)[0]
        total = len(want)
        src, dst, n1 = plan_removal(n, want)
        s_dev = torch.from_numpy(src).to(dev)
        d_dev = torch.from_numpy(dst).to(dev)
        moved = len(src)
        nbytes = moved * (D * 2 + 4)
        a = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        b = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        mv, cp = [], []
        for _ in range(repeats):                          # the two alternate
            mv += timed(lambda: idx.move_rows(s_dev, d_dev, n), 1, warm=1)
            cp += timed(lambda: hip.hipMemcpyAsync(b.data_ptr(), a.data_ptr(), nbytes, 3, stream),
                        1, warm=1)
        rate = lambda ms: 2 * nbytes / np.median(ms) / 1e6          # GB/s, read + write
        out(part="move", ticker=name_of(t), rows=n, deleted=total, moved=moved,
            bytes_read_plus_written=2 * nbytes, move_gb_per_s=rate(mv), memcpy_gb_per_s=rate(cp),
            fraction_of_memcpy=float(np.median(cp) / np.median(mv)),
            move=stats(mv), memcpy=stats(cp),
            note="move also reads 16 B of row indices per row; holes and movers lie in runs "
                 f"of up to {FILING} rows")
    idx.close()


def flt(ticker):
    return m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value=ticker))])


def part2(n, dev, batch, windows, iters, out):
    tick = tickers_of(n)
    host = np.empty((n, D), np.float32)                   # what the caller of a rebuild must hold
    vp = m.VectorParams(size=D, distance=m.Distance.COSINE, datatype="float16")
    a = QdrantClient(device=dev)
    a.create_collection("t", vp, capacity=n)
    for r0, mm, x in chunks(n, dev):
        host[r0:r0 + mm] = x.cpu().numpy()
        a.upsert("t", m.Batch(ids=list(range(r0, r0 + mm)), vectors=x,
                              payloads=[{"ticker": name_of(t), "n": r0 + i}
                                        for i, t in enumerate(tick[r0:r0 + mm].tolist())]))
    torch.cuda.synchronize()
    col = a._col("t")
    b = QdrantClient(device=dev)
    for ticker in ("A", "B"):
        before = len(col.row_ids)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        a.delete("t", m.FilterSelector(filter=flt(ticker)))
        e1.record()
        torch.cuda.synchronize()
        t_del = time.perf_counter() - t0
        after = len(col.row_ids)
        ids, pls = list(col.row_ids), list(col.payloads)  # the survivors, as their owner holds them
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.recreate_collection("t", vp, capacity=after)
        for r0 in range(0, after, batch):
            sel = ids[r0:r0 + batch]
            b.upsert("t", m.Batch(ids=sel, vectors=host[np.asarray(sel)], payloads=pls[r0:r0 + batch]))
        torch.cuda.synchronize()
        t_reb = time.perf_counter() - t0
        assert b.count("t").count == after and a.count("t", count_filter=flt(ticker)).count == 0
        out(part="delete_vs_rebuild", ticker=ticker, rows_before=before, deleted=before - after,
            fraction=(before - after) / before, delete_wall_s=t_del,
            delete_events_s=e0.elapsed_time(e1) / 1e3, rebuild_wall_s=t_reb,
            rebuild_over_delete=t_reb / t_del,
            note="the delete's wall time includes the host maps (ids, payloads, versions) of "
                 "the deleted and moved points; the rebuild's the host loop over every survivor")
    # the collection after both deletes against the one just rebuilt from its survivors
    q = torch.randn((B, D), generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    ia, ib = col.index, b._col("t").index
    sa, ra = ia.search(q, K)
    sb, rb = ib.search(q, K)
    torch.cuda.synchronize()
    assert torch.equal(ra, rb) and torch.equal(sa, sb), "deleted and rebuilt collections differ"

    def window(index):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            index.search(q, K)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    for index in (ia, ib):
        window(index)
    wa, wb = [], []
    for _ in range(windows):
        wa.append(window(ia))
        wb.append(window(ib))
    out(part="scan_after_delete", rows=ia.count, batch=B, k=K, iters_per_window=iters,
        after_delete_ms=[round(v, 4) for v in wa], rebuilt_ms=[round(v, 4) for v in wb],
        after_delete_median_ms=float(np.median(wa)), rebuilt_median_ms=float(np.median(wb)),
        results_identical=True)
    a.close()
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delete_10M.jsonl"))
    ap.add_argument("--parts", default="1,2")
    args = ap.parse_args()
    n = int(os.environ.get("ROWS", "10000000"))
    repeats = int(os.environ.get("REPEATS", "10"))
    dev = torch.device("cuda", 0)
    out = Out(args.out)
    out(part="setup", rows=n, dim=D, storage="fp16", filing_rows=FILING,
        device=torch.cuda.get_device_name(dev))
    if "1" in args.parts.split(","):
        part1(n, dev, repeats, out)
    if "2" in args.parts.split(","):
        part2(n, dev, int(os.environ.get("BATCH", str(CHUNK))),
              int(os.environ.get("WINDOWS", "5")), int(os.environ.get("ITERS", "100")), out)


if __name__ == "__main__":
    main()
