"""What a formula query costs on top of the batched search that feeds it.

ROWS (default 1M) x 384 fp16 seeded Gaussian rows on a FlatIndex with two key columns
(`ingested_at`, a datetime over two years, absent for one row in eight; `fiscal_year`, a number)
and a document-type tag; B = 32 requests of one prefetch each (a corpus row plus noise), C = 100
candidates, k = 15. In one process, alternating batch by batch after WARMUP (20) batches of each:
  search          FlatIndex.search(32 queries, k = C) alone
  search_recency  the same search, the arrangement of its lists into [B, 1, C], the gather of the
                  one key column the formula names and formula_rescore of rag's recency formula,
                  $score + 0.25 * exp_decay(ingested_at, now, 30 days) — the device work of
                  Collection.search_formula
  search_cond2    the same with $score + 0.1 * [document_type == 10-K and fiscal_year >= 2021]
                  + 0.25 * exp_decay(ingested_at) + 1e-4 * fiscal_year: one condition (tags
                  gathered) and two key columns
each timed by a HIP event pair around the call, ITERS (200) batches of each. The kernel's own
time: REPS (200) launches of rag_formula_rescore back to back on preallocated outputs between one
event pair, per launch, for either formula (an upper bound: it includes the gaps between
launches). One JSON line with the medians and the differences, to stdout and appended to --out
(default profiles/formula_timing.jsonl)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "financial-rag-system_amd"))

from ragmi import _lib  # noqa: E402
from ragmi import qdrant_models as m  # noqa: E402
from ragmi import rag  # noqa: E402
from ragmi.filters import KEY_ABSENT, PayloadRanges, PayloadTags  # noqa: E402
from ragmi.formula import compile_formula  # noqa: E402
from ragmi.index import FlatIndex, formula_rescore  # noqa: E402

D, B, C, K = 384, 32, 100, 15
CHUNK = 1 << 18
TYPES = ("10-K", "10-Q", "8-K")
T0_US, SPAN_US = 1_672_531_200_000_000, 2 * 365 * 86_400_000_000      # 2023-01-01, two years
NOW = "2025-01-01T00:00:00Z"


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(ts):
    return round(float(np.median(ts)), 4), [round(min(ts), 4), round(max(ts), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "formula_timing.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    pt, pr = PayloadTags(), PayloadRanges({"ingested_at": "datetime", "fiscal_year": "number"})
    codes = torch.tensor([pt.tag({"document_type": t}) for t in TYPES], dtype=torch.int64,
                         device=dev)
    idx = FlatIndex(D, args.rows, dev, storage="fp16")
    idx.keys_create(2)
    g = torch.Generator(device=dev)
    g.manual_seed(1000)
    q = None
    for r0 in range(0, args.rows, CHUNK):
        n = min(CHUNK, args.rows - r0)
        x = torch.randn((n, D), generator=g, device=dev)
        if q is None:
            q = (x[:B] + 0.5 * torch.randn((B, D), generator=g, device=dev)).contiguous()
        rows = torch.arange(r0, r0 + n, device=dev)
        tags = codes[torch.randint(0, 3, (n,), generator=g, device=dev)].to(torch.int32)
        idx.upsert(x, rows, tags, new_count=r0 + n)
        # the key of a positive double is its bit pattern (ragmi.filters.key_of_float)
        us = (T0_US + torch.randint(0, SPAN_US, (n,), generator=g, device=dev)).double()
        at = us.view(torch.int64).clone()
        at[torch.randint(0, 8, (n,), generator=g, device=dev) == 0] = KEY_ABSENT
        year = torch.randint(2018, 2025, (n,), generator=g, device=dev).double().view(torch.int64)
        idx.write_keys(0, rows, at)
        idx.write_keys(1, rows, year)
    torch.cuda.synchronize()

    recency = rag._recency(None, (30, 0.25), NOW, None, K, None, None, None)[0]
    decay = recency.formula.sum[1]
    cond = m.Filter(must=[
        m.FieldCondition(key="document_type", match=m.MatchValue(value="10-K")),
        m.FieldCondition(key="fiscal_year", range=m.Range(gte=2021))])
    cond2 = m.FormulaQuery(
        formula=m.SumExpression(sum=["$score", m.MultExpression(mult=[0.1, cond]), decay,
                                     m.MultExpression(mult=[1e-4, "fiscal_year"])]),
        defaults=recency.defaults)
    compiled = {"recency": compile_formula(recency, None, 1, pt, pr),
                "cond2": compile_formula(cond2, None, 1, pt, pr)}
    blobs = {n: torch.from_numpy(f.blob().view(np.int32)).to(dev) for n, f in compiled.items()}
    ncand = torch.full((B, 1), min(C, args.rows), dtype=torch.int32, device=dev)

    def search():
        return idx.search(q, C)

    def search_formula(name):
        f = compiled[name]
        s, ids = idx.search(q, C)
        s, ids = s.reshape(B, 1, C), ids.reshape(B, 1, C)
        tags = idx.gather_tags(ids) if f.has_cond else None
        keys = {c: idx.gather_keys(c, ids) for c in f.columns}
        return formula_rescore(s, ids, blobs[name], K, ncand, tags, keys)

    for name, f in compiled.items():                 # every request is answered
        s, r, status = search_formula(name)
        assert not bool(status.any()) and bool((r >= 0).all()), name
    for _ in range(args.warmup):
        search()
        search_formula("recency")
        search_formula("cond2")
    torch.cuda.synchronize()
    t = {"search": [], "recency": [], "cond2": []}
    for _ in range(args.iters):
        t["search"].append(event_ms(search))
        t["recency"].append(event_ms(lambda: search_formula("recency")))
        t["cond2"].append(event_ms(lambda: search_formula("cond2")))

    # the kernel alone: raw launches on fixed buffers
    lib = _lib.load()
    s, ids = idx.search(q, C)
    s, ids = s.reshape(B, 1, C).contiguous(), ids.reshape(B, 1, C).contiguous()
    tags = idx.gather_tags(ids)
    cols = [idx.gather_keys(c, ids) for c in range(2)]
    ptrs = (ctypes.c_void_p * 4)(cols[0].data_ptr(), cols[1].data_ptr(), None, None)
    out_s = torch.empty((B, K), dtype=torch.float32, device=dev)
    out_r = torch.empty((B, K), dtype=torch.int64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    kernel = {}
    for name, blob in blobs.items():
        def launches(n=args.reps, blob=blob):
            for _ in range(n):
                rc = lib.rag_formula_rescore(
                    s.data_ptr(), ids.data_ptr(), tags.data_ptr(), ptrs, ncand.data_ptr(),
                    blob.data_ptr(), blob.numel(), B, 1, C, K, out_s.data_ptr(),
                    out_r.data_ptr(), None, status.data_ptr(), stream)
                assert rc == 0
        launches(20)
        torch.cuda.synchronize()
        kernel[name] = [event_ms(launches) / args.reps for _ in range(5)]

    a, a_mm = med(t["search"])
    b, b_mm = med(t["recency"])
    c, c_mm = med(t["cond2"])
    rec = {"bench": "formula", "rows": args.rows, "dim": D, "storage": "fp16", "B": B, "L": 1,
           "C": C, "k": K, "warmup": args.warmup, "iters": args.iters,
           "search_ms": a, "search_ms_min_max": a_mm,
           "search_recency_ms": b, "search_recency_ms_min_max": b_mm,
           "recency_extra_ms": round(b - a, 4), "recency_ops": len(compiled["recency"].ops),
           "search_cond2_ms": c, "search_cond2_ms_min_max": c_mm,
           "cond2_extra_ms": round(c - a, 4), "cond2_ops": len(compiled["cond2"].ops),
           "kernel_reps": args.reps,
           "kernel_recency_us": round(1e3 * float(np.median(kernel["recency"])), 2),
           "kernel_cond2_us": round(1e3 * float(np.median(kernel["cond2"])), 2),
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
