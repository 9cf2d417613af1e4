"""Coalescer — concurrent single-query searches riding one GPU scan (host-only logic)."""
from __future__ import annotations

import threading
import time

import numpy as np


class _Req:
    __slots__ = ("q", "limit", "filt", "result", "exc", "wake", "lead")

    def __init__(self, q, limit, filt):
        self.q, self.limit, self.filt = q, limit, filt
        self.result = self.exc = None
        self.wake = threading.Event()
        self.lead = False


class Coalescer:
    """Rides concurrent single-query searches on one GPU scan.

    The reference's batched service still searches per request: main2.py's batch_processor
    fans a micro-batch out to process_independently tasks that each call
    retrieve_from_qdrant -> query_points from an asyncio.to_thread worker (<= 25 at once,
    main2.py:52-53,218,228). Unchanged, that is one full-corpus scan per query. Here the
    first caller becomes the LEADER and searches; callers arriving while a search runs queue
    up, and the next leader (the oldest queued request) searches all of them in ONE batched
    scan (per-query payload filters ride inside the kernel). With no concurrency a request
    runs at once (no added latency); `window_s` > 0 additionally holds a leader back for up
    to that long to gather more callers. Results are bit-identical to individual calls: every
    query's top-k is exact, independent of its batch-mates (tests/test_coalesce_gpu.py)."""

    def __init__(self, col, window_s: float = 0.0, max_batch: int = 32, search=None):
        self.col = col
        # what a leader calls for its batch: col.search (rows and scores), or for a Collection
        # its search_points, whose hits are resolved to points before the collection's lock is
        # released — a rider must not look rows up after a delete may have moved them
        self.search_fn = search
        self.window = float(window_s)
        self.max_batch = int(max_batch)
        self.lock = threading.Lock()
        self.pending: list[_Req] = []
        self.leader_active = False
        self.batches = 0            # scans issued (stats)
        self.requests = 0

    def search(self, q: np.ndarray, limit: int, filt):
        req = _Req(q, int(limit), filt)
        with self.lock:
            self.pending.append(req)
            self.requests += 1
            if not self.leader_active:
                self.leader_active = True
                req.lead = True
        if not req.lead:
            req.wake.wait()
            if not req.lead:                       # served by another leader
                if req.exc is not None:
                    raise req.exc
                return req.result
        batch: list[_Req] = []
        fatal = None
        try:
            if self.window > 0:
                t_end = time.perf_counter() + self.window
                while time.perf_counter() < t_end:
                    with self.lock:
                        if len(self.pending) >= self.max_batch:
                            break
                    time.sleep(min(5e-5, self.window / 4))
            with self.lock:
                batch = self.pending[:self.max_batch]
                del self.pending[:self.max_batch]
                self.batches += 1
            hits = (self.search_fn or self.col.search)(
                np.stack([r.q for r in batch]), max(r.limit for r in batch),
                [r.filt for r in batch])
            for r, h in zip(batch, hits):
                r.result = h[:r.limit]
        except BaseException as e:                 # every rider sees the failure
            for r in batch:
                r.exc = e
            if not isinstance(e, Exception):       # KeyboardInterrupt, SystemExit: re-raise
                fatal = e                          # after the hand-off below
        finally:
            # whatever was raised: hand leadership on and wake every rider, so no caller of
            # this collection can block forever behind a leader that is gone
            with self.lock:
                if req in self.pending:            # interrupted before taking the batch
                    self.pending.remove(req)
                if self.pending:                   # hand leadership to the oldest waiter
                    nxt = self.pending[0]
                    nxt.lead = True
                    nxt.wake.set()
                else:
                    self.leader_active = False
            for r in batch:
                if r is not req:
                    r.wake.set()
        if fatal is not None:
            raise fatal
        if req.exc is not None:
            raise req.exc
        return req.result
