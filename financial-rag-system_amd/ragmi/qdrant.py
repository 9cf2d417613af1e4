"""QdrantClient-shaped front end of the in-HBM flat index.

Drop-in for the calls the reference makes on `qdrant_client.QdrantClient`:
  get_collections()                       main.py:135, main2.py:337 (/ready)
  collection_exists(name)                 ingest.py:87, database.py:121
  create_collection(name, vectors_config) ingest.py:89-95, database.py:122-128
  upsert(name, points=[PointStruct])      ingest.py:171-175
  query_points(name, query, limit, query_filter) -> .points[i].{id,score,payload}
                                          main.py:232-237, main2.py:163
plus query_batch_points (one GPU scan for a whole micro-batch; main2.py:281-295 stage 2),
count (also filtered), retrieve, delete (by ids or by filter) and delete_collection.

`url` is accepted and ignored: the collection lives in this process's GPU memory (the
Qdrant service of docker-compose.yml:22 is replaced, not contacted). `path=` plays the role
of Qdrant's local mode / storage volume: existing collections under it are loaded at
construction and `save()` / `close()` write them back (ragmi.store shard format). Payloads stay host-side
keyed by row; the keyword payload fields used by the reference's `must` filter (`ticker`,
`document_type`, main.py:218-230) are dictionary-coded into a per-row uint32 tag in HBM
(16 bits per field) so filtering runs inside the scan kernel.
"""
from __future__ import annotations

import itertools
import os
import shutil
import threading
import time
import uuid
from typing import Any, Iterable

import numpy as np
import torch

from . import groups
from . import qdrant_models as models
from .filters import MAX_PROGRAMS, FilterProgram, UnsupportedFilter, compile_program, pack_view
from .index import (FUSION_MAX_ENTRIES, FUSION_MAX_LISTS, GROUPS_MAX, GROUPS_MAX_CELLS, MAX_K,
                    MMR_MAX_CANDIDATES, FlatIndex, fuse_rrf)
from .shardset import ShardSet, parse_devices

DEFAULT_TAG_FIELDS = ("ticker", "document_type")


def _norm_id(pid):
    """Qdrant point ids are unsigned ints or UUIDs; 32-hex md5 digests (ingest.py:151-154)
    are accepted as UUIDs and reported back in canonical dashed form."""
    if isinstance(pid, bool):
        raise ValueError("point id must be int or UUID string")
    if isinstance(pid, (int, np.integer)):
        if pid < 0:
            raise ValueError("integer point ids must be unsigned")
        return int(pid)
    if isinstance(pid, uuid.UUID):
        return str(pid)
    if isinstance(pid, str):
        return str(uuid.UUID(pid))
    raise ValueError(f"unsupported point id type {type(pid)!r}")


class PayloadTags:
    """Dictionary-codes up to two keyword payload fields into a per-row uint32 tag
    (16 bits per field, code 0 = field absent) and compiles Qdrant `must` filters on those
    fields into (mask, value) so the GPU scan filters with (tag & mask) == value.
    Host-only logic (no device code)."""

    def __init__(self, fields=DEFAULT_TAG_FIELDS):
        if len(fields) > 2:
            raise ValueError("at most two indexed keyword payload fields (16 bits each)")
        self.fields = tuple(fields)
        self.codes: list[dict[Any, int]] = [dict() for _ in self.fields]

    def code(self, f: int, value, create: bool) -> int | None:
        if isinstance(value, (list, dict)) or value is None:
            return None
        table = self.codes[f]
        c = table.get(value)
        if c is None and create:
            if len(table) >= 0xFFFF:
                raise OverflowError(f"more than 65535 distinct values for {self.fields[f]}")
            c = len(table) + 1          # 0 = field absent
            table[value] = c
        return c

    def value_of(self, f: int, code: int):
        """The payload value behind code `code` of field f, the reverse of `code`: codes are
        handed out in insertion order (1, 2, ...) and a dict keeps that order, so no second
        table is kept."""
        table = self.codes[f]
        if not 1 <= code <= len(table):
            raise KeyError(f"no value with code {code} for {self.fields[f]}")
        return next(itertools.islice(table, code - 1, None))

    def tag(self, payload: dict | None) -> int:
        tag = 0
        if payload:
            for f, key in enumerate(self.fields):
                if key in payload:
                    c = self.code(f, payload[key], create=True)
                    if c:
                        tag |= c << (16 * f)
        return tag

    def compile(self, flt: models.Filter | None):
        """Filter(must=[FieldCondition(key, MatchValue(v))...]) -> (mask, value); None when
        nothing can match (a value never ingested); (0, 0) for no filter."""
        if flt is None:
            return (0, 0)
        if flt.should or flt.must_not:
            raise UnsupportedFilter("only `must` conditions are supported (main.py:218-236)")
        mask = value = 0
        for cond in flt.must or []:
            if not isinstance(cond, models.FieldCondition) or cond.range is not None:
                raise UnsupportedFilter("only FieldCondition(key, match=MatchValue) is supported")
            if cond.key not in self.fields:
                raise UnsupportedFilter(
                    f"payload key {cond.key!r} is not an indexed keyword field "
                    f"{self.fields}; create the collection with payload_tag_fields")
            if not isinstance(cond.match, models.MatchValue):
                raise UnsupportedFilter("only MatchValue matches are supported")
            f = self.fields.index(cond.key)
            c = self.code(f, cond.match.value, create=False)
            if c is None:
                return None
            m = 0xFFFF << (16 * f)
            if mask & m and (value & m) != (c << (16 * f)):
                return None             # two different values for one field
            mask |= m
            value |= c << (16 * f)
        return (mask, value)


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
    query's top-k is exact, independent of its batch-mates (tests/test_qdrant_gpu.py)."""

    def __init__(self, col: "Collection", window_s: float = 0.0, max_batch: int = 32,
                 search=None):
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


def parse_selector(points_selector):
    """The `points_selector` of QdrantClient.delete -> ("ids", [normalised ids]) or
    ("filter", Filter): a plain list of ids, a PointIdsList, a FilterSelector or a bare
    Filter."""
    sel = points_selector
    if isinstance(sel, models.FilterSelector):
        if sel.filter is None:
            raise ValueError("FilterSelector needs a filter")
        return "filter", sel.filter
    if isinstance(sel, models.Filter):
        return "filter", sel
    if isinstance(sel, models.PointIdsList):
        sel = sel.points
    if isinstance(sel, (str, bytes, dict)) or not hasattr(sel, "__iter__"):
        raise ValueError("points_selector must be a list of ids, a PointIdsList, a "
                         "FilterSelector or a Filter")
    return "ids", [_norm_id(pid) for pid in sel]


def _storage_of(vectors_config) -> str:
    """VectorParams.datatype -> FlatIndex storage. Qdrant stores Float32 unless told otherwise
    (the reference never sets a datatype, database.py:124-130, ingest.py:89-95), so the
    default is fp32 storage: exact scores on the fp32 rows, the scan on their fp16 copy."""
    dt = getattr(vectors_config, "datatype", None)
    dt = getattr(dt, "value", dt)
    if dt is None or str(dt).lower() == "float32":
        return "fp32"
    if str(dt).lower() == "float16":
        return "fp16"
    raise NotImplementedError(f"vector datatype {dt!r} (float32 and float16 are supported)")


class Collection:
    """One COSINE collection: FlatIndex in HBM + host-side id/payload maps. With `devices`
    (one device index per shard, ragmi.shardset.parse_devices) the rows are striped over a
    ShardSet instead; rows, ids, payloads and tags stay global and host-side either way."""

    def __init__(self, name: str, dim: int, device, tag_fields=DEFAULT_TAG_FIELDS,
                 capacity: int = 1024, storage: str = "fp32", devices=None):
        self.name = name
        self.dim = dim
        self.tags = PayloadTags(tag_fields)
        devices = parse_devices(devices)
        self.index = (ShardSet(dim=dim, devices=devices, capacity=capacity, storage=storage)
                      if devices is not None else
                      FlatIndex(dim=dim, capacity=capacity, device=device, storage=storage))
        self.id_to_row: dict[Any, int] = {}
        self.row_ids: list[Any] = []
        self.payloads: list[dict | None] = []
        self.versions: list[int] = []
        self.op = 0
        self._unanswered = 0     # index.unanswered() as last read (Collection.search)
        self.rescued = 0         # queries re-answered on the full exact pass (stats)
        self.group_stats = {}    # routes grouped searches took (ragmi.groups.search_groups)
        self.lock = threading.RLock()
        # 32 queries per scan pass at D = 384, 4 groups of 32 at D = 1024 (ragmi.h)
        self.coalescer = Coalescer(self, 0.0, 32 if dim <= 384 else 128,
                                   search=self.search_points)

    def compile_filter(self, flt):
        """A Filter as the searches take it: the (mask, value) pair of PayloadTags.compile for
        every filter it accepts (today's path, untouched), else a FilterProgram
        (ragmi.filters.compile_program: should, must_not, min_should, MatchAny, MatchExcept,
        is-empty, nested filters); None when nothing can match. A filter neither accepts is
        refused with the general compiler's message, which names the cause. A filter with
        `min_should` goes to the general compiler at once: PayloadTags.compile never looked
        at that clause."""
        if getattr(flt, "min_should", None) is not None:
            return compile_program(self.tags, flt)
        try:
            return self.tags.compile(flt)
        except UnsupportedFilter:
            return compile_program(self.tags, flt)

    def _legacy_only(self, flt, what: str):
        """PayloadTags.compile for a route that takes no general filter yet: its refusal says
        that the route is the reason when the filter algebra would have accepted the filter."""
        try:
            if getattr(flt, "min_should", None) is not None:
                raise UnsupportedFilter("min_should is not a `must` condition")
            return self.tags.compile(flt)
        except UnsupportedFilter as e:
            compile_program(self.tags, flt)        # refused by both: the general message
            raise UnsupportedFilter(
                f"{what} takes only Filter(must=[FieldCondition(key, match=MatchValue)]); "
                f"general filters (should, must_not, MatchAny, ...) are out of scope here: {e}"
            ) from e

    # ---------------------------------------------------------------- writes
    def upsert(self, ids: list, vectors, payloads: list) -> int:
        with self.lock:
            self.op += 1
            vec = np.asarray(vectors, dtype=np.float32) if not isinstance(
                vectors, torch.Tensor) else vectors
            if vec.ndim != 2 or vec.shape[1] != self.dim:
                raise ValueError(f"vectors must be [n, {self.dim}]")
            # last write wins for duplicate ids inside one batch (Qdrant semantics)
            last: dict[Any, int] = {}
            for i, pid in enumerate(ids):
                last[_norm_id(pid)] = i
            rows, sel, tags = [], [], []
            new_count = len(self.row_ids)
            for pid, i in last.items():
                r = self.id_to_row.get(pid)
                if r is None:
                    r = new_count
                    new_count += 1
                    self.id_to_row[pid] = r
                    self.row_ids.append(pid)
                    self.payloads.append(None)
                    self.versions.append(0)
                p = payloads[i] if payloads is not None else None
                self.payloads[r] = dict(p) if p is not None else None
                self.versions[r] = self.op
                rows.append(r)
                sel.append(i)
                tags.append(self.tags.tag(p))
            if new_count > self.index.capacity:
                self.index.reserve(max(new_count, 2 * self.index.capacity))
            if rows:
                sel_t = vec[sel] if isinstance(vec, torch.Tensor) else vec[np.asarray(sel)]
                self.index.upsert(sel_t, np.asarray(rows, dtype=np.int64),
                                  np.asarray(tags, dtype=np.uint32), new_count=new_count)
            return self.op

    def delete(self, points_selector) -> int:
        """Remove the selected points (parse_selector). Unknown ids are ignored, duplicates
        collapse, a filter on a never-ingested value selects nothing; a filter is resolved on
        the device (select_rows over the tags), never by walking the payloads. The rows are
        removed from the index by the removal rule (ragmi.index.plan_removal) and the same
        (src, dst) moves are applied to the host maps: a moved point keeps its id, payload
        and version. Returns the operation id. The device work has finished on return."""
        kind, what = parse_selector(points_selector)
        with self.lock:
            # may refuse the filter
            flt = self._legacy_only(what, "Collection.delete") if kind == "filter" else None
            self.op += 1
            if kind == "ids":
                found = {self.id_to_row[pid] for pid in what if pid in self.id_to_row}
                rows = np.fromiter(found, dtype=np.int64, count=len(found))
            else:
                if flt is None or not self.row_ids:
                    rows = np.empty(0, np.int64)
                elif flt == (0, 0):
                    rows = np.arange(len(self.row_ids), dtype=np.int64)
                else:
                    rows = self.index.select_rows(flt[0], flt[1])[0].cpu().numpy()
            if rows.size:
                src, dst, n1 = self.index.remove_rows(rows)
                self._apply_removal(rows, src, dst, n1)
                torch.cuda.current_stream(self.index.device).synchronize()
            return self.op

    def _apply_removal(self, rows, src, dst, n1: int) -> None:
        """The host side of a removal: forget the deleted rows' ids, give every moved row's
        id, payload and version its new slot, truncate to the new count."""
        for r in rows.tolist():
            del self.id_to_row[self.row_ids[r]]
        for s, d in zip(src.tolist(), dst.tolist()):
            pid = self.row_ids[s]
            self.row_ids[d] = pid
            self.payloads[d] = self.payloads[s]
            self.versions[d] = self.versions[s]
            self.id_to_row[pid] = d
        del self.row_ids[n1:], self.payloads[n1:], self.versions[n1:]

    # ---------------------------------------------------------------- reads
    def count_matching(self, flt) -> int:
        """Points a Filter matches, counted on the device (select_rows with cap = 0)."""
        with self.lock:
            c = self.compile_filter(flt)
            if c is None or not self.row_ids:
                return 0
            if c == (0, 0):
                return len(self.row_ids)
            if isinstance(c, FilterProgram):
                return self.index.select_rows_view(pack_view([c]), cap=0)[1]
            return self.index.select_rows(c[0], c[1], cap=0)[1]

    def search_points(self, queries, limit: int, filters: list, with_vectors=False):
        """search with every hit resolved to its ScoredPoint (payload attached) under the same
        hold of the lock as the search that produced it: a delete moves rows, so a row number
        means a point only while the lock is held. What query_points, query_batch_points and
        the coalescer's leaders call."""
        with self.lock:
            return [[self.point(r, s, True, with_vectors) for r, s in h]
                    for h in self.search(queries, limit, filters)]

    def search(self, queries, limit: int, filters: list):
        """queries [B, dim]; filters: per query compiled filter ((mask, value) or None)."""
        with self.lock:
            B = len(filters)
            if limit < 1:
                return [[] for _ in range(B)]
            # Qdrant answers any limit with at most the collection's points (main.py:215,
            # 232-237): k <= 32 on the scan, <= 4096 on the large-k pass, beyond that on the
            # full exact pass (rag_index_search)
            k = min(limit, max(1, self.index.count))
            live = [i for i, f in enumerate(filters) if f is not None]
            out = [[] for _ in range(B)]
            if not live or self.index.count == 0:
                return out
            s, ids = self._lists(queries, filters, live, k)
            s = s.cpu().numpy()
            ids = ids.cpu().numpy()
            for j, i in enumerate(live):
                out[i] = [(int(r), float(sc)) for r, sc in zip(ids[j], s[j]) if r >= 0]
            return out

    def _lists(self, queries, filters: list, live: list, k: int):
        """The exact top-k lists of the `live` requests. Every live filter a (mask, value)
        pair: the path of every release so far, unchanged. Otherwise the view path
        (_view_lists)."""
        if not any(isinstance(filters[i], FilterProgram) for i in live):
            q, use = self._live_queries(queries, filters, live)
            return self._exact_lists(q, k, use)
        return self._view_lists(queries, filters, live, k)

    def _view_lists(self, queries, filters: list, live: list, k: int):
        """_lists with general filters among the live ones: the batch's distinct programs
        share view bits (a (mask, value) pair rides as its one-atom MASKEQ program; (0, 0)
        needs no bit, over any view it passes every row), every query gets the filter
        (1 << slot, 1 << slot), and one view search answers the batch. More than MAX_PROGRAMS
        distinct programs: the queries are dealt into calls of at most that many, each query
        into the first call that knows its program or has a free bit, and the results are
        scattered back."""
        q = queries if isinstance(queries, torch.Tensor) else np.asarray(queries, np.float32)
        q = q[live] if len(live) != len(filters) else q
        calls: list = []                       # (slots: {program: bit}, members, their filters)
        for j, i in enumerate(live):
            f = filters[i]
            prog = (f if isinstance(f, FilterProgram) else
                    None if tuple(f) == (0, 0) else FilterProgram.maskeq(*f))
            for slots, members, fl in calls:
                if prog is None or prog in slots or len(slots) < MAX_PROGRAMS:
                    break
            else:
                slots, members, fl = {}, [], []
                calls.append((slots, members, fl))
            bit = 0 if prog is None else 1 << slots.setdefault(prog, len(slots))
            members.append(j)
            fl.append((bit, bit))
        s = ids = None
        for slots, members, fl in calls:
            # every call holds a program: a call is opened for a query that brings one, except
            # the first, and a batch without any program never comes here
            blob = pack_view(list(slots))
            use = np.asarray(fl, dtype=np.uint32).reshape(-1, 2)
            if len(calls) == 1:
                return self._exact_lists(q, k, use, programs=blob)
            s1, i1 = self._exact_lists(q[members], k, use, programs=blob)
            if s is None:
                s = torch.empty((len(live), k), dtype=s1.dtype, device=s1.device)
                ids = torch.empty((len(live), k), dtype=i1.dtype, device=i1.device)
            sel = torch.as_tensor(members, device=s1.device)
            s[sel] = s1
            ids[sel] = i1
        return s, ids

    @staticmethod
    def _live_queries(queries, filters: list, live: list):
        """The queries of the `live` requests and their compiled filters as the index takes
        them ([n, 2] uint32, or None when no request filters)."""
        q = queries if isinstance(queries, torch.Tensor) else np.asarray(queries, np.float32)
        q = q[live] if len(live) != len(filters) else q
        fl = np.asarray([filters[i] for i in live], dtype=np.uint32).reshape(-1, 2)
        return q, (fl if fl.any() else None)

    def _exact_lists(self, q, k: int, use, programs=None):
        """The exact top-k lists (scores, rows) of queries `q`, as the index's tensors, with
        every query a large-k pass left unanswered re-answered on the full exact pass. What
        search reports and what the MMR path re-selects from. Called under the lock.
        `programs`: a filter-program blob; `use` then indexes the bits of its view, and the
        re-run takes the same blob."""
        view = {} if programs is None else {"programs": programs}
        if isinstance(self.index, ShardSet):
            # a shard that left a query unanswered hands the merge an all -1 list, which
            # the merged top-k does not show: the set reads its per-shard flags and
            # re-answers those queries itself (ShardSet.search, rescue)
            before = self.index.rescued
            s, ids = self.index.search(q, k, filters=use, rescue=True, **view)
            self.rescued += self.index.rescued - before
            return s, ids
        s, ids = self.index.search(q, k, filters=use, **view)
        short = (ids < 0).any(dim=1)
        if bool(short.any()):
            # a -1 is padding (fewer matching points than k) unless the pass left the
            # query unanswered (tier 3: more than 16384 rows tied within the error band
            # of its k-th best on the large-k pass). Only then, re-run those queries on
            # the full exact pass: an unanswered query must never read as "no documents"
            # (ADVICE r5).
            n_un = self.index.unanswered()
            if n_un > self._unanswered:
                redo = torch.nonzero(short).reshape(-1).tolist()
                s2, i2 = self.index.search(q[redo], k, filters=use[redo] if use is not None
                                           else None, full=True, **view)
                s[redo] = s2
                ids[redo] = i2
                self.rescued += len(redo)
            self._unanswered = n_un
        return s, ids

    def search_mmr(self, queries, limits, filters: list, diversity, candidates):
        """search with MMR re-selection, per request b: limits[b] hits chosen at diversity[b]
        from its candidates[b] nearest points (clamped to the collection's count) — one
        search at C = the largest of them, one MMR launch with per-query candidate counts.
        A request at diversity 0 with candidates = its limit is the plain search. Returns
        per request [(row, score)] in selection order."""
        with self.lock:
            B = len(filters)
            out = [[] for _ in range(B)]
            count = self.index.count
            live = [i for i, f in enumerate(filters) if f is not None and limits[i] >= 1]
            if not live or count == 0:
                return out
            ncand = np.minimum(np.asarray([candidates[i] for i in live], np.int64), count)
            ncand = np.maximum(ncand, 1).astype(np.int32)
            lim = [int(limits[i]) for i in live]
            C = int(ncand.max())
            k = min(max(lim), C)
            s, ids = self._lists(queries, filters, live, C)
            s, ids = self.index.mmr(s, ids, k, np.asarray([diversity[i] for i in live],
                                                          np.float32), ncand)
            s = s.cpu().numpy()
            ids = ids.cpu().numpy()
            for j, i in enumerate(live):
                out[i] = [(int(r), float(sc)) for r, sc in zip(ids[j], s[j]) if r >= 0][:lim[j]]
            return out

    def search_points_mmr(self, queries, limits, filters: list, diversity, candidates,
                          with_vectors=False):
        """search_mmr with every hit resolved to its ScoredPoint under the same hold of the
        lock (see search_points)."""
        with self.lock:
            return [[self.point(r, s, True, with_vectors) for r, s in h]
                    for h in self.search_mmr(queries, limits, filters, diversity, candidates)]

    def search_fusion(self, requests: list):
        """Fusion queries. `requests`: per request (rrf_k, [(vector, Filter or
        None, limit), ...], limit), as fusion_params returns them. Every prefetch of every
        request rides one batched search at C = the largest prefetch limit (clamped to the
        collection's count); the lists are arranged [B, Lmax, C] on the device, each cut to
        its own limit by ncand, and fused by rag_fuse_rrf in one launch per distinct rrf_k. A
        prefetch whose filter can match nothing, or whose limit is < 1, is an empty list and
        is not searched. Returns per request [(row, fused score)], best first."""
        with self.lock:
            out = [[] for _ in requests]
            count = self.index.count
            # every filter is compiled, so that a refusal does not depend on the limits
            compiled = [[self.compile_filter(f) for _, f, _ in pres] for _, pres, _ in requests]
            qs, filters, where = [], [], []          # the searched prefetches, flattened
            for b, (_, pres, limit) in enumerate(requests):
                if limit < 1 or count == 0:
                    continue
                for l, (vec, _, plim) in enumerate(pres):
                    if compiled[b][l] is not None and plim >= 1:
                        qs.append(vec)
                        filters.append(compiled[b][l])
                        where.append((b, l, min(plim, count)))
            if not qs:
                return out
            live = sorted({b for b, _, _ in where})
            slot = {b: j for j, b in enumerate(live)}
            Lmax = max(len(requests[b][1]) for b in live)
            C = max(n for _, _, n in where)
            if Lmax * C > FUSION_MAX_ENTRIES:
                raise ValueError(f"fusion: {Lmax} prefetches of up to {C} hits are {Lmax * C} "
                                 f"entries; at most {FUSION_MAX_ENTRIES} (prefetches x the "
                                 "largest prefetch limit) are fused")
            _, ids = self._lists(_stack_queries(qs, self.dim), filters, list(range(len(qs))), C)
            dev = ids.device
            rows = torch.full((len(live), Lmax, C), -1, dtype=torch.int64, device=dev)
            at = np.asarray([(slot[b], l) for b, l, _ in where], dtype=np.int64)
            rows[torch.from_numpy(at[:, 0]).to(dev), torch.from_numpy(at[:, 1]).to(dev)] = ids
            ncand = np.zeros((len(live), Lmax), dtype=np.int32)
            ncand[at[:, 0], at[:, 1]] = [n for _, _, n in where]
            lim = [int(requests[b][2]) for b in live]
            k = min(max(lim), Lmax * C)
            by_k: dict[int, list] = {}
            for j, b in enumerate(live):
                by_k.setdefault(requests[b][0], []).append(j)
            for rrf_k, members in by_k.items():
                if len(members) == len(live):
                    s, r = fuse_rrf(rows, k, rrf_k, ncand)
                else:
                    sel = torch.as_tensor(members, device=dev)
                    s, r = fuse_rrf(rows[sel], k, rrf_k, ncand[members])
                s = s.cpu().numpy()
                r = r.cpu().numpy()
                for m, j in enumerate(members):
                    out[live[j]] = [(int(x), float(sc)) for x, sc in zip(r[m], s[m])
                                    if x >= 0][:lim[j]]
            return out

    def search_points_fusion(self, requests: list, with_vectors=False):
        """search_fusion with every hit resolved to its ScoredPoint (score = the fused score)
        under the same hold of the lock (see search_points)."""
        with self.lock:
            return [[self.point(r, s, True, with_vectors) for r, s in h]
                    for h in self.search_fusion(requests)]

    def search_groups(self, queries, group_by: str, limit: int, group_size: int, filters: list,
                      with_vectors=False, candidates: int | None = None,
                      widen: int | None = None):
        """Grouped search (ragmi.groups.search_groups): per request the `limit`
        best groups of points sharing a value of tag field `group_by`, each with its
        `group_size` best hits — exact, whatever `candidates` / `widen` (policy) say. Returns
        per request a list of PointGroup (id = the payload value) whose hits are resolved to
        ScoredPoints under the same hold of the lock (see search_points). The route counters
        accumulate in `group_stats`."""
        if group_by not in self.tags.fields:
            raise UnsupportedFilter(
                f"group_by {group_by!r} is not an indexed keyword field {self.tags.fields}; "
                "create the collection with payload_tag_fields")
        f = self.tags.fields.index(group_by)
        shift = 16 * f
        key_mask = 0xFFFF << shift
        with self.lock:
            B = len(filters)
            out = [[] for _ in range(B)]
            count = self.index.count
            codes = self.tags.codes[f]
            live = [i for i, fl in enumerate(filters) if fl is not None]
            if any(isinstance(filters[i], FilterProgram) for i in live):
                raise UnsupportedFilter(
                    "query_points_groups takes only Filter(must=[FieldCondition(key, "
                    "match=MatchValue)]); a grouped search under a general filter (should, "
                    "must_not, MatchAny, ...) is out of scope: its exactness ladder composes "
                    "(mask, value) pairs")
            if limit < 1 or group_size < 1 or not live or count == 0 or not codes:
                return out
            # neither clamp can change a result: there are no more groups than codes, no
            # more hits than points
            G, S = min(int(limit), len(codes)), min(int(group_size), count)
            if G > GROUPS_MAX or G * S > GROUPS_MAX_CELLS:
                raise ValueError(f"grouped search: at most {GROUPS_MAX} groups and "
                                 f"{GROUPS_MAX_CELLS} hits in all (limit x group_size)")
            every = [c << shift for c in codes.values()]
            possible = [[filters[i][1] & key_mask] if filters[i][0] & key_mask else every
                        for i in live]
            q, use = self._live_queries(queries, filters, live)
            res = groups.search_groups(self.index, q, use, key_mask, possible, G, S, candidates,
                                       widen, search=self._exact_lists, stats=self.group_stats)
            for i, found in zip(live, res):
                out[i] = [models.PointGroup(
                    hits=[self.point(r, s, True, with_vectors) for r, s in hits],
                    id=self.tags.value_of(f, key >> shift)) for key, hits in found]
            return out

    def point(self, row: int, score: float, with_payload=True, with_vectors=False):
        payload = self.payloads[row] if with_payload else None
        vec = None
        if with_vectors:
            vec = (self.index.export_rows32(row, 1)[0] if self.index.storage == "fp32" else
                   self.index.export_rows(row, 1)[0].view(np.float16).astype(np.float32)).tolist()
        return models.ScoredPoint(id=self.row_ids[row], version=self.versions[row],
                                  score=score, payload=payload, vector=vec)


MMR_DIVERSITY = 0.5          # Mmr(diversity=None)
MMR_CANDIDATES = 100         # Mmr(candidates_limit=None): max(limit, this)


def nearest_of(query):
    """A query argument -> (vector, Mmr or None): a NearestQuery is unwrapped, anything else is
    the vector itself."""
    if isinstance(query, models.NearestQuery):
        return query.nearest, query.mmr
    return query, None


def mmr_params(mmr: models.Mmr, limit) -> tuple[float, int]:
    """(diversity, candidates) of an MMR request with the defaults filled in, or ValueError:
    the limit must be an int, diversity must lie in [0, 1], and the candidates (given, or the
    default max(limit, 100)) may not exceed RAG_MMR_MAX_CANDIDATES."""
    if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)):
        raise ValueError("an MMR query needs an int limit")
    div = MMR_DIVERSITY if mmr.diversity is None else float(mmr.diversity)
    if not 0.0 <= div <= 1.0:                                   # NaN fails too
        raise ValueError(f"Mmr.diversity must lie in [0, 1], got {mmr.diversity!r}")
    cand = mmr.candidates_limit
    if cand is None:
        cand = max(int(limit), MMR_CANDIDATES)
    elif isinstance(cand, bool) or not isinstance(cand, (int, np.integer)) or cand < 1:
        raise ValueError("Mmr.candidates_limit must be an int >= 1")
    if cand > MMR_MAX_CANDIDATES:
        raise ValueError(f"MMR re-selects from at most {MMR_MAX_CANDIDATES} candidates "
                         f"(candidates_limit, or a limit above it): got {int(cand)}")
    return div, int(cand)


RRF_K = 2                    # FusionQuery(Fusion.RRF), Rrf(k=None)


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def is_fusion(query) -> bool:
    """Whether a query argument asks for fusion of prefetched lists."""
    return isinstance(query, (models.FusionQuery, models.RrfQuery))


def fusion_params(query, prefetch, limit, query_filter=None):
    """(rrf_k, [(vector, Filter or None, limit), ...]) of a fusion request — query a FusionQuery
    or RrfQuery, prefetch a Prefetch or a list of them — or ValueError naming what is wrong or
    not built: DBSF, nested prefetches, a prefetch without a plain nearest query, a nearest /
    MMR query over prefetched candidates, a top-level filter."""
    if not is_fusion(query):
        raise ValueError("prefetch is only built for fusion: query must be FusionQuery(Fusion.RRF) "
                         "or RrfQuery(Rrf(k)); re-scoring prefetched candidates with a nearest "
                         "query is not built")
    if isinstance(query, models.FusionQuery):
        fusion = getattr(query.fusion, "value", query.fusion)
        if fusion == models.Fusion.DBSF.value:
            raise ValueError("Fusion.DBSF (distribution-based score fusion) is not built; "
                             "use Fusion.RRF")
        if fusion != models.Fusion.RRF.value:
            raise ValueError(f"unknown fusion {query.fusion!r}: Fusion.RRF is the one built")
        rrf_k = RRF_K
    else:
        rrf_k = getattr(query.rrf, "k", None)
        if rrf_k is None:
            rrf_k = RRF_K
        elif not _is_int(rrf_k) or rrf_k < 1:
            raise ValueError(f"Rrf.k must be an int >= 1, got {rrf_k!r}")
    if query_filter is not None:
        raise ValueError("a fusion query takes no top-level query_filter: the filter belongs on "
                         "each Prefetch(filter=...)")
    if not _is_int(limit):
        raise ValueError("a fusion query needs an int limit")
    if isinstance(prefetch, models.Prefetch):
        prefetch = [prefetch]
    if prefetch is None or len(prefetch) == 0:
        raise ValueError("a fusion query needs prefetches to fuse: prefetch=[Prefetch(...), ...]")
    if len(prefetch) > FUSION_MAX_LISTS:
        raise ValueError(f"a fusion query fuses at most {FUSION_MAX_LISTS} prefetches, "
                         f"got {len(prefetch)}")
    out = []
    for n, p in enumerate(prefetch):
        if not isinstance(p, models.Prefetch):
            raise ValueError(f"prefetch[{n}] is not a Prefetch")
        if p.prefetch is not None:
            raise ValueError(f"prefetch[{n}]: a nested Prefetch.prefetch is not built")
        vec, mmr = nearest_of(p.query)
        if vec is None or is_fusion(vec):
            raise ValueError(f"prefetch[{n}] needs a query: a vector or a NearestQuery")
        if mmr is not None:
            raise ValueError(f"prefetch[{n}]: an MMR query (NearestQuery.mmr) inside a prefetch "
                             "is not built")
        if not _is_int(p.limit):
            raise ValueError(f"prefetch[{n}] needs an int limit")
        out.append((vec, p.filter, int(p.limit)))
    return int(rrf_k), out


def _stack_queries(qs: list, dim: int):
    """Query vectors (lists, arrays, tensors) as one [n, dim] batch: a tensor when any of them
    is one, else a float32 array."""
    if any(isinstance(x, torch.Tensor) for x in qs):
        dev = next(x.device for x in qs if isinstance(x, torch.Tensor))
        Q = torch.stack([(x if isinstance(x, torch.Tensor) else
                          torch.as_tensor(np.asarray(x, np.float32))).to(dev).reshape(-1)
                         for x in qs])
    else:
        Q = np.stack([np.asarray(x, np.float32).reshape(-1) for x in qs])
    if Q.shape[1] != dim:
        raise ValueError(f"every query must be one {dim}-dim vector")
    return Q


def _payloads(points: list, with_payload) -> list:
    """search_points' hits (each call's own objects) as the caller asked for them."""
    if not with_payload:
        for p in points:
            p.payload = None
    return points


class QdrantClient:
    """In-process, GPU-resident replacement for qdrant_client.QdrantClient."""

    def __init__(self, url: str | None = None, *args, device=None, path: str | None = None,
                 coalesce: bool = True, coalesce_window_s: float = 0.0, devices=None, **kwargs):
        self.url = url
        self.device = device
        # devices: None = every collection is one FlatIndex on `device`; a list of device
        # indices (or "all") = every collection is a ShardSet with one shard per entry, the
        # first being the merge device (a repeated index: logical shards on one GPU)
        self.devices = parse_devices(devices)
        self.path = path
        # concurrent query_points calls share GPU scans (Coalescer); coalesce=False searches
        # every call on its own
        self.coalesce = bool(coalesce)
        self.coalesce_window_s = float(coalesce_window_s)
        self._collections: dict[str, Collection] = {}
        self._lock = threading.Lock()
        if path is not None and os.path.isdir(path):
            from .store import load_collection
            for name in sorted(os.listdir(path)):
                d = os.path.join(path, name)
                if os.path.isfile(os.path.join(d, "collection.json")):
                    col = load_collection(d, device, devices=self.devices)
                    col.coalescer.window = self.coalesce_window_s
                    self._collections[col.name] = col

    def save(self, path: str | None = None) -> None:
        """Persist every collection under `path` (default: the client's path); collection
        directories of deleted collections are removed."""
        from .store import save_collection
        path = path or self.path
        if path is None:
            raise ValueError("no storage path: pass path= here or to QdrantClient(...)")
        os.makedirs(path, exist_ok=True)
        with self._lock:
            cols = dict(self._collections)
        for name, col in cols.items():
            save_collection(col, os.path.join(path, name))
        for name in os.listdir(path):
            d = os.path.join(path, name)
            if name not in cols and os.path.isfile(os.path.join(d, "collection.json")):
                shutil.rmtree(d)

    # ---------------------------------------------------------------- collections
    def get_collections(self) -> models.CollectionsResponse:
        with self._lock:
            return models.CollectionsResponse(
                collections=[models.CollectionDescription(name=n) for n in self._collections])

    def collection_exists(self, collection_name: str) -> bool:
        with self._lock:
            return collection_name in self._collections

    def create_collection(self, collection_name: str, vectors_config: models.VectorParams,
                          payload_tag_fields: Iterable[str] = DEFAULT_TAG_FIELDS,
                          capacity: int = 1024, **kwargs) -> bool:
        if vectors_config.distance != models.Distance.COSINE:
            raise NotImplementedError("only Distance.COSINE collections (database.py:126)")
        storage = _storage_of(vectors_config)
        with self._lock:
            if collection_name in self._collections:
                raise ValueError(f"collection {collection_name!r} already exists")
            col = Collection(collection_name, int(vectors_config.size), self.device,
                             tuple(payload_tag_fields), capacity, storage,
                             devices=self.devices)
            col.coalescer.window = self.coalesce_window_s
            self._collections[collection_name] = col
        return True

    def recreate_collection(self, collection_name: str, vectors_config, **kwargs) -> bool:
        self.delete_collection(collection_name)
        return self.create_collection(collection_name, vectors_config, **kwargs)

    def delete_collection(self, collection_name: str, **kwargs) -> bool:
        with self._lock:
            col = self._collections.pop(collection_name, None)
        if col is not None:
            col.index.close()
        return col is not None

    def _col(self, name: str) -> Collection:
        with self._lock:
            col = self._collections.get(name)
        if col is None:
            raise ValueError(f"Collection `{name}` doesn't exist!")
        return col

    # ---------------------------------------------------------------- points
    def upsert(self, collection_name: str, points, wait: bool = True, **kwargs):
        col = self._col(collection_name)
        if isinstance(points, models.Batch):
            ids, vecs, pls = points.ids, points.vectors, points.payloads
        else:
            points = list(points)
            ids = [p.id for p in points]
            vecs = [p.vector for p in points]
            pls = [p.payload for p in points]
        if not ids:
            return models.UpdateResult(operation_id=col.op, status=models.UpdateStatus.COMPLETED)
        op = col.upsert(ids, vecs, pls)
        return models.UpdateResult(operation_id=op, status=models.UpdateStatus.COMPLETED)

    def delete(self, collection_name: str, points_selector, wait: bool = True,
               **kwargs) -> models.UpdateResult:
        """Remove points: `points_selector` is a list of ids, a PointIdsList, a
        FilterSelector or a bare Filter (the `must` class query_points supports)."""
        op = self._col(collection_name).delete(points_selector)
        return models.UpdateResult(operation_id=op, status=models.UpdateStatus.COMPLETED)

    def count(self, collection_name: str, count_filter: models.Filter | None = None,
              exact: bool = True, **kwargs) -> models.CountResult:
        col = self._col(collection_name)
        if count_filter is None:
            return models.CountResult(count=len(col.row_ids))
        return models.CountResult(count=col.count_matching(count_filter))

    def retrieve(self, collection_name: str, ids, with_payload=True, with_vectors=False,
                 **kwargs):
        col = self._col(collection_name)
        out = []
        with col.lock:                    # rows move under a delete
            for pid in ids:
                r = col.id_to_row.get(_norm_id(pid))
                if r is not None:
                    p = col.point(r, 0.0, with_payload, with_vectors)
                    out.append(models.Record(id=p.id, payload=p.payload, vector=p.vector))
        return out

    def query_points(self, collection_name: str, query=None, limit: int = 10,
                     query_filter: models.Filter | None = None, with_payload=True,
                     with_vectors=False, prefetch=None, **kwargs) -> models.QueryResponse:
        col = self._col(collection_name)
        if prefetch is not None or is_fusion(query):
            # a fusion request never rides the coalescer: its prefetches are their own batch
            rrf_k, pres = fusion_params(query, prefetch, limit, query_filter)
            pts = col.search_points_fusion([(rrf_k, pres, int(limit))], with_vectors)[0]
            return models.QueryResponse(points=_payloads(pts, with_payload))
        query, mmr = nearest_of(query)
        flt = col.compile_filter(query_filter)
        if mmr is not None:
            # an MMR request never rides the coalescer: its candidate search is its own pass
            div, cand = mmr_params(mmr, limit)
            q = query if isinstance(query, torch.Tensor) else np.asarray(query, dtype=np.float32)
            pts = col.search_points_mmr(q.reshape(1, -1), [int(limit)], [flt], [div], [cand],
                                        with_vectors)[0]
        elif self.coalesce and 1 <= int(limit) <= MAX_K and not with_vectors:
            q = (query.detach().float().cpu().numpy() if isinstance(query, torch.Tensor)
                 else np.asarray(query, dtype=np.float32))
            if q.shape != (col.dim,):
                q = q.reshape(-1)
                if q.shape != (col.dim,):
                    raise ValueError(f"query must be one {col.dim}-dim vector")
            pts = col.coalescer.search(q, int(limit), flt)
        else:
            q = query if isinstance(query, torch.Tensor) else np.asarray(query, dtype=np.float32)
            q = q.reshape(1, -1)
            pts = col.search_points(q, int(limit), [flt], with_vectors)[0]
        return models.QueryResponse(points=_payloads(pts, with_payload))

    def query_batch_points(self, collection_name: str, requests: list,
                           **kwargs) -> list[models.QueryResponse]:
        """One GPU scan for the whole batch (per-query filters ride along in the kernel). With
        MMR requests in it (QueryRequest.query = NearestQuery(..., mmr=Mmr(...))): one search
        at the batch's largest candidate count and one MMR launch, the plain requests riding
        at diversity 0 with their own limit as candidate count — unless a plain limit exceeds
        RAG_MMR_MAX_CANDIDATES, in which case the plain requests are searched on their own.
        Fusion requests (QueryRequest.prefetch with a FusionQuery / RrfQuery) are answered
        together by one search_points_fusion call, the remaining requests as a batch of their
        own, and the results are scattered back in request order."""
        col = self._col(collection_name)
        if not requests:
            return []
        fus = [i for i, r in enumerate(requests)
               if getattr(r, "prefetch", None) is not None or is_fusion(r.query)]
        if fus:
            par = [fusion_params(requests[i].query, requests[i].prefetch, requests[i].limit,
                                 requests[i].filter) for i in fus]
            out: list = [None] * len(requests)
            hits = col.search_points_fusion(
                [(rrf_k, pres, int(requests[i].limit)) for i, (rrf_k, pres) in zip(fus, par)])
            for i, h in zip(fus, hits):
                out[i] = models.QueryResponse(points=_payloads(h, requests[i].with_payload))
            rest = [i for i in range(len(requests)) if out[i] is None]
            for i, resp in zip(rest, self.query_batch_points(
                    collection_name, [requests[i] for i in rest], **kwargs)):
                out[i] = resp
            return out
        unwrapped = [nearest_of(r.query) for r in requests]
        qs = [v for v, _ in unwrapped]
        Q = torch.stack([x if isinstance(x, torch.Tensor) else
                         torch.as_tensor(np.asarray(x, np.float32)) for x in qs]) \
            if any(isinstance(x, torch.Tensor) for x in qs) else np.asarray(qs, np.float32)
        filters = [col.compile_filter(r.filter) for r in requests]
        if all(m is None for _, m in unwrapped):
            hits = col.search_points(Q, max(int(r.limit) for r in requests), filters)
        else:
            par = [mmr_params(m, r.limit) if m is not None else (0.0, max(int(r.limit), 1))
                   for (_, m), r in zip(unwrapped, requests)]
            limits = [int(r.limit) for r in requests]
            if max(c for _, c in par) <= MMR_MAX_CANDIDATES:
                hits = col.search_points_mmr(Q, limits, filters, [d for d, _ in par],
                                             [c for _, c in par])
            else:
                plain = [i for i, (_, m) in enumerate(unwrapped) if m is None]
                rest = [i for i, (_, m) in enumerate(unwrapped) if m is not None]
                hits = [None] * len(requests)
                for i, h in zip(plain, col.search_points(
                        Q[plain], max(limits[i] for i in plain), [filters[i] for i in plain])):
                    hits[i] = h
                for i, h in zip(rest, col.search_points_mmr(
                        Q[rest], [limits[i] for i in rest], [filters[i] for i in rest],
                        [par[i][0] for i in rest], [par[i][1] for i in rest])):
                    hits[i] = h
        return [models.QueryResponse(points=_payloads(h[:int(r.limit)], r.with_payload))
                for r, h in zip(requests, hits)]

    def query_points_groups(self, collection_name: str, query=None, group_by: str | None = None,
                            limit: int = 10, group_size: int = 3,
                            query_filter: models.Filter | None = None, with_payload=True,
                            with_vectors=False, **kwargs) -> models.GroupsResult:
        """Qdrant's grouped search: the `limit` best groups of points sharing a value of
        payload field `group_by` (one of the collection's payload_tag_fields), each with its
        `group_size` best hits; points without the field belong to no group. Exact: `limit`
        groups unless the filtered collection holds fewer values, `group_size` hits unless the
        group holds fewer points. A grouped request never rides the coalescer."""
        col = self._col(collection_name)
        if group_by is None:
            raise ValueError("query_points_groups needs group_by, a payload field")
        if kwargs.get("with_lookup") is not None:
            raise NotImplementedError("with_lookup (a join on another collection) is not supported")
        if is_fusion(query) or kwargs.get("prefetch") is not None:
            raise ValueError("a grouped query over prefetched candidates (prefetch, FusionQuery, "
                             "RrfQuery) is not built")
        query, mmr = nearest_of(query)
        if mmr is not None:
            raise ValueError("a grouped query cannot be an MMR query (NearestQuery.mmr)")
        flt = col.compile_filter(query_filter)
        q = query if isinstance(query, torch.Tensor) else np.asarray(query, dtype=np.float32)
        found = col.search_groups(q.reshape(1, -1), group_by, int(limit), int(group_size), [flt],
                                  with_vectors)[0]
        for g in found:
            _payloads(g.hits, with_payload)
        return models.GroupsResult(groups=found)

    def search_groups(self, collection_name: str, query_vector, group_by: str,
                      query_filter=None, limit: int = 10, group_size: int = 1,
                      with_payload=True, with_vectors=False, **kwargs) -> models.GroupsResult:
        """Legacy qdrant_client.search_groups: query_points_groups."""
        return self.query_points_groups(collection_name, query_vector, group_by, limit,
                                        group_size, query_filter, with_payload, with_vectors,
                                        **kwargs)

    def search(self, collection_name: str, query_vector, limit: int = 10,
               query_filter=None, with_payload=True, **kwargs):
        """Legacy qdrant_client.search: list[ScoredPoint]."""
        return self.query_points(collection_name, query_vector, limit, query_filter,
                                 with_payload).points

    def close(self) -> None:
        if self.path is not None and self._collections:
            self.save()
        with self._lock:
            cols = list(self._collections.values())
            self._collections.clear()
        for c in cols:
            c.index.close()
