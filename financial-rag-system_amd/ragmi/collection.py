"""Collection — one COSINE collection: an index in HBM (FlatIndex, or a ShardSet over several
devices) plus the host-side id / payload / version maps, and every search route over them.

A row number means a point only while the collection's lock is held (a delete moves rows):
every route resolves its hits to ScoredPoints under the same hold of the lock as the search
that produced them (`_points`). All index work goes on the caller's current stream.
"""
from __future__ import annotations

import threading
import uuid
from typing import Any

import numpy as np
import torch

from . import groups
from . import qdrant_models as models
from .coalesce import Coalescer
from .filters import (DEFAULT_TAG_FIELDS, KEY_ABSENT, MAX_PROGRAMS, FilterProgram,
                      PayloadRanges, PayloadTags, UnsupportedFilter, compile_filter,
                      compile_legacy_only, pack_view)
from .formula import BAD, MISSING, NONFINITE, compile_formula
from .index import (FUSION_MAX_ENTRIES, GROUPS_MAX, GROUPS_MAX_CELLS, ORDER_MAX,
                    SPARSE_MAX_QUERY_NNZ, SPARSE_MAX_SLOTS, SPARSE_SLOTS, FlatIndex,
                    formula_rescore, fuse_rrf, hits_of, host_or_tensor)
from .shardset import ShardSet, parse_devices
from .sparse import idf_weights, pack_rows, unpack_row


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


class SparsePrefetch:
    """The query of a sparse prefetch of a fusion request: a SparseVector and the `using` it
    came with (checked against the collection under its lock)."""

    def __init__(self, vector, using):
        self.vector, self.using = vector, using


def _is_vector(example) -> bool:
    """A recommend example is a point id (what _norm_id takes: an int, a UUID, a str) or,
    being anything else, a vector."""
    return not isinstance(example, (bool, int, np.integer, uuid.UUID, str))


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


def require_finite(vecs, what: str, names=None) -> None:
    """ValueError for the first vector of the batch `vecs` [n, dim] (array or tensor) that holds
    a non-finite component, naming it: `what` and names[i] (the point id) or its position i.
    Real Qdrant cannot receive such a vector at all (JSON has no spelling for inf or NaN); the
    index below does not check (its inputs may be device tensors) and stores or searches it as
    the zero vector (DESIGN.md "Values at the edges"). A tensor on a device is read back for
    this, so the check synchronises."""
    if isinstance(vecs, torch.Tensor):
        bad = (~torch.isfinite(vecs).all(dim=1)).cpu().numpy()
    else:
        bad = ~np.isfinite(np.asarray(vecs)).all(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        which = f"{names[i]!r}" if names is not None else f"at position {i}"
        raise ValueError(f"{what} {which} holds a non-finite component (inf or NaN)")


def stack_queries(qs: list, dim: int, one: bool = False, host: bool = False,
                  what: str = "query"):
    """The query stacker: query vectors given as lists, arrays or tensors, as one [n, dim]
    batch: a tensor when any of them is one, else a float32 array. one=True: `qs` is the one
    vector of a single request. host=True (the coalescer route, whose leader stacks its riders'
    queries on the host): tensors are brought to host numpy first. A vector with a non-finite
    component is refused (require_finite), named by `what` and its position in `qs`."""
    if host:
        qs = [x.detach().float().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in qs]
    if len(qs) == 1:
        Q = host_or_tensor(qs[0]).reshape(1, -1)
    elif any(isinstance(x, torch.Tensor) for x in qs):
        dev = next(x.device for x in qs if isinstance(x, torch.Tensor))
        Q = torch.stack([(x if isinstance(x, torch.Tensor) else
                          torch.as_tensor(np.asarray(x, np.float32))).to(dev).reshape(-1)
                         for x in qs])
    else:
        Q = np.stack([np.asarray(x, np.float32).reshape(-1) for x in qs])
    if Q.shape[1] != dim:
        raise ValueError(f"{'query' if one else 'every query'} must be one {dim}-dim vector")
    require_finite(Q, what)
    return Q


class SparseBatch:
    """The padded sparse queries of a batch (ragmi.sparse.pack_rows at 64 slots) as one object
    the list builders index like a query array: batch[members] is the sub-batch."""

    def __init__(self, terms, vals, nnz):
        self.terms, self.vals, self.nnz = terms, vals, nnz

    def __len__(self):
        return len(self.nnz)

    def __getitem__(self, members):
        m = np.asarray(members, dtype=np.int64)
        return SparseBatch(self.terms[m], self.vals[m], self.nnz[m])


class Collection:
    """One COSINE collection: FlatIndex in HBM + host-side id/payload maps. With `devices`
    (one device index per shard, ragmi.shardset.parse_devices) the rows are striped over a
    ShardSet instead; rows, ids, payloads and tags stay global and host-side either way.
    `index`: an object to use as the index (the protocol of DESIGN.md "Where the front end
    lives"); no FlatIndex / ShardSet is created then.
    `range_fields`: the numeric payload fields `range` conditions may name, a mapping of field
    to kind ("number" or "datetime") or a sequence of names all meaning "number" (at most 4;
    ragmi.filters.PayloadRanges). Each is a key column of the index, written with every upsert.
    A collection without any never calls the index's key methods.
    `sparse`: None, or (name, idf, slots) — the collection's one named sparse vector (DESIGN
    R19): a sparse column of `slots` slots per row in the index, written with every upsert (an
    empty row for a point without a sparse vector); idf: Modifier.IDF. A collection without one
    never calls the index's sparse methods."""

    BACKFILL_ROWS = 1 << 16      # rows per write_keys call of add_range_field

    def __init__(self, name: str, dim: int, device, tag_fields=DEFAULT_TAG_FIELDS,
                 capacity: int = 1024, storage: str = "fp32", devices=None, *, index=None,
                 range_fields=None, sparse=None):
        self.name = name
        self.dim = dim
        self.tags = PayloadTags(tag_fields)
        self.ranges = PayloadRanges(range_fields)
        clash = set(self.ranges.fields) & set(self.tags.fields)
        if clash:
            raise ValueError(f"{sorted(clash)}: a field is a keyword tag field or a range field, "
                             "not both")
        devices = parse_devices(devices)
        self.index = (index if index is not None else
                      ShardSet(dim=dim, devices=devices, capacity=capacity, storage=storage)
                      if devices is not None else
                      FlatIndex(dim=dim, capacity=capacity, device=device, storage=storage))
        self.id_to_row: dict[Any, int] = {}
        self.row_ids: list[Any] = []
        self.payloads: list[dict | None] = []
        self.versions: list[int] = []
        self.op = 0
        self.group_stats = {}    # routes grouped searches took (ragmi.groups.search_groups)
        self.lock = threading.RLock()
        # 32 queries per scan pass at D = 384, 4 groups of 32 at D = 1024 (ragmi.h)
        self.coalescer = Coalescer(self, 0.0, 32 if dim <= 384 else 128,
                                   search=self.search_points)
        if len(self.ranges):
            self.index.keys_create(len(self.ranges))
        self.sparse_name, self.sparse_idf, self.sparse_slots = None, False, 0
        self.sparse_len: list[int] = []      # per row, the nonzeros of its sparse row
        self._df = None                      # (df int64 [65535] host, N) of Modifier.IDF, cached
        if sparse is not None:
            name, idf, slots = sparse
            slots = SPARSE_SLOTS if slots is None else int(slots)
            if not isinstance(name, str) or name == "":
                self.index.close()
                raise ValueError('a sparse vector needs a name other than "" (the dense vector)')
            if not 16 <= slots <= SPARSE_MAX_SLOTS or slots % 16:
                self.index.close()
                raise ValueError(f"sparse_slots must be a multiple of 16 in [16, "
                                 f"{SPARSE_MAX_SLOTS}], got {slots}")
            try:
                self.index.sparse_create(slots)
            except BaseException:
                self.index.close()
                raise
            self.sparse_name, self.sparse_idf, self.sparse_slots = name, bool(idf), slots

    @property
    def rescued(self) -> int:
        """Queries re-answered on the full exact pass (the index's counter; stats). Setting it
        sets the index's counter."""
        return self.index.rescued

    @rescued.setter
    def rescued(self, n: int) -> None:
        self.index.rescued = n

    def compile_filter(self, flt):
        """ragmi.filters.compile_filter over this collection's tags and range fields."""
        return compile_filter(self.tags, flt, self.ranges)

    def add_range_field(self, name: str, kind: str) -> bool:
        """Declare range field `name` ("number" or "datetime") on a collection that may hold
        points — the engine of create_payload_index. Under the lock: the index grows a key
        column, the column is back-filled from the host payloads of all current rows in chunks
        of BACKFILL_ROWS, and the stream is synchronised. False when the field was declared
        already (with the same kind); ValueError for another kind, a tag field, or a fifth
        field."""
        with self.lock:
            if name in self.tags.fields:
                raise ValueError(f"{name!r} is a keyword tag field, it cannot be a range field")
            if name in self.ranges.fields:
                self.ranges.add(name, kind)          # same kind, or ValueError
                return False
            col = self.ranges.add(name, kind)
            self.index.keys_create(col + 1)
            n = len(self.row_ids)
            for r0 in range(0, n, self.BACKFILL_ROWS):
                rows = np.arange(r0, min(n, r0 + self.BACKFILL_ROWS), dtype=np.int64)
                keys = [self.ranges.keys(p)[col] for p in self.payloads[r0:r0 + len(rows)]]
                self.index.write_keys(col, rows, np.asarray(keys, dtype=np.int64))
            if n:
                torch.cuda.current_stream(self.index.device).synchronize()
            return True

    # ---------------------------------------------------------------- writes
    def upsert(self, ids: list, vectors, payloads: list, sparse: list | None = None) -> int:
        """`sparse`: per point its SparseVector or None, in a collection with a sparse vector
        (a point without one gets an empty sparse row: an upsert replaces the whole point)."""
        with self.lock:
            self.op += 1
            vec = host_or_tensor(vectors)
            if vec.ndim != 2 or vec.shape[1] != self.dim:
                raise ValueError(f"vectors must be [n, {self.dim}]")
            require_finite(vec, "upsert: the vector of point",
                           list(ids) if len(ids) == vec.shape[0] else None)
            sp = None
            if self.sparse_name is not None:
                # refused before anything is written: the error names the point
                sp = pack_rows(list(sparse) if sparse is not None else [None] * len(ids),
                               self.sparse_slots, list(ids), "upsert: the sparse vector of point")
            elif sparse is not None and any(v is not None for v in sparse):
                raise ValueError(f"collection {self.name!r} has no sparse vector")
            # last write wins for duplicate ids inside one batch (Qdrant semantics)
            last: dict[Any, int] = {}
            for i, pid in enumerate(ids):
                last[_norm_id(pid)] = i
            rows, sel, tags, keys = [], [], [], []
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
                    if sp is not None:
                        self.sparse_len.append(0)
                p = payloads[i] if payloads is not None else None
                self.payloads[r] = dict(p) if p is not None else None
                self.versions[r] = self.op
                rows.append(r)
                sel.append(i)
                tags.append(self.tags.tag(p))
                if len(self.ranges):
                    keys.append(self.ranges.keys(p))
            if new_count > self.index.capacity:
                self.index.reserve(max(new_count, 2 * self.index.capacity))
            if rows:
                sel_t = vec[sel] if isinstance(vec, torch.Tensor) else vec[np.asarray(sel)]
                self.index.upsert(sel_t, np.asarray(rows, dtype=np.int64),
                                  np.asarray(tags, dtype=np.uint32), new_count=new_count)
                # every column of every written row, under this hold of the lock: an overwrite
                # whose payload lacks the field writes KEY_ABSENT
                for c, col_keys in enumerate(np.asarray(keys, dtype=np.int64).T if keys else ()):
                    self.index.write_keys(c, np.asarray(rows, dtype=np.int64),
                                          np.ascontiguousarray(col_keys))
                if sp is not None:
                    # the sparse row of every written row, under this hold of the lock
                    pick = np.asarray(sel)
                    self.index.sparse_write(np.asarray(rows, dtype=np.int64), sp[0][pick],
                                            sp[1][pick])
                    for r, m in zip(rows, sp[2][pick].tolist()):
                        self.sparse_len[r] = m
                    self._df = None
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
            flt = (compile_legacy_only(self.tags, what, "Collection.delete", self.ranges)
                   if kind == "filter" else None)
            self.op += 1
            if kind == "ids":
                found = {self.id_to_row[pid] for pid in what if pid in self.id_to_row}
                rows = np.fromiter(found, dtype=np.int64, count=len(found))
            else:
                rows = self._matching(flt)[0]
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
            if self.sparse_name is not None:      # the device moved the sparse row with the rest
                self.sparse_len[d] = self.sparse_len[s]
        del self.row_ids[n1:], self.payloads[n1:], self.versions[n1:]
        if self.sparse_name is not None:
            del self.sparse_len[n1:]
            self._df = None

    # ---------------------------------------------------------------- reads
    def _matching(self, c, cap: int | None = None):
        """The rows a compiled filter selects, resolved on the device: (rows, total) — the
        first `cap` rows (default: all) as a host int64 array, None for cap = 0 (a pure count),
        and the count of every match. The one triage of a filter for row selection: nothing
        matches, every row matches, select_rows of a (mask, value) pair, select_rows_view of a
        FilterProgram. Called under the lock."""
        n = len(self.row_ids)
        if c is None or not n:
            return np.empty(0, np.int64), 0
        if c == (0, 0):
            return np.arange(n if cap is None else min(cap, n), dtype=np.int64), n
        if isinstance(c, FilterProgram):
            rows, total = self.index.select_rows_view(pack_view([c]), cap=cap)
        else:
            rows, total = self.index.select_rows(c[0], c[1], cap=cap)
        return (rows.cpu().numpy() if cap != 0 else None), total

    def count_matching(self, flt) -> int:
        """Points a Filter matches, counted on the device (select_rows with cap = 0)."""
        with self.lock:
            return self._matching(self.compile_filter(flt), cap=0)[1]

    def _points(self, hits: list, with_vectors=False) -> list:
        """Per request its hits [(row, score)] resolved to ScoredPoints (payload attached). A
        delete moves rows, so a row number means a point only while the lock is held: called
        under the same hold of the lock as the search that produced the hits."""
        return [[self.point(r, s, True, with_vectors) for r, s in h] for h in hits]

    def search_points(self, queries, limit: int, filters: list, with_vectors=False):
        """search with every hit resolved to its ScoredPoint under the same hold of the lock
        (_points). What query_points, query_batch_points and the coalescer's leaders call."""
        with self.lock:
            return self._points(self.search(queries, limit, filters), with_vectors)

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
            for i, h in zip(live, hits_of(*self._lists(queries, filters, live, k))):
                out[i] = h
            return out

    @staticmethod
    def _live(queries, filters: list, live: list):
        """The one slice of the live requests: their queries ([n, dim], a tensor staying a
        tensor) and their compiled filters."""
        q = host_or_tensor(queries)
        return (q[live] if len(live) != len(filters) else q), [filters[i] for i in live]

    @staticmethod
    def _pairs(fl: list):
        """(mask, value) filters as the index takes them: [n, 2] uint32, or None when no
        request filters."""
        use = np.asarray(fl, dtype=np.uint32).reshape(-1, 2)
        return use if use.any() else None

    def _lists(self, queries, filters: list, live: list, k: int):
        """The exact top-k lists of the `live` requests. Every live filter a (mask, value)
        pair: the path of every release so far, unchanged. Otherwise the view path
        (_view_lists)."""
        q, fl = self._live(queries, filters, live)
        if not any(isinstance(f, FilterProgram) for f in fl):
            return self._exact_lists(q, k, self._pairs(fl))
        return self._view_lists(q, fl, k)

    def _view_lists(self, q, fl: list, k: int, lists=None):
        """_lists with general filters among the live ones: the batch's distinct programs
        share view bits (a (mask, value) pair rides as its one-atom MASKEQ program; (0, 0)
        needs no bit, over any view it passes every row), every query gets the filter
        (1 << slot, 1 << slot), and one view search answers the batch. More than MAX_PROGRAMS
        distinct programs: the queries are dealt into calls of at most that many, each query
        into the first call that knows its program or has a free bit, and the results are
        scattered back. `lists`: the list builder (q, k, use, programs=) -> (scores, rows),
        _exact_lists unless the queries are sparse (_sparse_exact)."""
        lists = lists or self._exact_lists
        calls: list = []                       # (slots: {program: bit}, members, their filters)
        for j, f in enumerate(fl):
            prog = (f if isinstance(f, FilterProgram) else
                    None if tuple(f) == (0, 0) else FilterProgram.maskeq(*f))
            for slots, members, bits in calls:
                if prog is None or prog in slots or len(slots) < MAX_PROGRAMS:
                    break
            else:
                slots, members, bits = {}, [], []
                calls.append((slots, members, bits))
            bit = 0 if prog is None else 1 << slots.setdefault(prog, len(slots))
            members.append(j)
            bits.append((bit, bit))
        s = ids = None
        for slots, members, bits in calls:
            # every call holds a program: a call is opened for a query that brings one, except
            # the first, and a batch without any program never comes here
            blob = pack_view(list(slots))
            use = np.asarray(bits, dtype=np.uint32).reshape(-1, 2)
            if len(calls) == 1:
                return lists(q, k, use, programs=blob)
            s1, i1 = lists(q[members], k, use, programs=blob)
            if s is None:
                s = torch.empty((len(fl), k), dtype=s1.dtype, device=s1.device)
                ids = torch.empty((len(fl), k), dtype=i1.dtype, device=i1.device)
            sel = torch.as_tensor(members, device=s1.device)
            s[sel] = s1
            ids[sel] = i1
        return s, ids

    def _exact_lists(self, q, k: int, use, programs=None):
        """The exact top-k lists (scores, rows) of queries `q`, as the index's tensors, with
        every query a large-k pass left unanswered re-answered on the full exact pass (the
        index's search, rescue). What search reports and what the MMR path re-selects from.
        Called under the lock. `programs`: a filter-program blob; `use` then indexes the bits
        of its view."""
        view = {} if programs is None else {"programs": programs}
        return self.index.search(q, k, filters=use, rescue=True, **view)

    # ---------------------------------------------------------------- sparse queries
    def _need_sparse(self, using, what: str) -> None:
        """ValueError unless `using` names this collection's sparse vector."""
        if self.sparse_name is None:
            raise ValueError(f"{what}: collection {self.name!r} has no sparse vector (create it "
                             "with sparse_vectors_config={name: SparseVectorParams()})")
        if using is None:
            raise ValueError(f"{what}: a SparseVector query needs using={self.sparse_name!r}, the "
                             "name of the collection's sparse vector")
        if using != self.sparse_name:
            raise ValueError(f"{what}: using={using!r} is not a vector of collection "
                             f"{self.name!r}; its sparse vector is {self.sparse_name!r}")

    def sparse_stats(self):
        """(df, N) of Modifier.IDF: the document frequency of every term (host int64 [65535],
        rag_index_sparse_df) and the points with a non-empty sparse row. Cached; every upsert and
        delete invalidates it. Called under the lock; the first call after a write synchronises."""
        if self._df is None:
            self._df = (self.index.sparse_df().cpu().numpy(),
                        sum(1 for m in self.sparse_len if m > 0))
        return self._df

    def sparse_batch(self, vectors: list, what: str) -> SparseBatch:
        """Sparse query vectors as the padded batch the index takes, refused as
        ragmi.sparse.entries refuses them and above SPARSE_MAX_QUERY_NNZ nonzeros; under
        Modifier.IDF every weight is multiplied by its term's IDF (ragmi.sparse.idf_weights).
        Called under the lock."""
        for i, v in enumerate(vectors):
            n = len(getattr(v, "indices", None) or ())
            if n > SPARSE_MAX_QUERY_NNZ:
                # (explicit zeros count here: the refusal must not depend on the values)
                raise ValueError(f"{what} at position {i}: {n} entries, a sparse query holds at "
                                 f"most {SPARSE_MAX_QUERY_NNZ} (RAG_SPARSE_MAX_QUERY_NNZ)")
        terms, vals, nnz = pack_rows(vectors, SPARSE_MAX_QUERY_NNZ, None, what)
        if self.sparse_idf and len(nnz) and self.index.count:
            df, n_docs = self.sparse_stats()
            for i, m in enumerate(nnz.tolist()):
                vals[i, :m] = idf_weights(terms[i, :m], vals[i, :m], df, n_docs)
        return SparseBatch(terms, vals, nnz)

    def _sparse_exact(self, q: SparseBatch, k: int, use, programs=None):
        """_exact_lists for sparse queries: the index's sparse search with rescue."""
        view = {} if programs is None else {"programs": programs}
        return self.index.sparse_search(q.terms, q.vals, q.nnz, k, filters=use, rescue=True,
                                        **view)

    def _sparse_lists(self, q: SparseBatch, fl: list, k: int):
        """The exact sparse top-k lists of a batch whose compiled filters `fl` are all live:
        (mask, value) pairs ride as they are, general filters through the view path."""
        if not any(isinstance(f, FilterProgram) for f in fl):
            return self._sparse_exact(q, k, self._pairs(fl))
        return self._view_lists(q, fl, k, lists=self._sparse_exact)

    def search_sparse(self, requests: list):
        """Sparse queries. `requests`: per request (SparseVector, using, compiled
        filter, limit). The requests of the batch ride one sparse search at k = the largest
        limit (clamped to the collection's count), 32 per pass. The score is the sparse score; a
        point that shares no term with the query is no hit, so a list may be shorter than its
        limit. Returns per request [(row, score)], best first."""
        with self.lock:
            for _, using, _, _ in requests:
                self._need_sparse(using, "sparse query")
            batch = self.sparse_batch([v for v, _, _, _ in requests], "sparse query")
            out = [[] for _ in requests]
            count = self.index.count
            live = [i for i, (_, _, c, lim) in enumerate(requests) if c is not None and lim >= 1]
            if not live or count == 0:
                return out
            lims = [int(requests[i][3]) for i in live]
            k = min(max(lims), count)
            s, ids = self._sparse_lists(batch[live] if len(live) != len(requests) else batch,
                                        [requests[i][2] for i in live], k)
            for i, n, h in zip(live, lims, hits_of(s, ids)):
                out[i] = h[:n]
            return out

    def search_points_sparse(self, requests: list, with_vectors=False):
        """search_sparse with every hit resolved to its ScoredPoint under the same hold of the
        lock (_points)."""
        with self.lock:
            return self._points(self.search_sparse(requests), with_vectors)

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
            for i, n, h in zip(live, lim, hits_of(s, ids)):
                out[i] = h[:n]
            return out

    def search_points_mmr(self, queries, limits, filters: list, diversity, candidates,
                          with_vectors=False):
        """search_mmr with every hit resolved to its ScoredPoint under the same hold of the
        lock (_points)."""
        with self.lock:
            return self._points(self.search_mmr(queries, limits, filters, diversity, candidates),
                                with_vectors)

    def search_recommend(self, requests: list):
        """Recommend queries. `requests`: per request (positive, negative,
        strategy, compiled filter, limit) — the examples point ids and / or vectors, as
        recommend_params returns them. Under the lock: every id resolves to its row (an unknown
        id is a ValueError naming it) and the example rows are gathered on the device in their
        stored form (fp32 storage: the fp32 row; fp16: the halves widened), from where an id
        example is a caller's vector. Each request is one index.recommend call for limit + m
        hits, m its distinct id examples, with rescue: the example rows are dropped and the
        list is cut to limit, so example points never appear and `limit` hits still arrive.
        limit < 1, an empty collection and a filter nothing can match give [] without a launch.
        Returns per request [(row, score)], best first."""
        if not hasattr(self.index, "recommend"):               # a ShardSet has none
            raise NotImplementedError("recommend over a shard set is not built")
        with self.lock:
            out = []
            for pos, neg, strategy, c, limit in requests:
                # position in its side -> row, for the examples given by id
                by_id = [{j: self._example_row(x) for j, x in enumerate(side)
                          if not _is_vector(x)} for side in (pos, neg)]
                own = set(by_id[0].values()) | set(by_id[1].values())
                # the caller's vectors, before anything else: a refusal does not depend on limits
                for side, what in ((pos, "recommend: positive example"),
                                   (neg, "recommend: negative example")):
                    for j, x in enumerate(side):
                        if _is_vector(x):
                            require_finite(host_or_tensor(x).reshape(1, -1), what, [j])
                count = self.index.count
                if limit < 1 or count == 0 or c is None:
                    out.append([])
                    continue
                sides = []
                for side, rows in zip((pos, neg), by_id):
                    vecs = list(side)
                    if rows:
                        got = self.index.gather_rows(np.asarray(list(rows.values()), np.int64))
                        stored = got[1] if got[1] is not None else \
                            got[0].view(torch.float16).float()
                        for j, v in zip(rows, stored):
                            vecs[j] = v
                    sides.append(stack_queries(vecs, self.dim, what="recommend: example")
                                 if vecs else None)
                view = {}
                if isinstance(c, FilterProgram):
                    view = {"programs": pack_view([c]), "filters": (1, 1)}
                elif tuple(c) != (0, 0):
                    view = {"filters": tuple(c)}
                k = min(int(limit) + len(own), count)
                hits = hits_of(*(t.unsqueeze(0) for t in self.index.recommend(
                    sides[0], sides[1], strategy, k, rescue=True, **view)))[0]
                out.append([h for h in hits if h[0] not in own][:int(limit)])
            return out

    def _example_row(self, pid, what: str = "recommend") -> int:
        """The row of example point `pid`, or ValueError naming the id. Under the lock."""
        r = self.id_to_row.get(_norm_id(pid))
        if r is None:
            raise ValueError(f"{what}: example point {pid!r} is not in collection "
                             f"{self.name!r}")
        return r

    def search_points_recommend(self, requests: list, with_vectors=False):
        """search_recommend with every hit resolved to its ScoredPoint under the same hold of
        the lock (_points)."""
        with self.lock:
            return self._points(self.search_recommend(requests), with_vectors)

    def _check_prefetch_vectors(self, requests: list, route: str) -> None:
        """Every prefetch vector of a fusion or formula request list, searched or not, so that
        a refusal does not depend on the limits (require_finite; a sparse prefetch:
        _need_sparse and sparse_batch's refusals): the error names the request and the
        prefetch."""
        for b, (_, pres, _) in enumerate(requests):
            for l, (vec, _, _) in enumerate(pres):
                what = f"{route}: request {b}, the query of prefetch"
                if isinstance(vec, SparsePrefetch):
                    self._need_sparse(vec.using, f"{what} {l}")
                    self.sparse_batch([vec.vector], f"{what} {l}")
                else:
                    require_finite(host_or_tensor(vec).reshape(1, -1), what, [l])

    def search_discover(self, requests: list):
        """Discovery and context queries. `requests`: per request (target or None,
        [(positive, negative), ...], compiled filter, limit) — every example a point id or a
        vector, as discover_params returns them; no target: a context search. Under the lock:
        every id resolves to its row (an unknown id is a ValueError naming it) and the example
        rows are gathered on the device in their stored form, as search_recommend does. Each
        request is one index.discover call for limit + m hits, m its distinct id examples, with
        rescue — a saturated request (a context search with few pairs) is re-answered on the
        full pass, never returned empty —: the example rows are dropped and the list is cut to
        limit. limit < 1, an empty collection and a filter nothing can match give [] without a
        launch. Returns per request [(row, score)], best first."""
        if not hasattr(self.index, "discover"):                # a ShardSet has none
            raise NotImplementedError("discover over a shard set is not built")
        with self.lock:
            out = []
            for target, pairs, c, limit in requests:
                flat = ([] if target is None else [target]) + [x for pair in pairs for x in pair]
                by_id = {j: self._example_row(x, "discover") for j, x in enumerate(flat)
                         if not _is_vector(x)}
                own = set(by_id.values())
                count = self.index.count
                if limit < 1 or count == 0 or c is None:
                    out.append([])
                    continue
                vecs = list(flat)
                if by_id:
                    got = self.index.gather_rows(np.asarray(list(by_id.values()), np.int64))
                    stored = got[1] if got[1] is not None else got[0].view(torch.float16).float()
                    for j, v in zip(by_id, stored):
                        vecs[j] = v
                t = None
                if target is not None:
                    t, vecs = stack_queries(vecs[:1], self.dim)[0], vecs[1:]
                pos = stack_queries(vecs[0::2], self.dim) if vecs else None
                neg = stack_queries(vecs[1::2], self.dim) if vecs else None
                view = {}
                if isinstance(c, FilterProgram):
                    view = {"programs": pack_view([c]), "filters": (1, 1)}
                elif tuple(c) != (0, 0):
                    view = {"filters": tuple(c)}
                k = min(int(limit) + len(own), count)
                hits = hits_of(*(x.unsqueeze(0) for x in self.index.discover(
                    t, pos, neg, k, rescue=True, **view)))[0]
                out.append([h for h in hits if h[0] not in own][:int(limit)])
            return out

    def search_points_discover(self, requests: list, with_vectors=False):
        """search_discover with every hit resolved to its ScoredPoint under the same hold of the
        lock (_points)."""
        with self.lock:
            return self._points(self.search_discover(requests), with_vectors)

    def search_fusion(self, requests: list):
        """Fusion queries. `requests`: per request (rrf_k, [(vector, Filter or
        None, limit), ...], limit), as fusion_params returns them. Every prefetch of every
        request rides one batched search at C = the largest prefetch limit (clamped to the
        collection's count); the lists are arranged [B, Lmax, C] on the device, each cut to
        its own limit by ncand, and fused by rag_fuse_rrf in one launch per distinct rrf_k. A
        prefetch whose filter can match nothing, or whose limit is < 1, is an empty list and
        is not searched. A prefetch whose vector is a SparsePrefetch (hybrid search, DESIGN
        §R19) rides one batched sparse search beside the dense one, into the same row tensor;
        its list is cut by ncand to its real hits (rows sharing a term), which may be fewer
        than its limit. Returns per request [(row, fused score)], best first."""
        with self.lock:
            out = [[] for _ in requests]
            count = self.index.count
            # every filter is compiled, so that a refusal does not depend on the limits
            compiled = [[self.compile_filter(f) for _, f, _ in pres] for _, pres, _ in requests]
            self._check_prefetch_vectors(requests, "fusion")
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
            dense = [j for j, v in enumerate(qs) if not isinstance(v, SparsePrefetch)]
            sparse = [j for j, v in enumerate(qs) if isinstance(v, SparsePrefetch)]
            dev = self.index.device
            rows = torch.full((len(live), Lmax, C), -1, dtype=torch.int64, device=dev)
            at = np.asarray([(slot[b], l) for b, l, _ in where], dtype=np.int64)
            ncand = np.zeros((len(live), Lmax), dtype=np.int32)
            ncand[at[:, 0], at[:, 1]] = [n for _, _, n in where]
            if dense:
                _, ids = self._lists(stack_queries([qs[j] for j in dense], self.dim),
                                     [filters[j] for j in dense], list(range(len(dense))), C)
                rows[torch.from_numpy(at[dense, 0]).to(dev),
                     torch.from_numpy(at[dense, 1]).to(dev)] = ids
            if sparse:
                batch = self.sparse_batch([qs[j].vector for j in sparse], "fusion: sparse prefetch")
                _, ids = self._sparse_lists(batch, [filters[j] for j in sparse], C)
                rows[torch.from_numpy(at[sparse, 0]).to(dev),
                     torch.from_numpy(at[sparse, 1]).to(dev)] = ids
                real = (ids >= 0).sum(dim=1).cpu().numpy().astype(np.int32)
                ncand[at[sparse, 0], at[sparse, 1]] = np.minimum(
                    ncand[at[sparse, 0], at[sparse, 1]], real)
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
                for j, h in zip(members, hits_of(s, r)):
                    out[live[j]] = h[:lim[j]]
            return out

    def search_points_fusion(self, requests: list, with_vectors=False):
        """search_fusion with every hit resolved to its ScoredPoint (score = the fused score)
        under the same hold of the lock (_points)."""
        with self.lock:
            return self._points(self.search_fusion(requests), with_vectors)

    def search_formula(self, requests: list):
        """Formula queries. `requests`: per request (FormulaQuery, [(vector,
        Filter or None, limit), ...], limit), as formula_params returns them. Every formula is
        compiled over this collection's tag and range fields (ragmi.formula) with L = the
        request's number of prefetches. Every prefetch of every request rides one batched
        search at C = the largest prefetch limit (clamped to the collection's count), scores
        kept; the lists are arranged [B, Lmax, C] on the device, each cut to its own limit by
        ncand; the tags are gathered once when a formula has a condition, each key column once
        when a formula names it; rag_formula_rescore runs in one launch per distinct compiled
        formula. A prefetch whose filter can match nothing, or whose limit is < 1, is an empty
        list and is not searched. A request whose status comes back non-zero (a variable
        without value or default, a value that is not finite) raises ValueError for the call.
        Returns per request [(row, value)], best first."""
        with self.lock:
            out = [[] for _ in requests]
            count = self.index.count
            # compiled first, so that a refusal does not depend on the limits
            formulas = [compile_formula(q, None, len(pres), self.tags, self.ranges)
                        for q, pres, _ in requests]
            compiled = [[self.compile_filter(f) for _, f, _ in pres] for _, pres, _ in requests]
            self._check_prefetch_vectors(requests, "formula")
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
                raise ValueError(f"formula: {Lmax} prefetches of up to {C} hits are {Lmax * C} "
                                 f"entries; at most {FUSION_MAX_ENTRIES} (prefetches x the "
                                 "largest prefetch limit) are re-scored")
            sc, ids = self._lists(stack_queries(qs, self.dim), filters, list(range(len(qs))), C)
            dev = ids.device
            rows = torch.full((len(live), Lmax, C), -1, dtype=torch.int64, device=dev)
            scores = torch.full((len(live), Lmax, C), float("-inf"), dtype=torch.float32,
                                device=dev)
            at = np.asarray([(slot[b], l) for b, l, _ in where], dtype=np.int64)
            a0, a1 = torch.from_numpy(at[:, 0]).to(dev), torch.from_numpy(at[:, 1]).to(dev)
            rows[a0, a1] = ids
            scores[a0, a1] = sc
            ncand = np.zeros((len(live), Lmax), dtype=np.int32)
            ncand[at[:, 0], at[:, 1]] = [n for _, _, n in where]
            lim = [int(requests[b][2]) for b in live]
            k = min(max(lim), Lmax * C)
            by_blob: dict = {}
            for j, b in enumerate(live):
                by_blob.setdefault(formulas[b].blob().tobytes(), (formulas[b], []))[1].append(j)
            tags = (self.index.gather_tags(rows)
                    if any(f.has_cond for f, _ in by_blob.values()) else None)
            keys = {c: self.index.gather_keys(c, rows)
                    for c in sorted({c for f, _ in by_blob.values() for c in f.columns})}
            for f, members in by_blob.values():
                every = len(members) == len(live)
                sel = None if every else torch.as_tensor(members, device=dev)
                pick = lambda t: t if every or t is None else t[sel]
                s, r, status = formula_rescore(
                    pick(scores), pick(rows), f.blob(), k, ncand if every else ncand[members],
                    pick(tags) if f.has_cond else None,
                    {c: pick(keys[c]) for c in f.columns})
                status = status.cpu().numpy()
                if status.any():
                    bits = int(np.bitwise_or.reduce(status))
                    raise ValueError("formula: " + "; ".join(
                        text for bit, text in (
                            (MISSING, "a variable has no value for a candidate (a payload field "
                                      "the point lacks, or a $score[i] of a point outside "
                                      "prefetch i) and no entry in `defaults`"),
                            (NONFINITE, "a candidate's value is not finite (a division by zero "
                                        "without by_zero_default, or an overflow)"),
                            (BAD, "the device refused the compiled program")) if bits & bit))
                for j, h in zip(members, hits_of(s, r)):
                    out[live[j]] = h[:lim[j]]
            return out

    def search_points_formula(self, requests: list, with_vectors=False):
        """search_formula with every hit resolved to its ScoredPoint (score = the formula's
        value) under the same hold of the lock (_points)."""
        with self.lock:
            return self._points(self.search_formula(requests), with_vectors)

    def search_groups(self, queries, group_by: str, limit: int, group_size: int, filters: list,
                      with_vectors=False, candidates: int | None = None,
                      widen: int | None = None):
        """Grouped search (ragmi.groups.search_groups): per request the `limit`
        best groups of points sharing a value of tag field `group_by`, each with its
        `group_size` best hits — exact, whatever `candidates` / `widen` (policy) say. Returns
        per request a list of PointGroup (id = the payload value) whose hits are resolved to
        ScoredPoints under the same hold of the lock (_points). The route counters accumulate
        in `group_stats`."""
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
            q, fl = self._live(queries, filters, live)
            possible = [[v & key_mask] if m & key_mask else every for m, v in fl]
            res = groups.search_groups(self.index, q, self._pairs(fl), key_mask, possible, G, S,
                                       candidates, widen, search=self._exact_lists,
                                       stats=self.group_stats)
            for i, found in zip(live, res):
                points = self._points([hits for _, hits in found], with_vectors)
                out[i] = [models.PointGroup(hits=pts, id=self.tags.value_of(f, key >> shift))
                          for (key, _), pts in zip(found, points)]
            return out

    # ---------------------------------------------------------------- payload queries
    @staticmethod
    def _program_of(c):
        """A compiled filter (not None) as the index's payload queries take it: None for the
        (0, 0) everything filter, else the packed blob of its one program, a legacy (mask,
        value) pair as its one-atom program."""
        if c == (0, 0):
            return None
        return pack_view([c if isinstance(c, FilterProgram) else FilterProgram.maskeq(*c)])

    def order_spec(self, order_by):
        """(field, column, desc, lo, hi) of an order_by argument, a field name or an OrderBy:
        the field must be a declared range field; start_from becomes the inclusive bound on its
        side of the direction. ValueError names what is wrong."""
        ob = order_by if isinstance(order_by, models.OrderBy) else models.OrderBy(key=order_by)
        if not isinstance(ob.key, str) or ob.key not in self.ranges.fields:
            raise ValueError(
                f"order_by {ob.key!r} is not a declared range field (have {self.ranges.fields}): "
                "declare it with create_payload_index (integer, float or datetime); ordering by "
                "a keyword field is not built")
        col = self.ranges.fields.index(ob.key)
        direction = getattr(ob.direction, "value", ob.direction)
        if direction not in (None, models.Direction.ASC.value, models.Direction.DESC.value):
            raise ValueError(f"order_by direction {ob.direction!r}: Direction.ASC or Direction.DESC")
        desc = direction == models.Direction.DESC.value
        lo = hi = None
        if ob.start_from is not None:
            key = self.ranges.key_of(ob.key, ob.start_from)
            if key == KEY_ABSENT:
                kind = self.ranges.kinds[col]
                raise ValueError(
                    f"order_by start_from={ob.start_from!r} is not a value of {kind} field "
                    f"{ob.key!r} (" + ("a datetime or an RFC 3339 string" if kind == "datetime"
                                       else "a number") + ")")
            lo, hi = (None, key) if desc else (key, None)
        return ob.key, col, desc, lo, hi

    def _ordered_rows(self, order_by, limit, c):
        """(field, rows) of an ordered query under compiled filter `c`: the `limit` first rows
        by the field's value (index.order_rows; points without the field are left out). The
        refusals come first; nothing is launched for a filter nothing can match or a limit
        below 1. Called under the lock."""
        field, col, desc, lo, hi = self.order_spec(order_by)
        limit = int(limit)
        if limit > ORDER_MAX:
            raise ValueError(f"an ordered query returns at most {ORDER_MAX} points "
                             f"(RAG_ORDER_MAX), got limit={limit}")
        if c is None or limit < 1 or not self.row_ids:
            return field, []
        rows = self.index.order_rows(col, limit, desc, lo, hi, self._program_of(c))[1]
        return field, rows.cpu().tolist()

    def record(self, row: int, with_payload=True, with_vectors=False, order_field=None):
        """Row `row` as a Record; `order_field`: the payload field whose stored value becomes
        order_value. Called under the lock."""
        p = self.point(row, 0.0, with_payload, with_vectors)
        value = (self.payloads[row] or {}).get(order_field) if order_field is not None else None
        return models.Record(id=p.id, payload=p.payload, vector=p.vector, order_value=value)

    def scroll(self, flt, limit: int = 10, offset=None, with_payload=True, with_vectors=False,
               order_by=None):
        """The engine of QdrantClient.scroll: (records, next_page_offset). Without order_by the
        page holds the first `limit` matching points in storage (row) order from the row of
        point `offset` on — one select_rows_from of limit + 1 rows, the extra row's id being
        the next offset — and storage order is stable between writes (a delete moves tail rows
        into the holes). With order_by: the `limit` first points by that range field's value,
        no paging. The rows become Records under the same hold of the lock as the select."""
        if order_by is not None and offset is not None:
            raise ValueError("scroll: offset cannot be used together with order_by; continue an "
                             "ordered scroll with OrderBy(start_from=...)")
        limit = int(limit)
        with self.lock:
            c = self.compile_filter(flt)
            if order_by is not None:
                field, rows = self._ordered_rows(order_by, limit, c)
                return [self.record(r, with_payload, with_vectors, field) for r in rows], None
            row0 = 0
            if offset is not None:
                row0 = self.id_to_row.get(_norm_id(offset))
                if row0 is None:
                    raise ValueError(f"scroll: offset {offset!r} is not the id of a point of "
                                     f"collection {self.name!r}")
            if c is None or limit < 1 or not self.row_ids:
                return [], None
            rows = self.index.select_rows_from(row0, self._program_of(c), cap=limit + 1)[0]
            rows = rows.cpu().tolist()
            nxt = self.row_ids[rows[limit]] if len(rows) > limit else None
            return [self.record(r, with_payload, with_vectors) for r in rows[:limit]], nxt

    def search_points_order(self, requests: list, with_vectors=False) -> list:
        """The ORDER route: per request (order_by, compiled filter, limit) its `limit` first
        points by the field's value as ScoredPoints, score 0.0 and order_value set; one
        order_rows per request, resolved under the same hold of the lock."""
        out = []
        with self.lock:
            for order_by, c, limit in requests:
                field, rows = self._ordered_rows(order_by, limit, c)
                pts = []
                for r in rows:
                    p = self.point(r, 0.0, True, with_vectors)
                    p.order_value = (self.payloads[r] or {}).get(field)
                    pts.append(p)
                out.append(pts)
        return out

    def facet(self, key: str, flt, limit: int = 10) -> list:
        """[(value, count)] of tag field `key` over the points a Filter matches: one
        facet_counts call with n_codes = the codebook's size, code 0 (field absent) and zero
        counts dropped, ordered by (count desc, value asc; values that do not compare with each
        other by their str), the first `limit`. Exact."""
        if key not in self.tags.fields:
            raise NotImplementedError(
                f"facet on {key!r}: facets count the keyword fields fixed when the collection is "
                f"created (payload_tag_fields={self.tags.fields}); a facet on a range field is "
                "not built")
        f = self.tags.fields.index(key)
        with self.lock:
            c = self.compile_filter(flt)
            values = list(self.tags.codes[f])          # code i + 1 -> values[i]
            if c is None or int(limit) < 1 or not values or not self.row_ids:
                return []
            counts = self.index.facet_counts(f, len(values), self._program_of(c)).cpu().tolist()
        hits = [(v, n) for v, n in zip(values, counts[1:]) if n > 0]
        try:
            hits.sort(key=lambda h: (-h[1], h[0]))
        except TypeError:
            hits.sort(key=lambda h: (-h[1], str(h[0])))
        return hits[:int(limit)]

    def point(self, row: int, score: float, with_payload=True, with_vectors=False):
        payload = self.payloads[row] if with_payload else None
        vec = None
        if with_vectors:
            vec = (self.index.export_rows32(row, 1)[0] if self.index.storage == "fp32" else
                   self.index.export_rows(row, 1)[0].view(np.float16).astype(np.float32)).tolist()
            if self.sparse_name is not None:     # a collection with a sparse vector names both
                t, v = self.index.sparse_gather(np.asarray([row], dtype=np.int64))
                vec = {"": vec, self.sparse_name: unpack_row(t[0].cpu().numpy(),
                                                             v[0].cpu().numpy())}
        return models.ScoredPoint(id=self.row_ids[row], version=self.versions[row],
                                  score=score, payload=payload, vector=vec)
