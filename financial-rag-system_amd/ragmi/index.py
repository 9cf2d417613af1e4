"""FlatIndex — Python handle over the in-HBM flat cosine index of libragmi.so.

This is the storage + search engine that replaces the Qdrant server's COSINE collection
(reference main.py:92-95 get_qdrant, main.py:215-239 retrieve_from_qdrant, ingest.py:86-96
ensure_collection, ingest.py:148-175 upsert). Vectors live in HBM as fp16 in the MFMA
"tile16" layout; search runs the HIP scan + top-k + exact-rescoring merge on
the caller's current torch stream. Inputs may be numpy arrays (copied to the device) or cuda
torch tensors (used in place).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from .filters import (KEY_ABSENT, KEY_MAX, KEY_MIN, KEYS_MAX_COLS, MAX_PROGRAMS, REC_WORDS,
                      view_programs)

MAX_K = 32          # RAG_MAX_K in include/ragmi.h: the scan's certified top-k path
MAX_K_LARGE = 4096  # RAG_MAX_K_LARGE: k in (32, 4096] takes the exact large-k pass; larger k
                    # the full exact pass (and the packed exchange form stops here)
QUERY_TILE = 32     # RAG_QUERY_TILE
MMR_MAX_CANDIDATES = 1024   # RAG_MMR_MAX_CANDIDATES: the longest list rag_index_mmr re-selects from
GROUPS_MAX_CANDIDATES = 4096   # RAG_GROUPS_MAX_CANDIDATES: the longest list rag_group_select walks
GROUPS_MAX = 1024              # RAG_GROUPS_MAX: groups per query
GROUPS_MAX_CELLS = 4096        # RAG_GROUPS_MAX_CELLS: groups x hits per group
FUSION_MAX_LISTS = 16          # RAG_FUSION_MAX_LISTS: lists per request rag_fuse_rrf fuses
FUSION_MAX_ENTRIES = 4096      # RAG_FUSION_MAX_ENTRIES: lists x entries per list
ORDER_MAX = 4096               # RAG_ORDER_MAX: the longest list rag_index_order_rows returns
ORDER_DESC = 1                 # RAG_ORDER_DESC
SEARCH_FULL = 1     # RAG_SEARCH_FULL (rag_index_search_view)
STORAGE = {"fp16": 0, "fp32": 1}   # RAG_STORE_FP16 / RAG_STORE_FP32
PRESCAN_OFF, PRESCAN_AUTO, PRESCAN_ALWAYS = 0, 1, 2   # RAG_PRESCAN_*: FlatIndex.set_prescan
PRESCAN_ALWAYS6 = 3            # RAG_PRESCAN_ALWAYS6: every k <= 32 pass over the 6-bit copy
PRESCAN_MIN_ROWS = 500000      # RAG_PRESCAN_MIN_ROWS: auto mode's smallest shard
PRESCAN6_MIN_ROWS = 4000000    # RAG_PRESCAN6_MIN_ROWS: auto mode's smallest 6-bit shard
CREATE_DIAGNOSTIC = 0x100          # RAG_CREATE_DIAGNOSTIC: honour the RAGMI_* A/B knobs
RECO_AVERAGE, RECO_BEST, RECO_SUM = 0, 1, 2   # RAG_RECO_AVERAGE / _BEST / _SUM
RECO_MAX_SIDE = 16                 # RAG_RECO_MAX_SIDE: examples per side of a recommend request
DISCOVER_MAX_PAIRS = 15            # RAG_DISCOVER_MAX_PAIRS: pairs of a discover request (a target)
CONTEXT_MAX_PAIRS = 16             # RAG_CONTEXT_MAX_PAIRS: pairs of a context request (no target)
RECO_STRATEGIES = {"average_vector": RECO_AVERAGE, "best_score": RECO_BEST,
                   "sum_scores": RECO_SUM}
SPARSE_TERM_NONE = 0xFFFF          # RAG_SPARSE_TERM_NONE: the term of an empty slot
SPARSE_TERMS = 65535               # sparse terms lie in [0, SPARSE_TERMS)
SPARSE_SLOTS = 128                 # default slots per row of a sparse column
SPARSE_MAX_SLOTS = 512             # RAG_SPARSE_MAX_SLOTS
SPARSE_MAX_QUERY_NNZ = 64          # RAG_SPARSE_MAX_QUERY_NNZ: slots of a padded sparse query
SPARSE_MAX_UNION = 512             # RAG_SPARSE_MAX_UNION: distinct terms of one pass's queries


def sparse_groups(q_terms, q_nnz, max_queries: int = QUERY_TILE,
                  max_union: int = SPARSE_MAX_UNION) -> list:
    """The passes of a sparse search: [(b0, b1), ...] covering the B padded queries in order,
    each a run of at most `max_queries` consecutive queries whose distinct terms number at most
    `max_union` (the scorer's LDS weight table). Greedy: a query that would overflow the union
    opens the next pass; one query alone always fits (64 <= 512). Pure host code."""
    groups, b0, union = [], 0, set()
    for b in range(len(q_nnz)):
        terms = set(np.asarray(q_terms[b][:int(q_nnz[b])]).tolist())
        if b > b0 and (b - b0 == max_queries or len(union | terms) > max_union):
            groups.append((b0, b))
            b0, union = b, set()
        union |= terms
    if len(q_nnz) > b0:
        groups.append((b0, len(q_nnz)))
    return groups


class DiscoverStats(NamedTuple):
    """rag_index_discover_stats: discover / context passes since creation by path, and the last
    hot pass's counted candidates (of its last round) and rounds."""
    hot: int
    full: int
    candidates: int
    rounds: int


class RecoStats(NamedTuple):
    """rag_index_reco_stats: recommend passes since creation by path, and the last hot pass's
    counted candidates (of its last round) and rounds."""
    hot: int
    full: int
    candidates: int
    rounds: int


def reco_strategy(strategy) -> int:
    """A recommend strategy — None (average_vector), a RecommendStrategy, its value, or a
    RAG_RECO_* code — as its code; ValueError for anything else."""
    s = getattr(strategy, "value", strategy)
    if s is None:
        return RECO_AVERAGE
    if isinstance(s, str) and s in RECO_STRATEGIES:
        return RECO_STRATEGIES[s]
    if isinstance(s, (int, np.integer)) and not isinstance(s, bool) and \
            int(s) in RECO_STRATEGIES.values():
        return int(s)
    raise ValueError(f"unknown recommend strategy {strategy!r}: one of {sorted(RECO_STRATEGIES)}")


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _as_dev(x, dtype, device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=dtype)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(dtype=dtype)
        t = t.to(device=device, non_blocking=False)
    return t.contiguous()


def host_or_tensor(x):
    """Vectors as the index calls take them: a tensor stays a tensor (used in place), anything
    else becomes a float32 host array."""
    return x if isinstance(x, torch.Tensor) else np.asarray(x, np.float32)


def hits_of(scores, rows) -> list:
    """Exact lists [B, k] (tensors or arrays) -> per query [(row, score)] without the -1
    padding. Reads device lists back."""
    s = scores.cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)
    r = rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    return [[(int(x), float(sc)) for x, sc in zip(rj, sj) if x >= 0] for rj, sj in zip(r, s)]


def view_blob(programs, n_programs, device):
    """A filter-program blob (ragmi.filters.pack_view; a uint32 host array, or an int32 cuda
    tensor already on `device`) as the *_view calls take it: (int32 cuda tensor, words, U).
    `n_programs` None: read off the blob (filters.view_programs; host arrays only)."""
    if isinstance(programs, torch.Tensor):
        if n_programs is None:
            raise ValueError("a device blob needs n_programs")
        t = programs.to(device=device, dtype=torch.int32).contiguous().reshape(-1)
    else:
        a = np.ascontiguousarray(np.asarray(programs, dtype=np.uint32).reshape(-1))
        if n_programs is None:
            n_programs = view_programs(a)
        t = torch.from_numpy(a.view(np.int32)).to(device)
    U = int(n_programs)
    if not 1 <= U <= MAX_PROGRAMS or t.numel() < U * REC_WORDS:
        raise ValueError(f"a view blob holds 1 to {MAX_PROGRAMS} program records of "
                         f"{REC_WORDS} words")
    return t, t.numel(), U


def per_query(x, B: int, dtype, what: str) -> np.ndarray:
    """A scalar or one value per query -> a contiguous [B] host array of `dtype`."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.ndim == 0:
        a = np.full((B,), a)
    if a.shape != (B,):
        raise ValueError(f"{what} must be a scalar or one value per query")
    return np.ascontiguousarray(a.astype(dtype))


def plan_removal(count: int, rows):
    """The removal rule, the one place every layer takes it from (FlatIndex.remove_rows,
    ShardSet.remove_rows, Collection.delete). `rows`: the rows to delete, in [0, count),
    duplicates allowed. With D the distinct deleted rows and n1 = count - |D|: the holes
    D ∩ [0, n1), ascending, receive the survivors of the tail [n1, count) \\ D, ascending, pair
    by pair; no other row moves. Returns (src, dst, n1): row src[i] moves to slot dst[i]
    (int64 arrays, both ascending, src >= n1 > dst) and n1 is the new count. At most |D| rows
    move, so a delete costs what it deletes, not what the collection holds. Pure host code."""
    count = int(count)
    d = np.unique(np.asarray(rows, dtype=np.int64).reshape(-1))
    if d.size and (d[0] < 0 or d[-1] >= count):
        raise IndexError(f"rows to remove must lie in [0, {count})")
    n1 = count - int(d.size)
    dst = d[d < n1]
    stays = np.ones(count - n1, dtype=bool)
    stays[d[d >= n1] - n1] = False
    src = n1 + np.nonzero(stays)[0].astype(np.int64)
    return src, dst, n1


def order_bounds(lo, hi) -> tuple[int, int]:
    """The key bounds of order_rows with None filled in: the full interval of present keys."""
    return (KEY_MIN if lo is None else int(lo)), (KEY_MAX if hi is None else int(hi))


def order_rows_np(keys, limit: int, desc: bool = False, lo=None, hi=None, passing=None):
    """numpy restatement of rag_index_order_rows over one key column of `count` rows (`keys`
    int64 [count]; `passing`: bool [count], the rows the filter lets through, None = all):
    (keys, rows, eligible) of the `limit` best eligible rows by (key asc, row asc), or with
    `desc` (key desc, row asc). Eligible: passing, key != KEY_ABSENT, lo <= key <= hi."""
    k = np.asarray(keys, np.int64).reshape(-1)
    lo, hi = order_bounds(lo, hi)
    ok = (k != KEY_ABSENT) & (k >= lo) & (k <= hi)
    if passing is not None:
        ok &= np.asarray(passing, bool).reshape(-1)
    rows = np.nonzero(ok)[0].astype(np.int64)
    kk = k[rows]
    # a descending key order as an ascending one: ~k reverses int64 without overflow
    order = np.lexsort((rows, ~kk if desc else kk))[:int(limit)]
    return kk[order], rows[order], int(rows.size)


def facet_counts_np(tags, field: int, n_codes: int, passing=None) -> np.ndarray:
    """numpy restatement of rag_index_facet_counts over the tags of `count` rows: int64
    [n_codes + 1], the passing rows per code of tag field `field`; codes above n_codes are not
    counted."""
    t = np.asarray(tags, np.uint32).reshape(-1)
    c = ((t >> np.uint32(16 * int(field))) & np.uint32(0xFFFF)).astype(np.int64)
    ok = c <= int(n_codes)
    if passing is not None:
        ok &= np.asarray(passing, bool).reshape(-1)
    return np.bincount(c[ok], minlength=int(n_codes) + 1).astype(np.int64)


def rescue_unanswered(index, s, ids, again) -> None:
    """The rescue rule of FlatIndex.search(rescue=True), over the lists (s, ids) a search just
    returned: a list with a -1 is padding (fewer matching points than k) unless the pass left
    the query unanswered (tier 3: more than 16384 rows tied within the error band of its k-th
    best on the large-k pass), which shows as `index.unanswered()` risen past the watermark
    `index._unanswered`. Only then are the short queries re-run, `again(rows)` answering them
    on the full exact pass, written over their lists and counted in `index.rescued`: an
    unanswered query must never read as "no documents". Host logic over any index."""
    if bool((ids < 0).any()):
        n_un = index.unanswered()
        if n_un > index._unanswered:
            redo = torch.nonzero((ids < 0).any(dim=1)).reshape(-1).tolist()
            s[redo], ids[redo] = again(redo)
            index.rescued += len(redo)
        index._unanswered = n_un


class ListOps:
    """What FlatIndex and ShardSet compose alike from their own search, mmr and gather_tags."""

    def search_mmr(self, queries, k: int, diversity, candidates, filters=None):
        """search(k=C) followed by mmr, C = the largest of `candidates` (a scalar or one value
        per query: how many nearest candidates each query re-selects from), all on the device
        and the current stream. Returns (scores [B, k], rows [B, k]) as mmr does."""
        q, B, f = self._search_args(queries, k, filters)
        nc = per_query(candidates, B, np.int32, "candidates")
        if B and int(nc.min()) < 1:
            raise ValueError("candidates must be >= 1")
        C = int(nc.max()) if B else 1
        if C > MMR_MAX_CANDIDATES:
            raise ValueError(f"at most {MMR_MAX_CANDIDATES} MMR candidates per query")
        s, r = self.search(q, C, f)
        return self.mmr(s, r, k, diversity, None if B and (nc == C).all() else nc)

    def group_select(self, cand_scores, cand_rows, key_mask: int, G: int, S: int, ncand=None,
                     with_pos: bool = False) -> "GroupSelection":
        """The grouped walk over exact candidate lists (search(k=C)'s result; rows of this
        index): gather_tags of the rows, then rag_group_select, both on the current stream.
        The selection reads only the lists, so a ShardSet's result is the one-index result
        bit for bit. See group_select_tags for the result."""
        r = _as_dev(cand_rows, torch.int64, self.device)
        return group_select_tags(_as_dev(cand_scores, torch.float32, self.device), r,
                                 self.gather_tags(r), key_mask, G, S, ncand, with_pos)


class FlatIndex(ListOps):
    """In-HBM flat index with exact (score desc, row asc) top-k search. storage "fp16": the
    fp16 rows only (what the scan streams); "fp32": the normalised fp32 rows too, which the
    exact scores read (Qdrant's default Float32 vectors; rag_index_create_ex).
    diagnostic=True (bench / profiling scripts only) lets the process honour the RAGMI_*
    kernel A/B environment knobs (RAG_CREATE_DIAGNOSTIC); serving code leaves it off, and
    the library then ignores (and reports) any such variable."""

    def __init__(self, dim: int = 384, capacity: int = 0, device=None, storage: str = "fp16",
                 diagnostic: bool = False):
        dev = _lib.resolve_device(device)        # "cpu" refused before any HIP call
        _lib.require_gpu()
        self._L = _lib.load()
        self.device = torch.device("cuda", _lib.device_index(dev))
        self.dim = int(dim)
        if storage not in STORAGE:
            raise ValueError(f"storage must be one of {sorted(STORAGE)}")
        self.storage = storage
        h = ctypes.c_void_p()
        flags = STORAGE[storage] | (CREATE_DIAGNOSTIC if diagnostic else 0)
        check(self._L.rag_index_create_ex(self.dim, int(capacity), self.device.index, flags,
                                          ctypes.byref(h)))
        self._h = h
        self._unanswered = 0     # unanswered() as last read (search, rescue)
        self.rescued = 0         # queries re-answered on the full exact pass (stats)

    # ---------------------------------------------------------------- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.rag_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- properties
    @property
    def capacity(self) -> int:
        return int(self._L.rag_index_capacity(self._h))

    @property
    def count(self) -> int:
        return int(self._L.rag_index_count(self._h))

    def reserve(self, capacity: int) -> None:
        check(self._L.rag_index_reserve(self._h, int(capacity)))

    # ---------------------------------------------------------------- writes
    def upsert(self, vectors, rows, tags=None, new_count: int | None = None) -> None:
        """Normalise + store vectors [n, dim] at row slots `rows` [n] (overwrite allowed)."""
        v = _as_dev(vectors, torch.float32, self.device)
        if v.dim() != 2 or v.shape[1] != self.dim:
            raise ValueError(f"vectors must be [n, {self.dim}]")
        r = _as_dev(rows, torch.int64, self.device)
        n = v.shape[0]
        if r.shape != (n,):
            raise ValueError("rows must be [n]")
        if n and (int(r.min()) < 0 or int(r.max()) >= self.capacity):
            raise IndexError("row slot outside capacity; reserve() first")
        t = None
        if tags is not None:
            t = _as_dev(np.asarray(tags, dtype=np.uint32).view(np.int32)
                        if not isinstance(tags, torch.Tensor) else tags, torch.int32,
                        self.device)
        if new_count is None:
            new_count = max(self.count, int(r.max()) + 1 if n else 0)
        check(self._L.rag_index_upsert(self._h, v.data_ptr(), r.data_ptr(),
                                       t.data_ptr() if t is not None else None, n,
                                       int(new_count), _stream_ptr(self.device)))
        # staging tensors are released to the stream-ordered caching allocator (safe reuse).

    def set_count(self, new_count: int) -> None:
        check(self._L.rag_index_upsert(self._h, None, None, None, 0, int(new_count),
                                       _stream_ptr(self.device)))

    # ---------------------------------------------------------------- search
    def _search_args(self, queries, k, filters, k_max=None):
        if k < 1 or (k_max is not None and k > k_max):
            raise ValueError(f"k must be in [1, {k_max}]" if k_max else "k must be >= 1")
        q = _as_dev(queries, torch.float32, self.device)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.shape[-1] != self.dim:
            raise ValueError(f"query dim {q.shape[-1]} != index dim {self.dim}")
        B = q.shape[0]
        f = None
        if filters is not None:
            if isinstance(filters, torch.Tensor):
                f = filters.to(device=self.device, dtype=torch.int32).contiguous()
            else:
                f = torch.from_numpy(np.ascontiguousarray(
                    np.asarray(filters, dtype=np.uint32).reshape(B, 2)).view(np.int32))
                f = f.to(self.device)
            if f.shape != (B, 2):
                raise ValueError("filters must be [B, 2] (tag_mask, tag_value)")
        return q, B, f

    def _launch(self, q, f, k: int, id_offset: int, view, full=False, lists=None, packed=None):
        """The one search launch behind search and search_packed, on the current stream: into
        `lists` (scores, ids) or into `packed`; over the filter view of `view` (view_blob's
        triple) when there is one, else over the stored tags."""
        fp = f.data_ptr() if f is not None else None
        sp = lists[0].data_ptr() if lists is not None else None
        ip = lists[1].data_ptr() if lists is not None else None
        st = _stream_ptr(self.device)
        if view is not None:
            p, words, U = view
            check(self._L.rag_index_search_view(
                self._h, q.data_ptr(), q.shape[0], int(k), p.data_ptr(), words, U, fp,
                int(id_offset), SEARCH_FULL if full else 0, sp, ip,
                packed.data_ptr() if packed is not None else None, st))
        elif packed is not None:
            check(self._L.rag_index_search_packed(self._h, q.data_ptr(), q.shape[0], int(k), fp,
                                                  int(id_offset), packed.data_ptr(), st))
        else:
            fn = self._L.rag_index_search_full if full else self._L.rag_index_search
            check(fn(self._h, q.data_ptr(), q.shape[0], int(k), fp, int(id_offset), sp, ip, st))
        # staging tensors (q, f) go back to torch's stream-ordered caching allocator: any
        # reuse is enqueued on this same stream after our kernels, so no sync is needed.

    def search_packed(self, queries, k: int, filters=None, id_offset: int = 0,
                      programs=None, n_programs: int | None = None) -> torch.Tensor:
        """Top-k in the multi-GPU exchange form: int32 [B, k, 2] = (fp32 score bits, global
        row; -1 = none), enqueued on the current stream (rag_index_search_packed).
        `programs`: as in search."""
        q, B, f = self._search_args(queries, k, filters, k_max=MAX_K_LARGE)
        view = None if programs is None else view_blob(programs, n_programs, self.device)
        out = torch.empty((B, k, 2), dtype=torch.int32, device=self.device)
        self._launch(q, f, k, id_offset, view, packed=out)
        return out

    def search(self, queries, k: int, filters=None, id_offset: int = 0,
               out: tuple[torch.Tensor, torch.Tensor] | None = None, full: bool = False,
               programs=None, n_programs: int | None = None, rescue: bool = False):
        """Top-k of each query row. Returns (scores fp32 [B,k], ids int64 [B,k]) as cuda
        tensors, enqueued on the current stream (ids -1 where fewer than k rows match).
        `filters`: None, or per-query (tag_mask, tag_value) pairs [B, 2] (uint32).
        Any k >= 1: k <= 32 on the scan, k <= 4096 on the large-k pass, beyond on the full
        exact pass (every row scored exactly, then sorted); full=True forces the full pass
        (rag_index_search_full) — the same result, the path for queries a large-k pass left
        unanswered.
        `programs`: a filter-program blob (ragmi.filters.pack_view). The search then runs over
        the blob's filter view of the tags (rag_index_search_view) and `filters` are (mask,
        value) pairs over the VIEW's bits: (1 << s, 1 << s) asks for program s.
        rescue=True (Collection.search): queries the pass left unanswered are re-run with
        full=True under the same filters and programs (rescue_unanswered; counted in
        `rescued`). Reads the lists back, so it synchronises; without it nothing is read."""
        q, B, f = self._search_args(queries, k, filters)
        view = None if programs is None else view_blob(programs, n_programs, self.device)
        if out is None:
            out = (torch.empty((B, k), dtype=torch.float32, device=self.device),
                   torch.empty((B, k), dtype=torch.int64, device=self.device))
        self._launch(q, f, k, id_offset, view, full, lists=out)
        if rescue and not full:
            p, U = (None, None) if view is None else (view[0], view[2])
            rescue_unanswered(self, *out, lambda redo: self.search(
                q[redo], k, None if f is None else f[redo], id_offset, full=True, programs=p,
                n_programs=U))
        return out

    # ---------------------------------------------------------------- recommend
    def _reco_sides(self, pos, neg, strategy, average_ok=True):
        """(pos tensor or None, P, neg tensor or None, N, strategy code) of a recommend
        request, refused as the C ABI refuses it, but as ValueError."""
        code = reco_strategy(strategy)
        sides = []
        for name, x in (("positive", pos), ("negative", neg)):
            if x is None or len(x) == 0:
                sides.append((None, 0))
                continue
            t = _as_dev(x, torch.float32, self.device)
            if t.dim() == 1:
                t = t.unsqueeze(0)
            if t.dim() != 2 or t.shape[1] != self.dim:
                raise ValueError(f"{name} examples must be [n, {self.dim}]")
            if t.shape[0] > RECO_MAX_SIDE:
                raise ValueError(f"at most {RECO_MAX_SIDE} {name} examples (RAG_RECO_MAX_SIDE), "
                                 f"got {t.shape[0]}")
            sides.append((t, int(t.shape[0])))
        (p, P), (n, N) = sides
        if P + N == 0:
            raise ValueError("a recommend request needs at least one example")
        if code == RECO_AVERAGE and (P == 0 or not average_ok):
            raise ValueError("average_vector needs a positive example" if average_ok else
                             "bounds exist for best_score and sum_scores only")
        return p, P, n, N, code

    def recommend(self, pos, neg, strategy, k: int, filters=None, programs=None,
                  full: bool = False, rescue: bool = False, n_programs: int | None = None,
                  id_offset: int = 0):
        """One recommend request (rag_index_recommend; the contract: include/ragmi.h "Recommend
        queries"): `pos` / `neg` the example vectors [n, dim] (None or empty: none; at most 16
        a side), `strategy` a RecommendStrategy, its value or its RAG_RECO_* code. Returns
        (scores fp32 [k], ids int64 [k]) as cuda tensors, the k best rows by (score desc, row
        asc), -inf / -1 past the matching rows, enqueued on the current stream. The example rows
        themselves are not excluded (Collection.search_recommend does that).
        `filters`: None or one (tag_mask, tag_value) pair; `programs`: a filter-program blob,
        `filters` then being a pair over the view's bits, as in search. full=True forces the
        full pass. rescue=True: a request the hot pass left unanswered (more than 16384 rows
        within its bounds of the k-th best) is re-answered on the full pass and counted in
        `rescued` (rescue_unanswered); reads the list back, so it synchronises."""
        p, P, n, N, code = self._reco_sides(pos, neg, strategy)
        if k < 1:
            raise ValueError("k must be >= 1")
        f = None
        if filters is not None:
            f = torch.from_numpy(np.ascontiguousarray(
                np.asarray(filters, dtype=np.uint32).reshape(2)).view(np.int32)).to(self.device)
        view = None if programs is None else view_blob(programs, n_programs, self.device)
        def launch(full_pass: bool):
            s = torch.empty((1, k), dtype=torch.float32, device=self.device)
            ids = torch.empty((1, k), dtype=torch.int64, device=self.device)
            vp, words, U = (None, 0, 0) if view is None else (view[0].data_ptr(), view[1], view[2])
            check(self._L.rag_index_recommend(
                self._h, p.data_ptr() if P else None, P, n.data_ptr() if N else None, N, code,
                int(k), vp, words, U, f.data_ptr() if f is not None else None, int(id_offset),
                SEARCH_FULL if full_pass else 0, s.data_ptr(), ids.data_ptr(),
                _stream_ptr(self.device)))
            return s, ids

        s, ids = launch(full)
        if rescue and not full:
            rescue_unanswered(self, s, ids, lambda redo: launch(True))
        return s[0], ids[0]

    def reco_bounds(self, pos, neg, strategy, rows):
        """(lo, hi) fp32 [n]: the hot pass's certified bounds of the exact combined score of
        stored rows `rows` (best_score or sum_scores; rag_index_reco_bounds, diagnostic)."""
        p, P, n, N, code = self._reco_sides(pos, neg, strategy, average_ok=False)
        r = _as_dev(rows, torch.int64, self.device).reshape(-1)
        lo = torch.empty((r.numel(),), dtype=torch.float32, device=self.device)
        hi = torch.empty_like(lo)
        check(self._L.rag_index_reco_bounds(
            self._h, p.data_ptr() if P else None, P, n.data_ptr() if N else None, N, code,
            r.data_ptr() if r.numel() else None, r.numel(), lo.data_ptr(), hi.data_ptr(),
            _stream_ptr(self.device)))
        return lo, hi

    def reco_vector(self, pos, neg=None) -> torch.Tensor:
        """average_vector's target v fp32 [dim] (rag_index_reco_vector, diagnostic)."""
        p, P, n, N, _ = self._reco_sides(pos, neg, RECO_AVERAGE)
        v = torch.empty((self.dim,), dtype=torch.float32, device=self.device)
        check(self._L.rag_index_reco_vector(self._h, p.data_ptr(), P,
                                            n.data_ptr() if N else None, N, v.data_ptr(),
                                            _stream_ptr(self.device)))
        return v

    def reco_stats(self) -> "RecoStats":
        """(hot passes, full passes, candidates the last hot pass counted, rounds it ran) —
        rag_index_reco_stats; synchronises the device."""
        out = (ctypes.c_int64 * 4)()
        check(self._L.rag_index_reco_stats(self._h, out))
        return RecoStats(*[int(x) for x in out])

    # ---------------------------------------------------------------- discover
    def _discover_sides(self, target, pairs_pos, pairs_neg):
        """(target tensor or None, pos tensor or None, neg tensor or None, n) of a discover /
        context request, refused as the C ABI refuses it, but as ValueError."""
        t = None
        if target is not None:
            t = _as_dev(target, torch.float32, self.device).reshape(-1)
            if t.numel() != self.dim:
                raise ValueError(f"target must be [{self.dim}]")
        sides = []
        for name, x in (("positive", pairs_pos), ("negative", pairs_neg)):
            if x is None or len(x) == 0:
                sides.append((None, 0))
                continue
            v = _as_dev(x, torch.float32, self.device)
            if v.dim() == 1:
                v = v.unsqueeze(0)
            if v.dim() != 2 or v.shape[1] != self.dim:
                raise ValueError(f"{name} examples must be [n, {self.dim}]")
            sides.append((v, int(v.shape[0])))
        (p, P), (n, N) = sides
        if P != N:
            raise ValueError(f"a context pair is one positive and one negative: got {P} "
                             f"positives and {N} negatives")
        limit, name = (DISCOVER_MAX_PAIRS, "RAG_DISCOVER_MAX_PAIRS") if t is not None else \
            (CONTEXT_MAX_PAIRS, "RAG_CONTEXT_MAX_PAIRS")
        if P > limit:
            raise ValueError(f"at most {limit} context pairs ({name}), got {P}")
        if t is None and P == 0:
            raise ValueError("a context search (no target) needs at least one pair")
        return t, p, n, P

    def discover(self, target, pairs_pos, pairs_neg, k: int, filters=None, programs=None,
                 full: bool = False, rescue: bool = False, n_programs: int | None = None,
                 id_offset: int = 0):
        """One discovery request (rag_index_discover; the contract: include/ragmi.h "Discovery
        queries"): `target` a vector [dim] or None (None: a context search), `pairs_pos` /
        `pairs_neg` the pairs' positive and negative vectors [n, dim], pair i being
        (pairs_pos[i], pairs_neg[i]) — at most 15 with a target, 1 to 16 without. Returns
        (scores fp32 [k], ids int64 [k]) as cuda tensors, the k best rows by (score desc, row
        asc), -inf / -1 past the matching rows, enqueued on the current stream. Example rows are
        not excluded (Collection.search_discover does that). `filters`, `programs`, `full` as in
        recommend. rescue=True: a request the hot pass left unanswered (more than 16384 rows
        tied within its bounds of the k-th best: a context search with few pairs, a zero
        target) is re-answered on the full pass and counted in `rescued` (rescue_unanswered);
        reads the list back, so it synchronises."""
        t, p, n, P = self._discover_sides(target, pairs_pos, pairs_neg)
        if k < 1:
            raise ValueError("k must be >= 1")
        f = None
        if filters is not None:
            f = torch.from_numpy(np.ascontiguousarray(
                np.asarray(filters, dtype=np.uint32).reshape(2)).view(np.int32)).to(self.device)
        view = None if programs is None else view_blob(programs, n_programs, self.device)

        def launch(full_pass: bool):
            s = torch.empty((1, k), dtype=torch.float32, device=self.device)
            ids = torch.empty((1, k), dtype=torch.int64, device=self.device)
            vp, words, U = (None, 0, 0) if view is None else (view[0].data_ptr(), view[1], view[2])
            check(self._L.rag_index_discover(
                self._h, t.data_ptr() if t is not None else None,
                p.data_ptr() if P else None, n.data_ptr() if P else None, P, int(k), vp, words, U,
                f.data_ptr() if f is not None else None, int(id_offset),
                SEARCH_FULL if full_pass else 0, s.data_ptr(), ids.data_ptr(),
                _stream_ptr(self.device)))
            return s, ids

        s, ids = launch(full)
        if rescue and not full:
            rescue_unanswered(self, s, ids, lambda redo: launch(True))
        return s[0], ids[0]

    def discover_bounds(self, target, pairs_pos, pairs_neg, rows):
        """(lo, hi) fp32 [n]: the hot pass's certified bounds of the exact discover / context
        score of stored rows `rows` (rag_index_discover_bounds, diagnostic)."""
        t, p, n, P = self._discover_sides(target, pairs_pos, pairs_neg)
        r = _as_dev(rows, torch.int64, self.device).reshape(-1)
        lo = torch.empty((r.numel(),), dtype=torch.float32, device=self.device)
        hi = torch.empty_like(lo)
        check(self._L.rag_index_discover_bounds(
            self._h, t.data_ptr() if t is not None else None, p.data_ptr() if P else None,
            n.data_ptr() if P else None, P, r.data_ptr() if r.numel() else None, r.numel(),
            lo.data_ptr(), hi.data_ptr(), _stream_ptr(self.device)))
        return lo, hi

    def discover_stats(self) -> "DiscoverStats":
        """(hot passes, full passes, candidates the last hot pass counted, rounds it ran) —
        rag_index_discover_stats; synchronises the device."""
        out = (ctypes.c_int64 * 4)()
        check(self._L.rag_index_discover_stats(self._h, out))
        return DiscoverStats(*[int(x) for x in out])

    # ---------------------------------------------------------------- MMR
    def mmr(self, cand_scores, cand_rows, k: int, diversity, ncand=None,
            with_pos: bool = False):
        """Maximal marginal relevance over exact candidate lists (rag_index_mmr): k diverse
        hits re-selected from each query's top-C list `cand_scores` fp32 [B, C] / `cand_rows`
        int64 [B, C] (rows of this index, -1 = none; search(k=C)'s result). `diversity`: a
        scalar or one value per query in [0, 1] (0: the plain top-k, 1: similarity to the
        picks alone); `ncand`: None, a scalar or one value per query — only the first ncand[b]
        candidates of query b take part. Returns (scores fp32 [B, k], rows int64 [B, k]) in
        selection order, the score being the candidate's score to the query, -inf / -1 past
        the last pick; with_pos=True adds each pick's position in its list (int32 [B, k]).
        Enqueued on the current stream."""
        s = _as_dev(cand_scores, torch.float32, self.device)
        r = _as_dev(cand_rows, torch.int64, self.device)
        if s.dim() != 2 or s.shape != r.shape:
            raise ValueError("cand_scores and cand_rows must both be [B, C]")
        B, C = s.shape
        if not 1 <= C <= MMR_MAX_CANDIDATES:
            raise ValueError(f"C must be in [1, {MMR_MAX_CANDIDATES}] candidates")
        if k < 1:
            raise ValueError("k must be >= 1")
        div = per_query(diversity, B, np.float32, "diversity")
        if B and not ((div >= 0) & (div <= 1)).all():        # also refuses NaN
            raise ValueError("diversity must lie in [0, 1]")
        d = torch.from_numpy(div).to(self.device)
        n = None
        if ncand is not None:
            n = torch.from_numpy(per_query(ncand, B, np.int32, "ncand")).to(self.device)
        out_s = torch.empty((B, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((B, k), dtype=torch.int64, device=self.device)
        pos = torch.empty((B, k), dtype=torch.int32, device=self.device) if with_pos else None
        check(self._L.rag_index_mmr(self._h, s.data_ptr(), r.data_ptr(), B, C, int(k),
                                    d.data_ptr(), n.data_ptr() if n is not None else None,
                                    out_s.data_ptr(), out_i.data_ptr(),
                                    pos.data_ptr() if pos is not None else None,
                                    _stream_ptr(self.device)))
        return (out_s, out_i, pos) if with_pos else (out_s, out_i)

    # ---------------------------------------------------------------- grouped search
    def gather_tags(self, rows) -> torch.Tensor:
        """The tags of `rows` (int64, any shape; rag_index_gather_tags): an int32 tensor of the
        same shape holding the uint32 tag bits, 0 for a row outside [0, capacity) — such a row
        is never dereferenced. Enqueued on the current stream."""
        r = _as_dev(rows, torch.int64, self.device)
        out = torch.empty(r.shape, dtype=torch.int32, device=self.device)
        if r.numel():
            check(self._L.rag_index_gather_tags(self._h, r.data_ptr(), r.numel(), out.data_ptr(),
                                                _stream_ptr(self.device)))
        return out

    # ---------------------------------------------------------------- key columns
    def keys_create(self, n_cols: int) -> None:
        """Make the index hold `n_cols` key columns (1..4; rag_index_keys_create): int64
        [capacity] each, what the RANGE atom of a filter program compares. The number only
        grows; new columns hold KEY_ABSENT. Synchronises the device."""
        check(self._L.rag_index_keys_create(self._h, int(n_cols)))

    def keys_cols(self) -> int:
        """The number of key columns (rag_index_keys_cols)."""
        return int(self._L.rag_index_keys_cols(self._h))

    def write_keys(self, col: int, rows, keys) -> None:
        """keys[col][rows[i]] = keys[i] (int64 [n]; rag_index_write_keys): distinct rows, one
        outside [0, capacity) is skipped. Enqueued on the current stream."""
        r = _as_dev(rows, torch.int64, self.device).reshape(-1)
        k = _as_dev(keys, torch.int64, self.device).reshape(-1)
        if r.shape != k.shape:
            raise ValueError("rows and keys must pair up")
        check(self._L.rag_index_write_keys(self._h, int(col), r.data_ptr() if r.numel() else None,
                                           k.data_ptr() if r.numel() else None, r.numel(),
                                           _stream_ptr(self.device)))

    def gather_keys(self, col: int, rows) -> torch.Tensor:
        """The keys of column `col` at `rows` (int64, any shape; rag_index_gather_keys): an
        int64 tensor of the same shape, KEY_ABSENT for a row outside [0, capacity) — such a row
        is never dereferenced. Enqueued on the current stream."""
        r = _as_dev(rows, torch.int64, self.device)
        out = torch.empty(r.shape, dtype=torch.int64, device=self.device)
        check(self._L.rag_index_gather_keys(self._h, int(col), r.data_ptr() if r.numel() else None,
                                            r.numel(), out.data_ptr() if r.numel() else None,
                                            _stream_ptr(self.device)))
        return out

    # ---------------------------------------------------------------- sparse column
    def sparse_create(self, slots: int = SPARSE_SLOTS) -> None:
        """Make the index hold a sparse column of `slots` slots per row (a multiple of 16 in
        [16, 512]; rag_index_sparse_create): terms uint16 and values fp32 [capacity, slots], new
        rows empty. The same slot count again is a no-op, another one refused. Synchronises the
        device."""
        check(self._L.rag_index_sparse_create(self._h, int(slots)))

    def sparse_slots(self) -> int:
        """Slots per row of the sparse column, 0 without one (rag_index_sparse_slots)."""
        return int(self._L.rag_index_sparse_slots(self._h))

    def _sparse_rows(self, rows):
        S = self.sparse_slots()
        if S == 0:
            raise ValueError("the index has no sparse column (sparse_create)")
        return S, _as_dev(rows, torch.int64, self.device).reshape(-1)

    def sparse_write(self, rows, terms, vals) -> None:
        """Sparse row rows[i] = (terms[i], vals[i]): uint16 / fp32 [n, slots] in the stored layout
        (ragmi.sparse.pack_rows; include/ragmi.h "Sparse vectors"), distinct rows, one outside
        [0, capacity) skipped (rag_index_sparse_write). Enqueued on the current stream."""
        S, r = self._sparse_rows(rows)
        t = _as_dev(np.asarray(terms, np.uint16).view(np.int16)
                    if not isinstance(terms, torch.Tensor) else terms, torch.int16, self.device)
        v = _as_dev(vals, torch.float32, self.device)
        if tuple(t.shape) != (r.numel(), S) or tuple(v.shape) != (r.numel(), S):
            raise ValueError(f"terms and vals must be [n, {S}]")
        if r.numel():
            check(self._L.rag_index_sparse_write(self._h, r.data_ptr(), t.data_ptr(), v.data_ptr(),
                                                 r.numel(), _stream_ptr(self.device)))

    def sparse_gather(self, rows):
        """The stored sparse rows of `rows`: (terms int16 [n, slots] holding the uint16 bits, vals
        fp32 [n, slots]) as cuda tensors, an empty row for a row outside [0, capacity)
        (rag_index_sparse_gather). Enqueued on the current stream."""
        S, r = self._sparse_rows(rows)
        t = torch.empty((r.numel(), S), dtype=torch.int16, device=self.device)
        v = torch.empty((r.numel(), S), dtype=torch.float32, device=self.device)
        if r.numel():
            check(self._L.rag_index_sparse_gather(self._h, r.data_ptr(), r.numel(), t.data_ptr(),
                                                  v.data_ptr(), _stream_ptr(self.device)))
        return t, v

    def sparse_df(self) -> torch.Tensor:
        """Document frequency: an int64 cuda tensor [65535], entry t the rows below the count
        that hold term t (rag_index_sparse_df). Enqueued on the current stream."""
        out = torch.empty((SPARSE_TERMS,), dtype=torch.int64, device=self.device)
        check(self._L.rag_index_sparse_df(self._h, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def sparse_search(self, q_terms, q_vals, q_nnz, k: int, filters=None, programs=None,
                      n_programs: int | None = None, full: bool = False, rescue: bool = False,
                      id_offset: int = 0):
        """Top-k of B sparse queries by the sparse score (rag_index_sparse_search; the contract:
        include/ragmi.h "Sparse vectors"). The queries are padded host arrays
        (ragmi.sparse.pack_rows at 64 slots): q_terms uint16 [B, 64] ascending, q_vals fp32
        [B, 64], q_nnz [B]. Returns (scores fp32 [B, k], ids int64 [B, k]) as cuda tensors, -inf /
        -1 past the eligible rows. `filters`, `programs`: as in search. The queries go to the
        device in groups of consecutive queries, at most 32 and at most SPARSE_MAX_UNION distinct
        terms each (sparse_groups): one pass of the hot path per group. full=True forces the full
        pass. rescue=True: queries the hot pass left unanswered (more than 16384 rows at or above
        the threshold) are re-run on the full pass (rescue_unanswered; synchronises)."""
        qt = np.ascontiguousarray(np.asarray(q_terms, np.uint16))
        qv = np.ascontiguousarray(np.asarray(q_vals, np.float32))
        qn = np.ascontiguousarray(np.asarray(q_nnz, np.int32).reshape(-1))
        B = qn.shape[0]
        if qt.shape != (B, SPARSE_MAX_QUERY_NNZ) or qv.shape != qt.shape:
            raise ValueError(f"sparse queries are padded to [B, {SPARSE_MAX_QUERY_NNZ}]")
        if B and (int(qn.min()) < 0 or int(qn.max()) > SPARSE_MAX_QUERY_NNZ):
            raise ValueError(f"a sparse query holds 0 to {SPARSE_MAX_QUERY_NNZ} nonzeros")
        if k < 1:
            raise ValueError("k must be >= 1")
        if self.sparse_slots() == 0:
            raise ValueError("the index has no sparse column (sparse_create)")
        f = None
        if filters is not None:
            f = torch.from_numpy(np.ascontiguousarray(
                np.asarray(filters, dtype=np.uint32).reshape(B, 2)).view(np.int32)).to(self.device)
        view = None if programs is None else view_blob(programs, n_programs, self.device)
        vp, words, U = (None, 0, 0) if view is None else (view[0].data_ptr(), view[1], view[2])
        s = torch.empty((B, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((B, k), dtype=torch.int64, device=self.device)
        t_dev = torch.from_numpy(qt.view(np.int16)).to(self.device)
        v_dev = torch.from_numpy(qv).to(self.device)
        n_dev = torch.from_numpy(qn).to(self.device)
        for b0, b1 in ([(0, B)] if full else sparse_groups(qt, qn)):
            check(self._L.rag_index_sparse_search(
                self._h, t_dev[b0:].data_ptr(), v_dev[b0:].data_ptr(), n_dev[b0:].data_ptr(),
                b1 - b0, int(k), vp, words, U, f[b0:].data_ptr() if f is not None else None,
                int(id_offset), SEARCH_FULL if full else 0, s[b0:].data_ptr(),
                ids[b0:].data_ptr(), _stream_ptr(self.device)))
        if rescue and not full:
            def again(redo):
                return self.sparse_search(qt[redo], qv[redo], qn[redo], k,
                                          None if f is None else f[redo].cpu().numpy(),
                                          None if view is None else view[0], U or None, full=True,
                                          id_offset=id_offset)
            rescue_unanswered(self, s, ids, again)
        return s, ids

    # ---------------------------------------------------------------- row removal
    def select_rows(self, tag_mask: int, tag_value: int, cap: int | None = None,
                    out: torch.Tensor | None = None):
        """Rows r < count with (tag[r] & tag_mask) == tag_value, ascending
        (rag_index_select_rows): (rows int64 cuda tensor, total). At most `cap` rows are
        written (default: every match), the first ones; `total` counts every match. cap = 0 is
        a pure count. `out`: an int64 cuda tensor of at least `cap` elements to write into.
        Synchronises the current stream (the total is read back)."""
        if cap is None:
            cap = self.count if out is None else min(self.count, out.numel())
        return self._selected(cap, out, lambda rows, cap, n, st: self._L.rag_index_select_rows(
            self._h, int(tag_mask) & 0xFFFFFFFF, int(tag_value) & 0xFFFFFFFF, rows, cap, n, st))

    def _out(self, out, n: int, dtype, what: str) -> torch.Tensor:
        """A caller's `out=` buffer checked, or a fresh one: `n` elements of `dtype` here."""
        if out is None:
            return torch.empty((n,), dtype=dtype, device=self.device)
        if out.dtype != dtype or out.device != self.device or out.numel() < n \
                or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {str(dtype)[6:]} tensor of >= {what} "
                             "elements on the index's device")
        return out

    def _selected(self, cap, out, launch):
        """The tail of both selects: `launch(rows, cap, total, stream)` writes at most `cap`
        rows and the count of every match; (out[:min(total, cap)], total)."""
        cap = int(cap)
        if cap < 0:
            raise ValueError("cap must be >= 0")
        out = self._out(out, cap, torch.int64, "cap")
        n = torch.empty((1,), dtype=torch.int64, device=self.device)
        check(launch(out.data_ptr() if cap else None, cap, n.data_ptr(),
                     _stream_ptr(self.device)))
        total = int(n.item())
        return out[:min(total, cap)], total

    def filter_view(self, programs, n_programs: int | None = None,
                    out: torch.Tensor | None = None) -> torch.Tensor:
        """The filter view of the stored tags (rag_index_filter_view): an int32 cuda tensor
        [capacity] holding the uint32 words, bit s of word r = row r passes program s of the
        blob, 0 for rows at or past the count. `out`: a contiguous int32 tensor of at least
        `capacity` elements to write into. Enqueued on the current stream."""
        p, words, U = view_blob(programs, n_programs, self.device)
        cap = self.capacity
        out = self._out(out, cap, torch.int32, "capacity")
        check(self._L.rag_index_filter_view(self._h, p.data_ptr(), words, U, out.data_ptr(),
                                            _stream_ptr(self.device)))
        return out[:cap]

    def select_rows_view(self, programs, cap: int | None = None):
        """select_rows of the rows passing ONE filter program (the blob's first record;
        rag_index_select_rows_view): (rows int64 cuda tensor, total). Synchronises the current
        stream (the total is read back)."""
        p, words, _ = view_blob(programs, 1, self.device)
        return self._selected(self.count if cap is None else cap, None,
                              lambda rows, cap, n, st: self._L.rag_index_select_rows_view(
                                  self._h, p.data_ptr(), words, rows, cap, n, st))

    # ---------------------------------------------------------------- payload queries
    def _program(self, programs):
        """(blob tensor, its pointer, words) of the ONE filter program of a payload query;
        (None, None, 0) for programs = None, every row. The caller holds the tensor until its
        launch is enqueued."""
        if programs is None:
            return None, None, 0
        p, words, _ = view_blob(programs, 1, self.device)
        return p, p.data_ptr(), words

    def select_rows_from(self, row0: int, programs=None, cap: int | None = None):
        """select_rows_view restricted to rows >= row0 (rag_index_select_rows_from; programs
        None = every row): (rows int64 cuda tensor, total at or after row0). Synchronises the
        current stream (the total is read back)."""
        row0 = int(row0)
        if row0 < 0:
            raise ValueError("row0 must be >= 0")
        p, ptr, words = self._program(programs)
        if cap is None:
            cap = max(self.count - row0, 0)
        return self._selected(cap, None,
                              lambda rows, cap, n, st: self._L.rag_index_select_rows_from(
                                  self._h, ptr, words, row0, rows, cap, n, st))

    def order_rows(self, col: int, limit: int, desc: bool = False, lo=None, hi=None,
                   programs=None):
        """The `limit` best eligible rows of key column `col` (rag_index_order_rows): (keys
        int64 [n], rows int64 [n], eligible), n = min(limit, eligible), ordered by (key asc, row
        asc) or with `desc` (key desc, row asc). Eligible: below the count, passing the ONE
        program of `programs` (None = every row), key present and lo <= key <= hi (None = no
        bound). 1 <= limit <= ORDER_MAX. Synchronises the current stream (n is read back)."""
        limit = int(limit)
        if not 1 <= limit <= ORDER_MAX:
            raise ValueError(f"order_rows: limit must lie in [1, {ORDER_MAX}]")
        lo, hi = order_bounds(lo, hi)
        p, ptr, words = self._program(programs)
        keys = torch.empty((limit,), dtype=torch.int64, device=self.device)
        rows = torch.empty((limit,), dtype=torch.int64, device=self.device)
        n = torch.empty((2,), dtype=torch.int64, device=self.device)
        check(self._L.rag_index_order_rows(
            self._h, ptr, words, int(col), ORDER_DESC if desc else 0, lo, hi, limit,
            keys.data_ptr(), rows.data_ptr(), n.data_ptr(), _stream_ptr(self.device)))
        written, eligible = n.tolist()
        return keys[:written], rows[:written], int(eligible)

    def facet_counts(self, field: int, n_codes: int, programs=None) -> torch.Tensor:
        """Rows per code of tag field `field` (0 or 1; rag_index_facet_counts): an int64 cuda
        tensor [n_codes + 1], entry c the rows below the count that pass the ONE program of
        `programs` (None = every row) and whose code is c; codes above n_codes are not counted.
        Enqueued on the current stream."""
        n_codes = int(n_codes)
        if not 0 <= n_codes <= 0xFFFF:
            raise ValueError("facet_counts: n_codes must lie in [0, 65535]")
        p, ptr, words = self._program(programs)
        out = torch.empty((n_codes + 1,), dtype=torch.int64, device=self.device)
        check(self._L.rag_index_facet_counts(self._h, ptr, words, int(field), n_codes,
                                             out.data_ptr(), _stream_ptr(self.device)))
        return out

    def move_rows(self, src, dst, new_count: int) -> None:
        """Copy every stored form of row src[i] into slot dst[i], bit for bit, then set the
        count (rag_index_move_rows). The src and dst sets must be disjoint."""
        s = _as_dev(src, torch.int64, self.device).reshape(-1)
        d = _as_dev(dst, torch.int64, self.device).reshape(-1)
        if s.shape != d.shape:
            raise ValueError("src and dst must pair up")
        check(self._L.rag_index_move_rows(self._h, s.data_ptr() if s.numel() else None,
                                          d.data_ptr() if s.numel() else None, s.numel(),
                                          int(new_count), _stream_ptr(self.device)))

    def gather_rows(self, rows):
        """The stored forms of `rows` (any slots below capacity) packed row-major on the
        device: (fp16 bits int16 [n, dim], fp32 [n, dim] or None on fp16 storage, tags int32
        [n]) — rag_index_gather_rows, the staging form scatter_rows takes."""
        r = _as_dev(rows, torch.int64, self.device).reshape(-1)
        n = r.numel()
        f16 = torch.empty((n, self.dim), dtype=torch.int16, device=self.device)
        f32 = (torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
               if self.storage == "fp32" else None)
        tags = torch.empty((n,), dtype=torch.int32, device=self.device)
        if n:
            check(self._L.rag_index_gather_rows(self._h, r.data_ptr(), n, f16.data_ptr(),
                                                f32.data_ptr() if f32 is not None else None,
                                                tags.data_ptr(), _stream_ptr(self.device)))
        return f16, f32, tags

    def scatter_rows(self, rows, f16, f32, tags, new_count: int) -> None:
        """Write packed rows (gather_rows' form, tensors on this device) to the distinct
        slots `rows`, bit for bit, then set the count (rag_index_scatter_rows)."""
        r = _as_dev(rows, torch.int64, self.device).reshape(-1)
        n = r.numel()
        f16 = _as_dev(f16, torch.int16, self.device)
        tags = _as_dev(tags, torch.int32, self.device)
        if (f32 is not None) != (self.storage == "fp32"):
            raise ValueError("fp32 rows go with fp32 storage, and only with it")
        if f32 is not None:
            f32 = _as_dev(f32, torch.float32, self.device)
            if tuple(f32.shape) != (n, self.dim):
                raise ValueError(f"f32 must be [n, {self.dim}]")
        if tuple(f16.shape) != (n, self.dim) or tuple(tags.shape) != (n,):
            raise ValueError(f"f16 must be [n, {self.dim}] and tags [n]")
        check(self._L.rag_index_scatter_rows(
            self._h, r.data_ptr() if n else None, n, f16.data_ptr() if n else None,
            f32.data_ptr() if n and f32 is not None else None, tags.data_ptr() if n else None,
            int(new_count), _stream_ptr(self.device)))

    def remove_rows(self, rows):
        """Delete `rows` (host integers in [0, count), duplicates allowed): plan_removal, then
        one move_rows. Returns the plan (src, dst, new_count) for the caller's own per-row
        state. Enqueued on the current stream."""
        src, dst, n1 = plan_removal(self.count, rows)
        self.move_rows(src, dst, n1)
        return src, dst, n1

    # ---------------------------------------------------------------- introspection
    def _export(self, fn, ptr, row0: int, n, tail: tuple, dtype) -> np.ndarray:
        if n is None:
            n = self.count - row0
        out = np.empty((n,) + tail, dtype=dtype)
        torch.cuda.current_stream(self.device).synchronize()
        check(fn(self._h, int(row0), int(n), out.ctypes.data_as(ptr)))
        return out

    def export_rows(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        """Stored fp16 rows (uint16 bits) [n, dim], row-major."""
        return self._export(self._L.rag_index_export_rows, _lib.c_u16p, row0, n, (self.dim,),
                            np.uint16)

    def export_rows32(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        """fp32 storage: the stored normalised fp32 rows [n, dim]."""
        return self._export(self._L.rag_index_export_rows32, _lib.c_f32p, row0, n, (self.dim,),
                            np.float32)

    def export_tags(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        return self._export(self._L.rag_index_export_tags, _lib.c_u32p, row0, n, (), np.uint32)

    def _import(self, fn, ptr, a: np.ndarray, row0: int, tags, new_count) -> None:
        n = a.shape[0]
        t = None
        if tags is not None:
            t = np.ascontiguousarray(tags, dtype=np.uint32)
            if t.shape != (n,):
                raise ValueError("tags must be [n]")
        if new_count is None:
            new_count = max(self.count, row0 + n)
        torch.cuda.current_stream(self.device).synchronize()
        check(fn(self._h, int(row0), int(n), a.ctypes.data_as(ptr),
                 t.ctypes.data_as(_lib.c_u32p) if t is not None else None, int(new_count)))

    def import_rows(self, rows_f16, row0: int = 0, tags=None,
                    new_count: int | None = None) -> None:
        """Write already-stored fp16 rows [n, dim] (float16 or uint16 bits, host) back into
        rows [row0, row0+n) unchanged — the load side of persistence (no renormalisation)."""
        a = np.ascontiguousarray(rows_f16)
        if a.dtype == np.float16:
            a = a.view(np.uint16)
        if a.dtype != np.uint16 or a.ndim != 2 or a.shape[1] != self.dim:
            raise ValueError(f"rows must be float16/uint16 [n, {self.dim}]")
        self._import(self._L.rag_index_import_rows, _lib.c_u16p, a, row0, tags, new_count)

    def import_rows32(self, rows_f32, row0: int = 0, tags=None,
                      new_count: int | None = None) -> None:
        """fp32 storage: write saved fp32 rows [n, dim] back unchanged (their fp16 scan copy
        is re-derived by the same rounding as upsert)."""
        a = np.ascontiguousarray(rows_f32, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.dim:
            raise ValueError(f"rows must be float32 [n, {self.dim}]")
        self._import(self._L.rag_index_import_rows32, _lib.c_f32p, a, row0, tags, new_count)

    def set_scan_order(self, serial: bool) -> None:
        """serial=True: each pass's scan waits for the previous pass's scan on any stream
        (rag_index_set_scan_order); prep / seeding / select still overlap across streams."""
        mode = serial if isinstance(serial, int) and not isinstance(serial, bool) else int(bool(serial))
        check(self._L.rag_index_set_scan_order(self._h, mode))

    def set_prescan(self, mode: int) -> None:
        """0 off / 1 auto (default) / 2 always / 3 always 6-bit: whether k <= 32 passes stream
        the int8 (or 6-bit) copy of the rows (dim 384, fp16 storage) and certify the exact top-k
        from the fp16 rows; results are the same in every mode. Mode 3 builds the 6-bit copy of
        an index that has none (rag_index_set_prescan)."""
        check(self._L.rag_index_set_prescan(self._h, int(mode)))

    def prescan(self) -> int:
        """The prescan mode set (rag_index_prescan)."""
        return int(self._L.rag_index_prescan(self._h))

    def prescan_passes(self) -> int:
        """Search passes since creation that streamed a prescan copy, int8 or 6-bit
        (rag_index_prescan_passes): ceil(B / 32) per k <= 32 search the prescan took, nothing
        for any other. Host state; no synchronisation."""
        n = ctypes.c_int64()
        check(self._L.rag_index_prescan_passes(self._h, ctypes.byref(n)))
        return int(n.value)

    def prescan6_passes(self) -> int:
        """Those of prescan_passes() that streamed the 6-bit copy (rag_index_prescan6_passes)."""
        n = ctypes.c_int64()
        check(self._L.rag_index_prescan6_passes(self._h, ctypes.byref(n)))
        return int(n.value)

    def prescan_bounds(self, queries, rows) -> torch.Tensor:
        """[B, n] upper bounds u of the prescan for stored rows `rows` against `queries`
        (B <= 32), from the stored copy the current mode streams (rag_index_prescan_bounds;
        diagnostic)."""
        q = _as_dev(queries, torch.float32, self.device)
        r = _as_dev(rows, torch.int64, self.device)
        out = torch.empty((q.shape[0], r.shape[0]), dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self._L.rag_index_prescan_bounds(self._h, q.data_ptr(), int(q.shape[0]),
                                               r.data_ptr(), int(r.shape[0]), out.data_ptr()))
        return out

    def exactness_stats(self, n_last: int = 0):
        """(tier1 total, tier2 total, tiers of the last pass's first n_last queries): which
        path certified each top-k (0 error-bound check, 1 list re-scoring, 2 second pass);
        rag_index_exactness_stats. The totals count every query since creation; the per-query
        tiers cover only the most recent PASS (<= 32 queries, <= 128 on the D = 1024 wide
        scan) of this handle on any stream — not the whole last search when it had more
        queries, and not a search of this thread when other threads search concurrently.
        Synchronises the device."""
        t1 = ctypes.c_int64()
        t2 = ctypes.c_int64()
        last = np.empty((max(n_last, 0),), dtype=np.int32)
        check(self._L.rag_index_exactness_stats(
            self._h, ctypes.byref(t1), ctypes.byref(t2),
            last.ctypes.data_as(_lib.c_i32p) if n_last > 0 else None, int(n_last)))
        return int(t1.value), int(t2.value), last

    def unanswered(self) -> int:
        """Queries since creation that got NO result (their tier reads 3, their ids -1):
        k <= 32 passes whose second pass was skipped (RAGMI_RESCAN_WG=0, diagnostic handles
        only), and 32 < k <= 4096 passes where more than 16384 rows tie within the MFMA error
        band of a query's k-th best score after the last collection round (possible in
        production, e.g. thousands of identical boilerplate chunks). search(rescue=True) re-runs
        such queries on the full exact pass (search(full=True)). rag_index_unanswered;
        synchronises the device."""
        n = ctypes.c_int64()
        check(self._L.rag_index_unanswered(self._h, ctypes.byref(n)))
        return int(n.value)

    # ---------------------------------------------------------------- profiling
    def profile(self, every: int | bool) -> None:
        """Time every `every`-th scan launch with HIP events (0/False: off, True: every one)."""
        check(self._L.rag_profile_enable(self._h, int(every)))

    def bench_scan(self, queries: torch.Tensor, variant: int, reps: int = 10) -> float:
        """Diagnostic: avg device ms per launch of scan variant `variant` (rag_bench_scan)."""
        q = _as_dev(queries, torch.float32, self.device)
        ms = ctypes.c_double()
        torch.cuda.synchronize(self.device)
        check(self._L.rag_bench_scan(self._h, q.data_ptr(), q.shape[0], int(variant),
                                     int(reps), ctypes.byref(ms)))
        return float(ms.value)

    def profile_scan_ms(self) -> tuple[float, int]:
        tot = ctypes.c_double()
        n = ctypes.c_int64()
        check(self._L.rag_profile_scan_ms(self._h, ctypes.byref(tot), ctypes.byref(n)))
        return float(tot.value), int(n.value)

    def profile_scan_intervals(self, cap: int = 1 << 16) -> tuple[np.ndarray, np.ndarray]:
        """(start_ms, end_ms) of every recorded scan launch, relative to the first one's start
        (rag_profile_scan_intervals); clears the record."""
        a = np.zeros(cap, np.float64)
        b = np.zeros(cap, np.float64)
        n = ctypes.c_int64()
        dp = ctypes.POINTER(ctypes.c_double)
        check(self._L.rag_profile_scan_intervals(self._h, a.ctypes.data_as(dp),
                                                 b.ctypes.data_as(dp), cap, ctypes.byref(n)))
        m = min(int(n.value), cap)
        return a[:m], b[:m]


class PartitionStreams:
    """`parts` HIP streams on disjoint shares of the device's CUs
    (rag_stream_create_cu_partition) as torch streams, for `parts` batches in flight: a search
    issued on one sizes its scan to that share, so the batches scan side by side instead of
    interleaving over every CU. Results are the same on any stream. close() (or the end of
    the process) destroys them; call it only after their work has finished."""

    def __init__(self, device, parts: int, whole: bool = False):
        """whole=True: `parts` streams that each may use EVERY CU (a full CU mask): still one
        dedicated hardware queue per stream (a CU-masked queue is never shared), so batches in
        flight cannot land on one queue whatever streams the process created before (the
        serving-shape fix of DESIGN §R6.4)."""
        dev = _lib.resolve_device(device)
        self.device = torch.device("cuda", _lib.device_index(dev))
        self._L = _lib.load()
        self._raw, self.streams = [], []
        for p in range(parts):
            h = ctypes.c_void_p()
            check(self._L.rag_stream_create_cu_partition(self.device.index,
                                                         0 if whole else p, 1 if whole else parts,
                                                         ctypes.byref(h)))
            self._raw.append(h)
            self.streams.append(torch.cuda.ExternalStream(h.value, device=self.device))

    def __len__(self):
        return len(self.streams)

    def __getitem__(self, i):
        return self.streams[i]

    def close(self) -> None:
        if self._raw:
            torch.cuda.synchronize(self.device)
            for h in self._raw:
                self._L.rag_stream_destroy(h)
            self._raw, self.streams = [], []


def busy_union_ms(start_ms, end_ms) -> float:
    """Length of the union of [start, end) intervals: the time at least one of the launches
    was running (overlapping launches counted once)."""
    order = np.argsort(start_ms, kind="stable")
    busy, cur_a, cur_b = 0.0, None, None
    for i in order:
        a, b = float(start_ms[i]), float(end_ms[i])
        if cur_b is None or a > cur_b:
            if cur_b is not None:
                busy += cur_b - cur_a
            cur_a, cur_b = a, b
        else:
            cur_b = max(cur_b, b)
    if cur_b is not None:
        busy += cur_b - cur_a
    return busy


class GroupSelection(NamedTuple):
    """rag_group_select's outputs (cuda tensors): keys int32 [B, G] holding the uint32 key bits
    in opening order (0 past the last group), fill int32 [B, G], scores fp32 [B, G, S] (-inf
    padding), rows int64 [B, G, S] (-1 padding), count int32 [B, 2] = (groups, n_b), and pos
    int32 [B, G, S] (each hit's position in its list) or None."""
    keys: torch.Tensor
    fill: torch.Tensor
    scores: torch.Tensor
    rows: torch.Tensor
    count: torch.Tensor
    pos: torch.Tensor | None


def group_select_tags(cand_scores: torch.Tensor, cand_rows: torch.Tensor,
                      cand_tags: torch.Tensor, key_mask: int, G: int, S: int, ncand=None,
                      with_pos: bool = False) -> GroupSelection:
    """rag_group_select over candidate lists on one device (fp32 / int64 / int32 tag bits, all
    [B, C]): per query the first G groups of candidates sharing the key tag & key_mask (key 0:
    no group), each with its first S hits, in list order — include/ragmi.h. `ncand`: None, a
    scalar or one value per query. Index-free; enqueued on the current stream."""
    dev = cand_scores.device
    s = cand_scores.contiguous()
    r = cand_rows.contiguous()
    t = cand_tags.contiguous()
    if s.dim() != 2 or s.shape != r.shape or s.shape != t.shape:
        raise ValueError("cand_scores, cand_rows and cand_tags must all be [B, C]")
    if s.dtype != torch.float32 or r.dtype != torch.int64 or t.dtype != torch.int32:
        raise ValueError("candidates must be fp32 scores, int64 rows and int32 tag bits")
    B, C = s.shape
    G, S, key_mask = int(G), int(S), int(key_mask) & 0xFFFFFFFF
    if not 1 <= C <= GROUPS_MAX_CANDIDATES:
        raise ValueError(f"C must be in [1, {GROUPS_MAX_CANDIDATES}] candidates")
    if not 1 <= G <= GROUPS_MAX or S < 1 or G * S > GROUPS_MAX_CELLS:
        raise ValueError(f"G must be in [1, {GROUPS_MAX}], S >= 1 and G * S <= {GROUPS_MAX_CELLS}")
    if key_mask == 0:
        raise ValueError("key_mask must name the tag bits of the group_by field")
    n = None
    if ncand is not None:
        n = torch.from_numpy(per_query(ncand, B, np.int32, "ncand")).to(dev)
    keys = torch.empty((B, G), dtype=torch.int32, device=dev)
    fill = torch.empty((B, G), dtype=torch.int32, device=dev)
    out_s = torch.empty((B, G, S), dtype=torch.float32, device=dev)
    out_r = torch.empty((B, G, S), dtype=torch.int64, device=dev)
    pos = torch.empty((B, G, S), dtype=torch.int32, device=dev) if with_pos else None
    count = torch.empty((B, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):      # index-free: the launch goes to the current device
        check(_lib.load().rag_group_select(
            s.data_ptr(), r.data_ptr(), t.data_ptr(), n.data_ptr() if n is not None else None,
            B, C, key_mask, G, S, keys.data_ptr(), fill.data_ptr(), out_s.data_ptr(),
            out_r.data_ptr(), pos.data_ptr() if pos is not None else None, count.data_ptr(),
            _stream_ptr(dev)))
    return GroupSelection(keys, fill, out_s, out_r, count, pos)


def fuse_rrf(cand_rows: torch.Tensor, k: int, rrf_k: int = 2, ncand=None,
             with_count: bool = False):
    """rag_fuse_rrf over candidate lists on one device (int64 [B, L, C], -1 = none): per request
    the distinct rows of its L lists ordered by (fused reciprocal-rank score desc, row asc), the
    first k of them — include/ragmi.h. `ncand`: None, or int32 values [B, L] (a host array or a
    tensor on the lists' device). Returns (scores fp32 [B, k], rows int64 [B, k]) with -inf / -1
    padding, and the distinct-row counts int32 [B] when `with_count`. Index-free; enqueued on
    the current stream."""
    if not isinstance(cand_rows, torch.Tensor) or cand_rows.dim() != 3:
        raise ValueError("cand_rows must be a [B, L, C] tensor")
    if cand_rows.dtype != torch.int64:
        raise ValueError("cand_rows must be int64 rows")
    dev = cand_rows.device
    r = cand_rows.contiguous()
    B, L, C = r.shape
    k, rrf_k = int(k), int(rrf_k)
    if not 1 <= L <= FUSION_MAX_LISTS:
        raise ValueError(f"L must be in [1, {FUSION_MAX_LISTS}] lists")
    if C < 1 or L * C > FUSION_MAX_ENTRIES:
        raise ValueError(f"C must be >= 1 and L * C <= {FUSION_MAX_ENTRIES} entries")
    if k < 1 or rrf_k < 1:
        raise ValueError("k and rrf_k must be >= 1")
    n = None
    if ncand is not None:
        if isinstance(ncand, torch.Tensor):
            n = ncand.to(device=dev, dtype=torch.int32).contiguous()
        else:
            n = torch.from_numpy(np.ascontiguousarray(np.asarray(ncand, dtype=np.int32))).to(dev)
        if n.shape != (B, L):
            raise ValueError("ncand must be [B, L]")
    out_s = torch.empty((B, k), dtype=torch.float32, device=dev)
    out_r = torch.empty((B, k), dtype=torch.int64, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev) if with_count else None
    with torch.cuda.device(dev):      # index-free: the launch goes to the current device
        check(_lib.load().rag_fuse_rrf(
            r.data_ptr(), n.data_ptr() if n is not None else None, B, L, C, k, rrf_k,
            out_s.data_ptr(), out_r.data_ptr(),
            count.data_ptr() if count is not None else None, _stream_ptr(dev)))
    return (out_s, out_r, count) if with_count else (out_s, out_r)


def formula_rescore(cand_scores: torch.Tensor, cand_rows: torch.Tensor, program, k: int,
                    ncand=None, cand_tags=None, cand_keys=None, with_count: bool = False):
    """rag_formula_rescore over candidate lists on one device (fp32 scores and int64 rows
    [B, L, C], -1 = none): per request the distinct rows of its L lists re-scored by the formula
    program `program` (ragmi.formula's blob: a uint32 host array, or an int32 tensor on the
    lists' device) and ordered by (value desc, row asc), the first k of them — include/ragmi.h.
    `ncand`: None, or int32 values [B, L]. `cand_tags`: the rows' int32 tag bits [B, L, C]
    (gather_tags), needed when the program has a condition. `cand_keys`: a mapping or sequence
    of key column -> int64 keys [B, L, C] (gather_keys), None entries = not supplied. Returns
    (scores fp32 [B, k], rows int64 [B, k], status int32 [B]: bit 0 a missing variable, bit 1 a
    non-finite value, bit 2 a bad program) with -inf / -1 padding, and the distinct-row counts
    int32 [B] when `with_count`. Index-free; enqueued on the current stream."""
    if not isinstance(cand_rows, torch.Tensor) or cand_rows.dim() != 3:
        raise ValueError("cand_rows must be a [B, L, C] tensor")
    if not isinstance(cand_scores, torch.Tensor) or cand_scores.shape != cand_rows.shape:
        raise ValueError("cand_scores and cand_rows must both be [B, L, C] tensors")
    if cand_rows.dtype != torch.int64 or cand_scores.dtype != torch.float32:
        raise ValueError("candidates must be fp32 scores and int64 rows")
    dev = cand_rows.device
    r = cand_rows.contiguous()
    s = cand_scores.to(dev).contiguous()
    B, L, C = r.shape
    k = int(k)
    if not 1 <= L <= FUSION_MAX_LISTS:
        raise ValueError(f"L must be in [1, {FUSION_MAX_LISTS}] lists")
    if C < 1 or L * C > FUSION_MAX_ENTRIES:
        raise ValueError(f"C must be >= 1 and L * C <= {FUSION_MAX_ENTRIES} entries")
    if k < 1:
        raise ValueError("k must be >= 1")
    if isinstance(program, torch.Tensor):
        prog = program.to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
    else:
        a = np.ascontiguousarray(np.asarray(program, dtype=np.uint32).reshape(-1))
        prog = torch.from_numpy(a.view(np.int32)).to(dev)
    if prog.numel() < 2:
        raise ValueError("a formula blob holds at least its two header words")
    n = None
    if ncand is not None:
        if isinstance(ncand, torch.Tensor):
            n = ncand.to(device=dev, dtype=torch.int32).contiguous()
        else:
            n = torch.from_numpy(np.ascontiguousarray(np.asarray(ncand, dtype=np.int32))).to(dev)
        if n.shape != (B, L):
            raise ValueError("ncand must be [B, L]")
    t = None
    if cand_tags is not None:
        t = cand_tags.to(dev).contiguous()
        if t.shape != r.shape or t.dtype != torch.int32:
            raise ValueError("cand_tags must be int32 tag bits [B, L, C]")
    cols = [None] * KEYS_MAX_COLS
    for c, x in (cand_keys.items() if hasattr(cand_keys, "items") else
                 enumerate(cand_keys or ())):
        if x is None:
            continue
        if not 0 <= int(c) < KEYS_MAX_COLS:
            raise ValueError(f"key columns are 0..{KEYS_MAX_COLS - 1}")
        x = x.to(dev).contiguous()
        if x.shape != r.shape or x.dtype != torch.int64:
            raise ValueError("cand_keys must be int64 keys [B, L, C]")
        cols[int(c)] = x
    ptrs = (ctypes.c_void_p * KEYS_MAX_COLS)(*[x.data_ptr() if x is not None and x.numel()
                                               else None for x in cols])
    out_s = torch.empty((B, k), dtype=torch.float32, device=dev)
    out_r = torch.empty((B, k), dtype=torch.int64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev) if with_count else None
    with torch.cuda.device(dev):      # index-free: the launch goes to the current device
        check(_lib.load().rag_formula_rescore(
            s.data_ptr(), r.data_ptr(), t.data_ptr() if t is not None else None, ptrs,
            n.data_ptr() if n is not None else None, prog.data_ptr(), prog.numel(), B, L, C, k,
            out_s.data_ptr(), out_r.data_ptr(),
            count.data_ptr() if count is not None else None, status.data_ptr(),
            _stream_ptr(dev)))
    return (out_s, out_r, status, count) if with_count else (out_s, out_r, status)


def merge_topk(scores: torch.Tensor, ids: torch.Tensor, k: int):
    """Merge per-shard exact lists [n_lists, B, k] -> global [B, k] on the GPU."""
    L = _lib.load()
    n_lists, B, kk = scores.shape
    if kk != k:
        raise ValueError("list length must equal k")
    scores = scores.contiguous()
    ids = ids.contiguous()
    out_s = torch.empty((B, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=scores.device)
    check(L.rag_merge_topk(scores.data_ptr(), ids.data_ptr(), n_lists, B, k, out_s.data_ptr(),
                           out_i.data_ptr(), _stream_ptr(scores.device)))
    return out_s, out_i


def merge_topk_packed(packed: torch.Tensor, k: int):
    """Merge all-gathered packed lists int32 [n_lists, B, k, 2] -> (scores [B,k], ids [B,k])."""
    L = _lib.load()
    n_lists, B, kk, two = packed.shape
    if kk != k or two != 2 or packed.dtype != torch.int32:
        raise ValueError("packed lists must be int32 [n_lists, B, k, 2]")
    packed = packed.contiguous()
    out_s = torch.empty((B, k), dtype=torch.float32, device=packed.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=packed.device)
    check(L.rag_merge_topk_packed(packed.data_ptr(), n_lists, B, k, out_s.data_ptr(),
                                  out_i.data_ptr(), _stream_ptr(packed.device)))
    return out_s, out_i
