"""ShardSet — N FlatIndex shards on one or several GPUs, searched as one index from ONE process.

The reference service is one process whose every request reaches the index through
`get_qdrant().query_points(...)` (main.py:92-95, 232-237). `ragmi.dist.ShardedIndex` shards
over one process per GPU under torch.distributed; a ShardSet shards inside the process, so
`QdrantClient(devices=[0, 1, ...])` serves one collection from several GPUs behind the same
calls (rag_shardset_search, include/ragmi.h).

Row placement is striped: global row g lives on shard g % N at local row g // N. A Qdrant
collection grows by `upsert` with no total known in advance (ingest.py:171-175); contiguous
ranges would fill GPU 0 first, stripes fill every shard evenly at every size. Within a shard
local order is global order, so each shard's exact top-k by (score desc, local row asc) is
its exact top-k by (score desc, global row asc) and the merged list equals the unsharded one
bit for bit. Everything here works in global rows: a ShardSet offers what `collection.Collection`
and `ragmi.store` use of a FlatIndex.
"""
from __future__ import annotations

import ctypes
import functools
import threading

import numpy as np
import torch

from . import _lib
from ._lib import check
from .filters import KEY_ABSENT
from .index import FlatIndex, ListOps, _as_dev, host_or_tensor, plan_removal, view_blob

MAX_SHARDS = 64      # RAG_MAX_SHARDS in include/ragmi.h
SHARDSET_FULL = 1    # RAG_SHARDSET_FULL


# ------------------------------------------------------------------ placement (pure, host)
def shard_of(row, n: int):
    """Shard holding global row `row` (int or integer array)."""
    return row % n


def local_of(row, n: int):
    """Row slot of global row `row` on its shard."""
    return row // n


def global_of(local, shard, n: int):
    """Global row of local row `local` on shard `shard`."""
    return local * n + shard


def shard_count(count: int, shard: int, n: int) -> int:
    """Rows of shard `shard` when the set holds global rows [0, count)."""
    return max(0, -((shard - count) // n))


def shard_moves(src, dst, n: int) -> dict:
    """A removal plan in global rows (plan_removal's src -> dst pairs) split by shards:
    {(source shard, destination shard): (local source rows, local destination rows)}, pairs in
    plan order, only the shard pairs that occur."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    ss, ds = shard_of(src, n), shard_of(dst, n)
    out = {}
    for s, d in sorted(set(zip(ss.tolist(), ds.tolist()))):
        sel = (ss == s) & (ds == d)
        out[(s, d)] = (local_of(src[sel], n), local_of(dst[sel], n))
    return out


def parse_devices(spec, device_count: int | None = None) -> list[int] | None:
    """The `devices` argument of QdrantClient / the RAGMI_DEVICES variable -> device indices.
    None or "" -> None (one FlatIndex on one device, no shard set); "all" -> every visible
    device; "0,1,2,3", or a sequence of ints -> that list. An index may repeat: logical shards
    sharing one GPU (one-GPU rehearsal, tests). `device_count` (default: what torch sees)
    resolves "all" and bounds the indices when given."""
    if spec is None:
        return None
    if isinstance(spec, str):
        text = spec.strip()
        if not text:
            return None
        if text.lower() == "all":
            n = torch.cuda.device_count() if device_count is None else int(device_count)
            if n < 1:
                raise ValueError("devices='all': no HIP device visible")
            return list(range(n))
        try:
            devs = [int(p) for p in text.split(",")]
        except ValueError:
            raise ValueError(f"devices {spec!r}: expected 'all' or indices like '0,1,2,3'") from None
    else:
        devs = []
        for d in spec:
            if isinstance(d, bool) or not isinstance(d, (int, np.integer)):
                raise ValueError(f"devices {spec!r}: device indices must be ints")
            devs.append(int(d))
    if not 1 <= len(devs) <= MAX_SHARDS:
        raise ValueError(f"devices {spec!r}: 1 to {MAX_SHARDS} shards")
    for d in devs:
        if d < 0 or (device_count is not None and d >= device_count):
            raise ValueError(f"devices {spec!r}: no device {d}")
    return devs


def gather_merge_np(lists, k: int, id_mul: int, id_add):
    """numpy restatement of rag_merge_topk_gather: `lists` = packed int32 [B, k, 2] arrays
    (score bits, local row; -1 = none). Returns (scores [B, k], ids [B, k], empty [n, B])."""
    n, B = len(lists), lists[0].shape[0]
    out_s = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int64)
    empty = np.zeros((n, B), np.uint8)
    for b in range(B):
        sc, ids = [], []
        for l, lst in enumerate(lists):
            row = np.ascontiguousarray(lst[b])
            ok = row[:, 1] >= 0
            empty[l, b] = 0 if row[0, 1] >= 0 else 1
            sc.append(np.ascontiguousarray(row[:, 0]).view(np.float32)[ok])
            ids.append(row[ok, 1].astype(np.int64) * id_mul + int(id_add[l]))
        sc, ids = np.concatenate(sc), np.concatenate(ids)
        order = np.lexsort((ids, -sc.astype(np.float64)))[:k]     # score desc, then id asc
        out_s[b, :len(order)] = sc[order]
        out_i[b, :len(order)] = ids[order]
    return out_s, out_i, empty


def merge_topk_gather(lists, k: int, id_mul: int, id_add):
    """rag_merge_topk_gather over separate packed lists (cuda int32 [B, k, 2] tensors on one
    device). Returns (scores [B, k], ids [B, k], empty uint8 [n_lists, B]) on the current
    stream."""
    L = _lib.load()
    n = len(lists)
    B = lists[0].shape[0]
    dev = lists[0].device
    for t in lists:
        if t.dtype != torch.int32 or tuple(t.shape) != (B, k, 2) or not t.is_contiguous():
            raise ValueError("lists must be contiguous int32 [B, k, 2]")
    ptrs = (_lib.c_vp * n)(*[t.data_ptr() for t in lists])
    add = (ctypes.c_int64 * n)(*[int(a) for a in id_add])
    out_s = torch.empty((B, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((B, k), dtype=torch.int64, device=dev)
    empty = torch.empty((n, B), dtype=torch.uint8, device=dev)
    check(L.rag_merge_topk_gather(ptrs, n, B, int(k), int(id_mul), add, out_s.data_ptr(),
                                  out_i.data_ptr(), empty.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream))
    return out_s, out_i, empty


# ------------------------------------------------------------------ the set
def _keeps_device(fn):
    """The rag_index_* calls behind a FlatIndex leave the thread's current HIP device on that
    index's device; a method that walks shards on several devices puts the caller's back."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        prev = torch.cuda.current_device() if torch.cuda.is_available() else None
        try:
            return fn(*args, **kwargs)
        finally:
            if prev is not None:
                torch.cuda.set_device(prev)
    return wrapped


class ShardSet(ListOps):
    """N FlatIndex shards + the C shard-set handle, addressed in global rows. `devices`: one
    device index per shard (see parse_devices); `device`, the merge device, is the first."""

    @_keeps_device
    def __init__(self, dim: int = 384, devices=(0,), capacity: int = 0, storage: str = "fp16"):
        devs = parse_devices(devices)
        if devs is None:
            raise ValueError("ShardSet needs a list of devices")
        _lib.require_gpu()
        self._L = _lib.load()
        self.n = len(devs)
        self.dim = int(dim)
        self.storage = storage
        self.shards: list = []
        self._h = None
        self._scratch = None              # mmr's scratch index on the merge device
        self._scratch_lock = threading.Lock()
        self._scratch_done = None         # event behind the last launch that read the scratch
        per = -(-int(capacity) // self.n)
        try:
            for d in devs:
                self.shards.append(FlatIndex(dim, per, torch.device("cuda", d), storage))
            arr = (_lib.c_vp * self.n)(*[s._h.value for s in self.shards])
            h = ctypes.c_void_p()
            check(self._L.rag_shardset_create(arr, self.n, ctypes.byref(h)))
            self._h = h
        except BaseException:
            self.close()
            raise
        self.device = self.shards[0].device
        self._count = 0
        self._unanswered = [0] * self.n   # each shard's unanswered() as last read (rescue)
        self.rescued = 0                  # queries re-answered on the full exact pass

    # ---------------------------------------------------------------- lifetime
    @_keeps_device
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.rag_shardset_destroy(self._h)
        self._h = None
        for s in getattr(self, "shards", []):
            s.close()
        if getattr(self, "_scratch", None) is not None:
            self._scratch.close()
            self._scratch = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- properties
    @property
    def count(self) -> int:
        return self._count

    @property
    def capacity(self) -> int:
        return min(s.capacity for s in self.shards) * self.n

    @_keeps_device
    def reserve(self, capacity: int) -> None:
        per = -(-int(capacity) // self.n)
        for s in self.shards:
            if s.capacity < per:
                s.reserve(per)

    def _stripe(self, shard: int, row0: int, n: int):
        """Global rows [row0, row0 + n) that live on `shard`: (offset of the first one in the
        range, its local row, how many)."""
        first = (shard - row0) % self.n
        if first >= n:
            return first, 0, 0
        return first, (row0 + first) // self.n, -(-(n - first) // self.n)

    def _settle(self, shard) -> None:
        # a shard off the merge device is searched on a stream of its own, which nothing
        # orders behind the write just enqueued on that device's current stream
        if shard.device != self.device:
            torch.cuda.current_stream(shard.device).synchronize()

    # ---------------------------------------------------------------- writes
    @_keeps_device
    def upsert(self, vectors, rows, tags=None, new_count: int | None = None) -> None:
        """FlatIndex.upsert in global rows: each row goes to its shard."""
        r = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
        r = r.astype(np.int64).reshape(-1)
        v = host_or_tensor(vectors)
        if v.ndim != 2 or v.shape[1] != self.dim or v.shape[0] != r.shape[0]:
            raise ValueError(f"vectors must be [n, {self.dim}] with one row slot each")
        if r.size and (int(r.min()) < 0 or int(r.max()) >= self.capacity):
            raise IndexError("row slot outside capacity; reserve() first")
        t = None
        if tags is not None:
            t = (tags.detach().cpu().numpy().view(np.uint32) if isinstance(tags, torch.Tensor)
                 else np.asarray(tags, dtype=np.uint32))
        if new_count is None:
            new_count = max(self._count, int(r.max()) + 1 if r.size else 0)
        for s, shard in enumerate(self.shards):
            sel = np.nonzero(shard_of(r, self.n) == s)[0]
            cnt = shard_count(new_count, s, self.n)
            if sel.size:
                vs = v[torch.as_tensor(sel, device=v.device)] if isinstance(v, torch.Tensor) \
                    else v[sel]
                shard.upsert(vs, local_of(r[sel], self.n), t[sel] if t is not None else None,
                             new_count=cnt)
            elif shard.count != cnt:
                shard.set_count(cnt)
            self._settle(shard)
        self._count = int(new_count)

    # ---------------------------------------------------------------- sparse column
    def sparse_create(self, slots: int = 128) -> None:
        """Not built: a sparse search over several shards needs its own merge (the precedent:
        recommend). A collection with a sparse vector lives on one FlatIndex."""
        raise NotImplementedError("sparse vectors over a shard set are not built")

    # ---------------------------------------------------------------- key columns
    @_keeps_device
    def keys_create(self, n_cols: int) -> None:
        """FlatIndex.keys_create on every shard."""
        for shard in self.shards:
            shard.keys_create(n_cols)

    def keys_cols(self) -> int:
        return self.shards[0].keys_cols()

    @_keeps_device
    def write_keys(self, col: int, rows, keys) -> None:
        """FlatIndex.write_keys in global rows, striped like upsert: each key goes to the shard
        of its row."""
        r = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
        k = keys.detach().cpu().numpy() if isinstance(keys, torch.Tensor) else np.asarray(keys)
        r, k = r.astype(np.int64).reshape(-1), k.astype(np.int64).reshape(-1)
        if r.shape != k.shape:
            raise ValueError("rows and keys must pair up")
        for s, shard in enumerate(self.shards):
            sel = np.nonzero((r >= 0) & (shard_of(r, self.n) == s))[0]
            if sel.size:
                shard.write_keys(col, local_of(r[sel], self.n), k[sel])
                self._settle(shard)

    @_keeps_device
    def gather_keys(self, col: int, global_rows) -> torch.Tensor:
        """FlatIndex.gather_keys in global rows, as gather_tags: every shard gathers the keys of
        its own rows and the results are merged on the merge device; KEY_ABSENT for a row
        outside [0, capacity)."""
        g = _as_dev(global_rows, torch.int64, self.device)
        valid = (g >= 0) & (g < self.capacity)
        out = torch.full(g.shape, KEY_ABSENT, dtype=torch.int64, device=self.device)
        for sh, shard in enumerate(self.shards):
            own = valid & (shard_of(g, self.n) == sh)
            local = torch.where(own, local_of(g, self.n), -1)
            out = torch.where(own, shard.gather_keys(col, local.to(shard.device)).to(self.device),
                              out)
        return out

    # ---------------------------------------------------------------- row removal
    @_keeps_device
    def remove_rows(self, global_rows):
        """FlatIndex.remove_rows in global rows: the one plan (plan_removal), each (src, dst)
        pair mapped to (shard, local row) by shard_moves. Pairs inside a shard are one
        move_rows there; pairs between two shards are gathered on the source, the packed
        staging tensors copied to the destination's device (no kernel reads another GPU's
        memory) and scattered there. Local sources lie at or past their shard's new count and
        local destinations below it, so no pair waits for another. Returns the global plan
        (src, dst, new_count)."""
        src, dst, n1 = plan_removal(self._count, global_rows)
        for (s, d), (ls, ld) in shard_moves(src, dst, self.n).items():
            cnt = shard_count(n1, d, self.n)
            if s == d:
                self.shards[s].move_rows(ls, ld, cnt)
            else:
                f16, f32, tags = self.shards[s].gather_rows(ls)
                to = self.shards[d].device
                self.shards[d].scatter_rows(ld, f16.to(to), f32.to(to) if f32 is not None
                                            else None, tags.to(to), cnt)
                for c in range(self.keys_cols()):     # the keys travel with the staged rows
                    self.shards[d].write_keys(c, ld, self.shards[s].gather_keys(c, ls).to(to))
        for s, shard in enumerate(self.shards):
            cnt = shard_count(n1, s, self.n)
            if shard.count != cnt:
                shard.set_count(cnt)
            self._settle(shard)
        self._count = n1
        return src, dst, n1

    @_keeps_device
    def _select(self, cap, select):
        """`select(shard)`'s (local rows, total) of every shard mapped to global rows and merged
        ascending on the merge device: (rows int64 cuda tensor, total). The first `cap` global
        matches lie among each shard's first `cap`."""
        parts, total = [], 0
        for s, shard in enumerate(self.shards):
            rows, n = select(shard)
            total += n
            if rows.numel():
                parts.append((rows * self.n + s).to(self.device))
        if not parts:
            return torch.empty((0,), dtype=torch.int64, device=self.device), total
        merged = torch.sort(torch.cat(parts)).values
        return (merged if cap is None else merged[:int(cap)]), total

    def select_rows(self, tag_mask: int, tag_value: int, cap: int | None = None):
        """FlatIndex.select_rows over the set (_select)."""
        return self._select(cap, lambda shard: shard.select_rows(tag_mask, tag_value, cap))

    def select_rows_view(self, programs, cap: int | None = None):
        """FlatIndex.select_rows_view over the set (_select)."""
        return self._select(cap, lambda shard: shard.select_rows_view(programs, cap))

    # ---------------------------------------------------------------- payload queries
    def select_rows_from(self, row0: int, programs=None, cap: int | None = None):
        """FlatIndex.select_rows_from over the set: global row0 is, on shard s, its first local
        row at or after it, ceil((row0 - s) / n); then _select."""
        row0 = int(row0)
        if row0 < 0:
            raise ValueError("row0 must be >= 0")
        first = {id(shard): max(0, -((s - row0) // self.n)) for s, shard in enumerate(self.shards)}
        return self._select(cap, lambda shard: shard.select_rows_from(first[id(shard)], programs,
                                                                      cap))

    @_keeps_device
    def order_rows(self, col: int, limit: int, desc: bool = False, lo=None, hi=None,
                   programs=None):
        """FlatIndex.order_rows over the set, in global rows: every shard's own list (its local
        order is the global order of its rows) mapped to global rows, the lists merged on the
        merge device by (key, global row) and cut to `limit`; the eligible counts add up."""
        ks, rs, eligible = [], [], 0
        for s, shard in enumerate(self.shards):
            k, r, e = shard.order_rows(col, limit, desc, lo, hi, programs)
            eligible += e
            ks.append(k.to(self.device))
            rs.append((r * self.n + s).to(self.device))
        k, r = torch.cat(ks), torch.cat(rs)
        by_row = torch.sort(r).indices                  # then a stable sort by key: ties stay
        k, r = k[by_row], r[by_row]                     # in row order in both directions
        by_key = torch.sort(k, stable=True, descending=bool(desc)).indices[:int(limit)]
        return k[by_key], r[by_key], eligible

    @_keeps_device
    def facet_counts(self, field: int, n_codes: int, programs=None) -> torch.Tensor:
        """FlatIndex.facet_counts summed over the shards, on the merge device."""
        parts = [shard.facet_counts(field, n_codes, programs) for shard in self.shards]
        out = parts[0].to(self.device)
        for p in parts[1:]:
            out = out + p.to(self.device)
        return out

    # ---------------------------------------------------------------- search
    def _search_args(self, queries, k, filters):
        return self.shards[0]._search_args(queries, k, filters)     # on the merge device

    @_keeps_device
    def search(self, queries, k: int, filters=None, full: bool = False, rescue: bool = False,
               programs=None, n_programs: int | None = None):
        """Top-k of each query over all shards: (scores fp32 [B, k], ids int64 [B, k], global
        rows, -1 where fewer than k rows match) on the merge device's current stream —
        FlatIndex.search's result on the same rows, bit for bit. full=True: every shard
        answers by its full exact pass. rescue=True (Collection.search): read back which
        shards returned nothing per query; where such a shard's unanswered() rose, its
        large-k pass left the query unanswered and the merged top-k lacks that shard's rows,
        so those queries are re-run with full=True (counted once each in `rescued`).
        Synchronises when rescue is set. `programs`: as FlatIndex.search — every shard
        searches over the blob's filter view of its tags (rag_shardset_search_view), and the
        rescue re-runs with the same blob."""
        q, B, f = self._search_args(queries, k, filters)
        out_s = torch.empty((B, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((B, k), dtype=torch.int64, device=self.device)
        empty = torch.empty((self.n, B), dtype=torch.uint8, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        if programs is not None:
            programs, words, n_programs = view_blob(programs, n_programs, self.device)
            check(self._L.rag_shardset_search_view(
                self._h, q.data_ptr(), B, int(k), programs.data_ptr(), words, n_programs,
                f.data_ptr() if f is not None else None, SHARDSET_FULL if full else 0,
                out_s.data_ptr(), out_i.data_ptr(), empty.data_ptr(), st))
        else:
            check(self._L.rag_shardset_search(
                self._h, q.data_ptr(), B, int(k), f.data_ptr() if f is not None else None,
                SHARDSET_FULL if full else 0, out_s.data_ptr(), out_i.data_ptr(),
                empty.data_ptr(), st))
        if rescue and not full and B:
            e = empty.cpu().numpy().astype(bool)
            redo = np.zeros(B, bool)
            for s in np.nonzero(e.any(axis=1))[0]:
                n_un = self.shards[s].unanswered()
                if n_un > self._unanswered[s]:
                    redo |= e[s]
                self._unanswered[s] = n_un
            if redo.any():
                sel = torch.as_tensor(np.nonzero(redo)[0], device=self.device)
                s2, i2 = self.search(q[sel], k, f[sel] if f is not None else None, full=True,
                                     programs=programs, n_programs=n_programs)
                out_s[sel] = s2
                out_i[sel] = i2
                self.rescued += int(redo.sum())
        return out_s, out_i

    # ---------------------------------------------------------------- MMR
    def _mmr_scratch(self, slots: int):
        """The scratch FlatIndex on the merge device that mmr copies the candidates' rows into
        (same dim and storage as the shards), created on first use and grown on demand."""
        if self._scratch is None:
            self._scratch = FlatIndex(self.dim, slots, self.device, self.storage)
        elif self._scratch.capacity < slots:
            self._scratch.reserve(slots)
        return self._scratch

    @_keeps_device
    def mmr(self, cand_scores, cand_rows, k: int, diversity, ncand=None,
            with_pos: bool = False):
        """FlatIndex.mmr in global rows, composed of existing primitives: every shard gathers
        its own candidates' stored rows (gather_rows skips the -1 it is given for the others),
        the packed rows are copied to the merge device and scattered, bit for bit, into a
        scratch FlatIndex at slot b * C + j; rag_index_mmr runs there over the slots and its
        positions are mapped back to global rows. The rows travel unchanged, so the result is
        FlatIndex.mmr's on the same rows bit for bit. On the merge device's current stream."""
        s = _as_dev(cand_scores, torch.float32, self.device)
        g = _as_dev(cand_rows, torch.int64, self.device)
        if s.dim() != 2 or s.shape != g.shape:
            raise ValueError("cand_scores and cand_rows must both be [B, C]")
        B, C = g.shape
        flat = g.reshape(-1)
        valid = (flat >= 0) & (flat < self.capacity)
        slot = torch.arange(B * C, dtype=torch.int64, device=self.device)
        with self._scratch_lock:
            scratch = self._mmr_scratch(max(B * C, 1))
            stream = torch.cuda.current_stream(self.device)
            if self._scratch_done is not None:
                # the previous call's launch may still read the slots, on another stream
                stream.wait_event(self._scratch_done)
            for sh, shard in enumerate(self.shards):
                own = valid & (shard_of(flat, self.n) == sh)
                local = torch.where(own, local_of(flat, self.n), -1)
                f16, f32, tags = shard.gather_rows(local.to(shard.device))
                scratch.scatter_rows(torch.where(own, slot, -1), f16.to(self.device),
                                     f32.to(self.device) if f32 is not None else None,
                                     tags.to(self.device), B * C)
            out_s, _, pos = scratch.mmr(s, torch.where(valid, slot, -1).reshape(B, C), k,
                                        diversity, ncand, with_pos=True)
            self._scratch_done = stream.record_event()
        picked = torch.gather(g, 1, pos.clamp(min=0).to(torch.int64))
        rows = torch.where(pos >= 0, picked, -1)
        return (out_s, rows, pos) if with_pos else (out_s, rows)

    # ---------------------------------------------------------------- grouped search
    @_keeps_device
    def gather_tags(self, global_rows) -> torch.Tensor:
        """FlatIndex.gather_tags in global rows: every shard gathers the tags of its own rows
        (it is given -1 for the others, which the gather answers with 0), the per-shard results
        are copied to the merge device and combined. int32 tag bits, the shape of the rows,
        0 for a row outside [0, capacity)."""
        g = _as_dev(global_rows, torch.int64, self.device)
        valid = (g >= 0) & (g < self.capacity)
        out = torch.zeros(g.shape, dtype=torch.int32, device=self.device)
        for sh, shard in enumerate(self.shards):
            own = valid & (shard_of(g, self.n) == sh)
            local = torch.where(own, local_of(g, self.n), -1)
            out |= shard.gather_tags(local.to(shard.device)).to(self.device)
        return out

    @_keeps_device
    def unanswered(self) -> int:
        """Sum of the shards' FlatIndex.unanswered()."""
        return sum(s.unanswered() for s in self.shards)

    # ---------------------------------------------------------------- export / import
    @_keeps_device
    def _export(self, name: str, row0: int, n, shape_tail: tuple, dtype) -> np.ndarray:
        if n is None:
            n = self._count - row0
        out = np.empty((n,) + shape_tail, dtype=dtype)
        for s, shard in enumerate(self.shards):
            first, l0, m = self._stripe(s, row0, n)
            if m:
                out[first::self.n] = getattr(shard, name)(l0, m)
        return out

    def export_rows(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        """Stored fp16 rows (uint16 bits) [n, dim] of global rows [row0, row0 + n)."""
        return self._export("export_rows", row0, n, (self.dim,), np.uint16)

    def export_rows32(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        return self._export("export_rows32", row0, n, (self.dim,), np.float32)

    def export_tags(self, row0: int = 0, n: int | None = None) -> np.ndarray:
        return self._export("export_tags", row0, n, (), np.uint32)

    @_keeps_device
    def _import(self, name: str, a: np.ndarray, row0: int, tags, new_count) -> None:
        n = a.shape[0]
        t = None
        if tags is not None:
            t = np.ascontiguousarray(tags, dtype=np.uint32)
            if t.shape != (n,):
                raise ValueError("tags must be [n]")
        if new_count is None:
            new_count = max(self._count, row0 + n)
        for s, shard in enumerate(self.shards):
            first, l0, m = self._stripe(s, row0, n)
            cnt = shard_count(new_count, s, self.n)
            if m:
                getattr(shard, name)(np.ascontiguousarray(a[first::self.n]), l0,
                                     np.ascontiguousarray(t[first::self.n]) if t is not None
                                     else None, new_count=cnt)
            elif shard.count != cnt:
                shard.set_count(cnt)
                self._settle(shard)
        self._count = int(new_count)

    def import_rows(self, rows_f16, row0: int = 0, tags=None,
                    new_count: int | None = None) -> None:
        """FlatIndex.import_rows in global rows: the range is de-interleaved over the shards."""
        self._import("import_rows", np.asarray(rows_f16), row0, tags, new_count)

    def import_rows32(self, rows_f32, row0: int = 0, tags=None,
                      new_count: int | None = None) -> None:
        self._import("import_rows32", np.asarray(rows_f32), row0, tags, new_count)
