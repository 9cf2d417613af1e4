"""QdrantClient-shaped front end of the in-HBM flat index.

Drop-in for the calls the reference makes on `qdrant_client.QdrantClient`:
  get_collections()                       main.py:135, main2.py:337 (/ready)
  collection_exists(name)                 ingest.py:87, database.py:121
  create_collection(name, vectors_config) ingest.py:89-95, database.py:122-128
  upsert(name, points=[PointStruct])      ingest.py:171-175
  query_points(name, query, limit, query_filter) -> .points[i].{id,score,payload}
                                          main.py:232-237, main2.py:163
plus query_batch_points (one GPU scan for a whole micro-batch; main2.py:281-295 stage 2),
the prefetch routes of query_points (FusionQuery / RrfQuery, FormulaQuery), its OrderByQuery
and RecommendQuery routes, recommend (the legacy spelling of the latter), the DiscoverQuery /
ContextQuery route and its legacy spelling discover, scroll (in storage
order, or order_by a range field), facet, count (also filtered), retrieve, delete (by ids or by filter) and delete_collection.

`url` is accepted and ignored: the collection lives in this process's GPU memory (the
Qdrant service of docker-compose.yml:22 is replaced, not contacted). `path=` plays the role
of Qdrant's local mode / storage volume: existing collections under it are loaded at
construction and `save()` / `close()` write them back (ragmi.store shard format). Payloads stay host-side
keyed by row; the keyword payload fields used by the reference's `must` filter (`ticker`,
`document_type`, main.py:218-230) are dictionary-coded into a per-row uint32 tag in HBM
(16 bits per field) so filtering runs inside the scan kernel.

This module holds the client and the parsing of request arguments; the collection engine is
ragmi.collection, the coalescer ragmi.coalesce, the tag codebook and the filter compilers
ragmi.filters. Their public names are re-exported here.
"""
from __future__ import annotations

import os
import shutil
import threading
from typing import Iterable

import numpy as np

from . import qdrant_models as models
from .coalesce import Coalescer                                           # noqa: F401
from .collection import (Collection, SparsePrefetch, _norm_id, parse_selector,  # noqa: F401
                         stack_queries)
from .filters import (DEFAULT_TAG_FIELDS, PayloadTags, UnsupportedFilter,  # noqa: F401
                      compile_filter)
from .index import (CONTEXT_MAX_PAIRS, DISCOVER_MAX_PAIRS, FUSION_MAX_LISTS, MAX_K,
                    MMR_MAX_CANDIDATES, RECO_MAX_SIDE, SPARSE_SLOTS, reco_strategy)
from .shardset import parse_devices


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


def sparse_config(sparse_vectors_config, sparse_slots):
    """create_collection's sparse arguments -> Collection's `sparse` (name, idf, slots), None
    without a sparse vector. Exactly one sparse name is built (more: NotImplementedError), the
    name may not be "" (the dense vector), SparseIndexParams is accepted and ignored except for a
    datatype other than float32 (NotImplementedError)."""
    if not sparse_vectors_config:
        return None
    if not isinstance(sparse_vectors_config, dict):
        raise ValueError("sparse_vectors_config is a dict {name: SparseVectorParams(...)}")
    if len(sparse_vectors_config) > 1:
        raise NotImplementedError("one sparse vector per collection is built, got "
                                  f"{sorted(sparse_vectors_config)}")
    (name, par), = sparse_vectors_config.items()
    if not isinstance(name, str) or name == "":
        raise ValueError('a sparse vector needs a name other than "" (the dense vector)')
    par = par if par is not None else models.SparseVectorParams()
    dt = getattr(getattr(par, "index", None), "datatype", None)
    dt = getattr(dt, "value", dt)
    if dt is not None and str(dt).lower() != "float32":
        raise NotImplementedError(f"sparse vector datatype {dt!r} (float32 is stored)")
    mod = getattr(par, "modifier", None)
    mod = getattr(mod, "value", mod)
    if mod not in (None, models.Modifier.NONE.value, models.Modifier.IDF.value):
        raise ValueError(f"unknown sparse modifier {par.modifier!r}: Modifier.NONE or Modifier.IDF")
    return name, mod == models.Modifier.IDF.value, int(sparse_slots)


def split_vectors(col: Collection, ids: list, vectors) -> tuple:
    """(dense vectors, sparse list or None) of an upsert's vectors. A plain list or array of
    vectors means "dense only". A dict per point (PointStruct.vector) or one dict of lists
    (Batch.vectors) names them: "" is the dense vector and is required, the collection's sparse
    name maps to a SparseVector (absent or None: none); any other name is a ValueError."""
    def names_ok(d, who):
        for name in d:
            if name != "" and name != col.sparse_name:
                raise ValueError(f"{who}: {name!r} is not a vector of collection {col.name!r} "
                                 f'(it has "" and '
                                 + (repr(col.sparse_name) if col.sparse_name else "no sparse vector")
                                 + ")")
        if "" not in d or d[""] is None:
            raise ValueError(f'{who}: the dense vector (the "" entry) is required')
    if isinstance(vectors, dict):                       # Batch.vectors = {name: [per point]}
        names_ok(vectors, "upsert")
        sp = vectors.get(col.sparse_name) if col.sparse_name else None
        if sp is not None and len(sp) != len(ids):
            raise ValueError(f"upsert: {len(sp)} sparse vectors for {len(ids)} ids")
        return vectors[""], (list(sp) if sp is not None else None)
    if isinstance(vectors, (list, tuple)) and any(isinstance(v, dict) for v in vectors):
        dense, sp = [], []
        for pid, v in zip(ids, vectors):
            if isinstance(v, dict):
                names_ok(v, f"upsert: point {pid!r}")
                dense.append(v[""])
                sp.append(v.get(col.sparse_name) if col.sparse_name else None)
            else:
                dense.append(v)
                sp.append(None)
        return dense, sp
    return vectors, None


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
    return int(rrf_k), prefetch_lists(prefetch, "fusion", "to fuse", "fuses", sparse_ok=True)


def prefetch_lists(prefetch, what: str, to: str, verb: str, sparse_ok: bool = False) -> list:
    """[(vector, Filter or None, limit), ...] of the prefetches of a `what` query — a Prefetch or
    a list of 1 to RAG_FUSION_MAX_LISTS of them, each a plain nearest query with an int limit —
    or ValueError naming what is wrong or not built. sparse_ok (fusion): a prefetch may be
    Prefetch(query=SparseVector(...), using=name, ...); its vector comes back as a
    SparsePrefetch, whose `using` the collection checks. Elsewhere a sparse prefetch is refused,
    naming the route."""
    if isinstance(prefetch, models.Prefetch):
        prefetch = [prefetch]
    if prefetch is None or len(prefetch) == 0:
        raise ValueError(f"a {what} query needs prefetches {to}: prefetch=[Prefetch(...), ...]")
    if len(prefetch) > FUSION_MAX_LISTS:
        raise ValueError(f"a {what} query {verb} at most {FUSION_MAX_LISTS} prefetches, "
                         f"got {len(prefetch)}")
    out = []
    for n, p in enumerate(prefetch):
        if not isinstance(p, models.Prefetch):
            raise ValueError(f"prefetch[{n}] is not a Prefetch")
        if p.prefetch is not None:
            raise ValueError(f"prefetch[{n}]: a nested Prefetch.prefetch is not built")
        vec, mmr = nearest_of(p.query)
        using = getattr(p, "using", None)
        if isinstance(vec, models.SparseVector):
            if not sparse_ok:
                raise ValueError(f"prefetch[{n}]: a sparse prefetch inside a {what} query is not "
                                 "built; sparse prefetches are fused (FusionQuery / RrfQuery)")
            if mmr is not None:
                raise ValueError(f"prefetch[{n}]: an MMR query over a sparse vector is not built")
            if not _is_int(p.limit):
                raise ValueError(f"prefetch[{n}] needs an int limit")
            out.append((SparsePrefetch(vec, using), p.filter, int(p.limit)))
            continue
        if using not in (None, ""):
            raise ValueError(f"prefetch[{n}]: using={using!r} names a sparse vector, but the "
                             "query is a dense vector: pass a SparseVector, or drop `using`")
        if isinstance(vec, models.OrderByQuery):
            raise ValueError(f"prefetch[{n}]: an OrderByQuery inside a Prefetch is not built")
        if isinstance(vec, models.RecommendQuery):
            raise ValueError(f"prefetch[{n}]: a RecommendQuery inside a Prefetch is not built")
        if isinstance(vec, (models.DiscoverQuery, models.ContextQuery)):
            raise ValueError(f"prefetch[{n}]: a {type(vec).__name__} inside a Prefetch is not "
                             "built")
        if vec is None or is_fusion(vec) or isinstance(vec, models.FormulaQuery):
            raise ValueError(f"prefetch[{n}] needs a query: a vector or a NearestQuery")
        if mmr is not None:
            raise ValueError(f"prefetch[{n}]: an MMR query (NearestQuery.mmr) inside a prefetch "
                             "is not built")
        if not _is_int(p.limit):
            raise ValueError(f"prefetch[{n}] needs an int limit")
        out.append((vec, p.filter, int(p.limit)))
    return out


def formula_params(query, prefetch, limit, query_filter=None) -> list:
    """[(vector, Filter or None, limit), ...], the prefetches of a formula request — query a
    FormulaQuery, prefetch a Prefetch or a list of them, under the restrictions fusion places on
    them — or ValueError: a top-level filter, a limit that is no int, no prefetches. The formula
    itself is compiled by the collection (Collection.search_formula), which knows the fields."""
    if not isinstance(query, models.FormulaQuery):
        raise ValueError("formula_params: query must be a FormulaQuery")
    if query_filter is not None:
        raise ValueError("a formula query takes no top-level query_filter: the filter belongs on "
                         "each Prefetch(filter=...)")
    if not _is_int(limit):
        raise ValueError("a formula query needs an int limit")
    return prefetch_lists(prefetch, "formula", "to re-score", "re-scores")


FUSION, FORMULA, MMR, PLAIN = "fusion", "formula", "mmr", "plain"   # the routes of a request
ORDER = "order"
RECOMMEND = "recommend"
DISCOVER = "discover"
SPARSE = "sparse"


def route_of(query, prefetch=None) -> str:
    """The route of a request, decided once: FORMULA (prefetched candidates re-scored by a
    FormulaQuery), FUSION (prefetched lists fused; every other use of a prefetch goes there to
    be refused), ORDER (an OrderByQuery: no vector, the points by a range field's value), MMR (a
    NearestQuery with an Mmr), RECOMMEND (a RecommendQuery, with or without a prefetch: it
    refuses the prefetch itself), DISCOVER (a DiscoverQuery or a ContextQuery, likewise), SPARSE (a
    SparseVector, bare or the `nearest` of a NearestQuery,
    with or without a prefetch: it refuses the prefetch and an Mmr itself) or PLAIN."""
    if isinstance(nearest_of(query)[0], models.SparseVector):
        return SPARSE
    if isinstance(query, models.FormulaQuery):
        return FORMULA
    if isinstance(query, models.RecommendQuery):
        return RECOMMEND
    if isinstance(query, (models.DiscoverQuery, models.ContextQuery)):
        return DISCOVER
    if isinstance(query, models.OrderByQuery):
        return ORDER
    if prefetch is not None or isinstance(query, (models.FusionQuery, models.RrfQuery)):
        return FUSION
    return MMR if isinstance(query, models.NearestQuery) and query.mmr is not None else PLAIN


def order_params(col: Collection, req) -> tuple:
    """(order_by, compiled filter, limit) of an ORDER request, or ValueError: prefetched
    candidates cannot be ordered by a field, the limit must be an int."""
    if getattr(req, "prefetch", None) is not None:
        raise ValueError("an OrderByQuery over prefetched candidates (prefetch=...) is not built: "
                         "it orders the points a query_filter matches")
    if not _is_int(req.limit):
        raise ValueError("an order_by query needs an int limit")
    return req.query.order_by, col.compile_filter(req.filter), int(req.limit)


def recommend_params(query, limit) -> tuple:
    """(positive, negative, strategy code) of a recommend request — the examples as lists of
    point ids and / or vectors — or ValueError: the query must be a RecommendQuery over a
    RecommendInput, each side a list of at most RAG_RECO_MAX_SIDE examples, with at least one
    example in all and, for average_vector (the default), a positive one; the strategy must be a
    RecommendStrategy; the limit must be an int."""
    if not isinstance(query, models.RecommendQuery) or \
            not isinstance(query.recommend, models.RecommendInput):
        raise ValueError("recommend_params: query must be RecommendQuery(recommend="
                         "RecommendInput(...))")
    if not _is_int(limit):
        raise ValueError("a recommend query needs an int limit")
    rec = query.recommend
    sides = []
    for name, side in (("positive", rec.positive), ("negative", rec.negative)):
        if side is None:
            side = []
        if isinstance(side, (str, bytes, dict)) or not hasattr(side, "__len__"):
            raise ValueError(f"RecommendInput.{name} must be a list of point ids and / or vectors")
        if len(side) > RECO_MAX_SIDE:
            raise ValueError(f"a recommend query takes at most {RECO_MAX_SIDE} {name} examples "
                             f"(RAG_RECO_MAX_SIDE), got {len(side)}")
        sides.append(list(side))
    strategy = reco_strategy(rec.strategy)              # ValueError for an unknown one
    pos, neg = sides
    if not pos and not neg:
        raise ValueError("a recommend query needs at least one positive or negative example")
    if strategy == reco_strategy(None) and not pos:
        raise ValueError("RecommendStrategy.AVERAGE_VECTOR needs a positive example; "
                         "best_score and sum_scores take negatives alone")
    return pos, neg, strategy


def recommend_request(col: Collection, req) -> tuple:
    """(positive, negative, strategy, compiled filter, limit) of a RECOMMEND request, or
    ValueError: prefetched candidates cannot be recommended from, recommend scores the dense
    vector only (`using`, SparseVector examples) and knows no other collection's points
    (`lookup_from`)."""
    if getattr(req, "prefetch", None) is not None:
        raise ValueError("a RecommendQuery over prefetched candidates (prefetch=...) is not "
                         "built: it scores every point a query_filter matches")
    for name in ("using", "lookup_from"):
        if getattr(req, name, None) is not None:
            raise ValueError(f"a RecommendQuery with {name}=... is not built: recommend scores "
                             "the dense (unnamed) vector and examples are the collection's own "
                             "points")
    pos, neg, strategy = recommend_params(req.query, req.limit)
    if any(isinstance(x, models.SparseVector) for x in pos + neg):
        raise ValueError("a RecommendQuery with SparseVector examples is not built: recommend "
                         "scores the dense vector")
    return pos, neg, strategy, col.compile_filter(req.filter), int(req.limit)


def discover_params(query, limit) -> tuple:
    """(target or None, [(positive, negative), ...]) of a discovery request — every example a
    point id or a vector; no target: a context search — or ValueError: the query must be a
    DiscoverQuery over a DiscoverInput (a target and 0 to RAG_DISCOVER_MAX_PAIRS pairs) or a
    ContextQuery (1 to RAG_CONTEXT_MAX_PAIRS pairs), its context one ContextPair or a list of
    them, each with both sides; the limit must be an int."""
    if isinstance(query, models.DiscoverQuery):
        if not isinstance(query.discover, models.DiscoverInput):
            raise ValueError("discover_params: query must be DiscoverQuery(discover="
                             "DiscoverInput(target, context))")
        target, context, most, name = query.discover.target, query.discover.context, \
            DISCOVER_MAX_PAIRS, "RAG_DISCOVER_MAX_PAIRS"
        if target is None:
            raise ValueError("a DiscoverQuery needs a target; without one it is a "
                             "ContextQuery(context=[...])")
    elif isinstance(query, models.ContextQuery):
        target, context, most, name = None, query.context, CONTEXT_MAX_PAIRS, \
            "RAG_CONTEXT_MAX_PAIRS"
    else:
        raise ValueError("discover_params: query must be a DiscoverQuery or a ContextQuery")
    what = type(query).__name__
    if not _is_int(limit):
        raise ValueError("a discovery query needs an int limit")
    if context is None:
        context = []
    elif isinstance(context, models.ContextPair):
        context = [context]
    if isinstance(context, (str, bytes, dict)) or not hasattr(context, "__len__"):
        raise ValueError(f"{what}: context must be a ContextPair or a list of them")
    pairs = []
    for n, pair in enumerate(context):
        if not isinstance(pair, models.ContextPair):
            raise ValueError(f"{what}: context[{n}] is not a ContextPair")
        if pair.positive is None or pair.negative is None:
            raise ValueError(f"{what}: context[{n}] needs a positive and a negative example")
        pairs.append((pair.positive, pair.negative))
    if len(pairs) > most:
        raise ValueError(f"a {what} takes at most {most} context pairs ({name}), "
                         f"got {len(pairs)}")
    if target is None and not pairs:
        raise ValueError("a ContextQuery without pairs is not built: it needs at least one "
                         "ContextPair")
    return target, pairs


def discover_request(col: Collection, req) -> tuple:
    """(target or None, pairs, compiled filter, limit) of a DISCOVER request, or ValueError:
    prefetched candidates cannot be discovered among, discovery scores the dense vector only
    (`using`, SparseVector examples) and knows no other collection's points (`lookup_from`)."""
    what = type(req.query).__name__
    if getattr(req, "prefetch", None) is not None:
        raise ValueError(f"a {what} over prefetched candidates (prefetch=...) is not built: it "
                         "scores every point a query_filter matches")
    for name in ("using", "lookup_from"):
        if getattr(req, name, None) is not None:
            raise ValueError(f"a {what} with {name}=... is not built: discovery scores the dense "
                             "(unnamed) vector and examples are the collection's own points")
    target, pairs = discover_params(req.query, req.limit)
    if any(isinstance(x, models.SparseVector) for x in [target] + [x for p in pairs for x in p]):
        raise ValueError(f"a {what} with SparseVector examples is not built: discovery scores "
                         "the dense vector")
    return target, pairs, col.compile_filter(req.filter), int(req.limit)


def sparse_request(col: Collection, req) -> tuple:
    """(SparseVector, using, compiled filter, limit) of a SPARSE request, or ValueError:
    prefetched candidates cannot be re-scored by a sparse query, MMR over a sparse vector is not
    built, the limit must be an int. `using` is checked by the collection."""
    vec, mmr = nearest_of(req.query)
    if getattr(req, "prefetch", None) is not None:
        raise ValueError("a sparse query over prefetched candidates (prefetch=...) is not built: "
                         "fuse a sparse Prefetch with FusionQuery(Fusion.RRF) instead")
    if mmr is not None:
        raise ValueError("an MMR query (NearestQuery.mmr) over a sparse vector is not built")
    if getattr(req, "lookup_from", None) is not None:
        raise ValueError("a sparse query with lookup_from=... is not built")
    if not _is_int(req.limit):
        raise ValueError("a sparse query needs an int limit")
    return vec, getattr(req, "using", None), col.compile_filter(req.filter), int(req.limit)


def dense_using(col: Collection, req) -> None:
    """ValueError for a dense query that names a vector: `using` selects the sparse vector and
    goes with a SparseVector query."""
    using = getattr(req, "using", None)
    if using not in (None, ""):
        raise ValueError(f"using={using!r} with a dense query vector: `using` names the sparse "
                         f"vector of a collection and goes with query=SparseVector(...); drop it "
                         "for a dense query")


def answer(col: Collection, route: str, reqs: list, with_vectors=False, one=False) -> list:
    """The requests of one route (QueryRequests, in order) answered by one call on the
    collection: per request its resolved points (the ORDER route: one order_rows per request
    inside that call). On the MMR route a request without an Mmr rides at diversity 0 with its
    own limit as candidate count."""
    if route == FUSION:
        par = [fusion_params(r.query, r.prefetch, r.limit, r.filter) for r in reqs]
        return col.search_points_fusion(
            [(rrf_k, pres, int(r.limit)) for (rrf_k, pres), r in zip(par, reqs)], with_vectors)
    if route == FORMULA:
        return col.search_points_formula(
            [(r.query, formula_params(r.query, r.prefetch, r.limit, r.filter), int(r.limit))
             for r in reqs], with_vectors)
    if route == ORDER:
        return col.search_points_order([order_params(col, r) for r in reqs], with_vectors)
    if route == RECOMMEND:
        return col.search_points_recommend([recommend_request(col, r) for r in reqs],
                                           with_vectors)
    if route == DISCOVER:
        return col.search_points_discover([discover_request(col, r) for r in reqs], with_vectors)
    if route == SPARSE:
        return col.search_points_sparse([sparse_request(col, r) for r in reqs], with_vectors)
    for r in reqs:
        dense_using(col, r)
    qs, filters, limits, div, cand = [], [], [], [], []
    for r in reqs:
        q, mmr = nearest_of(r.query)
        qs.append(q)
        filters.append(col.compile_filter(r.filter))
        if route == MMR:
            d, c = mmr_params(mmr, r.limit) if mmr is not None else (0.0, max(int(r.limit), 1))
            div.append(d)
            cand.append(c)
        limits.append(int(r.limit))
    Q = stack_queries(qs, col.dim, one=one)
    if route == PLAIN:
        return col.search_points(Q, max(limits), filters, with_vectors)
    return col.search_points_mmr(Q, limits, filters, div, cand, with_vectors)


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
                          capacity: int = 1024, payload_range_fields=None,
                          sparse_vectors_config=None, sparse_slots: int = SPARSE_SLOTS,
                          **kwargs) -> bool:
        """`payload_range_fields`: the numeric payload fields `range` conditions may name, a
        mapping of field to "number" / "datetime" or a sequence of number fields
        (Collection(range_fields=...)); create_payload_index adds one later.
        `sparse_vectors_config`: {name: SparseVectorParams(...)}, the collection's one named
        sparse vector (sparse_config), stored in `sparse_slots` slots per point (a multiple of 16
        in [16, 512]): the most nonzeros a point's sparse vector may hold."""
        if vectors_config.distance != models.Distance.COSINE:
            raise NotImplementedError("only Distance.COSINE collections (database.py:126)")
        storage = _storage_of(vectors_config)
        sparse = sparse_config(sparse_vectors_config, sparse_slots)
        with self._lock:
            if collection_name in self._collections:
                raise ValueError(f"collection {collection_name!r} already exists")
            col = Collection(collection_name, int(vectors_config.size), self.device,
                             tuple(payload_tag_fields), capacity, storage,
                             devices=self.devices, range_fields=payload_range_fields,
                             sparse=sparse)
            col.coalescer.window = self.coalesce_window_s
            self._collections[collection_name] = col
        return True

    def create_payload_index(self, collection_name: str, field_name: str, field_schema=None,
                             **kwargs) -> models.UpdateResult:
        """Qdrant's create_payload_index. PayloadSchemaType.INTEGER / FLOAT declare `field_name`
        a number range field, DATETIME a datetime range field (Collection.add_range_field: a
        key column in HBM, back-filled from the points the collection holds); KEYWORD on one of
        the collection's payload_tag_fields is accepted as a no-op. Repeating a call with the
        same schema is a no-op; a fifth range field is a ValueError; any other schema is
        NotImplementedError."""
        col = self._col(collection_name)
        schema = getattr(field_schema, "value", field_schema)
        schema = schema.lower() if isinstance(schema, str) else schema
        kinds = {models.PayloadSchemaType.INTEGER.value: "number",
                 models.PayloadSchemaType.FLOAT.value: "number",
                 models.PayloadSchemaType.DATETIME.value: "datetime"}
        if schema == models.PayloadSchemaType.KEYWORD.value:
            if field_name not in col.tags.fields:
                raise NotImplementedError(
                    f"a keyword index on {field_name!r}: keyword fields are fixed when the "
                    f"collection is created (payload_tag_fields={col.tags.fields})")
        elif schema in kinds:
            col.add_range_field(field_name, kinds[schema])
        else:
            raise NotImplementedError(f"payload index schema {field_schema!r} is not supported "
                                      "(keyword, integer, float and datetime are)")
        return models.UpdateResult(operation_id=col.op, status=models.UpdateStatus.COMPLETED)

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
        vecs, sparse = split_vectors(col, ids, vecs)
        op = col.upsert(ids, vecs, pls) if sparse is None else col.upsert(ids, vecs, pls, sparse)
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

    def scroll(self, collection_name: str, scroll_filter: models.Filter | None = None,
               limit: int = 10, offset=None, with_payload=True, with_vectors=False,
               order_by=None, **kwargs):
        """Qdrant's scroll: (records, next_page_offset), the points `scroll_filter` matches, page
        by page. Without `order_by` the pages are in storage (row) order — Qdrant pages by point
        id; a documented deviation — which is stable between writes; `offset` is the id the page
        starts at (an unknown id is a ValueError) and next_page_offset the id to pass for the
        next page, None at the end. With `order_by` (a range field's name or an OrderBy): the
        `limit` (<= RAG_ORDER_MAX) first points by that field's value, each Record's order_value
        being its stored payload value, points without the field left out; `offset` is then
        refused and next_page_offset is None (continue with OrderBy.start_from). The rows are
        selected or ranked on the GPU (Collection.scroll)."""
        return self._col(collection_name).scroll(scroll_filter, limit, offset, with_payload,
                                                 with_vectors, order_by)

    def facet(self, collection_name: str, key: str, facet_filter: models.Filter | None = None,
              limit: int = 10, exact: bool = True, **kwargs) -> models.FacetResponse:
        """Qdrant's facet: how many points hold each value of keyword field `key` (one of the
        collection's payload_tag_fields, else NotImplementedError) under `facet_filter`, the
        `limit` most frequent values first, ties by value ascending. Counted on the GPU and
        always exact, whatever `exact` says (Collection.facet)."""
        hits = self._col(collection_name).facet(key, facet_filter, limit)
        return models.FacetResponse(hits=[models.FacetValueHit(value=v, count=n)
                                          for v, n in hits])

    def query_points(self, collection_name: str, query=None, limit: int = 10,
                     query_filter: models.Filter | None = None, with_payload=True,
                     with_vectors=False, prefetch=None, **kwargs) -> models.QueryResponse:
        """One request on its route (route_of, answer). A plain request with a limit the scan
        serves rides the coalescer; fusion, formula, MMR, order_by, recommend and discovery
        requests never do: their prefetches, their candidate search, their ranking of a key
        column, their pass over the examples are passes of their own."""
        col = self._col(collection_name)
        route = route_of(query, prefetch)
        if route == PLAIN and kwargs.get("using") not in (None, ""):
            dense_using(col, models.QueryRequest(query=query, using=kwargs.get("using")))
        if route == PLAIN and self.coalesce and 1 <= int(limit) <= MAX_K and not with_vectors:
            flt = col.compile_filter(query_filter)
            q = stack_queries([nearest_of(query)[0]], col.dim, one=True, host=True)[0]
            pts = col.coalescer.search(q, int(limit), flt)
        else:
            req = models.QueryRequest(query=query, filter=query_filter, limit=limit,
                                      prefetch=prefetch, using=kwargs.get("using"),
                                      lookup_from=kwargs.get("lookup_from"))
            pts = answer(col, route, [req], with_vectors, one=True)[0]
        return models.QueryResponse(points=_payloads(pts, with_payload))

    def query_batch_points(self, collection_name: str, requests: list,
                           **kwargs) -> list[models.QueryResponse]:
        """One GPU scan for the whole batch (per-query filters ride along in the kernel). The
        requests are partitioned by route once, each non-empty route is answered by one call
        (answer), fusion and formula first, then the order_by, the recommend and the discovery
        requests (routes of their own, answered one request at a time, in order), and the
        results are scattered back in request order.
        With MMR requests in the batch the plain requests ride with them, at diversity 0 with their own
        limit as candidate count: one search at the batch's largest candidate count and one
        MMR launch — unless a plain limit exceeds RAG_MMR_MAX_CANDIDATES, in which case the
        plain requests are searched on their own."""
        col = self._col(collection_name)
        routes: dict = {FUSION: [], FORMULA: [], ORDER: [], RECOMMEND: [], DISCOVER: [],
                        SPARSE: [], PLAIN: [], MMR: []}
        for i, r in enumerate(requests):
            routes[route_of(r.query, getattr(r, "prefetch", None))].append(i)
        if routes[MMR] and all(int(requests[i].limit) <= MMR_MAX_CANDIDATES
                               for i in routes[PLAIN]):
            routes = {FUSION: routes[FUSION], FORMULA: routes[FORMULA], ORDER: routes[ORDER],
                      RECOMMEND: routes[RECOMMEND], DISCOVER: routes[DISCOVER],
                      SPARSE: routes[SPARSE],
                      MMR: sorted(routes[MMR] + routes[PLAIN])}
        out: list = [None] * len(requests)
        for route, members in routes.items():
            if members:
                hits = answer(col, route, [requests[i] for i in members])
                for i, h in zip(members, hits):
                    r = requests[i]
                    out[i] = models.QueryResponse(
                        points=_payloads(h[:int(r.limit)], r.with_payload))
        return out

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
        if is_fusion(query) or isinstance(query, models.FormulaQuery) or \
                kwargs.get("prefetch") is not None:
            raise ValueError("a grouped query over prefetched candidates (prefetch, FusionQuery, "
                             "RrfQuery) is not built")
        if isinstance(query, models.RecommendQuery):
            raise ValueError("a grouped query cannot be a RecommendQuery: grouped recommend is "
                             "not built")
        if isinstance(query, (models.DiscoverQuery, models.ContextQuery)):
            raise ValueError(f"a grouped query cannot be a {type(query).__name__}: grouped "
                             "discovery is not built")
        query, mmr = nearest_of(query)
        if isinstance(query, models.SparseVector):
            raise ValueError("a grouped query cannot be a SparseVector query: grouped sparse "
                             "search is not built")
        if mmr is not None:
            raise ValueError("a grouped query cannot be an MMR query (NearestQuery.mmr)")
        flt = col.compile_filter(query_filter)
        found = col.search_groups(stack_queries([query], col.dim, one=True), group_by, int(limit),
                                  int(group_size), [flt], with_vectors)[0]
        for g in found:
            _payloads(g.hits, with_payload)
        return models.GroupsResult(groups=found)

    def recommend(self, collection_name: str, positive=None, negative=None, query_filter=None,
                  limit: int = 10, strategy=None, with_payload=True, with_vectors=False,
                  **kwargs):
        """Legacy qdrant_client.recommend: list[ScoredPoint] of
        query_points(query=RecommendQuery(RecommendInput(positive, negative, strategy)))."""
        query = models.RecommendQuery(recommend=models.RecommendInput(
            positive=positive, negative=negative, strategy=strategy))
        return self.query_points(collection_name, query, limit, query_filter, with_payload,
                                 with_vectors, **kwargs).points

    def discover(self, collection_name: str, target=None, context=None, query_filter=None,
                 limit: int = 10, with_payload=True, with_vectors=False, **kwargs):
        """Legacy qdrant_client.discover: list[ScoredPoint] of query_points with
        DiscoverQuery(DiscoverInput(target, context)) when a target is given, else with
        ContextQuery(context)."""
        query = models.ContextQuery(context=context) if target is None else \
            models.DiscoverQuery(discover=models.DiscoverInput(target=target, context=context))
        return self.query_points(collection_name, query, limit, query_filter, with_payload,
                                 with_vectors, **kwargs).points

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
