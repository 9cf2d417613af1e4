"""The reference's RAG-core function layer on the MI355X path (drop-in for main.py / main2.py /
ingest.py's hot-path functions, same names, arguments, return shapes and TESTING stubs).

  get_embedder / get_reranker / get_qdrant   main.py:80-95, main2.py:88-108 (lazy singletons)
  embed_query(query) -> list[float] (384)    main.py:211-213 (TESTING: zeros)
  embed_query_batch(queries) -> list[list]   main2.py:170-171
  embed(texts) -> {"embeddings": ...}        main.py:144-149 /embed (TESTING: zeros)
  retrieve_from_qdrant(vec, ticker, document_type=None, limit=15)
                                             main.py:215-239 (exception -> empty .points)
  rerank_documents(query, texts, top_k) -> (idx, scores)
                                             main.py:241-247 (TESTING: range / zeros)
  ensure_collection, embed_chunks, chunk_points, upsert_points
                                             ingest.py:52-66, 86-96, 148-175
plus the batched forms a rewritten main2.batch_processor uses:
  retrieve_batch  -> one GPU scan for all requests of a micro-batch (per-query filters)
  rerank_batch    -> one cross-encoder forward for all (query, chunk) pairs of a micro-batch
and, not in the reference:
  similar_chunks  -> the chunks most like some chunks and least like others (recommend query)
  retrieve_steered -> retrieve_from_qdrant steered by (liked, disliked) chunk pairs (discovery)
  hybrid retrieval -> ensure_collection(hybrid=True), chunk_points(sparse=True) and
                     retrieve_from_qdrant(hybrid_text=...): a BM25 sparse vector "bm25" beside
                     the dense one, fused by reciprocal rank (ragmi.sparse, DESIGN R19)

Models come from local directories (env RAGMI_BGE_DIR, RAGMI_CE_DIR: config.json +
model.safetensors + vocab.txt) — the reference's hub names cannot be fetched here. Env
RAGMI_STORAGE (optional) points the in-HBM collection at an on-disk shard directory
(ragmi.store), the role of the reference's Qdrant storage volume. Env RAGMI_DEVICES (optional,
"0,1,2,3" or "all") stripes the collection over several GPUs of the node from this one
process (ragmi.shardset); the functions below do not change.
"""
from __future__ import annotations

import hashlib
import os
from datetime import datetime, timezone
from functools import lru_cache

import numpy as np

from . import qdrant_models as models

TESTING = os.getenv("TESTING", "False") == "True"
QDRANT_URL = os.getenv("QDRANT_URL", "http://qdrant:6333")
COLLECTION_NAME = "financial_documents"          # main.py:25
VECTOR_SIZE = 384                                # database.py:31
EMBED_BATCH = 64                                 # ingest.py:27
UPSERT_BATCH = 256                               # ingest.py:28
RETRIEVE_LIMIT = 15                              # main.py:215
PRECISION = os.getenv("RAGMI_PRECISION", "fp16x3")
# main.py:23 — the loaders pass device = "cuda" if USE_GPU else "cpu" (main.py:83,89), read per
# call here so tests can set it; "cpu" makes the encoders raise RagmiDeviceError (this build
# has no CPU path): set USE_GPU=true, as the reference needs on a GPU host.


def _device() -> str:
    return "cuda" if os.getenv("USE_GPU", "false").lower() == "true" else "cpu"


def _testing() -> bool:
    return os.getenv("TESTING", "False") == "True"


# ------------------------------------------------------------------ lazy loaders
@lru_cache()
def get_embedder():
    if _testing():
        return None
    from .encoders import SentenceTransformer
    d = os.environ.get("RAGMI_BGE_DIR")
    if not d:
        raise RuntimeError("set RAGMI_BGE_DIR to a local bge-small-en-v1.5 directory "
                           "(config.json, model.safetensors, vocab.txt)")
    return SentenceTransformer(d, device=_device(), precision=PRECISION)


@lru_cache()
def get_reranker():
    if _testing():
        return None
    from .encoders import CrossEncoder
    d = os.environ.get("RAGMI_CE_DIR")
    if not d:
        raise RuntimeError("set RAGMI_CE_DIR to a local ms-marco-MiniLM-L-6-v2 directory")
    return CrossEncoder(d, device=_device(), precision=PRECISION)


@lru_cache()
def get_qdrant():
    if _testing():
        return None
    from .qdrant import QdrantClient
    # RAGMI_STORAGE: directory of saved collections (the Qdrant volume's role); loaded here,
    # written back by QdrantClient.save()/close(). RAGMI_DEVICES ("0,1,2,3" or "all"): the
    # collections are striped over these GPUs (ragmi.shardset); unset: one GPU
    return QdrantClient(url=QDRANT_URL, path=os.environ.get("RAGMI_STORAGE") or None,
                        devices=os.environ.get("RAGMI_DEVICES") or None)


# ------------------------------------------------------------------ stage 1: embed
def embed_query(query: str):
    if _testing():
        return [0.0] * VECTOR_SIZE
    return get_embedder().encode(query).tolist()


def embed_query_batch(queries):
    if _testing():
        return [[0.0] * VECTOR_SIZE for _ in queries]
    return get_embedder().encode(list(queries)).tolist()


def embed(texts):
    """/embed endpoint body (main.py:144-149)."""
    if _testing():
        return {"embeddings": [[0.0] * VECTOR_SIZE for _ in texts]}
    return {"embeddings": get_embedder().encode(list(texts)).tolist()}


# ------------------------------------------------------------------ stage 2: search
class _Empty:
    points: list = []


def _match(value):
    """A string: the reference's MatchValue of its upper case; a list or tuple of strings (a
    cross-company question, "10-K or 10-Q"): MatchAny of theirs."""
    if isinstance(value, (list, tuple)):
        return models.MatchAny(any=[v.upper() for v in value])
    return models.MatchValue(value=value.upper())


def _filter(ticker, document_type=None, ingested_since=None, ingested_until=None):
    must = [models.FieldCondition(key="ticker", match=_match(ticker))]
    if document_type:
        must.append(models.FieldCondition(key="document_type", match=_match(document_type)))
    if ingested_since is not None or ingested_until is not None:
        must.append(models.FieldCondition(key="ingested_at", range=models.DatetimeRange(
            gte=ingested_since, lt=ingested_until)))
    return models.Filter(must=must)


def _query(vector, diversity, candidates):
    """The `query` argument of a retrieval: the vector itself (the reference's call), or with
    `diversity` / `candidates` set, a NearestQuery that re-selects the hits by MMR."""
    if diversity is None and candidates is None:
        return vector
    return models.NearestQuery(nearest=vector,
                               mmr=models.Mmr(diversity=diversity, candidates_limit=candidates))


FUSION_PREFETCH = 50         # a rewrite's list is max(limit, this) hits long
SPARSE_NAME = "bm25"         # the sparse vector of a hybrid collection (ensure_collection)


def sparse_texts(texts, kind: str) -> list:
    """The BM25 SparseVector of each text, from the embedder's own WordPiece vocabulary:
    kind "document" (ragmi.sparse.bm25_document) or "query" (bm25_query)."""
    from .sparse import bm25_document, bm25_query, sequences
    ids, _, cu = get_embedder().tokenizer.encode_packed(list(texts))
    make = bm25_document if kind == "document" else bm25_query
    return [make(seq) for seq in sequences(ids, cu)]



def _fusion(vector, rewrites, flt, limit, rrf_k, diversity, candidates, sparse=None):
    """(query, prefetch) of a multi-query retrieval: the original vector and each rewrite become
    one Prefetch under the request's filter, fused by reciprocal rank (rrf_k None: the default
    constant). `sparse` (a SparseVector): one sparse prefetch of the same filter and limit more
    (hybrid retrieval)."""
    if diversity is not None or candidates is not None:
        raise ValueError("rewrites (fusion) cannot be combined with diversity / candidates (MMR)")
    query = (models.FusionQuery(fusion=models.Fusion.RRF) if rrf_k is None else
             models.RrfQuery(rrf=models.Rrf(k=rrf_k)))
    prefetch = [models.Prefetch(query=v, filter=flt, limit=max(limit, FUSION_PREFETCH))
                for v in [vector, *rewrites]]
    if sparse is not None:
        prefetch.append(models.Prefetch(query=sparse, using=SPARSE_NAME, filter=flt,
                                        limit=max(limit, FUSION_PREFETCH)))
    return query, prefetch


RECENCY_PREFETCH = 50        # a recency boost re-scores max(limit, this) hits
RECENCY_FIELD = "ingested_at"
RECENCY_DEFAULT = "1970-01-01T00:00:00Z"      # a chunk without a timestamp is as old as can be


def _recency(vector, recency, recency_now, flt, limit, diversity, candidates, rewrites):
    """(query, prefetch) of a recency-boosted retrieval, recency = (half_life_days, weight):
    $score + weight * exp_decay(datetime_key "ingested_at", target = now, scale = half_life_days
    * 86400 s, midpoint 0.5) over one prefetch of max(limit, 50) hits under the request's
    filter; a chunk without a timestamp counts as from the epoch. recency_now None: the current
    UTC time."""
    if diversity is not None or candidates is not None or rewrites is not None:
        raise ValueError("recency (a formula query) cannot be combined with rewrites (fusion) "
                         "or diversity / candidates (MMR)")
    half_life_days, weight = recency
    now = datetime.now(timezone.utc) if recency_now is None else recency_now
    decay = models.ExpDecayExpression(exp_decay=models.DecayParamsExpression(
        x=models.DatetimeKeyExpression(datetime_key=RECENCY_FIELD),
        target=models.DatetimeExpression(datetime=now),
        scale=float(half_life_days) * 86400.0, midpoint=0.5))
    query = models.FormulaQuery(
        formula=models.SumExpression(sum=[
            "$score", models.MultExpression(mult=[float(weight), decay])]),
        defaults={RECENCY_FIELD: RECENCY_DEFAULT})
    return query, [models.Prefetch(query=vector, filter=flt, limit=max(limit, RECENCY_PREFETCH))]


def retrieve_from_qdrant(query_vector, ticker, document_type=None, limit=RETRIEVE_LIMIT, *,
                         diversity=None, candidates=None, rewrites=None, rrf_k=None,
                         ingested_since=None, ingested_until=None, recency=None,
                         recency_now=None, hybrid_text=None):
    """ingested_since / ingested_until (keyword-only, not in the reference): only chunks whose
    `ingested_at` timestamp lies in [since, until) — RFC 3339 strings or datetime / date objects,
    either may be None; a DatetimeRange on `ingested_at` joins the `must` list. The collection
    needs `ingested_at` declared a datetime range field (one
    create_payload_index line); without it the filter is refused, which reads as no documents
    here, as every failure does. Both None is today's call.
    diversity / candidates (keyword-only, not in the reference): MMR re-selection of the
    `limit` hits from the `candidates` nearest (Mmr's defaults where one is None), so
    near-duplicate chunks do not fill the list; both None is the reference's call.
    rewrites (keyword-only): extra query vectors for the same question; the lists of the
    original and of each rewrite, max(limit, 50) hits under the same filter, are fused by
    reciprocal rank (constant rrf_k, None = 2) and cut to `limit`. None is today's call; with
    diversity / candidates it is a ValueError.
    recency (keyword-only) = (half_life_days, weight): newer chunks are boosted; the max(limit,
    50) nearest under the same filter are re-scored as $score + weight * 0.5 ** (age /
    half_life_days), age measured from `recency_now` (a datetime or RFC 3339 string; None = the
    current UTC time) to the chunk's `ingested_at`, and cut to `limit`. The collection needs
    `ingested_at` declared a datetime range field, as for ingested_since. None is today's call;
    with rewrites or diversity / candidates it is a ValueError.
    hybrid_text (keyword-only, not in the reference): the question's text; its BM25 query vector
    (the distinct WordPiece terms, weighted by the collection's IDF) becomes one sparse prefetch
    of the same filter and limit beside the dense one(s), fused by reciprocal rank as rewrites
    are. The collection needs the sparse vector "bm25" (ensure_collection(hybrid=True)) and
    chunks ingested with chunk_points(sparse=True). None is today's call; with recency or
    diversity / candidates it is a ValueError."""
    if _testing():
        return type("obj", (object,), {"points": []})
    if hybrid_text is not None:
        if recency is not None:
            raise ValueError("hybrid_text (fusion) cannot be combined with recency (a formula "
                             "query)")
        query, prefetch = _fusion(query_vector, rewrites or [],
                                  _filter(ticker, document_type, ingested_since, ingested_until),
                                  limit, rrf_k, diversity, candidates,
                                  sparse=sparse_texts([hybrid_text], "query")[0])
        try:
            return get_qdrant().query_points(collection_name=COLLECTION_NAME, query=query,
                                             prefetch=prefetch, limit=limit)
        except Exception:
            return type("obj", (object,), {"points": []})
    if recency is not None:
        query, prefetch = _recency(query_vector, recency, recency_now,
                                   _filter(ticker, document_type, ingested_since, ingested_until),
                                   limit, diversity, candidates, rewrites)
        try:
            return get_qdrant().query_points(collection_name=COLLECTION_NAME, query=query,
                                             prefetch=prefetch, limit=limit)
        except Exception:
            return type("obj", (object,), {"points": []})
    if rewrites is not None:
        query, prefetch = _fusion(query_vector, rewrites,
                                  _filter(ticker, document_type, ingested_since, ingested_until),
                                  limit, rrf_k, diversity, candidates)
        try:
            return get_qdrant().query_points(collection_name=COLLECTION_NAME, query=query,
                                             prefetch=prefetch, limit=limit)
        except Exception:
            return type("obj", (object,), {"points": []})
    # the reference's swallow-to-empty (main.py:232-239) unchanged: query_points answers any
    # limit exactly (large limits on the full exact pass), so an exception here is a real
    # failure, as it is for the reference's Qdrant call
    try:
        return get_qdrant().query_points(collection_name=COLLECTION_NAME,
                                         query=_query(query_vector, diversity, candidates),
                                         limit=limit,
                                         query_filter=_filter(ticker, document_type,
                                                              ingested_since, ingested_until))
    except Exception:
        return type("obj", (object,), {"points": []})


def similar_chunks(point_ids, not_like=(), ticker=None, limit=RETRIEVE_LIMIT):
    """Not in the reference: the `limit` chunks most like the chunks `point_ids` and least like
    the chunks `not_like` (point ids both; "like these two risk-factor paragraphs, not like this
    boilerplate one"), by Qdrant's best_score recommendation, under retrieve_from_qdrant's ticker
    filter when `ticker` is given. The example chunks are never among the hits. Every failure
    reads as no documents, as in retrieve_from_qdrant."""
    if _testing():
        return type("obj", (object,), {"points": []})
    query = models.RecommendQuery(recommend=models.RecommendInput(
        positive=list(point_ids), negative=list(not_like),
        strategy=models.RecommendStrategy.BEST_SCORE))
    try:
        return get_qdrant().query_points(collection_name=COLLECTION_NAME, query=query,
                                         limit=limit,
                                         query_filter=_filter(ticker) if ticker else None)
    except Exception:
        return type("obj", (object,), {"points": []})


def retrieve_steered(query_vector, prefer, ticker=None, limit=RETRIEVE_LIMIT):
    """Not in the reference: retrieve_from_qdrant steered by feedback. `prefer` is a list of
    (liked_point_id, disliked_point_id): the `limit` chunks nearest `query_vector` among those
    that lie on the liked side of the most pairs ("nearest to this question, but like the
    paragraphs users up-voted rather than the ones they down-voted"), by Qdrant's discovery
    search with the query as the target, under retrieve_from_qdrant's ticker filter when
    `ticker` is given. The example chunks are never among the hits. Every failure reads as no
    documents, as in retrieve_from_qdrant."""
    if _testing():
        return type("obj", (object,), {"points": []})
    query = models.DiscoverQuery(discover=models.DiscoverInput(
        target=query_vector,
        context=[models.ContextPair(positive=p, negative=n) for p, n in prefer]))
    try:
        return get_qdrant().query_points(collection_name=COLLECTION_NAME, query=query,
                                         limit=limit,
                                         query_filter=_filter(ticker) if ticker else None)
    except Exception:
        return type("obj", (object,), {"points": []})


def retrieve_batch(query_vectors, tickers, document_types=None, limit=RETRIEVE_LIMIT, *,
                   diversity=None, candidates=None, rewrites=None, rrf_k=None, recency=None,
                   recency_now=None):
    """One GPU scan for a whole micro-batch (main2.py:281-295 + 228), per-request filters;
    diversity / candidates as in retrieve_from_qdrant, for every request of the batch.
    rewrites: per request a list of extra query vectors (as in retrieve_from_qdrant); every
    prefetch of the batch rides one scan and one fusion launch.
    recency / recency_now: as in retrieve_from_qdrant, for every request of the batch (one
    `now` for all of them); one scan, one gather and one formula launch."""
    if _testing():
        return [type("obj", (object,), {"points": []}) for _ in tickers]
    document_types = document_types or [None] * len(tickers)
    if recency is not None:
        now = datetime.now(timezone.utc) if recency_now is None else recency_now
        reqs = []
        for v, t, d in zip(query_vectors, tickers, document_types):
            query, prefetch = _recency(v, recency, now, _filter(t, d), limit, diversity,
                                       candidates, rewrites)
            reqs.append(models.QueryRequest(query=query, prefetch=prefetch, limit=limit))
        return get_qdrant().query_batch_points(COLLECTION_NAME, reqs)
    if rewrites is not None:
        reqs = []
        for v, t, d, rw in zip(query_vectors, tickers, document_types, rewrites):
            query, prefetch = _fusion(v, rw or [], _filter(t, d), limit, rrf_k, diversity,
                                      candidates)
            reqs.append(models.QueryRequest(query=query, prefetch=prefetch, limit=limit))
        return get_qdrant().query_batch_points(COLLECTION_NAME, reqs)
    reqs = [models.QueryRequest(query=_query(v, diversity, candidates), limit=limit,
                                filter=_filter(t, d))
            for v, t, d in zip(query_vectors, tickers, document_types)]
    return get_qdrant().query_batch_points(COLLECTION_NAME, reqs)


# ------------------------------------------------------------------ stage 3: rerank
def rerank_documents(query, texts, top_k):
    if _testing() or not texts:
        return list(range(min(top_k, len(texts)))), np.zeros(len(texts))
    scores = get_reranker().predict([[query, t] for t in texts])
    idx = np.argsort(scores)[::-1][:top_k]
    return idx, scores


def rerank_batch(queries, texts_lists, top_k):
    """All (query, chunk) pairs of a micro-batch in ONE cross-encoder forward; per request
    the same (idx, scores) as rerank_documents."""
    if _testing():
        return [rerank_documents(q, t, top_k) for q, t in zip(queries, texts_lists)]
    pairs, owner = [], []
    for i, (q, texts) in enumerate(zip(queries, texts_lists)):
        pairs += [[q, t] for t in texts]
        owner += [i] * len(texts)
    # batch_size = all pairs: ONE packed forward (CrossEncoder.predict's default of 32 would
    # split a 32 x 15 micro-batch into 15 forwards)
    scores = (get_reranker().predict(pairs, batch_size=len(pairs)) if pairs
              else np.zeros(0, np.float32))
    out, pos = [], 0
    for i, texts in enumerate(texts_lists):
        s = scores[pos:pos + len(texts)]
        pos += len(texts)
        if len(texts) == 0:
            out.append(([], np.zeros(0)))
        else:
            out.append((np.argsort(s)[::-1][:top_k], s))
    return out


# ------------------------------------------------------------------ ingest
def ensure_collection(qdrant, collection_name=COLLECTION_NAME, hybrid=False):
    """ingest.py:86-96 / database.py:111-143. hybrid=True (not in the reference): the collection
    also declares the sparse vector "bm25" with Modifier.IDF, for chunk_points(sparse=True) and
    retrieve_from_qdrant(hybrid_text=...)."""
    if not qdrant.collection_exists(collection_name):
        extra = {} if not hybrid else {"sparse_vectors_config": {
            SPARSE_NAME: models.SparseVectorParams(modifier=models.Modifier.IDF)}}
        qdrant.create_collection(collection_name=collection_name,
                                 vectors_config=models.VectorParams(size=VECTOR_SIZE,
                                                                    distance=models.Distance.COSINE),
                                 **extra)


def embed_chunks(chunks, batch=EMBED_BATCH):
    """ingest.py:52-66 without the HTTP hop: same batching, local GPU embedder."""
    out = []
    for i in range(0, len(chunks), batch):
        out.extend(embed(chunks[i:i + batch])["embeddings"])
    return out


def chunk_points(ticker, f_type, file, chunks, embeddings, ingested_at=None, sparse=False):
    """ingest.py:148-168: md5 point ids (idempotent re-ingest) + payloads. sparse=True (not in
    the reference): every point's vector is {"": dense, "bm25": bm25_document of the chunk}, for a
    collection made by ensure_collection(hybrid=True)."""
    ts = ingested_at or datetime.now(timezone.utc).isoformat()
    pts = []
    bm25 = sparse_texts(chunks, "document") if sparse else None
    for n, (chunk, vector) in enumerate(zip(chunks, embeddings)):
        h = hashlib.md5(f"{ticker}_{f_type}_{file}_{chunk}".encode()).hexdigest()
        if bm25 is not None:
            vector = {"": vector, SPARSE_NAME: bm25[n]}
        pts.append(models.PointStruct(id=h, vector=vector, payload={
            "ticker": ticker.upper(), "document_type": f_type.upper(), "text": chunk,
            "source_file": file, "ingested_at": ts}))
    return pts


def upsert_points(qdrant, points, collection_name=COLLECTION_NAME, batch=UPSERT_BATCH):
    """ingest.py:171-175: memory-safe batched upsert."""
    for i in range(0, len(points), batch):
        qdrant.upsert(collection_name=collection_name, points=points[i:i + batch])
