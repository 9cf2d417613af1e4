"""Qdrant model types used by the reference, restated for the in-HBM index.

The reference imports `from qdrant_client.http import models` (main.py:36) and
`from qdrant_client.http.models import PointStruct, Distance, VectorParams` (ingest.py:11),
and uses: Distance.COSINE, VectorParams(size, distance), PointStruct(id, vector, payload),
Filter(must=[...]), FieldCondition(key, match=MatchValue(value)) (main.py:218-236), and
reads QueryResponse.points[i].id / .score / .payload (main.py:380, main2.py:230).
These dataclasses keep the same constructor keywords and attribute names.
"""
from __future__ import annotations

import enum
from dataclasses import dataclass, field
from typing import Any, Optional, Union

ExtendedPointId = Union[int, str]


class Distance(str, enum.Enum):
    COSINE = "Cosine"
    EUCLID = "Euclid"
    DOT = "Dot"
    MANHATTAN = "Manhattan"


class Datatype(str, enum.Enum):
    FLOAT32 = "float32"
    FLOAT16 = "float16"
    UINT8 = "uint8"


@dataclass
class VectorParams:
    size: int
    distance: Distance = Distance.COSINE
    on_disk: Optional[bool] = None
    # None = Qdrant's default, Float32 (the reference sets none: database.py:124-130,
    # ingest.py:89-95) -> fp32 storage; FLOAT16 -> fp16 storage (ragmi FlatIndex storage)
    datatype: Optional[str] = None


@dataclass
class SparseVector:
    """A sparse vector: values[i] at index indices[i]. Indices are distinct integers in
    [0, 65535) here (Qdrant: uint32), values finite; explicit zeros are dropped."""
    indices: list
    values: list


@dataclass
class SparseIndexParams:
    """Accepted and ignored (the sparse rows are scored flat, in HBM) except for `datatype`:
    anything but float32 is NotImplementedError."""
    full_scan_threshold: Optional[int] = None
    on_disk: Optional[bool] = None
    datatype: Optional[str] = None


class Modifier(str, enum.Enum):
    NONE = "none"
    IDF = "idf"


@dataclass
class SparseVectorParams:
    """One named sparse vector of create_collection(sparse_vectors_config={name: ...}).
    modifier Modifier.IDF: query weights are multiplied by the term's inverse document frequency
    (ragmi.sparse.idf_weights)."""
    index: Optional[SparseIndexParams] = None
    modifier: Optional[Modifier] = None


@dataclass
class PointStruct:
    """`vector`: the dense vector, or in a collection with a sparse vector a dict {"": dense,
    name: SparseVector}."""
    id: ExtendedPointId
    vector: Any
    payload: Optional[dict] = None


@dataclass
class Batch:
    ids: list
    vectors: Any
    payloads: Optional[list] = None


@dataclass
class MatchValue:
    value: Any


@dataclass
class MatchAny:
    any: list


@dataclass
class MatchExcept:
    """The field is present and none of these values (Qdrant's `except`, a Python keyword:
    the field is spelled `except_` as in qdrant_client)."""
    except_: list


@dataclass
class Range:
    """FieldCondition(key, range=Range(...)) on a number field: the value lies above `gt` /
    at or above `gte` and below `lt` / at or below `lte`; None = no bound on that side."""
    lt: Optional[float] = None
    gt: Optional[float] = None
    gte: Optional[float] = None
    lte: Optional[float] = None


@dataclass
class DatetimeRange:
    """Range on a datetime field: the bounds are RFC 3339 / ISO-8601 strings, or datetime /
    date objects (naive values are UTC, a date is its midnight)."""
    lt: Any = None
    gt: Any = None
    gte: Any = None
    lte: Any = None


class PayloadSchemaType(str, enum.Enum):
    """field_schema of QdrantClient.create_payload_index. INTEGER / FLOAT / DATETIME declare a
    range field, KEYWORD names an existing tag field; the others are refused."""
    KEYWORD = "keyword"
    INTEGER = "integer"
    FLOAT = "float"
    DATETIME = "datetime"
    BOOL = "bool"
    GEO = "geo"
    TEXT = "text"
    UUID = "uuid"


@dataclass
class FieldCondition:
    """`match` or `range` (a Range, a DatetimeRange, or a dict with the keys lt / gt / gte /
    lte), not both."""
    key: str
    match: Any = None
    range: Any = None


@dataclass
class PayloadField:
    key: str


@dataclass
class IsEmptyCondition:
    """The field is absent (or holds no scalar keyword value; ragmi.filters)."""
    is_empty: PayloadField


@dataclass
class MinShould:
    """Filter.min_should: at least `min_count` of `conditions` match."""
    conditions: list
    min_count: int


@dataclass
class Filter:
    must: Optional[list] = None
    should: Optional[list] = None
    must_not: Optional[list] = None
    min_should: Any = None


@dataclass
class PointIdsList:
    """Points selector of QdrantClient.delete: the points with these ids."""
    points: list = field(default_factory=list)
    shard_key: Any = None


@dataclass
class FilterSelector:
    """Points selector of QdrantClient.delete: the points a Filter matches."""
    filter: Optional[Filter] = None
    shard_key: Any = None


@dataclass
class ScoredPoint:
    id: ExtendedPointId
    version: int
    score: float
    payload: Optional[dict] = None
    vector: Any = None
    shard_key: Any = None
    order_value: Any = None


@dataclass
class Record:
    id: ExtendedPointId
    payload: Optional[dict] = None
    vector: Any = None
    shard_key: Any = None
    order_value: Any = None


@dataclass
class QueryResponse:
    points: list = field(default_factory=list)


@dataclass
class PointGroup:
    """One group of query_points_groups: the hits (ScoredPoints, best first) sharing the value
    `id` of the group_by payload field."""
    hits: list
    id: Any
    lookup: Any = None


@dataclass
class GroupsResult:
    groups: list = field(default_factory=list)


@dataclass
class CollectionDescription:
    name: str


@dataclass
class CollectionsResponse:
    collections: list = field(default_factory=list)


class UpdateStatus(str, enum.Enum):
    ACKNOWLEDGED = "acknowledged"
    COMPLETED = "completed"


@dataclass
class UpdateResult:
    operation_id: Optional[int]
    status: UpdateStatus


@dataclass
class CountResult:
    count: int


@dataclass
class Mmr:
    """Maximal marginal relevance parameters of a NearestQuery (Qdrant's query API). None
    fields take the defaults of QdrantClient.query_points: diversity 0.5, candidates_limit
    max(limit, 100)."""
    diversity: Optional[float] = None
    candidates_limit: Optional[int] = None


@dataclass
class NearestQuery:
    """query_points(query=NearestQuery(nearest=vector, mmr=Mmr(...))): the nearest points to
    `nearest`, re-selected for diversity when `mmr` is set; without it, the plain query."""
    nearest: Any
    mmr: Optional[Mmr] = None


class RecommendStrategy(str, enum.Enum):
    AVERAGE_VECTOR = "average_vector"
    BEST_SCORE = "best_score"
    SUM_SCORES = "sum_scores"


@dataclass
class RecommendInput:
    """The examples of a recommend query: `positive` and `negative` are lists of point ids
    and / or vectors (at most 16 each); `strategy` None takes RecommendStrategy.AVERAGE_VECTOR."""
    positive: Optional[list] = None
    negative: Optional[list] = None
    strategy: Optional[RecommendStrategy] = None


@dataclass
class RecommendQuery:
    """query_points(query=RecommendQuery(recommend=RecommendInput(...))): the points most like
    the positive examples and least like the negative ones; points given as examples by id are
    never among the hits."""
    recommend: RecommendInput


@dataclass
class ContextPair:
    """One example pair of a discovery or context query: a point id or a vector each."""
    positive: Any
    negative: Any


@dataclass
class DiscoverInput:
    """The examples of a discovery query: `target` a point id or a vector, `context` one
    ContextPair or a list of them (at most 15; none is allowed)."""
    target: Any
    context: Any = None


@dataclass
class DiscoverQuery:
    """query_points(query=DiscoverQuery(discover=DiscoverInput(target, context))): the points
    nearest the target among those on the positive side of the most context pairs; points given
    as examples by id are never among the hits."""
    discover: DiscoverInput


@dataclass
class ContextQuery:
    """query_points(query=ContextQuery(context=[ContextPair(...), ...])): the points on the
    positive side of every pair first (score 0), the others by how far they miss; `context` is
    one ContextPair or a list of 1 to 16."""
    context: Any


class Fusion(str, enum.Enum):
    RRF = "rrf"
    DBSF = "dbsf"


@dataclass
class FusionQuery:
    """query_points(prefetch=[Prefetch(...), ...], query=FusionQuery(fusion=Fusion.RRF)): the
    prefetched lists fused by reciprocal rank, with the default constant 2."""
    fusion: Fusion


@dataclass
class Rrf:
    """Reciprocal rank fusion parameters: a hit at 0-based position p of a prefetched list
    contributes 1 / (k + p). None takes the default, 2."""
    k: Optional[int] = None


@dataclass
class RrfQuery:
    """FusionQuery(Fusion.RRF) with its constant spelled out: RrfQuery(rrf=Rrf(k=60))."""
    rrf: Rrf


@dataclass
class Prefetch:
    """One candidate list of a fusion or formula query: the `limit` nearest points to `query` (a vector,
    or a NearestQuery without mmr) under `filter`. A nested `prefetch` is refused. In a fusion
    query `query` may be a SparseVector with `using` naming the collection's sparse vector."""
    query: Any = None
    filter: Optional[Filter] = None
    limit: int = 10
    prefetch: Any = None
    using: Any = None


# ---- formula queries (score boosting): the expression tree of FormulaQuery.formula. An
# expression is one of these, a number (a constant), a str (a variable: "$score", "$score[i]"
# or the name of a number range field), or a condition (FieldCondition, IsEmptyCondition,
# Filter: 1.0 when the candidate passes, else 0.0). ragmi.formula compiles it.
@dataclass
class SumExpression:
    sum: list


@dataclass
class MultExpression:
    mult: list


@dataclass
class NegExpression:
    neg: Any


@dataclass
class AbsExpression:
    abs: Any


@dataclass
class DivisionParams:
    """left / right; `by_zero_default`: the value when right == 0.0 (None: the request fails)."""
    left: Any
    right: Any
    by_zero_default: Optional[float] = None


@dataclass
class DivExpression:
    div: DivisionParams


@dataclass
class DatetimeExpression:
    """A constant point in time (an RFC 3339 string or a datetime / date object), as seconds
    since the epoch."""
    datetime: Any


@dataclass
class DatetimeKeyExpression:
    """The value of a datetime range field, as seconds since the epoch."""
    datetime_key: str


@dataclass
class DecayParamsExpression:
    """Decay of |x - target|: `scale` is the distance at which the decay reaches `midpoint`.
    None fields take the defaults: target 0.0, scale 1.0, midpoint 0.5."""
    x: Any
    target: Any = None
    scale: Optional[float] = None
    midpoint: Optional[float] = None


@dataclass
class LinDecayExpression:
    lin_decay: DecayParamsExpression


@dataclass
class ExpDecayExpression:
    exp_decay: DecayParamsExpression


@dataclass
class GaussDecayExpression:
    gauss_decay: DecayParamsExpression


@dataclass
class SqrtExpression:
    """Not built (refused by ragmi.formula, like the five below)."""
    sqrt: Any


@dataclass
class PowParams:
    base: Any
    exponent: Any


@dataclass
class PowExpression:
    pow: PowParams


@dataclass
class ExpExpression:
    exp: Any


@dataclass
class Log10Expression:
    log10: Any


@dataclass
class LnExpression:
    ln: Any


@dataclass
class GeoDistanceParams:
    origin: Any
    to: str


@dataclass
class GeoDistance:
    geo_distance: GeoDistanceParams


@dataclass
class FormulaQuery:
    """query_points(prefetch=[Prefetch(...), ...], query=FormulaQuery(formula=<expression>,
    defaults={...})): the prefetched candidates re-scored by the formula. `defaults`: the value
    of a variable a candidate lacks, keyed by field name or "$score[i]"."""
    formula: Any
    defaults: dict = field(default_factory=dict)


class Direction(str, enum.Enum):
    ASC = "asc"
    DESC = "desc"


@dataclass
class OrderBy:
    """Order of scroll(order_by=...) and OrderByQuery: by the value of range field `key`,
    ascending unless `direction` says Direction.DESC; `start_from`: the first value to return
    (inclusive: the smallest when ascending, the largest when descending), a number for a
    number field, a datetime or RFC 3339 string for a datetime field."""
    key: str
    direction: Optional[Direction] = None
    start_from: Any = None


@dataclass
class OrderByQuery:
    """query_points(query=OrderByQuery(order_by=...)): the `limit` first points by the value of
    a range field (a field name or an OrderBy); every score is 0.0 and order_value is set."""
    order_by: Any


@dataclass
class FacetValueHit:
    value: Any
    count: int


@dataclass
class FacetResponse:
    hits: list = field(default_factory=list)


@dataclass
class QueryRequest:
    """Batched query entry for query_batch_points (one per request of a micro-batch); `query`
    is a vector or a NearestQuery, or with `prefetch` a FusionQuery / RrfQuery / FormulaQuery,
    or a RecommendQuery, or a SparseVector with `using` naming the collection's sparse vector.
    `lookup_from` exists to be refused where it is set."""
    query: Any
    filter: Optional[Filter] = None
    limit: int = 10
    with_payload: Any = True
    prefetch: Any = None
    using: Any = None
    lookup_from: Any = None
