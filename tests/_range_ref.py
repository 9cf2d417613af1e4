"""The plain evaluator of the range tests: Qdrant's published filter rules walked over a payload
dict with range conditions compared as Python floats and timezone-aware datetimes. It never
sees a key and imports nothing from ragmi.filters: the independent check of the key encoding
(tests/test_range_cpu.py, test_range_gpu.py). Tag conditions go to _filters_ref.matches."""
import datetime as dt
import math

from _filters_ref import matches

UTC = dt.timezone.utc


def as_datetime(v):
    """A timezone-aware datetime, or None for what a datetime field holds no value for."""
    if isinstance(v, str):
        s = v.strip()
        if s[-1:] in "Zz":
            s = s[:-1] + "+00:00"
        try:
            v = dt.datetime.fromisoformat(s)
        except ValueError:
            return None
    elif isinstance(v, dt.date) and not isinstance(v, dt.datetime):
        v = dt.datetime(v.year, v.month, v.day)
    if not isinstance(v, dt.datetime):
        return None
    return v if v.tzinfo is not None else v.replace(tzinfo=UTC)


def as_number(v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return None
    v = float(v)
    return None if math.isnan(v) else v


def value_of(kind, v):
    return as_datetime(v) if kind == "datetime" else as_number(v)


def bounds_of(rng):
    get = rng.get if isinstance(rng, dict) else lambda k: getattr(rng, k)
    return {k: get(k) for k in ("gt", "gte", "lt", "lte") if get(k) is not None}


def in_range(kind, rng, v):
    x = value_of(kind, v)
    if x is None:
        return False
    for name, b in bounds_of(rng).items():
        b = value_of(kind, b)
        assert b is not None, (name, rng)
        if not {"gt": x > b, "gte": x >= b, "lt": x < b, "lte": x <= b}[name]:
            return False
    return True


def cond_matches(c, payload, kinds):
    from ragmi import qdrant_models as m
    if isinstance(c, m.Filter):
        return matches_range(c, payload, kinds)
    if isinstance(c, m.IsEmptyCondition) and c.is_empty.key in kinds:
        return value_of(kinds[c.is_empty.key], payload.get(c.is_empty.key)) is None
    if isinstance(c, m.FieldCondition) and c.range is not None:
        return in_range(kinds[c.key], c.range, payload.get(c.key))
    return matches(m.Filter(must=[c]), payload)           # a tag condition


def matches_range(flt, payload, kinds):
    """Whether `payload` passes Filter `flt`; `kinds`: range field -> "number" | "datetime"."""
    payload = payload or {}
    ok = lambda c: cond_matches(c, payload, kinds)
    if flt.must and not all(ok(c) for c in flt.must):
        return False
    if flt.should and not any(ok(c) for c in flt.should):
        return False
    if flt.must_not and any(ok(c) for c in flt.must_not):
        return False
    ms = flt.min_should
    if ms is not None and sum(ok(c) for c in ms.conditions) < ms.min_count:
        return False
    return True
