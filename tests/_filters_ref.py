"""The plain evaluator of the filter tests: Qdrant's published filter rules walked over a
payload dict, written without ragmi.filters (tests/test_filters_cpu.py, test_filters_gpu.py)."""


def absent(v):
    return v is None or isinstance(v, (list, dict))


def cond_matches(c, payload):
    from ragmi import qdrant_models as m
    if isinstance(c, m.Filter):
        return matches(c, payload)
    if isinstance(c, m.IsEmptyCondition):
        return absent(payload.get(c.is_empty.key))
    v = payload.get(c.key)
    if absent(v):
        return False
    if isinstance(c.match, m.MatchValue):
        return v == c.match.value
    if isinstance(c.match, m.MatchAny):
        return v in c.match.any
    if isinstance(c.match, m.MatchExcept):
        return v not in c.match.except_
    raise AssertionError(c)


def matches(flt, payload):
    if flt.must and not all(cond_matches(c, payload) for c in flt.must):
        return False
    if flt.should and not any(cond_matches(c, payload) for c in flt.should):
        return False
    if flt.must_not and any(cond_matches(c, payload) for c in flt.must_not):
        return False
    ms = flt.min_should
    if ms is not None and sum(cond_matches(c, payload) for c in ms.conditions) < ms.min_count:
        return False
    return True
