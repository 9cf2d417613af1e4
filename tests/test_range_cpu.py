"""CPU tests of range and datetime filters (ragmi.filters): the key encoding,
the typing of payload values, the compiler (bounds, reductions, refusals), the packed blob and
its numpy restatement against a plain evaluator that never sees a key (_range_ref), and the
routing of keys through Collection.upsert / add_range_field / ragmi.store over a stand-in
index that records its calls."""
import datetime as dt
import json
import math
import os
import sys

import numpy as np
import pytest

import _stubs as S
from _range_ref import matches_range

TICKERS = ["AAPL", "MSFT", "AMD", "NVDA"]
TYPES = ["10-K", "10-Q", "8-K"]
KINDS = {"fiscal_year": "number", "ingested_at": "datetime", "revenue": "number",
         "pages": "number"}
UTC = dt.timezone.utc
DBL_MAX = sys.float_info.max
DENORM = 5e-324


def fc(key, **kw):
    from ragmi import qdrant_models as m
    return m.FieldCondition(key=key, **kw)


def ranges(kinds=None):
    from ragmi.filters import PayloadRanges
    return PayloadRanges(KINDS if kinds is None else kinds)


def tags_of(payloads=()):
    from ragmi.qdrant import PayloadTags
    t = PayloadTags(("ticker", "document_type"))
    for tk in TICKERS:
        for ty in TYPES:
            t.tag({"ticker": tk, "document_type": ty})
    return t


# ------------------------------------------------------------------ 1. the key
def test_keys_are_strictly_increasing_over_sorted_doubles():
    from ragmi.filters import KEY_ABSENT, key_of_float
    xs = [-math.inf, -DBL_MAX, np.nextafter(-DBL_MAX, 0), -1e300, -2.0 ** 53 - 2, -2.0 ** 53,
          -1.0, np.nextafter(-1.0, 0), -2.2250738585072014e-308, -2 * DENORM, -DENORM, 0.0,
          DENORM, 2 * DENORM, 2.2250738585072014e-308, np.nextafter(1.0, 0), 1.0,
          np.nextafter(1.0, 2), 2.0 ** 53, 2.0 ** 53 + 2, 1e300, DBL_MAX, math.inf]
    assert xs == sorted(xs) and len(set(xs)) == len(xs)
    keys = [key_of_float(x) for x in xs]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    assert all(-(1 << 63) < k < (1 << 63) for k in keys) and KEY_ABSENT not in keys
    assert KEY_ABSENT == -(1 << 63)
    assert key_of_float(-0.0) == key_of_float(0.0) == 0
    assert key_of_float(-math.inf) & ((1 << 64) - 1) == 0x800FFFFFFFFFFFFF
    assert key_of_float(np.float32(1.5)) == key_of_float(1.5) == key_of_float(np.float64(1.5))
    with pytest.raises(ValueError):
        key_of_float(math.nan)
    # the rule itself, restated: b if b >= 0 else b ^ 0x7FFF...
    bits = np.array(xs, np.float64).view(np.int64)
    want = np.where(bits >= 0, bits, bits ^ np.int64(0x7FFFFFFFFFFFFFFF))
    assert keys == want.tolist()


def test_value_typing_numbers():
    from ragmi.filters import KEY_ABSENT, key_of_float
    r = ranges()
    for v in (True, False, np.bool_(True), "2021", None, [2021], {"y": 2021}, math.nan,
              np.float64("nan")):
        assert r.key_of("fiscal_year", v) == KEY_ABSENT, v
    for v, x in ((2021, 2021.0), (np.int64(-3), -3.0), (np.float32(0.25), 0.25), (1e-3, 1e-3),
                 (2 ** 53 + 1, float(2 ** 53 + 1)), (-math.inf, -math.inf), (10 ** 400, math.inf)):
        assert r.key_of("fiscal_year", v) == key_of_float(x), v
    assert r.key_of("fiscal_year", 2 ** 53 + 1) == r.key_of("fiscal_year", 2 ** 53)   # rounds
    assert r.keys({"fiscal_year": 2020, "pages": "x"}) == [key_of_float(2020.0), KEY_ABSENT,
                                                          KEY_ABSENT, KEY_ABSENT]
    assert r.keys(None) == [KEY_ABSENT] * 4
    assert r.fields == tuple(KINDS) and r.kinds == tuple(KINDS.values())
    assert ranges(["a", "b"]).kinds == ("number", "number")
    with pytest.raises(ValueError):
        ranges(["a", "b", "c", "d", "e"])
    with pytest.raises(ValueError):
        ranges({"a": "keyword"})


def test_value_typing_datetimes():
    from ragmi.filters import KEY_ABSENT, datetime_micros, key_of_float
    r = ranges()
    day = 86_400_000_000
    us = 19723 * day                                     # 2024-01-01T00:00:00Z
    assert dt.datetime(2024, 1, 1, tzinfo=UTC) - dt.datetime(1970, 1, 1, tzinfo=UTC) == \
        dt.timedelta(microseconds=us)
    cases = {"2024-01-01T00:00:00Z": us, "2024-01-01T05:30:00+05:30": us,
             "2023-12-31T19:00:00-05:00": us, "2024-01-01T00:00:00": us, "2024-01-01": us,
             "2024-01-01 00:00:00.000000+00:00": us, "2024-01-01T00:00:00.5Z": us + 500_000,
             "2024-01-01T00:00:00.123456789Z": us + 123_456, "2024-01-01T12:00Z": us + day // 2,
             "1969-12-31T23:59:59.999999Z": -1}
    for s, want in cases.items():
        assert datetime_micros(s) == want, s
        assert r.key_of("ingested_at", s) == key_of_float(float(want)), s
    assert datetime_micros(dt.datetime(2024, 1, 1)) == us                       # naive: UTC
    assert datetime_micros(dt.datetime(2024, 1, 1, 5, 30, tzinfo=dt.timezone(
        dt.timedelta(hours=5, minutes=30)))) == us
    assert datetime_micros(dt.date(2024, 1, 1)) == us
    assert datetime_micros(dt.datetime(2024, 1, 1, 0, 0, 0, 7, tzinfo=UTC)) == us + 7
    # far from the epoch, where timestamp() would round: integer arithmetic is exact
    assert datetime_micros("2255-06-05T04:03:02.000001Z") % 1_000_000 == 1
    for bad in ("yesterday", "2024-13-01", "2024-01-01T25:00:00Z", "", 20240101, 1.5, None,
                ["2024-01-01"], True):
        assert r.key_of("ingested_at", bad) == KEY_ABSENT, bad
    assert r.key_of("fiscal_year", "2024-01-01") == KEY_ABSENT      # a string on a number field


# ------------------------------------------------------------------ 2. compile
def one_atom(flt, r=None):
    from ragmi.filters import compile_program
    p = compile_program(tags_of(), flt, r or ranges())
    return p


def test_bounds_inclusive_and_exclusive():
    from ragmi import qdrant_models as m
    r = ranges()
    stored = [2019, 2020, 2021.0, 2021.5, 2022, 2023, None]
    keys = [r.keys({"fiscal_year": v}) for v in stored]
    for rng, want in [
            (m.Range(gt=2021), [2021.5, 2022, 2023]), (m.Range(gte=2021), [2021.0, 2021.5, 2022, 2023]),
            (m.Range(lt=2021), [2019, 2020]), (m.Range(lte=2021), [2019, 2020, 2021.0]),
            (m.Range(gte=2020, lte=2022), [2020, 2021.0, 2021.5, 2022]),
            (m.Range(gt=2020, lt=2022), [2021.0, 2021.5]),
            (m.Range(gt=2020, gte=2021.5, lt=2023, lte=2023), [2021.5, 2022]),
            (m.Range(gte=2021, lte=2021), [2021.0]), (m.Range(), stored[:-1]),
            ({"gte": 2022}, [2022, 2023]), ({"gt": 2019, "lte": 2020}, [2020]),
            (m.Range(gte=-math.inf, lte=math.inf), stored[:-1])]:
        flt = m.Filter(must=[fc("fiscal_year", range=rng)])
        p = one_atom(flt, r)
        got = [v for v, k in zip(stored, keys) if p.passes(0, k)]
        assert got == want, rng
        assert got == [v for v in stored if matches_range(flt, {"fiscal_year": v}, KINDS)]
    # datetimes: a bound equal to a stored instant, spelled differently
    flt = m.Filter(must=[fc("ingested_at", range=m.DatetimeRange(
        gte="2024-01-01T00:00:00Z", lt=dt.datetime(2024, 1, 2, tzinfo=UTC)))])
    p = one_atom(flt, r)
    for s, want in (("2024-01-01", True), ("2023-12-31T23:59:59.999999Z", False),
                    ("2024-01-02T05:30:00+05:30", False), ("2024-01-01T23:59:59.999999", True)):
        assert p.passes(0, r.keys({"ingested_at": s})) is want, s
        assert matches_range(flt, {"ingested_at": s}, KINDS) is want


def test_empty_interval_reduces():
    from ragmi import qdrant_models as m
    from ragmi.filters import compile_filter, compile_program
    r, t = ranges(), tags_of()
    for rng in (m.Range(gt=5, lt=5), m.Range(gte=6, lte=5), m.Range(gt=5, lte=5),
                m.Range(gt=1.0, lt=float(np.nextafter(1.0, 2)))):
        assert compile_program(t, m.Filter(must=[fc("pages", range=rng)]), r) is None
        assert compile_filter(t, m.Filter(must=[fc("pages", range=rng)]), r) is None
        assert compile_program(t, m.Filter(must_not=[fc("pages", range=rng)]), r) == (0, 0)
    assert compile_program(t, m.Filter(must=[fc("pages", range=m.Range(gte=1.0, lte=1.0))]), r)
    # beyond the infinities lie only keys no double has: an interval, but nothing inside it
    for rng in (m.Range(gt=math.inf), m.Range(lt=-math.inf)):
        p = compile_program(t, m.Filter(must=[fc("pages", range=rng)]), r)
        assert not any(p.passes(0, r.keys({"pages": v})) for v in (-math.inf, 0, math.inf, None))


def test_range_atoms_in_the_algebra():
    from ragmi import qdrant_models as m
    from ragmi.filters import KEY_MAX, KEY_MIN, MAX_ATOMS, UnsupportedFilter, compile_program
    r, t = ranges(), tags_of()
    year = lambda **kw: fc("fiscal_year", range=m.Range(**kw))
    # must_not passes absent rows; is-empty is the negation of the full interval
    p = compile_program(t, m.Filter(must_not=[year(gte=2021)]), r)
    assert p.passes(0, r.keys({})) and p.passes(0, r.keys({"fiscal_year": 2020}))
    assert not p.passes(0, r.keys({"fiscal_year": 2021}))
    e = compile_program(t, m.Filter(must=[m.IsEmptyCondition(m.PayloadField("fiscal_year"))]), r)
    assert e.atoms == (("range", 0, KEY_MIN, KEY_MAX),) and e.table == 0b01
    assert e.passes(0, r.keys({"fiscal_year": "x"})) and not e.passes(0, r.keys({"fiscal_year": -1}))
    # equal atoms are shared, and range atoms count towards the limit
    two = compile_program(t, m.Filter(should=[year(gte=2021), m.Filter(must=[
        year(gte=2021.0), fc("ticker", match=m.MatchValue("AMD"))])]), r)
    assert [a[0] for a in two.atoms] == ["range", "maskeq"]     # 2021 and 2021.0: one atom
    distinct = [year(gte=2000 + i) for i in range(MAX_ATOMS)]
    assert len(compile_program(t, m.Filter(should=distinct), r).atoms) == MAX_ATOMS
    with pytest.raises(UnsupportedFilter, match="9 distinct atoms"):
        compile_program(t, m.Filter(should=distinct + [fc("ticker", match=m.MatchValue("AMD"))]), r)
    # mixed with tag atoms under should / must_not / min_should / nesting
    flt = m.Filter(
        must=[fc("ticker", match=m.MatchAny(any=["AMD", "NVDA"]))],
        should=[year(gte=2022), m.Filter(must=[year(lt=2020), fc("document_type", match=m.MatchValue("10-K"))])],
        must_not=[fc("ingested_at", range=m.DatetimeRange(lt="2020-01-01"))],
        min_should=m.MinShould([year(gte=2023), fc("pages", range={"gt": 10}),
                                m.IsEmptyCondition(m.PayloadField("revenue"))], 2))
    p = compile_program(t, flt, r)
    n = 0
    for tk in TICKERS + [None]:
        for ty in TYPES:
            for y in (2019, 2022, 2023, None):
                for at in ("2019-06-01", "2021-01-01T00:00:00Z", None):
                    for pages, rev in ((5, 1.0), (11, None), (None, None), (12, 3e9)):
                        pay = {k: v for k, v in dict(ticker=tk, document_type=ty, fiscal_year=y,
                                                     ingested_at=at, pages=pages, revenue=rev).items()
                               if v is not None}
                        want = matches_range(flt, pay, KINDS)
                        assert p.passes(t.tag(pay), r.keys(pay)) is want, pay
                        n += want
    assert 0 < n < 100


def test_refusals_name_the_cause():
    from ragmi import qdrant_models as m
    from ragmi.filters import (UnsupportedFilter, compile_filter, compile_legacy_only,
                               compile_program)
    r, t = ranges(), tags_of()
    bad = {
        r"range.*'ticker'.*keyword": fc("ticker", range={"gte": 1}),
        r"range.*'text'.*not a declared range field": fc("text", range=m.Range(gte=1)),
        r"range.*'ingested_at'.*Range on a datetime field": fc("ingested_at", range=m.Range(gte=1)),
        r"range.*'pages'.*DatetimeRange on a number field":
            fc("pages", range=m.DatetimeRange(gte="2024-01-01")),
        r"'pages' has both `match` and `range`": fc("pages", match=m.MatchValue(3), range=m.Range(gte=1)),
        r"range.*'pages'.*gte=nan": fc("pages", range=m.Range(gte=math.nan)),
        r"range.*'pages'.*lt='7'": fc("pages", range={"lt": "7"}),
        r"range.*'pages'.*gt=True": fc("pages", range=m.Range(gt=True)),
        r"range.*'ingested_at'.*lte='soon'": fc("ingested_at", range=m.DatetimeRange(lte="soon")),
        r"range.*'ingested_at'.*gte=17": fc("ingested_at", range={"gte": 17}),
        r"range.*'pages'.*unknown keys \['from'\]": fc("pages", range={"from": 1}),
        r"range.*'pages'.*got int": fc("pages", range=7),
        r"'pages' is not an indexed keyword field": fc("pages", match=m.MatchValue(3)),
    }
    for pattern, cond in bad.items():
        for flt in (m.Filter(must=[cond]), m.Filter(should=[m.Filter(must_not=[cond])])):
            with pytest.raises(UnsupportedFilter, match=pattern):
                compile_program(t, flt, r)
            with pytest.raises(UnsupportedFilter, match=pattern):
                compile_filter(t, flt, r)
    # without a codebook every range is refused, naming the key (the call of older code)
    with pytest.raises(UnsupportedFilter, match="range.*'pages'"):
        compile_program(t, m.Filter(must=[fc("pages", range=m.Range(gte=1))]))
    # delete stays legacy-only: a valid range is refused by the route's message
    with pytest.raises(UnsupportedFilter, match="Collection.delete takes only"):
        compile_legacy_only(t, m.Filter(must=[fc("pages", range=m.Range(gte=1))]),
                            "Collection.delete", r)


# ------------------------------------------------------------------ 3. restatement
def random_payload(rng):
    pay = {}
    if rng.random() < 0.9:
        pay["ticker"] = TICKERS[rng.integers(0, 4)]
    if rng.random() < 0.9:
        pay["document_type"] = TYPES[rng.integers(0, 3)]
    u = rng.random()
    if u < 0.6:
        pay["fiscal_year"] = int(rng.integers(2018, 2026))
    elif u < 0.75:
        pay["fiscal_year"] = float(rng.integers(2018, 2026)) + 0.5
    elif u < 0.8:
        pay["fiscal_year"] = [None, "FY21", [2021], True][rng.integers(0, 4)]
    if rng.random() < 0.8:
        d = dt.datetime(2023, 1, 1, tzinfo=UTC) + dt.timedelta(hours=int(rng.integers(0, 2 * 8760)))
        form = rng.integers(0, 4)
        pay["ingested_at"] = [d.isoformat(), d.strftime("%Y-%m-%dT%H:%M:%SZ"),
                              d.astimezone(dt.timezone(dt.timedelta(hours=-7))).isoformat(),
                              d.date().isoformat()][form]
    if rng.random() < 0.7:
        pay["revenue"] = float(rng.choice([-2.5e9, -1.0, -0.0, 0.0, 1e-9, 1.0, 3.25e9, 1e12]))
    if rng.random() < 0.7:
        pay["pages"] = int(rng.integers(-3, 40))
    return pay


def random_range_condition(rng):
    from ragmi import qdrant_models as m
    key = list(KINDS)[rng.integers(0, 4)]
    names = [n for n in ("gt", "gte", "lt", "lte") if rng.random() < 0.45]
    if KINDS[key] == "datetime":
        vals = ["2023-07-01", "2024-01-01T00:00:00Z", "2024-06-30T12:00:00+02:00",
                dt.datetime(2023, 3, 1, 6, tzinfo=UTC)]
        rng_obj = m.DatetimeRange(**{n: vals[rng.integers(0, 4)] for n in names})
    else:
        vals = {"fiscal_year": [2019, 2021, 2021.5, 2024], "revenue": [-1.0, 0.0, -0.0, 1.0, 3.25e9],
                "pages": [-1, 0, 10, 25.5]}[key]
        rng_obj = m.Range(**{n: vals[rng.integers(0, len(vals))] for n in names})
        if rng.random() < 0.3:
            rng_obj = {n: getattr(rng_obj, n) for n in names}
    return fc(key, range=rng_obj)


def random_cond(rng, depth=0):
    from ragmi import qdrant_models as m
    u = rng.random()
    if u < 0.45:
        return random_range_condition(rng)
    if u < 0.55:
        return m.IsEmptyCondition(m.PayloadField(list(KINDS)[rng.integers(0, 4)]))
    if u < 0.7:
        return fc("ticker", match=m.MatchAny(any=[TICKERS[i] for i in rng.choice(4, 2, replace=False)]))
    if u < 0.85 or depth >= 2:
        return fc("document_type", match=m.MatchValue(TYPES[rng.integers(0, 3)]))
    return random_filter(rng, depth + 1)


def random_filter(rng, depth=0):
    from ragmi import qdrant_models as m
    conds = lambda hi: [random_cond(rng, depth) for _ in range(rng.integers(0, hi))]
    ms = m.MinShould(conds(4), int(rng.integers(1, 3))) if rng.random() < 0.25 else None
    return m.Filter(must=conds(3) or None, should=conds(3) or None, must_not=conds(2) or None,
                    min_should=ms)


def restatement_case():
    from ragmi.filters import FilterProgram, UnsupportedFilter, compile_program
    rng = np.random.default_rng(20240101)
    pays = [random_payload(rng) for _ in range(500)]
    pays[0], pays[1] = {}, {"fiscal_year": 2021, "pages": 10, "revenue": 0.0,
                            "ingested_at": "2024-01-01"}      # boundary-equal values
    t, r = tags_of(), ranges()
    flts, progs = [], []
    while len(progs) < 40:
        f = random_filter(rng)
        try:
            p = compile_program(t, f, r)
        except UnsupportedFilter:           # more than 8 atoms
            continue
        if isinstance(p, FilterProgram):
            flts.append(f)
            progs.append(p)
    tags = np.array([t.tag(p) for p in pays], np.uint32)
    keys = np.array([r.keys(p) for p in pays], np.int64).T.copy()       # [n_cols, N]
    return pays, flts, progs, tags, keys


def test_programs_and_blob_equal_the_plain_evaluator():
    from ragmi.filters import MAX_PROGRAMS, eval_view_np, pack_view, view_programs
    pays, flts, progs, tags, keys = restatement_case()
    want = np.array([[matches_range(f, p, KINDS) for p in pays] for f in flts])
    assert want.any(axis=1).sum() > 30 and (~want).any(axis=1).all()
    assert any(a[0] == "range" for p in progs for a in p.atoms)
    for f, p, w in zip(flts, progs, want):
        got = np.array([p.passes(int(t), keys[:, i]) for i, t in enumerate(tags)])
        np.testing.assert_array_equal(got, w, err_msg=repr(f))
    for lo in range(0, len(progs), MAX_PROGRAMS):
        chunk = progs[lo:lo + MAX_PROGRAMS]
        blob = pack_view(chunk)
        assert view_programs(blob) == len(chunk)
        view = eval_view_np(blob, tags, keys=keys)
        for s in range(len(chunk)):
            np.testing.assert_array_equal((view >> np.uint32(s)) & 1, want[lo + s])
        np.testing.assert_array_equal(view, eval_view_np(blob, tags, len(chunk), keys=keys))


def test_blob_layout_and_guards():
    from ragmi.filters import (ATOM_RANGE, KEY_ABSENT, REC_WORDS, FilterProgram, eval_view_np,
                               key_of_float, pack_view, view_programs)
    k = key_of_float
    a = ("range", 1, k(-2.0), k(3.0))
    b = ("range", 3, k(0.0), k(0.0))
    progs = [FilterProgram((a,), 0b10), FilterProgram((b, a), 0b0110), FilterProgram((a,), 0b01)]
    blob = pack_view(progs)
    # the only pool entries are bounds: two distinct intervals, 4 words each, stored once
    assert len(blob) == 3 * REC_WORDS + 8 and view_programs(blob) == 3
    assert blob[9:13].tolist() == [ATOM_RANGE, 1, 3 * REC_WORDS, 0]
    assert blob[REC_WORDS + 9:REC_WORDS + 17].tolist() == [ATOM_RANGE, 3, 3 * REC_WORDS + 4, 0,
                                                           ATOM_RANGE, 1, 3 * REC_WORDS, 0]
    lo, hi = blob[3 * REC_WORDS:3 * REC_WORDS + 4].view(np.int64)
    assert (lo, hi) == (k(-2.0), k(3.0)) and lo < 0 < hi
    assert view_programs(pack_view(progs[:1])) == 1
    keys = np.full((4, 6), KEY_ABSENT, np.int64)
    keys[1] = [k(-2.0), k(3.0), k(3.5), k(-2.5), KEY_ABSENT, k(0.0)]
    keys[3] = [k(0.0), k(-0.0), k(1.0), KEY_ABSENT, k(0.0), k(5e-324)]
    tags = np.zeros(6, np.uint32)
    view = eval_view_np(blob, tags, keys=keys)
    assert (view & 1).tolist() == [1, 1, 0, 0, 0, 1]
    assert ((view >> 1) & 1).tolist() == [0, 0, 0, 0, 1, 1]          # xor of b and a
    assert ((view >> 2) & 1).tolist() == [0, 0, 1, 1, 1, 0]          # not a: absent passes
    # guard 1: a column at or past n_cols is false, nothing read
    np.testing.assert_array_equal(eval_view_np(blob, tags, keys=keys[:2]) & 1, view & 1)
    assert ((eval_view_np(blob, tags, keys=keys[:2]) >> 1) & 1).tolist() == (view & 1).tolist()
    assert not (eval_view_np(blob, tags, keys=keys[:1]) & 1).any()
    bad = blob.copy()
    bad[10] = 4                                   # program 0's column: RAG_KEYS_MAX_COLS
    assert not (eval_view_np(bad, tags, 3, keys=keys) & 1).any()
    bad[10] = 0xFFFFFFFF
    assert not (eval_view_np(bad, tags, 3, keys=keys) & 1).any()
    # guard 2: bounds ending past the blob are false; the last offset that fits is read
    for off, fits in ((len(blob) - 4, True), (len(blob) - 3, False), (len(blob), False),
                      (0xFFFFFFFF, False), (0xFFFFFFFD, False)):
        bad = blob.copy()
        bad[11] = off
        got = eval_view_np(bad, tags, 3, keys=keys) & 1
        assert got.any() == fits, off
    # without columns the restatement is the kernel that knows no RANGE atom (kind 2 = MASKEQ)
    assert eval_view_np(blob, tags, 3).shape == tags.shape


def test_abi_is_declared_and_bound():
    import re

    from conftest import ROOT
    from ragmi import _lib, filters
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    for name in ("rag_index_keys_create", "rag_index_keys_cols", "rag_index_write_keys",
                 "rag_index_gather_keys"):
        assert name in _lib.INDEX_API
        decl = re.search(rf"int {name}\(([^;]*)\);", hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.INDEX_API[name][1]), name
    assert re.search(r"#define RAG_FILTER_ATOM_RANGE (\d+)", hdr).group(1) == str(filters.ATOM_RANGE)
    assert re.search(r"#define RAG_KEYS_MAX_COLS (\d+)", hdr).group(1) == str(filters.KEYS_MAX_COLS)
    assert "#define RAG_KEY_ABSENT INT64_MIN" in hdr and filters.KEY_ABSENT == -(1 << 63)
    assert re.search(r"#define RAG_FILTER_REC_WORDS (\d+)", hdr).group(1) == str(filters.REC_WORDS)


# ------------------------------------------------------------------ 4. routing over a stand-in
class _RecIndex:
    """Index stand-in (the `index=` protocol) that keeps tags and key columns in numpy and
    records every call of the key methods."""
    device = None
    storage = "fp16"
    rescued = 0

    def __init__(self, dim=2, capacity=16, device=None, storage="fp16"):
        self.dim = dim
        self.rows = np.zeros((capacity, dim), np.uint16)
        self.tag = np.zeros(capacity, np.uint32)
        self.cols = []
        self.count = 0
        self.calls = []

    @property
    def capacity(self):
        return len(self.tag)

    def reserve(self, cap):
        from ragmi.filters import KEY_ABSENT
        if cap > self.capacity:
            grow = cap - self.capacity
            self.rows = np.concatenate([self.rows, np.zeros((grow, self.dim), np.uint16)])
            self.tag = np.concatenate([self.tag, np.zeros(grow, np.uint32)])
            self.cols = [np.concatenate([c, np.full(grow, KEY_ABSENT, np.int64)]) for c in self.cols]

    def upsert(self, vectors, rows, tags=None, new_count=None):
        self.tag[rows] = tags
        self.rows[rows, 0] = 0x3C00                       # (1, 0, ...): a unit row
        self.count = new_count

    def keys_create(self, n):
        from ragmi.filters import KEY_ABSENT
        self.calls.append(("keys_create", n))
        while len(self.cols) < n:
            self.cols.append(np.full(self.capacity, KEY_ABSENT, np.int64))

    def keys_cols(self):
        return len(self.cols)

    def write_keys(self, col, rows, keys):
        self.calls.append(("write_keys", col, np.asarray(rows).tolist(), np.asarray(keys).tolist()))
        self.cols[col][np.asarray(rows)] = np.asarray(keys, np.int64)

    def gather_keys(self, col, rows):
        self.calls.append(("gather_keys", col))
        return self.cols[col][np.asarray(rows)]

    def select_rows_view(self, programs, cap=None):
        from ragmi.filters import eval_view_np
        keys = np.array([c[:self.count] for c in self.cols]) if self.cols else None
        return None, int((eval_view_np(programs, self.tag[:self.count], 1, keys=keys) & 1).sum())

    def export_rows(self, row0=0, n=None):
        return self.rows[row0:row0 + n].copy()

    def export_tags(self, row0=0, n=None):
        return self.tag[row0:row0 + n].copy()

    def import_rows(self, a, row0=0, tags=None, new_count=None):
        a = np.asarray(a)
        self.rows[row0:row0 + len(a)] = a.view(np.uint16) if a.dtype == np.float16 else a
        self.tag[row0:row0 + len(a)] = tags
        self.count = new_count

    def close(self):
        pass


class _NoStream:
    def synchronize(self):
        pass


@pytest.fixture
def no_stream(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _NoStream())


def key_calls(idx, name="write_keys"):
    return [c for c in idx.calls if c[0] == name]


def test_upsert_writes_every_column_of_every_row(no_stream):
    from ragmi.collection import Collection
    from ragmi.filters import KEY_ABSENT, key_of_float
    idx = _RecIndex()
    col = Collection("t", 2, None, index=idx,
                     range_fields={"fiscal_year": "number", "ingested_at": "datetime"})
    assert idx.calls == [("keys_create", 2)] and col.ranges.fields == ("fiscal_year", "ingested_at")
    v = np.ones((3, 2), np.float32)
    col.upsert([10, 11, 12], v, [{"fiscal_year": 2021, "ingested_at": "2024-01-01"},
                                 {"ticker": "AMD"}, {"fiscal_year": 2023.5}])
    us = 19723 * 86_400_000_000
    assert key_calls(idx) == [
        ("write_keys", 0, [0, 1, 2], [key_of_float(2021.0), KEY_ABSENT, key_of_float(2023.5)]),
        ("write_keys", 1, [0, 1, 2], [key_of_float(float(us)), KEY_ABSENT, KEY_ABSENT])]
    # an overwrite without the field writes ABSENT; a duplicate id in a batch: the last wins
    idx.calls.clear()
    col.upsert([10, 12, 12], v, [{"ingested_at": "2024-01-01"}, {"fiscal_year": 1}, {"fiscal_year": 2}])
    assert key_calls(idx) == [
        ("write_keys", 0, [0, 2], [KEY_ABSENT, key_of_float(2.0)]),
        ("write_keys", 1, [0, 2], [key_of_float(float(us)), KEY_ABSENT])]
    # growth past the capacity: the columns follow, and new rows get every column
    idx.calls.clear()
    col.upsert(list(range(100, 130)), np.ones((30, 2), np.float32), [{"fiscal_year": i} for i in range(30)])
    assert idx.capacity >= 33 and all(len(c) == idx.capacity for c in idx.cols)
    assert [len(c[2]) for c in key_calls(idx)] == [30, 30]
    from ragmi import qdrant_models as m
    flt = m.Filter(must=[fc("fiscal_year", range=m.Range(gte=2, lt=10))])
    assert col.count_matching(flt) == sum(matches_range(flt, p, {"fiscal_year": "number"})
                                          for p in col.payloads) == 9
    with pytest.raises(ValueError, match="not both"):
        Collection("t", 2, None, index=_RecIndex(), range_fields=["ticker"])


def test_add_range_field_backfills(no_stream, monkeypatch):
    from ragmi import qdrant_models as m
    from ragmi.collection import Collection
    from ragmi.filters import KEY_ABSENT, UnsupportedFilter, key_of_float
    idx = _RecIndex()
    col = Collection("t", 2, None, index=idx)
    pays = [{"pages": i} if i % 3 else {"ticker": "AMD"} for i in range(10)]
    col.upsert(list(range(10)), np.ones((10, 2), np.float32), pays)
    assert idx.calls == []                                   # no range fields: no key call at all
    flt = m.Filter(must=[fc("pages", range=m.Range(gt=4))])
    with pytest.raises(UnsupportedFilter, match="range.*'pages'"):
        col.compile_filter(flt)
    monkeypatch.setattr(Collection, "BACKFILL_ROWS", 4)      # three chunks
    client, _ = S.stub_client(col)
    res = client.create_payload_index("t", "pages", m.PayloadSchemaType.INTEGER)
    assert res.status == m.UpdateStatus.COMPLETED
    assert idx.calls[0] == ("keys_create", 1)
    want = [key_of_float(float(i)) if i % 3 else KEY_ABSENT for i in range(10)]
    assert [c[2] for c in key_calls(idx)] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert sum((c[3] for c in key_calls(idx)), []) == want
    assert col.count_matching(flt) == 3                      # pages 5, 7 and 8
    n = len(idx.calls)
    client.create_payload_index("t", "pages", "integer")     # idempotent, also as a string
    client.create_payload_index("t", "pages", m.PayloadSchemaType.FLOAT)
    client.create_payload_index("t", "ticker", m.PayloadSchemaType.KEYWORD)       # a no-op
    assert len(idx.calls) == n
    with pytest.raises(ValueError, match="already a number field"):
        client.create_payload_index("t", "pages", m.PayloadSchemaType.DATETIME)
    with pytest.raises(ValueError, match="keyword tag field"):
        client.create_payload_index("t", "ticker", m.PayloadSchemaType.FLOAT)
    for schema in (m.PayloadSchemaType.BOOL, m.PayloadSchemaType.GEO, m.PayloadSchemaType.TEXT,
                   m.PayloadSchemaType.UUID, None):
        with pytest.raises(NotImplementedError):
            client.create_payload_index("t", "x", schema)
    with pytest.raises(NotImplementedError):
        client.create_payload_index("t", "source_file", m.PayloadSchemaType.KEYWORD)
    for f in ("a", "b", "c"):
        client.create_payload_index("t", f, m.PayloadSchemaType.DATETIME)
    with pytest.raises(ValueError, match="at most 4 range fields"):
        client.create_payload_index("t", "e", m.PayloadSchemaType.FLOAT)
    assert col.ranges.as_dict() == {"pages": "number", "a": "datetime", "b": "datetime",
                                    "c": "datetime"} and idx.keys_cols() == 4


def test_store_round_trips_range_fields(tmp_path, no_stream, monkeypatch):
    from ragmi import collection, store
    from ragmi.collection import Collection
    plain = Collection("p", 2, None, index=_RecIndex())
    plain.upsert([1, 2], np.ones((2, 2), np.float32), [{"ticker": "AMD"}, {"pages": 3}])
    store.save_collection(plain, str(tmp_path / "p"))
    cj = json.load(open(tmp_path / "p" / "collection.json"))
    assert sorted(cj) == ["codebooks", "dim", "distance", "name", "op", "storage", "tag_fields"]
    assert plain.index.calls == []

    col = Collection("r", 2, None, index=_RecIndex(),
                     range_fields={"pages": "number", "ingested_at": "datetime"})
    pays = [{"pages": i, "ingested_at": f"2024-01-{i + 1:02d}"} if i % 4 else {"ticker": "AMD"}
            for i in range(9)]
    col.upsert(list(range(9)), np.ones((9, 2), np.float32), pays)
    store.save_collection(col, str(tmp_path / "r"))
    cj = json.load(open(tmp_path / "r" / "collection.json"))
    assert cj["range_fields"] == [["pages", "number"], ["ingested_at", "datetime"]]
    monkeypatch.setattr(collection, "FlatIndex",
                        lambda dim, capacity, device, storage: _RecIndex(dim, capacity))
    back = store.load_collection(str(tmp_path / "r"))
    assert back.ranges.as_dict() == col.ranges.as_dict() and back.payloads == col.payloads
    assert back.index.calls[0] == ("keys_create", 2)
    for c in range(2):
        np.testing.assert_array_equal(back.index.cols[c][:9], col.index.cols[c][:9])
    again = store.load_collection(str(tmp_path / "p"))
    assert len(again.ranges) == 0 and again.index.calls == []


def test_retrieve_adds_the_datetime_range():
    from ragmi import qdrant_models as m
    from ragmi import rag
    f = rag._filter("amd", None, "2024-01-01", None)
    assert f.must[-1] == m.FieldCondition(key="ingested_at", range=m.DatetimeRange(
        gte="2024-01-01", lt=None))
    f = rag._filter("amd", "10-k", None, dt.date(2025, 1, 1))
    assert f.must[-1].range == m.DatetimeRange(lt=dt.date(2025, 1, 1)) and len(f.must) == 3
    assert len(rag._filter("amd", "10-k").must) == 2                 # today's call
