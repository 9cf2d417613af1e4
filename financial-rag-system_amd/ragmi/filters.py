"""Filter programs: Qdrant's filter algebra over the two tag fields and the collection's range
fields, compiled for the GPU.

`PayloadTags.compile` (below) knows one filter shape, Filter(must=[FieldCondition(key,
match=MatchValue)]), and turns it into one (mask, value) pair. Everything else the tag can
answer — `should`, `must_not`, `min_should`, MatchAny, MatchExcept, "is empty", nested filters —
is compiled here into a PROGRAM: at most MAX_ATOMS atoms and a 256-bit truth table over them.
filter_view_kernel (csrc/filter_kernels.hip) evaluates up to MAX_PROGRAMS programs against every
row's tag in one streaming launch and writes a derived tag column, bit s = "the row passes
program s"; the search then runs unchanged over that column with the ordinary per-query filter
(1 << s, 1 << s) (the blob layout is include/ragmi.h's "Filter programs").

Semantics (Qdrant's published filter rules; parity with a Qdrant server is unpinned, as for
search, MMR and groups). The tag holds one 16-bit code per field, 0 = absent; "present" means
code != 0. A point whose value is a list, a dict or None has code 0 (PayloadTags.code), so it
counts as absent: IsEmpty is true for it and no match condition is.

  Filter(must, should, must_not, min_should) matches iff
    every `must` condition matches, and
    `should` is empty / None or at least one `should` condition matches, and
    no `must_not` condition matches, and
    `min_should` is None or at least min_count of its conditions match.
  Filter() matches every point.

  FieldCondition(key, match=MatchValue(v))            present and equal to v
  FieldCondition(key, match=MatchAny(any=[...]))      present and in the list ([] matches nothing)
  FieldCondition(key, match=MatchExcept(except_=[]))  present and not in the list
  IsEmptyCondition(is_empty=PayloadField(key))        code == 0
  a nested Filter, to any depth

Range fields (PayloadRanges; Collection(range_fields=...), create_payload_index): up to
KEYS_MAX_COLS numeric payload fields, "number" or "datetime", each a device column of one int64
KEY per row beside the tag (include/ragmi.h "Key columns").

  FieldCondition(key, range=Range(gt, gte, lt, lte))          on a number field
  FieldCondition(key, range=DatetimeRange(gt, gte, lt, lte))  on a datetime field
  (or a dict with those four keys on either)                  present and inside every bound
  IsEmptyCondition on a range field                           no value

key(x) of a double x (key_of_float): -0.0 taken as +0.0, b = the IEEE-754 bits as int64,
key = b if b >= 0 else b ^ 0x7FFFFFFFFFFFFFFF. A signed compare of keys is the numeric compare of
the doubles; KEY_ABSENT = INT64_MIN is "no value" and no double maps to it. A number field takes
Python / numpy ints and floats as float(x): an int beyond 2^53 rounds to the nearest double, as
it does in Qdrant's float range, so integer compares are exact only up to 2^53. bool, str, None,
lists, dicts and NaN are absent — PayloadTags.code's "not a scalar, so absent" rule. A datetime
field takes an RFC 3339 / ISO-8601 string or a datetime / date object as integer microseconds
since 1970-01-01T00:00:00Z, then float (exact for +-285 years): a trailing Z, numeric offsets,
naive values read as UTC (as Qdrant reads them), date-only values read as midnight; a string
that does not parse is absent. A range becomes ONE closed key interval, lo = max(key(gte),
key(gt) + 1) or KEY_ABSENT + 1, hi = min(key(lte), key(lt) - 1) or INT64_MAX; lo > hi compiles to
False. An absent value is in no range, so a range under must_not passes absent rows, and
is-empty is the negation of the full-interval atom. As for the rest of the algebra, parity with
a Qdrant server is unpinned.

A value that was never ingested is in no set. Refused with UnsupportedFilter, which names the
cause: a `range` on a key that is not a declared range field (a tag field included), a Range on
a datetime field or a DatetimeRange on a number field, a condition with both `match` and
`range`, a bound that is NaN or does not parse; keys outside the collection's
payload_tag_fields, any other condition or match class (HasId, IsNull, geo, text), and a filter
that needs more than MAX_ATOMS distinct atoms (range atoms count).

Atoms:
  ("maskeq", mask, value)        (tag & mask) == value — the legacy filter form
  ("inset", f, bitmap, nbits)    code_f(tag) < nbits and bit code_f of `bitmap` is set, where
                                 code_f = (tag >> 16 f) & 0xFFFF and nbits = len(codebook_f) + 1
                                 at compile time: a code at or past it is not a member
  ("range", col, lo, hi)         key != KEY_ABSENT and lo <= key <= hi, key = the row's key of
                                 range field `col`
A row passes iff bit idx of the table is set, idx = sum_i atom_i(tag, keys) << i.

Host-only, numpy-only. eval_view_np restates the kernel for the tests; nothing in the product
calls it.
"""
from __future__ import annotations

import datetime as _dt
import itertools
import math
import re
import struct
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import qdrant_models as models

MAX_ATOMS = 8          # RAG_FILTER_MAX_ATOMS
MAX_PROGRAMS = 32      # RAG_FILTER_MAX_PROGRAMS
REC_WORDS = 41         # RAG_FILTER_REC_WORDS: atom count, 8 table words, 8 atoms of 4 words
ATOM_MASKEQ = 0        # RAG_FILTER_ATOM_MASKEQ
ATOM_INSET = 1         # RAG_FILTER_ATOM_INSET
ATOM_RANGE = 2         # RAG_FILTER_ATOM_RANGE
KEYS_MAX_COLS = 4      # RAG_KEYS_MAX_COLS
KEY_ABSENT = -(1 << 63)            # RAG_KEY_ABSENT
KEY_MIN, KEY_MAX = KEY_ABSENT + 1, (1 << 63) - 1   # the full interval: every present key


class UnsupportedFilter(NotImplementedError):
    pass


DEFAULT_TAG_FIELDS = ("ticker", "document_type")


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


# ------------------------------------------------------------------ range fields
def key_of_float(x: float) -> int:
    """The order-preserving int64 key of a finite or infinite double (module docstring)."""
    x = float(x)
    if math.isnan(x):
        raise ValueError("NaN has no key")
    if x == 0.0:
        x = 0.0                                  # -0.0 and +0.0 share a key
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b if b >= 0 else b ^ 0x7FFFFFFFFFFFFFFF


_ISO = re.compile(r"(\d{4})-(\d{2})-(\d{2})"
                  r"(?:[Tt ](\d{2}):(\d{2})(?::(\d{2})(?:[.,](\d{1,9}))?)?"
                  r"\s?(Z|z|[+-]\d{2}(?::?\d{2})?)?)?")
_EPOCH = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)


def datetime_micros(value) -> int | None:
    """Integer microseconds since 1970-01-01T00:00:00Z of an RFC 3339 / ISO-8601 string or a
    datetime / date object, by integer arithmetic; None for anything else and for a string that
    does not parse. Naive values are UTC, a date is its midnight; digits of a fraction past the
    microsecond are dropped."""
    if isinstance(value, str):
        m = _ISO.fullmatch(value.strip())
        if m is None:
            return None
        y, mo, d, H, M, S, frac, tz = m.groups()
        off = _dt.timedelta(0)
        if tz and tz not in "Zz":
            off = _dt.timedelta(hours=int(tz[1:3]), minutes=int(tz[-2:]) if len(tz) > 3 else 0)
            if tz[0] == "-":
                off = -off
        try:
            value = _dt.datetime(int(y), int(mo), int(d), int(H or 0), int(M or 0), int(S or 0),
                                 int((frac or "0")[:6].ljust(6, "0")),
                                 tzinfo=_dt.timezone.utc) - off
        except (ValueError, OverflowError):
            return None
    elif isinstance(value, _dt.datetime):
        if value.tzinfo is None:
            value = value.replace(tzinfo=_dt.timezone.utc)
    elif isinstance(value, _dt.date):
        value = _dt.datetime(value.year, value.month, value.day, tzinfo=_dt.timezone.utc)
    else:
        return None
    try:
        return (value - _EPOCH) // _dt.timedelta(microseconds=1)
    except OverflowError:
        return None


RANGE_KINDS = ("number", "datetime")


def _number(value) -> float | None:
    """float(value) of a Python / numpy int or float, None for anything else (bool included)
    and for NaN; an int past the doubles is the infinity of its sign."""
    if isinstance(value, (bool, np.bool_)) or \
            not isinstance(value, (int, float, np.integer, np.floating)):
        return None
    try:
        x = float(value)
    except OverflowError:
        x = math.inf if value > 0 else -math.inf
    return None if math.isnan(x) else x


class PayloadRanges:
    """The codebook of a collection's range fields: the fields in column order, the kind of
    each ("number" or "datetime"), and the key of a payload value. `fields`: a mapping of field
    to kind, or a sequence of names that all mean "number". Host-only."""

    def __init__(self, fields=None):
        self.fields: tuple = ()
        self.kinds: tuple = ()
        items = (fields.items() if hasattr(fields, "items") else
                 [(f, "number") for f in (fields or ())])
        for name, kind in items:
            self.add(name, kind)

    def __len__(self) -> int:
        return len(self.fields)

    def as_dict(self) -> dict:
        return dict(zip(self.fields, self.kinds))

    def add(self, name: str, kind: str) -> int:
        """Declare range field `name`; returns its column. Repeating a declaration is a no-op,
        another kind for a declared field or a field past KEYS_MAX_COLS a ValueError."""
        if kind not in RANGE_KINDS:
            raise ValueError(f"range field {name!r}: kind must be one of {RANGE_KINDS}")
        if name in self.fields:
            col = self.fields.index(name)
            if self.kinds[col] != kind:
                raise ValueError(f"range field {name!r} is already a {self.kinds[col]} field")
            return col
        if len(self.fields) >= KEYS_MAX_COLS:
            raise ValueError(f"at most {KEYS_MAX_COLS} range fields per collection "
                             f"(have {self.fields})")
        self.fields += (name,)
        self.kinds += (kind,)
        return len(self.fields) - 1

    def _value(self, col: int, value) -> float | None:
        if self.kinds[col] == "datetime":
            us = datetime_micros(value)
            return None if us is None else float(us)
        return _number(value)

    def key_of(self, field: str, value) -> int:
        """The key of payload value `value` of field `field`, KEY_ABSENT for a value the
        field's kind does not take (module docstring)."""
        x = self._value(self.fields.index(field), value)
        return KEY_ABSENT if x is None else key_of_float(x)

    def keys(self, payload: dict | None) -> list:
        """One key per column for a point's payload."""
        return [self.key_of(f, payload[f]) if payload and f in payload else KEY_ABSENT
                for f in self.fields]

    def interval(self, field: str, rng):
        """(col, lo, hi) of a Range / DatetimeRange / dict on declared field `field`: the one
        closed key interval; lo > hi when nothing can lie inside."""
        col = self.fields.index(field)
        kind = self.kinds[col]
        if isinstance(rng, dict):
            extra = set(rng) - {"lt", "gt", "gte", "lte"}
            if extra:
                raise UnsupportedFilter(f"`range` on {field!r}: unknown keys {sorted(extra)} "
                                        "(lt, gt, gte, lte are the bounds)")
            get = rng.get
        elif isinstance(rng, (models.Range, models.DatetimeRange)):
            given = "datetime" if isinstance(rng, models.DatetimeRange) else "number"
            if given != kind:
                raise UnsupportedFilter(
                    f"`range` on {field!r}: a {type(rng).__name__} on a {kind} field (Range goes "
                    "with number fields, DatetimeRange with datetime fields)")
            get = lambda k: getattr(rng, k)
        else:
            raise UnsupportedFilter(f"`range` on {field!r}: expected a Range, a DatetimeRange or "
                                    f"a dict, got {type(rng).__name__}")

        def bound(name):
            x = self._value(col, get(name))
            if x is None:
                raise UnsupportedFilter(
                    f"`range` on {field!r}: bound {name}={get(name)!r} is not a "
                    f"{'datetime that parses (RFC 3339)' if kind == 'datetime' else 'number'}")
            return key_of_float(x)

        lo, hi = KEY_MIN, KEY_MAX
        if get("gte") is not None:
            lo = max(lo, bound("gte"))
        if get("gt") is not None:
            lo = max(lo, bound("gt") + 1)
        if get("lte") is not None:
            hi = min(hi, bound("lte"))
        if get("lt") is not None:
            hi = min(hi, bound("lt") - 1)
        return col, lo, hi


@dataclass(frozen=True)
class FilterProgram:
    """atoms: a tuple of atom tuples (module docstring); table: the truth table as an int, bit
    idx set = assignment idx passes. Hashable: equal programs share a view bit."""
    atoms: tuple
    table: int

    @staticmethod
    def maskeq(mask: int, value: int) -> "FilterProgram":
        """The one-atom program of a legacy (mask, value) filter."""
        return FilterProgram((("maskeq", int(mask), int(value)),), 0b10)

    def passes(self, tag: int, keys=None) -> bool:
        """`keys`: the row's key per range column (PayloadRanges.keys); None = no columns."""
        idx = 0
        for i, a in enumerate(self.atoms):
            idx |= int(_atom(a, tag, keys)) << i
        return bool((self.table >> idx) & 1)


def _atom(a, tag: int, keys=None) -> bool:
    if a[0] == "maskeq":
        return (tag & a[1]) == a[2]
    if a[0] == "range":
        if keys is None or a[1] >= len(keys):
            return False
        k = int(keys[a[1]])
        return k != KEY_ABSENT and a[2] <= k <= a[3]
    code = (tag >> (16 * a[1])) & 0xFFFF
    return code < a[3] and bool((a[2] >> code) & 1)


# ------------------------------------------------------------------ compile
def _as_list(x) -> list:
    if x is None:
        return []
    return list(x) if isinstance(x, (list, tuple)) else [x]


class _Compiler:
    """Walks a Filter into an expression over atom indices: True / False, ("atom", i),
    ("not", e), ("and", [e]), ("or", [e]), ("atleast", n, [e])."""

    def __init__(self, tags, ranges=None):
        self.tags = tags
        self.ranges = ranges if ranges is not None else PayloadRanges()
        self.atoms: list = []

    def atom(self, a):
        if a not in self.atoms:
            self.atoms.append(a)
        return ("atom", self.atoms.index(a))

    def field(self, key) -> int:
        if key not in self.tags.fields:
            raise UnsupportedFilter(
                f"payload key {key!r} is not an indexed keyword field {self.tags.fields}; "
                "create the collection with payload_tag_fields")
        return self.tags.fields.index(key)

    def codes(self, f: int, values) -> int:
        """Bitmap of the known codes of `values` (a never-ingested value is in no set)."""
        bm = 0
        for v in values:
            c = self.tags.code(f, v, create=False)
            if c:
                bm |= 1 << c
        return bm

    def inset(self, f: int, bm: int):
        return self.atom(("inset", f, bm, len(self.tags.codes[f]) + 1)) if bm else False

    def condition(self, cond):
        if isinstance(cond, models.Filter):
            return self.filter(cond)
        if isinstance(cond, models.IsEmptyCondition):
            key = getattr(cond.is_empty, "key", cond.is_empty)
            if key in self.ranges.fields:       # no value: not inside the full interval
                col = self.ranges.fields.index(key)
                return ("not", self.atom(("range", col, KEY_MIN, KEY_MAX)))
            f = self.field(key)
            return self.atom(("maskeq", 0xFFFF << (16 * f), 0))
        if not isinstance(cond, models.FieldCondition):
            raise UnsupportedFilter(
                f"condition {type(cond).__name__} is not supported (FieldCondition with "
                "MatchValue / MatchAny / MatchExcept, IsEmptyCondition and nested Filters are)")
        if cond.range is not None:
            if cond.match is not None:
                raise UnsupportedFilter(f"condition on {cond.key!r} has both `match` and `range`; "
                                        "give one")
            if cond.key not in self.ranges.fields:
                what = ("a keyword tag field: the tag holds keyword codes, not numbers"
                        if cond.key in self.tags.fields else "not a declared range field")
                raise UnsupportedFilter(
                    f"`range` on {cond.key!r}: {what} (range fields: {self.ranges.fields}; "
                    "declare one with range_fields / create_payload_index)")
            col, lo, hi = self.ranges.interval(cond.key, cond.range)
            return self.atom(("range", col, lo, hi)) if lo <= hi else False
        f = self.field(cond.key)
        m = cond.match
        fmask = 0xFFFF << (16 * f)
        if isinstance(m, models.MatchValue):
            c = self.tags.code(f, m.value, create=False)
            return self.atom(("maskeq", fmask, c << (16 * f))) if c else False
        if isinstance(m, models.MatchAny):
            return self.inset(f, self.codes(f, _as_list(m.any)))
        if isinstance(m, models.MatchExcept):
            present = ("not", self.atom(("maskeq", fmask, 0)))
            listed = self.inset(f, self.codes(f, _as_list(m.except_)))
            return ("and", [present, ("not", listed)])
        raise UnsupportedFilter(f"match {type(m).__name__} on {cond.key!r} is not supported "
                                "(MatchValue, MatchAny and MatchExcept are)")

    def filter(self, flt):
        parts = [self.condition(c) for c in _as_list(flt.must)]
        should = [self.condition(c) for c in _as_list(flt.should)]
        if should:
            parts.append(("or", should))
        parts += [("not", self.condition(c)) for c in _as_list(flt.must_not)]
        ms = flt.min_should
        if ms is not None:
            if not hasattr(ms, "conditions") or not hasattr(ms, "min_count"):
                raise UnsupportedFilter("min_should must be a MinShould(conditions, min_count)")
            parts.append(("atleast", int(ms.min_count),
                          [self.condition(c) for c in _as_list(ms.conditions)]))
        return ("and", parts)


def _ev(e, idx: int) -> bool:
    if e is True or e is False:
        return e
    op = e[0]
    if op == "atom":
        return bool((idx >> e[1]) & 1)
    if op == "not":
        return not _ev(e[1], idx)
    if op == "and":
        return all(_ev(x, idx) for x in e[1])
    if op == "or":
        return any(_ev(x, idx) for x in e[1])
    return sum(_ev(x, idx) for x in e[2]) >= e[1]        # atleast


def compile_program(tags, flt, ranges=None):
    """A Filter over `tags` (a PayloadTags: .fields, .codes, .code) and `ranges` (a
    PayloadRanges; None = no range fields) -> FilterProgram, or (0, 0) when every point matches
    (also flt None), or None when nothing can."""
    if flt is None:
        return (0, 0)
    if not isinstance(flt, models.Filter):
        raise UnsupportedFilter(f"expected a Filter, got {type(flt).__name__}")
    c = _Compiler(tags, ranges)
    expr = c.filter(flt)
    m = len(c.atoms)
    if m > MAX_ATOMS:
        raise UnsupportedFilter(f"the filter needs {m} distinct atoms (conditions on the tag); "
                                f"a filter program holds at most {MAX_ATOMS}")
    table = 0
    for idx in range(1 << m):
        if _ev(expr, idx):
            table |= 1 << idx
    if table == 0:
        return None
    if table == (1 << (1 << m)) - 1:
        return (0, 0)
    return FilterProgram(tuple(c.atoms), table)


# ------------------------------------------------------------------ the two front ends
def compile_filter(tags, flt, ranges=None):
    """A Filter as the searches take it (`ranges`: the collection's PayloadRanges, None = no
    range fields; PayloadTags.compile refuses every range, so a filter with one goes to the
    general compiler): the (mask, value) pair of PayloadTags.compile for
    every filter it accepts (the legacy path, untouched), else a FilterProgram
    (compile_program: should, must_not, min_should, MatchAny, MatchExcept, is-empty, nested
    filters); None when nothing can match. A filter neither accepts is refused with the general
    compiler's message, which names the cause. A filter with `min_should` goes to the general
    compiler at once: PayloadTags.compile never looked at that clause."""
    if getattr(flt, "min_should", None) is not None:
        return compile_program(tags, flt, ranges)
    try:
        return tags.compile(flt)
    except UnsupportedFilter:
        return compile_program(tags, flt, ranges)


def compile_legacy_only(tags, flt, what: str, ranges=None):
    """PayloadTags.compile for a route (`what`) that takes no general filter yet: its refusal
    says that the route is the reason when the filter algebra would have accepted the filter."""
    try:
        if getattr(flt, "min_should", None) is not None:
            raise UnsupportedFilter("min_should is not a `must` condition")
        return tags.compile(flt)
    except UnsupportedFilter as e:
        compile_program(tags, flt, ranges)    # refused by both: the general message
        raise UnsupportedFilter(
            f"{what} takes only Filter(must=[FieldCondition(key, match=MatchValue)]); "
            f"general filters (should, must_not, MatchAny, ...) are out of scope here: {e}"
        ) from e


# ------------------------------------------------------------------ device blob
def pack_view(programs) -> np.ndarray:
    """The device blob of U <= MAX_PROGRAMS programs (uint32; include/ragmi.h "Filter
    programs"): U records of REC_WORDS words, then the pool: the INSET atoms' bitmaps and the
    RANGE atoms' bounds (4 words: lo low, lo high, hi low, hi high), each distinct one once."""
    programs = list(programs)
    if not 1 <= len(programs) <= MAX_PROGRAMS:
        raise ValueError(f"a view holds 1 to {MAX_PROGRAMS} programs")
    rec = np.zeros((len(programs), REC_WORDS), np.uint32)
    pool: list = []
    where: dict = {}
    base = len(programs) * REC_WORDS
    for s, p in enumerate(programs):
        if len(p.atoms) > MAX_ATOMS:
            raise ValueError(f"a program holds at most {MAX_ATOMS} atoms")
        rec[s, 0] = len(p.atoms)
        for w in range(8):
            rec[s, 1 + w] = (p.table >> (32 * w)) & 0xFFFFFFFF
        for i, a in enumerate(p.atoms):
            d = rec[s, 9 + 4 * i:13 + 4 * i]
            if a[0] == "maskeq":
                d[:] = (ATOM_MASKEQ, a[1] & 0xFFFFFFFF, a[2] & 0xFFFFFFFF, 0)
            elif a[0] == "range":
                _, col, lo, hi = a
                key = ("range", lo, hi)
                if key not in where:       # equal intervals are stored once
                    where[key] = base + len(pool)
                    pool += [lo & 0xFFFFFFFF, (lo >> 32) & 0xFFFFFFFF,
                             hi & 0xFFFFFFFF, (hi >> 32) & 0xFFFFFFFF]
                d[:] = (ATOM_RANGE, col, where[key], 0)
            else:
                _, f, bm, nbits = a
                key = (bm, nbits)
                if key not in where:       # equal bitmaps are stored once
                    where[key] = base + len(pool)
                    pool += [(bm >> (32 * w)) & 0xFFFFFFFF for w in range((nbits + 31) // 32)]
                d[:] = (ATOM_INSET, f, where[key], nbits)
    return np.concatenate([rec.reshape(-1), np.asarray(pool, np.uint32)]).astype(np.uint32)


def view_programs(blob) -> int:
    """How many programs a well-formed blob (pack_view's) holds: the records end where the
    pool begins, at the smallest INSET or RANGE offset, or at the blob's end without one."""
    blob = np.asarray(blob, np.uint32).reshape(-1)
    end, n = len(blob), 0
    while (n + 1) * REC_WORDS <= end:
        r = blob[n * REC_WORDS:(n + 1) * REC_WORDS]
        for i in range(min(int(r[0]), MAX_ATOMS)):
            if r[9 + 4 * i] in (ATOM_INSET, ATOM_RANGE):
                end = min(end, int(r[11 + 4 * i]))
        n += 1
    return n


def eval_view_np(blob, tags, n_programs: int | None = None, keys=None) -> np.ndarray:
    """filter_view_kernel restated in numpy: view[r] = sum_s pass_s(tags[r], keys[:, r]) << s.
    Follows the kernel's guards: atom counts clamped to MAX_ATOMS, a bitmap word outside the
    blob reads as "not a member", a RANGE atom whose column is >= n_cols or whose bounds end
    past the blob is false. `keys`: the key columns, int64 [n_cols, N]. None restates the
    kernel of an index WITHOUT columns, which knows no RANGE atom: kind 2 is then an unknown
    kind and reads as MASKEQ, like every unknown kind."""
    blob = np.asarray(blob, np.uint32).reshape(-1)
    t = np.asarray(tags, np.uint32).reshape(-1)
    if keys is not None:
        keys = np.asarray(keys, np.int64).reshape(-1, t.shape[0])
    U = view_programs(blob) if n_programs is None else int(n_programs)
    words = len(blob)
    out = np.zeros(t.shape, np.uint32)
    for s in range(U):
        r = blob[s * REC_WORDS:(s + 1) * REC_WORDS]
        idx = np.zeros(t.shape, np.uint32)
        for i in range(min(int(r[0]), MAX_ATOMS)):
            kind, p0, p1, p2 = (int(x) for x in r[9 + 4 * i:13 + 4 * i])
            if keys is not None and kind == ATOM_RANGE:
                a = np.zeros(t.shape, np.uint32)
                if p0 < keys.shape[0] and p1 + 3 < words:
                    lo, hi = (int(x) for x in blob[p1:p1 + 4].copy().view(np.int64))
                    k = keys[p0]
                    a = ((k != KEY_ABSENT) & (k >= lo) & (k <= hi)).astype(np.uint32)
            elif kind == ATOM_INSET:
                code = (t >> np.uint32(16 * (p0 & 1))) & np.uint32(0xFFFF)
                w = p1 + (code >> np.uint32(5)).astype(np.int64)
                ok = (code < p2) & (w < words)
                bits = np.where(ok, blob[np.where(ok, w, 0)], 0).astype(np.uint32)
                a = (bits >> (code & np.uint32(31))) & np.uint32(1)
            else:
                a = ((t & np.uint32(p0)) == np.uint32(p1)).astype(np.uint32)
            idx |= a << np.uint32(i)
        tw = r[1 + (idx >> np.uint32(5)).astype(np.int64)]
        out |= ((tw >> (idx & np.uint32(31))) & np.uint32(1)) << np.uint32(s)
    return out
