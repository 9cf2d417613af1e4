"""Formula programs: the expression tree of a FormulaQuery compiled for the GPU.

A formula re-scores the candidates of a request's prefetched lists. Its
expressions (ragmi.qdrant_models; Qdrant's published formula expressions, parity with a Qdrant
server's arithmetic unpinned):

  a Python / numpy number                       a constant
  "$score"                                      the candidate's score (one prefetch only)
  "$score[i]"                                   its exact score in prefetch i; absent from that
                                                list: defaults["$score[i]"]
  any other str                                 the value of a number range field
  DatetimeKeyExpression(datetime_key=field)     a datetime range field, seconds since the epoch:
                                                the stored microseconds as a double / 1e6
  DatetimeExpression(datetime=...)              a constant time, converted the same way here
  FieldCondition / IsEmptyCondition / Filter    1.0 when the candidate passes, else 0.0
  SumExpression / MultExpression                non-empty, folded left to right
  NegExpression / AbsExpression
  DivExpression(DivisionParams(left, right, by_zero_default))
  LinDecay / ExpDecay / GaussDecayExpression(DecayParamsExpression(x, target, scale, midpoint))
      with d = |x - target| and one coefficient computed here with Python's math:
      lin    lam = (1 - midpoint) / scale       max(0.0, 1.0 - lam * d)
      exp    lam = ln(midpoint) / scale         E(lam * d)
      gauss  lam = ln(midpoint) / scale^2       E(lam * (d * d))
      E: include/ragmi.h "Formula queries"

compile_formula turns a tree into a postfix program of at most MAX_OPS ops over a stack at most
MAX_STACK deep: ops (kind, arg, flags, imm) and the condition programs (ragmi.filters
FilterPrograms) its COND ops name. Formula.blob() is the device form (include/ragmi.h). A
variable a candidate lacks takes its entry in `defaults` (a field name or "$score[i]"; a datetime
field's default is a datetime or string); without one the request fails at run time, as it does
when a value is not finite. Refused here with ValueError: what the text above excludes, an
undeclared field, bad decay parameters, more than MAX_CONDS distinct conditions, a program past
either limit; with NotImplementedError: sqrt, pow, exp, log10, ln and geo_distance expressions.

Host-only, numpy-only.
"""
from __future__ import annotations

import math
import re
import struct
from dataclasses import dataclass

import numpy as np

from . import qdrant_models as models
from .filters import FilterProgram, _number, compile_program, datetime_micros, pack_view

MAX_OPS = 64           # RAG_FORMULA_MAX_OPS
MAX_STACK = 8          # RAG_FORMULA_MAX_STACK
MAX_CONDS = 8          # RAG_FORMULA_MAX_CONDS
HDR_WORDS = 2          # RAG_FORMULA_HDR_WORDS
OP_WORDS = 6           # RAG_FORMULA_OP_WORDS
(CONST, SCORE, KEY, COND, ADD, MUL, NEG, ABS, DIV, LIN, EXP, GAUSS) = range(12)   # RAG_FORMULA_*
HAS_DEFAULT, IS_DATETIME = 1, 2                 # op flags
MISSING, NONFINITE, BAD = 1, 2, 4               # status bits (RAG_FORMULA_MISSING, ...)
POPS = {CONST: 0, SCORE: 0, KEY: 0, COND: 0, NEG: 1, ABS: 1, ADD: 2, MUL: 2, DIV: 2, LIN: 2,
        EXP: 2, GAUSS: 2}

_NOT_BUILT = {models.SqrtExpression: "sqrt", models.PowExpression: "pow",
              models.ExpExpression: "exp", models.Log10Expression: "log10",
              models.LnExpression: "ln", models.GeoDistance: "geo_distance"}
_DECAYS = {models.LinDecayExpression: ("lin_decay", LIN),
           models.ExpDecayExpression: ("exp_decay", EXP),
           models.GaussDecayExpression: ("gauss_decay", GAUSS)}
_CONDITIONS = (models.FieldCondition, models.IsEmptyCondition, models.Filter)
_SCORE_I = re.compile(r"\$score\[(\d+)\]")


def seconds_of(value) -> float:
    """A datetime or RFC 3339 string as seconds since the epoch: integer microseconds
    (filters.datetime_micros) as a double, divided by 1e6 in one fp64 division — the KEY op's
    conversion. ValueError for what does not parse."""
    us = datetime_micros(value)
    if us is None:
        raise ValueError(f"formula: {value!r} is not a datetime that parses (RFC 3339)")
    return float(us) / 1e6


@dataclass(frozen=True)
class Formula:
    """A compiled formula. ops: a tuple of (kind, arg, flags, imm); programs: the FilterPrograms
    of its COND ops; depth: the deepest the evaluation stack gets. Hashable: equal formulas
    share a launch."""
    ops: tuple
    programs: tuple
    depth: int

    @property
    def has_cond(self) -> bool:
        return bool(self.programs)

    @property
    def columns(self) -> tuple:
        """The key columns the program reads: its KEY ops' and its conditions' RANGE atoms'."""
        cols = {op[1] for op in self.ops if op[0] == KEY}
        cols |= {a[1] for p in self.programs for a in p.atoms if a[0] == "range"}
        return tuple(sorted(cols))

    def blob(self) -> np.ndarray:
        return pack_formula(self.ops, self.programs)


def pack_formula(ops, programs=()) -> np.ndarray:
    """The device blob (uint32; include/ragmi.h "Formula queries"): (op count, condition
    program count), 6 words per op (kind, arg, flags, 0, imm low, imm high), then the pack_view
    blob of the condition programs when there are any."""
    head = np.zeros(HDR_WORDS + OP_WORDS * len(ops), np.uint32)
    head[0], head[1] = len(ops), len(programs)
    for i, (kind, arg, flags, imm) in enumerate(ops):
        lo, hi = struct.unpack("<II", struct.pack("<d", float(imm)))
        head[HDR_WORDS + OP_WORDS * i:HDR_WORDS + OP_WORDS * (i + 1)] = (kind, arg, flags, 0, lo, hi)
    if not programs:
        return head
    return np.concatenate([head, pack_view(programs)]).astype(np.uint32)


def depth_of(ops) -> int:
    """The deepest the stack gets running `ops`; ValueError when an op lacks its operands or
    the program does not leave exactly one value."""
    depth = deepest = 0
    for op in ops:
        if depth < POPS[op[0]]:
            raise ValueError("formula: an op without its operands")
        depth += 1 - POPS[op[0]]
        deepest = max(deepest, depth)
    if depth != 1:
        raise ValueError("formula: the program must leave exactly one value")
    return deepest


class _Compiler:
    def __init__(self, defaults, n_lists: int, tags, ranges):
        self.defaults = dict(defaults or {})
        self.L = int(n_lists)
        self.tags, self.ranges = tags, ranges
        self.ops: list = []
        self.programs: list = []

    def emit(self, kind, arg=0, flags=0, imm=0.0):
        self.ops.append((kind, int(arg), int(flags), float(imm)))

    def number(self, value, what: str) -> float:
        x = _number(value)
        if x is None:
            raise ValueError(f"formula: {what} must be a number, got {value!r}")
        return x

    def default(self, name: str, datetime: bool = False):
        """(flags, imm) of variable `name`'s entry in defaults."""
        if name not in self.defaults:
            return 0, 0.0
        v = self.defaults[name]
        return HAS_DEFAULT, (seconds_of(v) if datetime else
                             self.number(v, f"defaults[{name!r}]"))

    def column(self, field: str, kind: str) -> int:
        if field not in self.ranges.fields:
            what = ("a keyword tag field, which holds no number" if field in self.tags.fields
                    else "not a declared range field")
            raise ValueError(f"formula: {field!r} is {what} (range fields: "
                             f"{self.ranges.fields}; declare one with create_payload_index)")
        col = self.ranges.fields.index(field)
        have = self.ranges.kinds[col]
        if have != kind:
            raise ValueError(
                f"formula: {field!r} is a {have} field: " +
                ("name it with DatetimeKeyExpression(datetime_key=...)" if have == "datetime"
                 else "DatetimeKeyExpression takes a datetime field; name it as a plain variable"))
        return col

    def variable(self, name: str):
        if name == "$score" or _SCORE_I.fullmatch(name):
            if name == "$score":
                if self.L != 1:
                    raise ValueError(f"formula: \"$score\" needs exactly one prefetch, the request "
                                     f"has {self.L}: write \"$score[i]\"")
                i = 0
            else:
                i = int(_SCORE_I.fullmatch(name).group(1))
                if i >= self.L:
                    raise ValueError(f"formula: {name} names prefetch {i} of {self.L}")
            flags, imm = self.default(f"$score[{i}]")
            if not flags and name == "$score":
                flags, imm = self.default("$score")
            return self.emit(SCORE, i, flags, imm)
        if name.startswith("$"):
            raise ValueError(f"formula: unknown variable {name!r} ($score and $score[i] are the "
                             "ones built)")
        col = self.column(name, "number")
        flags, imm = self.default(name)
        self.emit(KEY, col, flags, imm)

    def condition(self, cond):
        flt = cond if isinstance(cond, models.Filter) else models.Filter(must=[cond])
        prog = compile_program(self.tags, flt, self.ranges)
        if not isinstance(prog, FilterProgram):       # every point passes / none can
            return self.emit(CONST, imm=0.0 if prog is None else 1.0)
        if prog not in self.programs:
            if len(self.programs) >= MAX_CONDS:
                raise ValueError(f"formula: at most {MAX_CONDS} distinct conditions per formula")
            self.programs.append(prog)
        self.emit(COND, self.programs.index(prog))

    def fold(self, items, op: int, what: str):
        items = list(items) if isinstance(items, (list, tuple)) else None
        if not items:
            raise ValueError(f"formula: {what} needs a non-empty list of expressions")
        self.expr(items[0])
        for x in items[1:]:
            self.expr(x)
            self.emit(op)

    def decay(self, par, op: int, what: str):
        if not isinstance(par, models.DecayParamsExpression):
            raise ValueError(f"formula: {what} takes a DecayParamsExpression")
        scale = 1.0 if par.scale is None else self.number(par.scale, f"{what} scale")
        mid = 0.5 if par.midpoint is None else self.number(par.midpoint, f"{what} midpoint")
        if not scale > 0.0 or math.isinf(scale):
            raise ValueError(f"formula: {what} scale must be a finite number > 0, got {scale!r}")
        if not 0.0 < mid < 1.0:
            raise ValueError(f"formula: {what} midpoint must lie in (0, 1), got {mid!r}")
        lam = ((1.0 - mid) / scale if op == LIN else
               math.log(mid) / scale if op == EXP else math.log(mid) / (scale * scale))
        self.expr(par.x)
        self.expr(0.0 if par.target is None else par.target)
        self.emit(op, imm=lam)

    def expr(self, e):
        if type(e) in _NOT_BUILT:
            raise NotImplementedError(
                f"formula: the {_NOT_BUILT[type(e)]} expression is not built (sum, mult, div, "
                "neg, abs, lin_decay, exp_decay and gauss_decay are; sqrt, pow, exp, log10, ln "
                "and geo_distance are not)")
        if isinstance(e, str):
            return self.variable(e)
        if isinstance(e, _CONDITIONS):
            return self.condition(e)
        if isinstance(e, models.DatetimeExpression):
            return self.emit(CONST, imm=seconds_of(e.datetime))
        if isinstance(e, models.DatetimeKeyExpression):
            col = self.column(e.datetime_key, "datetime")
            flags, imm = self.default(e.datetime_key, datetime=True)
            return self.emit(KEY, col, flags | IS_DATETIME, imm)
        if isinstance(e, models.SumExpression):
            return self.fold(e.sum, ADD, "sum")
        if isinstance(e, models.MultExpression):
            return self.fold(e.mult, MUL, "mult")
        if isinstance(e, (models.NegExpression, models.AbsExpression)):
            neg = isinstance(e, models.NegExpression)
            self.expr(e.neg if neg else e.abs)
            return self.emit(NEG if neg else ABS)
        if isinstance(e, models.DivExpression):
            d = e.div
            if not isinstance(d, models.DivisionParams):
                raise ValueError("formula: div takes a DivisionParams")
            self.expr(d.left)
            self.expr(d.right)
            if d.by_zero_default is None:
                return self.emit(DIV)
            return self.emit(DIV, 0, HAS_DEFAULT, self.number(d.by_zero_default, "by_zero_default"))
        if type(e) in _DECAYS:
            attr, op = _DECAYS[type(e)]
            return self.decay(getattr(e, attr), op, attr)
        x = _number(e)
        if x is None:
            raise ValueError(f"formula: {e!r} is not an expression (a number, a variable name, a "
                             "condition or one of the *Expression types)")
        self.emit(CONST, imm=x)


def compile_formula(formula, defaults, n_lists: int, tags, ranges) -> Formula:
    """The expression tree `formula` of a request with `n_lists` prefetches over a collection's
    `tags` (PayloadTags) and `ranges` (PayloadRanges) -> Formula (module docstring)."""
    if isinstance(formula, models.FormulaQuery):
        formula, defaults = formula.formula, formula.defaults
    if defaults is not None and not isinstance(defaults, dict):
        raise ValueError("formula: defaults must be a dict of variable name to value")
    c = _Compiler(defaults, n_lists, tags, ranges)
    c.expr(formula)
    if len(c.ops) > MAX_OPS:
        raise ValueError(f"formula: {len(c.ops)} ops; a formula program holds at most {MAX_OPS}")
    depth = depth_of(c.ops)
    if depth > MAX_STACK:
        raise ValueError(f"formula: nested {depth} deep; the evaluation stack holds at most "
                         f"{MAX_STACK} values (put the deeper operand first)")
    return Formula(tuple(c.ops), tuple(c.programs), depth)
