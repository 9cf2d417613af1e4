"""Two restatements of formula queries (rag_formula_rescore; include/ragmi.h "Formula queries",
DESIGN §R14). TEST HELPER ONLY, used by test_formula_cpu.py and test_formula_gpu.py.

1. `rescore`: the kernel restated in numpy over the same arrays and the same blob. It parses the
   blob itself, applies the kernel's checks, runs the ops in order over fp64 arrays (numpy
   multiplies and adds one at a time: no fma) and orders by the kernel's own key. The GPU must
   match it bit for bit. Condition programs go through ragmi.filters.eval_view_np, the numpy
   restatement of the filter kernel they share their format with.

2. `walk` / `walk_request`: an independent walker of the request TREE over payload dicts, in
   Python floats. It imports nothing from ragmi.formula or ragmi.filters: conditions go through
   _range_ref.matches_range, datetimes through _range_ref.as_datetime as integer microseconds
   / 1e6, and E is written again, in scalar arithmetic.
"""
import datetime as dt
import math
import re

import numpy as np

from _range_ref import as_datetime, as_number, matches_range

# ------------------------------------------------------------------ E, twice
LOG2E = 1.4426950408889634
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
COEF = [1.0 / float(math.factorial(i)) for i in range(14)]     # i! is exact: correctly rounded


def E(a):
    """The decay exponential over an fp64 array: mul / add only."""
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        ok = a <= 0.0
        zero = ok & (a < -700.0)
        x = np.where(ok & ~zero, a, 0.0)
        n = np.rint(x * LOG2E)
        r = (x - n * LN2_HI) - n * LN2_LO
        p = np.full(x.shape, COEF[13])
        for i in range(12, -1, -1):
            p = p * r + COEF[i]
        v = p * np.ldexp(1.0, n.astype(np.int64))
    return np.where(zero, 0.0, np.where(ok, v, np.nan))


def E1(a: float) -> float:
    """E of one Python float, written on its own."""
    if not a <= 0.0:
        return math.nan
    if a < -700.0:
        return 0.0
    n = float(round(a * LOG2E))            # round half to even, as rint
    r = (a - n * LN2_HI) - n * LN2_LO
    p = COEF[13]
    for i in range(12, -1, -1):
        p = p * r + COEF[i]
    return math.ldexp(p, int(n))


# ------------------------------------------------------------------ 1. the kernel, in numpy
MAX_OPS, MAX_STACK, MAX_CONDS, MAX_COLS, HDR, OPW, REC = 64, 8, 8, 4, 2, 6, 41
(CONST, SCORE, KEY, COND, ADD, MUL, NEG, ABS, DIV, LIN, EXP, GAUSS) = range(12)
POPS = {CONST: 0, SCORE: 0, KEY: 0, COND: 0, NEG: 1, ABS: 1, ADD: 2, MUL: 2, DIV: 2, LIN: 2,
        EXP: 2, GAUSS: 2}
MISSING, NONFINITE, BAD = 1, 2, 4
KEY_ABSENT = -(1 << 63)


def list_lengths(cand_rows, ncand):
    """n[b][l] = min(ncand clamped to [0, C], the number of leading entries with row >= 0)."""
    B, L, C = cand_rows.shape
    n = np.empty((B, L), np.int64)
    for b in range(B):
        for l in range(L):
            bad = np.nonzero(cand_rows[b, l] < 0)[0]
            lim = C if ncand is None else min(max(int(np.asarray(ncand)[b][l]), 0), C)
            n[b, l] = min(lim, int(bad[0]) if bad.size else C)
    return n


def parse(blob, L, have_tags, have_cols):
    """(ops, U, pool) of a blob the kernel accepts, None of one it calls bad."""
    blob = np.asarray(blob, np.uint32).reshape(-1)
    words = len(blob)
    if words < HDR:
        return None
    n, U = int(blob[0]), int(blob[1])
    if n > MAX_OPS or U > MAX_CONDS or HDR + OPW * n + REC * U > words:
        return None
    ops, depth = [], 0
    for i in range(n):
        kind, arg, fl, _, lo, hi = (int(x) for x in blob[HDR + OPW * i:HDR + OPW * (i + 1)])
        imm = float(np.array([lo, hi], np.uint32).view(np.float64)[0])
        if kind not in POPS or depth < POPS[kind]:
            return None
        if (kind == SCORE and arg >= L) or (kind == COND and (arg >= U or not have_tags)) or \
                (kind == KEY and (arg >= MAX_COLS or not have_cols[arg])):
            return None
        depth += 1 - POPS[kind]
        if depth > MAX_STACK:
            return None
        ops.append((kind, arg, fl, imm))
    if depth != 1:
        return None
    return ops, U, blob[HDR + OPW * n:]


def value_key(f32):
    """The kernel's order-preserving uint32 of fp32 values: ascending in the value."""
    b = np.ascontiguousarray(f32, np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def rescore(cand_s, cand_r, blob, k, ncand=None, cand_t=None, cand_keys=None):
    """rag_formula_rescore over host arrays: cand_s fp32 / cand_r int64 [B, L, C], cand_t uint32
    [B, L, C] or None, cand_keys a dict / sequence of column -> int64 [B, L, C] (None = not
    supplied). Returns (scores fp32 [B, k], rows int64 [B, k], count int32 [B], status uint32
    [B]). Where the status is non-zero the scores and rows are what this restatement's own
    order gives, which the kernel need not match."""
    cand_s = np.asarray(cand_s, np.float32)
    cand_r = np.asarray(cand_r, np.int64)
    B, L, C = cand_r.shape
    cols = [None] * MAX_COLS
    for c, x in (cand_keys.items() if hasattr(cand_keys, "items") else enumerate(cand_keys or ())):
        cols[c] = None if x is None else np.asarray(x, np.int64)
    prog = parse(blob, L, cand_t is not None, [x is not None for x in cols])
    lens = list_lengths(cand_r, ncand)
    out_s = np.full((B, k), -np.inf, np.float32)
    out_r = np.full((B, k), -1, np.int64)
    count = np.zeros(B, np.int32)
    status = np.zeros(B, np.uint32)
    for b in range(B):
        first, per_list = {}, {}           # row -> its first entry e; (row, l) -> first score
        for l in range(L):
            for p in range(int(lens[b, l])):
                r = int(cand_r[b, l, p])
                first.setdefault(r, l * C + p)
                per_list.setdefault((r, l), cand_s[b, l, p])
        rows = np.array(sorted(first), np.int64)
        count[b] = len(rows)
        e0 = np.array([first[int(r)] for r in rows], np.int64)
        m = len(rows)
        st = 0
        val = np.zeros(m, np.float64)
        if prog is None:
            st = BAD
        elif m:
            ops, U, pool = prog
            tags = None if cand_t is None else np.asarray(cand_t, np.uint32)[b].reshape(-1)[e0]
            keys = np.stack([np.full(m, KEY_ABSENT, np.int64) if x is None else
                             x[b].reshape(-1)[e0] for x in cols])
            view = None
            stack = []
            with np.errstate(all="ignore"):
                for kind, arg, fl, imm in ops:
                    if kind == CONST:
                        stack.append(np.full(m, imm))
                    elif kind == SCORE:
                        got = [per_list.get((int(r), arg)) for r in rows]
                        miss = np.array([g is None for g in got])
                        v = np.array([0.0 if g is None else float(g) for g in got], np.float64)
                        if miss.any() and not fl & 1:
                            st |= MISSING
                        stack.append(np.where(miss, imm if fl & 1 else 0.0, v))
                    elif kind == KEY:
                        kk = keys[arg]
                        miss = kk == KEY_ABSENT
                        bits = np.where(kk >= 0, kk, kk ^ np.int64(0x7FFFFFFFFFFFFFFF))
                        v = bits.view(np.float64)
                        if fl & 2:
                            v = v / 1e6
                        if miss.any() and not fl & 1:
                            st |= MISSING
                        stack.append(np.where(miss, imm if fl & 1 else 0.0, v))
                    elif kind == COND:
                        if view is None:
                            from ragmi.filters import eval_view_np
                            view = eval_view_np(pool, tags, U, keys=keys)
                        stack.append(((view >> np.uint32(arg)) & np.uint32(1)).astype(np.float64))
                    elif kind == NEG:
                        stack.append(-stack.pop())
                    elif kind == ABS:
                        stack.append(np.abs(stack.pop()))
                    else:
                        y, x = stack.pop(), stack.pop()
                        if kind == ADD:
                            v = x + y
                        elif kind == MUL:
                            v = x * y
                        elif kind == DIV:
                            v = x / y
                            if (y == 0.0).any():
                                if fl & 1:
                                    v = np.where(y == 0.0, imm, v)
                                else:
                                    st |= NONFINITE
                        elif kind == LIN:
                            t = 1.0 - imm * np.abs(x - y)
                            v = np.where(t > 0.0, t, 0.0)
                        elif kind == EXP:
                            v = E(imm * np.abs(x - y))
                        else:
                            d = np.abs(x - y)
                            v = E(imm * (d * d))
                        stack.append(v)
                val = stack.pop()
        with np.errstate(all="ignore"):
            f = val.astype(np.float32)
        f[f == 0.0] = 0.0
        if not np.isfinite(f).all():
            st |= NONFINITE
        status[b] = st
        order = np.lexsort((rows, ~value_key(f)))[:k]
        out_s[b, :len(order)] = f[order]
        out_r[b, :len(order)] = rows[order]
    return out_s, out_r, count, status


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 2. the tree walker
class Missing(Exception):
    pass


class NonFinite(Exception):
    pass


EPOCH = dt.datetime(1970, 1, 1, tzinfo=dt.timezone.utc)


def seconds(v):
    """A datetime value as seconds since the epoch (integer microseconds / 1e6); None for what
    a datetime field holds no value for."""
    d = as_datetime(v)
    return None if d is None else float((d - EPOCH) // dt.timedelta(microseconds=1)) / 1e6


def walk(e, defaults, payload, scores, kinds) -> float:
    """The fp64 value of expression `e` for one candidate: `payload` its dict, `scores` its
    score per prefetch (None where it is absent), `kinds` the range fields."""
    from ragmi import qdrant_models as m
    go = lambda x: walk(x, defaults, payload, scores, kinds)
    payload = payload or {}
    if isinstance(e, str):
        s = re.fullmatch(r"\$score(?:\[(\d+)\])?", e)
        if s:
            assert s.group(1) is not None or len(scores) == 1
            i = int(s.group(1) or 0)
            if scores[i] is not None:
                return float(scores[i])
            if f"$score[{i}]" not in defaults:
                raise Missing(e)
            return float(defaults[f"$score[{i}]"])
        assert kinds[e] == "number"
        v = as_number(payload.get(e))
        if v is None:
            if e not in defaults:
                raise Missing(e)
            v = float(defaults[e])
        return 0.0 if v == 0.0 else v      # a stored -0.0 is +0.0 (the key encoding)
    if isinstance(e, m.DatetimeKeyExpression):
        assert kinds[e.datetime_key] == "datetime"
        v = seconds(payload.get(e.datetime_key))
        if v is None:
            if e.datetime_key not in defaults:
                raise Missing(e.datetime_key)
            v = seconds(defaults[e.datetime_key])
        return v
    if isinstance(e, m.DatetimeExpression):
        return seconds(e.datetime)
    if isinstance(e, (m.FieldCondition, m.IsEmptyCondition)):
        return 1.0 if matches_range(m.Filter(must=[e]), payload, kinds) else 0.0
    if isinstance(e, m.Filter):
        return 1.0 if matches_range(e, payload, kinds) else 0.0
    if isinstance(e, m.SumExpression):
        v = go(e.sum[0])
        for x in e.sum[1:]:
            v = v + go(x)
        return v
    if isinstance(e, m.MultExpression):
        v = go(e.mult[0])
        for x in e.mult[1:]:
            v = v * go(x)
        return v
    if isinstance(e, m.NegExpression):
        return -go(e.neg)
    if isinstance(e, m.AbsExpression):
        return abs(go(e.abs))
    if isinstance(e, m.DivExpression):
        x, y = go(e.div.left), go(e.div.right)
        if y == 0.0:
            if e.div.by_zero_default is None:
                raise NonFinite("division by zero")
            return float(e.div.by_zero_default)
        return x / y
    for cls, attr in ((m.LinDecayExpression, "lin_decay"), (m.ExpDecayExpression, "exp_decay"),
                      (m.GaussDecayExpression, "gauss_decay")):
        if isinstance(e, cls):
            par = getattr(e, attr)
            scale = 1.0 if par.scale is None else float(par.scale)
            mid = 0.5 if par.midpoint is None else float(par.midpoint)
            d = abs(go(par.x) - (0.0 if par.target is None else go(par.target)))
            if attr == "lin_decay":
                return max(0.0, 1.0 - ((1.0 - mid) / scale) * d)
            if attr == "exp_decay":
                return E1((math.log(mid) / scale) * d)
            return E1((math.log(mid) / (scale * scale)) * (d * d))
    assert isinstance(e, (int, float, np.integer, np.floating)) and not isinstance(e, bool), e
    return float(e)


def walk_request(query, lists, payload_of, kinds, limit):
    """A formula request answered by the walker. `query`: the FormulaQuery; `lists`: per
    prefetch its hits [(id, score)], best first; `payload_of`: id -> payload dict. Returns
    [(id, fp32 value)] by (value descending, id ascending), cut to `limit`; raises Missing /
    NonFinite as the request would fail."""
    seen = {}
    for l, hits in enumerate(lists):
        for pid, sc in hits:
            seen.setdefault(pid, [None] * len(lists))
            if seen[pid][l] is None:
                seen[pid][l] = sc
    out = []
    for pid, scores in seen.items():
        with np.errstate(all="ignore"):
            f = np.float32(walk(query.formula, query.defaults or {}, payload_of(pid), scores,
                                kinds))
        if not np.isfinite(f):
            raise NonFinite(pid)
        out.append((pid, np.float32(0.0) if f == 0.0 else f))
    out.sort(key=lambda h: (-float(h[1]), h[0]))
    return out[:limit]
