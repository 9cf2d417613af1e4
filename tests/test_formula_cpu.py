"""CPU tests of formula queries (ragmi.formula): the compiler (op order, stack
depth, limits, every refusal), the compiled program run by the numpy restatement of the kernel
against the independent tree walker (tests/_formula_ref.py) on random payloads and formulas, E
against numpy.exp, rag_formula_rescore's argument refusals through ctypes (no device), and the
client's routing checks that need no search."""
import ctypes
import datetime as dt
import os

import numpy as np
import pytest

from conftest import ROOT

import _formula_ref as F

RAG_EINVAL, RAG_ERANGE = -1, -4
V = [0.0, 1.0, 0.0, 0.0]
KINDS = {"fiscal_year": "number", "ingested_at": "datetime", "revenue": "number"}
UTC = dt.timezone.utc


def books():
    from ragmi.filters import PayloadRanges, PayloadTags
    return PayloadTags(), PayloadRanges(KINDS)


def comp(expr, defaults=None, L=1, tr=None):
    from ragmi.formula import compile_formula
    tags, ranges = tr or books()
    return compile_formula(expr, defaults, L, tags, ranges)


# ------------------------------------------------------------------ 1. the models
def test_models_keep_qdrant_clients_keywords():
    from ragmi import qdrant_models as m
    q = m.FormulaQuery(formula=m.SumExpression(sum=["$score", 1.0]))
    assert q.defaults == {} and q.formula.sum == ["$score", 1.0]
    assert m.FormulaQuery(formula=1.0, defaults={"x": 2}).defaults == {"x": 2}
    d = m.DivisionParams(left=1.0, right="x")
    assert (d.left, d.right, d.by_zero_default) == (1.0, "x", None)
    p = m.DecayParamsExpression(x="x")
    assert (p.x, p.target, p.scale, p.midpoint) == ("x", None, None, None)
    assert m.LinDecayExpression(lin_decay=p).lin_decay is p
    assert m.ExpDecayExpression(exp_decay=p).exp_decay is p
    assert m.GaussDecayExpression(gauss_decay=p).gauss_decay is p
    assert m.MultExpression(mult=[1]).mult == [1] and m.NegExpression(neg=1).neg == 1
    assert m.AbsExpression(abs=1).abs == 1 and m.DivExpression(div=d).div is d
    assert m.DatetimeExpression(datetime="2024-01-01").datetime == "2024-01-01"
    assert m.DatetimeKeyExpression(datetime_key="t").datetime_key == "t"


# ------------------------------------------------------------------ 2. the compiler
def test_op_order_depth_and_blob():
    from ragmi import formula as fm
    from ragmi import qdrant_models as m
    f = comp(m.SumExpression(sum=["$score", m.MultExpression(mult=[0.25, "fiscal_year"]), 3]))
    assert [op[0] for op in f.ops] == [fm.SCORE, fm.CONST, fm.KEY, fm.MUL, fm.ADD, fm.CONST,
                                       fm.ADD]
    assert f.depth == 3 and f.columns == (0,) and not f.has_cond
    # a left-leaning sum stays shallow, a right-leaning one costs a level per term
    assert comp(m.SumExpression(sum=[1.0] * 30)).depth == 2
    right = 1.0
    for _ in range(7):
        right = m.SumExpression(sum=[1.0, right])
    assert comp(right).depth == 8
    blob = f.blob()
    assert blob.dtype == np.uint32 and len(blob) == fm.HDR_WORDS + fm.OP_WORDS * 7
    assert blob[0] == 7 and blob[1] == 0
    assert blob[2 + 6].tolist() == fm.CONST and blob[2 + 6 + 4:2 + 6 + 6].view(np.float64)[0] == 0.25
    assert F.parse(blob, 1, False, [True] * 4)[0] == list(f.ops)
    # conditions: equal ones share a program, the blob ends in their pack_view blob
    tr = books()
    tr[0].tag({"ticker": "AMD", "document_type": "10-K"})
    c = m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))
    g = comp(m.SumExpression(sum=[c, c, m.FieldCondition(key="revenue", range=m.Range(gt=0))]),
             tr=tr)
    assert [op[:2] for op in g.ops if op[0] == fm.COND] == [(fm.COND, 0), (fm.COND, 0),
                                                            (fm.COND, 1)]
    assert len(g.programs) == 2 and g.has_cond and g.columns == (2,)
    from ragmi.filters import pack_view
    assert np.array_equal(g.blob()[2 + 6 * len(g.ops):], pack_view(g.programs))
    # a condition nothing / everything passes is a constant
    never = m.FieldCondition(key="ticker", match=m.MatchValue(value="NONE"))
    assert comp(never, tr=tr).ops == ((fm.CONST, 0, 0, 0.0),)
    assert comp(m.Filter(), tr=tr).ops == ((fm.CONST, 0, 0, 1.0),)
    # hashable: equal formulas are equal
    assert comp(m.SumExpression(sum=["$score", 1])) == comp(m.SumExpression(sum=["$score", 1.0]))


def test_limits_are_refused():
    from ragmi import qdrant_models as m
    assert len(comp(m.SumExpression(sum=[1.0] * 32)).ops) == 63
    with pytest.raises(ValueError, match="at most 64"):
        comp(m.SumExpression(sum=[1.0] * 33))
    deep = 1.0
    for _ in range(8):
        deep = m.SumExpression(sum=[1.0, deep])
    with pytest.raises(ValueError, match="at most 8 values"):
        comp(deep)
    tr = books()
    for i in range(9):
        tr[0].tag({"ticker": f"T{i}"})
    conds = [m.FieldCondition(key="ticker", match=m.MatchValue(value=f"T{i}")) for i in range(9)]
    assert len(comp(m.SumExpression(sum=conds[:8]), tr=tr).programs) == 8
    with pytest.raises(ValueError, match="at most 8 distinct conditions"):
        comp(m.SumExpression(sum=conds), tr=tr)


def test_refusals_name_their_cause():
    from ragmi import qdrant_models as m
    from ragmi.filters import UnsupportedFilter
    decay = lambda **kw: m.ExpDecayExpression(exp_decay=m.DecayParamsExpression(x=1.0, **kw))
    for expr, L, word in (
            ("$score", 2, r"\$score\[i\]"),
            ("$score[2]", 2, "prefetch 2 of 2"),
            ("$other", 1, "unknown variable"),
            ("ingested_at", 1, "DatetimeKeyExpression"),
            ("nope", 1, "create_payload_index"),
            ("ticker", 1, "create_payload_index"),
            (m.DatetimeKeyExpression(datetime_key="fiscal_year"), 1, "number field"),
            (m.DatetimeKeyExpression(datetime_key="nope"), 1, "create_payload_index"),
            (m.DatetimeExpression(datetime="yesterday"), 1, "does not|not a datetime"),
            (m.SumExpression(sum=[]), 1, "non-empty"),
            (m.MultExpression(mult=None), 1, "non-empty"),
            (decay(scale=0), 1, "scale"), (decay(scale=-1.0), 1, "scale"),
            (decay(midpoint=0.0), 1, "midpoint"), (decay(midpoint=1.0), 1, "midpoint"),
            (decay(midpoint=float("nan")), 1, "midpoint"),
            (m.LinDecayExpression(lin_decay=1.0), 1, "DecayParamsExpression"),
            (m.DivExpression(div=(1.0, 2.0)), 1, "DivisionParams"),
            (True, 1, "not an expression"), (None, 1, "not an expression"),
            (float("nan"), 1, "not an expression"), ([1.0], 1, "not an expression")):
        with pytest.raises(ValueError, match=word):
            comp(expr, L=L)
    for expr, word in ((m.SqrtExpression(sqrt=1.0), "sqrt"),
                       (m.PowExpression(pow=m.PowParams(base=2.0, exponent=2.0)), "pow"),
                       (m.ExpExpression(exp=1.0), "exp"), (m.Log10Expression(log10=1.0), "log10"),
                       (m.LnExpression(ln=1.0), "ln"),
                       (m.GeoDistance(geo_distance=m.GeoDistanceParams(origin=None, to="x")),
                        "geo_distance")):
        with pytest.raises(NotImplementedError, match=f"the {word} expression is not built"):
            comp(m.SumExpression(sum=[1.0, expr]))
    with pytest.raises(UnsupportedFilter):            # the filter algebra's own refusal
        comp(m.FieldCondition(key="nope", match=m.MatchValue(value=1)))
    with pytest.raises(ValueError, match="defaults"):
        comp("$score", defaults=[1.0])


def test_defaults_are_converted():
    from ragmi import formula as fm
    from ragmi import qdrant_models as m
    f = comp("$score[1]", {"$score[1]": 2, "$score[0]": 9}, L=2)
    assert f.ops == ((fm.SCORE, 1, fm.HAS_DEFAULT, 2.0),)
    assert comp("$score[0]", {}, L=2).ops == ((fm.SCORE, 0, 0, 0.0),)
    assert comp("$score", None).ops == ((fm.SCORE, 0, 0, 0.0),)
    assert comp("revenue", {"revenue": np.float32(1.5)}).ops == ((fm.KEY, 2, fm.HAS_DEFAULT, 1.5),)
    key = m.DatetimeKeyExpression(datetime_key="ingested_at")
    want = 1704067200.25
    for d in ("2024-01-01T00:00:00.25Z", dt.datetime(2024, 1, 1, 0, 0, 0, 250000, tzinfo=UTC),
              "2024-01-01T09:00:00.250+09:00"):
        assert comp(key, {"ingested_at": d}).ops == \
            ((fm.KEY, 1, fm.HAS_DEFAULT | fm.IS_DATETIME, want),)
    assert comp(key).ops == ((fm.KEY, 1, fm.IS_DATETIME, 0.0),)
    assert comp(m.DatetimeExpression(datetime="1970-01-01")).ops == ((fm.CONST, 0, 0, 0.0),)
    assert comp(m.DatetimeExpression(datetime=dt.date(2024, 1, 1))).ops[0][3] == 1704067200.0
    with pytest.raises(ValueError, match="not a datetime"):
        comp(key, {"ingested_at": "soon"})
    with pytest.raises(ValueError, match="must be a number"):
        comp("revenue", {"revenue": "1"})
    # the decay coefficients, with Python's math
    import math
    par = lambda **kw: m.DecayParamsExpression(x="revenue", **kw)
    lin = comp(m.LinDecayExpression(lin_decay=par(scale=4.0, midpoint=0.25)))
    assert lin.ops[-1] == (fm.LIN, 0, 0, 0.75 / 4.0) and lin.ops[1] == (fm.CONST, 0, 0, 0.0)
    assert comp(m.ExpDecayExpression(exp_decay=par(scale=3.0))).ops[-1][3] == math.log(0.5) / 3.0
    assert comp(m.GaussDecayExpression(gauss_decay=par(scale=3.0, midpoint=0.1))).ops[-1][3] == \
        math.log(0.1) / 9.0
    assert comp(m.ExpDecayExpression(exp_decay=par())).ops[-1][3] == math.log(0.5)


# ------------------------------------------------------------------ 3. E
def test_E_against_numpy_exp():
    rng = np.random.default_rng(0)
    a = np.concatenate([np.linspace(-700.0, 0.0, 1_000_001), -700.0 * rng.random(1_000_000),
                        -np.exp(rng.uniform(-40.0, 6.5, 500_000)),
                        [0.0, -0.0, -700.0, -1e-300, -np.log(2.0) / 2]])
    a = a[a >= -700.0]
    got, want = F.E(a), np.exp(a)
    rel = np.abs(got - want) / want
    print(f"E: max relative error {rel.max() / 2.0**-53:.3f} * 2^-53 over {len(a)} arguments")
    assert rel.max() <= 2.0 ** -51
    assert (got.astype(np.float32) == want.astype(np.float32)).all()
    assert F.E(np.array([0.0]))[0] == 1.0 and F.E(np.array([-0.0]))[0] == 1.0
    below = np.array([np.nextafter(-700.0, -np.inf), -701.0, -1e10, -np.inf])
    assert (F.E(below) == 0.0).all() and F.E(np.array([-700.0]))[0] > 0.0
    assert np.isnan(F.E(np.array([1e-300, 5.0, np.nan]))).all()
    # the scalar restatement is the same function
    some = a[::9973]
    assert [F.E1(float(x)) for x in some] == F.E(some).tolist()
    assert F.E1(0.0) == 1.0 and F.E1(-701.0) == 0.0 and np.isnan(F.E1(1.0))


# ------------------------------------------------------------------ 4. restatement vs walker
TICKERS = ["AMD", "NVDA", "INTC"]


def payloads(rng, n):
    t0 = dt.datetime(2023, 1, 1, tzinfo=UTC)
    pay = []
    for r in range(n):
        p = {"n": r}
        if rng.random() < 0.9:
            p["ticker"] = TICKERS[rng.integers(0, 3)]
        if rng.random() < 0.8:
            p["document_type"] = ["10-K", "8-K"][rng.integers(0, 2)]
        u = rng.random()
        if u < 0.7:
            p["fiscal_year"] = int(rng.integers(2018, 2025))
        elif u < 0.8:
            p["fiscal_year"] = [None, "FY21", True][rng.integers(0, 3)]
        if rng.random() < 0.8:
            d = t0 + dt.timedelta(seconds=int(rng.integers(0, 2 * 365 * 86400)),
                                  microseconds=int(rng.integers(0, 1_000_000)))
            p["ingested_at"] = [d.isoformat(), d.astimezone(dt.timezone(dt.timedelta(
                hours=-5))).isoformat(), d.date().isoformat()][rng.integers(0, 3)]
        if rng.random() < 0.8:
            p["revenue"] = float(rng.choice([-2.5e9, -1.0, -0.0, 0.0, 1.0, 3.25e9, 0.1]))
        pay.append(p)
    return pay


def random_expr(rng, L, depth=0):
    """A random expression tree over the corpus' fields, at most 4 levels of operators."""
    from ragmi import qdrant_models as m
    go = lambda: random_expr(rng, L, depth + 1)
    leaf = depth >= 3 or rng.random() < 0.3
    if leaf:
        c = rng.integers(0, 7)
        if c == 0:
            return float(rng.choice([0.0, -1.5, 0.1, 3.0, 1e9]))
        if c == 1:
            return f"$score[{rng.integers(0, L)}]"
        if c == 2:
            return ["fiscal_year", "revenue"][rng.integers(0, 2)]
        if c == 3:
            return m.DatetimeKeyExpression(datetime_key="ingested_at")
        if c == 4:
            return m.DatetimeExpression(datetime="2024-03-01T12:00:00Z")
        if c == 5:
            return m.FieldCondition(key="ticker", match=m.MatchAny(any=["AMD", "INTC"]))
        return m.Filter(must_not=[m.FieldCondition(key="fiscal_year", range=m.Range(lt=2021))],
                        should=[m.IsEmptyCondition(is_empty=m.PayloadField(key="revenue")),
                                m.FieldCondition(key="document_type",
                                                 match=m.MatchValue(value="10-K"))])
    c = rng.integers(0, 8)
    if c == 0:
        return m.SumExpression(sum=[go() for _ in range(rng.integers(1, 4))])
    if c == 1:
        return m.MultExpression(mult=[go() for _ in range(rng.integers(1, 4))])
    if c == 2:
        return m.NegExpression(neg=go())
    if c == 3:
        return m.AbsExpression(abs=go())
    if c == 4:
        return m.DivExpression(div=m.DivisionParams(
            left=go(), right=go(), by_zero_default=[None, -2.0][rng.integers(0, 2)]))
    par = m.DecayParamsExpression(x=go(), target=[None, go()][rng.integers(0, 2)],
                                  scale=[None, 30 * 86400.0, 2.5][rng.integers(0, 3)],
                                  midpoint=[None, 0.3][rng.integers(0, 2)])
    return [m.LinDecayExpression(lin_decay=par), m.ExpDecayExpression(exp_decay=par),
            m.GaussDecayExpression(gauss_decay=par)][c - 5]


def test_compiled_program_equals_the_tree_walker():
    from ragmi import qdrant_models as m
    from ragmi.filters import PayloadRanges, PayloadTags
    from ragmi.formula import compile_formula
    rng = np.random.default_rng(1)
    N, C = 300, 12
    pay = payloads(rng, N)
    pt, pr = PayloadTags(), PayloadRanges(KINDS)
    tags = np.array([pt.tag(p) for p in pay], np.uint32)
    keys = np.array([pr.keys(p) for p in pay], np.int64).T.copy()
    every = {"fiscal_year": 2020, "revenue": -3.5, "ingested_at": "2022-06-01T00:00:00Z",
             "$score[0]": 0.0, "$score[1]": -1.0, "$score[2]": 0.25}
    ran = failed = 0
    for trial in range(300):
        L = int(rng.integers(1, 4))
        expr = random_expr(rng, L)
        defaults = every if trial % 3 else {k: every[k] for k in list(every)[trial % 5::2]}
        query = m.FormulaQuery(formula=expr, defaults=defaults)
        try:
            f = compile_formula(query, None, L, pt, pr)
        except ValueError as e:
            assert "at most" in str(e)               # too deep or too long: not this test's
            continue
        rows = np.stack([rng.permutation(40 + 30 * trial % N)[:C] for _ in range(L)])[None]
        rows = (rows + trial) % N
        scores = np.sort(rng.standard_normal((1, L, C)).astype(np.float32), axis=2)[:, :, ::-1]
        ncand = rng.integers(0, C + 1, (1, L)).astype(np.int32)
        s, r, count, status = F.rescore(
            scores, rows, f.blob(), L * C, ncand, tags[rows] if f.has_cond else None,
            {c: keys[c][rows] for c in f.columns})
        lists = [[(int(rows[0, l, p]), scores[0, l, p]) for p in range(ncand[0, l])]
                 for l in range(L)]
        try:
            want = F.walk_request(query, lists, lambda i: pay[i], KINDS, L * C)
        except F.Missing:
            assert status[0] & F.MISSING
            failed += 1
            continue
        except F.NonFinite:
            assert status[0] & F.NONFINITE
            failed += 1
            continue
        assert status[0] == 0, (trial, expr)
        ran += 1
        assert count[0] == len(want)
        assert r[0, :count[0]].tolist() == [h[0] for h in want], (trial, expr)
        assert F.bits(s[0, :count[0]]).tolist() == \
            [int(np.float32(h[1]).view(np.uint32)) for h in want], (trial, expr)
        assert (r[0, count[0]:] == -1).all() and np.isneginf(s[0, count[0]:]).all()
    assert ran >= 150 and failed >= 10, (ran, failed)


def test_restatement_orders_and_flags():
    from ragmi import formula as fm
    score = fm.pack_formula([(fm.SCORE, 0, 0, 0.0)])
    rows = np.array([[[4, 9, 2, 7, 5, 6]]], np.int64)
    sc = np.array([[[0.5, -0.0, 0.0, -1e-3, 0.5, -np.float32(2.0)]]], np.float32)
    s, r, count, status = F.rescore(sc, rows, score, 8)
    assert r[0].tolist() == [4, 5, 2, 9, 7, 6, -1, -1] and count[0] == 6 and status[0] == 0
    assert F.bits(s[0, 2:4]).tolist() == [0, 0]                 # -0.0 reported as +0.0
    # a bad blob evaluates nothing
    for blob in (np.array([1], np.uint32), fm.pack_formula([(fm.ADD, 0, 0, 0.0)]),
                 fm.pack_formula([(fm.SCORE, 1, 0, 0.0)]), fm.pack_formula([(fm.KEY, 0, 0, 0.0)]),
                 fm.pack_formula([(fm.CONST, 0, 0, 1.0)] * 2), fm.pack_formula([(12, 0, 0, 0.0)]),
                 fm.pack_formula([(fm.CONST, 0, 0, 1.0)] * 9 + [(fm.ADD, 0, 0, 0.0)] * 8)):
        assert F.rescore(sc, rows, blob, 3)[3].tolist() == [F.BAD]


# ------------------------------------------------------------------ 5. argument refusals
def test_argument_errors_need_no_device():
    from ragmi import _build, _lib
    _build.build()
    L = _lib.load()
    assert len(_lib.INDEX_API["rag_formula_rescore"][1]) == 16
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)

    def call(B=1, L_=2, C=4, k=3, words=8, s=p, rows=p, prog=p, out_s=p, out_r=p, st=p):
        return L.rag_formula_rescore(s, rows, None, None, None, prog, words, B, L_, C, k, out_s,
                                     out_r, None, st, None)

    for kw, code, word in (({"L_": 0}, RAG_ERANGE, b"L must be"), ({"L_": 17}, RAG_ERANGE, b"16"),
                           ({"L_": -1}, RAG_ERANGE, b"L must be"),
                           ({"C": 0}, RAG_ERANGE, b"C must be"),
                           ({"L_": 1, "C": 4097}, RAG_ERANGE, b"L * C"),
                           ({"L_": 16, "C": 257}, RAG_ERANGE, b"4096"),
                           ({"L_": 16, "C": 1 << 30}, RAG_ERANGE, b"L * C"),
                           ({"k": 0}, RAG_EINVAL, b"k must be"),
                           ({"B": -1}, RAG_EINVAL, b"B must be"),
                           ({"words": 1}, RAG_EINVAL, b"words must be"),
                           ({"s": None}, RAG_EINVAL, b"NULL"), ({"rows": None}, RAG_EINVAL, b"NULL"),
                           ({"prog": None}, RAG_EINVAL, b"NULL"),
                           ({"out_s": None}, RAG_EINVAL, b"NULL"),
                           ({"out_r": None}, RAG_EINVAL, b"NULL"),
                           ({"st": None}, RAG_EINVAL, b"NULL")):
        assert call(**kw) == code and word in L.rag_last_error(), kw
    assert call(B=0, s=None, rows=None, prog=None, out_s=None, out_r=None, st=None) == 0
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    for line in ("#define RAG_FORMULA_MAX_OPS 64", "#define RAG_FORMULA_MAX_STACK 8",
                 "int rag_formula_rescore(", "parity with a Qdrant server's own arithmetic is\n"
                 " * unpinned"):
        assert line in hdr
    assert "rag_formula_rescore" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    from ragmi import formula as fm
    for name in ("CONST", "SCORE", "KEY", "COND", "ADD", "MUL", "NEG", "ABS", "DIV", "LIN", "EXP",
                 "GAUSS"):
        assert f"RAG_FORMULA_{name} = {getattr(fm, name)}" in hdr


def test_formula_rescore_checks_before_any_launch():
    import torch
    from ragmi import formula as fm
    from ragmi.index import formula_rescore
    rows = torch.zeros((1, 2, 4), dtype=torch.int64)
    sc = torch.zeros((1, 2, 4), dtype=torch.float32)
    blob = fm.pack_formula([(fm.SCORE, 0, 0, 0.0)])
    big = lambda *shape: (torch.zeros(shape, dtype=torch.float32),
                          torch.zeros(shape, dtype=torch.int64))
    for s, r, kw in ((sc, rows.to(torch.int32), {}), (sc.double(), rows, {}), (sc[0], rows[0], {}),
                     (sc[:, :1], rows, {}), (sc, rows, {"k": 0}), (*big(1, 17, 1), {}),
                     (*big(1, 16, 257), {}), (*big(1, 2, 0), {}),
                     (sc, rows, {"ncand": np.zeros((2, 2))}), (sc, rows, {"program": blob[:1]}),
                     (sc, rows, {"cand_tags": torch.zeros((1, 2, 3), dtype=torch.int32)}),
                     (sc, rows, {"cand_keys": {4: rows}}), (sc, rows, {"cand_keys": {0: sc}})):
        with pytest.raises(ValueError):
            formula_rescore(s, r, **{"program": blob, "k": 3, **kw})


# ------------------------------------------------------------------ 6. routing, no search
def test_client_refusals_and_rag_arguments(monkeypatch):
    from test_groups_cpu import stub_client
    from ragmi import qdrant_models as m
    from ragmi import rag
    from ragmi.qdrant import FORMULA, FUSION, formula_params, route_of
    client, col = stub_client()
    fq = m.FormulaQuery(formula=m.SumExpression(sum=["$score", 1.0]))
    one = [m.Prefetch(query=V)]
    f = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="AMD"))])
    assert route_of(fq, one) == FORMULA and route_of(fq) == FORMULA and route_of(V, one) == FUSION
    assert formula_params(fq, m.Prefetch(query=V, filter=f, limit=7), 5) == [(V, f, 7)]
    for args, word in (((fq, None, 5), "needs prefetches to re-score"),
                       ((fq, [], 5), "needs prefetches"),
                       ((fq, [m.Prefetch(query=V)] * 17, 5), "re-scores at most 16"),
                       ((fq, [m.Prefetch(query=V, prefetch=m.Prefetch(query=V))], 5), "nested"),
                       ((fq, [m.Prefetch(query=fq)], 5), r"prefetch\[0\] needs a query"),
                       ((fq, [m.Prefetch(query=m.NearestQuery(nearest=V, mmr=m.Mmr()))], 5), "MMR"),
                       ((fq, one, 5.0), "int limit"), ((fq, [V], 5), "not a Prefetch"),
                       ((V, one, 5), "FormulaQuery")):
        with pytest.raises(ValueError, match=word):
            formula_params(*args)
    with pytest.raises(ValueError, match="belongs on each Prefetch"):
        client.query_points("t", fq, prefetch=one, query_filter=f)
    with pytest.raises(ValueError, match="needs prefetches"):
        client.query_points("t", fq)
    with pytest.raises(ValueError, match="re-scoring"):                    # the old refusal stays
        client.query_points("t", V, prefetch=one)
    with pytest.raises(ValueError, match="grouped query over prefetched"):
        client.query_points_groups("t", fq, group_by="ticker", prefetch=one)
    with pytest.raises(ValueError, match="grouped query over prefetched"):
        client.query_points_groups("t", fq, group_by="ticker")
    with pytest.raises(ValueError, match="create_payload_index"):          # compiled, then refused
        client.query_points("t", m.FormulaQuery(formula="fiscal_year"), prefetch=one)
    with pytest.raises(ValueError, match=r"\$score\[i\]"):
        client.query_batch_points("t", [m.QueryRequest(query=V), m.QueryRequest(
            query=m.FormulaQuery(formula="$score"), prefetch=one * 2)])
    assert col.index.calls == [] and col.coalescer.requests == 0
    never = m.Filter(must=[m.FieldCondition(key="ticker", match=m.MatchValue(value="NONE"))])
    assert client.query_points("t", fq, prefetch=one, limit=0).points == []
    two = m.FormulaQuery(formula=m.SumExpression(sum=["$score[0]", "$score[1]"]))
    assert client.query_points("t", two, prefetch=[m.Prefetch(query=V, filter=never),
                                                   m.Prefetch(query=V, limit=0)]).points == []
    assert col.index.calls == [] and col.coalescer.requests == 0
    col.index.count = 5000
    with pytest.raises(ValueError, match="4800.*4096"):                    # 16 x 300 entries
        client.query_points("t", m.FormulaQuery(formula="$score[3]", defaults={"$score[3]": 0}),
                            prefetch=[m.Prefetch(query=V, limit=300)] * 16)
    col.index.count = 40
    assert col.index.calls == []
    # rag: the recency formula, and what it cannot be combined with
    monkeypatch.setenv("TESTING", "False")
    for kw in ({"rewrites": [V]}, {"diversity": 0.5}, {"candidates": 100}):
        with pytest.raises(ValueError, match="recency"):
            rag.retrieve_from_qdrant(V, "AMD", recency=(30, 0.25), **kw)
        with pytest.raises(ValueError, match="recency"):
            rag.retrieve_batch([V], ["AMD"], recency=(30, 0.25),
                               **{k: ([v] if k == "rewrites" else v) for k, v in kw.items()})
    now = dt.datetime(2024, 6, 1, tzinfo=UTC)
    q, pre = rag._recency(V, (30, 0.25), now, rag._filter("amd"), 15, None, None, None)
    assert q == m.FormulaQuery(
        formula=m.SumExpression(sum=["$score", m.MultExpression(mult=[0.25, m.ExpDecayExpression(
            exp_decay=m.DecayParamsExpression(
                x=m.DatetimeKeyExpression(datetime_key="ingested_at"),
                target=m.DatetimeExpression(datetime=now), scale=30 * 86400.0, midpoint=0.5))])]),
        defaults={"ingested_at": "1970-01-01T00:00:00Z"})
    assert len(pre) == 1 and pre[0].limit == 50 and pre[0].filter == rag._filter("AMD")
    assert rag._recency(V, (7, 1), None, None, 80, None, None, None)[1][0].limit == 80
