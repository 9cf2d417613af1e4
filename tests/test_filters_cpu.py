"""CPU tests of the filter algebra (ragmi.filters): compiled programs and their
packed blob against a plain evaluator that walks the Filter over a payload dict, the
reductions and refusals, Collection.compile_filter's legacy path, and the client's routing
(slot sharing, the > 32-program split, mixed batches, the out-of-scope refusals) over a stand-in
index."""
import itertools
import os
import re

import numpy as np
import pytest

import _stubs as S
from _filters_ref import absent, cond_matches, matches   # noqa: F401
from conftest import ROOT

TICKERS = ["AAPL", "MSFT", "AMD", "NVDA", "INTC", "TSM"]
TYPES = ["10-K", "10-Q", "8-K", "DEF14A"]
FIELDS = ("ticker", "document_type")
VALUES = {"ticker": TICKERS, "document_type": TYPES}


# ------------------------------------------------------------------ fixtures
def ingested_tags():
    """PayloadTags after ingesting every (ticker, type) pair: ticker codes 1..6, type 1..4."""
    from ragmi.qdrant import PayloadTags
    tags = PayloadTags(FIELDS)
    for t, d in itertools.product(TICKERS, TYPES):
        tags.tag({"ticker": t, "document_type": d})
    return tags


def payload_of(c0, c1, variant=0):
    """A payload whose tag is c0 | c1 << 16; code 0 is an absent field, in one of the forms
    PayloadTags.code maps to 0: missing, None, a list, a dict."""
    p = {}
    for key, c in (("ticker", c0), ("document_type", c1)):
        if c:
            p[key] = VALUES[key][c - 1]
        elif variant % 4 == 1:
            p[key] = None
        elif variant % 4 == 2:
            p[key] = ["AAPL", "MSFT"]
        elif variant % 4 == 3:
            p[key] = {"a": 1}
    return p


def random_condition(rng, depth):
    from ragmi import qdrant_models as m
    kind = rng.integers(0, 6 if depth < 3 else 5)
    key = FIELDS[rng.integers(0, 2)]
    pool = VALUES[key] + ["NEVER-INGESTED"]
    pick = lambda n: [pool[i] for i in rng.choice(len(pool), n, replace=False)]
    if kind == 0:
        return m.FieldCondition(key=key, match=m.MatchValue(value=pick(1)[0]))
    if kind == 1:
        return m.FieldCondition(key=key, match=m.MatchAny(any=pick(rng.integers(0, 4))))
    if kind == 2:
        return m.FieldCondition(key=key, match=m.MatchExcept(except_=pick(rng.integers(0, 4))))
    if kind in (3, 4):
        return m.IsEmptyCondition(is_empty=m.PayloadField(key=key))
    return random_filter(rng, depth + 1)


def random_filter(rng, depth=1):
    from ragmi import qdrant_models as m
    conds = lambda hi: [random_condition(rng, depth) for _ in range(rng.integers(0, hi))]
    f = m.Filter()
    which = rng.integers(0, 16) or 15
    if which & 1:
        f.must = conds(3)
    if which & 2:
        f.should = conds(3)
    if which & 4:
        f.must_not = conds(3)
    if which & 8:
        cs = conds(4)
        f.min_should = m.MinShould(conditions=cs, min_count=int(rng.integers(0, len(cs) + 2)))
    return f


def all_tags():
    c0, c1 = np.meshgrid(np.arange(len(TICKERS) + 1), np.arange(len(TYPES) + 1), indexing="ij")
    return c0.reshape(-1), c1.reshape(-1)


def view_bits(compiled, tag_words):
    """What a compiled filter says about each tag, through the packed blob."""
    from ragmi.filters import FilterProgram, eval_view_np, pack_view
    if compiled is None:
        return np.zeros(len(tag_words), bool)
    if compiled == (0, 0):
        return np.ones(len(tag_words), bool)
    assert isinstance(compiled, FilterProgram)
    bits = eval_view_np(pack_view([compiled]), tag_words)
    assert ((bits == 0) | (bits == 1)).all()
    assert [compiled.passes(int(t)) for t in tag_words] == bits.astype(bool).tolist()
    return bits.astype(bool)


# ------------------------------------------------------------------ 1. trees vs brute force
def test_random_filter_trees_match_the_plain_evaluator():
    from ragmi.filters import UnsupportedFilter, compile_program
    tags = ingested_tags()
    c0, c1 = all_tags()
    words = (c0 | (c1 << 16)).astype(np.uint32)
    rng = np.random.default_rng(7)
    done = too_wide = programs = 0
    kinds = set()
    while done < 400:
        flt = random_filter(rng)
        try:
            compiled = compile_program(tags, flt)
        except UnsupportedFilter as e:
            assert "atoms" in str(e)
            too_wide += 1
            continue
        got = view_bits(compiled, words)
        for variant in range(4):
            want = [matches(flt, payload_of(a, b, variant)) for a, b in zip(c0, c1)]
            assert got.tolist() == want, flt
        # the payloads really carry those tags
        assert all(tags.tag(payload_of(a, b, 2)) == w for a, b, w in zip(c0, c1, words))
        programs += not isinstance(compiled, tuple) and compiled is not None
        kinds.add(type(compiled).__name__)
        done += 1
    assert programs > 200 and too_wide < done
    assert kinds == {"FilterProgram", "tuple", "NoneType"}


def test_named_shapes():
    """The shapes the corpus asks for, spelled out."""
    from ragmi import qdrant_models as m
    from ragmi.filters import FilterProgram, compile_program
    tags = ingested_tags()
    c0, c1 = all_tags()
    words = (c0 | (c1 << 16)).astype(np.uint32)
    fc = m.FieldCondition
    two = compile_program(tags, m.Filter(must=[fc("ticker", m.MatchAny(any=["AAPL", "MSFT"]))]))
    assert isinstance(two, FilterProgram) and len(two.atoms) == 1 and two.atoms[0][0] == "inset"
    assert view_bits(two, words).tolist() == [a in (1, 2) for a in c0]
    not8k = compile_program(tags, m.Filter(must_not=[fc("document_type", m.MatchValue("8-K"))]))
    assert view_bits(not8k, words).tolist() == [b != 3 for b in c1]        # absent passes
    kq = compile_program(tags, m.Filter(should=[fc("document_type", m.MatchValue("10-K")),
                                                fc("document_type", m.MatchValue("10-Q"))]))
    assert view_bits(kq, words).tolist() == [b in (1, 2) for b in c1]
    # syntactically equal atoms are shared
    twice = compile_program(tags, m.Filter(
        must=[fc("ticker", m.MatchAny(any=["AAPL", "AMD"]))],
        should=[fc("ticker", m.MatchAny(any=["AAPL", "AMD"])), fc("document_type", m.MatchValue("8-K"))]))
    assert len(twice.atoms) == 2


def test_reductions_and_refusals():
    from ragmi import qdrant_models as m
    from ragmi.filters import MAX_ATOMS, FilterProgram, UnsupportedFilter, compile_program
    tags = ingested_tags()
    fc = m.FieldCondition
    aapl = fc("ticker", m.MatchValue("AAPL"))
    assert compile_program(tags, None) == (0, 0)
    assert compile_program(tags, m.Filter()) == (0, 0)
    assert compile_program(tags, m.Filter(must=[], should=[], must_not=[])) == (0, 0)
    # constant true / false, found by the truth table, not by the syntax
    assert compile_program(tags, m.Filter(should=[aapl, m.Filter(must_not=[aapl])])) == (0, 0)
    assert compile_program(tags, m.Filter(must=[aapl], must_not=[aapl])) is None
    assert compile_program(tags, m.Filter(must=[fc("ticker", m.MatchAny(any=[]))])) is None
    assert compile_program(tags, m.Filter(must=[fc("ticker", m.MatchValue("NOPE"))])) is None
    assert compile_program(tags, m.Filter(must=[fc("ticker", m.MatchAny(any=["NOPE"]))])) is None
    # a never-ingested value is simply in no set
    p = compile_program(tags, m.Filter(must=[fc("ticker", m.MatchAny(any=["NOPE", "AMD"]))]))
    q = compile_program(tags, m.Filter(must=[fc("ticker", m.MatchAny(any=["AMD"]))]))
    assert p == q and isinstance(p, FilterProgram)
    # except of unknown values: present
    e = compile_program(tags, m.Filter(must=[fc("ticker", m.MatchExcept(except_=["NOPE"]))]))
    assert e.passes(3) and not e.passes(0) and not e.passes(2 << 16)
    assert compile_program(tags, m.Filter(min_should=m.MinShould([aapl], 2))) is None
    assert compile_program(tags, m.Filter(min_should=m.MinShould([], 0))) == (0, 0)
    # 8 atoms fit, 9 do not
    vals = [fc("ticker", m.MatchValue(t)) for t in TICKERS] + \
           [fc("document_type", m.MatchValue(t)) for t in TYPES]
    assert MAX_ATOMS == 8
    eight = compile_program(tags, m.Filter(min_should=m.MinShould(vals[:8], 2)))
    assert len(eight.atoms) == 8
    with pytest.raises(UnsupportedFilter, match="9 distinct atoms"):
        compile_program(tags, m.Filter(min_should=m.MinShould(vals[:9], 2)))
    with pytest.raises(UnsupportedFilter, match="range"):
        compile_program(tags, m.Filter(should=[fc("ticker", range={"gte": 1})]))
    with pytest.raises(UnsupportedFilter, match="'text'"):
        compile_program(tags, m.Filter(should=[fc("text", m.MatchValue("x"))]))
    with pytest.raises(UnsupportedFilter, match="'sector'"):
        compile_program(tags, m.Filter(must_not=[m.IsEmptyCondition(m.PayloadField("sector"))]))

    class HasIdCondition:
        has_id = [1]

    class MatchText:
        text = "x"

    with pytest.raises(UnsupportedFilter, match="HasIdCondition"):
        compile_program(tags, m.Filter(must_not=[HasIdCondition()]))
    with pytest.raises(UnsupportedFilter, match="MatchText"):
        compile_program(tags, m.Filter(should=[fc("ticker", MatchText())]))


def test_pack_view_layout_and_guards():
    """The blob of include/ragmi.h: records of 41 words, then the bitmap pool; eval_view_np
    follows the kernel's guards on a malformed blob."""
    from ragmi.filters import (ATOM_INSET, MAX_PROGRAMS, REC_WORDS, FilterProgram, eval_view_np,
                               pack_view, view_programs)
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    for name, v in (("RAG_FILTER_MAX_ATOMS", 8), ("RAG_FILTER_MAX_PROGRAMS", MAX_PROGRAMS),
                    ("RAG_FILTER_REC_WORDS", REC_WORDS), ("RAG_FILTER_ATOM_INSET", ATOM_INSET)):
        assert re.search(rf"#define {name} {v}\b", hdr), name
    a = FilterProgram((("inset", 0, 0b0110, 7), ("maskeq", 0xFFFF0000, 0)), 0b1000)
    b = FilterProgram((("inset", 1, 1 << 40, 41),), 0b01)
    c = FilterProgram((("inset", 0, 0b0110, 7),), 0b10)          # a's bitmap, stored once
    blob = pack_view([a, b, c])
    assert blob.dtype == np.uint32 and len(blob) == 3 * REC_WORDS + 1 + 2
    assert view_programs(blob) == 3 and view_programs(pack_view([FilterProgram.maskeq(1, 1)])) == 1
    assert blob[0] == 2 and blob[1] == 0b1000 and list(blob[9:13]) == [1, 0, 3 * REC_WORDS, 7]
    assert list(blob[2 * REC_WORDS + 9:2 * REC_WORDS + 13]) == [1, 0, 3 * REC_WORDS, 7]
    tags = np.array([1, 2, 3, 2 | (5 << 16), 40 << 16, 41 << 16, 0], np.uint32)
    want = [[p.passes(int(t)) for p in (a, b, c)] for t in tags]
    got = eval_view_np(blob, tags)
    assert [[bool(g >> s & 1) for s in range(3)] for g in got] == want
    assert got.tolist() == [0b111, 0b111, 0b010, 0b110, 0b000, 0b010, 0b010]
    with pytest.raises(ValueError):
        pack_view([a] * (MAX_PROGRAMS + 1))
    with pytest.raises(ValueError):
        pack_view([])
    # an offset past the blob, a length past the pool, an atom count past 8: no IndexError,
    # and the out-of-blob word reads as "not a member"
    bad = pack_view([c]).copy()
    bad[11] = 0xFFFFFFF0
    assert eval_view_np(bad, tags, 1).tolist() == [0] * len(tags)
    bad = pack_view([c]).copy()
    bad[12] = 0xFFFF                                              # claims 65535 bits
    assert eval_view_np(bad, np.array([1, 2, 40, 65535], np.uint32), 1).tolist() == [1, 1, 0, 0]
    bad = pack_view([c]).copy()
    bad[0] = 1000
    assert eval_view_np(bad, tags, 1).shape == tags.shape


def test_abi_is_declared_and_bound():
    from ragmi import _lib
    hdr = open(os.path.join(ROOT, "include", "ragmi.h")).read()
    for name in ("rag_index_filter_view", "rag_index_search_view", "rag_index_select_rows_view",
                 "rag_shardset_search_view"):
        assert name in _lib.INDEX_API
        decl = re.search(rf"int {name}\(([^;]*)\);", hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.INDEX_API[name][1]), name
    from _index_src import index_host_source
    assert '#include "filter_kernels.hip"' in index_host_source()


# ------------------------------------------------------------------ 2. compile_filter
def legacy_filters():
    from ragmi import qdrant_models as m
    fc = m.FieldCondition
    return [None, m.Filter(), m.Filter(must=[]),
            m.Filter(must=[fc("ticker", m.MatchValue("AMD"))]),
            m.Filter(must=[fc("document_type", m.MatchValue("10-Q"))]),
            m.Filter(must=[fc("ticker", m.MatchValue("TSM")), fc("document_type", m.MatchValue("8-K"))]),
            m.Filter(must=[fc("ticker", m.MatchValue("NOPE"))]),
            m.Filter(must=[fc("ticker", m.MatchValue("AMD")), fc("ticker", m.MatchValue("TSM"))]),
            m.Filter(must=[fc("ticker", m.MatchValue("AMD")), fc("ticker", m.MatchValue("AMD"))])]


def bare_collection():
    return S.stub_collection(_StubIndex([]), dim=2, tags=ingested_tags())


def test_compile_filter_keeps_the_legacy_path():
    from ragmi import qdrant_models as m
    from ragmi.filters import FilterProgram
    from ragmi.qdrant import UnsupportedFilter
    col = bare_collection()
    for f in legacy_filters():
        want = col.tags.compile(f)
        got = col.compile_filter(f)
        assert got == want and type(got) is type(want), f
    fc = m.FieldCondition
    # PayloadTags.compile still refuses what it refused
    for f in (m.Filter(should=[fc("ticker", m.MatchValue("AMD"))]),
              m.Filter(must=[fc("ticker", m.MatchAny(any=["AMD"]))]),
              m.Filter(must=[m.Filter()])):
        with pytest.raises(UnsupportedFilter):
            col.tags.compile(f)
        assert isinstance(col.compile_filter(f), (FilterProgram, tuple))
    # min_should, which PayloadTags.compile never looked at, is honoured
    amd = fc("ticker", m.MatchValue("AMD"))
    both = m.Filter(must=[amd], min_should=m.MinShould([fc("document_type", m.MatchValue("8-K"))], 1))
    assert col.tags.compile(both) == col.tags.compile(m.Filter(must=[amd]))
    prog = col.compile_filter(both)
    code = lambda t, d: col.tags.tag({"ticker": t, "document_type": d})
    assert prog.passes(code("AMD", "8-K")) and not prog.passes(code("AMD", "10-K"))
    assert col.compile_filter(m.Filter(min_should=m.MinShould([amd], 2))) is None
    # an unknown key and a range stay refused
    with pytest.raises(UnsupportedFilter, match="'text'"):
        col.compile_filter(m.Filter(must=[fc("text", m.MatchValue("x"))]))
    with pytest.raises(UnsupportedFilter):
        col.compile_filter(m.Filter(must=[fc("ticker", range={"gte": 1})]))


# ------------------------------------------------------------------ 3. routing over a stand-in
class _StubIndex:
    """FlatIndex stand-in: a search answers every query with the rows passing its filter over
    the tag column (the stored tags, or eval_view_np's view of them under `programs`), in row
    order, and records the call."""
    device = None

    def __init__(self, tags):
        self.tag = np.asarray(tags, np.uint32)
        self.calls = []
        self.selects = []

    @property
    def count(self):
        return len(self.tag)

    def unanswered(self):
        return 0

    def search(self, q, k, filters=None, full=False, programs=None, n_programs=None,
               rescue=False):
        import torch
        from ragmi.filters import eval_view_np, view_programs
        col = self.tag if programs is None else eval_view_np(programs, self.tag)
        B = len(q)
        self.calls.append({"B": B, "U": None if programs is None else view_programs(programs),
                           "filters": None if filters is None else np.array(filters),
                           "q": np.array(q)})
        s = np.full((B, k), -np.inf, np.float32)
        ids = np.full((B, k), -1, np.int64)
        for b in range(B):
            mask, value = (0, 0) if filters is None else (int(x) for x in filters[b])
            rows = np.nonzero((col & np.uint32(mask)) == np.uint32(value))[0][:k]
            ids[b, :len(rows)] = rows
            s[b, :len(rows)] = 1.0 - 1e-3 * rows - float(q[b][0])
        return torch.from_numpy(s), torch.from_numpy(ids)

    def select_rows(self, mask, value, cap=None):
        raise AssertionError("the legacy select is not the route of a general filter")

    def select_rows_view(self, programs, cap=None):
        from ragmi.filters import eval_view_np
        self.selects.append(cap)
        return None, int((eval_view_np(programs, self.tag, 1) & 1).sum())


def routed_collection():
    rng = np.random.default_rng(3)
    n = 500
    payloads = [payload_of(int(rng.integers(0, 7)), int(rng.integers(0, 5)), int(v))
                for v in rng.integers(0, 4, n)]
    tags = ingested_tags()
    return S.stub_collection(_StubIndex([tags.tag(p) for p in payloads]), dim=2,
                             payloads=payloads, tags=tags)


def brute(col, flt, k):
    return [r for r, p in enumerate(col.payloads) if flt is None or matches(flt, p)][:k]


def run(col, flts, k=7):
    q = np.arange(len(flts), dtype=np.float32).reshape(-1, 1).repeat(2, axis=1)
    out = col.search(q, k, [col.compile_filter(f) for f in flts])
    for j, (f, hits) in enumerate(zip(flts, out)):
        assert [r for r, _ in hits] == brute(col, f, k), (j, f)
        # every hit's score carries its own query: nothing was scattered to the wrong place
        assert all(abs(s - (1.0 - 1e-3 * r - j)) < 1e-4 for r, s in hits)
    return out


def test_routing_shares_slots_and_leaves_the_legacy_path_alone():
    from ragmi import qdrant_models as m
    col = routed_collection()
    fc = m.FieldCondition
    any2 = m.Filter(must=[fc("ticker", m.MatchAny(any=["AAPL", "MSFT"]))])
    not8k = m.Filter(must_not=[fc("document_type", m.MatchValue("8-K"))])
    amd = m.Filter(must=[fc("ticker", m.MatchValue("AMD"))])
    nope = m.Filter(must=[fc("ticker", m.MatchValue("NOPE"))])
    # legacy filters only: the legacy call, no blob
    run(col, [amd, None, nope, amd])
    assert [c["U"] for c in col.index.calls] == [None] and col.index.calls[0]["B"] == 3
    col.index.calls.clear()
    run(col, [None, None])
    assert col.index.calls[0]["filters"] is None and col.index.calls[0]["U"] is None
    col.index.calls.clear()
    # a mixed batch: one view call, equal programs share a bit, (0, 0) takes none, a filter
    # that can match nothing is not sent
    run(col, [any2, amd, None, not8k, any2, nope, amd, m.Filter(must=[m.Filter(must=[not8k])])])
    (call,) = col.index.calls
    assert call["B"] == 7 and call["U"] == 3
    assert call["filters"].tolist() == [[1, 1], [2, 2], [0, 0], [4, 4], [1, 1], [2, 2], [4, 4]]


def test_routing_splits_more_than_32_distinct_programs():
    from ragmi import qdrant_models as m
    col = routed_collection()
    fc = m.FieldCondition
    subsets = [c for n in (1, 2, 3) for c in itertools.combinations(TICKERS, n)][:40]
    flts = [m.Filter(must=[fc("ticker", m.MatchAny(any=list(c)))],
                     must_not=[fc("document_type", m.MatchValue("8-K"))]) for c in subsets]
    assert len({col.compile_filter(f) for f in flts}) == 40
    order = [0, 39, 5, 33, 5] + list(range(40)) + [None, 38]
    run(col, [None if i is None else flts[i] for i in order])
    calls = col.index.calls
    assert [c["U"] for c in calls] == [32, 8]
    assert sum(c["B"] for c in calls) == len(order)
    for c in calls:
        bits = c["filters"][:, 0]
        assert (c["filters"][:, 0] == c["filters"][:, 1]).all()
        assert all(b == 0 or (b & (b - 1)) == 0 for b in bits.tolist())
        assert len(set(bits.tolist()) - {0}) == c["U"]


def test_count_and_the_out_of_scope_refusals():
    from ragmi import qdrant_models as m
    from ragmi.qdrant import UnsupportedFilter
    col = routed_collection()
    fc = m.FieldCondition
    flt = m.Filter(must=[fc("ticker", m.MatchAny(any=["AAPL", "MSFT"]))],
                   must_not=[fc("document_type", m.MatchValue("8-K"))])
    assert col.count_matching(flt) == len(brute(col, flt, 10 ** 9)) > 0
    assert col.index.selects == [0]
    assert col.count_matching(m.Filter(should=[])) == len(col.payloads)
    assert col.count_matching(m.Filter(must=[fc("ticker", m.MatchAny(any=[]))])) == 0
    with pytest.raises(UnsupportedFilter, match="Collection.delete"):
        col.delete(m.FilterSelector(filter=flt))
    with pytest.raises(UnsupportedFilter, match="Collection.delete"):
        col.delete(m.Filter(should=[fc("ticker", m.MatchValue("AMD"))]))
    with pytest.raises(UnsupportedFilter, match="Collection.delete"):
        col.delete(m.Filter(min_should=m.MinShould([fc("ticker", m.MatchValue("AMD"))], 1)))
    with pytest.raises(UnsupportedFilter, match="query_points_groups"):
        col.search_groups(np.zeros((1, 2), np.float32), "ticker", 3, 2, [col.compile_filter(flt)])
    assert len(col.payloads) == 500


def test_rag_filter_takes_lists():
    from ragmi import qdrant_models as m
    from ragmi import rag
    f = rag._filter("aapl", "10-k")
    assert f == m.Filter(must=[m.FieldCondition("ticker", m.MatchValue("AAPL")),
                               m.FieldCondition("document_type", m.MatchValue("10-K"))])
    assert rag._filter("aapl") == m.Filter(must=[m.FieldCondition("ticker", m.MatchValue("AAPL"))])
    g = rag._filter(["aapl", "msft"], ("10-k", "10-q"))
    assert g.must[0].match == m.MatchAny(any=["AAPL", "MSFT"])
    assert g.must[1].match == m.MatchAny(any=["10-K", "10-Q"])
