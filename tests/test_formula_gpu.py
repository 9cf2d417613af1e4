"""GPU tests of formula queries (rag_formula_rescore / formula_rescore_kernel,
ragmi.index.formula_rescore, Collection.search_formula behind QdrantClient.query_points /
query_batch_points, ragmi.rag's recency): values bit-equal (as uint32), rows, counts and status
equal to the numpy restatement of tests/_formula_ref.py — on synthetic lists, on FlatIndex lists
of the 3001-row range corpus — and through the client against the independent tree walker applied
to separate query_points calls."""
import ctypes
import datetime as dt

import numpy as np
import pytest
import torch

import _formula_ref as F
import oracle_scan as O
import test_range_gpu as R

pytestmark = pytest.mark.gpu

UTC = dt.timezone.utc
CANARY = 0x5A5A5A5A


def ops_blob(*ops, programs=()):
    from ragmi.formula import pack_formula
    return pack_formula(list(ops), programs)


def score_blob():
    from ragmi import formula as fm
    return ops_blob((fm.SCORE, 0, 0, 0.0))


def keys_of(values):
    """The keys of doubles (None = absent), any shape."""
    from ragmi.filters import KEY_ABSENT, key_of_float
    a = np.asarray(values, dtype=object)
    return np.array([KEY_ABSENT if v is None else key_of_float(v) for v in a.reshape(-1)],
                    np.int64).reshape(a.shape)


def rescored(gpu, s, r, blob, k, ncand=None, tags=None, keys=None):
    """formula_rescore over host lists, back on the host: (scores, rows, count, status)."""
    from ragmi.index import formula_rescore
    dev = lambda a, t: None if a is None else torch.as_tensor(np.ascontiguousarray(a).view(t),
                                                              device=gpu)
    keys = {c: dev(x, np.int64) for c, x in (keys or {}).items()}
    out = formula_rescore(dev(np.asarray(s, np.float32), np.float32),
                          dev(np.asarray(r, np.int64), np.int64), blob, k, ncand,
                          dev(None if tags is None else np.asarray(tags, np.uint32), np.int32),
                          keys, with_count=True)
    torch.cuda.synchronize()
    vs, vr, st, cnt = (x.cpu().numpy() for x in out)
    return vs, vr, cnt, st.view(np.uint32)


def same(got, want):
    """status and counts always; values and rows where the status is 0 (else unspecified)."""
    assert np.array_equal(got[3], want[3]), (got[3], want[3])
    assert np.array_equal(got[2], want[2])
    ok = want[3] == 0
    assert np.array_equal(got[1][ok], want[1][ok])
    assert np.array_equal(F.bits(got[0][ok]), F.bits(want[0][ok]))


def check(gpu, s, r, blob, k, ncand=None, tags=None, keys=None):
    got = rescored(gpu, s, r, blob, k, ncand, tags, keys)
    host = ncand.cpu().numpy() if isinstance(ncand, torch.Tensor) else ncand
    want = F.rescore(s, r, blob, k, host, tags, keys)
    same(got, want)
    return got


# ------------------------------------------------------------------ 1. the kernel, synthetic lists
def test_one_pick_then_padding_an_empty_list_and_no_request(gpu):
    from ragmi.index import formula_rescore
    got = check(gpu, [[[0.75]]], [[[5]]], score_blob(), 3)
    assert got[1].tolist() == [[5, -1, -1]] and got[2].tolist() == [1] and got[3].tolist() == [0]
    assert got[0][0, 0] == np.float32(0.75) and np.isneginf(got[0][0, 1:]).all()
    got = check(gpu, [[[0.75]]], [[[-1]]], score_blob(), 3)            # an empty list
    assert got[1].tolist() == [[-1, -1, -1]] and got[2].tolist() == [0] and got[3].tolist() == [0]
    out = formula_rescore(torch.zeros((0, 3, 20), device=gpu),
                          torch.zeros((0, 3, 20), dtype=torch.int64, device=gpu), score_blob(), 15)
    assert [tuple(x.shape) for x in out] == [(0, 15), (0, 15), (0,)]      # no count asked for
    assert [x.dtype for x in out] == [torch.float32, torch.int64, torch.int32]


def test_ties_signs_and_zeros_order_as_the_values_do(gpu):
    rows = np.array([[[7, 9, 5, 3], [9, 7, 1, 2]]], np.int64)
    sc = np.array([[[0.5, 0.5, 0.25, -0.0], [9, 9, 0.0, -1e-30]]], np.float32)
    check(gpu, sc, rows, score_blob(), 8)          # rows of list 1 alone have no $score[0]
    from ragmi import formula as fm
    both = ops_blob((fm.SCORE, 0, 1, -0.125), (fm.SCORE, 1, 1, 0.0), (fm.NEG, 0, 0, 0.0),
                    (fm.MUL, 0, 0, 0.0))
    got = check(gpu, sc, rows, both, 8)
    assert got[3].tolist() == [0] and got[2].tolist() == [6]
    # an exact tie goes to the smaller row; negatives below zeros below positives; -0.0 is +0.0
    rng = np.random.default_rng(0)
    vals = np.concatenate([[0.0, -0.0, 1e-45, -1e-45, 1.5, 1.5, -1.5, -1.5, 3e38, -3e38],
                           rng.standard_normal(54) * 10.0 ** rng.integers(-30, 30, 54)])
    rows = rng.permutation(1000)[:64].reshape(1, 1, 64).astype(np.int64)
    got = check(gpu, vals.astype(np.float32).reshape(1, 1, 64), rows, score_blob(), 64)
    v = got[0][0]
    assert (np.diff(v) <= 0).all() and (v < 0).any() and (v > 0).any()
    zero = np.nonzero(v == 0)[0]
    assert len(zero) == 2 and F.bits(v[zero]).tolist() == [0, 0]
    assert got[1][0, zero[0]] < got[1][0, zero[1]]
    pair = np.nonzero(v == np.float32(1.5))[0]
    assert got[1][0, pair[0]] < got[1][0, pair[1]]


def test_ragged_lists_defaults_and_the_missing_flag(gpu):
    from ragmi import formula as fm
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 120, (4, 3, 100)).astype(np.int64)
    rows[1, 0, 50] = -1                                     # ends its list mid-way
    sc = rng.standard_normal((4, 3, 100)).astype(np.float32)
    ncand = np.array([[100, 37, 0], [100, 1, 100], [0, 0, 0], [100, 100, 100]], np.int32)
    weighted = lambda fl: ops_blob(
        (fm.CONST, 0, 0, 0.5), (fm.SCORE, 0, fl, -1.0), (fm.MUL, 0, 0, 0.0),
        (fm.CONST, 0, 0, 0.25), (fm.SCORE, 1, fl, 0.0), (fm.MUL, 0, 0, 0.0), (fm.ADD, 0, 0, 0.0),
        (fm.SCORE, 2, fl, 2.0), (fm.ADD, 0, 0, 0.0))
    assert F.list_lengths(rows, ncand)[1].tolist() == [50, 1, 100]
    got = check(gpu, sc, rows, weighted(1), 15, ncand)
    assert got[3].tolist() == [0, 0, 0, 0] and got[2][2] == 0
    got = check(gpu, sc, rows, weighted(0), 15, ncand)
    # request 2 has no candidate, so nothing can be missing there
    assert got[3].tolist() == [F.MISSING, F.MISSING, 0, F.MISSING]
    check(gpu, sc, rows, weighted(1), 15, torch.as_tensor(ncand, device=gpu))
    check(gpu, sc, rows, weighted(1), 15)
    odd = np.array([[150, -4, 100]] * 4, np.int32)          # clamped counts
    check(gpu, sc, rows, weighted(1), 40, odd)
    # every row in every list: nothing is missing without defaults either
    full = np.stack([np.stack([rng.permutation(100) for _ in range(3)]) for _ in range(2)])
    got = check(gpu, sc[:2], full.astype(np.int64), weighted(0), 100)
    assert got[3].tolist() == [0, 0] and got[2].tolist() == [100, 100]


def decay_case(n, rng):
    """n arguments d >= 0 of a decay, from 0 past 700, as a [1, 1, n] request."""
    d = np.concatenate([[0.0, 1e-300, 0.5, 1.0, 10.0, 100.0, 699.999, 700.0,
                         np.nextafter(700.0, 800.0), 701.0, 1e6, np.inf],
                        700.0 * rng.random(n - 12)])
    rows = rng.permutation(1 << 20)[:n].reshape(1, 1, n).astype(np.int64)
    return d, rows, np.zeros((1, 1, n), np.float32)


def test_decay_exponential_bit_for_bit_in_fp64(gpu):
    """E's fp64 result checked to the last bit through three fp32 outputs: E itself, E minus its
    fp32 rounding (a key column), and that minus its own rounding; each difference is exact in
    fp64, so one differing bit anywhere in E's 53 shows in one of them."""
    from ragmi import formula as fm
    rng = np.random.default_rng(3)
    d, rows, sc = decay_case(4096, rng)
    for kind, d in ((fm.EXP, d), (fm.GAUSS, d / 26.4)):       # gauss: d * d runs to 703
        with np.errstate(all="ignore"):
            e = F.E(-d if kind == fm.EXP else -(d * d))
            hi1 = e.astype(np.float32).astype(np.float64)
            hi2 = (e - hi1).astype(np.float32).astype(np.float64)
        keys = {0: keys_of(d).reshape(1, 1, -1), 1: keys_of(hi1).reshape(1, 1, -1),
                2: keys_of(hi2).reshape(1, 1, -1)}
        head = [(fm.KEY, 0, 0, 0.0), (fm.CONST, 0, 0, 0.0), (kind, 0, 0, -1.0)]
        minus = lambda c: [(fm.KEY, c, 0, 0.0), (fm.NEG, 0, 0, 0.0), (fm.ADD, 0, 0, 0.0)]
        for ops in (head, head + minus(1), head + minus(1) + minus(2)):
            got = check(gpu, sc, rows, ops_blob(*ops), 4096, keys=keys)
            assert got[3].tolist() == [0] and got[2].tolist() == [4096]
        top = rescored(gpu, sc, rows, ops_blob(*head), 4096, keys=keys)
        assert top[0][0, 0] == 1.0 and top[0][0, -1] == 0.0        # E(0) = 1, E(< -700) = 0


def test_each_op_once(gpu):
    from ragmi import formula as fm
    rng = np.random.default_rng(4)
    n = 40
    rows = rng.permutation(500)[:n].reshape(1, 1, n).astype(np.int64)
    sc = rng.standard_normal((1, 1, n)).astype(np.float32)
    x = [None if i % 7 == 3 else float(v) for i, v in
         enumerate(np.concatenate([[0.0, -0.0, 1.0, -2.5e9], rng.integers(-3, 4, n - 4)]))]
    epoch = [0, 1, 1704067200250000, 1718236800000000, None, -86400000000]
    t = [epoch[i % len(epoch)] for i in range(n)]
    keys = {0: keys_of(x).reshape(1, 1, n),
            3: keys_of([None if v is None else float(v) for v in t]).reshape(1, 1, n)}
    S, K0 = (fm.SCORE, 0, 0, 0.0), (fm.KEY, 0, 1, 0.5)
    for ops, want_status in (
            ([S, K0, (fm.DIV, 0, 1, -7.0)], 0),                       # by zero, with a default
            ([S, K0, (fm.DIV, 0, 0, 0.0)], F.NONFINITE),              # and without
            ([S, (fm.KEY, 0, 0, 0.0), (fm.ADD, 0, 0, 0.0)], F.MISSING),
            ([(fm.KEY, 3, 3, -1.0)], 0),                              # datetimes, absent -> -1
            ([(fm.KEY, 3, 2, 0.0)], F.MISSING),
            ([(fm.KEY, 3, 1, 0.0), (fm.CONST, 0, 0, 1e-6), (fm.MUL, 0, 0, 0.0)], 0),
            ([S, (fm.ABS, 0, 0, 0.0), K0, (fm.NEG, 0, 0, 0.0), (fm.MUL, 0, 0, 0.0)], 0),
            ([K0, (fm.CONST, 0, 0, 1.0), (fm.LIN, 0, 0, 0.4)], 0),    # clamped at 0 from |d| 2.5
            ([K0, S, (fm.GAUSS, 0, 0, -0.3)], 0),
            ([K0, (fm.CONST, 0, 0, 3e38), (fm.MUL, 0, 0, 0.0), (fm.CONST, 0, 0, 10.0),
              (fm.MUL, 0, 0, 0.0)], F.NONFINITE),                     # overflows fp32, not fp64
            ([(fm.CONST, 0, 0, 1.0), (fm.CONST, 0, 0, 2.0), (fm.CONST, 0, 0, 3.0),
              (fm.CONST, 0, 0, 4.0), (fm.CONST, 0, 0, 5.0), (fm.CONST, 0, 0, 6.0),
              (fm.CONST, 0, 0, 7.0), S, (fm.ADD, 0, 0, 0.0), (fm.MUL, 0, 0, 0.0),
              (fm.DIV, 0, 0, 0.0), (fm.ADD, 0, 0, 0.0), (fm.MUL, 0, 0, 0.0), (fm.DIV, 0, 0, 0.0),
              (fm.ADD, 0, 0, 0.0)], 0)):                               # the stack at its depth 8
        got = check(gpu, sc, rows, ops_blob(*ops), n, keys=keys)
        assert got[3].tolist() == [want_status], ops
    lin = rescored(gpu, sc, rows, ops_blob(K0, (fm.CONST, 0, 0, 1.0), (fm.LIN, 0, 0, 0.4)), n,
                   keys=keys)
    assert lin[0].min() == 0.0 and lin[0].max() == 1.0
    secs = rescored(gpu, sc, rows, ops_blob((fm.KEY, 3, 3, -1.0)), n, keys=keys)[0][0]
    assert set(secs.tolist()) == {float(np.float32(v)) for v in (
        0.0, 1e-6, 1704067200.25, 1718236800.0, -1.0, -86400.0)}


def test_conditions_read_the_first_entrys_tag_and_keys(gpu):
    from ragmi import formula as fm
    from ragmi import qdrant_models as m
    from ragmi.filters import PayloadRanges, PayloadTags, compile_program
    pt, pr = PayloadTags(), PayloadRanges({"year": "number", "at": "datetime"})
    rng = np.random.default_rng(5)
    pay = [{"ticker": ["A", "B", "C"][i % 3], "document_type": ["K", "Q"][i % 2],
            **({"year": 2015 + i % 10} if i % 4 else {}),
            **({"at": f"2024-0{1 + i % 9}-01"} if i % 5 else {})} for i in range(200)]
    tag = np.array([pt.tag(p) for p in pay], np.uint32)
    key = np.array([pr.keys(p) for p in pay], np.int64).T
    fc = m.FieldCondition
    progs = [compile_program(pt, f, pr) for f in (
        m.Filter(must=[fc("ticker", m.MatchAny(any=["A", "C"]))]),
        m.Filter(must=[fc("year", range=m.Range(gte=2019))],
                 must_not=[fc("document_type", m.MatchValue("Q"))]),
        m.Filter(should=[m.IsEmptyCondition(m.PayloadField("at")),
                         fc("at", range=m.DatetimeRange(lt="2024-04-01"))]))]
    rows = rng.integers(0, 200, (3, 2, 40)).astype(np.int64)
    sc = rng.standard_normal((3, 2, 40)).astype(np.float32)
    ops = [(fm.COND, 0, 0, 0.0), (fm.COND, 1, 0, 0.0), (fm.CONST, 0, 0, 2.0), (fm.MUL, 0, 0, 0.0),
           (fm.ADD, 0, 0, 0.0), (fm.COND, 2, 0, 0.0), (fm.CONST, 0, 0, 4.0), (fm.MUL, 0, 0, 0.0),
           (fm.ADD, 0, 0, 0.0)]
    blob = ops_blob(*ops, programs=progs)
    keys = {0: key[0][rows], 1: key[1][rows]}
    got = check(gpu, sc, rows, blob, 80, tags=tag[rows], keys=keys)
    assert got[3].tolist() == [0, 0, 0] and len(set(got[0].reshape(-1).tolist())) >= 5
    # a RANGE atom on a column that was not supplied is false; the tags alone still answer
    check(gpu, sc, rows, blob, 80, tags=tag[rows], keys={1: keys[1]})
    check(gpu, sc, rows, blob, 80, tags=tag[rows])
    # the slot read is the FIRST entry's: give every later entry of a row another tag and key
    first = np.zeros(rows.shape, bool)
    for b in range(3):
        seen = set()
        for e, r in enumerate(rows[b].reshape(-1)):
            first[b].reshape(-1)[e] = r not in seen
            seen.add(r)
    t2 = np.where(first, tag[rows], np.uint32(0))
    k2 = {c: np.where(first, x, -5) for c, x in keys.items()}
    again = rescored(gpu, sc, rows, blob, 80, tags=t2, keys=k2)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    # a tag array is needed: without one the program is refused
    assert rescored(gpu, sc, rows, blob, 80, keys=keys)[3].tolist() == [F.BAD] * 3


def canaried(gpu, n, dtype, pad=64):
    """n elements of `dtype` between two pads of CANARY words: (whole tensor, the n in it)."""
    whole = torch.full((n + 2 * pad,), CANARY, dtype=torch.int32, device=gpu)
    if dtype == torch.int64:
        whole = torch.full((n + 2 * pad,), (CANARY << 32) | CANARY, dtype=torch.int64, device=gpu)
    return whole, whole[pad:pad + n]


def test_bad_blobs_set_the_flag_and_write_only_the_outputs(gpu):
    """Judged by canaries around every output tensor, never by a fault: each blob below is
    refused by the kernel's own checks before an op runs."""
    from ragmi import _lib, formula as fm
    from ragmi.filters import FilterProgram
    B, L, C, k = 2, 2, 8, 5
    rng = np.random.default_rng(6)
    rows = torch.as_tensor(rng.integers(0, 12, (B, L, C)).astype(np.int64), device=gpu)
    sc = torch.as_tensor(rng.standard_normal((B, L, C)).astype(np.float32), device=gpu)
    tags = torch.zeros((B, L, C), dtype=torch.int32, device=gpu)
    col0 = torch.zeros((B, L, C), dtype=torch.int64, device=gpu)
    ptrs = (ctypes.c_void_p * 4)(col0.data_ptr(), None, None, None)
    one = FilterProgram.maskeq(0xFFFF, 1)
    S = (fm.SCORE, 0, 0, 0.0)
    many = ops_blob(*([S] + [(fm.CONST, 0, 0, 1.0), (fm.ADD, 0, 0, 0.0)] * 32))   # 65 ops
    lying = ops_blob(S)
    lying[0] = 1000                                        # more ops than words
    ten_conds = ops_blob((fm.COND, 9, 0, 0.0), programs=[one])
    ten_conds[1] = 10                                      # more programs than the limit
    cut = ops_blob((fm.COND, 0, 0, 0.0), programs=[one])[:-5]   # the record ends past the blob
    cases = {
        "65 ops": many, "an op count past the words": lying,
        "stack underflow": ops_blob(S, (fm.ADD, 0, 0, 0.0)),
        "stack overflow": ops_blob(*([S] * 9 + [(fm.ADD, 0, 0, 0.0)] * 8)),
        "two values left": ops_blob(S, S), "no op": ops_blob(),
        "column 7": ops_blob((fm.KEY, 7, 0, 0.0)), "column 2 is NULL": ops_blob((fm.KEY, 2, 0, 0.0)),
        "list 2 of 2": ops_blob((fm.SCORE, 2, 0, 0.0)),
        "program 9": ops_blob((fm.COND, 9, 0, 0.0), programs=[one]),
        "10 programs": ten_conds, "a cut record": cut, "kind 12": ops_blob((12, 0, 0, 0.0)),
        "kind 2^31": ops_blob((1 << 31, 0, 0, 0.0))}
    lib = _lib.load()
    for name, blob in cases.items():
        assert F.parse(blob, L, True, [True, False, False, False]) is None, name
        prog = torch.from_numpy(np.ascontiguousarray(blob).view(np.int32)).to(gpu)
        outs = [canaried(gpu, B * k, torch.int32), canaried(gpu, B * k, torch.int64),
                canaried(gpu, B, torch.int32), canaried(gpu, B, torch.int32)]
        with torch.cuda.device(gpu):
            rc = lib.rag_formula_rescore(
                sc.data_ptr(), rows.data_ptr(), tags.data_ptr(), ptrs, None, prog.data_ptr(),
                prog.numel(), B, L, C, k, outs[0][1].data_ptr(), outs[1][1].data_ptr(),
                outs[2][1].data_ptr(), outs[3][1].data_ptr(),
                torch.cuda.current_stream(gpu).cuda_stream)
        assert rc == 0, name
        torch.cuda.synchronize()
        for (whole, part), word in zip(outs, (CANARY, (CANARY << 32) | CANARY, CANARY, CANARY)):
            w = whole.cpu().numpy()
            assert (w[:64] == word).all() and (w[-64:] == word).all(), name
        assert outs[3][1].cpu().tolist() == [F.BAD] * B, name
        want = F.rescore(sc.cpu().numpy(), rows.cpu().numpy(), blob, k, None,
                         tags.cpu().numpy(), [col0.cpu().numpy()])
        assert outs[2][1].cpu().tolist() == want[2].tolist(), name        # the counts stand
        assert (outs[1][1].cpu().numpy() != (CANARY << 32) | CANARY).all(), name   # all written
    # the same inputs with a good program pass
    good = ops_blob((fm.SCORE, 0, 1, 0.0))
    assert rescored(gpu, sc.cpu().numpy(), rows.cpu().numpy(), good, k)[3].tolist() == [0, 0]


def test_the_full_4096_entries(gpu):
    from ragmi import formula as fm
    rng = np.random.default_rng(7)
    rows = np.empty((2, 16, 256), np.int64)
    rows[0] = rng.permutation(1 << 20)[:4096].reshape(16, 256)          # all distinct
    rows[1] = np.stack([rng.permutation(300)[:256] for _ in range(16)])  # heavily overlapping
    sc = rng.standard_normal((2, 16, 256)).astype(np.float32)
    ops = [(fm.SCORE, 0, 1, 0.0)]
    for l in range(1, 16):
        ops += [(fm.SCORE, l, 1, 0.0), (fm.CONST, 0, 0, 1.0 / (l + 1)), (fm.MUL, 0, 0, 0.0),
                (fm.ADD, 0, 0, 0.0)]
    blob = ops_blob(*ops)                                                # 61 ops
    got = check(gpu, sc, rows, blob, 4096)
    assert got[2].tolist() == [4096, 300] and got[3].tolist() == [0, 0]
    # determinism, and the prefix property
    again = rescored(gpu, sc, rows, blob, 4096)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    short = rescored(gpu, sc, rows, blob, 15)
    assert np.array_equal(short[1], got[1][:, :15])
    assert np.array_equal(F.bits(short[0]), F.bits(got[0][:, :15]))


def test_lists_and_k_past_the_block(gpu):
    from ragmi import formula as fm
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 1500, (2, 4, 600)).astype(np.int64)
    rows[1] = np.stack([rng.permutation(5000)[:600] for _ in range(4)])
    sc = rng.standard_normal((2, 4, 600)).astype(np.float32)
    ncand = np.array([[600, 513, 512, 1], [600, 600, 600, 600]], np.int32)
    blob = ops_blob((fm.SCORE, 0, 1, 0.0), (fm.SCORE, 3, 1, -1.0), (fm.ADD, 0, 0, 0.0),
                    (fm.SCORE, 1, 1, 0.5), (fm.MUL, 0, 0, 0.0))
    check(gpu, sc, rows, blob, 700, ncand)
    check(gpu, sc, rows, blob, 5000)                        # k past L * C: padding only


def test_rows_around_2_to_the_40_a_duplicate_and_33_requests(gpu):
    from ragmi import formula as fm
    rng = np.random.default_rng(9)
    rows = (1 << 40) + rng.integers(-40, 40, (2, 3, 30)).astype(np.int64)
    rows[0, 1, :4] = [2**62, 0, 2**63 - 1, 2**31]
    sc = rng.standard_normal((2, 3, 30)).astype(np.float32)
    blob = ops_blob((fm.SCORE, 0, 1, 0.0), (fm.SCORE, 1, 1, 0.0), (fm.ADD, 0, 0, 0.0),
                    (fm.SCORE, 2, 1, 0.0), (fm.ADD, 0, 0, 0.0))
    check(gpu, sc, rows, blob, 90)
    # the same row twice in one list contributes its first occurrence
    got = check(gpu, [[[1.0, 5.0, 3.0]]], [[[4, 8, 4]]], score_blob(), 3)
    assert got[1].tolist() == [[8, 4, -1]] and got[0][0, :2].tolist() == [5.0, 1.0]
    rows = rng.integers(0, 50, (33, 3, 20)).astype(np.int64)
    sc = rng.standard_normal((33, 3, 20)).astype(np.float32)
    ncand = rng.integers(0, 21, (33, 3)).astype(np.int32)
    check(gpu, sc, rows, blob, 15, ncand)


# ------------------------------------------------------------------ 2. through the index
def formulas(now="2024-09-01T00:00:00Z"):
    """The three request shapes of the client tests: (FormulaQuery, number of prefetches)."""
    from ragmi import qdrant_models as m
    from ragmi import rag
    recency = rag._recency(None, (30, 0.25), now, None, 15, None, None, None)[0]
    bonus = m.FormulaQuery(formula=m.SumExpression(sum=["$score", m.MultExpression(mult=[
        0.1, m.FieldCondition(key="document_type", match=m.MatchValue(value="10-K"))])]))
    weighted = m.FormulaQuery(
        formula=m.SumExpression(sum=[m.MultExpression(mult=[0.7, "$score[0]"]),
                                     m.MultExpression(mult=[0.3, "$score[1]"]),
                                     m.MultExpression(mult=[1e-3, "pages"])]),
        defaults={"$score[0]": 0.0, "$score[1]": -0.5, "pages": 0})
    return {"recency": (recency, 1), "bonus": (bonus, 1), "weighted": (weighted, 2)}


@pytest.mark.parametrize("storage", ["fp16", "fp32"])
def test_index_lists_rescore_as_the_restatement(gpu, storage):
    from ragmi.formula import compile_formula
    from ragmi.index import formula_rescore
    c = R.corpus(384)
    idx = R.view_index(gpu, 384, storage)
    enc = O.encode_rows(c["x"]) if storage == "fp16" else O.encode_rows32(c["x"])
    B, C = 4, 50
    ref_s, ref_r = O.search(enc, c["q"][:2 * B], C)
    s, r = idx.search(c["q"][:2 * B], C)
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy(), ref_r)
    assert np.array_equal(F.bits(s.cpu().numpy()), F.bits(ref_s))
    tags = idx.gather_tags(r)
    keys = [idx.gather_keys(col, r) for col in range(4)]
    torch.cuda.synchronize()
    assert np.array_equal(tags.cpu().numpy().view(np.uint32), c["tags"][ref_r])
    for col in range(4):
        assert np.array_equal(keys[col].cpu().numpy(), c["keys"][col][ref_r])
    ncand = np.array([[50, 20], [35, 50], [50, 50], [1, 0]], np.int32)
    for name, (query, L) in formulas().items():
        f = compile_formula(query, None, L, c["pt"], c["pr"])
        shape = (2 * B // L, L, C)
        for nc in (None, ncand[:, :L] if L == 2 else None):
            out = formula_rescore(
                s.reshape(shape), r.reshape(shape), f.blob(), 15, nc,
                tags.reshape(shape) if f.has_cond else None,
                {col: keys[col].reshape(shape) for col in f.columns}, with_count=True)
            torch.cuda.synchronize()
            vs, vr, st, cnt = (x.cpu().numpy() for x in out)
            want = F.rescore(ref_s.reshape(shape), ref_r.reshape(shape), f.blob(), 15, nc,
                             c["tags"][ref_r].reshape(shape) if f.has_cond else None,
                             {col: c["keys"][col][ref_r].reshape(shape) for col in f.columns})
            same((vs, vr, cnt, st.view(np.uint32)), want)
            assert (want[3] == 0).all(), name


# ------------------------------------------------------------------ 3. the client
def b32(x) -> int:
    return int(np.float32(x).view(np.uint32))


def prefetches(L, variants=(0, 1), limits=(50, 30)):
    """One or two prefetches over the corpus' queries: a ticker filter on the program route, a
    range filter."""
    from ragmi import qdrant_models as m
    c = R.corpus(384)
    flts = [m.Filter(must=[m.FieldCondition("ticker", m.MatchAny(any=["T03", "T04", "T05"]))]),
            c["flts"]["years"]]
    return [m.Prefetch(query=c["q"][variants[l]].tolist() if l else torch.as_tensor(
        c["q"][variants[l]]), filter=flts[l], limit=limits[l]) for l in range(L)]


def expected(cl, query, pres, limit, with_payload=True):
    """[(id, value bits, payload)]: the tree walker over one query_points call per prefetch
    (ids are the rows' own numbers in this collection)."""
    pay = R.corpus(384)["pay"]
    lists = [[(p.id, np.float32(p.score)) for p in cl.query_points(
        "c", pre.query, limit=pre.limit, query_filter=pre.filter).points] for pre in pres]
    hits = F.walk_request(query, lists, lambda i: pay[i], R.KINDS, limit)
    return [(i, b32(v), pay[i] if with_payload else None) for i, v in hits]


def reported(res):
    return [(p.id, b32(p.score), p.payload) for p in res.points]


def test_client_rescores_as_the_walker_over_separate_calls(gpu):
    from ragmi import qdrant_models as m
    cl = R.client(gpu)
    col = cl._col("c")
    rides = col.coalescer.requests
    for name, (query, L) in formulas().items():
        pres = prefetches(L)
        want = expected(cl, query, pres, 15)
        assert len(want) == 15, name
        rides = col.coalescer.requests
        got = cl.query_points("c", query, prefetch=pres, limit=15)
        assert col.coalescer.requests == rides               # a formula request never coalesces
        assert isinstance(got, m.QueryResponse) and isinstance(got.points[0], m.ScoredPoint)
        assert reported(got) == want, name
        # past the distinct candidates: no padding
        far = cl.query_points("c", query, prefetch=pres, limit=500)
        assert reported(far) == expected(cl, query, pres, 500) and 15 < len(far.points) <= 80
        bare = cl.query_points("c", query, prefetch=pres, limit=15, with_payload=False)
        assert reported(bare) == expected(cl, query, pres, 15, with_payload=False)
    # the recency formula moves hits: its order is not the similarity order
    query, _ = formulas()["recency"]
    one = prefetches(1)
    plain = cl.query_points("c", one[0].query, limit=50, query_filter=one[0].filter)
    boosted = cl.query_points("c", query, prefetch=one[0], limit=50)    # a bare Prefetch
    assert sorted(p.id for p in plain.points) == sorted(p.id for p in boosted.points)
    assert [p.id for p in plain.points] != [p.id for p in boosted.points]
    # nothing to re-score
    never = m.Filter(must=[m.FieldCondition("ticker", m.MatchValue("ZZZ"))])
    assert cl.query_points("c", query, prefetch=[m.Prefetch(query=R.corpus(384)["q"][0],
                                                            filter=never)]).points == []


def test_client_failures_name_their_cause(gpu):
    from ragmi import qdrant_models as m
    cl = R.client(gpu)
    pres = prefetches(2)
    with pytest.raises(ValueError, match="no entry in `defaults`"):     # some hits lack the field
        cl.query_points("c", m.FormulaQuery(formula="fiscal_year"), prefetch=pres[:1], limit=5)
    with pytest.raises(ValueError, match="no entry in `defaults`"):     # rows of one list only
        cl.query_points("c", m.FormulaQuery(formula=m.SumExpression(
            sum=["$score[0]", "$score[1]"])), prefetch=pres, limit=5)
    k8 = m.FieldCondition(key="document_type", match=m.MatchValue(value="8-K"))
    div = lambda d: m.FormulaQuery(formula=m.DivExpression(div=m.DivisionParams(
        left="$score", right=k8, by_zero_default=d)))
    with pytest.raises(ValueError, match="not finite"):
        cl.query_points("c", div(None), prefetch=pres[:1], limit=5)
    ok = cl.query_points("c", div(-1.0), prefetch=pres[:1], limit=50)
    assert reported(ok) == expected(cl, div(-1.0), pres[:1], 50)
    assert {p.score for p in ok.points} >= {-1.0}
    with pytest.raises(ValueError, match="not finite"):                  # one bad request fails
        cl.query_batch_points("c", [                                     # the call
            m.QueryRequest(query=div(-1.0), prefetch=pres[:1], limit=5),
            m.QueryRequest(query=div(None), prefetch=pres[:1], limit=5)])


def test_batch_mixes_formula_fusion_mmr_and_plain(gpu):
    from ragmi import qdrant_models as m
    cl = R.client(gpu)
    c = R.corpus(384)
    fs = formulas()
    reqs = [m.QueryRequest(query=fs["recency"][0], prefetch=prefetches(1), limit=15),
            m.QueryRequest(query=c["q"][3].tolist(), limit=7, filter=c["flts"]["since"]),
            m.QueryRequest(query=m.FusionQuery(fusion=m.Fusion.RRF), prefetch=prefetches(2),
                           limit=20),
            m.QueryRequest(query=fs["weighted"][0], prefetch=prefetches(2, (2, 3), (40, 60)),
                           limit=30, with_payload=False),
            m.QueryRequest(query=m.NearestQuery(nearest=c["q"][2].tolist(),
                                                mmr=m.Mmr(diversity=0.5, candidates_limit=40)),
                           limit=10),
            m.QueryRequest(query=fs["recency"][0], prefetch=prefetches(1, (5,), (25,)), limit=4),
            m.QueryRequest(query=fs["bonus"][0], prefetch=prefetches(1, (4,)), limit=15)]
    got = cl.query_batch_points("c", reqs)
    assert len(got) == len(reqs)
    for r, g in zip(reqs, got):
        alone = cl.query_points("c", r.query, limit=r.limit, query_filter=r.filter,
                                with_payload=r.with_payload, prefetch=r.prefetch)
        assert reported(g) == reported(alone) and len(g.points) == r.limit
    assert reported(got[0]) == expected(cl, reqs[0].query, reqs[0].prefetch, 15)
    assert reported(got[3]) == expected(cl, reqs[3].query, reqs[3].prefetch, 30,
                                        with_payload=False)
    assert reported(got[6]) == expected(cl, reqs[6].query, reqs[6].prefetch, 15)


def test_three_logical_shards_return_the_same_points(gpu):
    one, three = R.client(gpu), R.client(gpu, [gpu.index] * 3)
    for name, (query, L) in formulas().items():
        for lim in (15, 120):
            a = one.query_points("c", query, prefetch=prefetches(L), limit=lim)
            b = three.query_points("c", query, prefetch=prefetches(L), limit=lim)
            assert reported(a) == reported(b) and len(a.points) >= 15, name


def test_rag_recency(gpu, monkeypatch):
    from ragmi import qdrant_models as m
    from ragmi import rag
    cl = R.client(gpu)
    q = R.corpus(384)["q"]
    monkeypatch.setenv("TESTING", "False")
    monkeypatch.setattr(rag, "COLLECTION_NAME", "c")
    monkeypatch.setattr(rag, "get_qdrant", lambda: cl)
    now = dt.datetime(2024, 9, 1, tzinfo=UTC)
    flt = rag._filter("t03")
    query = formulas()["recency"][0]
    assert query.formula.sum[1].mult[1].exp_decay.target.datetime == "2024-09-01T00:00:00Z"
    pres = [m.Prefetch(query=q[0], filter=flt, limit=50)]
    want = cl.query_points("c", query, prefetch=pres, limit=15)
    got = rag.retrieve_from_qdrant(q[0], "t03", recency=(30, 0.25), recency_now=now)
    assert reported(got) == reported(want) == expected(cl, query, pres, 15)
    assert all(p.payload["ticker"] == "T03" for p in got.points)
    plain = cl.query_points("c", q[0], limit=15, query_filter=flt)
    assert reported(rag.retrieve_from_qdrant(q[0], "t03")) == reported(plain)
    assert reported(rag.retrieve_from_qdrant(q[0], "t03", recency=None)) == reported(plain)
    # the boost reorders: some pair of points both calls return stands the other way round
    order = {p.id: n for n, p in enumerate(plain.points)}
    shared = [order[p.id] for p in got.points if p.id in order]
    assert len(shared) >= 2 and shared != sorted(shared)
    # a chunk without a timestamp rides at the epoch's decay: its value is its score
    far = rag.retrieve_from_qdrant(q[0], "t03", limit=60, recency=(30, 0.25), recency_now=now)
    bare = [p for p in far.points if "ingested_at" not in p.payload]
    raw = {p.id: p.score for p in cl.query_points("c", q[0], limit=60, query_filter=flt).points}
    assert bare and all(b32(p.score) == b32(raw[p.id]) for p in bare)
    both = rag.retrieve_batch([q[0], q[1]], ["t03", "t04"], recency=(30, 0.25), recency_now=now)
    assert reported(both[0]) == reported(want) and len(both[1].points) == 15
    assert all(p.payload["ticker"] == "T04" for p in both[1].points)
