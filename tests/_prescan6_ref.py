"""Numpy restatement of the 6-bit prescan's arithmetic (prep_kernels.hip "6-bit scan copy",
qprep8_slot, u_bound6): the row quantiser, the two int8 query planes with their F / A / C, and
the upper bound u, each step rounded to fp32 where the device rounds. test_prescan6_cpu.py
checks the inequality u >= e on it; test_prescan6_gpu.py compares the device's u with it bit
for bit."""
import numpy as np

K_ROW_NORM = 1.001          # kRowNorm
SLACK = np.float32(2.0 ** -20)   # kU8Slack
QMAX = 31                   # Copy6::kQMax
UP = 1.0 + 2.0 ** -20

f32 = np.float32


def quantise_rows6(c):
    """c: stored rows as fp32 values of their fp16 bits [n, D] -> (v int [n, D] in [-31, 31],
    s fp32 [n] = max|c| / 31, E fp32 [n] = ||c - s v||_2 rounded up)."""
    c = np.asarray(c, f32)
    m = np.abs(c).max(axis=1)
    s = (m / f32(QMAX)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(s[:, None] > 0, np.rint((c / s[:, None]).astype(f32)), f32(0))
    v = np.clip(v, -QMAX, QMAX)
    d = c.astype(np.float64) - s.astype(np.float64)[:, None] * v.astype(np.float64)
    e2 = (d * d).sum(axis=1)
    E = np.where(e2 > 0, (np.sqrt(e2) * UP), 0.0).astype(f32)
    return v.astype(np.int64), s, E


def query_planes(y):
    """y: canonically normalised queries fp32 [b, D] -> (hi, lo int [b, D], sq, A, C fp32 [b])."""
    y = np.asarray(y, f32)
    m = np.abs(y).max(axis=1)
    s1 = (m / f32(127)).astype(f32)
    sq = (s1 / f32(254)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = np.where(s1[:, None] > 0, np.rint((y / s1[:, None]).astype(f32)), f32(0))
        hi = np.clip(hi, -127, 127)
        rho = y.astype(np.float64) - s1.astype(np.float64)[:, None] * hi.astype(np.float64)
        lo = np.where(sq[:, None] > 0,
                      np.rint((rho / sq.astype(np.float64)[:, None]).astype(f32)), f32(0))
    lo = np.clip(lo, -127, 127)
    dd = y.astype(np.float64) - sq.astype(np.float64)[:, None] * (254.0 * hi + lo)
    F = np.sqrt((dd * dd).sum(axis=1)) * UP
    Y = np.sqrt((y.astype(np.float64) ** 2).sum(axis=1)) * UP
    A = ((Y + F) * UP).astype(f32)
    C = ((K_ROW_NORM * F + float(SLACK)) * UP).astype(f32)
    return hi.astype(np.int64), lo.astype(np.int64), sq, A, C


def _fma32(a, b, c):
    """fl32(a * b + c) for fp32 arrays: the product of two fp32 is exact in fp64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def upper_bounds(v, s, E, hi, lo, sq, A, C):
    """u [b, n] as the scan evaluates it: bytes 4 v, stored scale s / 4, one int32 -> fp32
    conversion of I6 = 254 (4 v . hi) + 4 v . lo, then two fp32 fmas."""
    v4 = 4 * v
    I6 = 254 * (hi @ v4.T) + lo @ v4.T                       # exact integers [b, n]
    assert np.abs(I6).max(initial=0) < 2 ** 31
    If = I6.astype(f32)                                      # RNE, as v_cvt_f32_i32
    s4 = (f32(0.25) * s).astype(f32)
    scale = (s4[None, :] * sq[:, None]).astype(f32)
    tail = _fma32(np.broadcast_to(E[None, :], If.shape), np.broadcast_to(A[:, None], If.shape),
                  np.broadcast_to(C[:, None], If.shape))
    return _fma32(If, scale, tail)
