"""Vectors at the edges of the value space and a plain statement of what the index does with
them (DESIGN.md "Values at the edges"): a vector whose canonical sumsq is not finite (some
component is inf or NaN), or is zero, normalises to the zero vector: fp32 +0.0 in every element,
so fp16 0x0000; finite inputs keep every bit. TEST HELPER ONLY, shared by test_oracle_scan.py
(CPU) and test_values_gpu.py.

`plain_*` below share nothing with oracle/scan_ref.c: numpy float64 throughout, numpy's own
roundings to fp32 and fp16.
"""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
NONFINITE = ("pinf", "ninf", "nan", "allnan", "inf_nan")
FINITE = ("sub", "tiny", "huge", "fltmax", "fltmax_one", "negzero", "onehot_p", "onehot_m",
          "straddle")


def special(name: str, D: int, rng) -> np.ndarray:
    """One fp32 vector [D] of the named kind."""
    g = rng.standard_normal(D)
    j = int(rng.integers(D))
    if name == "pinf":                       # one +inf among Gaussian components
        g[j] = np.inf
    elif name == "ninf":
        g[j] = -np.inf
    elif name == "nan":
        g[j] = np.nan
    elif name == "allnan":
        g[:] = np.nan
    elif name == "inf_nan":                  # inf beside NaN (and a -inf)
        g[j], g[(j + 1) % D], g[(j + 7) % D] = np.inf, np.nan, -np.inf
    elif name == "sub":                      # every component an fp32 subnormal
        g *= 1e-42
    elif name == "tiny":
        g *= 1e-30
    elif name == "huge":                     # squares far beyond fp32's range
        g *= 3e36
    elif name == "fltmax":                   # every component +-FLT_MAX
        g = np.where(g < 0, -1.0, 1.0) * float(FLT_MAX)
    elif name == "fltmax_one":
        # one FLT_MAX beside O(1) components and bands of larger ones: the rest normalise to fp32
        # subnormals (g / 3.4e38), to zero (1e-7 g / 3.4e38), and around fp16's smallest subnormal
        # 6e-8 (1e31 g / 3.4e38) and inside fp16's subnormals (1e33 g / 3.4e38)
        q = D // 4
        g[q:2 * q] *= 1e31
        g[2 * q:3 * q] *= 1e33
        g[3 * q:] *= 1e-7
        g[j % q] = float(FLT_MAX)
    elif name == "negzero":
        g[::3] = -0.0
    elif name in ("onehot_p", "onehot_m"):
        g[:] = 0.0
        g[j] = 1.0 if name == "onehot_p" else -1.0
    elif name == "straddle":                 # normalised elements on both sides of 2^-14
        g = 2.0 ** -14 * np.where(g < 0, -1.0, 1.0) * rng.uniform(0.5, 2.0, D)
        g[j] = 1.0
    else:
        raise KeyError(name)
    with np.errstate(over="ignore"):
        return g.astype(np.float32)


def specials(names, D: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.stack([special(n, D, rng) for n in names])


def plain_normalize(x) -> np.ndarray:
    """fp32 [n, D]: x / ||x|| in numpy float64, rounded to fp32; the zero vector for a row with a
    non-finite component or of norm 0."""
    x = np.asarray(x, np.float32)
    x64 = x.astype(np.float64)
    drop = ~np.isfinite(x).all(axis=1)
    x64[drop] = 0.0
    nrm = np.sqrt((x64 * x64).sum(axis=1))
    drop |= nrm == 0.0
    nrm[drop] = 1.0
    y = (x64 / nrm[:, None]).astype(np.float32)
    y[drop] = 0.0
    return y


def plain_store(x, storage: str = "fp16") -> np.ndarray:
    """The stored rows of input vectors x: fp16 bits (uint16) or the fp32 rows."""
    y = plain_normalize(x)
    return y if storage == "fp32" else y.astype(np.float16).view(np.uint16)


def plain_search(x, q, k: int, storage: str = "fp16"):
    """(scores fp32 [B, k], rows int64 [B, k]) by (score desc, row asc) over the stored rows of x
    against queries q: float64 matmul rounded to fp32, full lexsort."""
    c = plain_store(x, storage)
    c = (c.view(np.float16) if c.dtype == np.uint16 else c).astype(np.float64)
    s = (plain_normalize(q).astype(np.float64) @ c.T).astype(np.float32) + np.float32(0.0)
    rows = np.arange(c.shape[0])
    out_s = np.empty((len(s), k), np.float32)
    out_i = np.empty((len(s), k), np.int64)
    for b in range(len(s)):
        order = np.lexsort((rows, -s[b].astype(np.float64)))[:k]
        out_s[b], out_i[b] = s[b][order], order
    return out_s, out_i


def ulps(y, ref64) -> np.ndarray:
    """|y - fp32(ref64)| in units of fp32's spacing at fp32(ref64), subnormals included."""
    r = np.asarray(ref64, np.float64).astype(np.float32)
    return np.abs(np.asarray(y, np.float32).astype(np.float64) - r.astype(np.float64)) / \
        np.spacing(np.abs(r)).astype(np.float64)
