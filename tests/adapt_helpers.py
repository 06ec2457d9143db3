"""Shared by tests/test_adapt_host.py and tests/test_gpu_adapt.py: the input set of the online-loading-update tests, built on
online_helpers.inputs(k) with four designed series, and the yardstick the device is gated by (test infrastructure).

The yardstick.  The device differs from trmf.online.series_ridge (a direct weighted ridge) by being a recursion in the element
type with another summation order, so an fp32 session may be no farther from the fp64 series_ridge ON THE SAME W than 8x
(online_helpers.GATE, the project's allowance for another summation order) the fp32 recursive twin trmf.online.SeriesStats is
on the same input; an fp64 session no farther than that bound scaled by eps64 / eps32.  A designed series is also held on its
own scale: its row within GATE x max(the twin's error on that row, k eps32) of the row's own largest element -- the floor is the
rounding of one k-term sum, for the cases where the twin happens to round exactly as the fp64 result does."""
import functools

import numpy as np
import scipy.sparse as smat

import online_helpers as OH
from helpers import relmax
from rawsparse_helpers import RawSparse

BLOCK = OH.TN // 2                                           # two online blocks of 12 rows
MID = OH.FIRST + BLOCK
NO_ENTRY, ONE_OLD, LATE_ONLY, TWICE = 3, 8, 21, 30            # the designed series (17 is online_helpers' single-entry row's)
DESIGNED = (NO_ENTRY, ONE_OLD, LATE_ONLY, TWICE)
TWICE_ROW = OH.FIRST + 2
CASES = ((0.5, 1.0), (0.5, 0.95))                            # (lambdaI, gamma)
SMALL_RIDGE = (1e-2, 0.95)                                   # for k <= 16 only: with fewer entries than unknowns the ridge alone conditions the system
EPS32 = float(np.finfo(np.float32).eps)


@functools.lru_cache(maxsize=None)
def entries(k, density=0.3):
    """(rows, cols, vals) of online_helpers.inputs(k, density)['Y'] with the designed series: no entry at all; a single entry in
    the history and none later; entries only in the last block; one cell stored twice (two values)."""
    Y = OH.inputs(k, density)['Y'].tocoo()
    r, c, v = Y.row.astype(np.int64), Y.col.astype(np.int64), Y.data.astype(np.float32)
    keep = (c != NO_ENTRY) & (c != ONE_OLD) & ~((c == LATE_ONLY) & (r < MID))
    r, c, v = r[keep], c[keep], v[keep]
    r = np.concatenate([r, [10, TWICE_ROW, TWICE_ROW]])
    c = np.concatenate([c, [ONE_OLD, TWICE, TWICE]])
    v = np.concatenate([v, np.array([0.625, 0.25, 0.875], dtype=np.float32)])
    if not np.any((c == LATE_ONLY) & (r >= MID)):
        r, c, v = np.append(r, MID + 1), np.append(c, LATE_ONLY), np.append(v, np.float32(0.5))
    assert np.count_nonzero((r == TWICE_ROW) & (c == TWICE)) >= 2 and not np.any(c == NO_ENTRY)
    for a in (r, c, v):
        a.setflags(write=False)
    return r, c, v


def raw_rows(k, lo, hi, dtype, density=0.3, seed=None):
    """Rows lo..hi-1 of the designed matrix as the six arrays of the C ABI (row numbers from 0).  seed None: canonical order
    (ascending indices, the two copies of the doubled cell next to each other); otherwise rawsparse_helpers' random orders."""
    r, c, v = entries(k, density)
    keep = (r >= lo) & (r < hi)
    r, c, v = r[keep] - lo, c[keep], v[keep]
    shape = (hi - lo, OH.N)
    if seed is not None:
        return RawSparse(r, c, v, shape, dtype, seed=seed)
    a, b = np.lexsort((c, r)), np.lexsort((r, c))
    rp = np.zeros(shape[0] + 1, np.uint64); np.cumsum(np.bincount(r, minlength=shape[0]), out=rp[1:])
    cp = np.zeros(shape[1] + 1, np.uint64); np.cumsum(np.bincount(c, minlength=shape[1]), out=cp[1:])
    return RawSparse.from_arrays(shape, dtype, rp, c[a].astype(np.uint32), v[a].astype(dtype), cp, r[b].astype(np.uint32), v[b].astype(dtype))


def csc_of(k, lo, hi, dtype, density=0.3):
    """The same rows as a scipy CSC that keeps both copies of the doubled cell (scipy's constructors from an entry list add them)."""
    raw = raw_rows(k, lo, hi, dtype, density)
    return smat.csc_matrix((raw.val, raw.row_idx.astype(np.int32), raw.col_ptr.astype(np.int32)), shape=raw.shape)


def dense_of(k, lo, hi, dtype, density=0.3):
    """The same rows dense, the two copies of the doubled cell added (a dense matrix has one value per cell)."""
    r, c, v = entries(k, density)
    out = np.zeros((OH.T, OH.N), dtype=np.float64)
    np.add.at(out, (r, c), v.astype(np.float64))
    return np.ascontiguousarray(out[lo:hi].astype(dtype))


def training(k, lo, hi, dtype, storage, density=0.3):
    return dense_of(k, lo, hi, dtype, density) if storage == 'dense' else csc_of(k, lo, hi, dtype, density)


def recursive(W, k, dtype, gamma, missing=True, storage='sparse', density=0.3, cuts=(OH.FIRST, MID, OH.T)):
    """trmf.online.SeriesStats in `dtype` over the designed matrix: built on the rows before cuts[0], then block by block."""
    from trmf import SeriesStats
    W = np.asarray(W).astype(dtype)
    st = SeriesStats(W[:cuts[0]], training(k, 0, cuts[0], dtype, storage, density), gamma, missing)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        st.absorb(W[:hi], training(k, lo, hi, dtype, storage, density))
    return st


def direct(W, k, lamI, gamma, missing=True, storage='sparse', density=0.3, rows=OH.T):
    """trmf.online.series_ridge in fp64 over the first `rows` rows of the designed matrix."""
    from trmf import series_ridge
    return series_ridge(np.asarray(W, dtype=np.float64)[:rows], training(k, 0, rows, np.float64, storage, density), lamI, gamma, missing)


def yardstick(W, k, lamI, gamma, missing=True, storage='sparse', density=0.3):
    """(H of the fp64 direct ridge on W's fp32 values, relmax of the fp32 recursion against it, per-series own-scale errors)."""
    W32 = np.asarray(W).astype(np.float32)
    h64 = direct(W32, k, lamI, gamma, missing, storage, density)
    h32 = recursive(W32, k, np.float32, gamma, missing, storage, density).solve(lamI)
    return h64, relmax(h32, h64), own_scale(h32, h64)


def own_scale(H, ref):
    """Per series: max |H[j] - ref[j]| over max |ref[j]| (0 for a series whose reference row is zero and is met exactly)."""
    H, ref = np.asarray(H, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    num, den = np.abs(H - ref).max(axis=1), np.abs(ref).max(axis=1)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), num)


def bound(dtype, dev32):
    return OH.GATE * dev32 * (1.0 if np.dtype(dtype) == np.float32 else OH.EPS_SCALE)


def row_bound(dtype, k, twin_row):
    return bound(dtype, max(float(twin_row), k * EPS32))
