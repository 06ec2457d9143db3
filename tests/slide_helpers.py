"""Shared by tests/test_slide_host.py and tests/test_gpu_slide.py: the input sets of the sliding-window tests (test infrastructure).

Built on the small designs of online_helpers / adapt_helpers / rawsparse_helpers: T = 96 rows of 50 series, ranks from
online_helpers.RANKS.  `slid` is the statement of the storage contract of trmf_session_slide: both orientations of a session's Y
pass through trmf.online.slide_entries (a stable filter, row numbers reduced), the block's entries follow per row / per column."""
import functools

import numpy as np

import adapt_helpers as AH
import online_helpers as OH
from rawsparse_helpers import RawSparse, stacked

T0 = AH.MID                     # 84 rows resident, then the block of rows 84..95
RETIRE = 20
DOUBLE_GONE = (5, 12)           # a cell stored twice in a row that is retired (adapt_helpers stores (74, 30) twice: that one stays)
STATS_RETIRE = 30               # of 84 absorbed rows: fewer than half (a downdate that removes most of S_j cancels by construction)
EPS32 = AH.EPS32


@functools.lru_cache(maxsize=None)
def entries(k, density=0.3):
    """adapt_helpers.entries(k) plus one cell stored twice in a row that is retired."""
    r, c, v = AH.entries(k, density)
    r = np.concatenate([r, [DOUBLE_GONE[0]] * 2]); c = np.concatenate([c, [DOUBLE_GONE[1]] * 2])
    v = np.concatenate([v, np.array([0.375, 0.8125], dtype=np.float32)])
    for a in (r, c, v):
        a.setflags(write=False)
    return r, c, v


def raw_rows(k, lo, hi, dtype, seed, density=0.3):
    """Rows lo..hi-1 as the six arrays of the C ABI in rawsparse_helpers' random orders (neither orientation sorted)."""
    r, c, v = entries(k, density)
    keep = (r >= lo) & (r < hi)
    return RawSparse(r[keep] - lo, c[keep], v[keep], (hi - lo, OH.N), dtype, seed=seed + lo)


def dense_rows(k, lo, hi, dtype, density=0.3):
    r, c, v = entries(k, density)
    out = np.zeros((OH.T, OH.N), dtype=np.float64)
    np.add.at(out, (r, c), v.astype(np.float64))
    return np.ascontiguousarray(out[lo:hi].astype(dtype))


def slid(raw, retire, tail=None):
    """The arrays a session holds after slide(tail, retire) on a session created over `raw`: each orientation filtered in its
    stored order by trmf.online.slide_entries, then the block appended as append_rows appends it (rawsparse_helpers.stacked)."""
    from trmf.online import slide_entries
    T, n = raw.shape
    rows_csr = np.repeat(np.arange(T, dtype=np.int64), np.diff(raw.row_ptr.astype(np.int64)))
    r, c, v = slide_entries(rows_csr, raw.col_idx, raw.val_t, retire)
    cols_csc = np.repeat(np.arange(n, dtype=np.int64), np.diff(raw.col_ptr.astype(np.int64)))
    r2, c2, v2 = slide_entries(raw.row_idx.astype(np.int64), cols_csc, raw.val, retire)
    rp = np.zeros(T - retire + 1, np.uint64); np.cumsum(np.bincount(r, minlength=T - retire), out=rp[1:])
    cp = np.zeros(n + 1, np.uint64); np.cumsum(np.bincount(c2, minlength=n), out=cp[1:])
    out = RawSparse.from_arrays((T - retire, n), raw.dtype, rp, c.astype(np.uint32), v, cp, r2.astype(np.uint32), v2)
    return out if tail is None else stacked(out, tail)


# ---- the column shapes of the compaction ---------------------------------------------------------------------------------------
SHAPE_T, SHAPE_RETIRE = 300, 150
SHAPE_LENGTHS = (0, 1, 63, 64, 65, 130)
SHAPE_PLACES = ('late', 'early', 'mixed')       # the retirement takes none / all / an interleaved part of the column


@functools.lru_cache(maxsize=None)
def shape_problem(dtype, seed=5):
    """One column per (length, placement): `late` columns hold timestamps >= SHAPE_RETIRE only, `early` ones < SHAPE_RETIRE only,
    `mixed` ones both (in a random stored order, so the survivors are interleaved with the retired), plus one column of 140 entries
    with repeated cells.  Every retained row keeps at least one entry through the last column."""
    rng = np.random.RandomState(seed)
    rows, cols = [], []
    j = 0
    for L in SHAPE_LENGTHS:
        for place in SHAPE_PLACES:
            lo, hi = {'late': (SHAPE_RETIRE, SHAPE_T), 'early': (0, SHAPE_RETIRE), 'mixed': (0, SHAPE_T)}[place]
            rr = rng.permutation(np.arange(lo, hi))[:L]
            if place == 'mixed' and L > 1:
                assert np.any(rr < SHAPE_RETIRE) and np.any(rr >= SHAPE_RETIRE)
            rows.append(rr); cols.append(np.full(L, j)); j += 1
    rr = rng.randint(0, SHAPE_T, size=140)                  # repeated cells, more than two chunks of 64
    rows.append(rr); cols.append(np.full(rr.size, j)); j += 1
    rows.append(np.arange(SHAPE_T)); cols.append(np.full(SHAPE_T, j)); j += 1
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.rand(rows.size).astype(np.float32) + np.float32(0.25)
    return RawSparse(rows, cols, vals, (SHAPE_T, j), dtype, seed=seed + 1)


# ---- the statistics: the downdate recursion as a NumPy twin ----------------------------------------------------------------------
def stats_training(k, lo, hi, dtype):
    """Rows lo..hi-1 as a scipy CSC that keeps both copies of a doubled cell, canonical order (adapt_helpers.csc_of's form)."""
    import scipy.sparse as smat
    r, c, v = entries(k)
    keep = (r >= lo) & (r < hi)
    r, c, v = r[keep] - lo, c[keep], v[keep].astype(dtype)
    b = np.lexsort((r, c))
    cp = np.zeros(OH.N + 1, np.int64); np.cumsum(np.bincount(c, minlength=OH.N), out=cp[1:])
    return smat.csc_matrix((v[b], r[b].astype(np.int32), cp.astype(np.int32)), shape=(hi - lo, OH.N))


def downdate_twin(W, k, dtype, gamma, retire=STATS_RETIRE):
    """trmf.SeriesStats in `dtype` through the sequence of the device test: built on rows 0..71, rows 72..83 absorbed, the `retire`
    oldest rows retired with a downdate, rows 84..95 absorbed.  W: the 96 rows as they were BEFORE the retirement."""
    from trmf import SeriesStats
    W = np.asarray(W).astype(dtype)
    st = SeriesStats(W[:OH.FIRST], stats_training(k, 0, OH.FIRST, dtype), gamma, True)
    st.absorb(W[:T0], stats_training(k, OH.FIRST, T0, dtype))
    st.retire(W, stats_training(k, 0, T0, dtype), retire)
    st.absorb(W[retire:], stats_training(k, T0, OH.T, dtype))
    return st


def downdate_direct(W, k, lamI, gamma, retire=STATS_RETIRE):
    """trmf.online.series_ridge in fp64 on the retained rows alone."""
    from trmf import series_ridge
    return series_ridge(np.asarray(W, dtype=np.float64)[retire:], stats_training(k, retire, OH.T, np.float64), lamI, gamma, True)
