"""Shared by tests/test_churn_host.py and tests/test_gpu_churn.py: the input sets of the series-churn tests (test infrastructure).

Built on the designs of online_helpers / adapt_helpers / slide_helpers: T = 96 rows of 50 series, lags (1, 2, 5).  A session holds
series 0..37 and churns: a designed set is retired and / or series 38..49 join.  `churned` is the statement of the storage contract
of trmf_session_change_series: both orientations of a session's Y pass through trmf.churn_entries (a stable filter with the kept
series renumbered; the block's entries merged stably behind the survivors of the same row / as whole columns behind the kept ones)."""
import functools

import numpy as np

import adapt_helpers as AH
import online_helpers as OH
import slide_helpers as SH
from rawsparse_helpers import RawSparse

N0 = 38                                              # series resident before the churn; 38..49 are the block
M = OH.N - N0
# the first series, the last one, two neighbours, the series with the cell stored twice (adapt_helpers.TWICE) -- and, with it in,
# slide_helpers' doubled cell (5, 12) stays
RETIRED = (0, 14, 15, AH.TWICE, N0 - 1)
EPS32 = AH.EPS32
SUM_TOL = 1e-12                                      # fp64 sums of the same terms in another order (the adapt tests' tolerance)


def keep_mask(n=N0, retired=RETIRED):
    keep = np.ones(n, dtype=bool)
    keep[list(retired)] = False
    return keep


def raw_cols(k, lo, hi, dtype, seed, density=0.3):
    """Series lo..hi-1 over all 96 rows as the six arrays of the C ABI in rawsparse_helpers' random orders, numbered from 0."""
    r, c, v = SH.entries(k, density)
    keep = (c >= lo) & (c < hi)
    return RawSparse(r[keep], c[keep] - lo, v[keep], (OH.T, hi - lo), dtype, seed=seed + 7 * lo)


def raw_part(k, rlo, rhi, series, dtype, seed, density=0.3):
    """Rows rlo..rhi-1 of the listed series (old numbers, in their new order) as the six arrays of the C ABI, random orders."""
    r, c, v = SH.entries(k, density)
    new = np.full(OH.N, -1, dtype=np.int64)
    new[np.asarray(series, dtype=np.int64)] = np.arange(len(series))
    keep = (r >= rlo) & (r < rhi) & (new[c] >= 0)
    return RawSparse(r[keep] - rlo, new[c[keep]], v[keep], (rhi - rlo, len(series)), dtype, seed=seed + 13 * rlo + len(series))


def dense_cols(k, lo, hi, dtype, density=0.3):
    return np.ascontiguousarray(SH.dense_rows(k, 0, OH.T, dtype, density)[:, lo:hi])


def entry_lists(raw):
    """(rows, cols, vals) of the CSR arrays in stored order, and of the CSC arrays in stored order."""
    T, n = raw.shape
    rows_csr = np.repeat(np.arange(T, dtype=np.int64), np.diff(raw.row_ptr.astype(np.int64)))
    cols_csc = np.repeat(np.arange(n, dtype=np.int64), np.diff(raw.col_ptr.astype(np.int64)))
    return (rows_csr, raw.col_idx.astype(np.int64), raw.val_t), (raw.row_idx.astype(np.int64), cols_csc, raw.val)


def churned(raw, keep=None, block=None):
    """The arrays a session holds after change_series(keep, block) on a session created over `raw`: each orientation through
    trmf.churn_entries."""
    from trmf import churn_entries
    T, n = raw.shape
    csr, csc = entry_lists(raw)
    bcsr, bcsc = entry_lists(block) if block is not None else (None, None)
    r, c, v = churn_entries(*csr, keep, n, bcsr, major='row')
    r2, c2, v2 = churn_entries(*csc, keep, n, bcsc, major='col')
    n1 = (n if keep is None else int(np.count_nonzero(keep))) + (block.shape[1] if block is not None else 0)
    rp = np.zeros(T + 1, np.uint64); np.cumsum(np.bincount(r, minlength=T), out=rp[1:])
    cp = np.zeros(n1 + 1, np.uint64); np.cumsum(np.bincount(c2, minlength=n1), out=cp[1:])
    return RawSparse.from_arrays((T, n1), raw.dtype, rp, c.astype(np.uint32), v, cp, r2.astype(np.uint32), v2)


def brute_churn(rows, cols, vals, keep, n, block, major):
    """churn_entries as a loop over the entries: per major index (row, or NEW column) the survivors in stored order, then the
    block's entries of that index in stored order."""
    keep = np.ones(n, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    new = {}
    for j in range(n):
        if keep[j]:
            new[j] = len(new)
    nk = len(new)
    items = [(int(r), new[int(c)], v) for r, c, v in zip(rows, cols, vals) if keep[int(c)]]
    if block is None:
        return items
    items += [(int(r), int(c) + nk, v) for r, c, v in zip(*block)]
    key = (lambda e: e[0]) if major == 'row' else (lambda e: e[1])
    out = []
    for m in sorted(set(key(e) for e in items)):
        out += [e for e in items if key(e) == m]
    return out


# ---- what the contract promises equal on both sessions (test_gpu_slide._after's list) ------------------------------------------
def after(s, T1):
    """Three iterations (with the CG's step counts), the objective, the filter, the smoother and a forecast."""
    out = {}
    s.run(3)
    out['cg'] = [x['cg_iter'] for x in s.stats(3)]
    m = s.download()
    out['W'], out['H'], out['theta'] = m.W.copy(), m.H.copy(), m.lag_val.copy()
    out['J'] = np.float64(s.objective())
    out['assim'], out['Wa'] = s.assimilate(T1 - 6, return_latent=True)
    out['smooth'], out['Ws'] = s.smooth(T1 - 10, return_latent=True)
    out['Y5'], out['W5'] = s.forecast(5, return_latent=True)
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], np.ndarray) or isinstance(a[key], np.floating):
            assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


# ---- the row shapes of the compaction ------------------------------------------------------------------------------------------
SHAPE_T, SHAPE_N, SHAPE_M = 12, 140, 70
SHAPE_LENGTHS = (0, 1, 63, 64, 65, 130)
SHAPE_BLOCK_LENGTHS = (0, 1, 65)


@functools.lru_cache(maxsize=None)
def shape_problem(dtype, seed=5):
    """T = 12 rows of n = 140 series: rows of 0, 1, 63, 64, 65 and 130 entries (twice each, so that the lag set fits), and one of
    140 entries with repeated cells; plus a block of 70 new series whose rows hold 0, 1 and 65 entries in turn."""
    rng = np.random.RandomState(seed)
    rows, cols = [], []
    for i, L in enumerate(SHAPE_LENGTHS + SHAPE_LENGTHS[1:]):
        cc = rng.permutation(SHAPE_N)[:L]
        rows.append(np.full(L, i)); cols.append(cc)
    cc = rng.randint(0, SHAPE_N, size=140)                  # repeated cells, more than two steps of 64
    rows.append(np.full(cc.size, SHAPE_T - 1)); cols.append(cc)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.rand(rows.size).astype(np.float32) + np.float32(0.25)
    raw = RawSparse(rows, cols, vals, (SHAPE_T, SHAPE_N), dtype, seed=seed + 1)
    brows, bcols = [], []
    for i in range(SHAPE_T):
        L = SHAPE_BLOCK_LENGTHS[i % 3]
        cc = rng.randint(0, SHAPE_M, size=L) if L > 1 else rng.permutation(SHAPE_M)[:L]
        brows.append(np.full(L, i)); bcols.append(cc)
    brows, bcols = np.concatenate(brows), np.concatenate(bcols)
    bvals = rng.rand(brows.size).astype(np.float32) + np.float32(0.25)
    return raw, RawSparse(brows, bcols, bvals, (SHAPE_T, SHAPE_M), dtype, seed=seed + 2)


def shape_keeps():
    """Every row loses none, all and an interleaved part of its series."""
    rng = np.random.RandomState(9)
    return {'none': None, 'all': np.zeros(SHAPE_N, dtype=bool), 'mixed': rng.rand(SHAPE_N) < 0.5}


# ---- the cold-start fit ------------------------------------------------------------------------------------------------------
FIT_LENGTHS = (0, 1, 64, 65, OH.T)                   # entries of the designed new series; one more holds a cell stored twice
FIT_M = len(FIT_LENGTHS) + 1 + 6                      # ... and six ordinary ones at density 0.3


@functools.lru_cache(maxsize=None)
def fit_entries(k):
    """(rows, cols, vals) of 12 new series over the 96 rows: no entry, one, exactly 64, 65, all 96, one with a cell stored twice
    (and 30 % of the others), six at 30 %."""
    rng = np.random.RandomState(300 + k)
    rows, cols = [], []
    for j, L in enumerate(FIT_LENGTHS):
        rows.append(np.sort(rng.permutation(OH.T)[:L])); cols.append(np.full(L, j))
    for j in range(len(FIT_LENGTHS), FIT_M):
        rr = np.flatnonzero(rng.rand(OH.T) < 0.3)
        if j == len(FIT_LENGTHS):
            rr = np.sort(np.concatenate([rr, rr[:1]]))     # the first of its cells a second time
        rows.append(rr); cols.append(np.full(rr.size, j))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = (rng.rand(rows.size).astype(np.float32) + np.float32(0.25))
    for a in (rows, cols, vals):
        a.setflags(write=False)
    return rows, cols, vals


def fit_raw(k, dtype, seed=None):
    """The new series as the six arrays of the C ABI: canonical order (seed None) or random stored orders."""
    r, c, v = fit_entries(k)
    shape = (OH.T, FIT_M)
    if seed is not None:
        return RawSparse(r, c, v, shape, dtype, seed=seed)
    a, b = np.lexsort((c, r)), np.lexsort((r, c))
    rp = np.zeros(shape[0] + 1, np.uint64); np.cumsum(np.bincount(r, minlength=shape[0]), out=rp[1:])
    cp = np.zeros(shape[1] + 1, np.uint64); np.cumsum(np.bincount(c, minlength=shape[1]), out=cp[1:])
    return RawSparse.from_arrays(shape, dtype, rp, c[a].astype(np.uint32), v[a].astype(dtype), cp, r[b].astype(np.uint32), v[b].astype(dtype))


def fit_csc(raw):
    """scipy CSC over the raw CSC arrays, both copies of the doubled cell kept, in the stored order."""
    import scipy.sparse as smat
    return smat.csc_matrix((raw.val, raw.row_idx.astype(np.int32), raw.col_ptr.astype(np.int32)), shape=raw.shape)


def fit_dense(k, dtype):
    r, c, v = fit_entries(k)
    out = np.zeros((OH.T, FIT_M), dtype=np.float64)
    np.add.at(out, (r, c), v.astype(np.float64))
    return np.ascontiguousarray(out.astype(dtype))


def fit_yardstick(W, Ynew, lamI, gamma, missing):
    """(H of the fp64 series_ridge on W's fp32 values, relmax of the fp32 twin SeriesStats(W, Ynew, gamma, missing).solve(lamI)
    against it, the twin's per-series own-scale errors).  Ynew: a RawSparse (its CSC arrays as stored, duplicates kept) or a dense
    array."""
    from trmf import SeriesStats, series_ridge
    from helpers import relmax
    W32 = np.asarray(W).astype(np.float32)
    as_dt = (lambda dt: fit_csc(Ynew.astype(dt))) if isinstance(Ynew, RawSparse) else (lambda dt: np.asarray(Ynew).astype(dt))
    h64 = series_ridge(W32.astype(np.float64), as_dt(np.float64), lamI, gamma, missing)
    h32 = SeriesStats(W32, as_dt(np.float32), gamma, missing).solve(lamI)
    return h64, relmax(h32, h64), AH.own_scale(h32, h64)


def fit_sq_err(Ynew, W, Hnew):
    """fp64: sum over the new series' stored entries (dense: every cell) of (y - w_t . h_j)^2."""
    W64, H64 = np.asarray(W, dtype=np.float64), np.asarray(Hnew, dtype=np.float64)
    if isinstance(Ynew, RawSparse):
        p = np.einsum('ed,ed->e', W64[Ynew.rows], H64[Ynew.cols])
        return float(((Ynew.vals.astype(np.float64) - p) ** 2).sum())
    return float(((np.asarray(Ynew, dtype=np.float64) - W64.dot(H64.T)) ** 2).sum())
