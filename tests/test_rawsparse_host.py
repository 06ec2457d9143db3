"""CPU: the oracle side of the non-canonical sparse input tests (tests/rawsparse_helpers.py, oracle_py.Mat on raw arrays).

Before the restatement may judge a kernel on input that is not a canonical CSR/CSC pair -- duplicate entries kept apart, stored
zeros, a random order inside rows and columns, the CSC not the transpose order of the CSR -- it is itself checked here: against a
per-entry fp64 NumPy model of the F-solve, against the doubled-entries identity, and against the reference's own build where
oracle/_ref exists.  `PyMatrix(coo_matrix)` is shown to hand the library exactly such input."""
import types

import numpy as np
import pytest
import scipy.sparse as smat

import oracle_py as O
from helpers import TOL, relfro, relmax
from rawsparse_helpers import RawSparse, dirty_problem, doubled, entry_fsolve, entry_objective, start_factors
from trmf.rf_util import PyMatrix

BIG = 10 ** 6
HYPER = dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5)
# One direct solve of a k x k system whose condition is at most (entries * k / 3 + lambda) / lambda ~ 3e3 here: k * cond * eps is
# 3e-12 in fp64; fp32 at the direct-solve gate the GPU tests use (tests/test_gpu_split.py)
SOLVE_GATE = {'float64': 1e-10, 'float32': 2e-4}


def _multiset(ptr, idx, val):
    major = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr.astype(np.int64)))
    order = np.lexsort((val, idx, major))
    return major[order], np.asarray(idx)[order], np.asarray(val)[order]


def test_dirty_pattern_is_what_it_says():
    raw, d = dirty_problem(120, 40, 0.25, np.float64, seed=3)
    T, n = raw.shape
    assert raw.nnz == d['rows'].size == int(raw.row_ptr[-1]) == int(raw.col_ptr[-1])
    cells = d['rows'] * n + d['cols']
    assert np.unique(cells).size < 0.9 * cells.size                     # repeated cells
    assert 0.05 < np.mean(raw.vals == 0) < 0.15                          # stored zeros
    assert np.diff(raw.col_ptr.astype(np.int64))[d['long_col']] > T and np.diff(raw.row_ptr.astype(np.int64))[d['long_row']] > n
    assert np.diff(raw.row_ptr.astype(np.int64))[d['empty_row']] == 0 and np.diff(raw.col_ptr.astype(np.int64))[d['empty_col']] == 0
    # neither orientation is sorted, and the CSC is not the transpose order of the CSR
    assert np.any(np.diff(raw.col_idx[:int(raw.row_ptr[1 + d['long_row']])].astype(np.int64)) < 0)
    lo, hi = int(raw.col_ptr[d['long_col']]), int(raw.col_ptr[d['long_col'] + 1])
    assert np.any(np.diff(raw.row_idx[lo:hi].astype(np.int64)) < 0)      # a transposed CSR would list a column's timestamps ascending
    with pytest.raises(AssertionError):
        RawSparse([0, T], [0, 0], [1.0, 1.0], (T, n), np.float64)        # an out-of-range index never leaves the helper


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_pymatrix_of_a_coo_holds_the_same_entries_as_rawsparse(dtype):
    """PyMatrix(coo_matrix) keeps duplicates apart and stored zeros (the reference's coo path): per row and per column the same
    multiset of (index, value) as RawSparse, nnz counting every copy; RawSparse.pymatrix() exposes its own arrays unchanged."""
    raw, d = dirty_problem(90, 35, 0.3, dtype, seed=5)
    py = PyMatrix(raw.coo(), dtype=dtype)
    assert py.nnz == raw.nnz == d['rows'].size and (py.rows, py.cols) == raw.shape and py.type == PyMatrix.SPARSE
    for ptr, idx, val in (('row_ptr', 'col_idx', 'val_t'), ('col_ptr', 'row_idx', 'val')):
        a = _multiset(py.py_buf[ptr], py.py_buf[idx], py.py_buf[val])
        b = _multiset(getattr(raw, ptr), getattr(raw, idx), getattr(raw, val))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert py.py_buf[val].dtype == np.dtype(dtype)
    own = raw.pymatrix()
    assert own.nnz == raw.nnz and own.type == PyMatrix.SPARSE and own.dtype == np.dtype(dtype).type
    assert np.array_equal(np.ctypeslib.as_array(own.row_ptr, (raw.shape[0] + 1,)), raw.row_ptr)
    assert np.array_equal(np.ctypeslib.as_array(own.row_idx, (raw.nnz,)), raw.row_idx)
    assert np.array_equal(np.ctypeslib.as_array(own.col_idx, (raw.nnz,)), raw.col_idx)
    assert own.val == raw.val.ctypes.data and own.val_t == raw.val_t.ctypes.data
    # and scipy's canonical conversion really is another problem (what oracle_py.Mat did to a coo before it took raw arrays)
    assert raw.canonical().nnz < raw.nnz


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_restatement_fsolve_on_raw_arrays_equals_the_per_entry_model(dtype):
    """One F-solve of each orientation, the restatement fed the raw arrays against normal equations formed entry by entry in fp64."""
    T, n, k = 120, 40, 8
    raw, _ = dirty_problem(T, n, 0.25, dtype, seed=7)
    W0, H0, Th0 = start_factors(T, n, k, 2, dtype, seed=7)
    gate = SOLVE_GATE[np.dtype(dtype).name]
    # item side through the whole train entry (CSC arrays)
    W, H, Th = W0.copy(), H0.copy(), np.asfortranarray(Th0.copy())
    O.train_port(raw, [1, 2], W, H, Th, HYPER, max_iter=1, periods=(BIG, 1, BIG), threads=2)
    want = entry_fsolve(raw.cols, raw.rows, raw.vals, W0, H0, float(dtype(HYPER['lambdaI'])))
    assert np.array_equal(W, W0) and np.array_equal(Th, Th0)
    assert relmax(H, want) < gate, relmax(H, want)
    # the canonicalised matrix is far from it: the check discriminates
    Hc = H0.copy()
    O.train_port(raw.canonical().astype(dtype), [1, 2], W0.copy(), Hc, np.asfortranarray(Th0.copy()), HYPER, max_iter=1, periods=(BIG, 1, BIG), threads=2)
    assert relmax(Hc, want) > 1e-2
    # timestamp side through the bare F-solve (CSR arrays)
    csr = types.SimpleNamespace(indptr=raw.row_ptr, indices=raw.col_idx, data=raw.val_t, shape=raw.shape)
    X = O.fsolve_port(csr, H0, W0.copy(), 0.25, threads=2)
    want = entry_fsolve(raw.rows, raw.cols, raw.vals, H0, W0, 0.25)
    assert relmax(X, want) < gate, relmax(X, want)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_objective_on_raw_arrays_is_the_sum_over_entries(dtype):
    T, n, k = 100, 30, 6
    raw, _ = dirty_problem(T, n, 0.3, dtype, seed=11)
    W, H, Th = start_factors(T, n, k, 3, dtype, seed=2)
    lags = np.array([1, 2, 5], dtype=np.uint32)
    J = O.objective(raw, lags, W, H, Th, HYPER)
    assert abs(J - entry_objective(raw, lags, W, H, Th, HYPER)) <= 1e-12 * J
    Jc = O.objective(raw.canonical(), lags, W, H, Th, HYPER)            # existing callers: scipy input as before
    assert abs(Jc - J) > 1e-3 * J


def _train(Y, lags, W0, H0, Th0, hyper, iters, fn=O.train_port, **kw):
    W, H, Th = W0.copy(), H0.copy(), np.asfortranarray(Th0.copy())
    log = fn(Y, np.asarray(lags, dtype=np.uint32), W, H, Th, hyper, max_iter=iters, threads=2, **kw)
    return W, H, Th, log


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_entry_order_does_not_matter_beyond_rounding(dtype):
    T, n, k = 120, 40, 8
    raw, _ = dirty_problem(T, n, 0.25, dtype, seed=13)
    f0 = start_factors(T, n, k, 3, dtype, seed=13)
    a = _train(raw, [1, 2, 4], *f0, HYPER, 3)
    b = _train(raw.reordered(99), [1, 2, 4], *f0, HYPER, 3)
    tol = TOL[np.dtype(dtype).name]['factor']
    assert relfro(b[0], a[0]) < tol and relfro(b[1], a[1]) < tol and relfro(b[2], a[2]) < 10 * tol


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_doubled_entries_equal_halved_weights_on_the_restatement(dtype):
    """Every entry stored twice under (lambdaI, lambdaAR, lambdaLag) is the canonical problem under (lambdaI/2, lambdaAR/2, lambdaLag):
    the loss doubles, so both ridge weights halve relative to it; the lag-weight solve sees W only."""
    T, n, k = 120, 40, 8
    rng = np.random.RandomState(17)
    Y = smat.random(T, n, density=0.25, random_state=rng, format='csr', dtype=np.float64).astype(dtype)
    Y.sort_indices()
    coo = Y.tocoo()
    twice = doubled(RawSparse(coo.row, coo.col, coo.data, (T, n), dtype, seed=1), seed=2)
    assert twice.nnz == 2 * Y.nnz
    f0 = start_factors(T, n, k, 3, dtype, seed=17)
    half = dict(lambdaI=HYPER['lambdaI'] / 2, lambdaAR=HYPER['lambdaAR'] / 2, lambdaLag=HYPER['lambdaLag'])
    a = _train(twice, [1, 2, 4], *f0, HYPER, 3)
    b = _train(Y, [1, 2, 4], *f0, half, 3)
    tol = TOL[np.dtype(dtype).name]['factor']
    assert relfro(a[0], b[0]) < tol and relfro(a[1], b[1]) < tol and relfro(a[2], b[2]) < 10 * tol
    assert all(abs(x['cg_iter'] - y['cg_iter']) <= 1 for x, y in zip(a[3], b[3]))
    c = _train(Y, [1, 2, 4], *f0, HYPER, 3)                              # and it is not the canonical problem at the full weights
    assert relfro(a[1], c[1]) > 1e-2


@pytest.mark.parametrize('lags', [[1, 2, 4], [1, 1, 2]], ids=['lags124', 'lags112'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_reference_build_agrees_with_the_restatement_on_the_dirty_pattern(dtype, lags):
    """Where oracle/_ref exists: the reference's own build takes the raw arrays as they are, like the restatement (also with a
    repeated lag); after 3 iterations the two agree far inside the parity gates."""
    if O.ref(dtype) is None:
        pytest.skip('oracle/_ref has not been built')
    T, n, k = 120, 40, 8
    raw, _ = dirty_problem(T, n, 0.25, dtype, seed=19)
    f0 = start_factors(T, n, k, len(lags), dtype, seed=19)
    a = _train(raw, lags, *f0, HYPER, 3)
    b = _train(raw, lags, *f0, HYPER, 3, fn=O.train_ref)
    tol = TOL[np.dtype(dtype).name]['factor'] / 10
    assert all(np.all(np.isfinite(x)) for x in a[:3] + b[:3])
    assert relfro(a[0], b[0]) < tol and relfro(a[1], b[1]) < tol and relfro(a[2], b[2]) < 10 * tol, [relfro(x, y) for x, y in zip(a[:3], b[:3])]
