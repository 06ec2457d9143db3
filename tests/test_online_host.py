"""CPU: the host side of the online updates -- trmf.online.filter_rows (the NumPy statement of trmf_session_assimilate) against an
independent check, its guards, Model.assimilate, the refusals of rolling_validate(update='assimilate'), the new C entry point and
the yardstick the device tests are gated by.  No compute is launched here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as smat

import online_helpers as OH
from helpers import make_model, relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, 'include')


def _systems(d, W, lamI, lamAR, missing, first):
    """(A_i, b_i) of every row first.. in fp64, formed entry by entry from the definition, with the prior from W's own rows."""
    H, theta, back = d['H'].astype(np.float64), d['theta'].astype(np.float64), d['lag_set'].astype(int)
    Yd = np.asarray(d['Y'].todense(), dtype=np.float64)
    stored = np.zeros(Yd.shape, dtype=bool)
    c = d['Y'].tocoo()
    stored[c.row, c.col] = True
    for i in range(first, W.shape[0]):
        A = (lamI + lamAR) * np.eye(d['k'])
        b = np.zeros(d['k'])
        for j in range(H.shape[0]):
            if stored[i, j] or not missing:
                A += np.outer(H[j], H[j])
                b += Yd[i, j] * H[j]
        p = sum(theta[l] * W[i - back[l]] for l in range(len(back)))
        yield i, A, b + lamAR * p


@pytest.mark.parametrize('missing', [True, False])
@pytest.mark.parametrize('lamI,lamAR', OH.LAMBDAS)
@pytest.mark.parametrize('k', [1, 7, 40])
def test_filter_rows_zeroes_the_gradient_of_every_row(k, lamI, lamAR, missing):
    d = OH.inputs(k)
    W = OH.twin(d, np.float64, lamI, lamAR, missing)
    assert np.array_equal(W[:OH.FIRST], d['W'][:OH.FIRST].astype(np.float64))        # earlier rows are not touched
    for i, A, b in _systems(d, W, lamI, lamAR, missing, OH.FIRST):
        assert np.abs(A.dot(W[i]) - b).max() <= 1e-10 * max(np.abs(b).max(), np.abs(A).max() * np.abs(W[i]).max()), i


def test_noise_free_ar_data_is_a_fixed_point():
    """Y = W* H^T with W* following the AR model exactly and lambdaI = 0: every new row's minimiser is the AR roll-out itself."""
    from trmf import Model, filter_rows
    rng = np.random.RandomState(3)
    k, n, T0, Tn = 5, 30, 40, 12
    lags = np.array([1, 2, 5], dtype=np.uint32)
    theta = rng.randn(3, k)
    theta = theta / (np.abs(theta).sum(axis=0) + 0.1)
    model = make_model(rng.rand(T0, k), rng.rand(n, k), theta, lags)
    Wstar = model.latent_forecast(Tn)
    Ynew = Wstar[T0:].dot(model.H.T)
    for missing, Yrows in ((False, Ynew), (True, smat.csr_matrix(Ynew * (rng.rand(Tn, n) < 0.5)))):
        grown = np.vstack([model.W, np.zeros((Tn, k))])
        got = filter_rows(grown, model.H, lags, model.lag_val, Yrows, T0, 0.0, 2.0, missing)
        assert relmax(got[T0:], Wstar[T0:]) <= 1e-12, missing


def test_guards_and_the_empty_row():
    from trmf import filter_rows
    d = OH.inputs(7)
    W64 = d['W'].astype(np.float64)
    for lamI, lamAR in ((0.5, 50.0), (0.0, 1.0)):
        got = OH.twin(d, np.float64, lamI, lamAR)
        i = OH.EMPTY_ROW
        p = np.sum(got[i - d['lag_set'].astype(int)] * d['theta'].astype(np.float64), axis=0)
        assert np.allclose(got[i], lamAR * p / (lamI + lamAR), rtol=1e-13, atol=0)
    args = (d['H'].astype(np.float64), d['lag_set'], d['theta'].astype(np.float64))
    with pytest.raises(ValueError, match='lag 0'):
        filter_rows(W64, d['H'].astype(np.float64), np.array([0, 1, 2], dtype=np.uint32), d['theta'].astype(np.float64), d['Y'][OH.FIRST:], OH.FIRST, 0.5, 0.5, True)
    with pytest.raises(ValueError, match='largest lag'):
        filter_rows(W64, args[0], args[1], args[2], d['Y'][4:], 4, 0.5, 0.5, True)
    with pytest.raises(ValueError, match='outside'):
        filter_rows(W64, args[0], args[1], args[2], d['Y'][:0], OH.T + 1, 0.5, 0.5, True)
    with pytest.raises(ValueError, match='row %d' % OH.EMPTY_ROW):      # no ridge at all and an empty row: singular
        filter_rows(W64, args[0], args[1], args[2], d['Y'][OH.FIRST:], OH.FIRST, 0.0, 0.0, True)
    same = filter_rows(W64, args[0], args[1], args[2], d['Y'][OH.T:], OH.T, 0.5, 0.5, True)      # first_row == rows: nothing to do
    assert np.array_equal(same, W64)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_model_assimilate_grows_a_new_model(dtype):
    from trmf import Model, filter_rows
    d = OH.inputs(16)
    m = make_model(d['W'][:OH.FIRST].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    before = (m.W.copy(), m.H.copy(), m.lag_val.copy())
    g = m.assimilate(d['Y'][OH.FIRST:].astype(dtype), 0.5, 50.0, missing=True)
    assert isinstance(g, Model) and g.m == OH.T and m.m == OH.FIRST and g.W.dtype == dtype
    assert all(np.array_equal(a, b) for a, b in zip(before, (m.W, m.H, m.lag_val)))          # the input model is untouched
    assert np.array_equal(g.W[:OH.FIRST], m.W) and np.array_equal(g.H, m.H) and np.array_equal(g.lag_val, m.lag_val)
    assert g.H is not m.H and np.array_equal(g.lag_set, m.lag_set)
    want = filter_rows(np.vstack([m.W, np.zeros((OH.TN, 16), dtype)]), m.H, m.lag_set, m.lag_val, d['Y'][OH.FIRST:].astype(dtype), OH.FIRST, 0.5, 50.0, True)
    assert np.array_equal(g.W, want)
    dense = m.assimilate(np.asarray(d['Y'][OH.FIRST:].todense()).astype(dtype), 0.5, 50.0, missing=False)
    assert np.array_equal(dense.W, OH.twin(d, dtype, 0.5, 50.0, missing=False, W=np.vstack([m.W, np.zeros((OH.TN, 16), dtype)])))


@pytest.mark.parametrize('lamI,lamAR', OH.LAMBDAS)
@pytest.mark.parametrize('k', OH.RANKS)
def test_yardstick_of_the_device_tests_stays_small(k, lamI, lamAR):
    """The fp32 twin's deviation from the fp64 twin on the GPU tests' inputs: the device is gated by 8x this figure, so it must
    not be loose itself (a NumPy trial of these inputs gave at most 3.3e-6)."""
    for missing in (True, False):
        _, dev = OH.yardstick(k, lamI, lamAR, missing)
        print('online yardstick k=%d lambdaI=%g lambdaAR=%g missing=%d: %.3e' % (k, lamI, lamAR, missing, dev))
        assert dev <= 1e-5


def _inputs_as_first_written(k, density=0.3, lags=OH.LAGS):
    """The recipe of online_helpers.inputs before it took a shape, kept here word for word."""
    rng = np.random.RandomState(1000 + k)
    W = rng.rand(96, k).astype(np.float32)
    H = rng.rand(50, k).astype(np.float32)
    theta = rng.randn(len(lags), k)
    theta = np.asfortranarray((theta / (np.abs(theta).sum(axis=0) + 0.1)).astype(np.float32))
    mask = rng.rand(96, 50) < density
    mask[77] = False
    mask[83] = False
    mask[83, 17] = True
    vals = rng.rand(96, 50).astype(np.float32)
    vals[vals == 0] = 0.5
    return W, H, theta, smat.csr_matrix(np.where(mask, vals, np.float32(0)).astype(np.float32))


@pytest.mark.parametrize('k,density', [(1, 0.3), (16, 0.3), (40, 0.7), (64, 1.0)])
def test_generalised_inputs_return_the_old_arrays_for_the_old_arguments(k, density):
    W, H, theta, Y = _inputs_as_first_written(k, density)
    for d in (OH.inputs(k, density), OH.inputs(k, density, OH.LAGS, OH.T, OH.N, OH.FIRST)):
        assert np.array_equal(d['W'], W) and np.array_equal(d['H'], H) and np.array_equal(d['theta'], theta)
        assert d['theta'].flags.f_contiguous and d['lag_set'].tolist() == list(OH.LAGS) and d['k'] == k
        assert np.array_equal(d['Y'].indptr, Y.indptr) and np.array_equal(d['Y'].indices, Y.indices) and np.array_equal(d['Y'].data, Y.data)
    other = OH.inputs(16, 0.3, (1, 7, 30), 64, 50, 40)                      # another shape: the designed rows move with first
    assert other['W'].shape == (64, 16) and other['Y'].shape == (64, 50) and other['theta'].shape == (3, 16)
    assert other['Y'][45].nnz == 0 and other['Y'][51].nnz == 1


@pytest.mark.parametrize('missing', [True, False])
@pytest.mark.parametrize('k', [7, 40])
def test_row_systems_reproduce_filter_rows_in_fp64(k, missing):
    """The fp64 systems the conditioning tests measure the device by (online_helpers.row_systems, prior_of), solved by NumPy,
    are the rows of filter_rows in fp64 to 1e-10 on the standard input -- and the per-entry model of the raw-sparse tests is too."""
    d = OH.inputs(k)
    lamI, lamAR = OH.LAMBDAS[1]
    W = OH.twin(d, np.float64, lamI, lamAR, missing)
    S = OH.row_systems(d, np.float64, lamI, lamAR, missing)
    assert len(S) == OH.TN
    for r, (A, b) in enumerate(S):
        i = OH.FIRST + r
        x = np.linalg.solve(A, b + lamAR * OH.prior_of(W, i, d['lag_set'], d['theta'].astype(np.float64)))
        assert relmax(x, W[i]) <= 1e-10, i
    eta = OH.row_backward_errors(d, S, W, np.float64, lamAR)
    assert eta.max() <= 8 * 2.0 ** -53
    c = d['Y'].tocoo()
    assert relmax(OH.entry_filter(c.row, c.col, c.data, d['W'], d['H'], d['lag_set'], d['theta'], OH.FIRST, lamI, lamAR, missing)[OH.FIRST:],
                  W[OH.FIRST:]) <= 1e-10
    for Wx in (d['W'], W):
        a, b = OH.sq_err(d, Wx, OH.FIRST, missing), OH.sq_err_entries(c.row, c.col, c.data, Wx, d['H'], OH.FIRST, OH.T, missing)
        assert a[1] == b[1] and abs(a[0] - b[0]) <= 1e-12 * a[0]              # one reading on a canonical matrix


@pytest.mark.parametrize('scale,lamI,lamAR', OH.HARD_CASES)
@pytest.mark.parametrize('k', OH.HARD_RANKS)
def test_hard_filter_problem_stays_out_of_the_breakdown_regime(k, scale, lamI, lamAR):
    """filter_rows refuses no case of the hard problem in fp32 (nor in fp64), and the twin's own teacher-forced backward error
    stays below 8 u on both paths: the device gate 4 x max(twin, u) is never a gate against a broken yardstick."""
    from conditioning_helpers import U
    d = OH.hard_filter_problem(k, scale)
    for missing, Y in ((True, d['Y']), (False, d['Yd'])):
        cond = max(float(np.linalg.cond(A)) for A, _ in OH.row_systems(d, np.float64, lamI, lamAR, missing))
        for dtype in (np.float32, np.float64):
            W = OH.twin(d, dtype, lamI, lamAR, missing, d['first'], Y=Y)            # raises where a row breaks down
            eta = OH.row_backward_errors(d, OH.row_systems(d, dtype, lamI, lamAR, missing), W, dtype, lamAR)
            u = U[np.dtype(dtype).name]
            print('hard filter problem k=%d scale=%g lambdaI=%g lambdaAR=%g missing=%d %s: cond up to %.1e, twin eta %.2f u (row %d)' % (
                k, scale, lamI, lamAR, missing, np.dtype(dtype).name, cond, eta.max() / u, d['first'] + int(eta.argmax())))
            assert np.all(np.isfinite(W)) and eta.max() < 8 * u


def test_filter_rows_sums_the_prior_in_lag_set_order_and_counts_a_repeated_lag_twice():
    """An unsorted lag set is refused when a session is created (the lag set of the C interface is ascending), so this order is
    the host's alone; a repeated lag passes both and counts twice."""
    from trmf import filter_rows
    d = OH.inputs(7)
    W64, H64, Y = d['W'].astype(np.float64), d['H'].astype(np.float64), d['Y'][OH.FIRST:].astype(np.float64)
    th = d['theta'].astype(np.float64)
    a = filter_rows(W64, H64, np.array([1, 2, 5]), th, Y, OH.FIRST, 0.5, 0.5, True)
    b = filter_rows(W64, H64, np.array([5, 1, 2]), th[[2, 0, 1]], Y, OH.FIRST, 0.5, 0.5, True)
    assert relmax(b[OH.FIRST:], a[OH.FIRST:]) <= 1e-13
    rep = filter_rows(W64, H64, np.array([1, 2, 2, 5]), th[[0, 1, 1, 2]], Y, OH.FIRST, 0.5, 0.5, True)
    once = filter_rows(W64, H64, np.array([1, 2, 5]), th * np.array([[1.0], [2.0], [1.0]]), Y, OH.FIRST, 0.5, 0.5, True)
    assert relmax(rep[OH.FIRST:], once[OH.FIRST:]) <= 1e-13


def test_fit_noise_reads_a_repeated_cell_as_the_training_objective_does():
    """missing = 0 on a sparse Y with a cell stored twice: ||Y||^2 of the objective is the sum of squares of the stored values, so
    the cell's residual is p^2 + sum_e y_e (y_e - 2 p) -- not (sum_e y_e - p)^2.  A canonical matrix keeps its bits."""
    from trmf import fit_noise
    d = OH.inputs(7)
    c = d['Y'].tocoo()
    args = (d['W'], d['H'], d['lag_set'], d['theta'])
    canon = fit_noise(*args, d['Y'], missing=False)
    dense = fit_noise(*args, np.asarray(d['Y'].todense()), missing=False)
    assert np.array_equal(canon[0], dense[0]) and np.array_equal(canon[1], dense[1])
    dup = smat.coo_matrix((np.concatenate([c.data, c.data[:40] + np.float32(0.25)]),
                           (np.concatenate([c.row, c.row[:40]]), np.concatenate([c.col, c.col[:40]]))), shape=d['Y'].shape)
    got = fit_noise(*args, dup, missing=False)
    want = np.zeros(OH.N)
    for j in range(OH.N):                                                   # series j alone: its entries against the one row h_j
        e = dup.col == j
        want[j] = OH.sq_err_entries(dup.row[e], np.zeros(e.sum(), int), dup.data[e], d['W'], d['H'][j:j + 1], 0, OH.T, False)[0]
    assert np.allclose(got[2]['sq'], want, rtol=1e-12, atol=0) and np.all(got[2]['cnt'] == OH.T)
    merged = fit_noise(*args, dup.tocsr(), missing=False)                  # a caller who sums duplicates first states another problem
    assert not np.allclose(merged[2]['sq'], want, rtol=1e-3)
    per_entry = fit_noise(*args, dup, missing=True)                         # missing = 1: one residual per stored entry
    assert per_entry[2]['cnt'].sum() == dup.nnz


def test_rolling_validate_says_where_an_online_update_does_not_apply():
    import trmf
    Y = np.abs(np.random.RandomState(0).randn(120, 6)) + 0.5
    kw = dict(k=3, window_size=8, nr_windows=3, max_iter=2)
    with pytest.raises(ValueError, match='resident'):
        trmf.rolling_validate(Y, [1, 2, 5], update='assimilate', resident=False, **kw)
    with pytest.raises(ValueError, match='resident'):
        trmf.rolling_validate(smat.csr_matrix(Y), [1, 2, 5], update='assimilate', **kw)
    with pytest.raises(ValueError, match='transform'):
        trmf.rolling_validate(Y, [1, 2, 5], update='assimilate', transform=True, missing=False, **kw)
    with pytest.raises(ValueError, match='retrain'):
        trmf.rolling_validate(Y, [1, 2, 5], update='smooth', **kw)
    with pytest.raises(ValueError, match='transform'):
        trmf.grid_search(Y, [1, 2, 5], {'lambdaI': [0.5]}, update='assimilate', transform=True, missing=False, **kw)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_libraries_export_the_assimilate_entry_point(dtype):
    from trmf import session
    lib = session.lib_for(dtype)
    assert hasattr(lib, 'trmf_session_assimilate')
    assert lib.trmf_session_assimilate.restype is ctypes.c_int32 and len(lib.trmf_session_assimilate.argtypes) == 4


def test_assimilate_sums_layout_matches_header(tmp_path):
    from trmf.session import TrmfAssimilateSums
    names = [name for name, _ in TrmfAssimilateSums._fields_]
    assert names == ['rows', 'entries', 'sq_err_before', 'sq_err_after']
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trmf_abi.h"\n'
                   'int main(void) { printf("%zu", sizeof(TrmfAssimilateSums));\n'
                   + ''.join(' printf(" %%zu", offsetof(TrmfAssimilateSums, %s));\n' % name for name in names)
                   + ' printf("\\n"); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run(['cc', '-I', HEADER_DIR, str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(TrmfAssimilateSums)] + [getattr(TrmfAssimilateSums, name).offset for name in names]
