"""GPU (-m gpu): held-out evaluation on the device (trmf_session_set_heldout / _eval_heldout), live weights (set_lambdas) and the
imputation front end (impute, grid_impute).  Small shapes: the whole file is meant to take well under a minute."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as smat

import oracle_py as O
import trmf
from helpers import TOL, make_model
from trmf import ImputeMetrics, grid_impute, impute, synth
from trmf.impute import _cells_matrix, training_matrix
from trmf.model import NormalizedTransform
from trmf.rf_util import PyMatrix
from trmf.session import Session, TrmfHeldoutSums

pytestmark = pytest.mark.gpu

LAGS = [1, 2, 3, 6]
SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}


def _heldout(T, n, count, seed, zipf=False):
    """Sorted unique cells (rows, cols) and truths: random values of both signs, about 10 % exact zeros."""
    rng = np.random.RandomState(seed)
    if zipf:        # a few series and a few timestamps hold most of the set
        r = np.minimum(rng.zipf(1.6, count * 3) - 1, T - 1)
        c = np.minimum(rng.zipf(1.4, count * 3) - 1, n - 1)
        keys = np.unique(rng.permutation(T)[r].astype(np.int64) * n + rng.permutation(n)[c])[:count]
    else:
        keys = np.unique(rng.randint(0, T * n, size=count).astype(np.int64))
    rows, cols = keys // n, keys % n
    y = rng.uniform(0.5, 2.0, size=keys.size) * rng.choice([-1.0, 1.0], size=keys.size)
    y[rng.rand(keys.size) < 0.1] = 0.0
    return rows, cols, y


def _problem(dtype, k, full, T=240, n=150):
    if full:
        Y = synth.dense_problem(n, T, k, LAGS, dtype=dtype, seed=1)['Y']
    else:
        Y = synth.sparse_problem(n=n, T=T, k=k, nlag=len(LAGS), density=0.15, dtype=dtype, seed=1)['Y']
    m0 = synth.initial_model(Y, LAGS, k, seed=0, dtype=dtype)
    return Y, m0


def _copy(m0):
    return make_model(m0.W, m0.H, m0.lag_val, m0.lag_set)


def _numpy_eval(model, rows, cols, y):
    W, H = model.W.astype(np.float64), model.H.astype(np.float64)
    return np.einsum('ij,ij->i', W[rows], H[cols])


def _check_sums(dev, pred_dev, model, rows, cols, y, dtype):
    ref = _numpy_eval(model, rows, cols, y)
    bound = 4 * model.k * np.finfo(dtype).eps * np.einsum('ij,ij->i', np.abs(model.W[rows].astype(np.float64)), np.abs(model.H[cols].astype(np.float64)))
    assert np.all(np.abs(pred_dev.astype(np.float64) - ref) <= bound + 1e-300)
    d = ref - y
    nz = y != 0
    want = dict(sq_err=np.sum(d * d), abs_err=np.sum(np.abs(d)), abs_truth=np.sum(np.abs(y)), rel_err=np.sum(np.abs(d[nz]) / np.abs(y[nz])))
    assert dev['count'] == y.size and dev['count_nonzero'] == int(nz.sum())
    for key, v in want.items():
        assert abs(dev[key] - v) <= SUM_TOL[dtype] * abs(v), (key, dev[key], v)


CASES = [(np.float32, 8, False, False), (np.float32, 40, False, True), (np.float64, 60, False, False), (np.float32, 96, False, False),
         (np.float64, 96, False, True), (np.float64, 40, True, False), (np.float32, 60, True, False)]


@pytest.mark.parametrize('dtype,k,full,zipf', CASES, ids=['%s-k%d-%s%s' % (np.dtype(c[0]).name, c[1], 'full' if c[2] else 'sparse', '-zipf' if c[3] else '') for c in CASES])
def test_eval_heldout_matches_numpy_of_downloaded_factors(dtype, k, full, zipf):
    Y, m0 = _problem(dtype, k, full)
    T, n = Y.shape
    rows, cols, y = _heldout(T, n, 3000, seed=k, zipf=zipf)
    model = _copy(m0)
    with Session(Y, model, missing=not full, **synth.HYPER) as s:
        s.run(2)
        s.set_heldout(_cells_matrix(y, rows, cols, (T, n), dtype))
        sums, pred = s.eval_heldout_sums(predictions=True)
        sums2, pred2 = s.eval_heldout_sums(predictions=True)
        s.download()
    assert sums == sums2 and np.array_equal(pred, pred2)          # repeated evaluations: the same bits
    _check_sums(sums, pred, model, rows, cols, y, dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_eval_between_runs_leaves_the_trajectory_alone(dtype):
    Y, m0 = _problem(dtype, 16, False)
    rows, cols, y = _heldout(*Y.shape, 2000, seed=5)
    a, b = _copy(m0), _copy(m0)
    with Session(Y, a, **synth.HYPER) as s:
        s.set_heldout(_cells_matrix(y, rows, cols, Y.shape, dtype))
        s.run(3)
        s.eval_heldout(predictions=True)
        st_before = s.stats(3)
        s.run(3).download()
        st = s.stats(6)
    with Session(Y, b, **synth.HYPER) as s:
        s.run(6).download()
        st_ref = s.stats(6)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)
    assert [x['f'] for x in st] == [x['f'] for x in st_ref] and [x['f'] for x in st_before] == [x['f'] for x in st_ref[:3]]


def test_eval_after_append_rows_covers_the_grown_rows():
    dtype = np.float32
    Y, m0 = _problem(dtype, 16, False, T=300)
    T0 = 240
    rows, cols, y = _heldout(T0, Y.shape[1], 1500, seed=7)
    with Session(Y[:T0], synth.initial_model(Y[:T0], LAGS, 16, seed=0, dtype=dtype), **synth.HYPER) as s:
        s.run(2)
        s.set_heldout(_cells_matrix(y, rows, cols, (T0, Y.shape[1]), dtype))
        s.append_rows(Y[T0:])
        s.run(1)
        grown = make_model(np.zeros((300, 16), dtype), s.model.H, s.model.lag_val, LAGS)
        s.model = grown
        s.download()
        sums, pred = s.eval_heldout_sums(predictions=True)      # the old set is still valid
        _check_sums(sums, pred, grown, rows, cols, y, dtype)
        r2, c2, y2 = _heldout(300, Y.shape[1], 1500, seed=8)
        assert r2.max() >= T0
        s.set_heldout(_cells_matrix(y2, r2, c2, (300, Y.shape[1]), dtype))
        sums, pred = s.eval_heldout_sums(predictions=True)
        _check_sums(sums, pred, grown, r2, c2, y2, dtype)


@pytest.mark.parametrize('full', [False, True], ids=['missing', 'full'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_set_lambdas_after_rewind_is_bit_identical_to_a_fresh_session(dtype, full):
    Y, m0 = _problem(dtype, 16, full)
    new = dict(lambdaI=2.0, lambdaAR=5.0, lambdaLag=0.05)
    a, b = _copy(m0), _copy(m0)
    with Session(Y, a, missing=not full, **synth.HYPER) as s:
        s.mark().run(4).rewind()
        s.set_lambdas(new['lambdaI'], new['lambdaAR'], new['lambdaLag']).run(4).download()
    with Session(Y, b, missing=not full, **new) as s:
        s.run(4).download()
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)
    c = _copy(m0)
    with Session(Y, c, missing=not full, **synth.HYPER) as s:         # (the new weights did change something)
        s.run(4).download()
    assert not np.array_equal(a.W, c.W)


def _panel(T=2000, n=60, k=8, seed=0):
    full = synth.imputation_problem(n, T, k, LAGS, observed=1.0, dtype=np.float32, seed=seed)['Y'].toarray()
    rng = np.random.RandomState(seed + 1)
    mask = rng.rand(T, n) < 0.8
    return full, mask


def test_impute_metrics_model_and_training_matrix():
    Y, mask = _panel()
    Y[np.flatnonzero(mask.ravel())[:50] // Y.shape[1], np.flatnonzero(mask.ravel())[:50] % Y.shape[1]] = 0.0   # observed true zeros
    hyper = dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5)
    filled, metrics, model = impute(Y, mask, LAGS, k=8, max_iter=5, seed=0, **hyper)
    miss = ~mask
    rows, cols = np.nonzero(miss)
    pred_np = np.einsum('ij,ij->i', model.W[rows].astype(np.float64), model.H[cols].astype(np.float64))
    ref = ImputeMetrics.generate(Y[rows, cols], pred_np)
    assert metrics.count == ref.count == miss.sum()
    for key in ('nd', 'nrmse', 'mse', 'mape'):
        assert abs(getattr(metrics, key) - getattr(ref, key)) <= 1e-5 * abs(getattr(ref, key)), key
    assert np.array_equal(filled[mask], Y[mask])
    assert np.allclose(filled[miss], pred_np, rtol=1e-4, atol=1e-5)
    # the same factors as train() on the mask-built COO, bit for bit
    Ytr = training_matrix(Y, mask, np.float32)
    m2 = synth.initial_model(Ytr, LAGS, 8, seed=0, dtype=np.float32)
    trmf.train(Ytr, m2, max_iter=5, missing=True, **hyper)
    assert np.array_equal(model.W, m2.W) and np.array_equal(model.H, m2.H) and np.array_equal(model.lag_val, m2.lag_val)
    # the observed zeros are trained on: dropping them (a matrix of the non-zeros) gives other factors
    nzY = smat.csr_matrix(np.where(mask, Y, 0).astype(np.float32))
    assert nzY.nnz == Ytr.nnz - 50
    m3 = synth.initial_model(Ytr, LAGS, 8, seed=0, dtype=np.float32)
    trmf.train(nzY, m3, max_iter=5, missing=True, **hyper)
    assert not np.array_equal(model.H, m3.H)


def test_impute_with_nan_in_missing_cells():
    Y, mask = _panel(T=600, n=30)
    Y = Y.astype(np.float64)
    miss = np.flatnonzero(~mask.ravel())
    Y.ravel()[miss[::2]] = np.nan
    filled, metrics, model = impute(Y, mask, LAGS, k=4, max_iter=3)
    assert np.all(np.isfinite(filled))
    finite = ~mask & np.isfinite(Y)
    assert metrics.count == finite.sum()
    Y.ravel()[miss] = np.nan
    filled, metrics, _ = impute(Y, mask, LAGS, k=4, max_iter=3)
    assert metrics is None and np.all(np.isfinite(filled))


def test_grid_impute_matches_impute_at_every_point():
    Y, mask = _panel(T=800, n=40)
    grid = {'k': [4, 8], 'lambdaI': [0.5, 2.0], 'lambdaAR': [50.0, 5.0]}
    results, best_nrmse, best_nd = grid_impute(Y, mask, LAGS, grid, max_iter=4, seed=0)
    assert len(results) == 8
    for r in results:
        kws = r['kws']
        _, m, _ = impute(Y, mask, LAGS, k=kws['k'], lambdaI=kws['lambdaI'], lambdaAR=kws['lambdaAR'], lambdaLag=kws['lambdaLag'],
                         max_iter=4, seed=0)
        assert m == r['metrics'], kws
    assert best_nrmse['metrics'].nrmse == min(r['metrics'].nrmse for r in results)
    assert best_nd['metrics'].nd == min(r['metrics'].nd for r in results)


def _raw(s):
    """Direct ABI calls (outputs prefilled with sentinels)."""
    sums = TrmfHeldoutSums(7, 7, 7.0, 7.0, 7.0, 7.0)
    pred = np.full(8, -3.0, dtype=s.model.W.dtype)
    rc = s.lib.trmf_session_eval_heldout(s.handle, ctypes.byref(sums), pred.ctypes.data)
    return rc, sums.as_dict(), pred


def _rejections(s, Y, dtype):
    T, n = Y.shape
    rc, sums, pred = _raw(s)                                              # no held-out set yet
    assert rc == -1 and sums['count'] == 7 and np.all(pred == -3.0)
    assert 'no held-out set' in s.lib.trmf_last_error().decode()
    with pytest.raises(RuntimeError):
        s.set_heldout(PyMatrix(np.ones((4, n), dtype=dtype), dtype=dtype))   # not sparse
    with pytest.raises(RuntimeError):
        s.set_heldout(smat.csr_matrix(np.ones((4, n + 1), dtype=dtype)))     # wrong column count
    with pytest.raises(RuntimeError):
        s.set_heldout(smat.csr_matrix(np.ones((T + 1, n), dtype=dtype)))     # more rows than the session
    bad = PyMatrix(smat.csr_matrix(np.ones((3, n), dtype=dtype)), dtype=dtype)
    bad.py_buf['col_idx'][5] = n + 3                                      # an index out of range
    with pytest.raises(RuntimeError):
        s.set_heldout(bad)
    with pytest.raises(RuntimeError):
        s.set_lambdas(float('nan'), 1.0, 1.0)
    rows, cols, y = _heldout(T, n, 500, seed=2)
    s.run(1)
    s.set_heldout(_cells_matrix(y, rows, cols, (T, n), dtype))
    return s.run(1).eval_heldout_sums()


@pytest.mark.parametrize('devices', [None, '0,0'])
def test_rejected_calls_leave_the_session_usable(devices, monkeypatch):
    dtype = np.float32
    if devices:
        monkeypatch.setenv('TRMF_DEVICES', devices)
    Y, m0 = _problem(dtype, 16, False)
    with Session(Y, _copy(m0), **synth.HYPER) as s:
        sums = _rejections(s, Y, dtype)
        assert sums['count'] > 0
    Yd, md = _problem(dtype, 8, True)                                  # a session training on a series transform
    with Session(Yd, _copy(md), missing=False, **synth.HYPER) as s:
        rows, cols, y = _heldout(*Yd.shape, 300, seed=4)
        s.set_heldout(_cells_matrix(y, rows, cols, Yd.shape, dtype))
        s.set_transform(NormalizedTransform(Yd))
        rc, sums, pred = _raw(s)
        assert rc == -1 and sums['count'] == 7 and np.all(pred == -3.0)
        assert 'series transform' in s.lib.trmf_last_error().decode()
        s.run(1).sync()                                                   # still usable


def test_group_sums_are_bit_identical_to_one_rank(monkeypatch):
    dtype = np.float32
    Y, m0 = _problem(dtype, 16, False)
    rows, cols, y = _heldout(*Y.shape, 3000, seed=9)
    out = []
    for env in ({'TRMF_TILE': 'narrow'}, {'TRMF_DEVICES': '0,0'}):
        for key in ('TRMF_TILE', 'TRMF_DEVICES'):
            monkeypatch.delenv(key, raising=False)
        for key, v in env.items():
            monkeypatch.setenv(key, v)
        with Session(Y, _copy(m0), **synth.HYPER) as s:
            s.set_heldout(_cells_matrix(y, rows, cols, Y.shape, dtype))
            s.run(3)
            out.append(s.eval_heldout_sums(predictions=True))
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


def test_metrics_agree_with_the_reference_build_factors():
    """fp64, one small case: the device's metrics of its own factors against the host metrics of the factors the reference
    build (or, where it is absent, the C restatement) trains from the same start.  Parity gate of the factors (helpers.TOL,
    1e-6 relative) -> the same order on the scores, whose truths are independent of the model (errors of order one)."""
    dtype = np.float64
    p = synth.sparse_problem(n=200, T=150, k=8, nlag=3, density=0.1, dtype=dtype, seed=3)
    m0 = synth.initial_model(p['Y'], p['lag_set'], 8, seed=0, dtype=dtype)
    W, H, Th = m0.W.copy(), m0.H.copy(), np.asfortranarray(m0.lag_val.copy())
    cpu_train = O.train_ref if O.ref(np.float64) is not None else O.train_port
    cpu_train(p['Y'], p['lag_set'], W, H, Th, synth.HYPER, max_iter=5)
    rows, cols, y = _heldout(150, 200, 2000, seed=11)
    with Session(p['Y'], _copy(m0), **synth.HYPER) as s:
        s.run(5)
        s.set_heldout(_cells_matrix(y, rows, cols, (150, 200), dtype))
        got = s.eval_heldout()
    ref = ImputeMetrics.generate(y, np.einsum('ij,ij->i', W[rows], H[cols]))
    tol = TOL['float64']['factor'] * 10
    for key in ('nd', 'nrmse', 'mse', 'mape'):
        assert abs(getattr(got, key) - getattr(ref, key)) <= tol * abs(getattr(ref, key)), key
