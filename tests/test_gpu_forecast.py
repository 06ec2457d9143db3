"""GPU (-m gpu): forecasting and scoring on the device (trmf_session_forecast / _forecast_scores / _forecast_reset), the rolling
evaluation that uses them (rolling_validate(forecast_on_device=True)) and append_rows above rank 64.  Small shapes: the whole file
is meant to take well under a minute."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as smat

import trmf
from forecast_helpers import fields, series_sums
from helpers import make_model
from trmf import Metrics, synth
from trmf.model import NormalizedTransform
from trmf.rf_util import PyMatrix
from trmf.session import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, 'golden', 'py_harness.npz'))
LAGS = [1, 2, 3, 6]
LAGS_WEEK = list(range(1, 25)) + list(range(168, 192))          # the paper scripts' 48 lags: reach 191
SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}                 # tests/test_gpu_impute.py


def _sparse(dtype, k, lags, T, n=150):
    rng = np.random.RandomState(1)
    Y = smat.random(T, n, density=0.15, random_state=rng, format='csr', dtype=np.float64)
    Y.data = rng.randn(Y.nnz)
    Y = Y.astype(dtype)
    return Y, synth.initial_model(Y, lags, k, seed=0, dtype=dtype)


def _dense(dtype, k, lags=LAGS, T=240, n=150):
    Y = synth.dense_problem(n, T, k, lags, dtype=dtype, seed=1)['Y']
    return Y, synth.initial_model(Y, lags, k, seed=0, dtype=dtype)


def _copy(m0):
    return make_model(m0.W, m0.H, m0.lag_val, m0.lag_set)


def _truth(steps, n, dtype, seed, zeros=True):
    """Values of both signs, about 10 % exact zeros."""
    rng = np.random.RandomState(seed)
    y = rng.uniform(0.5, 2.0, size=(steps, n)) * rng.choice([-1.0, 1.0], size=(steps, n))
    if zeros:
        y[rng.rand(steps, n) < 0.1] = 0.0
    return y.astype(dtype)


def _dot_reference(Wnew, H, dtype):
    """fp64 product and the elementwise bound of a k-term dot product in the element type (tests/test_gpu_impute.py:_check_sums)."""
    W64, H64 = Wnew.astype(np.float64), H.astype(np.float64)
    return W64.dot(H64.T), 4 * H.shape[1] * np.finfo(dtype).eps * np.abs(W64).dot(np.abs(H64).T)


# ---- 1. the roll-out --------------------------------------------------------------------------------------------------------
ROLL = [(dt, k, lags, T, False) for dt in (np.float32, np.float64) for k in (8, 40, 60, 96, 130) for lags, T in ((LAGS, 240), (LAGS_WEEK, 400))]
# the form that reads its rows from global memory (a lag set whose LDS ring would not fit), forced where the ring does fit
ROLL += [(np.float64, 40, LAGS_WEEK, 400, True), (np.float32, 130, LAGS, 240, True)]


@pytest.mark.parametrize('dtype,k,lags,T,from_global', ROLL,
                         ids=['%s-k%d-reach%d%s' % (np.dtype(c[0]).name, c[1], c[2][-1], '-global' if c[4] else '') for c in ROLL])
def test_rollout_is_bit_identical_to_latent_forecast(dtype, k, lags, T, from_global, monkeypatch):
    if from_global:
        monkeypatch.setenv('TRMF_FORECAST_GLOBAL', '1')
    Y, m0 = _sparse(dtype, k, lags, T)
    model = _copy(m0)
    with Session(Y, model, **synth.HYPER) as s:
        s.run(2)
        got = {steps: s.forecast(steps, return_forecast=False, return_latent=True) for steps in (1, 24, 200)}
        s.download()
    for steps, Wnew in got.items():
        want = model.latent_forecast(steps)[model.m:]
        assert Wnew.dtype == dtype and Wnew.shape == (steps, k)
        assert np.array_equal(Wnew, want), (steps, np.abs(Wnew - want).max())


# ---- 2. forecast values -----------------------------------------------------------------------------------------------------
VALUES = [(np.float32, 8), (np.float64, 40), (np.float32, 60), (np.float64, 96), (np.float32, 130)]


@pytest.mark.parametrize('dtype,k', VALUES, ids=['%s-k%d' % (np.dtype(c[0]).name, c[1]) for c in VALUES])
def test_forecast_values_plain_and_clipped(dtype, k):
    Y, m0 = _sparse(dtype, k, LAGS, 240)
    model = _copy(m0)
    with Session(Y, model, **synth.HYPER) as s:
        s.run(2)
        Ynew, Wnew = s.forecast(24, return_latent=True)
        thr = float(np.median(Ynew))
        Yclip = s.forecast(24, threshold=thr)
        s.download()
    assert np.array_equal(Wnew, model.latent_forecast(24)[model.m:])
    ref, bound = _dot_reference(Wnew, model.H, dtype)
    assert Ynew.dtype == dtype and Ynew.shape == (24, Y.shape[1])
    assert np.all(np.abs(Ynew.astype(np.float64) - ref) <= bound + 1e-300)
    thr = float(dtype(thr))                                     # the threshold as the element type holds it
    clear = np.abs(ref - thr) > bound                           # elements whose side of the threshold rounding cannot change
    assert clear.mean() > 0.9 and (ref < thr)[clear].any() and (ref > thr)[clear].any()
    assert np.all(np.abs(Yclip.astype(np.float64) - np.maximum(ref, thr))[clear] <= bound[clear] + 1e-300)
    assert np.all(Yclip >= dtype(thr))


@pytest.mark.parametrize('dtype,k', [(np.float32, 40), (np.float64, 60), (np.float64, 96)], ids=['float32-k40', 'float64-k60', 'float64-k96'])
def test_forecast_values_through_a_series_transform(dtype, k):
    Y, m0 = _dense(dtype, k)
    Y = np.ascontiguousarray(Y * np.linspace(0.5, 30.0, Y.shape[1]).astype(dtype) + dtype(3.0))       # series of different level and scale
    tr = NormalizedTransform(Y)
    model = _copy(m0)
    with Session(Y, model, missing=False, **synth.HYPER) as s:
        s.set_transform(tr)
        s.run(2)
        Ynew, Wnew = s.forecast(24, return_latent=True)
        s.download()
    assert np.array_equal(Wnew, model.latent_forecast(24)[model.m:])
    y64, bound = _dot_reference(Wnew, model.H, dtype)
    a, b = tr.a.astype(np.float64), tr.b.astype(np.float64)
    ref = (y64 - b) / a                                          # transform.postprocess of the fp64 product
    eps = np.finfo(dtype).eps
    assert np.all(np.abs(Ynew.astype(np.float64) - ref) <= bound / np.abs(a) + 4 * eps * (np.abs(y64) + np.abs(b)) / np.abs(a))


# ---- 3. scores of one call --------------------------------------------------------------------------------------------------
SCORES = [(np.float32, 8), (np.float64, 40), (np.float32, 60), (np.float64, 96), (np.float32, 130)]


@pytest.mark.parametrize('dtype,k', SCORES, ids=['%s-k%d' % (np.dtype(c[0]).name, c[1]) for c in SCORES])
def test_scores_of_one_call_match_numpy_of_the_returned_forecast(dtype, k):
    Y, m0 = _sparse(dtype, k, LAGS, 240, n=333)                 # (two workgroups, the second one partly idle)
    truth = _truth(24, 333, dtype, seed=k)
    with Session(Y, _copy(m0), **synth.HYPER) as s:
        s.run(2)
        assert s.forecast_series_sums()[0] == 0 and not s.forecast_series_sums()[1].any()
        Ynew = s.forecast(24, truth=truth)
        rows, table = s.forecast_series_sums()
        assert np.array_equal(s.forecast(24), Ynew)             # scoring does not change the forecast
    want = series_sums(truth, Ynew)
    assert rows == 24 and table.shape == (333, 6)
    assert np.array_equal(table[:, 5], want[:, 5]) and 0 < want[:, 5].sum() < truth.size
    assert np.all(np.abs(table - want) <= SUM_TOL[dtype] * np.abs(want)), np.abs(table / want - 1).max()


# ---- 4. accumulation across windows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('refit', [False, True], ids=['raw', 'refitted-transform'])
def test_scores_accumulate_across_windows_and_reset(refit):
    dtype, k, T0, win = np.float64, 40, 240, 8
    Y, _ = _dense(dtype, k, T=T0 + 3 * win)
    Y = np.ascontiguousarray(Y * np.linspace(0.5, 5.0, Y.shape[1]) + 1.0)
    assert not (Y == 0).any()
    m0 = synth.initial_model(Y[:T0], LAGS, k, seed=0, dtype=dtype)
    forecasts = []
    with Session(Y[:T0], m0, missing=False, **synth.HYPER) as s:
        if refit:
            s.set_transform(NormalizedTransform(Y[:T0]))
        for w in range(3):
            cut = T0 + w * win
            if w:
                s.append_rows(Y[cut - win:cut])
                if refit and w == 2:
                    s.set_transform(NormalizedTransform(Y[:cut]))
            s.run(2)
            forecasts.append(s.forecast(win, truth=Y[cut:cut + win]))
        rows, table = s.forecast_series_sums()
        got = s.forecast_scores()
        # from the final state: the same three calls after a reset give the same bits again
        runs = []
        for _ in range(2):
            s.reset_forecast_scores()
            assert s.forecast_series_sums()[0] == 0 and not s.forecast_series_sums()[1].any()
            for w in range(3):
                s.forecast(win, truth=Y[T0 + w * win:T0 + (w + 1) * win], return_forecast=False)
            runs.append(s.forecast_series_sums())
    assert rows == 3 * win
    want = Metrics.generate(Y[T0:], np.vstack(forecasts))
    assert np.allclose(fields(got), fields(want), rtol=1e-12, atol=0), (got, want)
    assert np.allclose(table, series_sums(Y[T0:], np.vstack(forecasts)), rtol=1e-12, atol=0)
    assert runs[0][0] == runs[1][0] == 3 * win and np.array_equal(runs[0][1], runs[1][1]) and runs[0][1].any()


# ---- 5. no side effects -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_forecast_between_runs_leaves_the_trajectory_alone(dtype):
    Y, m0 = _sparse(dtype, 16, LAGS, 240)
    truth = _truth(24, Y.shape[1], dtype, seed=3)
    a, b = _copy(m0), _copy(m0)
    with Session(Y, a, **synth.HYPER) as s:
        s.run(2)
        first = s.forecast(24, truth=truth, return_latent=True)
        second = s.forecast(24, truth=truth, return_latent=True)
        s.run(2).download()
        st = s.stats(4)
    with Session(Y, b, **synth.HYPER) as s:
        s.run(2).run(2).download()
        st_ref = s.stats(4)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)
    keep = [key for key in st[0] if not key.startswith('ms_')]              # (the phase times are wall-clock measurements)
    assert len(st) == len(st_ref) == 4 and [[x[key] for key in keep] for x in st] == [[x[key] for key in keep] for x in st_ref]


# ---- 6. end to end against the reference's capture ---------------------------------------------------------------------------
def test_rolling_validate_on_device_matches_reference_harness():
    Y = GOLD['rv_Y']
    kw = dict(k=3, window_size=8, nr_windows=3, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=4, threads=2, seed=0)
    for missing in (False, True):
        got = trmf.rolling_validate(Y, [1, 2, 5], missing=missing, threshold=0, forecast_on_device=True, **kw)
        assert np.allclose(fields(got), GOLD['rv_missing%d' % int(missing)], rtol=1e-7), missing
    got = trmf.rolling_validate(Y, [1, 2, 5], missing=False, threshold=None, transform=True, forecast_on_device=True, **kw)
    assert np.allclose(fields(got), GOLD['rv_transform'], rtol=1e-7)


def test_grid_search_on_device_matches_reference_harness(capsys):
    results, best = trmf.grid_search(GOLD['rv_Y'], [1, 2, 5], {'lambdaI': [0.5, 5.0], 'lambdaAR': [5, 50]}, k=3, window_size=8,
                                     nr_windows=2, max_iter=3, missing=True, threshold=0, threads=2, seed=0, forecast_on_device=True)
    assert all(r['kws']['forecast_on_device'] for r in results)
    assert np.allclose([r['metrics'].m_nd for r in results], GOLD['gs_m_nd'], rtol=1e-7)
    assert np.allclose(fields(best), GOLD['gs_best'], rtol=1e-7)
    assert 'm_nd=' in capsys.readouterr().out


# ---- 7. several ranks -------------------------------------------------------------------------------------------------------
def _group_case(out_path):
    """Body of the child processes of the test below: train, forecast and score, save everything."""
    dtype = np.float32
    Y, m0 = _sparse(dtype, 16, LAGS, 240)
    truth = _truth(24, Y.shape[1], dtype, seed=9)
    with Session(Y, _copy(m0), **synth.HYPER) as s:
        s.run(3)
        Ynew, Wnew = s.forecast(24, truth=truth, return_latent=True)
        rows, table = s.forecast_series_sums()
        np.savez(out_path, Ynew=Ynew, Wnew=Wnew, rows=rows, table=table, metrics=fields(s.forecast_scores()), describe=s.describe())


def test_group_forecast_is_bit_identical_to_one_rank(tmp_path):
    out = []
    for tag, extra in (('one', {'TRMF_TILE': 'narrow'}), ('two', {'TRMF_DEVICES': '0,0'})):
        env = {key: v for key, v in os.environ.items() if key not in ('TRMF_TILE', 'TRMF_DEVICES')}
        env.update(extra, TRMF_TEST='1', PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
        path = str(tmp_path / (tag + '.npz'))
        code = 'import test_gpu_forecast as t; t._group_case(%r)' % path
        done = subprocess.run([sys.executable, '-c', code], env=env, cwd=HERE, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stderr[-2000:]
        out.append(np.load(path))
    assert '2 ranks' in str(out[1]['describe']) and '1 rank' in str(out[0]['describe'])
    for key in ('Ynew', 'Wnew', 'rows', 'table', 'metrics'):
        assert np.array_equal(out[0][key], out[1][key]), key
    assert out[0]['rows'] == 24 and out[0]['table'].any()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('devices', [None, '0,0'])
def test_refused_calls_leave_everything_alone(devices, monkeypatch):
    dtype = np.float32
    if devices:
        monkeypatch.setenv('TRMF_DEVICES', devices)
    Y, m0 = _sparse(dtype, 16, LAGS, 240)
    n, k = Y.shape[1], 16
    truth = _truth(8, n, dtype, seed=4)
    model = _copy(m0)
    with Session(Y, model, **synth.HYPER) as s:
        s.run(1)
        s.forecast(8, truth=truth, return_forecast=False)
        before = s.forecast_series_sums()

        def refused(steps, py_truth, needle):
            Ynew, Wnew = np.full((8, n), -3.0, dtype), np.full((8, k), -3.0, dtype)
            rc = s.lib.trmf_session_forecast(s.handle, steps, 0, 0.0, ctypes.byref(py_truth) if py_truth is not None else None,
                                             Ynew.ctypes.data, Wnew.ctypes.data)
            assert rc == -1 and needle in s.lib.trmf_last_error().decode(), s.lib.trmf_last_error().decode()
            assert np.all(Ynew == -3.0) and np.all(Wnew == -3.0)
            after = s.forecast_series_sums()
            assert after[0] == before[0] and np.array_equal(after[1], before[1])

        refused(0, None, 'steps')
        refused(8, PyMatrix(smat.csr_matrix(truth), dtype=dtype), 'dense')
        refused(8, PyMatrix(np.ascontiguousarray(truth[:, :-1]), dtype=dtype), 'truth is')
        refused(8, PyMatrix(truth[:5], dtype=dtype), 'truth is')
        with pytest.raises(RuntimeError):
            s.forecast(0)
        with pytest.raises(RuntimeError):
            s.forecast(8, truth=smat.csr_matrix(truth))
        with pytest.raises(TypeError):
            s.forecast(8, truth=truth.astype(np.float64))                   # the other element type
        after = s.forecast_series_sums()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
        # the session (under TRMF_DEVICES: the group) still runs and forecasts correctly
        s.run(1)
        Ynew, Wnew = s.forecast(8, truth=np.asfortranarray(truth), return_latent=True)      # (a column-major truth is dense too)
        rows, table = s.forecast_series_sums()
        s.download()
    assert np.array_equal(Wnew, model.latent_forecast(8)[model.m:])
    ref, bound = _dot_reference(Wnew, model.H, dtype)
    assert np.all(np.abs(Ynew.astype(np.float64) - ref) <= bound + 1e-300)
    want = before[1] + series_sums(truth, Ynew, prev=truth[-1])
    assert rows == 16 and np.all(np.abs(table - want) <= SUM_TOL[dtype] * np.abs(want))


# ---- 9. append_rows above rank 64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_append_rows_rolls_every_column_forward_above_rank_64(dtype):
    """On the commit before this test the appended rows of W had only their first 64 columns rolled forward (one 64-thread
    workgroup, one thread per latent dimension): columns 64.. of the new rows stayed zero."""
    k, T0, Tn = 96, 240, 24
    Y, _ = _sparse(dtype, k, LAGS, T0 + Tn)
    prev = synth.initial_model(Y[:T0], LAGS, k, seed=0, dtype=dtype)
    with Session(Y[:T0], prev, **synth.HYPER) as s:
        s.run(2).download()
        s.append_rows(Y[T0:])
        grown = make_model(np.zeros((T0 + Tn, k), dtype), prev.H, prev.lag_val, LAGS)
        s.model = grown
        s.download()
    want = prev.latent_forecast(Tn)
    assert np.array_equal(grown.W[:T0], prev.W)
    assert np.array_equal(grown.W[T0:, :64], want[T0:, :64])
    assert np.array_equal(grown.W[T0:], want[T0:]), 'columns 64.. differ: %d of them zero' % int((grown.W[T0:, 64:] == 0).sum())
