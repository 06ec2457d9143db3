"""GPU (-m gpu): the fixed-interval smoother on the device -- trmf_session_smooth (smooth_ar_kernel, smooth_apply_kernel,
smooth_update_kernel, smooth_finish_kernel) behind Session.smooth / Session.update(smooth_back=) and
rolling_validate(update='assimilate', smooth_back=).  Small shapes: the whole file takes a few seconds.

The yardstick.  The truth is trmf.smooth_rows in fp64 (a direct solve of the window's system) on the factors the session holds.
The device runs preconditioned conjugate gradients to rtol 1e-5 (fp32) / 1e-10 (fp64), so its distance from the truth is the
truncation error of the iteration plus rounding; the PCG twin of smooth_helpers.py runs the same iteration in NumPy in the same
element type and order of operations.  The device may be no farther from the truth (max |x - x*| / max |x*|) than 8 x the twin is
on the same input, must report convergence, and must take the twin's number of steps +- 2."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as smat

import online_helpers as OH
import smooth_helpers as SH
import trmf
from forecast_helpers import fields
from helpers import evidence, make_model, relmax
from trmf import Metrics, synth
from trmf.rf_util import PyMatrix
from trmf.session import Session, TrmfSmoothSums

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}             # the tolerance tests/test_gpu_online.py uses for the same sums
IDS = ['float32', 'float64']


def _model(d, dtype, rows=None):
    m = make_model(d['W'][:rows].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    if d['k'] == 1:     # PyMatrix tags a (rows, 1) array column-major, like the reference's; the two orders are the same bytes
        m.pyW.type = m.pyH.type = PyMatrix.DENSE_ROWMAJOR
    return m


def _training(d, dtype, storage):
    Y = d['Y'].astype(dtype)
    return np.ascontiguousarray(Y.toarray()) if storage == 'dense' else Y


def _smooth(d, dtype, lamI, lamAR, first, missing=True, storage='sparse', max_iter=SH.MAX_ITER):
    """(downloaded model, sums, Wnew, describe) of one session over the input set after smooth(first)."""
    model = _model(d, dtype)
    with Session(_training(d, dtype, storage), model, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5, missing=missing) as s:
        assert np.array_equal(s.download().W, d['W'].astype(dtype))      # the truth's W is the session's own
        sums, Wnew = s.smooth(first, rtol=SH.RTOL[np.dtype(dtype)], max_iter=max_iter, return_latent=True)
        s.download()
        return model, sums, Wnew, s.describe()


def _gate(what, d, model, sums, Wnew, dtype, lamI, lamAR, first, missing=True, **kw):
    want, dist, steps, converged = SH.yardstick(d['k'], lamI, lamAR, first, np.dtype(dtype), missing, **kw)
    assert converged
    got = SH.measure(model.W[first:], want[first:])
    evidence('smoother %s %s lambdaI=%g lambdaAR=%g first_row=%d: distance to the fp64 direct solve %.3e = %.2f x the twin\'s %.3e '
             '(gate 8 x); steps %d, twin %d; residual %.2e' % (what, np.dtype(dtype).name, lamI, lamAR, first, got, got / dist, dist,
                                                              sums['iterations'], steps, sums['residual']))
    assert np.array_equal(model.W[:first], d['W'][:first].astype(dtype))              # earlier rows keep their bits
    assert np.array_equal(Wnew, model.W[first:])
    assert sums['rows'] == d['W'].shape[0] - first
    assert got <= SH.GATE * dist, (what, got, dist)
    assert sums['converged'] == 1 and sums['residual'] <= SH.RTOL[np.dtype(dtype)]
    assert abs(sums['iterations'] - steps) <= SH.ITER_SLACK, (what, sums['iterations'], steps)
    # the two objectives against the host's fp64 J_win
    tol = SH.OBJ_TOL[np.dtype(dtype)]
    before = SH.objective_of(d, d['W'].astype(dtype), lamI, lamAR, first, missing)
    after = SH.objective_of(d, model.W, lamI, lamAR, first, missing)
    assert abs(sums['objective_before'] - before) <= tol * before and abs(sums['objective_after'] - after) <= tol * after, (sums, before, after)
    assert sums['objective_after'] <= sums['objective_before']


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first', SH.FIRSTS)
@pytest.mark.parametrize('lamI,lamAR', OH.LAMBDAS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('k', OH.RANKS)
def test_smooth_matches_the_direct_solve_within_the_twins_distance(k, dtype, lamI, lamAR, first):
    d = SH.inputs(k)
    model, sums, Wnew, _ = _smooth(d, dtype, lamI, lamAR, first)
    _gate('k=%d' % k, d, model, sums, Wnew, dtype, lamI, lamAR, first)
    assert sums['entries'] == d['Y'][first:].nnz


# ---- 2. geometry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name,kw', SH.GEOMETRY, ids=[g[0] for g in SH.GEOMETRY])
def test_window_and_lag_geometry(name, kw, dtype):
    kw = dict(kw)
    k, first, missing = kw.pop('k'), kw.pop('first'), kw.pop('missing', True)
    lamI, lamAR = SH.GEOMETRY_LAMBDAS
    ikw = {key: kw[key] for key in ('lags', 'T', 'N') if key in kw}
    d = SH.inputs(k, 0.3, first=kw.get('ifirst', OH.FIRST), **ikw)
    model, sums, Wnew, _ = _smooth(d, dtype, lamI, lamAR, first, missing, 'dense' if not missing else 'sparse')
    _gate(name, d, model, sums, Wnew, dtype, lamI, lamAR, first, missing, **kw)


LAYOUTS = [('k-by-k', {}, 'sparse', True, ''),
           ('packed', {'TRMF_NO_HV_TILE': '1'}, 'sparse', True, 'unfused'),
           ('shared-dense', {}, 'dense', False, ''),
           ('shared-sparse', {}, 'sparse', False, ''),
           ('theta-from-global', {'TRMF_FORECAST_GLOBAL': '1'}, 'sparse', True, '')]


@pytest.mark.parametrize('dtype,k', [(np.float32, 40), (np.float64, 7)], ids=['float32-k40', 'float64-k7'])
@pytest.mark.parametrize('name,env,storage,missing,must', LAYOUTS, ids=[p[0] for p in LAYOUTS])
def test_every_gram_layout(name, env, storage, missing, must, dtype, k, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    lamI, lamAR = OH.LAMBDAS[0]
    first = SH.FIRSTS[0]
    d = SH.inputs(k)
    model, sums, Wnew, desc = _smooth(d, dtype, lamI, lamAR, first, missing, storage)
    assert must in desc, desc
    _gate(name, d, model, sums, Wnew, dtype, lamI, lamAR, first, missing)
    assert sums['entries'] == (OH.TN * OH.N if not missing else d['Y'][first:].nnz)
    for key, W in (('sq_err_before', d['W'].astype(dtype)), ('sq_err_after', model.W)):
        want, _ = OH.sq_err(d, W, first, missing)
        assert abs(sums[key] - want) <= SUM_TOL[dtype] * abs(want), (key, sums[key], want)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_one_row_and_lags_beyond_the_window_are_the_filter(dtype):
    k, (lamI, lamAR) = 40, OH.LAMBDAS[1]
    for lags, first in ((OH.LAGS, OH.T - 1), ((30, 40), OH.FIRST)):
        d = SH.inputs(k, lags=lags)
        w64, dev32 = OH.yardstick_of(d, lamI, lamAR, True, first)
        model = _model(d, dtype)
        with Session(_training(d, dtype, 'sparse'), model, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5) as s:
            sums = s.smooth(first, rtol=SH.RTOL[np.dtype(dtype)], max_iter=SH.MAX_ITER)
            s.download()
        twin = _model(d, dtype)
        with Session(_training(d, dtype, 'sparse'), twin, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5) as s:
            s.assimilate(first)
            s.download()
        b = OH.bound(dtype, dev32)
        got, filt = relmax(model.W[first:], w64[first:]), relmax(twin.W[first:], w64[first:])
        evidence('smoother lags %s first_row %d %s: %.3e from the fp64 filter twin (assimilate %.3e, bound %.3e), %d steps' % (
            lags, first, np.dtype(dtype).name, got, filt, b, sums['iterations']))
        assert got <= b and filt <= b and sums['converged'] == 1
        assert sums['iterations'] <= 3                           # the preconditioner is exact: one step, the residual replacement, one refinement step


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_an_empty_window_is_a_no_op_with_zero_sums(dtype):
    d = SH.inputs(16)
    model = _model(d, dtype)
    with Session(_training(d, dtype, 'sparse'), model, lambdaLag=0.5) as s:
        sums, Wnew = s.smooth(OH.T, return_latent=True)
        assert sums == dict(rows=0, entries=0, iterations=0, converged=0, residual=0.0, sq_err_before=0.0, sq_err_after=0.0,
                            objective_before=0.0, objective_after=0.0) and Wnew.shape == (0, 16)
        assert np.array_equal(s.download().W, d['W'].astype(dtype))


def test_the_window_cap_is_refused_by_name(monkeypatch):
    dtype = np.float32
    d = SH.inputs(16)
    model = _model(d, dtype)
    monkeypatch.setenv('TRMF_SMOOTH_MAX_ROWS', '23')
    with Session(_training(d, dtype, 'sparse'), model, lambdaLag=0.5) as s:
        with pytest.raises(RuntimeError, match='cap of 23 rows'):
            s.smooth(OH.FIRST)                                               # 24 rows
        assert np.array_equal(s.download().W, d['W'].astype(dtype))
        sums = TrmfSmoothSums()                                              # ... and the outputs keep their bytes
        ctypes.memset(ctypes.byref(sums), 0x5a, ctypes.sizeof(sums))
        marked = bytes(sums)
        Wnew = np.full((OH.TN, 16), 7, dtype=dtype)
        assert s.lib.trmf_session_smooth(s.handle, OH.FIRST, 0.0, 0, ctypes.byref(sums), Wnew.ctypes.data) == -1
        assert bytes(sums) == marked and (Wnew == 7).all() and np.array_equal(s.download().W, d['W'].astype(dtype))
        assert s.smooth(OH.FIRST + 1)['rows'] == 23


# ---- 3. behaviour ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_call_that_reaches_max_iter_still_commits_and_lowers_the_objective(dtype):
    k, (lamI, lamAR) = 40, OH.LAMBDAS[0]
    d = SH.inputs(k)
    model, sums, Wnew, _ = _smooth(d, dtype, lamI, lamAR, SH.FIRSTS[1], max_iter=1)
    assert sums['converged'] == 0 and sums['iterations'] == 1 and 0 < sums['residual'] < 1e3
    assert not np.array_equal(model.W[SH.FIRSTS[1]:], d['W'][SH.FIRSTS[1]:].astype(dtype)) and np.array_equal(Wnew, model.W[SH.FIRSTS[1]:])
    assert sums['objective_after'] <= sums['objective_before']
    after = SH.objective_of(d, model.W, lamI, lamAR, SH.FIRSTS[1])
    assert abs(sums['objective_after'] - after) <= SH.OBJ_TOL[np.dtype(dtype)] * after


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_identical_calls_from_the_same_state_give_the_same_bits(dtype):
    k, (lamI, lamAR) = 40, OH.LAMBDAS[0]
    d = SH.inputs(k)
    a = _smooth(d, dtype, lamI, lamAR, SH.FIRSTS[1])
    b = _smooth(d, dtype, lamI, lamAR, SH.FIRSTS[1])
    assert np.array_equal(a[0].W, b[0].W) and np.array_equal(a[2], b[2]) and a[1] == b[1]


@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_two_ranks_are_bit_identical_to_one(storage, missing, monkeypatch):
    dtype, k = np.float32, 40
    d = SH.inputs(k)

    def run():
        model = _model(d, dtype)
        with Session(_training(d, dtype, storage), model, missing=missing, lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5) as s:
            sums, Wnew = s.smooth(SH.FIRSTS[1], return_latent=True)
            return s.download().W.copy(), sums, Wnew, s.describe()

    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = run()
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two = run()
    assert '1 rank' in one[3] and '2 ranks' in two[3]
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2]) and one[1] == two[1]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_refused_calls_leave_w_the_outputs_and_the_session_as_they_were(dtype):
    d = SH.inputs(16, 1.0)         # every cell stored but for the two designed rows: the empty row is the first singular block
    Y = _training(d, dtype, 'sparse')
    W0 = d['W'].astype(dtype)

    def refused(s, match, first=OH.FIRST, rtol=0.0, max_iter=0):
        sums = TrmfSmoothSums()
        ctypes.memset(ctypes.byref(sums), 0x5a, ctypes.sizeof(sums))
        marked = bytes(sums)
        Wnew = np.full((OH.T, 16), 7, dtype=dtype)
        rc = s.lib.trmf_session_smooth(s.handle, first, rtol, max_iter, ctypes.byref(sums), Wnew.ctypes.data)
        assert rc == -1 and match in s.lib.trmf_last_error().decode(), s.lib.trmf_last_error().decode()
        assert bytes(sums) == marked and (Wnew == 7).all()
        assert np.array_equal(s.download().W, W0)

    model = _model(d, dtype)
    with Session(Y, model, lambdaI=0.0, lambdaAR=0.0, lambdaLag=0.5) as s:
        refused(s, 'largest lag', first=4)
        refused(s, 'first_row', first=OH.T + 1)
        refused(s, 'rtol', rtol=float('nan'))
        refused(s, 'rtol', rtol=float('inf'))
        refused(s, 'max_iter', max_iter=1 << 20)
        refused(s, 'row %d' % OH.EMPTY_ROW)                                   # no ridge at all and an empty row
        s.set_lambdas(0.5, 50.0, 0.5)
        assert s.smooth(OH.FIRST)['converged'] == 1                          # the session still works
        s.run(1).download()
        assert np.isfinite(model.W).all()
    lag0 = make_model(W0, d['H'].astype(dtype), d['theta'].astype(dtype), np.array([0, 1, 5], dtype=np.uint32))
    with Session(Y, lag0, lambdaLag=0.5) as s:
        refused(s, 'lag 0')
    rng = np.random.RandomState(5)
    theta = np.asfortranarray((0.2 * rng.randn(3, 96)).astype(dtype))
    big = make_model(rng.rand(OH.T, 96).astype(dtype), rng.rand(OH.N, 96).astype(dtype), theta, d['lag_set'])
    Wbig = big.W.copy()
    with Session(Y, big, lambdaLag=0.5) as s:
        with pytest.raises(RuntimeError, match='ranks 1..64'):
            s.smooth(OH.FIRST)
        assert np.array_equal(s.download().W, Wbig)


def test_series_statistics_go_stale_only_below_the_absorbed_rows():
    dtype, k = np.float32, 16
    d = SH.inputs(k)
    Y = _training(d, dtype, 'sparse')
    model = _model(d, dtype, OH.FIRST)
    with Session(Y[:OH.FIRST], model, **synth.HYPER) as s:
        s.init_series_stats(1.0)
        s.update(Y[OH.FIRST:])
        assert s.series_stats_info()['absorbed_rows'] == OH.FIRST
        s.smooth(OH.FIRST)                                                   # at the absorbed rows: nothing they hold has moved
        info = s.series_stats_info()
        assert info['valid'] and not info['stale']
        s.adapt_series()
        s.smooth(OH.T - 4)                                                   # everything is absorbed now: any window is below
        info = s.series_stats_info()
        assert info['stale'] and not info['valid']


def test_noise_tables_scores_mark_and_counter_are_untouched():
    dtype, k = np.float32, 16
    d = SH.inputs(k)
    truth = np.random.RandomState(2).rand(4, OH.N).astype(dtype)
    model = _model(d, dtype)
    with Session(_training(d, dtype, 'sparse'), model, **synth.HYPER) as s:
        s.run(2).mark()
        marked = [a.copy() for a in (s.download().W, model.H, model.lag_val)]
        s.fit_noise()
        s.forecast(4, truth=truth, return_forecast=False)
        s.forecast_dist(4, truth=truth)
        state = (s.noise(), s.forecast_series_sums(), s.interval_series_sums())
        st = s.stats(8)
        s.smooth(OH.FIRST)
        moved = s.download().W.copy()
        again = (s.noise(), s.forecast_series_sums(), s.interval_series_sums())
        for (a0, a1), (b0, b1) in zip(state, again):
            assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
        keep = [key for key in st[0] if not key.startswith('ms_')]
        assert [[x[key] for key in keep] for x in s.stats(8)] == [[x[key] for key in keep] for x in st]
        assert not np.array_equal(moved[OH.FIRST:], marked[0][OH.FIRST:]) and np.array_equal(moved[:OH.FIRST], marked[0][:OH.FIRST])
        assert np.array_equal(model.H, marked[1]) and np.array_equal(model.lag_val, marked[2])        # H and Theta stay fixed
        s.rewind().download()
        assert all(np.array_equal(a, b) for a, b in zip(marked, (model.W, model.H, model.lag_val)))


# ---- 4. Session.update and the rolling evaluation -------------------------------------------------------------------------------
@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_update_with_smooth_back_equals_append_assimilate_smooth(storage, missing):
    dtype, k = np.float32, 16
    d = SH.inputs(k)
    Y = _training(d, dtype, storage)
    a, b = _model(d, dtype, OH.FIRST), _model(d, dtype, OH.FIRST)
    with Session(Y[:OH.FIRST], a, missing=missing, **synth.HYPER) as s:
        s.run(2)
        s.append_rows(Y[OH.FIRST:])
        s.model = make_model(np.zeros((OH.T, k), dtype), a.H, a.lag_val, a.lag_set)
        want = s.assimilate(OH.FIRST)
        filtered = s.download().W.copy()
        want['smooth'] = s.smooth(OH.FIRST - 8)
        by_hand = s.download().W.copy()
    with Session(Y[:OH.FIRST], b, missing=missing, **synth.HYPER) as s:
        s.run(2)
        got = s.update(Y[OH.FIRST:], smooth_back=8)
        grown = s.download()
        with pytest.raises(ValueError, match='Huber'):
            s.update(Y[OH.FIRST:], robust_c=3.0, smooth_back=8)
        assert s.rows() == OH.T                                              # refused before anything was appended
    assert got == want and got['smooth']['rows'] == OH.TN + 8 and got['smooth']['converged'] == 1
    assert np.array_equal(grown.W, by_hand) and not np.array_equal(by_hand[OH.FIRST - 8:], filtered[OH.FIRST - 8:])
    assert got['smooth']['objective_after'] < got['smooth']['objective_before']


GOLD_Y = np.load(OH.__file__.replace('online_helpers.py', 'golden/py_harness.npz'))['rv_Y']
ROLL = dict(k=3, window_size=8, nr_windows=3, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=4, threads=2, seed=0)
ROLL_LAGS = [1, 2, 5]


@pytest.mark.parametrize('missing', [True, False], ids=['observed', 'full'])
def test_rolling_validate_with_smooth_back_equals_the_loop_by_hand(missing):
    dtype = np.float32
    Y = np.ascontiguousarray(GOLD_Y.astype(dtype))
    win, nw = ROLL['window_size'], ROLL['nr_windows']
    start = Y.shape[0] - win * nw
    got = trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, update='assimilate', smooth_back=8, **ROLL)
    model = trmf.Model.initialize(Y[:start], ROLL_LAGS, ROLL['k'], seed=0)
    dev = []
    with Session(smat.csr_matrix(Y[:start]) if missing else Y[:start], model, missing=missing, log_norms=False, timing=0,
                 lambdaI=ROLL['lambdaI'], lambdaAR=ROLL['lambdaAR'], lambdaLag=ROLL['lambdaLag']) as s:
        s.run(ROLL['max_iter']).download()
        for w in range(nw):
            cut = start + w * win
            if w:
                block = Y[cut - win:cut]
                s.append_rows(smat.csr_matrix(block) if missing else block)
                s.model = make_model(np.zeros((cut, ROLL['k']), dtype), s.model.H, s.model.lag_val, s.model.lag_set)
                s.assimilate(cut - win)
                assert s.smooth(cut - win - 8)['converged'] == 1
            dev.append(s.download().forecast(win, threshold=0)[0])
    dev = np.vstack(dev)
    assert np.array_equal(fields(got), fields(Metrics.generate(Y[start:], dev, missing=missing)))
    plain = trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, update='assimilate', **ROLL)
    assert not np.array_equal(fields(got), fields(plain))                    # the smoother moved the rows the forecasts start from
    on_dev = trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, update='assimilate', smooth_back=8, forecast_on_device=True, **ROLL)
    assert np.allclose(fields(on_dev), fields(got), rtol=1e-4), (on_dev, got)
    results, _ = trmf.grid_search(Y, ROLL_LAGS, {'lambdaI': [0.5]}, missing=missing, threshold=0, update='assimilate', smooth_back=8,
                                  **{key: v for key, v in ROLL.items() if key != 'lambdaI'})
    assert np.array_equal(fields(results[0]['metrics']), fields(got))
