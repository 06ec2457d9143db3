"""GPU (-m gpu): the robust fixed-interval smoother on the device -- trmf_session_smooth_robust (smooth_robust_part_kernel,
smooth_robust_fold_kernel, then the factor and smooth_* kernels once per sweep) behind Session.smooth_robust and
Session.update(smooth_robust=True) / rolling_validate(smooth_robust=True).  Small shapes: the whole file takes a few seconds.

The yardstick.  The truth is trmf.robust_smooth_rows in fp64 (every sweep solved directly) on the factors the session holds.
The IRLS twin of smooth_robust_helpers.py runs the device's computation in NumPy in the element type: the same weights, every
sweep by the smoother's PCG at rtol 1e-5 (fp32) / 1e-10 (fp64).  The device's rows may be no farther from the truth
(max |x - x*| / max |x*|) than 8 x the twin's are on the same input, and its weights no farther (max abs difference outside cells
within 1e-4 of their threshold) than 8 x the twin's."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as smat

import online_helpers as OH
import smooth_helpers as SH
import smooth_robust_helpers as SR
import trmf
from forecast_helpers import fields
from helpers import evidence, make_model
from trmf import Metrics, synth
from trmf.rf_util import PyMatrix
from trmf.session import Session, TrmfRobustSmoothSums

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ['float32', 'float64']
SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}             # the tolerance tests/test_gpu_online.py uses for the same sums
NAMES = list(SR.CASES)


def _model(d, dtype, rows=None, W=None):
    W = d['W'] if W is None else W
    m = make_model(np.ascontiguousarray(W[:rows].astype(dtype)), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    if d['k'] == 1:     # PyMatrix tags a (rows, 1) array column-major, like the reference's; the two orders are the same bytes
        m.pyW.type = m.pyH.type = PyMatrix.DENSE_ROWMAJOR
    return m


def _training(d, dtype, storage):
    Y = d['Y'].astype(dtype)
    return np.ascontiguousarray(Y.toarray()) if storage == 'dense' else Y


def _run(name, dtype, max_iter=SH.MAX_ITER, c=SR.C, sweeps=SR.SWEEPS):
    """(downloaded model, sums, Wnew, weights) of one session over the case's input set after smooth_robust(first)."""
    spec = SR.CASES[name]
    d, scale = SR.case(name)
    model = _model(d, dtype)
    with Session(_training(d, dtype, spec['storage']), model, lambdaI=spec['lamI'], lambdaAR=spec['lamAR'], lambdaLag=0.5, missing=spec['missing']) as s:
        sums, Wnew, om = s.smooth_robust(spec['first'], c, sweeps, scale, rtol=SH.RTOL[np.dtype(dtype)], max_iter=max_iter, return_latent=True,
                                         return_weights=True)
        s.download()
    return model, sums, Wnew, om


def _objectives(name, dtype, model, sums):
    spec = SR.CASES[name]
    d, scale = SR.case(name)
    tol = SH.OBJ_TOL[np.dtype(dtype)]
    kw = dict(missing=spec['missing'], storage=spec['storage'])
    before = SR.objective_of(d, d['W'].astype(dtype), spec['lamI'], spec['lamAR'], spec['first'], scale, **kw)
    after = SR.objective_of(d, model.W, spec['lamI'], spec['lamAR'], spec['first'], scale, **kw)
    print('   J_rob before %.10g (device %.10g), after %.10g (device %.10g)' % (before, sums['objective_before'], after, sums['objective_after']))
    assert abs(sums['objective_before'] - before) <= tol * before and abs(sums['objective_after'] - after) <= tol * after, (sums, before, after)
    assert sums['objective_after'] <= sums['objective_before']


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', NAMES)
def test_the_device_matches_the_fp64_statement_within_the_twins_distance(name, dtype, monkeypatch):
    spec = SR.CASES[name]
    if spec['slice']:
        monkeypatch.setenv('TRMF_SMOOTH_ROBUST_SLICE', str(spec['slice']))
    d, scale = SR.case(name)
    t, y = SR.truth(name), SR.yardstick(name, np.dtype(dtype))
    assert y['converged']
    first = spec['first']
    model, sums, Wnew, om = _run(name, dtype)
    got = SH.measure(model.W[first:], t['w64'][first:])
    keep = ~t['border']
    got_om = float(np.abs(om.astype(np.float64) - t['om64'])[keep].max())
    want_down, nborder = int((t['om64'] < 1).sum()), int(t['border'].sum())
    evidence('robust smoother %s %s: rows %.3e = %.2f x the twin\'s %.3e, weights %.3e = %.2f x the twin\'s %.3e (gate 8 x); steps %d, twin %d; '
             'down-weighted %d (statement %d, borderline %d) of %d' % (name, np.dtype(dtype).name, got, got / y['rows'], y['rows'], got_om,
                                                                      got_om / y['weights'], y['weights'], sums['iterations'], sum(y['steps']),
                                                                      sums['downweighted'], want_down, nborder, sums['entries']))
    assert np.array_equal(model.W[:first], d['W'][:first].astype(dtype))              # earlier rows keep their bits
    assert np.array_equal(Wnew, model.W[first:])
    assert om.shape == t['om64'].shape
    entries = (d['W'].shape[0] - first) * d['H'].shape[0] if not spec['missing'] else d['Y'][first:].nnz
    assert sums['rows'] == d['W'].shape[0] - first and sums['entries'] == entries and sums['sweeps'] == SR.SWEEPS
    assert got <= SH.GATE * y['rows'], (name, got, y['rows'])
    assert got_om <= SH.GATE * y['weights'], (name, got_om, y['weights'])
    assert sums['converged'] == 1 and sums['residual'] <= SH.RTOL[np.dtype(dtype)]
    assert sums['downweighted'] == int((om < 1).sum())
    assert abs(int(sums['downweighted']) - want_down) <= nborder
    assert np.array_equal((om < 1)[keep], (t['om64'] < 1)[keep])
    want_sum = float(t['om64'].sum())
    assert abs(sums['weight_sum'] - float(om.astype(np.float64).sum())) <= SUM_TOL[dtype] * want_sum
    assert abs(sums['weight_sum'] - want_sum) <= SUM_TOL[dtype] * want_sum + SH.GATE * y['weights'] * om.size
    _objectives(name, dtype, model, sums)
    for key, W in (('sq_err_before', d['W'].astype(dtype)), ('sq_err_after', model.W)):
        want, _ = OH.sq_err(d, W, first, spec['missing'])
        assert abs(sums[key] - want) <= SUM_TOL[dtype] * abs(want), (key, sums[key], want)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_an_infinite_c_minimises_the_plain_smoothers_objective(dtype):
    k, (lamI, lamAR), first = 40, OH.LAMBDAS[0], SH.FIRSTS[0]
    name = 'a-k%d-%g-%g-first%d' % (k, lamI, lamAR, first)
    d = SH.inputs(k)
    want, dist, _, converged = SH.yardstick(k, lamI, lamAR, first, np.dtype(dtype))
    model, sums, Wnew, om = _run(name, dtype, c=float('inf'), sweeps=1)
    got = SH.measure(model.W[first:], want[first:])
    evidence('robust smoother c=inf %s: distance to the fp64 direct solve of the plain smoother %.3e = %.2f x its twin\'s %.3e' % (
        np.dtype(dtype).name, got, got / dist, dist))
    assert converged and got <= SH.GATE * dist
    assert (om == 1).all() and sums['downweighted'] == 0 and sums['weight_sum'] == om.size
    after = SH.objective_of(d, model.W, lamI, lamAR, first)
    assert abs(sums['objective_after'] - after) <= SH.OBJ_TOL[np.dtype(dtype)] * after


# ---- 2. behaviour ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_sweeps_that_reach_max_iter_still_commit_and_lower_the_objective(dtype):
    name = 'a-k40-0.5-50-first40'
    d, _ = SR.case(name)
    model, sums, Wnew, om = _run(name, dtype, max_iter=3)
    assert sums['converged'] == 0 and sums['iterations'] == 3 * SR.SWEEPS and 0 < sums['residual'] < 1e3
    assert not np.array_equal(model.W[40:], d['W'][40:].astype(dtype)) and np.array_equal(Wnew, model.W[40:])
    _objectives(name, dtype, model, sums)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_identical_calls_from_the_same_state_give_the_same_bits(dtype):
    name = 'a-k40-0.5-50-first40'
    a, b = _run(name, dtype), _run(name, dtype)
    assert np.array_equal(a[0].W, b[0].W) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[1] == b[1]


def test_two_ranks_are_bit_identical_to_one(monkeypatch):
    name, dtype = 'a-k40-0.5-50-first40', np.float32
    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = _run(name, dtype)
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two = _run(name, dtype)
    assert np.array_equal(one[0].W, two[0].W) and np.array_equal(one[2], two[2]) and np.array_equal(one[3], two[3]) and one[1] == two[1]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_an_empty_window_is_a_no_op_with_zero_sums(dtype):
    d = SH.inputs(16)
    model = _model(d, dtype)
    with Session(_training(d, dtype, 'sparse'), model, lambdaLag=0.5) as s:
        sums, Wnew, om = s.smooth_robust(OH.T, scale=0.3, return_latent=True, return_weights=True)
        assert sums == dict(rows=0, entries=0, downweighted=0, sweeps=0, iterations=0, converged=0, residual=0.0, weight_sum=0.0, sq_err_before=0.0,
                            sq_err_after=0.0, objective_before=0.0, objective_after=0.0) and Wnew.shape == (0, 16) and om.size == 0
        assert np.array_equal(s.download().W, d['W'].astype(dtype))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_refused_calls_leave_w_the_outputs_and_the_session_as_they_were(dtype, monkeypatch):
    d = OH.inputs(16, 1.0)         # every cell stored but for the two designed rows: the empty row is the first singular block
    Y = _training(d, dtype, 'sparse')
    W0 = d['W'].astype(dtype)
    ones = np.full(OH.N, 0.3)

    def refused(s, match, first=OH.FIRST, c=1.5, sweeps=4, scale=ones, rtol=0.0, max_iter=0):
        sums = TrmfRobustSmoothSums()
        ctypes.memset(ctypes.byref(sums), 0x5a, ctypes.sizeof(sums))
        marked = bytes(sums)
        Wnew = np.full((OH.T, 16), 7, dtype=dtype)
        om = np.full(OH.T * OH.N, 7, dtype=dtype)
        before = s.describe()
        rc = s.lib.trmf_session_smooth_robust(s.handle, first, c, sweeps, scale.ctypes.data if scale is not None else None, rtol, max_iter,
                                              ctypes.byref(sums), Wnew.ctypes.data, om.ctypes.data)
        assert rc == -1 and match in s.lib.trmf_last_error().decode(), s.lib.trmf_last_error().decode()
        assert bytes(sums) == marked and (Wnew == 7).all() and (om == 7).all()
        assert np.array_equal(s.download().W, W0) and s.describe() == before

    model = _model(d, dtype)
    with Session(Y, model, lambdaI=0.0, lambdaAR=0.0, lambdaLag=0.5) as s:
        refused(s, 'largest lag', first=4)
        refused(s, 'first_row', first=OH.T + 1)
        refused(s, 'rtol', rtol=float('nan'))
        refused(s, 'max_iter', max_iter=1 << 20)
        refused(s, 'c must be positive', c=0.0)
        refused(s, 'c must be positive', c=float('nan'))
        refused(s, 'sweeps 0', sweeps=0)
        refused(s, 'sweeps 65', sweeps=65)
        refused(s, 'no scale given', scale=None)
        bad = ones.copy(); bad[3] = 0.0
        refused(s, 'scale of series 3', scale=bad)
        refused(s, 'row %d' % OH.EMPTY_ROW)                                   # no ridge at all and an empty row
        monkeypatch.setenv('TRMF_SMOOTH_MAX_ROWS', '23')
        refused(s, 'cap of 23 rows')
        monkeypatch.delenv('TRMF_SMOOTH_MAX_ROWS')
        s.set_lambdas(0.5, 50.0, 0.5)
        assert s.smooth_robust(OH.FIRST, 1.5, 4, 0.3)['converged'] == 1      # the session still works
        s.run(1).download()
        assert np.isfinite(model.W).all()
    lag0 = make_model(W0, d['H'].astype(dtype), d['theta'].astype(dtype), np.array([0, 1, 5], dtype=np.uint32))
    with Session(Y, lag0, lambdaLag=0.5) as s:
        refused(s, 'lag 0')
    full = _model(d, dtype)
    with Session(Y, full, lambdaLag=0.5, missing=False) as s:
        refused(s, 'sparse storage with missing == 0')
    rng = np.random.RandomState(5)
    theta = np.asfortranarray((0.2 * rng.randn(3, 96)).astype(dtype))
    big = make_model(rng.rand(OH.T, 96).astype(dtype), rng.rand(OH.N, 96).astype(dtype), theta, d['lag_set'])
    Wbig = big.W.copy()
    with Session(Y, big, lambdaLag=0.5) as s:
        with pytest.raises(RuntimeError, match='ranks 1..64'):
            s.smooth_robust(OH.FIRST, scale=0.3)
        assert np.array_equal(s.download().W, Wbig)


def test_series_statistics_go_stale_only_below_the_absorbed_rows():
    dtype, k = np.float32, 16
    d = SH.inputs(k)
    Y = _training(d, dtype, 'sparse')
    model = _model(d, dtype, OH.FIRST)
    with Session(Y[:OH.FIRST], model, **synth.HYPER) as s:
        s.init_series_stats(1.0)
        s.update(Y[OH.FIRST:])
        s.smooth_robust(OH.FIRST, scale=0.3)                                 # at the absorbed rows: nothing they hold has moved
        info = s.series_stats_info()
        assert info['valid'] and not info['stale']
        s.adapt_series()
        s.smooth_robust(OH.T - 4, scale=0.3)                                 # everything is absorbed now: any window is below
        info = s.series_stats_info()
        assert info['stale'] and not info['valid']


@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_run_after_the_robust_smoother_equals_a_fresh_session_from_the_downloaded_factors(storage, missing):
    """The weighted Grams live in scratch of the call's own: the X phase's Gram cache is not polluted."""
    dtype, k = np.float32, 16
    d = OH.inputs(k)
    Y = _training(d, dtype, storage)
    a = _model(d, dtype)
    with Session(Y, a, missing=missing, **synth.HYPER) as s:
        s.smooth_robust(OH.FIRST - 8, 2.0, 3, 0.3)
        s.download()
        b = make_model(a.W, a.H, a.lag_val, a.lag_set)
        s.run(1).download()
    with Session(Y, b, missing=missing, **synth.HYPER) as s:
        s.run(1).download()
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)


# ---- 3. Session.update ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_update_with_the_keyword_equals_append_assimilate_robust_smooth_robust(storage, missing):
    dtype, k = np.float32, 16
    d = SH.inputs(k)
    Y = _training(d, dtype, storage)
    a, b = _model(d, dtype, OH.FIRST), _model(d, dtype, OH.FIRST)
    with Session(Y[:OH.FIRST], a, missing=missing, **synth.HYPER) as s:
        s.run(2)
        s.append_rows(Y[OH.FIRST:])
        s.model = make_model(np.zeros((OH.T, k), dtype), a.H, a.lag_val, a.lag_set)
        want = s.assimilate_robust(OH.FIRST, 2.0, 3, 0.3)
        filtered = s.download().W.copy()
        want['smooth'] = s.smooth_robust(OH.FIRST - 8, 2.0, 3, 0.3)
        by_hand = s.download().W.copy()
    with Session(Y[:OH.FIRST], b, missing=missing, **synth.HYPER) as s:
        s.run(2)
        for kw in (dict(robust_c=2.0, scale=0.3), dict(smooth_back=8), {}):
            with pytest.raises(ValueError, match='smooth_robust=True needs both'):
                s.update(Y[OH.FIRST:], smooth_robust=True, **kw)
        with pytest.raises(ValueError, match='Huber'):                       # without the keyword: the refusal of before
            s.update(Y[OH.FIRST:], robust_c=2.0, scale=0.3, smooth_back=8)
        assert s.rows() == OH.FIRST                                          # refused before anything was appended
        got = s.update(Y[OH.FIRST:], robust_c=2.0, robust_sweeps=3, scale=0.3, smooth_back=8, smooth_robust=True)
        grown = s.download()
    assert got == want and got['smooth']['rows'] == OH.TN + 8 and got['smooth']['converged'] == 1 and got['smooth']['sweeps'] == 3
    assert np.array_equal(grown.W, by_hand) and not np.array_equal(by_hand[OH.FIRST - 8:], filtered[OH.FIRST - 8:])
    assert got['smooth']['objective_after'] < got['smooth']['objective_before']


GOLD_Y = np.load(OH.__file__.replace('online_helpers.py', 'golden/py_harness.npz'))['rv_Y']
ROLL = dict(k=3, window_size=8, nr_windows=3, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=4, threads=2, seed=0)
ROLL_LAGS = [1, 2, 5]


def test_rolling_validate_with_the_keyword_equals_the_loop_by_hand():
    dtype = np.float32
    Y = np.array(GOLD_Y, dtype=dtype, order='C')
    win, nw = ROLL['window_size'], ROLL['nr_windows']
    start = Y.shape[0] - win * nw
    spikes = np.random.RandomState(7).rand(win * (nw - 1), Y.shape[1]) < 0.05    # spiked cells in the windows that are absorbed online
    Y[start:start + win * (nw - 1)][spikes] += 20.0 * Y.std()
    kw = dict(missing=False, threshold=0, update='assimilate', robust_c=3, **ROLL)
    got = trmf.rolling_validate(Y, ROLL_LAGS, smooth_back=8, smooth_robust=True, **kw)
    model = trmf.Model.initialize(Y[:start], ROLL_LAGS, ROLL['k'], seed=0)
    dev = []
    with Session(Y[:start], model, missing=False, log_norms=False, timing=0, lambdaI=ROLL['lambdaI'], lambdaAR=ROLL['lambdaAR'],
                 lambdaLag=ROLL['lambdaLag']) as s:
        s.run(ROLL['max_iter']).download()
        s.fit_noise()
        for w in range(nw):
            cut = start + w * win
            if w:
                s.append_rows(Y[cut - win:cut])
                s.model = make_model(np.zeros((cut, ROLL['k']), dtype), s.model.H, s.model.lag_val, s.model.lag_set)
                s.assimilate_robust(cut - win, 3.0, 4)
                assert s.smooth_robust(cut - win - 8, 3.0, 4)['converged'] == 1
            dev.append(s.download().forecast(win, threshold=0)[0])
    assert np.array_equal(fields(got), fields(Metrics.generate(Y[start:], np.vstack(dev), missing=False)))
    filtered = trmf.rolling_validate(Y, ROLL_LAGS, **kw)
    assert not np.array_equal(fields(got), fields(filtered))                 # the smoother moved the rows the forecasts start from
    on_dev = trmf.rolling_validate(Y, ROLL_LAGS, smooth_back=8, smooth_robust=True, forecast_on_device=True, **kw)
    assert np.allclose(fields(on_dev), fields(got), rtol=1e-4), (on_dev, got)
    results, _ = trmf.grid_search(Y, ROLL_LAGS, {'lambdaI': [0.5]}, smooth_back=8, smooth_robust=True,
                                  **{key: v for key, v in kw.items() if key != 'lambdaI'})
    assert np.array_equal(fields(results[0]['metrics']), fields(got))
    with pytest.raises(ValueError, match='undo the Huber weights'):          # without the keyword: the refusal of before
        trmf.rolling_validate(Y, ROLL_LAGS, smooth_back=8, **kw)


# ---- 4. quality -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SR.QUALITY_SEEDS)
def test_spikes_bend_the_plain_smoother_and_not_the_robust_one(seed):
    """fp32 on the device, from the fp64 statements' filtered rows: the robust smoother's new rows are at most a quarter as far from
    the rows smoothed on the clean data as the plain smoother's, and no farther than the robust filter's by more than the parity
    gate (8 x the fp32 IRLS twin's distance from the fp64 statement, as a share of max |x*|, an RMS being at most a maximum)."""
    dtype, q, p = np.float32, SR.QUALITY, SR.quality_panel(seed)
    first, new = p['first'], p['new']
    Y = np.zeros((q['T'], q['n']), dtype=dtype)
    Y[first:] = p['dirty'].toarray()
    Y = smat.csr_matrix(Y)
    rows = {}
    for key, start in (('plain', p['plain_f']), ('robust', p['robust_f'])):
        model = make_model(np.ascontiguousarray(start.astype(dtype)), p['H'].astype(dtype), np.asfortranarray(p['lag_val'].astype(dtype)), p['lag_set'])
        with Session(Y, model, lambdaI=q['lamI'], lambdaAR=q['lamAR'], lambdaLag=0.5) as s:
            if key == 'plain':
                assert s.smooth(first)['converged'] == 1
            else:
                assert s.smooth_robust(first, q['c'], q['sweeps'], q['sigma'])['converged'] == 1
            rows[key] = s.download().W.copy()
    twin = SR.irls_twin(p['robust_f'], p['H'], p['lag_set'], p['lag_val'], p['dirty'].astype(dtype), first, q['lamI'], q['lamAR'], True, q['sigma'],
                        q['c'], q['sweeps'], dtype, SH.RTOL[np.dtype(dtype)], SH.MAX_ITER)[0]
    slack = SH.GATE * SH.measure(twin[first:], p['robust_s'][first:]) * float(np.abs(p['robust_s'][first:]).max())
    d_plain, d_robust = SR.rms_distance(rows['plain'], p['ref'], new), SR.rms_distance(rows['robust'], p['ref'], new)
    d_filter = SR.rms_distance(p['robust_f'].astype(dtype), p['ref'], new)
    evidence('spiked panel seed %d float32: plain smoother %.4f, robust filter %.4f, robust smoother %.4f = %.3f of the plain smoother\'s (slack %.2e)' % (
        seed, d_plain, d_filter, d_robust, d_robust / d_plain, slack))
    assert d_robust <= 0.25 * d_plain
    assert d_robust <= d_filter + slack
