"""GPU (-m gpu): outlier-robust online updates on the device -- trmf_session_assimilate_robust (assim_robust_part_kernel,
assim_robust_solve_kernel) behind Session.assimilate_robust / Session.update(robust_c=...) and
rolling_validate(update='assimilate', robust_c=...).  Small shapes: the whole file takes a few seconds.

The yardstick is test_gpu_online.py's: the device differs from trmf.robust_filter_rows by summation order only, so an fp32 session
may be no farther from the fp64 statement than OH.GATE x the fp32 statement is on the same input, an fp64 session no farther than
that scaled by eps64 / eps32; rows by relmax, weights by their largest absolute difference.  A cell whose residual lies within
1e-4 (relative) of its threshold may fall on either side: those cells alone are excluded from the count of down-weighted cells
(robust_helpers.margins; the input sets have none)."""
import numpy as np
import pytest
import scipy.sparse as smat

import online_helpers as OH
import robust_helpers as RH
import trmf
from forecast_helpers import fields
from helpers import evidence, make_model, relmax
from trmf import synth
from trmf.rf_util import PyMatrix
from trmf.session import Session

pytestmark = pytest.mark.gpu

SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}             # test_gpu_online.py's
DTYPES = [np.float32, np.float64]
IDS = ['float32', 'float64']


def _model(d, dtype, rows=None):
    m = make_model(d['W'][:rows].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    if d['k'] == 1:     # PyMatrix tags a (rows, 1) array column-major, like the reference's; the two orders are the same bytes
        m.pyW.type = m.pyH.type = PyMatrix.DENSE_ROWMAJOR
    return m


def _robust(d, dtype, lamI, lamAR, scale, c=RH.C, sweeps=RH.SWEEPS, missing=True, Y=None):
    """(downloaded model, sums, Wnew, weights) of one session over the input set after assimilate_robust(first)."""
    model = _model(d, dtype)
    Y = d['Y'].astype(dtype) if Y is None else Y
    with Session(Y, model, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5, missing=missing) as s:
        sums, Wnew, om = s.assimilate_robust(d['first'], c, sweeps, scale, return_latent=True, return_weights=True)
        s.download()
    return model, sums, Wnew, om


def _gate(what, d, y, dtype, model, sums, Wnew, om, entries):
    first = d['first']
    b_rows, b_om = OH.bound(dtype, y['dev_rows']), OH.bound(dtype, y['dev_weights'])
    got = relmax(model.W[first:], y['w64'][first:])
    got_om = float(np.abs(om.astype(np.float64) - y['om64']).max()) if om.size else 0.0
    want_down = int((y['om64'] < 1).sum())
    want_sum = float(y['om64'].sum())
    evidence('robust update %s %s: rows %.3e = %.2f x the bound %.3e, weights %.3e = %.2f x the bound %.3e; down-weighted %d (statement %d, '
             'borderline %d) of %d' % (what, np.dtype(dtype).name, got, got / b_rows, b_rows, got_om, got_om / max(b_om, 1e-300), b_om,
                                       sums['downweighted'], want_down, int(y['border'].sum()), sums['entries']))
    assert np.array_equal(model.W[:first], d['W'][:first].astype(dtype))             # earlier rows keep their bits
    assert np.array_equal(Wnew, model.W[first:])
    assert om.shape == y['om64'].shape
    assert got <= b_rows, (what, got, b_rows)
    assert got_om <= b_om, (what, got_om, b_om)
    assert sums['rows'] == model.W.shape[0] - first and sums['entries'] == entries
    assert sums['downweighted'] == int((om < 1).sum())
    assert abs(int(sums['downweighted']) - want_down) <= int(y['border'].sum())
    assert np.array_equal((om < 1)[~y['border']], (y['om64'] < 1)[~y['border']])
    assert abs(sums['weight_sum'] - float(om.astype(np.float64).sum())) <= SUM_TOL[dtype] * want_sum
    assert abs(sums['weight_sum'] - want_sum) <= SUM_TOL[dtype] * want_sum + b_om * om.size


# ---- 1. the matrix of cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lamI,lamAR', OH.LAMBDAS)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('k', OH.RANKS)
def test_the_robust_update_matches_the_numpy_statement(k, dtype, lamI, lamAR):
    d, scale, y = RH.case_a(k, lamI, lamAR)
    model, sums, Wnew, om = _robust(d, dtype, lamI, lamAR, scale)
    _gate('k=%d lambdaI=%g lambdaAR=%g' % (k, lamI, lamAR), d, y, dtype, model, sums, Wnew, om, d['Y'][OH.FIRST:].nnz)
    for key, W in (('sq_err_before', d['W'].astype(dtype)), ('sq_err_after', model.W)):
        want, _ = OH.sq_err(d, W, OH.FIRST)
        assert abs(sums[key] - want) <= SUM_TOL[dtype] * abs(want), (key, sums[key], want)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('k', RH.B_RANKS)
def test_rows_of_zero_to_three_slices(k, dtype, monkeypatch):
    monkeypatch.setenv('TRMF_ASSIM_ROBUST_SLICE', str(RH.SLICE))
    lamI, lamAR = OH.LAMBDAS[1]
    d, scale, y = RH.case_b(k, lamI, lamAR)
    model, sums, Wnew, om = _robust(d, dtype, lamI, lamAR, scale)
    _gate('slices k=%d' % k, d, y, dtype, model, sums, Wnew, om, sum(RH.B_LENGTHS))


# ---- 2. paths ---------------------------------------------------------------------------------------------------------------------
PATH_CASES = [(np.float32, 40), (np.float64, 7)]
PATH_IDS = ['float32-k40', 'float64-k7']


@pytest.mark.parametrize('dtype,k', PATH_CASES, ids=PATH_IDS)
def test_dense_storage_reports_a_matrix_of_weights(dtype, k):
    lamI, lamAR = OH.LAMBDAS[0]
    d = OH.inputs(k)
    Yd = np.ascontiguousarray(d['Y'].toarray())
    scale = RH.plain_scale(d, lamI, lamAR, missing=False)
    y = RH.yardstick_of(d, lamI, lamAR, scale, missing=False, Y=Yd)
    down, border = RH.exercised(y)
    assert 0.03 <= down <= 0.97 and border <= 0.01
    model, sums, Wnew, om = _robust(d, dtype, lamI, lamAR, scale, missing=False, Y=Yd.astype(dtype))
    assert om.shape == (OH.TN, OH.N)
    _gate('dense-full k=%d' % k, d, y, dtype, model, sums, Wnew, om, OH.TN * OH.N)
    want, _ = OH.sq_err(d, model.W, OH.FIRST, False)
    assert abs(sums['sq_err_after'] - want) <= SUM_TOL[dtype] * want


@pytest.mark.parametrize('dtype,k', PATH_CASES, ids=PATH_IDS)
def test_every_cell_stored(dtype, k):
    lamI, lamAR = OH.LAMBDAS[0]
    d = OH.inputs(k, 1.0)
    scale = RH.plain_scale(d, lamI, lamAR)
    y = RH.yardstick_of(d, lamI, lamAR, scale)
    down, border = RH.exercised(y)
    assert 0.03 <= down <= 0.97 and border <= 0.01
    model, sums, Wnew, om = _robust(d, dtype, lamI, lamAR, scale)
    _gate('every-cell-stored k=%d' % k, d, y, dtype, model, sums, Wnew, om, d['Y'][OH.FIRST:].nnz)


@pytest.mark.parametrize('dtype,k', PATH_CASES, ids=PATH_IDS)
def test_a_lag_that_reaches_behind_the_new_block(dtype, k):
    """The prior is formed from global memory: lags 1 and 2 read rows of this call, lag 30 only rows from before it."""
    lamI, lamAR = OH.LAMBDAS[1]
    d = OH.inputs(k, lags=(1, 2, 30))
    scale = RH.plain_scale(d, lamI, lamAR)
    y = RH.yardstick_of(d, lamI, lamAR, scale)
    down, border = RH.exercised(y)
    assert 0.03 <= down <= 0.97 and border <= 0.01
    model, sums, Wnew, om = _robust(d, dtype, lamI, lamAR, scale)
    _gate('long-lag k=%d' % k, d, y, dtype, model, sums, Wnew, om, d['Y'][OH.FIRST:].nnz)


@pytest.mark.parametrize('sweeps', [1, 8])
@pytest.mark.parametrize('dtype,k', PATH_CASES, ids=PATH_IDS)
def test_one_sweep_and_eight(dtype, k, sweeps):
    lamI, lamAR = OH.LAMBDAS[1]
    d = OH.inputs(k)
    scale = RH.plain_scale(d, lamI, lamAR)
    y = RH.yardstick_of(d, lamI, lamAR, scale, sweeps=sweeps)
    down, border = RH.exercised(y)
    assert 0.03 <= down <= 0.97 and border <= 0.01
    model, sums, Wnew, om = _robust(d, dtype, lamI, lamAR, scale, sweeps=sweeps)
    _gate('sweeps=%d k=%d' % (sweeps, k), d, y, dtype, model, sums, Wnew, om, d['Y'][OH.FIRST:].nnz)


@pytest.mark.parametrize('dtype,k', PATH_CASES, ids=PATH_IDS)
def test_a_scale_per_series_equals_the_resident_noise_of_its_squares(dtype, k):
    lamI, lamAR = OH.LAMBDAS[1]
    d = OH.inputs(k)
    base = RH.plain_scale(d, lamI, lamAR)
    scale = base * np.linspace(0.6, 1.6, OH.N)
    y = RH.yardstick_of(d, lamI, lamAR, scale)
    down, border = RH.exercised(y)
    assert 0.03 <= down <= 0.97 and border <= 0.01
    model, sums, Wnew, om = _robust(d, dtype, lamI, lamAR, scale)
    _gate('per-series scale k=%d' % k, d, y, dtype, model, sums, Wnew, om, d['Y'][OH.FIRST:].nnz)
    other = _model(d, dtype)
    with Session(d['Y'].astype(dtype), other, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5) as s:
        s.set_noise(scale * scale, np.ones(k))
        sums2, Wnew2, om2 = s.assimilate_robust(OH.FIRST, RH.C, RH.SWEEPS, return_latent=True, return_weights=True)
        sigma2, q = s.noise()
    assert np.array_equal(Wnew2, Wnew) and np.array_equal(om2, om) and sums2 == sums
    assert np.array_equal(sigma2, scale * scale) and np.array_equal(q, np.ones(k))       # the tables stay


@pytest.mark.parametrize('dtype,k', PATH_CASES, ids=PATH_IDS)
def test_an_infinite_c_is_the_plain_filter(dtype, k):
    lamI, lamAR = OH.LAMBDAS[1]
    d = OH.inputs(k)
    w64, dev32 = OH.yardstick(k, lamI, lamAR)
    model, sums, Wnew, om = _robust(d, dtype, lamI, lamAR, 1.0, c=np.inf)
    assert np.all(om == 1) and sums['downweighted'] == 0 and sums['weight_sum'] == float(om.size) == float(sums['entries'])
    got = relmax(model.W[OH.FIRST:], w64[OH.FIRST:])
    assert got <= OH.bound(dtype, dev32), (got, OH.bound(dtype, dev32))


# ---- 3. contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_repeated_calls_from_the_same_state_give_the_same_bits(dtype):
    k, (lamI, lamAR) = 40, OH.LAMBDAS[1]
    d, scale, _ = RH.case_a(k, lamI, lamAR)
    model = _model(d, dtype)
    with Session(d['Y'].astype(dtype), model, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5) as s:
        s.mark()
        a = s.assimilate_robust(OH.FIRST, RH.C, RH.SWEEPS, scale, return_latent=True, return_weights=True)
        Wa = s.download().W.copy()
        s.rewind()
        b = s.assimilate_robust(OH.FIRST, RH.C, RH.SWEEPS, scale, return_latent=True, return_weights=True)
        Wb = s.download().W.copy()
        empty = s.assimilate_robust(OH.T, RH.C, RH.SWEEPS, scale, return_latent=True, return_weights=True)      # first_row == rows
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(Wa, Wb)
    assert empty[0] == dict(rows=0, entries=0, downweighted=0, weight_sum=0.0, sq_err_before=0.0, sq_err_after=0.0)
    assert empty[1].shape == (0, k) and empty[2].shape == (0,)


def _state(s):
    m = s.download()
    rows, table = s.forecast_series_sums()
    return [m.W.copy(), m.H.copy(), m.lag_val.copy(), rows, table.copy()] + [a.copy() for a in s.noise()]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_refused_calls_leave_the_session_as_it_was(dtype):
    d = OH.inputs(16, 1.0)         # every cell stored but for the two designed rows: the empty row is the first singular system
    Y = d['Y'].astype(dtype)
    scale = np.full(OH.N, 0.3)
    truth = np.random.RandomState(2).rand(4, OH.N).astype(dtype)

    def refused(s, match, first=OH.FIRST, c=RH.C, sweeps=RH.SWEEPS, scale=scale):
        with pytest.raises(RuntimeError, match=match):
            s.assimilate_robust(first, c, sweeps, scale, return_latent=True, return_weights=True)

    model = _model(d, dtype)
    with Session(Y, model, lambdaI=0.0, lambdaAR=0.0, lambdaLag=0.5) as s:
        refused(s, 'no noise fitted or set', scale=None)
        s.set_noise(np.full(OH.N, 0.09), np.ones(16))
        s.forecast(4, truth=truth, return_forecast=False)
        s.mark()
        before = _state(s)
        refused(s, 'largest lag', first=4)
        refused(s, 'first_row', first=OH.T + 1)
        for c in (0.0, -1.0, np.nan):
            refused(s, 'c must be positive', c=c)
        for sweeps in (0, 65):
            refused(s, 'sweeps', sweeps=sweeps)
        for v in (0.0, -0.3, np.nan, np.inf):
            bad = scale.copy()
            bad[13] = v
            refused(s, 'series 13', scale=bad)
        refused(s, 'row %d' % OH.EMPTY_ROW)                                    # no ridge at all and an empty row: a bad pivot
        assert _same(before, _state(s))
        s.set_noise(np.zeros(OH.N), np.ones(16))                              # a resident sigma2 of zero is no scale
        refused(s, 'series 0', scale=None)
        s.set_noise(np.full(OH.N, 0.09), np.ones(16))
        s.set_lambdas(0.5, 50.0, 0.5)
        ok = s.assimilate_robust(OH.FIRST, RH.C, RH.SWEEPS)                    # the session still works, with the resident scale
        assert ok['rows'] == OH.TN and 0 < ok['downweighted'] < ok['entries']
        after = _state(s)
        assert not np.array_equal(after[0][OH.FIRST:], before[0][OH.FIRST:]) and _same(before[1:], after[1:])
        s.rewind()
        assert _same(before, _state(s))                                        # the mark was not moved
        s.run(1).download()
        assert np.isfinite(model.W).all()
    # a lag set with lag 0
    lag0 = make_model(d['W'].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), np.array([0, 1, 5], dtype=np.uint32))
    with Session(Y, lag0, lambdaLag=0.5) as s:
        refused(s, 'lag 0')
        assert np.array_equal(s.download().W, d['W'].astype(dtype))
    # rank above 64
    rng = np.random.RandomState(5)
    theta = np.asfortranarray((0.2 * rng.randn(3, 96)).astype(dtype))
    big = make_model(rng.rand(OH.T, 96).astype(dtype), rng.rand(OH.N, 96).astype(dtype), theta, d['lag_set'])
    W0 = big.W.copy()
    with Session(Y, big, lambdaLag=0.5) as s:
        refused(s, 'ranks 1..64')
        assert np.array_equal(s.download().W, W0)
    # sparse storage without missing
    full = _model(d, dtype)
    with Session(Y, full, lambdaI=0.5, lambdaAR=0.5, lambdaLag=0.5, missing=False) as s:
        refused(s, 'without a slot')
        assert np.array_equal(s.download().W, d['W'].astype(dtype))
        assert s.assimilate(OH.FIRST)['rows'] == OH.TN                        # the plain filter covers it


def test_two_ranks_are_bit_identical_to_one(monkeypatch):
    dtype, k = np.float32, 40
    lamI, lamAR = OH.LAMBDAS[1]
    d, scale, _ = RH.case_a(k, lamI, lamAR)
    Y = d['Y'].astype(dtype)

    def run():
        model = _model(d, dtype, OH.FIRST)
        with Session(Y[:OH.FIRST], model, **synth.HYPER) as s:
            s.run(2)
            sums = s.update(Y[OH.FIRST:], robust_c=RH.C, scale=scale)
            again = s.assimilate_robust(OH.FIRST + 3, RH.C, RH.SWEEPS, scale, return_latent=True, return_weights=True)
            grown = s.download()
            return grown.W.copy(), grown.H.copy(), sums, again, s.describe()

    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = run()
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two = run()
    assert '1 rank' in one[4] and '2 ranks' in two[4]
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and one[2] == two[2]
    assert one[3][0] == two[3][0] and np.array_equal(one[3][1], two[3][1]) and np.array_equal(one[3][2], two[3][2])


# ---- 4. Session.update and the rolling evaluation ---------------------------------------------------------------------------------
@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_update_with_robust_c_equals_append_rows_then_assimilate_robust(storage, missing):
    dtype, k = np.float32, 16
    d = OH.inputs(k)
    Y = d['Y'].astype(dtype)
    Y = np.ascontiguousarray(Y.toarray()) if storage == 'dense' else Y
    scale = 0.3
    a, b, c = (_model(d, dtype, OH.FIRST) for _ in range(3))
    with Session(Y[:OH.FIRST], a, missing=missing, **synth.HYPER) as s:
        s.run(2)
        s.append_rows(Y[OH.FIRST:])
        s.model = make_model(np.zeros((OH.T, k), dtype), a.H, a.lag_val, a.lag_set)
        s.mark()
        want = s.assimilate_robust(OH.FIRST, 2.0, 3, scale)
        Wr = s.download().W.copy()
        s.rewind()
        plain = s.assimilate(OH.FIRST)
        Wp = s.download().W.copy()
    with Session(Y[:OH.FIRST], b, missing=missing, **synth.HYPER) as s:
        s.run(2)
        got = s.update(Y[OH.FIRST:], robust_c=2.0, robust_sweeps=3, scale=scale)
        assert s.rows() == OH.T and s.model.m == OH.T
        Wb = s.download().W.copy()
    with Session(Y[:OH.FIRST], c, missing=missing, **synth.HYPER) as s:          # without robust_c: today's bits
        s.run(2)
        got_plain = s.update(Y[OH.FIRST:])
        Wc = s.download().W.copy()
    assert got == want and np.array_equal(Wb, Wr) and 0 < got['downweighted'] < got['entries']
    assert got_plain == plain and np.array_equal(Wc, Wp) and not np.array_equal(Wr[OH.FIRST:], Wp[OH.FIRST:])


@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_run_after_a_robust_update_equals_a_fresh_session_from_the_downloaded_factors(storage, missing):
    dtype, k = np.float32, 16
    d = OH.inputs(k)
    Y = d['Y'].astype(dtype)
    Y = np.ascontiguousarray(Y.toarray()) if storage == 'dense' else Y
    a = _model(d, dtype)
    with Session(Y, a, missing=missing, **synth.HYPER) as s:
        s.assimilate_robust(OH.FIRST, 2.0, 3, 0.3)
        s.download()
        b = make_model(a.W, a.H, a.lag_val, a.lag_set)
        s.run(2).download()
    with Session(Y, b, missing=missing, **synth.HYPER) as s:
        s.run(2).download()
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)


GOLD_Y = np.load(OH.__file__.replace('online_helpers.py', 'golden/py_harness.npz'))['rv_Y']
ROLL = dict(k=3, window_size=8, nr_windows=3, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=4, threads=2, seed=0)
ROLL_LAGS = [1, 2, 5]


def test_rolling_validate_with_robust_updates_equals_the_host_loop():
    dtype = np.float32
    Y = np.array(GOLD_Y, dtype=dtype, order='C')
    win, nw = ROLL['window_size'], ROLL['nr_windows']
    start = Y.shape[0] - win * nw
    rng = np.random.RandomState(7)
    spikes = rng.rand(win * (nw - 1), Y.shape[1]) < 0.05                          # spiked cells in the windows that are absorbed online
    Y[start:start + win * (nw - 1)][spikes] += 20.0 * Y.std()
    got = trmf.rolling_validate(Y, ROLL_LAGS, missing=False, threshold=0, update='assimilate', robust_c=3, **ROLL)
    plain = trmf.rolling_validate(Y, ROLL_LAGS, missing=False, threshold=0, update='assimilate', **ROLL)
    # the host loop: window 0 trained on the device, its noise fitted on the host, every later window through Model.assimilate
    model = trmf.Model.initialize(Y[:start], ROLL_LAGS, ROLL['k'], seed=0)
    with Session(Y[:start], model, missing=False, log_norms=False, timing=0, lambdaI=ROLL['lambdaI'], lambdaAR=ROLL['lambdaAR'],
                 lambdaLag=ROLL['lambdaLag']) as s:
        s.run(ROLL['max_iter']).download()
    m = make_model(model.W, model.H, model.lag_val, model.lag_set).fit_noise(Y[:start], missing=False)
    host = [m.forecast(win, threshold=0)[0]]
    for w in range(1, nw):
        cut = start + w * win
        m = m.assimilate(Y[cut - win:cut], ROLL['lambdaI'], ROLL['lambdaAR'], missing=False, robust_c=3, robust_sweeps=4)
        assert (m.robust_weights < 1).any()
        host.append(m.forecast(win, threshold=0)[0])
    want = trmf.Metrics.generate(Y[start:], np.vstack(host), missing=False)
    assert np.allclose(fields(got), fields(want), rtol=1e-4), (got, want)
    assert not np.allclose(fields(got), fields(plain), rtol=1e-6), (got, plain)
    on_dev = trmf.rolling_validate(Y, ROLL_LAGS, missing=False, threshold=0, update='assimilate', robust_c=3, forecast_on_device=True, **ROLL)
    assert np.allclose(fields(on_dev), fields(got), rtol=1e-4), (on_dev, got)
