"""GPU (-m gpu): forecast uncertainty on the device -- trmf_session_fit_noise (noise_resid_kernel, noise_innov_kernel),
trmf_session_forecast_dist (forecast_psi_kernel, forecast_dist_kernel) and the interval table behind Session.fit_noise /
forecast_dist / interval_scores and rolling_validate(interval_level=...).  Small shapes: the whole file takes a few seconds.

The gates.  The device and trmf/uncertainty.py do fp64 arithmetic on identical stored values and differ by summation order
only, so every bound below is computed from the operands (u = 2^-52):
  sigma2   per residual r = y - w.h an error d <= (k + 2) u (|y| + sum_d |w_d h_d|), through the square 2 |r| d + d^2, plus
           count u relative for the sum of the non-negative squares
  q        the one-step latent forecasts are the same bits on both sides; (count + 4) u relative for difference, square and sum
  Ysd      (k + 4) u relative before the final rounding, i.e. at most 1 ulp of the element type after it
  sums     cells / covered exact; sd_sum, abs_truth, z2_sum (steps + 2) u relative; nll_sum, crps_sum (steps + 8) u sum|terms|
           (the 8 allows the device math library's fp64 erf / log / exp a couple of ulp each)"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as smat

import online_helpers as OH
import trmf
from forecast_helpers import fields
from helpers import evidence, make_model
from trmf import IntervalMetrics, Metrics, synth
from trmf.model import NormalizedTransform
from trmf.rf_util import PyMatrix
from trmf.session import Session
from trmf.uncertainty import fit_noise, forecast_std, interval_terms, z_of_level

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
DTYPES = [np.float32, np.float64]
EMPTY_SERIES = 13
RANKS = (1, 7, 16, 40, 64, 96)                              # every NT with and without pad columns, and the sliced form
MODES = [('observed-sparse', True, 'sparse'), ('full-sparse', False, 'sparse'), ('full-dense', False, 'dense')]


def _inputs(k):
    """online_helpers.inputs with one series emptied (copies: the helper's arrays are shared)."""
    d = dict(OH.inputs(k))
    Y = d['Y'].tolil(copy=True)
    Y[:, EMPTY_SERIES] = 0
    d['Y'] = smat.csr_matrix(Y.tocsr())
    d['Y'].eliminate_zeros()
    assert d['Y'].getnnz(axis=0)[EMPTY_SERIES] == 0 and d['Y'].getnnz(axis=0).max() >= 29
    return d


def _model(d, dtype, lag_set=None, theta=None):
    m = make_model(d['W'].astype(dtype), d['H'].astype(dtype), (d['theta'] if theta is None else theta).astype(dtype),
                   d['lag_set'] if lag_set is None else lag_set)
    if d['W'].shape[1] == 1:     # PyMatrix tags a (rows, 1) array column-major, like the reference's; the two orders are the same bytes
        m.pyW.type = m.pyH.type = PyMatrix.DENSE_ROWMAJOR
    return m


def _training(d, dtype, storage):
    Y = d['Y'].astype(dtype)
    return np.ascontiguousarray(Y.toarray()) if storage == 'dense' else Y


# ---- 1. fit_noise against the NumPy statement ------------------------------------------------------------------------------------
def _sigma2_bounds(d, dtype, missing):
    """Per series: the bound on |device sq_j / cnt_j - NumPy's|, relative to NumPy's sigma2_j; and the pooled value's."""
    W, H = d['W'].astype(dtype).astype(np.float64), d['H'].astype(dtype).astype(np.float64)
    k = W.shape[1]
    Yd = np.asarray(d['Y'].astype(dtype).toarray(), dtype=np.float64)
    mask = np.asarray(d['Y'].toarray() != 0) if missing else np.ones(Yd.shape, dtype=bool)
    absdot = np.abs(W).dot(np.abs(H).T)
    r = Yd - W.dot(H.T)
    delta = (k + 2) * U * (np.abs(Yd) + absdot)
    per_cell = np.where(mask, 2 * np.abs(r) * delta + delta * delta, 0.0)
    sq = np.where(mask, r * r, 0.0).sum(axis=0)
    cnt = mask.sum(axis=0)
    bound = per_cell.sum(axis=0) + cnt * U * sq
    return bound, sq, cnt, per_cell.sum() + cnt.sum() * U * sq.sum()


def _check_fit(d, dtype, name, missing, storage, what):
    model = _model(d, dtype)
    with Session(_training(d, dtype, storage), model, lambdaLag=0.5, missing=missing) as s:
        stats = s.fit_noise()
        sigma2, q = s.noise()
        again = s.fit_noise()
        sigma2b, qb = s.noise()
    assert stats == again and np.array_equal(sigma2, sigma2b) and np.array_equal(q, qb)           # the same bits on every call
    ref_s2, ref_q, info = fit_noise(model.W, model.H, model.lag_set, model.lag_val, _training(d, dtype, 'sparse'), missing)
    bound, sq, cnt, pooled_bound = _sigma2_bounds(d, dtype, missing)
    has = cnt > 0
    ratio = np.abs(sigma2[has] * cnt[has] - ref_s2[has] * cnt[has]) / bound[has]
    pooled_ratio = abs(stats['pooled_sigma2'] - info['pooled']) * cnt.sum() / pooled_bound
    m = int(model.lag_set.max())
    q_bound = (OH.T - m + 4) * U * ref_q
    q_ratio = np.abs(q - ref_q) / q_bound
    evidence('fit_noise %s %s %s: sigma2 measured / bound max %.3f, pooled %.3f, q max %.3f' % (
        what, np.dtype(dtype).name, name, ratio.max(), pooled_ratio, q_ratio.max()))
    assert ratio.max() <= 1.0 and pooled_ratio <= 1.0 and q_ratio.max() <= 1.0
    assert stats['series_pooled'] == int((~has).sum()) == (1 if missing else 0)
    if missing:
        assert sigma2[EMPTY_SERIES] == stats['pooled_sigma2']                                     # the emptied series takes the pooled value
    assert stats['sigma2_min'] == sigma2.min() and stats['sigma2_max'] == sigma2.max()
    assert stats['q_min'] == q.min() and stats['q_max'] == q.max()


@pytest.mark.parametrize('name,missing,storage', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
@pytest.mark.parametrize('k', RANKS)
def test_fit_noise_matches_the_numpy_statement(k, dtype, name, missing, storage):
    _check_fit(_inputs(k), dtype, name, missing, storage, 'k=%d' % k)


@pytest.mark.parametrize('name,missing,storage', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('dtype,k', [(np.float32, 40), (np.float64, 7), (np.float32, 96)], ids=['float32-k40', 'float64-k7', 'float32-k96'])
def test_fit_noise_with_several_items_per_series(dtype, k, name, missing, storage, monkeypatch):
    monkeypatch.setenv('TRMF_NOISE_CHUNK', '8')             # a 29-entry series takes four items, a 96-timestamp one twelve
    _check_fit(_inputs(k), dtype, name, missing, storage, 'chunk=8 k=%d' % k)


def test_fit_noise_refuses_a_history_no_longer_than_the_largest_lag():
    d = _inputs(7)
    model = make_model(d['W'][:6], d['H'], d['theta'], np.array([1, 2, 5], dtype=np.uint32))
    with Session(d['Y'][:6], model, lambdaLag=0.5) as s:
        s.fit_noise()                                       # 6 rows reach past lag 5
    # (a session cannot be created with rows <= the largest lag: the guard is the library's own, exercised through the NumPy twin)
    with pytest.raises(ValueError, match='largest lag'):
        fit_noise(d['W'][:5], d['H'], d['lag_set'], d['theta'], d['Y'][:5])


# ---- 2. forecast_dist ------------------------------------------------------------------------------------------------------------
FC_T = 200
LAG_SETS = {'reach5': (1, 2, 5), 'reach191': (1, 2, 191)}


def _fc_inputs(k, n, lags, seed=0):
    rng = np.random.RandomState(4000 + 10 * k + n + len(lags) + seed)
    W = rng.rand(FC_T, k).astype(np.float32)
    H = rng.rand(n, k).astype(np.float32)
    theta = rng.randn(len(lags), k)
    theta = np.asfortranarray((theta / (np.abs(theta).sum(axis=0) + 0.1)).astype(np.float32))
    Y = (rng.rand(FC_T, n) * np.linspace(0.5, 3.0, n)).astype(np.float32)
    return dict(W=W, H=H, theta=theta, lag_set=np.array(lags, dtype=np.uint32), Y=Y, k=k,
                sigma2=np.linspace(0.05, 0.6, n), q=np.linspace(0.02, 0.3, k))


def _check_sd(Ysd, ref64, k, dtype, what):
    if np.dtype(dtype) == np.float64:
        rel = np.abs(Ysd - ref64) / ref64
        assert rel.max() <= (k + 4) * U, (what, rel.max())
        return rel.max() / ((k + 4) * U)
    ref = ref64.astype(np.float32)
    ulps = np.abs(Ysd.astype(np.float64) - ref.astype(np.float64)) / np.spacing(ref).astype(np.float64)
    assert ulps.max() <= 1.0, (what, ulps.max())
    return ulps.max()


@pytest.mark.parametrize('n', [50, 300])
@pytest.mark.parametrize('lags', sorted(LAG_SETS))
@pytest.mark.parametrize('transform', [False, True], ids=['raw', 'transform'])
@pytest.mark.parametrize('dtype,k', [(np.float32, 40), (np.float64, 7), (np.float32, 96)], ids=['float32-k40', 'float64-k7', 'float32-k96'])
def test_forecast_dist_mean_is_forecasts_and_sd_matches_numpy(dtype, k, transform, lags, n):
    d = _fc_inputs(k, n, LAG_SETS[lags])
    model = _model(d, dtype)
    Y = d['Y'].astype(dtype)
    tr = NormalizedTransform(Y) if transform else None
    worst = 0.0
    with Session(Y, model, lambdaLag=0.5, missing=False) as s:
        if tr is not None:
            s.set_transform(tr)
        s.set_noise(d['sigma2'], d['q'])
        for steps in (1, 24, 200):
            ref = forecast_std(model.H, model.lag_set, model.lag_val, d['sigma2'], d['q'], steps, transform=tr, dtype=np.float64)
            for threshold in (None, 0.7):
                want_Y, want_W = s.forecast(steps, threshold=threshold, return_latent=True)
                Ynew, Ysd, Wnew = s.forecast_dist(steps, threshold=threshold, return_latent=True)
                assert np.array_equal(Ynew, want_Y) and np.array_equal(Wnew, want_W), (steps, threshold)
                assert Ysd.dtype == dtype and Ysd.shape == (steps, n)
                worst = max(worst, _check_sd(Ysd, ref, k, dtype, (steps, threshold)))
    evidence('forecast_dist %s k=%d n=%d %s %s: Ysd worst %.3f of its gate (fp64: (k + 4) u relative; fp32: 1 ulp)' % (
        np.dtype(dtype).name, k, n, lags, 'transform' if transform else 'raw', worst))


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_global_memory_forms_give_the_same_bits(dtype, monkeypatch):
    d = _fc_inputs(16, 50, LAG_SETS['reach191'])

    def run():
        with Session(d['Y'].astype(dtype), _model(d, dtype), lambdaLag=0.5, missing=False) as s:
            s.set_noise(d['sigma2'], d['q'])
            return s.forecast_dist(200, return_latent=True)

    lds = run()
    monkeypatch.setenv('TRMF_FORECAST_GLOBAL', '1')
    glob = run()
    assert all(np.array_equal(a, b) for a, b in zip(lds, glob))


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_explosive_lag_weights_are_refused_and_nothing_is_written(dtype):
    d = _fc_inputs(7, 50, LAG_SETS['reach5'])
    theta = d['theta'].copy()
    theta[:, 0] *= 3.0 / abs(theta[0, 0])                   # |theta_1| = 3 in dimension 0
    model = _model(d, dtype, theta=theta)
    steps, n, k = 2000, 50, 7
    truth = np.ones((steps, n), dtype=dtype)
    with Session(d['Y'].astype(dtype), model, lambdaLag=0.5, missing=False) as s:
        s.set_noise(d['sigma2'], d['q'])
        s.forecast_dist(4, truth=truth[:4])
        rows, table = s.interval_series_sums()
        with pytest.raises(RuntimeError, match='explosive'):
            s.forecast_dist(steps)
        Ynew, Ysd, Wnew = (np.full(shape, -7, dtype=dtype) for shape in ((steps, n), (steps, n), (steps, k)))
        pyT = PyMatrix(truth, dtype=np.dtype(dtype))
        rc = s.lib.trmf_session_forecast_dist(s.handle, steps, 0, 0.0, 1.0, ctypes.byref(pyT), Ynew.ctypes.data, Ysd.ctypes.data, Wnew.ctypes.data)
        assert rc == -1 and b'explosive' in s.lib.trmf_last_error()
        assert (Ynew == -7).all() and (Ysd == -7).all() and (Wnew == -7).all()
        rows2, table2 = s.interval_series_sums()
        assert rows2 == rows == 4 and np.array_equal(table2, table)
        assert np.isfinite(s.forecast_dist(4)[1]).all()      # the session still works


# ---- 3. interval sums --------------------------------------------------------------------------------------------------------------
def _sums_gate(table, truth, Ynew, Ysd, level, steps_total, what):
    """The device's table against a NumPy loop in step order over the device's own returned values."""
    zq = z_of_level(level)
    want = np.zeros_like(table)
    tol = np.zeros_like(table)
    lo = 0
    for t, y, sd in zip(truth, Ynew, Ysd):
        e = t.astype(np.float64) - y.astype(np.float64)
        margin = np.abs(np.abs(e) - zq * sd.astype(np.float64)) / sd.astype(np.float64)
        assert margin.min() >= 1e-9, (what, margin.min())   # no cell sits on the interval's edge: covered is decided alike
        want += IntervalMetrics.series_sums(t, y, sd, level)
        terms = interval_terms(t, y, sd, zq)
        for c, term in enumerate(terms):
            tol[:, c + 1] += np.abs(term).sum(axis=0)
        lo += t.shape[0]
    assert lo == steps_total
    assert np.array_equal(table[:, 0], want[:, 0]) and np.array_equal(table[:, 1], want[:, 1]), what
    worst = {}
    for c, name, slack in ((2, 'sd_sum', 2), (3, 'abs_truth', 2), (4, 'z2_sum', 2), (5, 'nll_sum', 8), (6, 'crps_sum', 8)):
        bound = (steps_total + slack) * U * tol[:, c]
        ratio = np.abs(table[:, c] - want[:, c]) / bound
        worst[name] = ratio.max()
        assert ratio.max() <= 1.0, (what, name, ratio.max())
    return worst


@pytest.mark.parametrize('transform', [False, True], ids=['raw', 'transform'])
@pytest.mark.parametrize('dtype,k', [(np.float32, 40), (np.float64, 7), (np.float64, 96)], ids=['float32-k40', 'float64-k7', 'float64-k96'])
def test_interval_sums_accumulate_and_reset(dtype, k, transform):
    n, level = 300, 0.9
    d = _fc_inputs(k, n, LAG_SETS['reach5'])
    model = _model(d, dtype)
    Y = d['Y'].astype(dtype)
    rng = np.random.RandomState(77)
    truths = [(rng.rand(steps, n) * np.linspace(0.5, 3.0, n) + 0.01).astype(dtype) for steps in (24, 7)]
    with Session(Y, model, lambdaLag=0.5, missing=False) as s:
        if transform:
            s.set_transform(NormalizedTransform(Y))
        s.set_noise(d['sigma2'], d['q'])
        assert s.interval_series_sums()[0] == 0 and not s.interval_series_sums()[1].any()
        outs = [s.forecast_dist(t.shape[0], level=level, truth=t) for t in truths]
        rows, table = s.interval_series_sums()
        assert rows == 31
        worst = _sums_gate(table, truths, [o[0] for o in outs], [o[1] for o in outs], level, 31, (k, transform))
        evidence('interval sums %s k=%d %s: measured / bound %s' % (np.dtype(dtype).name, k, 'transform' if transform else 'raw',
                                                                    ' '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
        got = s.interval_scores(level)
        want = IntervalMetrics.from_series_sums(table, level)
        assert got == want and 0 <= got.coverage <= 1
        s.forecast_dist(5, level=level)                     # no truth: nothing is scored
        assert s.interval_series_sums()[0] == 31
        s.reset_interval_scores()
        assert s.interval_series_sums()[0] == 0 and not s.interval_series_sums()[1].any()
        one = s.forecast_dist(24, level=level, truth=truths[0])
        rows, table = s.interval_series_sums()
        assert rows == 24 and np.array_equal(one[0], outs[0][0]) and np.array_equal(one[1], outs[0][1])
        _sums_gate(table, truths[:1], [one[0]], [one[1]], level, 24, (k, transform, 'after reset'))
        Ynew, lo, hi = s.forecast_interval(24, level=level, threshold=0.4)
        half = s.forecast_dist(24, level=level, threshold=0.4)[1] * dtype(z_of_level(level))
        assert np.array_equal(hi, Ynew + half) and np.array_equal(lo, np.maximum(Ynew - half, dtype(0.4)))


# ---- 4. contract ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_repeated_calls_and_the_noise_round_trip(dtype):
    d = _inputs(40)
    truth = np.random.RandomState(3).rand(12, OH.N).astype(dtype)
    with Session(_training(d, dtype, 'sparse'), _model(d, dtype), lambdaLag=0.5) as s:
        s.fit_noise()
        a = s.forecast_dist(12, truth=truth, return_latent=True)
        ta = s.interval_series_sums()[1]
        s.reset_interval_scores().fit_noise()
        b = s.forecast_dist(12, truth=truth, return_latent=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(ta, s.interval_series_sums()[1])
        sigma2, q = np.linspace(0.0, 2.0, OH.N), np.linspace(3.0, 0.0, 40)       # zeros are legal variances
        s.set_noise(sigma2, q)
        got = s.noise()
        assert np.array_equal(got[0], sigma2) and np.array_equal(got[1], q)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_refused_calls(dtype):
    d = _inputs(16)
    truth = np.ones((4, OH.N), dtype=dtype)
    with Session(_training(d, dtype, 'sparse'), _model(d, dtype), lambdaLag=0.5) as s:
        with pytest.raises(RuntimeError, match='no noise'):
            s.forecast_dist(4)
        with pytest.raises(RuntimeError, match='fitted or set'):
            s.noise()
        good = (np.ones(OH.N), np.ones(16))
        for bad in (-1.0, np.nan, np.inf):
            for which in (0, 1):
                tables = [good[0].copy(), good[1].copy()]
                tables[which][3] = bad
                with pytest.raises(RuntimeError, match='negative or not finite'):
                    s.set_noise(*tables)
        with pytest.raises(RuntimeError, match='no noise'):  # a refused set_noise sets nothing
            s.forecast_dist(4)
        with pytest.raises(ValueError, match='sigma2 must have'):
            s.set_noise(good[0][:-1], good[1])
        s.set_noise(*good)
        with pytest.raises(RuntimeError, match='dense'):
            s.forecast_dist(4, truth=smat.csr_matrix(truth))
        with pytest.raises(RuntimeError, match='4 x'):
            s.forecast_dist(4, truth=truth[:3])
        with pytest.raises(RuntimeError, match='steps'):
            s.forecast_dist(0)
        with pytest.raises(ValueError, match='level'):
            s.forecast_dist(4, level=1.0)
        for zq in (0.0, -1.0, float('nan')):
            Ynew = np.full((4, OH.N), -7, dtype=dtype)
            rc = s.lib.trmf_session_forecast_dist(s.handle, 4, 0, 0.0, zq, None, Ynew.ctypes.data, None, None)
            assert rc == -1 and b'zq' in s.lib.trmf_last_error() and (Ynew == -7).all()
        assert s.interval_series_sums()[0] == 0
        assert np.array_equal(s.noise()[0], good[0])
        assert s.forecast_dist(4, truth=truth)[1].shape == (4, OH.N)


def test_the_session_is_untouched_by_successful_and_refused_calls():
    dtype, k = np.float32, 16
    d = _inputs(k)
    truth = np.random.RandomState(2).rand(4, OH.N).astype(dtype)
    Y = _training(d, dtype, 'sparse')
    a, b = _model(d, dtype), _model(d, dtype)
    with Session(Y, a, **synth.HYPER) as s:
        s.run(2).mark()
        marked = [x.copy() for x in (s.download().W, a.H, a.lag_val)]
        s.forecast(4, truth=truth, return_forecast=False)
        rows, table = s.forecast_series_sums()
        st = s.stats(8)
        keep = [key for key in st[0] if not key.startswith('ms_')]
        with pytest.raises(RuntimeError, match='no noise'):
            s.forecast_dist(4, truth=truth)
        s.fit_noise()
        s.forecast_dist(4, truth=truth)
        with pytest.raises(RuntimeError, match='dense'):
            s.forecast_dist(4, truth=smat.csr_matrix(truth))
        s.set_noise(*s.noise())
        s.forecast_interval(4, truth=truth)
        st2 = s.stats(8)
        assert len(st2) == len(st) == 2 and [[x[key] for key in keep] for x in st2] == [[x[key] for key in keep] for x in st]
        rows2, table2 = s.forecast_series_sums()
        assert rows2 == rows == 4 and np.array_equal(table2, table)          # the point table and its kept truth row
        assert s.interval_series_sums()[0] == 8
        s.forecast(4, truth=truth, return_forecast=False)
        kept_row = s.forecast_series_sums()[1]
        s.download()
        assert all(np.array_equal(x, y) for x, y in zip(marked, (a.W, a.H, a.lag_val)))
        s.run(1).download()
        after = [x.copy() for x in (a.W, a.H, a.lag_val)]
        assert len(s.stats(8)) == 3
        s.rewind().download()
        assert all(np.array_equal(x, y) for x, y in zip(marked, (a.W, a.H, a.lag_val)))
    with Session(Y, b, **synth.HYPER) as s:                 # the same trajectory without any of the calls
        s.run(2)
        s.forecast(4, truth=truth, return_forecast=False)
        s.forecast(4, truth=truth, return_forecast=False)
        assert np.array_equal(s.forecast_series_sums()[1], kept_row)
        s.run(1).download()
    assert all(np.array_equal(x, y) for x, y in zip(after, (b.W, b.H, b.lag_val)))


@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_two_ranks_are_bit_identical_to_one(storage, missing, monkeypatch):
    dtype, k = np.float32, 40
    # (full observation fits an all-zero series exactly -- h_j = 0, sigma2_j = 0 -- and a zero deviation scores NaN: the emptied
    # series belongs to the observed-entries case, where it takes the pooled value)
    d = _inputs(k) if missing else dict(OH.inputs(k))
    Y = _training(d, dtype, storage)
    truth = np.random.RandomState(9).rand(6, OH.N).astype(dtype)

    def run():
        with Session(Y, _model(d, dtype), missing=missing, **synth.HYPER) as s:
            s.run(2)
            stats = s.fit_noise()
            noise = s.noise()
            out = s.forecast_dist(6, truth=truth, return_latent=True)
            table = s.interval_series_sums()[1]
            s.set_noise(noise[0] * 2, noise[1] * 3)
            return stats, noise, out, table, s.forecast_dist(6)[1], s.describe()

    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = run()
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two = run()
    assert '1 rank' in one[5] and '2 ranks' in two[5]
    assert one[0] == two[0] and all(np.array_equal(x, y) for x, y in zip(one[1], two[1]))
    assert all(np.array_equal(x, y) for x, y in zip(one[2], two[2]))
    assert np.array_equal(one[3], two[3]) and np.array_equal(one[4], two[4])


# ---- 5. the rolling evaluation ---------------------------------------------------------------------------------------------------------
ROLL = dict(k=3, window_size=8, nr_windows=3, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=4, threads=2, seed=0)
ROLL_LAGS = [1, 2, 5]


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_rolling_validate_with_intervals(dtype):
    Y = np.ascontiguousarray(OH.inputs(16)['Y'].toarray().astype(dtype))     # the dense 96 x 50 panel
    assert Y.shape == (OH.T, OH.N)
    level, win, nw = 0.9, ROLL['window_size'], ROLL['nr_windows']
    start = Y.shape[0] - win * nw
    kw = dict(missing=False, threshold=0, forecast_on_device=True, **ROLL)
    plain = trmf.rolling_validate(Y, ROLL_LAGS, **kw)
    assert isinstance(plain, Metrics)                        # the default returns what it returns today
    point, iv = trmf.rolling_validate(Y, ROLL_LAGS, interval_level=level, **kw)
    assert isinstance(point, Metrics) and isinstance(iv, IntervalMetrics)
    assert np.array_equal(fields(point), fields(plain))
    # the host loop: the same session, every window's model downloaded, Model.fit_noise / Model.forecast_std on the host
    model = trmf.Model.initialize(Y[:start], ROLL_LAGS, ROLL['k'], seed=0)
    tables = np.zeros((Y.shape[1], 7))
    with Session(Y[:start], model, missing=False, log_norms=False, timing=0,
                 lambdaI=ROLL['lambdaI'], lambdaAR=ROLL['lambdaAR'], lambdaLag=ROLL['lambdaLag']) as s:
        for w in range(nw):
            cut = start + w * win
            if w:
                model = trmf.Model.initialize(Y[:cut], ROLL_LAGS, ROLL['k'], seed=0, warm_start_model=model)
                s.append_rows(Y[cut - win:cut])
                s.model = model
            s.run(ROLL['max_iter']).download()
            mean = s.forecast(win, threshold=0)
            sd = model.fit_noise(Y[:cut], missing=False).forecast_std(win)
            s.fit_noise()
            dev_mean, dev_sd = s.forecast_dist(win, level=level, threshold=0)
            assert np.array_equal(dev_mean, mean) and dev_sd.shape == sd.shape
            tables += IntervalMetrics.series_sums(Y[cut:cut + win], mean, sd, level)
    host = IntervalMetrics.from_series_sums(tables, level)
    evidence('rolling intervals %s: device %s | host loop %s' % (np.dtype(dtype).name, iv, host))
    # a cell's sd differs by at most an ulp of the element type (fp64: by the fit's summation order), so the scores -- smooth in sd
    # with condition numbers below 3 (z2: 2; crps: 1 + |z| / g(z) <= 2.6; nll: |1 - z^2| absolute) -- move by a few ulp
    eps = 8 * float(np.finfo(dtype).eps) if dtype == np.float32 else 8 * (2 * Y.shape[0] + 8) * U
    assert iv.coverage == host.coverage and iv.m_coverage == host.m_coverage
    for name in ('width', 'z2', 'crps'):
        assert abs(getattr(iv, name) - getattr(host, name)) <= eps * abs(getattr(host, name)), name
    assert abs(iv.nll - host.nll) <= eps * (1.0 + host.z2 + abs(host.nll))
