"""CPU: the NumPy statement of the forecast uncertainty (trmf/uncertainty.py) -- noise fit, impulse response, predictive standard
deviation and interval scores -- against closed forms, hand-built tables and the generative model itself."""
import math

import numpy as np
import pytest
import scipy.sparse as smat
from scipy.special import erf, ndtri

import trmf
from helpers import make_model
from trmf import IntervalMetrics, fit_noise, forecast_std, impulse_response
from trmf.uncertainty import forecast_var, interval_terms, latent_forecast_var, z_of_level

EPS = float(np.finfo(np.float64).eps)
LAGS = np.array([1, 2, 5], dtype=np.uint32)


def _contractive(rng, nlag, k):
    theta = rng.randn(nlag, k)
    return np.asfortranarray(theta / (np.abs(theta).sum(axis=0) + 0.1))


# ---- 1. the impulse response is the roll-out's linear map ----------------------------------------------------------------------
def test_impulse_response_equals_the_rollout_of_a_unit_impulse():
    rng = np.random.RandomState(0)
    k, T, steps = 4, 20, 30
    theta = _contractive(rng, len(LAGS), k)
    W = rng.randn(T, k)
    bumped = W.copy()
    bumped[-1] += 1.0                                   # a unit impulse in the last row of every (independent) dimension
    base = make_model(W, rng.randn(3, k), theta, LAGS).latent_forecast(steps)[T:]
    moved = make_model(bumped, rng.randn(3, k), theta, LAGS).latent_forecast(steps)[T:]
    psi = impulse_response(LAGS, theta, steps + 1)
    assert np.array_equal(psi[0], np.ones(k))
    # (the difference of two roll-outs carries the rounding of their own size, |W| ~ 3, not of psi's)
    assert np.abs((moved - base) - psi[1:]).max() <= 1e-13 * max(np.abs(psi).max(), np.abs(moved).max())


def test_lag_zero_contributes_nothing_as_in_the_rollout():
    rng = np.random.RandomState(1)
    theta = _contractive(rng, 3, 2)
    with_zero = impulse_response([0, 1, 5], theta, 12)
    without = impulse_response([1, 5], theta[1:], 12)
    assert np.array_equal(with_zero, without)


# ---- 2. AR(1) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('theta', [0.7, -0.4, 0.0])
def test_ar1_variance_has_its_closed_form(theta):
    q, steps = 0.3, 20
    v = latent_forecast_var([1], np.array([[theta]]), [q], steps)[:, 0]
    s = np.arange(steps)
    want = q * (1.0 - theta ** (2 * (s + 1))) / (1.0 - theta ** 2)
    assert np.abs(v - want).max() <= 1e-14 * np.abs(want).max()
    assert np.all(np.abs(v / want - 1.0) <= 1e-14)


# ---- 3. fit_noise on hand-built residuals ----------------------------------------------------------------------------------------
def _planted():
    """Dyadic values throughout, so that every product and sum below is exact in fp64: W follows the AR recursion plus a known
    innovation table, Y = W H^T plus a known residual table on the stored cells."""
    rng = np.random.RandomState(3)
    T, n, k, m = 12, 6, 2, 5
    theta = np.asfortranarray(np.array([[0.5, -0.25], [0.25, 0.5], [-0.5, 0.25]]))
    eta = rng.randint(-4, 5, size=(T, k)) / 8.0
    W = np.zeros((T, k))
    W[:m] = rng.randint(-3, 4, size=(m, k)).astype(np.float64)
    for i in range(m, T):
        W[i] = sum(theta[l] * W[i - int(LAGS[l])] for l in range(3)) + eta[i]
    H = rng.randint(-2, 3, size=(n, k)).astype(np.float64)
    R = rng.randint(-6, 7, size=(T, n)) / 4.0
    mask = rng.rand(T, n) < 0.6
    mask[:, 4] = False                                  # a series without a stored entry
    mask[0, 0] = True
    return dict(T=T, n=n, k=k, m=m, theta=theta, eta=eta, W=W, H=H, R=R, mask=mask)


def test_fit_noise_recovers_planted_residuals_exactly():
    p = _planted()
    full = p['W'].dot(p['H'].T) + p['R']
    full[full == 0] = 0.0
    rows, cols = np.nonzero(p['mask'])
    Y = smat.csr_matrix((full[rows, cols], (rows, cols)), shape=full.shape)        # explicit entries, zeros included
    sigma2, q, info = fit_noise(p['W'], p['H'], LAGS, p['theta'], Y, missing=True)
    cnt = p['mask'].sum(axis=0)
    sq = (np.where(p['mask'], p['R'], 0.0) ** 2).sum(axis=0)
    pooled = sq.sum() / cnt.sum()
    want = np.where(cnt > 0, sq / np.maximum(cnt, 1), pooled)
    assert cnt[4] == 0 and info['series_pooled'] == 1 and np.array_equal(info['cnt'], cnt.astype(np.float64))
    assert np.abs(sigma2 - want).max() <= 2 * EPS * want.max() and abs(sigma2[4] - pooled) <= 2 * EPS * pooled
    assert abs(info['pooled'] - pooled) <= 2 * EPS * pooled
    want_q = (p['eta'][p['m']:] ** 2).sum(axis=0) / (p['T'] - p['m'])
    assert np.abs(q - want_q).max() <= 2 * EPS * want_q.max()


def test_fit_noise_full_observation_reads_absent_entries_as_zero():
    p = _planted()
    stored = np.where(p['mask'], p['W'].dot(p['H'].T) + p['R'], 0.0)
    Y = smat.csr_matrix(stored)
    sigma2, q, info = fit_noise(p['W'], p['H'], LAGS, p['theta'], Y, missing=False)
    want = ((stored - p['W'].dot(p['H'].T)) ** 2).sum(axis=0) / p['T']
    assert info['series_pooled'] == 0 and np.array_equal(info['cnt'], np.full(p['n'], float(p['T'])))
    assert np.abs(sigma2 - want).max() <= 2 * EPS * want.max()
    dense = fit_noise(p['W'], p['H'], LAGS, p['theta'], stored, missing=False)
    assert np.array_equal(dense[0], sigma2) and np.array_equal(dense[1], q)


def test_fit_noise_guards():
    p = _planted()
    Y = smat.csr_matrix(np.where(p['mask'], 1.0, 0.0))
    with pytest.raises(ValueError, match='largest lag'):
        fit_noise(p['W'][:5], p['H'], LAGS, p['theta'], Y[:5])
    with pytest.raises(ValueError, match='sparse'):
        fit_noise(p['W'], p['H'], LAGS, p['theta'], Y.toarray(), missing=True)
    with pytest.raises(ValueError, match='describe'):
        fit_noise(p['W'], p['H'], LAGS, p['theta'], Y[:, :3])
    with pytest.raises(ValueError, match='no stored entry'):
        fit_noise(p['W'], p['H'], LAGS, p['theta'], smat.csr_matrix(Y.shape))


# ---- 4. the formula against the generative model ---------------------------------------------------------------------------------
def test_predictive_interval_covers_the_generative_model():
    """True parameters, not fitted ones: R independent futures from one state; per (step, series) the share inside the 90 %
    interval is Binomial(R, 0.9) / R, so every one of the 96 cells must lie within 5 standard deviations of 0.9."""
    rng = np.random.RandomState(20161)
    k, n, steps, R, level = 3, 8, 12, 4000, 0.9
    m = int(LAGS.max())
    theta = _contractive(rng, len(LAGS), k)
    H = rng.randn(n, k)
    sigma2 = rng.uniform(0.05, 0.5, size=n)
    q = rng.uniform(0.1, 1.0, size=k)
    hist = rng.randn(m, k)
    Wf = np.zeros((R, m + steps, k))
    Wf[:, :m] = hist
    for s in range(m, m + steps):
        Wf[:, s] = sum(theta[l] * Wf[:, s - int(LAGS[l])] for l in range(len(LAGS))) + rng.randn(R, k) * np.sqrt(q)
    futures = Wf[:, m:].dot(H.T) + rng.randn(R, steps, n) * np.sqrt(sigma2)
    model = make_model(hist, H, theta, LAGS)
    mean = model.forecast(steps)[0]
    sd = forecast_std(H, LAGS, theta, sigma2, q, steps)
    inside = (np.abs(futures - mean) <= z_of_level(level) * sd).mean(axis=0)
    dev = np.abs(inside - level) / math.sqrt(level * (1 - level) / R)
    print('generative coverage: worst cell %.2f standard deviations, mean coverage %.4f' % (dev.max(), inside.mean()))
    assert inside.shape == (steps, n) and dev.max() <= 5.0, dev.max()
    # what the gate would see without the psi accumulation / without the H^2 weighting
    flat = np.sqrt(sigma2[None, :] + (H * H).dot(q)[None, :] * np.ones((steps, 1)))
    assert (np.abs((np.abs(futures - mean) <= z_of_level(level) * flat).mean(axis=0) - level) / math.sqrt(level * (1 - level) / R)).max() > 10
    unweighted = np.sqrt(sigma2[None, :] + latent_forecast_var(LAGS, theta, q, steps).sum(axis=1)[:, None])
    assert (np.abs((np.abs(futures - mean) <= z_of_level(level) * unweighted).mean(axis=0) - level) / math.sqrt(level * (1 - level) / R)).max() > 10


# ---- 5. forecast_std, the Model methods, IntervalMetrics -------------------------------------------------------------------------
def test_forecast_std_transform_rounding_and_guards():
    rng = np.random.RandomState(5)
    k, n, steps = 3, 5, 7
    theta = _contractive(rng, 3, k).astype(np.float32)
    H = rng.randn(n, k).astype(np.float32)
    sigma2, q = rng.uniform(0.1, 1, n), rng.uniform(0.1, 1, k)
    V = forecast_var(H, LAGS, theta, sigma2, q, steps)
    psi = impulse_response(LAGS, theta, steps)
    by_hand = np.array([[sigma2[j] + sum(float(H[j, d]) ** 2 * q[d] * (psi[:s + 1, d] ** 2).sum() for d in range(k)) for j in range(n)]
                        for s in range(steps)])
    assert np.abs(V - by_hand).max() <= (k + 4) * EPS * by_hand.max()
    sd = forecast_std(H, LAGS, theta, sigma2, q, steps)
    assert sd.dtype == np.float32 and np.array_equal(sd, np.sqrt(V).astype(np.float32))

    class Tr(object):
        a = np.linspace(-2.0, 3.0, n).reshape(1, n).astype(np.float32)
    scaled = forecast_std(H, LAGS, theta, sigma2, q, steps, transform=Tr, dtype=np.float64)
    assert np.array_equal(scaled, np.sqrt(V) / np.abs(Tr.a.astype(np.float64)))
    for bad in (np.r_[sigma2[:-1], -1.0], np.r_[sigma2[:-1], np.nan]):
        with pytest.raises(ValueError, match='finite and not negative'):
            forecast_std(H, LAGS, theta, bad, q, steps)
    with pytest.raises(ValueError, match='sigma2 must have'):
        forecast_std(H, LAGS, theta, sigma2[:-1], q, steps)
    explosive = theta.copy()
    explosive[0, 0] = 3.0
    with pytest.raises(ValueError, match='explosive'):
        forecast_std(H, LAGS, explosive, sigma2, q, 2000)


def test_model_fit_noise_and_forecast_std():
    rng = np.random.RandomState(6)
    T, n, k = 40, 6, 2
    theta = _contractive(rng, 3, k).astype(np.float32)
    W, H = rng.rand(T, k).astype(np.float32), rng.rand(n, k).astype(np.float32)
    Y = smat.csr_matrix(np.where(rng.rand(T, n) < 0.5, rng.rand(T, n), 0.0).astype(np.float32))
    model = make_model(W, H, theta, LAGS)
    with pytest.raises(ValueError, match='no noise fitted'):
        model.forecast_std(4)
    assert model.fit_noise(Y, missing=True) is model
    sigma2, q, _ = fit_noise(W, H, LAGS, theta, Y, True)
    assert np.array_equal(model.noise[0], sigma2) and np.array_equal(model.noise[1], q)
    assert np.array_equal(model.forecast_std(4), forecast_std(H, LAGS, theta, sigma2, q, 4))
    # under a transform the residuals are those of the transformed values and the deviation is reported in raw units
    raw = (rng.rand(T, n) * np.linspace(1, 4, n)).astype(np.float32)
    tr = trmf.model.NormalizedTransform(raw)
    model.transform = tr
    model.fit_noise(raw, missing=False)
    s2, qq, _ = fit_noise(W, H, LAGS, theta, tr.preprocess(raw).astype(np.float32), False)
    assert np.array_equal(model.noise[0], s2)
    assert np.array_equal(model.forecast_std(3), forecast_std(H, LAGS, theta, s2, qq, 3, transform=tr))


def test_interval_metrics_against_hand_computed_cells():
    truth = np.array([[1.0, -2.0], [0.5, 4.0], [3.0, 0.0]])
    mean = np.array([[1.5, -2.0], [0.0, 1.0], [3.0, 0.25]])
    sd = np.array([[0.5, 1.0], [0.25, 1.0], [2.0, 0.125]])
    level = 0.8
    zq = float(ndtri(0.9))
    cells = []
    for i in range(3):
        for j in range(2):
            e, s = truth[i, j] - mean[i, j], sd[i, j]
            z = e / s
            Phi, phi = 0.5 * (1 + erf(z / math.sqrt(2))), math.exp(-z * z / 2) / math.sqrt(2 * math.pi)
            cells.append((j, abs(e) <= zq * s, s, abs(truth[i, j]), z * z, 0.5 * math.log(2 * math.pi * s * s) + 0.5 * z * z,
                          s * (z * (2 * Phi - 1) + 2 * phi - 1 / math.sqrt(math.pi))))
    got = IntervalMetrics.generate(truth, mean, sd, level)
    N = len(cells)
    want = dict(coverage=sum(c[1] for c in cells) / N, width=2 * zq * sum(c[2] for c in cells) / sum(c[3] for c in cells),
                z2=sum(c[4] for c in cells) / N, nll=sum(c[5] for c in cells) / N, crps=sum(c[6] for c in cells) / N,
                m_coverage=np.mean([np.mean([c[1] for c in cells if c[0] == j]) for j in range(2)]))
    assert got._fields == ('coverage', 'width', 'z2', 'nll', 'crps', 'm_coverage')
    for name in got._fields:
        assert abs(getattr(got, name) - want[name]) <= 1e-14 * max(1.0, abs(want[name])), name
    assert want['coverage'] == 3 / 6 and got.crps > 0
    table = IntervalMetrics.series_sums(truth, mean, sd, level)
    assert table.shape == (2, 7) and np.array_equal(table[:, 0], [3.0, 3.0]) and np.array_equal(table[:, 1], [2.0, 1.0])
    assert got == IntervalMetrics.from_series_sums(table, level)
    # a perfectly calibrated normal sample scores what the theory says
    rng = np.random.RandomState(8)
    z = rng.randn(20000, 3)
    cal = IntervalMetrics.generate(2.0 * z, np.zeros_like(z), np.full_like(z, 2.0), 0.9)
    assert abs(cal.coverage - 0.9) < 0.01 and abs(cal.z2 - 1.0) < 0.03 and abs(cal.crps - 2.0 / math.sqrt(math.pi)) < 0.02


def test_interval_metrics_guards():
    ok = np.ones((2, 2))
    for level in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match='level'):
            IntervalMetrics.generate(ok, ok, ok, level)
    with pytest.raises(ValueError, match='one shape'):
        IntervalMetrics.generate(ok, ok[:1], ok, 0.9)
    with pytest.raises(ValueError, match='n x 7'):
        IntervalMetrics.from_series_sums(np.zeros((3, 6)), 0.9)
    with pytest.raises(ValueError, match='no scored cell'):
        IntervalMetrics.from_series_sums(np.zeros((3, 7)), 0.9)
    with pytest.raises(ValueError, match='forecast_on_device'):
        trmf.rolling_validate(np.ones((40, 3), dtype=np.float32), [1, 2], k=2, window_size=4, nr_windows=2, interval_level=0.9)
    assert len(interval_terms(ok, ok, ok, 1.0)) == 6
