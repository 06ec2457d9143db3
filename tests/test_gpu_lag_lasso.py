"""GPU (-m gpu): sparse lag weights -- theta_lasso_kernel behind trmf_session_set_lag_penalty / _solve_lags / _lag_stats and
the front end above them -- against optimality conditions and the fp64 NumPy restatement of tests/lag_helpers.py.

Designed inputs (tests/lag_helpers.py: SHAPES, designed): W is a noisy AR process on lags {1: 0.5, 24: 0.4} handed to the
session as the initial model, Y any small sparse matrix (n = 20), Theta0 the model's random start, lambdaLag = 0.5,
lambdaL1 = 0.2 median_t |b_t|_inf.  Every tolerance is derived where it is used (lag_helpers.kkt_bound for the KKT residuals: it
adds a third, fp64-arithmetic term to the specification's two-term form and says so); small shapes, a few seconds for the whole file."""
import functools

import numpy as np
import pytest
import scipy.sparse as smat

import lag_helpers as L
import trmf
from forecast_helpers import fields
from helpers import make_model
from trmf import synth
from trmf.session import Session

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
CASES = [(name, dt) for name in sorted(L.SHAPES) for dt in DTYPES]
N_ITEMS = 20


def _eps(dtype):
    return float(np.finfo(dtype).eps)


@functools.lru_cache(maxsize=None)
def _inputs(name, dtype):
    """The designed problem in the library's element type, its restatement solved once (shared, never modified)."""
    dtype = np.dtype(dtype).type
    d = L.designed(name, dtype)
    T, k, lags = d['T'], d['k'], d['lags']
    Y = smat.random(T, N_ITEMS, density=0.2, random_state=np.random.RandomState(5), format='csr', dtype=np.float64).astype(dtype)
    m0 = synth.initial_model(Y, lags, k, seed=0, dtype=dtype)
    m0.W[:] = d['W']
    d['Y'], d['m0'] = Y, m0
    d['th0'] = m0.lag_val.astype(np.float64)
    d['Gabs'], d['babs'] = L.gram_rhs(d['W'], lags, absolute=True)
    ref = [L.lasso_cd(d['G'][t], d['b'][t], d['lam'], d['l1'], d['th0'][:, t]) for t in range(k)]
    d['theta_ref'] = np.stack([r[0] for r in ref], axis=1)                 # |L| x k
    d['sweeps_ref'] = [r[1] for r in ref]
    for v in (d['W'], d['G'], d['b'], d['Gabs'], d['babs'], d['th0'], d['theta_ref']):
        v.setflags(write=False)
    return d


def _copy(m):
    return make_model(m.W, m.H, m.lag_val, m.lag_set)


def _open(d, **kw):
    model = _copy(d['m0'])
    hyper = dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=d['lam'])
    hyper.update(kw)
    return Session(d['Y'], model, missing=True, **hyper), model


@functools.lru_cache(maxsize=None)
def _solved(name, dtype, refit):
    """Theta and the record after set_lag_penalty(l1, refit); solve_lags() on the designed inputs (computed once per case)."""
    d = _inputs(name, dtype)
    sess, model = _open(d)
    with sess:
        sess.set_lag_penalty(d['l1'], refit).solve_lags()
        stats = sess.lag_stats()
        desc = sess.describe()
        sess.download()
    assert np.array_equal(model.W, d['W'])                                 # solve_lags leaves W alone
    theta = model.lag_val.copy()
    theta.setflags(write=False)
    return theta, stats, desc


def _bounds(d, theta, stats, dtype, th0=None):
    """B (|L| x k) of lag_helpers.kkt_bound for a downloaded Theta."""
    th0 = d['th0'] if th0 is None else th0
    n_sum = d['T'] - max(d['lags'])
    return np.stack([L.kkt_bound(d['G'][t], d['b'][t], d['Gabs'][t], d['babs'][t], d['lam'], theta[:, t], th0[:, t], n_sum,
                                 int(stats['per_dim'][t, 0]), dtype) for t in range(theta.shape[1])], axis=1)


def _assert_kkt(G, b, lam, l1, theta, B, dims, what):
    """Non-zero coordinates: |g_j + l1 sign th_j| <= B_j; zero coordinates: |g_j| <= l1 + B_j (g from fp64 arithmetic on the
    downloaded Theta).  Prints the worst ratio before asserting."""
    worst = 0.0
    for t in dims:
        th = theta[:, t].astype(np.float64)
        g, res = L.kkt(G[t], b[t], lam, l1, th)
        worst = max(worst, float((res / B[:, t]).max()))
    print('%s: worst KKT residual / bound %.3g (l1 %.4g, max bound / l1 %.2e)' % (what, worst, l1, float(B.max()) / l1))
    assert float(B.max()) <= 1e-3 * l1, 'the tolerance must never decide the support'
    assert worst <= 1.0, what


# ---- 1. optimality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dtype', CASES)
def test_solve_lags_satisfies_the_kkt_conditions(name, dtype):
    d = _inputs(name, dtype)
    theta, stats, desc = _solved(name, dtype, False)
    assert 'lag penalty: lasso' in desc and 'refit=0' in desc
    assert stats['capped'] == 0 and not stats['per_dim'][:, 2].any(), stats['per_dim']      # the restatement needs < 100 sweeps
    assert stats['refit_skipped'] == 0
    assert stats['per_dim'][:, 0].min() >= 1
    print('sweeps: device %d..%d, restatement %d..%d' % (stats['per_dim'][:, 0].min(), stats['per_dim'][:, 0].max(), min(d['sweeps_ref']), max(d['sweeps_ref'])))
    B = _bounds(d, theta, stats, dtype)
    _assert_kkt(d['G'], d['b'], d['lam'], d['l1'], theta, B, range(d['k']), '%s %s' % (name, np.dtype(dtype).name))


# ---- 2. support and values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dtype', CASES)
def test_support_and_values_match_the_restatement(name, dtype):
    d = _inputs(name, dtype)
    theta, stats, _ = _solved(name, dtype, False)
    ref = d['theta_ref']
    B = _bounds(d, theta, stats, dtype)
    unclear = np.zeros(ref.shape, dtype=bool)
    for t in range(d['k']):
        g, _ = L.kkt(d['G'][t], d['b'][t], d['lam'], d['l1'], ref[:, t])
        zero = ref[:, t] == 0
        unclear[:, t] = np.where(zero, np.abs(g) > 0.98 * d['l1'], np.abs(ref[:, t]) < 1e-3)
    assert unclear.mean() <= 0.10                                           # first on the restatement itself
    assert np.array_equal((theta != 0)[~unclear], (ref != 0)[~unclear])
    assert not np.signbit(theta[theta == 0]).any()                          # zeros are +0
    for t in range(d['k']):
        if not np.array_equal(theta[:, t] != 0, ref[:, t] != 0):
            continue                                                        # (an unclear coordinate decided the other way)
        S = np.flatnonzero(ref[:, t] != 0)
        if len(S) == 0:
            continue
        inv = np.linalg.inv(d['G'][t][np.ix_(S, S)] + d['lam'] * np.eye(len(S)))
        tol = np.abs(inv).sum(axis=1).max() * B[:, t].max()                 # |inv|_inf max_j B_j: both solve the same sign-fixed linear system up to B
        assert np.abs(theta[:, t].astype(np.float64) - ref[:, t]).max() <= tol, (name, t)
    assert np.array_equal(stats['per_dim'][:, 1], (theta != 0).sum(axis=0))


# ---- 3. refit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dtype', CASES)
def test_refit_is_the_ridge_solution_on_the_selected_support(name, dtype):
    """Tolerance on the support, per dimension with m = |S|, A = G_SS + lambdaLag I, everything in the 2-norm and then taken
    coordinate-wise (|x|_inf <= |x|_2):
      * the device's fp64 Cholesky and numpy's LU each: 4 m (3 m + 1) u64 cond(A) |theta| (Higham, Accuracy and Stability of
        Numerical Algorithms, Theorem 10.4 with 10.6: backward error 4 m (3 m + 1) u |A|_2), i.e. c m cond eps64 with c = 2 (3 m + 1),
        twice
      * the two Grams are the same rounded products added in different orders: |inv|_2 2 n_sum u64 (|Gabs_SS|_2 |theta|_2 + |babs_S|_2)
      * one rounding to the element type: u_real |theta_j|."""
    d = _inputs(name, dtype)
    lasso, _, _ = _solved(name, dtype, False)
    theta, stats, desc = _solved(name, dtype, True)
    assert 'refit=1' in desc and stats['refit_skipped'] == 0 and stats['capped'] == 0
    assert np.array_equal(theta != 0, lasso != 0)                           # the refit keeps the lasso's support
    off = theta[lasso == 0]
    assert np.all(off == 0) and not np.signbit(off).any()                   # bit-exact +0
    u64, ureal, n_sum = L.U64, _eps(dtype) / 2, d['T'] - max(d['lags'])
    worst = 0.0
    for t in range(d['k']):
        S = np.flatnonzero(theta[:, t] != 0)
        want, cond = L.refit(d['G'][t], d['b'][t], d['lam'], theta[:, t])
        m = len(S)
        if m == 0:
            continue
        A = d['G'][t][np.ix_(S, S)] + d['lam'] * np.eye(m)
        n2 = np.linalg.norm(want)
        tol = 2 * 4 * m * (3 * m + 1) * u64 * cond * n2
        tol += np.linalg.norm(np.linalg.inv(A), 2) * 2 * n_sum * u64 * (np.linalg.norm(d['Gabs'][t][np.ix_(S, S)], 2) * n2 + np.linalg.norm(d['babs'][t][S]))
        err = np.abs(theta[S, t].astype(np.float64) - want[S])
        worst = max(worst, float((err / (tol + ureal * np.abs(want[S]))).max()))
    print('%s %s: worst refit error / tolerance %.3g' % (name, np.dtype(dtype).name, worst))
    assert worst <= 1.0
    assert np.array_equal(stats['per_dim'][:, 1], (theta != 0).sum(axis=0))


# ---- 4. ridge limit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dtype', CASES)
def test_tiny_l1_is_the_ridge_path(name, dtype):
    """lambdaL1 = 1e-12 |b|_inf against the ridge kernels (Cholesky in the element type), per dimension in the 2-norm.  Three terms:
      * the specification's: the Cholesky's own bound c |L| cond(A) eps(real) |theta|_2, A = G + lambdaLag I, with the FIXED c = 4.
        Higham (Accuracy and Stability of Numerical Algorithms, Theorem 10.4): the computed solution solves (A + dA) x = b with
        |dA| <= gamma_{3n+1} |R^T| |R|, gamma_m ~ m u, u = eps / 2.  With rho = | |R^T| |R| |_2 / |A|_2 the forward error is
        cond u (3 n + 1) rho to first order.  The ridge kernel also rounds G (|dG| <= u |A| <= u |R^T| |R|: cond u rho), b and
        the diagonal's + lambdaLag (cond u each) to the element type.  Sum: cond eps/2 ((3 n + 2) rho + 2).  rho lies between 1 and n;
        the worst case n would make the term quadratic in |L| and the check vacuous (8 x |theta| at 160 lags in fp32), so the test
        computes rho from the fp64 factor of its own A and asserts rho <= 2 (1.0 .. 1.7 on the designed inputs): then the sum is
        <= cond eps (3 n + 3) <= 4 n cond eps for n >= 3.  (At 160 lags in fp32, cond ~ 500: 4 % of |theta|.)
      * the distance between the two problems' EXACT minimisers, |A^-1 lambdaL1 sign(theta)|_2.  The specification's tolerance
        leaves it out, and with it no solver could pass in fp64: lambdaL1 is 1e-12 |b|_inf, ~1e4 u64 relative before any amplification.
      * the lasso solve's own distance from its exact minimiser, |A^-1|_2 |B|_2 with the KKT bound B of test 1."""
    d = _inputs(name, dtype)
    n = len(d['lags'])
    l1 = 1e-12 * float(np.abs(d['b']).max())
    sess, model = _open(d)
    with sess:
        sess.mark()
        sess.set_lag_penalty(l1, False).solve_lags()
        stats = sess.lag_stats()
        lasso = sess.download().lag_val.copy()
        sess.rewind().set_lag_penalty(0.0, False).solve_lags()
        assert not sess.lag_stats()['per_dim'].any() and 'lag penalty: ridge' in sess.describe()
        ridge = sess.download().lag_val.copy()
    assert stats['capped'] == 0
    B = _bounds(d, lasso, stats, dtype)
    worst = first = 0.0
    for t in range(d['k']):
        A = d['G'][t] + d['lam'] * np.eye(n)
        inv = np.linalg.inv(A)
        exact = np.linalg.solve(A, d['b'][t])
        R = np.linalg.cholesky(A).T
        rho = np.linalg.norm(np.abs(R.T).dot(np.abs(R)), 2) / np.linalg.norm(A, 2)
        assert n >= 3 and rho <= 2.0, (t, rho)                              # what c = 4 rests on: a property of the inputs
        tol = 4 * n * np.linalg.cond(A) * _eps(dtype) * np.linalg.norm(exact)
        first = max(first, tol / np.linalg.norm(exact))
        tol += np.linalg.norm(inv.dot(l1 * np.sign(exact)))
        tol += np.linalg.norm(inv, 2) * np.linalg.norm(B[:, t])
        worst = max(worst, float(np.linalg.norm(lasso[:, t].astype(np.float64) - ridge[:, t].astype(np.float64)) / tol))
    print('%s %s: worst |lasso - ridge| / tolerance %.3g (largest first term %.3g |theta|_2)' % (name, np.dtype(dtype).name, worst, first))
    assert first < 0.05, 'the tolerance must stay a check'
    assert worst <= 1.0


# ---- 5. full shrinkage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_full_shrinkage_gives_exact_zeros_and_training_goes_on(dtype):
    d = _inputs('lags24', dtype)
    sess, model = _open(d)
    with sess:
        sess.set_lag_penalty(1.25 * float(np.abs(d['b']).max()), False).solve_lags()      # >= max_t |b_t|_inf: theta = 0 is optimal
        stats = sess.lag_stats()
        _, Wnew = sess.forecast(5, return_latent=True)
        theta = sess.download().lag_val.copy()
        sess.run(2)
        J = sess.objective()
        sess.download()
    assert np.all(theta == 0) and not np.signbit(theta).any()
    assert not stats['per_dim'][:, 1].any() and stats['capped'] == 0
    assert np.all(Wnew == 0)                                                # the rolled rows of an all-zero AR model
    assert np.isfinite(J) and np.all(np.isfinite(model.W)) and np.all(np.isfinite(model.H)) and np.all(np.isfinite(model.lag_val))


# ---- 6. determinism and neutrality ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_mark_rewind_repeats_the_bits_with_l1_on(dtype):
    d = _inputs('gap', dtype)
    sess, model = _open(d, period_Lag=2)
    with sess:
        sess.set_lag_penalty(d['l1'], True).mark()
        a = sess.solve_lags().download().lag_val.copy()
        sa = sess.lag_stats()
        b = sess.rewind().solve_lags().download().lag_val.copy()
        sb = sess.lag_stats()
        assert np.array_equal(a, b) and np.array_equal(sa['per_dim'], sb['per_dim'])
        sess.rewind().run(4).download()
        first = [model.W.copy(), model.H.copy(), model.lag_val.copy(), sess.lag_stats()['per_dim']]
        sess.rewind().run(4).download()
        again = [model.W, model.H, model.lag_val, sess.lag_stats()['per_dim']]
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        assert first[3][:, 0].all()                                        # lasso solves ran


def _train_problem(dtype, missing):
    if missing:
        p = synth.sparse_problem(n=300, T=260, k=8, nlag=5, density=0.08, dtype=dtype, seed=4)
    else:
        p = synth.dense_problem(40, 260, 8, [1, 2, 3, 4, 7], dtype=dtype, seed=4)
    return p, synth.initial_model(p['Y'], p['lag_set'], 8, seed=1, dtype=dtype)


@pytest.mark.parametrize('missing', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_penalty_set_and_cleared_leaves_the_default_path_alone(dtype, missing):
    p, m0 = _train_problem(dtype, missing)
    out = []
    for touch in (False, True):
        model = _copy(m0)
        with Session(p['Y'], model, missing=missing, **synth.HYPER) as s:
            if touch:
                s.set_lag_penalty(3.0, True).set_lag_penalty(0.0, False)
            s.run(4).download()
            assert 'lag penalty: ridge' in s.describe()
        out.append(model)
    assert all(np.array_equal(getattr(out[0], f), getattr(out[1], f)) for f in ('W', 'H', 'lag_val'))


# ---- 7. through the ALS loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('missing', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_als_loop_with_l1_ends_at_a_kkt_point(dtype, missing):
    p, m0 = _train_problem(dtype, missing)
    lags = [int(v) for v in p['lag_set']]
    ridge = _copy(m0)
    with Session(p['Y'], ridge, missing=missing, period_Lag=2, **synth.HYPER) as s:
        s.run(6).download()
    _, b0 = L.gram_rhs(ridge.W, lags)
    l1 = 0.2 * float(np.median(np.abs(b0).max(axis=1)))                     # the designed inputs' rule, at the ridge run's factors
    model = _copy(m0)
    with Session(p['Y'], model, missing=missing, period_Lag=2, lambdaLagL1=l1, **synth.HYPER) as s:
        s.run(6).download()
        stats = s.lag_stats()
    G, b = L.gram_rhs(model.W, lags)
    Gabs, babs = L.gram_rhs(model.W, lags, absolute=True)
    d = dict(G=G, b=b, Gabs=Gabs, babs=babs, lam=synth.HYPER['lambdaLag'], T=model.W.shape[0], lags=lags)
    B = _bounds(d, model.lag_val, stats, dtype, th0=m0.lag_val.astype(np.float64))
    dims = [t for t in range(model.k) if not stats['per_dim'][t, 2]]
    print('capped dimensions: %d of %d; sweeps %s' % (stats['capped'], model.k, stats['per_dim'][:, 0].tolist()))
    _assert_kkt(G, b, d['lam'], l1, model.lag_val, B, dims, 'ALS %s missing=%d' % (np.dtype(dtype).name, missing))
    assert [len(s_) for s_ in model.selected_lags()] == stats['per_dim'][:, 1].tolist()


# ---- 8. two ranks on one device ------------------------------------------------------------------------------------------------------------
def test_two_ranks_give_the_bits_of_one(monkeypatch):
    from dist_worker import _problem
    p, m0 = _problem('c4')
    dtype = np.float32
    Y = p['Y'].astype(dtype)
    _, b0 = L.gram_rhs(m0.W.astype(dtype), p['lag_set'])
    l1 = 0.05 * float(np.median(np.abs(b0).max(axis=1)))

    def run():
        model = make_model(m0.W.astype(dtype), m0.H.astype(dtype), np.asfortranarray(m0.lag_val.astype(dtype)), p['lag_set'])
        with Session(Y, model, missing=True, lambdaLagL1=l1, lag_refit=True, **synth.HYPER) as s:
            s.run(4).download()
            return model, s.lag_stats(), s.describe()

    monkeypatch.delenv('TRMF_DEVICES', raising=False)
    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one, s1, d1 = run()
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two, s2, d2 = run()
    assert '1 rank' in d1 and '2 ranks' in d2 and 'lasso' in d1 and 'lasso' in d2
    assert np.array_equal(one.lag_val, two.lag_val) and np.array_equal(one.W, two.W) and np.array_equal(one.H, two.H)
    assert np.array_equal(s1['per_dim'], s2['per_dim']) and s1['capped'] == s2['capped'] and s1['refit_skipped'] == s2['refit_skipped']
    assert s1['per_dim'][:, 0].all()                                        # a lasso solve did run


# ---- 9. front end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('missing', [True, False])
def test_train_with_l1_is_the_session_path(missing):
    dtype = np.float64
    p, m0 = _train_problem(dtype, missing)
    a, b, c = _copy(m0), _copy(m0), _copy(m0)
    kw = dict(max_iter=4, missing=missing, lambdaLagL1=2.0, lag_refit=True, **synth.HYPER)
    trmf.train(p['Y'], a, **kw)
    b.fit(p['Y'], **kw)
    with Session(p['Y'], c, missing=missing, log_norms=False, timing=0, lambdaLagL1=2.0, lag_refit=True, **synth.HYPER) as s:
        s.run(4).download()
    for f in ('W', 'H', 'lag_val'):
        assert np.array_equal(getattr(a, f), getattr(c, f)) and np.array_equal(getattr(b, f), getattr(c, f)), f
    assert not np.array_equal(a.lag_val, m0.lag_val)


def test_rolling_validate_with_l1_on_every_path():
    pd = synth.dense_problem(12, 150, 3, [1, 2, 5], dtype=np.float64, seed=2)
    kw = dict(k=3, window_size=8, nr_windows=3, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=4, threads=2, seed=0, missing=True,
              lambdaLagL1=1.0, lag_refit=True)
    host = trmf.rolling_validate(pd['Y'], [1, 2, 5], forecast_on_device=False, **kw)
    dev = trmf.rolling_validate(pd['Y'], [1, 2, 5], forecast_on_device=True, **kw)
    fresh = trmf.rolling_validate(pd['Y'], [1, 2, 5], resident=False, **kw)
    assert np.allclose(fields(dev), fields(host), rtol=1e-7)               # tests/test_gpu_forecast.py's tolerance
    assert np.allclose(fields(fresh), fields(host), rtol=1e-7)
    results, best = trmf.grid_search(pd['Y'], [1, 2, 5], {'lambdaLagL1': [0.0, 1.0]}, **dict(kw, lag_refit=False))
    assert [r['kws']['lambdaLagL1'] for r in results] == [0.0, 1.0]
    assert np.array_equal(fields(results[0]['metrics']), fields(trmf.rolling_validate(pd['Y'], [1, 2, 5], **dict(kw, lambdaLagL1=0.0, lag_refit=False))))


def test_grid_impute_with_l1_matches_fresh_sessions():
    full = synth.imputation_problem(30, 400, 4, [1, 2, 5], observed=1.0, dtype=np.float32, seed=0)['Y'].toarray()
    mask = np.random.RandomState(1).rand(*full.shape) < 0.8
    grid = {'lambdaLagL1': [0.0, 0.5, 5.0], 'lambdaAR': [50.0, 5.0]}
    results, _, _ = trmf.grid_impute(full, mask, [1, 2, 5], grid, k=4, max_iter=4, seed=0, lag_refit=True)
    assert len(results) == 6
    for r in results:
        kws = r['kws']
        _, m, _ = trmf.impute(full, mask, [1, 2, 5], k=4, lambdaI=kws['lambdaI'], lambdaAR=kws['lambdaAR'], lambdaLag=kws['lambdaLag'],
                              max_iter=4, seed=0, lambdaLagL1=kws['lambdaLagL1'], lag_refit=True)
        assert m == r['metrics'], kws


@pytest.mark.parametrize('devices', [None, '0,0'])
def test_rejected_penalty_leaves_the_session_usable(devices, monkeypatch):
    if devices:
        monkeypatch.setenv('TRMF_DEVICES', devices)
    d = _inputs('lags24', np.float32)
    sess, model = _open(d)
    with sess:
        sess.set_lag_penalty(d['l1'], False)
        for bad in (float('nan'), -1.0, float('inf')):
            assert sess.lib.trmf_session_set_lag_penalty(sess.handle, bad, 0) == -1
            assert 'lambdaLagL1' in sess.lib.trmf_last_error().decode()
            with pytest.raises(RuntimeError):
                sess.set_lag_penalty(bad)
        assert 'lag penalty: lasso' in sess.describe()                      # the earlier setting stands
        sess.solve_lags()
        assert sess.lag_stats()['per_dim'][:, 0].all()
        sess.run(2).download()
    assert np.all(np.isfinite(model.W)) and np.all(np.isfinite(model.lag_val))
