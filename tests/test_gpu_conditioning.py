"""GPU (-m gpu): every solve on ill-conditioned and badly scaled problems ("Backward-error gates").

The rest of the suite feeds the solver unit-scale data, uniform start factors and ridge weights that keep cond_2 of the F-solve
systems at 1e2 ... 1e4, and gates forward errors; the arithmetic of the direct solves (the reciprocal square root behind the fp32
pivots, the Newton steps of the fp64 reciprocal, the pad column that carries the right-hand side) is almost unconstrained by that.
Here the systems reach cond_2 1e5 ... 1e10, where a forward error says nothing (the reference's own is 6e-3 ... 4e-2 in fp32), and
the gate is the BACKWARD error (tests/conditioning_helpers.py), which a sound factorisation keeps at about one unit roundoff:

  a. F-solve alone: the GPU's worst normwise eta over the item rows is at most 4 x the C restatement's worst eta, measured here on
     the same arrays in the same element type.  Row kernels, forced split, full observation; ranks 8 ... 80; both element types.
     The factor 4 is an argument, not a measurement: the fp32 kernel spends about three roundings per scaled element (a reciprocal
     square root good to 1 ulp, then a multiplication) where the reference spends one correctly rounded division.
  b. 2^p Y gives 2^p H bit for bit (p = +-20): A does not depend on y and every operation on the right-hand side is linear.
  c. Theta-solve alone on a smooth series (nearly collinear lagged copies), register form and forced LDS form, byte-equal to each
     other: 4 x the restatement's worst eta, with a floor of 2 u under the gate (the restatement sums the Gram in fp64 and sits
     near u / 3 in fp32; a reference that lands on the solution must not set an unreachable bar).
  d. A row whose factorisation breaks down does not touch its neighbours: bit-identical to a run without it, and inside gate a.
  e. Three iterations at ten hyper-parameter and data-scale extremes on every X-solve form and on the dense path, at the project's
     own parity gates (helpers.TOL, CG counts +-1, the measured fp32 noise floor where an fp32 run misses the direct gate).

tests/test_conditioning_host.py keeps the cases of a-d out of the breakdown regime (cond u <= 0.1, restatement eta <= 16 u)."""
import functools

import numpy as np
import pytest
import scipy.sparse as smat

import conditioning_helpers as C
import oracle_py as O
from helpers import TOL, assert_within_fp32_noise, evidence, fp32_noise_yardstick, make_model, relfro
from theta_helpers import lag_model
from trmf.session import Session

pytestmark = pytest.mark.gpu

BIG = C.BIG
MARGIN = 4.0
SPLIT_ENV = {'TRMF_LONG_ROW': '24', 'TRMF_LONG_CHUNK': '32'}
FORCED = ('TRMF_LONG_ROW', 'TRMF_LONG_CHUNK', 'TRMF_THETA_SOLVE', 'TRMF_PERSIST', 'TRMF_NO_HV_TILE', 'TRMF_TILE')


def _env(monkeypatch, env):
    for key in FORCED:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)


def _assert_fsolve_path(d, path, k):
    """describe() names the kernel family the case is about (tests/test_gpu_noncanonical.py _assert_path)."""
    assert ('split rows' in d) == (path == 'split'), d
    assert ('generic' in d) == (k > 64), d


def one_fsolve(Y, p, lam, dtype, missing=True):
    """One F-solve alone (periods (BIG, 1, BIG)) through the session; the untouched factors come back bit-equal."""
    W0, Th0 = p['W0'].astype(dtype), np.asfortranarray(p['Th0'].astype(dtype))
    model = make_model(W0, p['H0'].astype(dtype), Th0, p['lags'])
    with Session(Y, model, period_W=BIG, period_H=1, period_Lag=BIG, missing=missing, lambdaI=lam, lambdaAR=50.0, lambdaLag=0.5) as s:
        s.run(1)
        s.download()
        d = s.describe()
    assert np.array_equal(model.W, W0) and np.array_equal(model.lag_val, Th0)
    return model.H, d


def _gate(what, name, S, cond, X_gpu, X_ref, rows=None, floor=0.0):
    """Both sides' figures on record, then: the GPU's worst normwise eta <= max(MARGIN x the restatement's, floor)."""
    g, r = C.measure(S, X_gpu, rows), C.measure(S, X_ref, rows)
    u = C.U[name]
    evidence('conditioning %s %s: %s | %s | largest cond %.2e; GPU / restatement %.2f, GPU eta / u %.2f' % (
        what, name, C.line('GPU', g), C.line('restatement', r), cond.max(), g['eta'].max() / r['eta'].max(), g['eta'].max() / u))
    assert np.all(np.isfinite(np.asarray(X_gpu)[g['rows']]))
    assert g['eta'].max() <= max(MARGIN * r['eta'].max(), floor), (g['eta'].max(), r['eta'].max())


# ---- a. F-solve backward error -----------------------------------------------------------------------------------------------------
FSOLVE = C.fsolve_cases()


@pytest.mark.parametrize('name,k,path,scale,lam', FSOLVE, ids=['%s-k%d-%s-s%g-l%g' % c for c in FSOLVE])
def test_fsolve_backward_error(name, k, path, scale, lam, monkeypatch):
    dtype, full = np.dtype(name), path == 'full'
    _env(monkeypatch, SPLIT_ENV if path == 'split' else {})
    p = C.hard_case(k, scale, lam, full)
    Y = np.ascontiguousarray(p['Yd'].astype(dtype)) if full else p['Y'].astype(dtype)
    H, d = one_fsolve(Y, p, lam, dtype, missing=not full)
    _assert_fsolve_path(d, path, k)
    Href = C.restated_fsolve(p, lam, dtype, full)
    _gate('F-solve k=%d %s scale %g lambdaI %g' % (k, path, scale, lam), name, p['sys'], p['cond'], H, Href)


# ---- b. 2^p Y gives 2^p H bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['rows', 'split'])
@pytest.mark.parametrize('name', ['float32', 'float64'])
@pytest.mark.parametrize('k', [8, 40, 64])
def test_power_of_two_scaling_of_the_observations_is_exact(k, name, path, monkeypatch):
    dtype = np.dtype(name)
    _env(monkeypatch, SPLIT_ENV if path == 'split' else {})
    p = C.hard_case(k, 1.0, 0.5)
    H, d = one_fsolve(p['Y'].astype(dtype), p, 0.5, dtype)
    _assert_fsolve_path(d, path, k)
    assert np.all(np.isfinite(H)) and np.abs(H).max() > 0
    for e in (20, -20):
        f = dtype.type(2.0 ** e)
        Ys = p['Y'].astype(dtype) * f
        assert np.array_equal(Ys.data / f, p['Y'].data.astype(dtype))                      # the scaling itself is exact
        Hs, _ = one_fsolve(Ys, p, 0.5, dtype)
        differing = np.flatnonzero((Hs != H * f).any(axis=1))
        evidence('conditioning scaling k=%d %s %s: Y x 2^%d, rows of H that are not 2^%d H bit for bit: %d of %d%s' % (
            k, name, path, e, e, len(differing), len(H), '' if not len(differing) else ' (first %s, lengths %s)' % (
                differing[:8].tolist(), [p['lengths'][i] for i in differing[:8]])))
        assert np.array_equal(Hs, H * f)


# ---- c. Theta-solve backward error -------------------------------------------------------------------------------------------------
THETA = C.theta_cases()
REG_MAX = 32                                                               # kThetaRegMax of csrc/theta_kernels.hpp


def solve_lags(W, lags, lam):
    model = lag_model(W, 20, lags)
    with Session(C.theta_y(W.shape[0]).astype(W.dtype), model, missing=True, lambdaI=0.5, lambdaAR=50.0, lambdaLag=lam) as s:
        theta = s.solve_lags().download().lag_val.copy()
        d = s.describe()
    assert np.array_equal(model.W, W) and not np.any(model.H)                # the untouched factors
    return theta, d


@pytest.mark.parametrize('name,k,lagname,lam', THETA, ids=['%s-k%d-%s-l%g' % c for c in THETA])
def test_theta_solve_backward_error(name, k, lagname, lam, monkeypatch):
    c = C.theta_case(k, lagname, lam, name)
    W, lags = np.ascontiguousarray(c['W']), c['lags']
    _env(monkeypatch, {})
    reg, d_reg = solve_lags(W, lags, lam)
    _env(monkeypatch, {'TRMF_THETA_SOLVE': 'lds'})
    lds, d_lds = solve_lags(W, lags, lam)
    form = 'solve in LDS' if len(lags) > REG_MAX else 'solve in registers, class %d' % (8 if len(lags) <= 8 else 16 if len(lags) <= 16 else 32)
    assert form in d_reg and 'solve in LDS' in d_lds, (d_reg, d_lds)
    assert np.array_equal(reg, lds)
    ref = C.restated_theta(W, lags, lam)
    _gate('Theta-solve k=%d %s lambdaLag %g (%s)' % (k, lagname, lam, form), name, c['sys'], c['cond'], reg.T, ref.T, floor=2 * C.U[name])


# ---- d. a row that breaks down does not touch its neighbours -----------------------------------------------------------------------
@pytest.mark.parametrize('pos', range(4))
@pytest.mark.parametrize('k', C.BREAK_RANKS)
def test_a_row_that_breaks_down_leaves_its_neighbours_alone(k, pos, monkeypatch):
    _env(monkeypatch, {})
    p = C.breakdown_problem(k, pos)
    dtype = np.dtype('float32')
    H, d = one_fsolve(p['Y'], p, C.BREAK_LAM, dtype)
    Hb, _ = one_fsolve(p['Yb'], p, C.BREAK_LAM, dtype)
    _assert_fsolve_path(d, 'rows', k)
    deg, others = p['deg'], p['others']
    row = H[deg]
    held = 'non-finite values (%d NaN, %d Inf of %d)' % (np.isnan(row).sum(), np.isinf(row).sum(), k) if not np.all(np.isfinite(row)) else \
        'its unsolved right-hand side' if np.allclose(row, p['rhs'], rtol=1e-5, atol=0) else 'finite values, max |h| %.3g' % np.abs(row).max()
    evidence('conditioning breakdown k=%d, position %d of its quad: row %d holds %s' % (k, pos, deg, held))
    assert np.array_equal(H[others], Hb[others])
    Href = O.fsolve_port(smat.csr_matrix(p['Y'].T), p['W0'], p['H0'].copy(), C.BREAK_LAM)
    _gate('breakdown k=%d position %d, the other rows' % (k, pos), 'float32', p['sys'], p['cond'], H, Href, rows=others)


# ---- e. three iterations at the extremes -------------------------------------------------------------------------------------------
XPATHS = {'persist': {}, 'launch-per-step': {'TRMF_PERSIST': '0'}, 'unfused': {'TRMF_NO_HV_TILE': '1'}, 'dense': {}}
XFORM = {'persist': 'persistent', 'launch-per-step': 'one launch per CG step', 'unfused': 'X-solve unfused'}
# every case on every path once; the (element type, rank) pairs rotate so that each meets every path and most cases
EXTREME = [(case, path, C.EXT_RANKS[(i + j) % len(C.EXT_RANKS)]) for i, case in enumerate(C.EXTREMES) for j, path in enumerate(XPATHS)]


@functools.lru_cache(maxsize=None)
def _restated_iterations(case, name, k, dense):
    """Three iterations of the restatement, computed once per case and shared (read only)."""
    dtype = np.dtype(name)
    Y, hyper = C.extreme_problem(case, dtype, dense)
    W, H, Th = (a.astype(dtype) for a in C.extreme_start(k))
    Th = np.asfortranarray(Th)
    log = O.train_port(Y, C.EXT_LAGS, W, H, Th, hyper, max_iter=3, missing=not dense)
    for a in (W, H, Th):
        a.setflags(write=False)
    return W, H, Th, log


@pytest.mark.parametrize('case,path,rank', EXTREME, ids=['%s-%s-%s-k%d' % (c, p, r[0], r[1]) for c, p, r in EXTREME])
def test_three_iterations_at_the_extremes(case, path, rank, monkeypatch):
    name, k = rank
    dtype, dense = np.dtype(name), path == 'dense'
    _env(monkeypatch, XPATHS[path])
    Y, hyper = C.extreme_problem(case, dtype, dense)
    W0, H0, Th0 = (a.astype(dtype) for a in C.extreme_start(k))
    model = make_model(W0, H0, Th0, C.EXT_LAGS)
    with Session(Y, model, missing=not dense, **hyper) as s:
        s.run(3); st = s.stats(3); s.download(); d = s.describe()
    W, H, Th, log = _restated_iterations(case, name, k, dense)
    assert all(np.all(np.isfinite(a)) for a in (W, H, Th, model.W, model.H, model.lag_val))
    Yobj = C.all_cells(Y) if dense else Y
    Jo = O.objective(Yobj, C.EXT_LAGS, W, H, Th, hyper)
    Jp = O.objective(Yobj, C.EXT_LAGS, model.W, model.H, model.lag_val, hyper)
    tol = TOL[name]
    cg_o, cg_p = [l['cg_iter'] for l in log], [x['cg_iter'] for x in st]
    got = (relfro(model.W, W), relfro(model.H, H), relfro(model.lag_val, Th), abs(Jp - Jo) / abs(Jo))
    evidence('conditioning 3 iterations %s %s %s k=%d (%s): relfro W %.2e H %.2e Th %.2e (gate %.0e); J rel %.2e (gate %.0e); CG %s vs %s' % (
        case, path, name, k, d, got[0], got[1], got[2], tol['factor'], got[3], tol['objective'], cg_p, cg_o))
    assert 'split rows' not in d and 'generic' not in d, d
    if not dense:
        assert XFORM[path] in d and all(other not in d for key, other in XFORM.items() if key != path), d
    direct = got[3] < tol['objective'] and got[1] < tol['factor'] and got[0] < tol['factor'] and got[2] < 10 * tol['factor']
    if not direct:
        # fp32 only: the truncated CG's noise floor, measured on the reference side on the same inputs (helpers.fp32_noise_yardstick)
        assert name == 'float32' and not dense, got
        ys = fp32_noise_yardstick(Y, C.EXT_LAGS, W0, H0, Th0, hyper, 3)
        assert_within_fp32_noise(model, ys, C.EXT_LAGS, hyper, what='conditioning %s %s k=%d' % (case, path, k))
    assert all(abs(a - b) <= 1 for a, b in zip(cg_o, cg_p))
