"""CPU: the sparse lag weights (L1-penalised Theta-solve) up to the device boundary -- exported symbols, the front end's argument
checks, Model.selected_lags, and the NumPy restatement of tests/lag_helpers.py against its own optimality conditions on the
designed inputs the GPU tests use.  No compute is launched here."""
import os
import re

import numpy as np
import pytest

import lag_helpers as L
import trmf
from helpers import make_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES, designed = L.SHAPES, L.designed


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_libraries_export_the_lag_penalty_entry_points(dtype):
    from trmf import session
    lib = session.lib_for(dtype)
    for name in ('trmf_session_set_lag_penalty', 'trmf_session_solve_lags', 'trmf_session_lag_stats'):
        assert hasattr(lib, name), name
    assert lib.trmf_session_set_lag_penalty.argtypes is not None           # prototyped by session.bind


def test_helper_constants_are_the_headers():
    text = open(os.path.join(ROOT, 'exp-trmf-nips16_amd', 'csrc', 'theta_kernels.hpp')).read()
    eps = [float(v) for v in re.findall(r'constexpr double kLassoEps = ([0-9.e+-]+);', text)]
    assert eps == [L.LASSO_EPS['float32'], L.LASSO_EPS['float64']]           # the TRMF_F32 branch first
    assert int(re.search(r'constexpr int kLassoMaxSweeps = (\d+);', text).group(1)) == L.LASSO_MAX_SWEEPS


def test_gram_rhs_is_the_lagged_inner_product():
    rng = np.random.default_rng(3)
    W = rng.standard_normal((40, 2))
    lags = [1, 3, 7]
    G, b = L.gram_rhs(W, lags)
    for t in range(2):
        for a, la in enumerate(lags):
            assert np.isclose(b[t, a], sum(W[i, t] * W[i - la, t] for i in range(7, 40)), rtol=1e-13)
            for c, lc in enumerate(lags):
                assert np.isclose(G[t, a, c], sum(W[i - la, t] * W[i - lc, t] for i in range(7, 40)), rtol=1e-13)
    Ga, ba = L.gram_rhs(W, lags, absolute=True)
    assert np.all(Ga >= np.abs(G) - 1e-12) and np.all(ba >= np.abs(b) - 1e-12)
    G32, _ = L.gram_rhs(W.astype(np.float32), lags)                           # products rounded to the element type, sums in fp64
    want = (W.astype(np.float32)[7 - 1:40 - 1, 0] * W.astype(np.float32)[7 - 3:40 - 3, 0]).astype(np.float64).sum()
    assert G32[0, 0, 1] == want


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_restatement_satisfies_its_own_kkt_conditions(name):
    d = designed(name, np.float64)
    np.random.seed(0)
    th0 = np.random.randn(len(d['lags']), d['k'])
    Gabs, babs = L.gram_rhs(d['W'], d['lags'], absolute=True)
    sweeps, unclear, total = [], 0, 0
    for t in range(d['k']):
        th, s = L.lasso_cd(d['G'][t], d['b'][t], d['lam'], d['l1'], th0[:, t])
        g, res = L.kkt(d['G'][t], d['b'][t], d['lam'], d['l1'], th)
        # stopped at delta <= 1e-13 = kLassoEps of the fp64 library: the bound the device is held to, with fp64 as the element type
        assert np.all(res <= L.kkt_bound(d['G'][t], d['b'][t], Gabs[t], babs[t], d['lam'], th, th0[:, t], d['T'] - max(d['lags']), s, np.float64))
        zero = th == 0
        unclear += int(np.sum(zero & (np.abs(g) > 0.98 * d['l1']))) + int(np.sum(~zero & (np.abs(th) < 1e-3)))
        total += len(th)
        sweeps.append(s)
        assert {1, 24} <= set(np.asarray(d['lags'])[~zero])               # the true lags are always found
        ref, _ = L.refit(d['G'][t], d['b'][t], d['lam'], th)
        assert np.all(ref[zero] == 0) and np.all(ref[~zero] != 0)
    assert max(sweeps) <= 100 < L.LASSO_MAX_SWEEPS                         # far from the device's cap
    assert unclear <= 0.1 * total


def test_full_shrinkage_of_the_restatement_is_exact_zero():
    d = designed('lags24', np.float64)
    big = 1.25 * float(np.abs(d['b']).max())
    th, _ = L.lasso_cd(d['G'][0], d['b'][0], d['lam'], big, np.ones(24))
    assert np.all(th == 0)


def _model(k=3, lags=(1, 2, 5)):
    rng = np.random.RandomState(0)
    return make_model(rng.rand(30, k), rng.rand(7, k), np.asfortranarray(rng.randn(len(lags), k)), list(lags))


def test_selected_lags():
    m = _model()
    m.lag_val[:] = np.array([[0.5, 0.0, -1e-4], [0.0, 0.0, 0.3], [-0.2, 0.0, 0.0]])
    got = m.selected_lags()
    assert [g.tolist() for g in got] == [[1, 5], [], [1, 2]]
    assert [g.tolist() for g in m.selected_lags(tol=1e-3)] == [[1, 5], [], [2]]
    assert all(g.dtype == np.uint32 for g in got)
    with pytest.raises(ValueError):
        m.selected_lags(tol=-1)


@pytest.mark.parametrize('bad', [-1.0, float('nan'), float('inf'), -1e-300])
def test_front_end_rejects_bad_weights_before_any_device_call(bad):
    from trmf.session import Session, check_lag_penalty
    m = _model()
    Y = np.random.RandomState(1).rand(30, 7)
    with pytest.raises(ValueError, match='lambdaLagL1'):
        check_lag_penalty(bad)
    with pytest.raises(ValueError, match='lambdaLagL1'):
        Session(Y, m, missing=False, lambdaLagL1=bad)                      # raised before the library is asked for a device
    with pytest.raises(ValueError, match='lambdaLagL1'):
        trmf.train(Y, m, lambdaLagL1=bad)
    with pytest.raises(ValueError, match='lambdaLagL1'):
        m.fit(Y, lambdaLagL1=bad)
    with pytest.raises(ValueError, match='lambdaLagL1'):
        trmf.rolling_validate(np.random.RandomState(2).rand(80, 7), [1, 2], k=2, window_size=4, nr_windows=2, lambdaLagL1=bad)
    with pytest.raises(ValueError, match='lambdaLagL1'):
        trmf.grid_impute(Y, Y > 0.2, [1, 2], {'lambdaLagL1': [0.1, bad]}, k=2)
    with pytest.raises(TypeError, match='lambdaLagL1'):
        check_lag_penalty('much')


def test_grid_impute_knows_the_new_keys():
    Y = np.random.RandomState(1).rand(30, 7)
    with pytest.raises(ValueError, match='cannot vary'):
        trmf.grid_impute(Y, Y > 0.2, [1, 2], {'lag_refit': [True, False]})        # a fixed setting, not a grid key


def test_check_lag_penalty_normalises_the_defaults():
    from trmf.session import check_lag_penalty
    assert check_lag_penalty(0) == (0.0, False)
    assert check_lag_penalty(np.float32(0.5), 1) == (0.5, True)
