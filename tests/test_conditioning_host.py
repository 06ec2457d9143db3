"""CPU: the conditions on the inputs of tests/test_gpu_conditioning.py, checked on the reference side.

For every case of the GPU tests of the direct solves the C restatement is run in the case's element type and must come back finite,
every system must satisfy cond_2(A) u <= 0.1 (u = 2^-24 / 2^-53), and the restatement's own worst normwise backward error must be at
most 16 u.  These are conditions that keep the cases out of the breakdown regime -- where no factorisation owes anybody an answer
-- not accuracy gates; the gate of the GPU tests is a multiple of the restatement's figure measured there.  The one row that is
built to break down is checked for exactly that: the restatement leaves it unsolved (posv's info is ignored, trmf.cpp:395) or
non-finite, and its neighbours are what they are without it."""
import math

import numpy as np
import pytest
import scipy.sparse as smat

import conditioning_helpers as C
import lag_helpers
import oracle_py as O
from helpers import evidence

COND_U, ETA_U = 0.1, 16.0


def _check(what, name, S, cond, X, rows=None):
    u = C.U[name]
    m = C.measure(S, X, rows)
    evidence('conditioning host %s %s: %s; cond %.2e (cond u %.3f); eta / u %.2f' % (what, name, C.line('restatement', m), cond.max(), cond.max() * u, m['eta'].max() / u))
    assert np.all(np.isfinite(np.asarray(X)[m['rows']]))
    assert cond.max() * u <= COND_U
    assert m['eta'].max() <= ETA_U * u
    return m


def test_backward_error_of_known_vectors():
    """The helper itself: an exact solution has eta = 0; a residual of known size gives the quotient by hand."""
    A = np.array([[4.0, 1.0], [1.0, 3.0]]); x = np.array([1.0, -2.0]); b = A.dot(x)
    assert C.backward_error(A, b, x) == (0.0, 0.0)
    norm, comp = C.backward_error(A, b + np.array([0.5, 0.0]), x)
    assert norm == 0.5 / (5.0 * 2.0 + 5.0)                                   # ||A||_inf = 5, ||x||_inf = 2, b = (2.5, -5)
    assert comp == 0.5 / (4.0 + 2.0 + 2.5)                                   # row 0: |A||x| = 4 + 2, |b| = 2.5
    assert C.backward_error(A, b, np.array([np.nan, 0.0])) == (float('inf'), float('inf'))


def test_exact_sum_is_the_correctly_rounded_sum():
    """Against math.fsum on 48-bit products spread over sixty binades; and where a plain fp64 sum in one order differs from it."""
    rs = np.random.RandomState(0)
    a, b = rs.randn(500, 7).astype(np.float32).astype(np.float64), (rs.randn(500, 7) * 2.0 ** rs.randint(-30, 30, (500, 7))).astype(np.float32).astype(np.float64)
    P = a * b
    want = np.array([math.fsum(P[:, j]) for j in range(7)])
    got = C.exact_sum(P)
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))            # the closing addition rounds once more, never twice
    plain = np.zeros(7)
    for row in P:
        plain += row
    assert np.any(plain != want)
    assert np.array_equal(C.exact_sum(np.zeros((3, 2))), np.zeros(2))


def test_theta_systems_are_the_sums_of_gram_rhs():
    """Same entries as lag_helpers.gram_rhs up to what its fp64 sums lose in their order (n u of the sum of |products|)."""
    for name in ('float32', 'float64'):
        c = C.theta_case(8, 'gap', 0.5, name)
        G, b = lag_helpers.gram_rhs(c['W'], c['lags'])
        S, n = c['sys'], c['sys']['lens'][0]
        u64 = C.U['float64']
        assert np.all(np.abs(S['A'] - 0.5 * np.eye(len(c['lags'])) - G) <= (n + 2) * u64 * S['Aabs'])
        assert np.all(np.abs(S['b'] - b) <= n * u64 * S['babs'])
        assert np.any(S['b'] != b) == (name == 'float64')                    # 24-bit products add exactly in fp64, 48-bit ones do not


FSOLVE = sorted({(name, k, 'full' if path == 'full' else 'rows', scale, lam) for name, k, path, scale, lam in C.fsolve_cases()})


@pytest.mark.parametrize('name,k,path,scale,lam', FSOLVE, ids=['%s-k%d-%s-s%g-l%g' % c for c in FSOLVE])
def test_fsolve_cases_are_within_reach(name, k, path, scale, lam):
    """The split path solves the systems of the row path, so the two share a case here."""
    full = path == 'full'
    p = C.hard_case(k, scale, lam, full)
    H = C.restated_fsolve(p, lam, np.dtype(name), full)
    _check('F-solve k=%d %s scale %g lambdaI %g' % (k, path, scale, lam), name, p['sys'], p['cond'], H)


THETA = C.theta_cases()


@pytest.mark.parametrize('name,k,lagname,lam', THETA, ids=['%s-k%d-%s-l%g' % c for c in THETA])
def test_theta_cases_are_within_reach(name, k, lagname, lam):
    c = C.theta_case(k, lagname, lam, name)
    Th = C.restated_theta(c['W'], c['lags'], lam)
    _check('Theta-solve k=%d %s lambdaLag %g' % (k, lagname, lam), name, c['sys'], c['cond'], Th.T)


@pytest.mark.parametrize('pos', range(4))
@pytest.mark.parametrize('k', C.BREAK_RANKS)
def test_the_breakdown_row_on_the_restatement(k, pos):
    p = C.breakdown_problem(k, pos)
    W0 = p['W0']
    H = O.fsolve_port(smat.csr_matrix(p['Y'].T), W0, p['H0'].copy(), C.BREAK_LAM)
    Hb = O.fsolve_port(smat.csr_matrix(p['Yb'].T), W0, p['H0'].copy(), C.BREAK_LAM)
    deg, others = p['deg'], p['others']
    assert np.linalg.matrix_rank(p['sys']['A'][deg] - C.BREAK_LAM * np.eye(k)) == 1
    assert np.float32(p['sys']['A'][deg].diagonal().min() + C.BREAK_LAM) == np.float32(p['sys']['A'][deg].diagonal().min())   # the ridge is below the rounding
    unsolved = np.all(np.isfinite(H[deg])) and np.allclose(H[deg], p['rhs'], rtol=1e-5, atol=0)
    evidence('conditioning host breakdown k=%d position %d: the restatement leaves row %d %s' % (
        k, pos, deg, 'unsolved (its right-hand side)' if unsolved else 'non-finite' if not np.all(np.isfinite(H[deg])) else 'finite and solved'))
    assert unsolved or not np.all(np.isfinite(H[deg]))
    assert np.array_equal(H[others], Hb[others])
    _check('breakdown k=%d position %d, the other rows' % (k, pos), 'float32', p['sys'], p['cond'], H, others)
