"""The ridge lag-weight solve after its two kernels were made short: theta_gram_kernel's sixteen-threads-per-block closing
reduction, and theta_solve_reg_kernel -- the |L| x |L| system in the registers of one wavefront for |L| <= kThetaRegMax = 32 --
beside theta_solve_kernel (LDS / global scratch), which stays for longer lag sets.

Inputs go in as a model's W (theta_helpers.lag_model) and come back as Session.solve_lags().download().lag_val (|L| x k: column t is
the Theta of latent dimension t); Y is any small sparse matrix.  Three properties, in both libraries:

  1. the register form gives the bytes of the LDS form (TRMF_TEST=1 TRMF_THETA_SOLVE=lds, read when a session is created,
     forces the latter; describe() names the form that runs, so the comparison cannot be between a form and itself unnoticed),
  2. every timestamp is counted once in every chunk / slice geometry: W holds small integers, so each product and each fp64 sum
     is exact in any order and Theta is held against numpy.linalg.solve in fp64 on lag_helpers.gram_rhs,
  3. the Theta of a latent dimension does not depend on the other dimensions of the model.

Tolerance of 2: 2e-4 (fp32) / 1e-9 (fp64) of max |Theta| -- what tests/test_oracle_golden.py asks of a factor.  The systems are
built to be well conditioned (cond_2 <= 100, asserted), and a CPU test below shows that a float32 Cholesky in NumPy of the same
systems stays inside the fp32 tolerance, so the bound asks nothing of the device that fp32 arithmetic cannot give."""
import functools

import numpy as np
import pytest
import scipy.sparse as smat

import lag_helpers as L
from helpers import relmax
from theta_helpers import lag_model
from trmf.session import Session

DTYPES = [np.float32, np.float64]
N_ITEMS = 20
GAPPED = (1, 2, 3, 7, 24)
REG_MAX = 32                                                               # kThetaRegMax of csrc/theta_kernels.hpp


def _consecutive(n):
    return tuple(range(1, n + 1))


def _open(W, lags, lam):
    """A session whose model carries W (copied) and a zero Theta; Y is a small sparse matrix of the right shape."""
    T, k = W.shape
    dtype = W.dtype.type
    Y = smat.random(T, N_ITEMS, density=0.2, random_state=np.random.RandomState(5), format='csr', dtype=np.float64).astype(dtype)
    model = lag_model(W, N_ITEMS, lags)
    return Session(Y, model, missing=True, lambdaI=0.5, lambdaAR=50.0, lambdaLag=lam), model


def _solve(W, lags, lam):
    sess, model = _open(W, lags, lam)
    with sess:
        theta = sess.solve_lags().download().lag_val.copy()
        desc = sess.describe()
    assert np.array_equal(model.W, W)                                       # solve_lags leaves W alone
    return theta, desc


def _form(lags):
    n = len(lags)
    return 'solve in LDS' if n > REG_MAX else 'solve in registers, class %d' % (8 if n <= 8 else 16 if n <= 16 else 32)


# ---- 1. the register form is byte-equal to the LDS form ---------------------------------------------------------------------------
FORM_LAGS = [_consecutive(n) for n in (1, 2, 5, 8, 16, 17, 31, 32)] + [GAPPED, _consecutive(REG_MAX + 1)]


@functools.lru_cache(maxsize=None)
def _ar_latent(T, k, dtype):
    """A noisy AR process (lag_helpers.ar_latent): neighbouring lags are correlated, so the factorisation has work to do."""
    W = L.ar_latent(T, k, np.random.default_rng(3)).astype(dtype)
    W.setflags(write=False)
    return W


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k', [1, 8, 40])
@pytest.mark.parametrize('lags', FORM_LAGS, ids=lambda l: 'gap' if l == GAPPED else 'L%d' % len(l))
def test_register_form_gives_the_bytes_of_the_lds_form(lags, k, dtype, monkeypatch):
    W = _ar_latent(max(lags) + 700, k, np.dtype(dtype).type)
    monkeypatch.delenv('TRMF_THETA_SOLVE', raising=False)
    dflt, d_dflt = _solve(W, lags, 0.5)
    monkeypatch.setenv('TRMF_THETA_SOLVE', 'lds')
    lds, d_lds = _solve(W, lags, 0.5)
    assert _form(lags) in d_dflt and 'solve in LDS' in d_lds, (d_dflt, d_lds)   # longer than the cap: the LDS form either way
    assert np.all(np.isfinite(lds)) and np.abs(lds).max() > 0
    assert np.array_equal(dflt, lds)


# ---- 2. every timestamp is counted once -------------------------------------------------------------------------------------------
COUNT_LAM = 4.0
COUNT_K = 5
COUNT_EXTRA = (1, 3, 511, 512, 513, 2 * 512 + 7)                            # T - midx; kThetaChunk = 512
COUNT_LAGS = [_consecutive(n) for n in (1, 4, 5, 16, 17)] + [GAPPED]
COUNT_CASES = [(lags, extra) for lags in COUNT_LAGS for extra in COUNT_EXTRA]
COUNT_TOL = {'float32': 2e-4, 'float64': 1e-9}


@functools.lru_cache(maxsize=None)
def _count_case(lags, extra):
    """Integer W in [-3, 3] (exact in either element type), the fp64 systems A = G + lambdaLag I, b and their solutions (k x |L|)."""
    T = max(lags) + extra
    W = np.random.RandomState(1000 * len(lags) + extra).randint(-3, 4, size=(T, COUNT_K)).astype(np.float64)
    G, b = L.gram_rhs(W, lags)
    A = G + COUNT_LAM * np.eye(len(lags))
    ref = np.stack([np.linalg.solve(A[t], b[t]) for t in range(COUNT_K)], axis=1)       # |L| x k
    for v in (W, A, b, ref):
        v.setflags(write=False)
    return W, A, b, ref


def test_counting_systems_are_within_reach_of_fp32():
    """CPU: cond_2(A) <= 100 for every system of test 2, and a float32 Cholesky solve in NumPy stays inside the fp32 tolerance."""
    worst_cond = worst_err = 0.0
    for lags, extra in COUNT_CASES:
        W, A, b, ref = _count_case(lags, extra)
        assert np.array_equal(W.astype(np.float32).astype(np.float64), W)
        got = np.empty_like(ref)
        for t in range(COUNT_K):
            worst_cond = max(worst_cond, float(np.linalg.cond(A[t])))
            A32, b32 = A[t].astype(np.float32), b[t].astype(np.float32)
            assert np.array_equal(A32.astype(np.float64), A[t]) and np.array_equal(b32.astype(np.float64), b[t])   # integers < 2^24
            R = np.linalg.cholesky(A32).T.astype(np.float32)
            z = np.zeros(len(lags), dtype=np.float32)
            for q in range(len(lags)):                                      # the substitutions in float32 as well
                z[q] = (b32[q] - np.float32(np.dot(R[:q, q], z[:q]))) / R[q, q]
            x = np.zeros(len(lags), dtype=np.float32)
            for q in range(len(lags) - 1, -1, -1):
                x[q] = (z[q] - np.float32(np.dot(R[q, q + 1:], x[q + 1:]))) / R[q, q]
            got[:, t] = x
        worst_err = max(worst_err, relmax(got, ref))
    print('counting systems: worst cond_2 %.3g, worst float32 Cholesky error %.3g of max |Theta|' % (worst_cond, worst_err))
    assert worst_cond <= 100.0
    assert worst_err < COUNT_TOL['float32']


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lags,extra', COUNT_CASES, ids=lambda v: ('gap' if v == GAPPED else 'L%d' % len(v)) if isinstance(v, tuple) else 'n%d' % v)
def test_every_timestamp_is_counted_once(lags, extra, dtype):
    W, A, b, ref = _count_case(lags, extra)
    theta, _ = _solve(W.astype(dtype), lags, COUNT_LAM)
    err = relmax(theta, ref)
    print('|L| %d, T - midx %d, %s: Theta off by %.3g of max |Theta|' % (len(lags), extra, np.dtype(dtype).name, err))
    assert err < COUNT_TOL[np.dtype(dtype).name]


# ---- 3. Theta of a dimension is independent of its neighbours ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lags', [_consecutive(16), GAPPED, _consecutive(REG_MAX + 1)], ids=['L16', 'gap', 'L33'])
def test_theta_of_a_dimension_is_independent_of_the_others(lags, dtype):
    """Dimension 7 of a k = 40 model against the same series as a k = 1 model: column 7 of the one lag_val (|L| x k) and the only
    column of the other hold the same bytes."""
    W = _ar_latent(max(lags) + 700, 40, np.dtype(dtype).type)
    full, d40 = _solve(W, lags, 0.5)
    alone, d1 = _solve(np.ascontiguousarray(W[:, 7:8]), lags, 0.5)
    assert _form(lags) in d40 and _form(lags) in d1
    assert full.shape == (len(lags), 40) and alone.shape == (len(lags), 1)
    assert np.array_equal(full[:, 7], alone[:, 0])
