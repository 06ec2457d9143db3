"""Host (no GPU): online loading updates -- trmf.online.series_ridge (the direct weighted ridge, the specification of
trmf_session_adapt_series), its recursive twin trmf.online.SeriesStats (recursive least squares with forgetting, the form the device
keeps resident) and Model.assimilate(adapt=True)."""
import numpy as np
import pytest

import adapt_helpers as AH
import online_helpers as OH
from helpers import make_model, relmax
from trmf import SeriesStats, filter_rows, series_ridge

RECURSION_TOL = 1e-12          # fp64 recursion against the fp64 direct solve, relmax (measured on this input set: <= 5.5e-13)


@pytest.mark.parametrize('gamma', [1.0, 0.95])
@pytest.mark.parametrize('lamI', [0.5, 1e-2])
@pytest.mark.parametrize('k', OH.RANKS)
def test_the_recursion_equals_the_direct_ridge_in_fp64(k, lamI, gamma):
    """Measured (relmax, this input set): <= 1.8e-14 for lambdaI = 0.5; for lambdaI = 1e-2  k <= 16: <= 2.5e-14,  k = 40: 1.3e-13 /
    1.9e-13 (gamma 1 / 0.95),  k = 64: 5.5e-13 / 3.2e-13.  At k = 64 a series has ~29 entries for 64 unknowns, so the ridge alone
    conditions 35 directions and a last-bit difference in S is amplified by 1 / lambdaI; there the solver matters: with two
    triangular solves after the Cholesky factorisation the same tables give 1.5e-12 (entry-by-entry sums) .. 1.8e-12 (block sums),
    with LAPACK's general solve (trmf.online._ridge_solve) 5.5e-13."""
    W = OH.inputs(k)['W']
    got = AH.recursive(W, k, np.float64, gamma).solve(lamI)
    want = AH.direct(W, k, lamI, gamma)
    print('k=%d lambdaI=%g gamma=%g: recursion vs direct %.3e' % (k, lamI, gamma, relmax(got, want)))
    assert relmax(got, want) <= RECURSION_TOL


@pytest.mark.parametrize('missing,storage', [(True, 'sparse'), (False, 'sparse'), (False, 'dense')], ids=['observed', 'sparse-full', 'dense-full'])
def test_without_forgetting_init_plus_blocks_equals_init_on_the_grown_matrix(missing, storage):
    k = 16
    W = OH.inputs(k)['W'].astype(np.float64)
    grown = AH.recursive(W, k, np.float64, 1.0, missing, storage)
    whole = SeriesStats(W, AH.training(k, 0, OH.T, np.float64, storage), 1.0, missing)
    assert grown.rows == whole.rows == OH.T
    assert relmax(grown.S, whole.S) <= 1e-13 and relmax(grown.r, whole.r) <= 1e-13
    assert relmax(grown.solve(0.5), AH.direct(W, k, 0.5, 1.0, missing, storage)) <= RECURSION_TOL


@pytest.mark.parametrize('gamma', [1.0, 0.95])
def test_the_designed_series(gamma):
    k, lamI = 7, 0.5
    W = OH.inputs(k)['W'].astype(np.float64)
    H = AH.recursive(W, k, np.float64, gamma).solve(lamI)
    om = gamma ** (OH.T - 1 - np.arange(OH.T))
    r, c, v = AH.entries(k)
    assert not H[AH.NO_ENTRY].any()                                                     # no entry: r = 0, the ridge makes the system regular
    for j in (AH.ONE_OLD, AH.LATE_ONLY, AH.TWICE):                                      # from the entry list, one term per stored entry
        e = np.flatnonzero(c == j)
        S = sum(om[r[i]] * np.outer(W[r[i]], W[r[i]]) for i in e)
        rhs = sum(om[r[i]] * float(v[i]) * W[r[i]] for i in e)
        assert relmax(H[j], np.linalg.solve(S + lamI * np.eye(k), rhs)) <= 1e-12, j
    assert np.count_nonzero(c == AH.ONE_OLD) == 1 and r[c == AH.ONE_OLD][0] < OH.FIRST
    assert r[c == AH.LATE_ONLY].min() >= AH.MID
    # the doubled cell is two observations: another answer than the cell stored once with the sum of the two values
    once = AH.csc_of(k, 0, OH.T, np.float64).copy()
    once.sum_duplicates()
    assert relmax(series_ridge(W, once, lamI, gamma)[AH.TWICE], H[AH.TWICE]) > 1e-6


def test_refusals():
    k = 7
    W = OH.inputs(k)['W'].astype(np.float64)
    Y = AH.csc_of(k, 0, OH.T, np.float64)
    for bad in (0.0, 1.5, -0.1, float('nan')):
        with pytest.raises(ValueError, match='forget'):
            series_ridge(W, Y, 0.5, bad)
        with pytest.raises(ValueError, match='forget'):
            SeriesStats(W, Y, bad)
    # no ridge: the series without an entry is the smallest under-determined one (the single-entry series follows it)
    with pytest.raises(ValueError, match='series %d' % AH.NO_ENTRY):
        series_ridge(W, Y, 0.0)
    with pytest.raises(ValueError, match='series %d' % AH.NO_ENTRY):
        SeriesStats(W, Y).solve(0.0)
    with pytest.raises(ValueError, match='rows'):
        series_ridge(W[:-1], Y, 0.5)
    st = SeriesStats(W[:OH.FIRST], Y[:OH.FIRST])
    with pytest.raises(ValueError, match='absorb'):
        st.absorb(W, Y[OH.FIRST:OH.FIRST + 3])                                          # 24 new rows of W, 3 of Y
    with pytest.raises(ValueError, match='absorb'):
        st.absorb(W[:, :k - 1], Y[OH.FIRST:])
    with pytest.raises(ValueError, match='absorb'):
        st.absorb(W, Y[OH.FIRST:, :OH.N - 1])
    assert st.rows == OH.FIRST                                                          # a refused block leaves the statistics as they were


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('missing', [True, False], ids=['observed', 'full'])
def test_model_assimilate_with_adapt_equals_filter_then_series_ridge(dtype, missing):
    k, lamI, lamAR, gamma = 16, 0.5, 50.0, 0.95
    d = OH.inputs(k)
    head, tail = AH.csc_of(k, 0, OH.FIRST, dtype).tocsr(), AH.csc_of(k, OH.FIRST, OH.T, dtype).tocsr()
    m = make_model(d['W'][:OH.FIRST].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    with pytest.raises(ValueError, match='init_series_stats'):
        m.assimilate(tail, lamI, lamAR, missing=missing, adapt=True, forget=gamma)
    m.init_series_stats(head, gamma, missing)
    H0 = m.H.copy()
    with pytest.raises(ValueError, match='forget'):
        m.assimilate(tail, lamI, lamAR, missing=missing, adapt=True, forget=1.0)
    out = m.assimilate(tail, lamI, lamAR, missing=missing, adapt=True, forget=gamma)
    assert np.array_equal(m.H, H0) and m.series_stats.rows == OH.FIRST and out.series_stats.rows == OH.T       # this model is left untouched
    grown = np.zeros((OH.T, k), dtype=dtype)
    grown[:OH.FIRST] = m.W
    Wf = filter_rows(grown, m.H, m.lag_set, m.lag_val, tail, OH.FIRST, lamI, lamAR, missing)
    assert np.array_equal(out.W, Wf)                                                    # the filter first, with the OLD loadings
    want = AH.direct(Wf, k, lamI, gamma, missing)
    tol = 1e-12 if dtype == np.float64 else OH.GATE * AH.yardstick(Wf, k, lamI, gamma, missing)[1]
    assert relmax(out.H, want) <= tol
    plain = m.assimilate(tail, lamI, lamAR, missing=missing)
    assert np.array_equal(plain.H, m.H) and np.array_equal(plain.W, Wf)                 # the default: today's behaviour
