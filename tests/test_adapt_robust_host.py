"""Host (no GPU): robust online loading updates -- trmf.online.SeriesStats.absorb_robust (the NumPy statement of
trmf_session_adapt_series_robust), trmf.robust_series_objective and Model.assimilate(adapt=True, robust_c=, adapt_robust=True)."""
import copy

import numpy as np
import pytest

import adapt_helpers as AH
import adapt_robust_helpers as ARH
import online_helpers as OH
import robust_helpers as RH
from helpers import make_model
from trmf import SeriesStats, robust_filter_rows, robust_series_objective

MATRIX = [(k, lamI, gamma) for k in OH.RANKS for lamI, gamma in AH.CASES]
IDS = ['k%d-lamI%g-gamma%g' % c for c in MATRIX]


@pytest.mark.parametrize('k,lamI,gamma', MATRIX, ids=IDS)
def test_every_case_exercises_both_branches_and_the_objective_never_rises(k, lamI, gamma):
    """Measured on these cases (c = 1.5, 4 sweeps): 10 - 31 % of a block's entries down-weighted in the last sweep, the smallest
    margin of an entry to its threshold 4.5e-4 (relative; k = 7, gamma = 0.95, second block)."""
    for b, y in enumerate(ARH.host_sequence(k, lamI, gamma)):
        down, border = ARH.exercised(y)
        print('k=%d lambdaI=%g gamma=%g block %d: %.1f %% down-weighted, %.2f %% borderline, fp32 statement: H %.2e weights %.2e'
              % (k, lamI, gamma, b, 100 * down, 100 * border, y['dev_H'], y['dev_weights']))
        assert 0.03 <= down <= 0.97 and border <= 0.01
        W64, Y64, before = y['W'].astype(np.float64), ARH.cast(y['Ynew'], np.float64), y['before']
        H = y['Hin'].astype(np.float64)
        J = [robust_series_objective(before, W64, Y64, H, lamI, y['scale'], ARH.C)]
        for s in range(1, ARH.SWEEPS + 1):
            H = copy.deepcopy(before).absorb_robust(W64, Y64, y['Hin'].astype(np.float64), lamI, y['scale'], ARH.C, s)[0]
            J.append(robust_series_objective(before, W64, Y64, H, lamI, y['scale'], ARH.C))
            assert J[-1] <= J[-2] + 1e-9 * abs(J[-2]), (s, J)
        assert np.array_equal(H, y['H64']) and J[-1] < J[0]


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('k,lamI,gamma', MATRIX, ids=IDS)
def test_an_infinite_c_is_absorb_and_solve_bit_for_bit(k, lamI, gamma, dtype):
    d = OH.inputs(k)
    W = d['W'].astype(dtype)
    plain = SeriesStats(W[:OH.FIRST], AH.csc_of(k, 0, OH.FIRST, dtype), gamma)
    robust = copy.deepcopy(plain)
    H = d['H'].astype(dtype)
    for lo, hi in ARH.BLOCKS:
        Ynew = AH.csc_of(k, lo, hi, dtype)
        want = plain.absorb(W[:hi], Ynew).solve(lamI)
        H, wts = robust.absorb_robust(W[:hi], Ynew, H, lamI, 1.0, float('inf'), 3)
        assert np.array_equal(H, want) and np.array_equal(robust.S, plain.S) and np.array_equal(robust.r, plain.r) and robust.rows == plain.rows == hi
        assert (wts.data == 1).all() and wts.nnz == Ynew.nnz and wts.shape == (hi - lo, OH.N)
        assert np.array_equal(robust.solve(lamI), H)                          # the invariant h = (S + lambdaI I)^-1 r of the committed tables


SEEDS = (0, 1, 2, 3, 4)


@pytest.mark.parametrize('gamma', [1.0, 0.95])
@pytest.mark.parametrize('seed', SEEDS)
def test_spikes_are_kept_out_of_the_loadings(seed, gamma):
    """||H_robust - H_clean|| <= 0.25 ||H_plain - H_clean|| on robust_helpers.spiked_panel(200, 30, 4, [1, 2, 5], 40, 0.5, seed): 3 % of
    the new cells spiked by +-40 sigma, a clean history, lambdaI = 0.5, c = 3, scale sigma, 4 sweeps.  Measured: 0.071 - 0.091."""
    lamI, sigma = 0.5, 0.5
    W, H, lag_set, lag_val, clean, spiked, first, hit = RH.spiked_panel(200, 30, 4, [1, 2, 5], 40, 0.5, seed)
    W = np.ascontiguousarray(W, dtype=np.float64)
    base = SeriesStats(W[:first], _history(seed, first), gamma)
    H0 = np.ascontiguousarray(H, dtype=np.float64)                             # the loadings the session holds: the panel's own
    Hclean = copy.deepcopy(base).absorb(W, clean.tocsc()).solve(lamI)
    Hplain = copy.deepcopy(base).absorb(W, spiked.tocsc()).solve(lamI)
    Hrobust, wts = copy.deepcopy(base).absorb_robust(W, spiked.tocsc(), H0, lamI, sigma, 3.0, 4)
    ratio = np.linalg.norm(Hrobust - Hclean) / np.linalg.norm(Hplain - Hclean)
    print('seed %d gamma %g: ||H_robust - H_clean|| / ||H_plain - H_clean|| = %.3f; %d of %d spiked cells down-weighted'
          % (seed, gamma, ratio, int((wts.toarray()[hit.toarray() > 0] < 1).sum()), int((hit.toarray() > 0).sum())))
    assert ratio <= 0.25
    assert (wts.toarray()[hit.toarray() > 0] < 1).all()


def _history(seed, first, observed=0.5, sigma=0.5):
    """The clean history of the spiked panel: the panel's own rows before the new block with the panel's own noise (the first draw
    of robust_helpers.spiked_panel's generator) on `observed` of the cells."""
    import scipy.sparse as smat
    from trmf import Model
    g = Model.syn_gen(200, 30, 4, [1, 2, 5], seed=seed, dtype=np.float64)
    Y = (g['Y'] + sigma * np.random.RandomState(seed + 1).randn(200, 30))[:first]
    mask = np.random.RandomState(seed + 2).rand(first, 30) < observed
    rows, cols = np.nonzero(mask)
    return smat.csc_matrix((Y[rows, cols], (rows, cols)), shape=Y.shape)


def test_the_designed_series():
    k, lamI, gamma = 7, 0.5, 0.95
    seq = ARH.host_sequence(k, lamI, gamma)
    for b, y in enumerate(seq):
        assert not y['H64'][AH.NO_ENTRY].any()                                 # no entry: r = 0, the ridge makes the system regular
        assert y['indptr'][AH.NO_ENTRY + 1] == y['indptr'][AH.NO_ENTRY]
    # the cell stored twice is two observations with a weight each: two values, two residuals
    y = seq[0]
    col = slice(y['indptr'][AH.TWICE], y['indptr'][AH.TWICE + 1])
    twice = np.flatnonzero(y['rows'][col] == AH.TWICE_ROW - OH.FIRST)
    assert twice.size == 2
    r, c, v = AH.entries(k)
    vals = v[(r == AH.TWICE_ROW) & (c == AH.TWICE)]
    assert vals.size == 2 and vals[0] != vals[1]
    # a series without a new entry keeps the plain solution of its decayed tables, whatever the sweep count
    assert y['indptr'][AH.ONE_OLD + 1] == y['indptr'][AH.ONE_OLD]
    plain = copy.deepcopy(y['before']).absorb(y['W'].astype(np.float64), ARH.cast(y['Ynew'], np.float64)).solve(lamI)
    assert np.array_equal(y['H64'][AH.ONE_OLD], plain[AH.ONE_OLD])
    # a series whose entries all lie within the threshold has the plain update's row
    full = np.flatnonzero([(y['om64'][y['indptr'][j]:y['indptr'][j + 1]] == 1).all() for j in range(OH.N)])
    assert full.size and all(np.array_equal(y['H64'][j], plain[j]) for j in full)


def test_refusals():
    k = 7
    d = OH.inputs(k)
    W, H = d['W'].astype(np.float64), d['H'].astype(np.float64)
    Y = AH.csc_of(k, 0, OH.T, np.float64)
    st = SeriesStats(W[:OH.FIRST], Y[:OH.FIRST])
    S0, r0 = st.S.copy(), st.r.copy()
    ok = dict(W=W, Ynew=Y[OH.FIRST:], H=H, lambdaI=0.5, scale=1.0)
    for bad, match in ((dict(c=0.0), 'c must be positive'), (dict(c=-1.0), 'c must be positive'), (dict(c=float('nan')), 'c must be positive'),
                       (dict(sweeps=0), 'sweeps'), (dict(scale=0.0), 'scale'), (dict(scale=-1.0), 'scale'), (dict(scale=float('nan')), 'scale'),
                       (dict(scale=float('inf')), 'scale'), (dict(scale=np.ones(OH.N - 1)), 'scale'), (dict(Ynew=Y[OH.FIRST:OH.FIRST + 3]), 'absorb_robust'),
                       (dict(W=W[:, :k - 1]), 'absorb_robust'), (dict(H=H[:-1]), 'absorb_robust'), (dict(lambdaI=0.0), 'series %d' % AH.NO_ENTRY)):
        with pytest.raises(ValueError, match=match):
            st.absorb_robust(**dict(ok, **bad))
        if 'sweeps' not in bad and 'lambdaI' not in bad:                       # the objective has the same guards
            with pytest.raises(ValueError, match=match.replace('absorb_robust', 'robust_series_objective')):
                robust_series_objective(st, **dict(ok, **bad))
        assert st.rows == OH.FIRST and np.array_equal(st.S, S0) and np.array_equal(st.r, r0)       # a refused block leaves the statistics as they were
    shared = SeriesStats(W[:OH.FIRST], Y[:OH.FIRST], 1.0, False)               # the full-observation form keeps one shared S
    with pytest.raises(ValueError, match='shared S'):
        shared.absorb_robust(**ok)
    with pytest.raises(ValueError, match='shared S'):
        robust_series_objective(shared, **ok)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_model_assimilate_with_adapt_robust(dtype):
    k, lamI, lamAR, gamma, scale = 16, 0.5, 50.0, 0.95, 0.2
    d = OH.inputs(k)
    head, tail = AH.csc_of(k, 0, OH.FIRST, dtype).tocsr(), AH.csc_of(k, OH.FIRST, OH.T, dtype).tocsr()
    m = make_model(d['W'][:OH.FIRST].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    m.init_series_stats(head, gamma, True)
    H0 = m.H.copy()
    for bad in (dict(adapt=True), dict(robust_c=2.0, scale=scale)):
        with pytest.raises(ValueError, match='adapt_robust'):
            m.assimilate(tail, lamI, lamAR, adapt_robust=True, forget=gamma, **bad)
    out = m.assimilate(tail, lamI, lamAR, robust_c=2.0, robust_sweeps=3, scale=scale, adapt=True, forget=gamma, adapt_robust=True)
    assert np.array_equal(m.H, H0) and m.series_stats.rows == OH.FIRST and out.series_stats.rows == OH.T       # this model is left untouched
    grown = np.zeros((OH.T, k), dtype=dtype)
    grown[:OH.FIRST] = m.W
    Wf, om = robust_filter_rows(grown, m.H, m.lag_set, m.lag_val, tail, OH.FIRST, lamI, lamAR, True, scale, 2.0, 3)
    assert np.array_equal(out.W, Wf) and np.array_equal(out.robust_weights, om)      # the robust filter first, with the OLD loadings
    want, wts = copy.deepcopy(m.series_stats).absorb_robust(Wf, tail, m.H, lamI, scale, 2.0, 3)
    assert np.array_equal(out.H, want) and np.array_equal(out.adapt_weights.data, wts.data) and 0 < (wts.data < 1).sum() < wts.nnz
    assert np.array_equal(out.series_stats.solve(lamI), out.H)
    # without the flag: the unweighted update under robust_c, as before
    plain = m.assimilate(tail, lamI, lamAR, robust_c=2.0, robust_sweeps=3, scale=scale, adapt=True, forget=gamma)
    assert np.array_equal(plain.W, Wf) and np.array_equal(plain.H, copy.deepcopy(m.series_stats).absorb(Wf, tail).solve(lamI))
    assert not hasattr(plain, 'adapt_weights') and not np.array_equal(plain.H, out.H)
