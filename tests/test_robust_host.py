"""CPU: trmf.robust_filter_rows, the NumPy statement of the Huber-weighted forward filter (trmf_session_assimilate_robust), and
the input sets the device tests use (tests/robust_helpers.py)."""
import numpy as np
import pytest
import scipy.sparse as smat

import online_helpers as OH
import robust_helpers as RH
import trmf
from helpers import make_model, relmax
from trmf import filter_rows, robust_filter_rows

CASES_A = [(k, lamI, lamAR) for k in OH.RANKS for lamI, lamAR in OH.LAMBDAS]
CASES_B = [(k,) + OH.LAMBDAS[1] for k in RH.B_RANKS]


@pytest.mark.parametrize('case', [('a',) + c for c in CASES_A] + [('b',) + c for c in CASES_B], ids=lambda c: '%s-k%d-%g-%g' % c)
def test_the_input_sets_exercise_both_branches_of_the_weight(case):
    which, k, lamI, lamAR = case
    d, scale, y = (RH.case_a if which == 'a' else RH.case_b)(k, lamI, lamAR)
    down, border = RH.exercised(y)
    print('set %s k=%d lambdaI=%g lambdaAR=%g: scale %.4f, %.1f %% down-weighted, %.2f %% borderline, fp32 statement: rows %.2e weights %.2e, '
          'robust vs plain rows %.2e' % (which, k, lamI, lamAR, scale, 100 * down, 100 * border, y['dev_rows'], y['dev_weights'],
                                         relmax(y['w64'][d['first']:], OH.twin(d, np.float64, lamI, lamAR, True, d['first'])[d['first']:])))
    assert 0.03 <= down <= 0.97
    assert border <= 0.01
    # the two statements agree on which cells are down-weighted, the borderline ones apart
    agree = (y['om32'] < 1) == (y['om64'] < 1)
    assert agree[~y['border']].all()
    assert y['om64'].shape == (d['Y'][d['first']:].nnz,) and y['om64'].min() > 0 and y['om64'].max() == 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('k', [7, 40])
def test_an_infinite_c_is_the_plain_filter(k, dtype):
    lamI, lamAR = OH.LAMBDAS[1]
    d = OH.inputs(k)
    w64, dev32 = OH.yardstick(k, lamI, lamAR)
    W, om = RH.statement(d, dtype, lamI, lamAR, 1.0, c=np.inf, sweeps=3)
    assert np.all(om == 1)
    assert relmax(W[OH.FIRST:], w64[OH.FIRST:]) <= OH.bound(dtype, dev32)
    assert np.array_equal(W[:OH.FIRST], d['W'][:OH.FIRST].astype(dtype))


def _huber_objective(w, Hi, y, t, lamI, lamAR, prior):
    r = np.abs(y - Hi.dot(w))
    rho = np.where(r <= t, 0.5 * r * r, t * r - 0.5 * t * t)
    return rho.sum() + 0.5 * lamI * w.dot(w) + 0.5 * lamAR * (w - prior).dot(w - prior)


def test_the_huber_objective_never_increases_over_the_sweeps():
    k, (lamI, lamAR) = 16, OH.LAMBDAS[1]
    d, scale, _ = RH.case_a(k, lamI, lamAR)
    W, H, th = d['W'].astype(np.float64), d['H'].astype(np.float64), d['theta'].astype(np.float64)
    t = RH.C * scale
    worst = 0.0
    for i in range(OH.FIRST, OH.T):
        row = OH.rows_of(d['Y'], i, i + 1, np.float64)
        prior = OH.prior_of(W[:i + 1], i, d['lag_set'], th)
        prev = _huber_objective(prior, H[row.indices], row.data, t, lamI, lamAR, prior)
        for s in range(1, 13):
            w = robust_filter_rows(W[:i + 1], H, d['lag_set'], th, row, i, lamI, lamAR, True, scale, RH.C, s)[0][i]
            cur = _huber_objective(w, H[row.indices], row.data, t, lamI, lamAR, prior)
            worst = max(worst, (cur - prev) / max(abs(prev), 1e-300))
            prev = cur
    print('largest relative increase of a row objective over 12 sweeps: %.3e' % worst)
    assert worst <= 1e-12


PANELS = [dict(T=120, n=48, k=5, lags=(1, 2, 7), new_rows=12, observed=0.6, seed=11),
          dict(T=300, n=200, k=40, lags=(1, 2, 3, 24), new_rows=24, observed=0.5, seed=12)]


@pytest.mark.parametrize('panel', PANELS, ids=['120x48-k5', '300x200-k40'])
def test_spikes_bend_the_plain_filter_and_not_the_robust_one(panel):
    W, H, lag_set, lag_val, clean, spiked, first, hit = RH.spiked_panel(**panel)
    lamI, lamAR, sigma = 0.5, 2.0, 0.5
    ref = filter_rows(W, H, lag_set, lag_val, clean, first, lamI, lamAR, True)[first:]
    plain = filter_rows(W, H, lag_set, lag_val, spiked, first, lamI, lamAR, True)[first:]
    robust, om = robust_filter_rows(W, H, lag_set, lag_val, spiked, first, lamI, lamAR, True, sigma, 3.0, 4)
    e_plain = np.linalg.norm(plain - ref) / np.linalg.norm(ref)
    e_robust = np.linalg.norm(robust[first:] - ref) / np.linalg.norm(ref)
    flagged = om < 1
    print('spiked panel %dx%d k=%d: plain %.3f robust %.3f ratio %.3f; %d of %d spiked cells flagged, %d others' % (
        panel['T'], panel['n'], panel['k'], e_plain, e_robust, e_robust / e_plain, int((flagged & (hit.data > 0)).sum()), int((hit.data > 0).sum()),
        int((flagged & (hit.data == 0)).sum())))
    assert e_robust <= 0.5 * e_plain
    assert (flagged & (hit.data > 0)).sum() >= 0.9 * (hit.data > 0).sum()


def test_every_refusal_is_a_value_error():
    d = OH.inputs(7)
    W, H, th = d['W'].astype(np.float64), d['H'].astype(np.float64), d['theta'].astype(np.float64)
    rows = OH.rows_of(d['Y'], OH.FIRST, OH.T, np.float64)
    call = lambda **kw: robust_filter_rows(**dict(dict(W=W, H=H, lag_set=d['lag_set'], lag_val=th, Yrows=rows, first_row=OH.FIRST, lambdaI=0.5,
                                                       lambdaAR=0.5, missing=True, scale=0.3, c=1.5, sweeps=4), **kw))
    call()
    with pytest.raises(ValueError, match='lag 0'):
        call(lag_set=np.array([0, 1, 5], dtype=np.uint32))
    with pytest.raises(ValueError, match='largest lag'):
        call(first_row=4, Yrows=OH.rows_of(d['Y'], 4, OH.T, np.float64))
    with pytest.raises(ValueError, match='first_row'):
        call(first_row=OH.T + 1)
    with pytest.raises(ValueError, match='were expected'):
        call(Yrows=rows[1:])
    bad = np.full(OH.N, 0.3)
    for v in (0.0, -1.0, np.nan, np.inf):
        bad[13] = v
        with pytest.raises(ValueError, match=r'scale\[13\]'):
            call(scale=bad)
    with pytest.raises(ValueError, match='one value per series'):
        call(scale=np.full(OH.N + 1, 0.3))
    for c in (0.0, -2.0, np.nan):
        with pytest.raises(ValueError, match='c must be positive'):
            call(c=c)
    with pytest.raises(ValueError, match='sweeps'):
        call(sweeps=0)
    with pytest.raises(ValueError, match='sparse rows without missing'):
        call(missing=False)
    with pytest.raises(ValueError, match='row %d.*positive definite' % OH.EMPTY_ROW):
        call(lambdaI=0.0, lambdaAR=0.0)
    call(missing=False, Yrows=np.asarray(rows.todense()))                   # dense rows, every series: covered


def test_dense_rows_report_a_matrix_of_weights():
    k, (lamI, lamAR) = 7, OH.LAMBDAS[1]
    d = OH.inputs(k)
    Yd = np.asarray(d['Y'].todense(), dtype=np.float64)
    scale = RH.plain_scale(d, lamI, lamAR, missing=False)
    W, om = RH.statement(d, np.float64, lamI, lamAR, scale, missing=False, Y=Yd)
    assert om.shape == (OH.TN, OH.N) and 0.03 <= (om < 1).mean() <= 0.97
    # with missing, the non-zeros of an array are the observations and every other cell reads 1
    Ws, oms = RH.statement(d, np.float64, lamI, lamAR, scale)
    Wm, omm = RH.statement(d, np.float64, lamI, lamAR, scale, Y=Yd)
    mask = np.asarray(d['Y'][OH.FIRST:].todense()) != 0
    assert np.array_equal(Wm, Ws) and np.array_equal(omm[mask], oms) and np.all(omm[~mask] == 1)


def test_a_cell_stored_twice_gets_two_weights():
    k, (lamI, lamAR) = 7, OH.LAMBDAS[1]
    d, scale, _ = RH.case_a(k, lamI, lamAR)
    rows = OH.rows_of(d['Y'], OH.FIRST, OH.T, np.float64).tocsr()
    r = 3
    lo = rows.indptr[r]
    # the first entry of new row 3 once more, with a value far from the first: two observations of one cell
    data = np.insert(rows.data, lo + 1, rows.data[lo] + 10.0)
    indices = np.insert(rows.indices, lo + 1, rows.indices[lo])
    indptr = rows.indptr.copy()
    indptr[r + 1:] += 1
    twice = smat.csr_matrix((data, indices, indptr), shape=rows.shape)
    assert twice.nnz == rows.nnz + 1 and not twice.has_canonical_format
    W, om = robust_filter_rows(d['W'].astype(np.float64), d['H'].astype(np.float64), d['lag_set'], d['theta'].astype(np.float64), twice, OH.FIRST,
                               lamI, lamAR, True, scale, RH.C, RH.SWEEPS)
    assert om.shape == (rows.nnz + 1,)
    assert om[lo + 1] < 0.1 and om[lo] > om[lo + 1]                        # the far value is an outlier, its twin is not as far


def test_model_assimilate_with_robust_c_is_the_function():
    k, (lamI, lamAR) = 7, OH.LAMBDAS[1]
    d, scale, _ = RH.case_a(k, lamI, lamAR)
    dtype = np.float32
    m = make_model(d['W'][:OH.FIRST].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    block = OH.rows_of(d['Y'], OH.FIRST, OH.T, dtype)
    with pytest.raises(ValueError, match='fit_noise'):
        m.assimilate(block, lamI, lamAR, robust_c=RH.C)
    m.noise = (np.full(OH.N, scale * scale), np.ones(k))
    grown = m.assimilate(block, lamI, lamAR, robust_c=RH.C, robust_sweeps=RH.SWEEPS)
    W0 = np.zeros((OH.T, k), dtype=dtype)
    W0[:OH.FIRST] = m.W
    want, om = robust_filter_rows(W0, m.H, m.lag_set, m.lag_val, block, OH.FIRST, lamI, lamAR, True, np.sqrt(m.noise[0]), RH.C, RH.SWEEPS)
    assert np.array_equal(grown.W, want) and np.array_equal(grown.robust_weights, om) and grown.noise is m.noise
    assert np.array_equal(m.assimilate(block, lamI, lamAR, robust_c=RH.C, scale=np.full(OH.N, scale)).W,
                          robust_filter_rows(W0, m.H, m.lag_set, m.lag_val, block, OH.FIRST, lamI, lamAR, True, np.full(OH.N, scale), RH.C, 4)[0])
    # the default stays what it was
    plain = m.assimilate(block, lamI, lamAR)
    assert np.array_equal(plain.W, filter_rows(W0, m.H, m.lag_set, m.lag_val, block, OH.FIRST, lamI, lamAR, True)) and not hasattr(plain, 'robust_weights')


def test_rolling_validate_refuses_robust_retraining():
    Y = np.random.RandomState(0).rand(60, 5).astype(np.float32)
    with pytest.raises(ValueError, match="update='assimilate'"):
        trmf.rolling_validate(Y, [1, 2], k=2, window_size=4, nr_windows=2, robust_c=3.0)
