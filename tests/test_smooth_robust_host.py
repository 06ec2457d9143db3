"""CPU: the robust smoother's host statement (trmf.robust_smooth_rows, trmf.robust_window_objective), the conditions every input
of tests/test_gpu_smooth_robust.py must meet to check anything, the IRLS twin the device is gated by, the smooth_robust keyword of
Model.assimilate / rolling_validate, and the quality claim on the spiked panels in fp64."""
import numpy as np
import pytest

import online_helpers as OH
import robust_helpers as RH
import smooth_helpers as SH
import smooth_robust_helpers as SR
import trmf
from trmf import robust_smooth_rows, robust_window_objective, smooth_rows, window_objective

NAMES = list(SR.CASES)


@pytest.mark.parametrize('name', NAMES)
def test_every_device_input_exercises_both_branches_and_the_twin_converges(name):
    t = SR.truth(name)
    print('%s: down-weighted %.1f %%, borderline %.2f %%' % (name, 100 * t['down'], 100 * t['border_share']))
    assert SR.DOWN_MIN <= t['down'] <= SR.DOWN_MAX and t['border_share'] <= SR.BORDER_MAX
    for dtype in (np.float32, np.float64):
        y = SR.yardstick(name, np.dtype(dtype))
        print('   twin %s: rows %.3e weights %.3e steps %s' % (np.dtype(dtype).name, y['rows'], y['weights'], y['steps']))
        assert y['converged'] and max(y['steps']) < SH.MAX_ITER
        assert 0 < y['rows'] < (1e-2 if dtype == np.float32 else 1e-7)


@pytest.mark.parametrize('name', NAMES)
def test_every_sweep_lowers_the_huber_objective(name):
    spec = SR.CASES[name]
    d, scale = SR.case(name)
    J = [SR.objective_of(d, d['W'], spec['lamI'], spec['lamAR'], spec['first'], scale, missing=spec['missing'], storage=spec['storage'])]
    for sweeps in range(1, SR.SWEEPS + 1):
        W = SR.statement(d, np.float64, spec['lamI'], spec['lamAR'], spec['first'], scale, sweeps=sweeps, missing=spec['missing'],
                         storage=spec['storage'])[0]
        assert np.array_equal(W[:spec['first']], d['W'][:spec['first']].astype(np.float64))
        J.append(SR.objective_of(d, W, spec['lamI'], spec['lamAR'], spec['first'], scale, missing=spec['missing'], storage=spec['storage']))
    assert all(b <= a * (1 + 1e-14) for a, b in zip(J, J[1:])), J


def test_an_infinite_c_is_the_plain_smoother_and_its_objective():
    d = OH.inputs(16)
    first, (lamI, lamAR) = 72, OH.LAMBDAS[0]
    W, H, th = d['W'].astype(np.float64), d['H'].astype(np.float64), d['theta'].astype(np.float64)
    rows = OH.rows_of(d['Y'], first, OH.T, np.float64)
    got, om = robust_smooth_rows(W, H, d['lag_set'], th, rows, first, lamI, lamAR, True, 0.3, np.inf, 2)
    want = smooth_rows(W, H, d['lag_set'], th, rows, first, lamI, lamAR, True)
    assert (om == 1).all() and om.shape == (rows.nnz,) and np.allclose(got, want, rtol=0, atol=1e-12)
    assert robust_window_objective(got, H, d['lag_set'], th, rows, first, lamI, lamAR, True, 0.3, np.inf) == pytest.approx(
        window_objective(got, H, d['lag_set'], th, rows, first, lamI, lamAR, True), rel=1e-14)


def test_the_weights_are_the_last_sweeps_and_an_empty_window_is_a_no_op():
    name = 'a-k7-0.5-50-first72'
    spec = SR.CASES[name]
    d, scale = SR.case(name)
    prev = SR.statement(d, np.float64, spec['lamI'], spec['lamAR'], 72, scale, sweeps=SR.SWEEPS - 1)[0]
    om = SR.truth(name)['om64']
    rows = OH.rows_of(d['Y'], 72, OH.T, np.float64)
    H = d['H'].astype(np.float64)
    want = np.ones(rows.nnz)
    for r in range(rows.shape[0]):
        lo, hi = rows.indptr[r], rows.indptr[r + 1]
        res = np.abs(rows.data[lo:hi] - H[rows.indices[lo:hi]].dot(prev[72 + r]))
        want[lo:hi] = np.where(res > SR.C * scale, SR.C * scale / np.maximum(res, 1e-300), 1.0)
    assert np.allclose(om, want, rtol=1e-12, atol=0)
    W = d['W'].astype(np.float64)
    got, om0 = robust_smooth_rows(W, H, d['lag_set'], d['theta'].astype(np.float64), rows[:0], OH.T, 0.5, 50.0, True, scale)
    assert np.array_equal(got, W) and om0.size == 0


def test_every_refusal_is_a_value_error():
    d = OH.inputs(7)
    W, H, th = d['W'].astype(np.float64), d['H'].astype(np.float64), d['theta'].astype(np.float64)
    rows = OH.rows_of(d['Y'], OH.FIRST, OH.T, np.float64)
    call = lambda **kw: robust_smooth_rows(**dict(dict(W=W, H=H, lag_set=d['lag_set'], lag_val=th, Yrows=rows, first_row=OH.FIRST, lambdaI=0.5,
                                                       lambdaAR=0.5, missing=True, scale=0.3, c=1.5, sweeps=4), **kw))
    call()
    for kw, match in ((dict(lag_set=np.array([0, 1, 5])), 'lag 0'), (dict(first_row=4), 'largest lag'), (dict(first_row=OH.T + 1), 'first_row'),
                      (dict(Yrows=rows[1:]), 'Yrows'), (dict(missing=False), 'sparse rows without missing'), (dict(scale=np.ones(3)), 'scale has shape'),
                      (dict(scale=-1.0), 'not finite and positive'), (dict(c=0.0), 'c must be positive'), (dict(sweeps=0), 'sweeps')):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    dense = np.ones((OH.TN, OH.N))
    with pytest.raises(ValueError, match='row %d' % OH.FIRST):                   # no ridge and fewer series than the rank allows
        robust_smooth_rows(W[:, :7], np.zeros_like(H), d['lag_set'], th, dense, OH.FIRST, 0.0, 0.0, False, 0.3)


def test_model_assimilate_takes_the_keyword_and_refuses_it_alone():
    dtype = np.float64
    d = OH.inputs(7)
    Yd = np.asarray(d['Y'].toarray(), dtype=dtype)
    m = trmf.Model.from_arrays(d['W'][:OH.FIRST].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    block, back = Yd[OH.FIRST:], Yd[OH.FIRST - 8:OH.FIRST]
    with pytest.raises(ValueError, match='Huber'):                               # without the keyword: the refusal of before, word for word
        m.assimilate(block, 0.5, 50.0, robust_c=1.5, scale=0.3, smooth_back=8, Yback=back)
    for kw in (dict(robust_c=1.5, scale=0.3), dict(smooth_back=8, Yback=back), {}):
        with pytest.raises(ValueError, match='smooth_robust=True needs both'):
            m.assimilate(block, 0.5, 50.0, smooth_robust=True, **kw)
    got = m.assimilate(block, 0.5, 50.0, robust_c=1.5, scale=0.3, smooth_back=8, Yback=back, smooth_robust=True)
    filt = m.assimilate(block, 0.5, 50.0, robust_c=1.5, scale=0.3)
    want, om = robust_smooth_rows(filt.W, m.H, m.lag_set, m.lag_val, Yd[OH.FIRST - 8:], OH.FIRST - 8, 0.5, 50.0, True, 0.3, 1.5, 4)
    assert np.array_equal(got.W, want) and np.array_equal(got.robust_weights, om) and om.shape == (OH.TN + 8, OH.N)
    assert not np.array_equal(got.W[OH.FIRST - 8:], filt.W[OH.FIRST - 8:]) and np.array_equal(got.W[:OH.FIRST - 8], filt.W[:OH.FIRST - 8])


def test_rolling_validate_refuses_the_keyword_alone_before_anything_runs():
    Y = np.random.RandomState(0).rand(60, 5)
    for kw in (dict(robust_c=3.0), dict(smooth_back=4), {}):
        with pytest.raises(ValueError, match='smooth_robust=True needs both'):
            trmf.rolling_validate(Y, [1, 2], k=2, window_size=4, nr_windows=2, update='assimilate', smooth_robust=True, **kw)
    with pytest.raises(ValueError, match='undo the Huber weights'):
        trmf.rolling_validate(Y, [1, 2], k=2, window_size=4, nr_windows=2, update='assimilate', robust_c=3.0, smooth_back=4)


@pytest.mark.parametrize('seed', SR.QUALITY_SEEDS)
def test_spikes_bend_the_plain_smoother_and_not_the_robust_one(seed):
    p = SR.quality_panel(seed)
    dist = {key: SR.rms_distance(p[key], p['ref'], p['new']) for key in ('plain_f', 'plain_s', 'robust_f', 'robust_s')}
    print('spiked panel seed %d: plain filter %.4f, plain smoother %.4f, robust filter %.4f, robust smoother %.4f (%.3f of the plain smoother)' % (
        seed, dist['plain_f'], dist['plain_s'], dist['robust_f'], dist['robust_s'], dist['robust_s'] / dist['plain_s']))
    assert dist['robust_s'] <= 0.25 * dist['plain_s']
    assert dist['robust_s'] <= dist['robust_f']
