"""GPU (-m gpu): online updates on the device -- trmf_session_assimilate (assim_factor_kernel, assim_chain_kernel) behind
Session.assimilate / Session.update and rolling_validate(update='assimilate').  Small shapes: the whole file takes a few seconds.

The yardstick.  The device differs from trmf.online.filter_rows by summation order only, so an fp32 session may be no farther
from the fp64 twin than 8x the fp32 twin is on the same input (online_helpers.yardstick; the 8 allows for another order of
summation across a 24-row chain), an fp64 session no farther than that bound scaled by eps64 / eps32.  Teacher-forced, every row
must meet the same bound on its own, with its prior formed from the device's own earlier rows: a failure names a row."""
import numpy as np
import pytest
import scipy.sparse as smat

import online_helpers as OH
import trmf
from forecast_helpers import fields
from helpers import evidence, make_model, relmax
from trmf import Metrics, synth
from trmf.model import NormalizedTransform
from trmf.rf_util import PyMatrix
from trmf.session import Session

pytestmark = pytest.mark.gpu

SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}             # the tolerance tests/test_gpu_impute.py uses for its fp64 sums
DTYPES = [np.float32, np.float64]


def _model(d, dtype, rows=OH.T):
    m = make_model(d['W'][:rows].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    if d['k'] == 1:     # PyMatrix tags a (rows, 1) array column-major, like the reference's; the two orders are the same bytes
        m.pyW.type = m.pyH.type = PyMatrix.DENSE_ROWMAJOR
    return m


def _training(d, dtype, storage):
    Y = d['Y'].astype(dtype)
    return np.ascontiguousarray(Y.toarray()) if storage == 'dense' else Y


def _assimilate(d, dtype, lamI, lamAR, missing=True, storage='sparse', first=OH.FIRST, transform=None):
    """(downloaded model, sums, Wnew, describe) of one session over the input set after assimilate(first)."""
    model = _model(d, dtype)
    with Session(_training(d, dtype, storage), model, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5, missing=missing) as s:
        if transform is not None:
            s.set_transform(transform)
        sums, Wnew = s.assimilate(first, return_latent=True)
        s.download()
        return model, sums, Wnew, s.describe()


def _gate(what, d, model, dtype, lamI, lamAR, missing, w64, dev32, first=OH.FIRST, Y=None):
    b = OH.bound(dtype, dev32)
    got = relmax(model.W[first:], w64[first:])
    rows = OH.teacher_forced(d, model.W, lamI, lamAR, missing, first, Y=Y)
    worst = int(np.argmax(rows))
    evidence('online update %s %s lambdaI=%g lambdaAR=%g: relmax to the fp64 twin %.3e = %.2f x its bound %.3e (fp32 twin %.3e); '
             'teacher-forced worst row %d: %.3e = %.2f x' % (what, np.dtype(dtype).name, lamI, lamAR, got, got / b, b, dev32,
                                                             first + worst, rows[worst], rows[worst] / b))
    assert np.array_equal(model.W[:first], d['W'][:first].astype(dtype))            # earlier rows keep their bits
    assert got <= b, (what, got, b)
    assert rows[worst] <= b, (what, 'row', first + worst, rows[worst], b)


# ---- 1. the matrix of cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lamI,lamAR', OH.LAMBDAS)
@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
@pytest.mark.parametrize('k', OH.RANKS)
def test_assimilate_matches_the_numpy_twin(k, dtype, lamI, lamAR):
    d = OH.inputs(k)
    w64, dev32 = OH.yardstick(k, lamI, lamAR)
    model, sums, Wnew, _ = _assimilate(d, dtype, lamI, lamAR)
    _gate('k=%d' % k, d, model, dtype, lamI, lamAR, True, w64, dev32)
    assert np.array_equal(Wnew, model.W[OH.FIRST:])
    assert sums['rows'] == OH.TN and sums['entries'] == d['Y'][OH.FIRST:].nnz


# ---- 2. paths -----------------------------------------------------------------------------------------------------------------
#        name                  environment                                         storage   missing density  describe() must hold
PATHS = [('dense-full', {}, 'dense', False, 0.3, ''),
         ('sparse-full', {}, 'sparse', False, 0.3, ''),
         ('every-cell-stored', {}, 'sparse', True, 1.0, ''),                  # (a dense Y with missing != 0 is refused at create)
         ('packed-gram', {'TRMF_NO_HV_TILE': '1'}, 'sparse', True, 0.3, 'unfused'),
         ('split-rows', {'TRMF_LONG_ROW': '24', 'TRMF_LONG_CHUNK': '32'}, 'sparse', True, 0.7, 'split rows'),
         ('split-rows-packed', {'TRMF_LONG_ROW': '24', 'TRMF_LONG_CHUNK': '32', 'TRMF_NO_HV_TILE': '1'}, 'sparse', True, 0.7, 'split rows'),
         ('global-reach', {'TRMF_FORECAST_GLOBAL': '1'}, 'sparse', True, 0.3, ''),
         ('global-reach-full', {'TRMF_FORECAST_GLOBAL': '1'}, 'dense', False, 0.3, ''),
         ('four-chunks', {'TRMF_ASSIM_CHUNK': '7'}, 'sparse', True, 0.3, ''),
         ('four-chunks-global', {'TRMF_ASSIM_CHUNK': '7', 'TRMF_FORECAST_GLOBAL': '1'}, 'sparse', True, 0.3, '')]


@pytest.mark.parametrize('dtype,k', [(np.float32, 40), (np.float64, 7)], ids=['float32-k40', 'float64-k7'])
@pytest.mark.parametrize('name,env,storage,missing,density,must', PATHS, ids=[p[0] for p in PATHS])
def test_every_path_matches_the_numpy_twin(name, env, storage, missing, density, must, dtype, k, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    lamI, lamAR = OH.LAMBDAS[0]
    d = OH.inputs(k, density)
    w64, dev32 = OH.yardstick(k, lamI, lamAR, missing, density)
    model, sums, Wnew, desc = _assimilate(d, dtype, lamI, lamAR, missing, storage)
    assert must in desc, desc
    _gate(name, d, model, dtype, lamI, lamAR, missing, w64, dev32)
    assert np.array_equal(Wnew, model.W[OH.FIRST:])
    assert sums['entries'] == (OH.TN * OH.N if not missing else d['Y'][OH.FIRST:].nnz)
    for key, W in (('sq_err_before', d['W'].astype(dtype)), ('sq_err_after', model.W)):
        want, _ = OH.sq_err(d, W, OH.FIRST, missing)
        assert abs(sums[key] - want) <= SUM_TOL[dtype] * abs(want), (key, sums[key], want)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_an_active_series_transform_is_what_gets_assimilated(dtype):
    k, (lamI, lamAR) = 16, OH.LAMBDAS[1]
    d = OH.inputs(k)
    raw = _training(d, dtype, 'dense') * np.linspace(0.5, 3.0, OH.N).astype(dtype) + dtype(1)
    tr = NormalizedTransform(raw)
    assert np.asarray(tr.a).dtype == dtype
    trained = smat.csr_matrix(tr.preprocess(raw).astype(dtype))         # the values the session trains on, in its own dtype
    model = _model(d, dtype)
    with Session(raw, model, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5, missing=False) as s:
        s.set_transform(tr)
        sums = s.assimilate(OH.FIRST)
        s.download()
    w64, dev32 = OH.yardstick_of(d, lamI, lamAR, False, Y=trained)
    _gate('transform', d, model, dtype, lamI, lamAR, False, w64, dev32, Y=trained)
    want, cnt = OH.sq_err(d, model.W, OH.FIRST, False, Y=trained)
    assert sums['entries'] == cnt and abs(sums['sq_err_after'] - want) <= SUM_TOL[dtype] * abs(want)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_a_range_of_one_row_and_an_empty_range(dtype):
    k, (lamI, lamAR) = 40, OH.LAMBDAS[1]
    d = OH.inputs(k)
    first = OH.T - 1
    w64, dev32 = OH.yardstick(k, lamI, lamAR, True, 0.3, first)
    model = _model(d, dtype)
    with Session(_training(d, dtype, 'sparse'), model, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5) as s:
        sums, Wnew = s.assimilate(OH.T, return_latent=True)              # first_row == rows: nothing to do
        assert sums == dict(rows=0, entries=0, sq_err_before=0.0, sq_err_after=0.0) and Wnew.shape == (0, k)
        assert np.array_equal(s.download().W, d['W'].astype(dtype))
        sums, Wnew = s.assimilate(first, return_latent=True)
        s.download()
    _gate('one-row', d, model, dtype, lamI, lamAR, True, w64, dev32, first)
    assert sums['rows'] == 1 and np.array_equal(Wnew, model.W[first:])


# ---- 3. contract --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_repeated_calls_give_the_same_bits_and_the_sums_match_numpy(dtype):
    k, (lamI, lamAR) = 40, OH.LAMBDAS[0]
    d = OH.inputs(k)
    model = _model(d, dtype)
    with Session(_training(d, dtype, 'sparse'), model, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5) as s:
        a, Wa = s.assimilate(OH.FIRST, return_latent=True)
        first = s.download().W.copy()
        b, Wb = s.assimilate(OH.FIRST, return_latent=True)
        second = s.download().W.copy()
    assert np.array_equal(Wa, Wb) and np.array_equal(first, second) and np.array_equal(Wa, first[OH.FIRST:])
    assert b['sq_err_before'] == a['sq_err_after'] == b['sq_err_after']               # the second call starts where the first ended
    before, cnt = OH.sq_err(d, d['W'].astype(dtype), OH.FIRST)
    after, _ = OH.sq_err(d, first, OH.FIRST)
    assert a['rows'] == OH.TN and a['entries'] == cnt
    assert abs(a['sq_err_before'] - before) <= SUM_TOL[dtype] * before and abs(a['sq_err_after'] - after) <= SUM_TOL[dtype] * after
    assert a['sq_err_after'] < a['sq_err_before']


def _refused(s, first, match):
    with pytest.raises(RuntimeError, match=match):
        s.assimilate(first)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_refused_calls_leave_the_session_as_it_was(dtype):
    d = OH.inputs(16, 1.0)         # every cell stored but for the two designed rows: the empty row is the first singular system
    Y = _training(d, dtype, 'sparse')
    # first_row below the largest lag / above rows; no ridge at all and an empty row
    model = _model(d, dtype)
    with Session(Y, model, lambdaI=0.0, lambdaAR=0.0, lambdaLag=0.5) as s:
        _refused(s, 4, 'largest lag')
        _refused(s, OH.T + 1, 'first_row')
        _refused(s, OH.FIRST, 'row %d' % OH.EMPTY_ROW)
        assert np.array_equal(s.download().W, d['W'].astype(dtype))
        s.set_lambdas(0.5, 50.0, 0.5)
        assert s.assimilate(OH.FIRST)['rows'] == OH.TN                       # the session still works
        s.run(1).download()
        assert np.isfinite(model.W).all()
    # a lag set with lag 0
    lag0 = make_model(d['W'].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), np.array([0, 1, 5], dtype=np.uint32))
    with Session(Y, lag0, lambdaLag=0.5) as s:
        _refused(s, OH.FIRST, 'lag 0')
        assert np.array_equal(s.download().W, d['W'].astype(dtype))
        s.run(1).download()
        assert np.isfinite(lag0.W).all()
    # rank above 64: the generic kernels' territory
    rng = np.random.RandomState(5)
    theta = np.asfortranarray((0.2 * rng.randn(3, 96)).astype(dtype))
    big = make_model(rng.rand(OH.T, 96).astype(dtype), rng.rand(OH.N, 96).astype(dtype), theta, d['lag_set'])
    W0 = big.W.copy()
    with Session(Y, big, lambdaLag=0.5) as s:
        _refused(s, OH.FIRST, 'ranks 1..64')
        assert np.array_equal(s.download().W, W0)
        s.run(1).download()
        assert np.isfinite(big.W).all()


def test_mark_counter_statistics_and_forecast_scores_are_untouched():
    dtype, k = np.float32, 16
    d = OH.inputs(k)
    truth = np.random.RandomState(2).rand(4, OH.N).astype(dtype)
    model = _model(d, dtype)
    with Session(_training(d, dtype, 'sparse'), model, **synth.HYPER) as s:
        s.run(2).mark()
        marked = [a.copy() for a in (s.download().W, model.H, model.lag_val)]
        s.forecast(4, truth=truth, return_forecast=False)
        rows, table = s.forecast_series_sums()
        st = s.stats(8)
        s.assimilate(OH.FIRST)
        moved = s.download().W.copy()
        keep = [key for key in st[0] if not key.startswith('ms_')]
        st2 = s.stats(8)
        assert len(st2) == len(st) == 2 and [[x[key] for key in keep] for x in st2] == [[x[key] for key in keep] for x in st]
        rows2, table2 = s.forecast_series_sums()
        assert rows2 == rows == 4 and np.array_equal(table2, table)
        assert not np.array_equal(moved[OH.FIRST:], marked[0][OH.FIRST:]) and np.array_equal(moved[:OH.FIRST], marked[0][:OH.FIRST])
        assert np.array_equal(model.H, marked[1]) and np.array_equal(model.lag_val, marked[2])        # H and Theta stay fixed
        s.rewind().download()
        assert all(np.array_equal(a, b) for a, b in zip(marked, (model.W, model.H, model.lag_val)))
        s.run(1)
        assert len(s.stats(8)) == 3                                           # the counter went on from the mark's 2


@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_run_after_assimilate_equals_a_fresh_session_from_the_downloaded_factors(storage, missing):
    dtype, k = np.float32, 16
    d = OH.inputs(k)
    Y = _training(d, dtype, storage)
    a = _model(d, dtype)
    with Session(Y, a, missing=missing, **synth.HYPER) as s:
        s.assimilate(OH.FIRST)
        s.download()
        b = make_model(a.W, a.H, a.lag_val, a.lag_set)
        s.run(2).download()
    with Session(Y, b, missing=missing, **synth.HYPER) as s:
        s.run(2).download()
    assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)


# ---- 4. Session.update and the rolling evaluation -----------------------------------------------------------------------------
@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_update_equals_append_rows_then_assimilate(storage, missing):
    dtype, k = np.float32, 16
    d = OH.inputs(k)
    Y = _training(d, dtype, storage)
    a, b = _model(d, dtype, OH.FIRST), _model(d, dtype, OH.FIRST)
    with Session(Y[:OH.FIRST], a, missing=missing, **synth.HYPER) as s:
        s.run(2)
        s.append_rows(Y[OH.FIRST:])
        rolled = make_model(np.zeros((OH.T, k), dtype), a.H, a.lag_val, a.lag_set)
        s.model = rolled
        prior = s.download().W.copy()                                         # the new rows as the AR roll-out left them
        want = s.assimilate(OH.FIRST)
        s.download()
    with Session(Y[:OH.FIRST], b, missing=missing, **synth.HYPER) as s:
        s.run(2)
        got = s.update(Y[OH.FIRST:])
        assert s.rows() == OH.T and s.model is not b and s.model.m == OH.T
        grown = s.download()                                                  # works without the caller's help
    assert got == want and got['rows'] == OH.TN
    assert np.array_equal(grown.W, rolled.W) and np.array_equal(grown.H, rolled.H) and np.array_equal(grown.lag_val, rolled.lag_val)
    assert np.array_equal(grown.lag_set, b.lag_set) and not np.array_equal(grown.W[OH.FIRST:], prior[OH.FIRST:])
    # right after append_rows, sq_err_before is the one-step-ahead forecast error of the block
    step, _ = OH.sq_err(dict(d, H=rolled.H), prior, OH.FIRST, missing)
    assert abs(got['sq_err_before'] - step) <= SUM_TOL[dtype] * step


GOLD_Y = np.load(OH.__file__.replace('online_helpers.py', 'golden/py_harness.npz'))['rv_Y']
ROLL = dict(k=3, window_size=8, nr_windows=3, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=4, threads=2, seed=0)
ROLL_LAGS = [1, 2, 5]


def _host_online_forecasts(model0, Y, dtype, missing, threshold):
    """The online rolling loop on the host: window 0's trained model (cast to dtype), then Model.assimilate per window."""
    win, nw = ROLL['window_size'], ROLL['nr_windows']
    start = Y.shape[0] - win * nw
    m = make_model(model0.W.astype(dtype), model0.H.astype(dtype), model0.lag_val.astype(dtype), model0.lag_set)
    out = []
    for w in range(nw):
        cut = start + w * win
        if w:
            block = Y[cut - win:cut].astype(dtype)
            m = m.assimilate(smat.csr_matrix(block) if missing else block, ROLL['lambdaI'], ROLL['lambdaAR'], missing=missing)
        out.append(m.forecast(win, threshold=threshold)[0])
    return np.vstack(out)


@pytest.mark.parametrize('missing', [True, False], ids=['observed', 'full'])
def test_rolling_validate_with_online_updates_equals_the_host_loop(missing):
    dtype = np.float32
    Y = np.ascontiguousarray(GOLD_Y.astype(dtype))
    win, nw = ROLL['window_size'], ROLL['nr_windows']
    start = Y.shape[0] - win * nw
    got = trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, update='assimilate', **ROLL)
    # the same loop by hand: window 0 trained on the device, every later window through Session.update
    model = trmf.Model.initialize(Y[:start], ROLL_LAGS, ROLL['k'], seed=0)
    dev = []
    with Session(smat.csr_matrix(Y[:start]) if missing else Y[:start], model, missing=missing, log_norms=False, timing=0,
                 lambdaI=ROLL['lambdaI'], lambdaAR=ROLL['lambdaAR'], lambdaLag=ROLL['lambdaLag']) as s:
        s.run(ROLL['max_iter']).download()
        model0 = make_model(model.W, model.H, model.lag_val, model.lag_set)
        for w in range(nw):
            cut = start + w * win
            if w:
                block = Y[cut - win:cut]
                s.update(smat.csr_matrix(block) if missing else block)
            dev.append(s.download().forecast(win, threshold=0)[0])
    dev = np.vstack(dev)
    assert np.array_equal(fields(got), fields(Metrics.generate(Y[start:], dev, missing=missing)))
    # against Model.assimilate on the host, gated like the rows themselves: 8 x what fp32 rounding costs the host loop
    f64 = _host_online_forecasts(model0, Y, np.float64, missing, 0)
    f32 = _host_online_forecasts(model0, Y, np.float32, missing, 0)
    yard, dist = relmax(f32, f64), relmax(dev, f64)
    evidence('online rolling evaluation missing=%d: device forecasts %.3e from the fp64 host loop, fp32 host loop %.3e (%.2f x the bound)' % (
        missing, dist, yard, dist / (OH.GATE * yard)))
    assert dist <= OH.GATE * yard
    # forecast and scoring on the device as well: the same windows, the forecasts' own rounding apart (a forecast moves by
    # ~ k eps32 |y|, a score -- a ratio of summed |errors| to summed |y| -- by that over its own size: 2e-7 / 0.01 at the worst)
    on_dev = trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, update='assimilate', forecast_on_device=True, **ROLL)
    assert np.allclose(fields(on_dev), fields(got), rtol=1e-4), (on_dev, got)
    assert not np.allclose(fields(got), fields(trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, **ROLL)), rtol=1e-6)


def test_rolling_validate_retrain_is_the_default_bit_for_bit():
    Y = GOLD_Y
    for kw in (dict(missing=True), dict(missing=False, forecast_on_device=True)):
        assert np.array_equal(fields(trmf.rolling_validate(Y, ROLL_LAGS, threshold=0, update='retrain', **kw, **ROLL)),
                              fields(trmf.rolling_validate(Y, ROLL_LAGS, threshold=0, **kw, **ROLL)))
    results, _ = trmf.grid_search(Y, ROLL_LAGS, {'lambdaI': [0.5]}, missing=False, threshold=0, update='assimilate', **{k: v for k, v in ROLL.items() if k != 'lambdaI'})
    assert np.array_equal(fields(results[0]['metrics']),
                          fields(trmf.rolling_validate(Y, ROLL_LAGS, missing=False, threshold=0, update='assimilate', **ROLL)))


# ---- 5. several ranks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_two_ranks_are_bit_identical_to_one(storage, missing, monkeypatch):
    dtype, k = np.float32, 40
    d = OH.inputs(k)
    Y = _training(d, dtype, storage)

    def run():
        model = _model(d, dtype, OH.FIRST)
        with Session(Y[:OH.FIRST], model, missing=missing, **synth.HYPER) as s:
            s.run(2)
            sums = s.update(Y[OH.FIRST:])
            again, Wnew = s.assimilate(OH.FIRST + 3, return_latent=True)
            grown = s.download()
            return grown.W.copy(), grown.H.copy(), sums, again, Wnew, s.describe()

    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = run()
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two = run()
    assert '1 rank' in one[5] and '2 ranks' in two[5]
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and np.array_equal(one[4], two[4])
    assert one[2] == two[2] and one[3] == two[3]
