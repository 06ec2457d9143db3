"""GPU (-m gpu): online loading updates on the device -- trmf_session_series_stats_init / trmf_session_adapt_series
(adapt_series_kernel, adapt_part_kernel, the adapt_full_* kernels) behind Session.init_series_stats / adapt_series /
update(adapt=True) and rolling_validate(adapt_series=True).  Small shapes: the whole file takes a few seconds.

The yardstick (tests/adapt_helpers.py).  H is checked teacher-forced: against trmf.online.series_ridge in fp64 on the W the
session itself holds -- the rows a block's statistics were formed from do not change afterwards, so the downloaded W is the W of
every stage.  An fp32 session may be no farther from it than 8x the fp32 recursive twin is on the same input, an fp64 session no
farther than that scaled by eps64 / eps32.  A ratio above 1 is a finding to explain, not a gate to widen."""
import numpy as np
import pytest

import adapt_helpers as AH
import online_helpers as OH
import trmf
from forecast_helpers import fields
from helpers import evidence, make_model, relmax
from trmf import Metrics, synth
from trmf.rf_util import PyMatrix
from trmf.session import Session

pytestmark = pytest.mark.gpu

SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}             # tests/test_gpu_online.py
DTYPES = [np.float32, np.float64]
LAM_AR = 50.0
BLOCKS = ((OH.FIRST, AH.MID), (AH.MID, OH.T))


def _model(d, dtype, rows=OH.FIRST):
    m = make_model(d['W'][:rows].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    if d['k'] == 1:     # PyMatrix tags a (rows, 1) array column-major, like the reference's; the two orders are the same bytes
        m.pyW.type = m.pyH.type = PyMatrix.DENSE_ROWMAJOR
    return m


def _part(k, lo, hi, dtype, storage='sparse', density=0.3, seed=None):
    """Rows lo..hi-1 of the designed matrix as a session takes them (the seed: rawsparse_helpers' random entry orders)."""
    if storage == 'dense':
        return AH.dense_of(k, lo, hi, dtype, density)
    return AH.raw_rows(k, lo, hi, dtype, density, None if seed is None else seed + lo).pymatrix()


def _open(k, dtype, lamI, storage='sparse', missing=True, density=0.3, seed=None, **kw):
    d = OH.inputs(k, density)
    model = _model(d, dtype)
    hyper = dict(lambdaI=lamI, lambdaAR=LAM_AR, lambdaLag=0.5)
    hyper.update(kw)
    return Session(_part(k, 0, OH.FIRST, dtype, storage, density, seed), model, missing=missing, **hyper)


def _sequence(k, dtype, lamI, gamma, adapt=True, **where):
    """init, update 12 rows, adapt, update 12 rows, adapt, download: dict(W, H, Wmid, Hmid (after the first block), sums)."""
    part = {key: where[key] for key in ('storage', 'density', 'seed') if key in where}
    with _open(k, dtype, lamI, **where) as s:
        if adapt:
            s.init_series_stats(gamma)
            assert s.series_stats_info() == dict(valid=True, stale=False, absorbed_rows=OH.FIRST, forget=gamma)
        out = dict(sums=[])
        for lo, hi in BLOCKS:
            out['sums'].append(s.update(_part(k, lo, hi, dtype, **part), adapt=adapt))
            if k == 1:  # (the grown host model's (rows, 1) arrays: see _model)
                s.model.pyW.type = s.model.pyH.type = PyMatrix.DENSE_ROWMAJOR
            m = s.download()
            if hi == AH.MID:
                out['Wmid'], out['Hmid'] = m.W.copy(), m.H.copy()
        if adapt:
            assert s.series_stats_info()['absorbed_rows'] == OH.T
        out['W'], out['H'] = m.W.copy(), m.H.copy()
        return out


def _gate(what, k, dtype, lamI, gamma, W, H, missing=True, storage='sparse', density=0.3):
    ref = AH.direct(W, k, lamI, gamma, missing, storage, density)
    _, yard, twin_rows = AH.yardstick(W, k, lamI, gamma, missing, storage, density)
    b, got = AH.bound(dtype, yard), relmax(H, ref)
    own = AH.own_scale(H, ref)
    evidence('online loadings %s %s k=%d lambdaI=%g gamma=%g: relmax to the fp64 direct ridge %.3e = %.2f x its bound %.3e (fp32 recursion %.3e); '
             'designed series on their own scale: %s' % (what, np.dtype(dtype).name, k, lamI, gamma, got, got / b, b, yard,
                                                         ', '.join('%d: %.2f x' % (j, own[j] / AH.row_bound(dtype, k, twin_rows[j])) for j in AH.DESIGNED[1:])))
    assert got <= b, (what, got, b)
    assert not H[AH.NO_ENTRY].any()                                           # no entry: h = 0 exactly (lambdaI > 0)
    for j in AH.DESIGNED[1:]:
        assert own[j] <= AH.row_bound(dtype, k, twin_rows[j]), (what, 'series', j, own[j], AH.row_bound(dtype, k, twin_rows[j]))
    return got / b


# ---- 1. the matrix of cases ---------------------------------------------------------------------------------------------------
MATRIX = [(k, lamI, gamma) for k in OH.RANKS for lamI, gamma in AH.CASES + ((AH.SMALL_RIDGE,) if k <= 16 else ())]


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
@pytest.mark.parametrize('k,lamI,gamma', MATRIX, ids=['k%d-lamI%g-gamma%g' % c for c in MATRIX])
def test_adapt_matches_the_direct_ridge(k, lamI, gamma, dtype):
    got = _sequence(k, dtype, lamI, gamma)
    _gate('matrix', k, dtype, lamI, gamma, got['W'], got['H'])
    for (lo, hi), (assim, adapted) in zip(BLOCKS, got['sums']):
        r = AH.entries(k)[0]
        assert adapted['series'] == OH.N and adapted['rows'] == hi - lo == assim['rows']
        assert adapted['entries'] == np.count_nonzero((r >= lo) & (r < hi)) == assim['entries']
    # W up to the first adapt is what the same sequence without adapt gives, bit for bit; after it the new H steers the filter
    plain = _sequence(k, dtype, lamI, gamma, adapt=False)
    assert np.array_equal(got['Wmid'], plain['Wmid']) and np.array_equal(plain['H'], OH.inputs(k)['H'].astype(dtype))
    assert not np.array_equal(got['Hmid'], plain['Hmid']) and not np.array_equal(got['W'][AH.MID:], plain['W'][AH.MID:])


# ---- 2. paths -----------------------------------------------------------------------------------------------------------------
#        name                 storage   missing density seed  environment
PATHS = [('dense-full', 'dense', False, 0.3, None, {}),
         ('sparse-full', 'sparse', False, 0.3, None, {}),
         ('every-cell-stored', 'sparse', True, 1.0, None, {}),
         ('non-canonical', 'sparse', True, 0.3, 77, {}),                       # unsorted columns and rows, the doubled cell's copies apart
         ('init-in-items', 'sparse', True, 0.3, None, {'TRMF_ADAPT_CHUNK': '8'})]   # the init pass cuts every column into items of 8 entries


def _sq_err(k, dtype, W, H, lo, hi, missing, storage, density):
    """sum of the squared errors of rows lo..hi-1 in fp64: per stored entry (missing), per cell of the dense matrix, or the
    training objective's reading of sparse storage without missing (online_helpers.sq_err_entries)."""
    if storage == 'dense':
        P = np.asarray(W, np.float64)[lo:hi].dot(np.asarray(H, np.float64).T)
        return float(((AH.dense_of(k, lo, hi, dtype, density).astype(np.float64) - P) ** 2).sum()), (hi - lo) * OH.N
    r, c, v = AH.entries(k, density)
    keep = r < hi
    return OH.sq_err_entries(r[keep], c[keep], v[keep].astype(dtype), W, H, lo, hi, missing)


@pytest.mark.parametrize('dtype,k', [(np.float32, 40), (np.float64, 7)], ids=['float32-k40', 'float64-k7'])
@pytest.mark.parametrize('name,storage,missing,density,seed,env', PATHS, ids=[p[0] for p in PATHS])
def test_every_path_matches_the_direct_ridge(name, storage, missing, density, seed, env, dtype, k, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    lamI, gamma = AH.CASES[1]
    got = _sequence(k, dtype, lamI, gamma, storage=storage, missing=missing, density=density, seed=seed)
    _gate(name, k, dtype, lamI, gamma, got['W'], got['H'], missing, storage, density)
    sums = got['sums'][1][1]                                                   # the second adapt: rows MID.. with H before / after
    before, cnt = _sq_err(k, dtype, got['W'], got['Hmid'], AH.MID, OH.T, missing, storage, density)
    after, _ = _sq_err(k, dtype, got['W'], got['H'], AH.MID, OH.T, missing, storage, density)
    assert sums['entries'] == cnt and sums['rows'] == AH.BLOCK
    assert abs(sums['sq_err_before'] - before) <= SUM_TOL[dtype] * before and abs(sums['sq_err_after'] - after) <= SUM_TOL[dtype] * after
    assert sums['max_abs_change'] == float(np.abs(got['H'] - got['Hmid']).max())


# ---- 3. refused calls ---------------------------------------------------------------------------------------------------------
def _refused(s, match, H):
    with pytest.raises(RuntimeError, match=match):
        s.adapt_series()
    assert np.array_equal(s.download().H, H)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_refused_calls_leave_the_session_as_it_was(dtype):
    k, gamma = 7, 0.95
    H0 = OH.inputs(k)['H'].astype(dtype)
    with _open(k, dtype, 0.0) as s:                                            # no ridge: the series without an entry is singular
        assert s.series_stats_info() == dict(valid=False, stale=False, absorbed_rows=0, forget=1.0)
        _refused(s, 'no series statistics', H0)
        for bad in (0.0, 1.5, float('nan')):
            with pytest.raises(RuntimeError, match='forget'):
                s.init_series_stats(bad)
        s.init_series_stats(gamma)
        s.update(_part(k, OH.FIRST, AH.MID, dtype))
        _refused(s, 'series %d' % AH.NO_ENTRY, H0)
        assert s.series_stats_info() == dict(valid=True, stale=False, absorbed_rows=OH.FIRST, forget=gamma)       # nothing was absorbed
        s.set_lambdas(0.5, LAM_AR, 0.5)
        s.adapt_series()
        s.update(_part(k, AH.MID, OH.T, dtype), adapt=True)
        m = s.download()
        H1 = m.H.copy()
        _gate('after refusals', k, dtype, 0.5, gamma, m.W, H1)
        # stale tables: each names the cause and says what to do
        s.run(1)
        H2 = s.download().H.copy()
        assert s.series_stats_info()['stale']
        _refused(s, 'stale.*initialise', H2)
        s.init_series_stats(gamma)
        s.mark()
        assert s.series_stats_info()['valid']
        s.rewind()
        _refused(s, 'stale.*initialise', H2)
        s.init_series_stats(gamma)
        s.assimilate(OH.T)                                                     # nothing below the absorbed rows: still valid
        assert s.series_stats_info()['valid']
        s.assimilate(OH.T - 2)
        _refused(s, 'stale.*initialise', H2)
        s.init_series_stats(1.0)
        sums, Hn = s.adapt_series(return_loadings=True)                        # no new row: H refitted from the tables as they are
        m = s.download()
        assert sums['rows'] == 0 and sums['entries'] == 0 and np.array_equal(Hn, m.H)
        assert relmax(m.H, AH.direct(m.W, k, 0.5, 1.0)) <= AH.bound(dtype, AH.yardstick(m.W, k, 0.5, 1.0)[1])
    # rank above 64: the generic kernels' territory
    rng = np.random.RandomState(5)
    theta = np.asfortranarray((0.2 * rng.randn(3, 96)).astype(dtype))
    big = make_model(rng.rand(OH.FIRST, 96).astype(dtype), rng.rand(OH.N, 96).astype(dtype), theta, OH.inputs(k)['lag_set'])
    with Session(_part(k, 0, OH.FIRST, dtype), big, lambdaLag=0.5) as s:
        with pytest.raises(RuntimeError, match='ranks 1..64'):
            s.init_series_stats(1.0)


# ---- 4. reproducibility -------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ('W', 'H', 'Wmid', 'Hmid')) and a['sums'] == b['sums']


@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_two_sessions_and_two_ranks_give_the_same_bits(storage, missing, monkeypatch):
    dtype, k = np.float32, 40
    lamI, gamma = AH.CASES[1]
    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = _sequence(k, dtype, lamI, gamma, storage=storage, missing=missing)
    again = _sequence(k, dtype, lamI, gamma, storage=storage, missing=missing)
    assert _same(one, again)
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    with _open(k, dtype, lamI, storage=storage, missing=missing) as s:
        assert '2 ranks' in s.describe()
    two = _sequence(k, dtype, lamI, gamma, storage=storage, missing=missing)
    assert _same(one, two)


# ---- 5. equivalence and state -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
def test_update_with_adapt_equals_append_assimilate_adapt(storage, missing):
    dtype, k, gamma = np.float32, 16, 0.95
    block = lambda: _part(k, OH.FIRST, OH.T, dtype, storage)
    with _open(k, dtype, 0.5, storage=storage, missing=missing) as s:
        s.run(2)
        s.init_series_stats(gamma)
        s.append_rows(block())
        s.model = make_model(np.zeros((OH.T, k), dtype), s.model.H, s.model.lag_val, s.model.lag_set)
        want = (s.assimilate(OH.FIRST), s.adapt_series())
        a = s.download()
        Ynew, Wnew = s.forecast(6, return_latent=True)
    with _open(k, dtype, 0.5, storage=storage, missing=missing) as s:
        s.run(2)
        got = s.update(block(), adapt=True, forget=gamma)                      # no statistics yet: update initialises them before the append
        b = s.download()
        assert s.series_stats_info() == dict(valid=True, stale=False, absorbed_rows=OH.T, forget=gamma)
    assert got == want and np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)
    # the forecast after the update reads the new H: the host roll-out times it, within a k-term dot product's rounding
    assert np.array_equal(Wnew, a.latent_forecast(6)[a.m:])
    ref = Wnew.astype(np.float64).dot(a.H.astype(np.float64).T)
    tol = 4 * k * np.finfo(dtype).eps * np.abs(Wnew.astype(np.float64)).dot(np.abs(a.H.astype(np.float64)).T)       # tests/test_gpu_forecast.py
    assert np.all(np.abs(Ynew.astype(np.float64) - ref) <= tol + 1e-300)
    with _open(k, dtype, 0.5, storage=storage, missing=missing) as s:          # the defaults: today's call, today's return value
        s.run(2)
        plain = s.update(block())
        assert plain == want[0] and not s.series_stats_info()['valid']
        assert np.array_equal(s.download().W, a.W)


def test_mark_counter_statistics_scores_and_noise_are_untouched():
    dtype, k = np.float32, 16
    truth = np.random.RandomState(2).rand(4, OH.N).astype(dtype)
    with _open(k, dtype, 0.5, storage='dense', missing=False) as s:
        s.run(2).mark()
        marked = [a.copy() for a in (s.download().W, s.model.H, s.model.lag_val)]
        s.fit_noise()
        s.forecast(4, truth=truth, return_forecast=False)
        s.forecast_dist(4, level=0.9, truth=truth)
        rows, table = s.forecast_series_sums()
        iv = s.interval_series_sums()
        noise = [a.copy() for a in s.noise()]
        st = s.stats(8)
        s.init_series_stats(0.98)
        s.adapt_series()
        keep = [key for key in st[0] if not key.startswith('ms_')]
        st2 = s.stats(8)
        assert len(st2) == len(st) == 2 and [[x[key] for key in keep] for x in st2] == [[x[key] for key in keep] for x in st]
        rows2, table2 = s.forecast_series_sums()
        assert rows2 == rows == 4 and np.array_equal(table2, table)
        iv2 = s.interval_series_sums()
        assert iv2[0] == iv[0] == 4 and iv2[1].tobytes() == iv[1].tobytes()     # (bytes: a sum may be NaN)
        assert all(np.array_equal(a, b) for a, b in zip(noise, s.noise()))
        m = s.download()
        assert np.array_equal(m.W, marked[0]) and np.array_equal(m.lag_val, marked[2]) and not np.array_equal(m.H, marked[1])
        s.rewind().download()
        assert all(np.array_equal(a, b) for a, b in zip(marked, (s.model.W, s.model.H, s.model.lag_val)))
        s.run(1)
        assert len(s.stats(8)) == 3                                           # the counter went on from the mark's 2


# ---- 6. the rolling evaluation ------------------------------------------------------------------------------------------------
GOLD_Y = np.load(OH.__file__.replace('online_helpers.py', 'golden/py_harness.npz'))['rv_Y']
ROLL = dict(k=3, window_size=8, nr_windows=3, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=4, threads=2, seed=0)
ROLL_LAGS = [1, 2, 5]


def _host_loop(model0, Y, dtype, missing, gamma):
    """The adaptive online loop on the host: window 0's trained model (cast), then Model.assimilate(adapt=True) per window."""
    import scipy.sparse as smat
    win, nw = ROLL['window_size'], ROLL['nr_windows']
    start = Y.shape[0] - win * nw
    as_y = lambda a: smat.csr_matrix(a) if missing else a
    m = make_model(model0.W.astype(dtype), model0.H.astype(dtype), model0.lag_val.astype(dtype), model0.lag_set)
    m.init_series_stats(as_y(Y[:start].astype(dtype)), gamma, missing)
    out = []
    for w in range(nw):
        cut = start + w * win
        if w:
            m = m.assimilate(as_y(Y[cut - win:cut].astype(dtype)), ROLL['lambdaI'], ROLL['lambdaAR'], missing=missing, adapt=True, forget=gamma)
        out.append(m.forecast(win, threshold=0)[0])
    return np.vstack(out)


@pytest.mark.parametrize('missing', [True, False], ids=['observed', 'full'])
def test_rolling_validate_with_adaptive_loadings_equals_the_host_loop(missing):
    import scipy.sparse as smat
    dtype, gamma = np.float32, 0.95
    Y = np.ascontiguousarray(GOLD_Y.astype(dtype))
    win, nw = ROLL['window_size'], ROLL['nr_windows']
    start = Y.shape[0] - win * nw
    got = trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, update='assimilate', adapt_series=True, forget=gamma, **ROLL)
    # the same loop by hand: window 0 trained on the device, every later window through Session.update(adapt=True)
    model = trmf.Model.initialize(Y[:start], ROLL_LAGS, ROLL['k'], seed=0)
    as_y = lambda a: smat.csr_matrix(a) if missing else a
    dev = []
    with Session(as_y(Y[:start]), model, missing=missing, log_norms=False, timing=0,
                 lambdaI=ROLL['lambdaI'], lambdaAR=ROLL['lambdaAR'], lambdaLag=ROLL['lambdaLag']) as s:
        s.run(ROLL['max_iter']).download()
        model0 = make_model(model.W, model.H, model.lag_val, model.lag_set)
        for w in range(nw):
            cut = start + w * win
            if w:
                s.update(as_y(Y[cut - win:cut]), adapt=True, forget=gamma)
            dev.append(s.download().forecast(win, threshold=0)[0])
    dev = np.vstack(dev)
    assert np.array_equal(fields(got), fields(Metrics.generate(Y[start:], dev, missing=missing)))
    # against Model.assimilate(adapt=True) on the host, gated like the rows themselves: 8 x what fp32 rounding costs the host loop
    f64, f32 = _host_loop(model0, Y, np.float64, missing, gamma), _host_loop(model0, Y, np.float32, missing, gamma)
    yard, dist = relmax(f32, f64), relmax(dev, f64)
    evidence('adaptive online rolling evaluation missing=%d: device forecasts %.3e from the fp64 host loop, fp32 host loop %.3e (%.2f x the bound)' % (
        missing, dist, yard, dist / (OH.GATE * yard)))
    assert dist <= OH.GATE * yard
    on_dev = trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, update='assimilate', forecast_on_device=True, adapt_series=True,
                                   forget=gamma, **ROLL)
    assert np.allclose(fields(on_dev), fields(got), rtol=1e-4), (on_dev, got)       # tests/test_gpu_online.py: the forecasts' own rounding
    # the default is today's evaluation, bit for bit, and adapting is another one
    frozen = trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, update='assimilate', **ROLL)
    assert np.array_equal(fields(frozen), fields(trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, update='assimilate',
                                                                        adapt_series=False, forget=1.0, **ROLL)))
    assert not np.allclose(fields(got), fields(frozen), rtol=1e-6)
    with pytest.raises(ValueError, match='adapt_series'):
        trmf.rolling_validate(Y, ROLL_LAGS, missing=missing, threshold=0, adapt_series=True, **ROLL)
