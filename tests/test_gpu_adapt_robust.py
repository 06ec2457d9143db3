"""GPU (-m gpu): robust online loading updates on the device -- trmf_session_adapt_series_robust (adapt_robust_series_kernel,
adapt_robust_objective_kernel) behind Session.adapt_series_robust / update(adapt_robust=True) and
rolling_validate(adapt_robust=True).  Small shapes: the whole file takes a few seconds.

The yardstick (tests/adapt_robust_helpers.py).  H and the weights are checked teacher-forced: against the fp64 statement
trmf.online.SeriesStats.absorb_robust on the W the session itself holds and the H it held before the call.  An fp32 session may be
no farther from it than 8x the fp32 statement is from its fp64 twin on the same input, an fp64 session no farther than that scaled
by eps64 / eps32.  Borderline cells alone are excused from the (u < 1) comparison.  A ratio above 1 is a finding to explain, not a
gate to widen."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as smat

import adapt_helpers as AH
import adapt_robust_helpers as ARH
import online_helpers as OH
import trmf
from forecast_helpers import fields
from helpers import evidence, make_model, relmax
from trmf.rf_util import PyMatrix
from trmf.session import Session, TrmfRobustAdaptSums

pytestmark = pytest.mark.gpu

SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}             # tests/test_gpu_online.py
DTYPES = [np.float32, np.float64]
LAM_AR = 50.0
C, SWEEPS = ARH.C, ARH.SWEEPS


def _model(d, dtype, rows=OH.FIRST):
    m = make_model(d['W'][:rows].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    if d['k'] == 1:     # PyMatrix tags a (rows, 1) array column-major, like the reference's; the two orders are the same bytes
        m.pyW.type = m.pyH.type = PyMatrix.DENSE_ROWMAJOR
    return m


def _part(k, lo, hi, dtype, storage='sparse', seed=None):
    if storage == 'dense':
        return AH.dense_of(k, lo, hi, dtype)
    return AH.raw_rows(k, lo, hi, dtype, 0.3, None if seed is None else seed + lo).pymatrix()


def _open(k, dtype, lamI, storage='sparse', missing=True, seed=None, **kw):
    hyper = dict(lambdaI=lamI, lambdaAR=LAM_AR, lambdaLag=0.5)
    hyper.update(kw)
    return Session(_part(k, 0, OH.FIRST, dtype, storage, seed), _model(OH.inputs(k), dtype), missing=missing, **hyper)


def _grow(s, block, rows):
    """append_rows + a host model of the new size (what Session.update does before it filters)."""
    s.append_rows(block)
    k = s.model.k
    s.model = make_model(np.zeros((rows, k), s.model.W.dtype), s.model.H, s.model.lag_val, s.model.lag_set)
    if k == 1:
        s.model.pyW.type = s.model.pyH.type = PyMatrix.DENSE_ROWMAJOR


def _sequence(k, dtype, lamI, gamma, c=C, sweeps=SWEEPS, seed=None, twin=True, scales=None):
    """init, then per block: append, plain filter, download W and H, robust loading update with the case's scale.  A list of
    dict(y (the Twin's block), sums, H, weights, W, Hin) per block."""
    out = []
    with _open(k, dtype, lamI, seed=seed) as s:
        s.init_series_stats(gamma)
        tw = None
        for b, (lo, hi) in enumerate(ARH.BLOCKS):
            _grow(s, _part(k, lo, hi, dtype, seed=seed), hi)
            s.assimilate(lo)
            m = s.download()
            W, Hin = m.W.copy(), m.H.copy()
            y = None
            if twin:
                if tw is None:
                    tw = ARH.Twin(W[:lo], AH.csc_of(k, 0, lo, np.float32), gamma)
                y = tw.block(W, AH.csc_of(k, lo, hi, np.float32), Hin, lamI, None if scales is None else scales[b], c, sweeps)
            scale = y['scale'] if y is not None else scales[b]
            sums, H, weights = s.adapt_series_robust(c, sweeps, scale, return_loadings=True, return_weights=True)
            assert np.array_equal(s.download().H, H)
            assert s.series_stats_info() == dict(valid=True, stale=False, absorbed_rows=hi, forget=gamma)
            out.append(dict(y=y, sums=sums, H=H, weights=weights, W=W, Hin=Hin, scale=scale))
    return out


def _gate(what, k, dtype, lamI, gamma, blocks):
    worst = 0.0
    for b, blk in enumerate(blocks):
        y, H, wts = blk['y'], blk['H'], blk['weights']
        down, border = ARH.exercised(y)
        assert 0.03 <= down <= 0.97 and border <= 0.01, (what, b, down, border)
        bH, bw = ARH.bound(dtype, y['dev_H']), ARH.bound(dtype, y['dev_weights'])
        gH = relmax(H, y['H64'])
        assert np.array_equal(wts.indices, y['rows']) and np.array_equal(wts.indptr, y['indptr'])
        gw = float(np.abs(wts.data.astype(np.float64) - y['om64']).max())
        evidence('robust online loadings %s %s k=%d lambdaI=%g gamma=%g block %d: H relmax to the fp64 statement %.3e = %.2f x its bound %.3e '
                 '(fp32 statement %.3e); weights max abs diff %.3e = %.2f x its bound %.3e (fp32 statement %.3e); %.0f %% down-weighted, %d borderline'
                 % (what, np.dtype(dtype).name, k, lamI, gamma, b, gH, gH / bH, bH, y['dev_H'], gw, gw / bw, bw, y['dev_weights'], 100 * down,
                    int(y['border'].sum())))
        assert gH <= bH, (what, b, gH, bH)
        assert gw <= bw, (what, b, gw, bw)
        clear = ~y['border']
        assert np.array_equal((wts.data < 1)[clear], (y['om64'] < 1)[clear])
        assert abs(int(blk['sums']['downweighted']) - int((y['om64'] < 1).sum())) <= int(y['border'].sum())
        assert not H[AH.NO_ENTRY].any()                                        # no entry: h = 0 exactly (lambdaI > 0)
        worst = max(worst, gH / bH, gw / bw)
    return worst


def _check_sums(k, dtype, lamI, blk, lo, hi, first):
    sums, wts, y = blk['sums'], blk['weights'], blk['y']
    r = AH.entries(k)[0]
    cnt = np.count_nonzero((r >= lo) & (r < hi))
    assert sums['series'] == OH.N and sums['rows'] == hi - lo and sums['entries'] == cnt == wts.nnz
    assert sums['downweighted'] == int((wts.data < 1).sum())
    assert abs(sums['weight_sum'] - float(wts.data.astype(np.float64).sum())) <= 1e-12 * cnt
    assert sums['max_abs_change'] == float(np.abs(blk['H'] - blk['Hin']).max())
    assert sums['objective_after'] <= sums['objective_before']
    if first:       # the tables of the rows before the first block are the init pass's: the twin's in the session's element type
        from trmf import SeriesStats
        before = SeriesStats(blk['W'][:lo], ARH.cast(AH.csc_of(k, 0, lo, np.float32), dtype), y['before'].forget, True)
        Ynew = ARH.cast(AH.csc_of(k, lo, hi, np.float32), dtype)
        for key, H in (('objective_before', blk['Hin']), ('objective_after', blk['H'])):
            want = trmf.robust_series_objective(before, blk['W'], Ynew, H, lamI, blk['scale'], C)
            assert abs(sums[key] - want) <= SUM_TOL[dtype] * abs(want), (key, sums[key], want)


# ---- 1. the matrix of cases ---------------------------------------------------------------------------------------------------
MATRIX = [(k, lamI, gamma) for k in OH.RANKS for lamI, gamma in AH.CASES]


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
@pytest.mark.parametrize('k,lamI,gamma', MATRIX, ids=['k%d-lamI%g-gamma%g' % c for c in MATRIX])
def test_the_robust_update_matches_the_numpy_statement(k, lamI, gamma, dtype):
    blocks = _sequence(k, dtype, lamI, gamma)
    _gate('matrix', k, dtype, lamI, gamma, blocks)
    for b, (lo, hi) in enumerate(ARH.BLOCKS):
        _check_sums(k, dtype, lamI, blocks[b], lo, hi, b == 0)
    # the cell stored twice carries a weight per copy
    wts = blocks[0]['weights']
    col = wts.indices[wts.indptr[AH.TWICE]:wts.indptr[AH.TWICE + 1]]
    r, c, _ = AH.entries(k)
    copies = np.count_nonzero((r == AH.TWICE_ROW) & (c == AH.TWICE))
    assert np.count_nonzero(col == AH.TWICE_ROW - OH.FIRST) == copies >= 2


# ---- 2. tail shapes: the batch boundaries and the group-of-4 remainders ----------------------------------------------------------
TAILS = (0, 1, 3, 4, 5, 63, 64, 65, 129)          # one series per length (nine series: one per tail the kernel treats differently)
T_HIST, T_NEW = 16, 130


@functools.lru_cache(maxsize=None)
def _tail_problem(k):
    rng = np.random.RandomState(3000 + k)
    n, T = len(TAILS), T_HIST + T_NEW
    W = rng.rand(T, k).astype(np.float32)
    H = rng.rand(n, k).astype(np.float32)
    theta = rng.randn(len(OH.LAGS), k)
    theta = np.asfortranarray((theta / (np.abs(theta).sum(axis=0) + 0.1)).astype(np.float32))
    mask = np.zeros((T, n), dtype=bool)
    mask[:T_HIST] = rng.rand(T_HIST, n) < 0.5
    for j, L in enumerate(TAILS):
        mask[T_HIST + np.sort(rng.permutation(T_NEW)[:L]), j] = True
    vals = rng.rand(T, n).astype(np.float32)
    vals[vals == 0] = 0.5
    Y = smat.csc_matrix(np.where(mask, vals, np.float32(0)).astype(np.float32))
    assert np.diff(Y[T_HIST:].tocsc().indptr).tolist() == list(TAILS)
    return dict(W=W, H=H, theta=theta, lag_set=np.array(OH.LAGS, dtype=np.uint32), Y=Y, k=k)


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
@pytest.mark.parametrize('k', (7, 40, 64))
def test_tails_of_every_batch_and_group_shape(k, dtype):
    d = _tail_problem(k)
    lamI, gamma = 0.5, 0.95
    head, tail = d['Y'][:T_HIST].tocsr().astype(dtype), d['Y'][T_HIST:].tocsr().astype(dtype)
    with Session(head, _model(d, dtype, T_HIST), missing=True, lambdaI=lamI, lambdaAR=LAM_AR, lambdaLag=0.5) as s:
        s.init_series_stats(gamma)
        _grow(s, tail, T_HIST + T_NEW)
        s.assimilate(T_HIST)
        m = s.download()
        W, Hin = m.W.copy(), m.H.copy()
        tw = ARH.Twin(W[:T_HIST], d['Y'][:T_HIST].tocsc(), gamma)
        y = tw.block(W, d['Y'][T_HIST:].tocsc(), Hin, lamI)
        sums, H, wts = s.adapt_series_robust(C, SWEEPS, y['scale'], return_loadings=True, return_weights=True)
    assert np.diff(wts.indptr).tolist() == list(TAILS) and np.array_equal(wts.indices, y['rows'])
    bH, bw = ARH.bound(dtype, y['dev_H']), ARH.bound(dtype, y['dev_weights'])
    gH, gw = relmax(H, y['H64']), float(np.abs(wts.data.astype(np.float64) - y['om64']).max())
    evidence('robust online loadings tails %s k=%d: H %.3e = %.2f x its bound %.3e; weights %.3e = %.2f x its bound %.3e; %d of %d down-weighted'
             % (np.dtype(dtype).name, k, gH, gH / bH, bH, gw, gw / bw, bw, int((y['om64'] < 1).sum()), y['om64'].size))
    assert gH <= bH and gw <= bw, (gH, bH, gw, bw)
    clear = ~y['border']
    assert np.array_equal((wts.data < 1)[clear], (y['om64'] < 1)[clear]) and (y['om64'] < 1).any()
    assert sums['entries'] == sum(TAILS) and sums['objective_after'] <= sums['objective_before']


# ---- 3. c = inf is the plain update, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
@pytest.mark.parametrize('k', (7, 40, 64))
def test_an_infinite_c_is_adapt_series_bit_for_bit(k, dtype):
    lamI, gamma = AH.CASES[1]
    (lo, mid), (_, hi) = ARH.BLOCKS
    got = []
    for robust in (False, True):
        with _open(k, dtype, lamI) as s:
            s.init_series_stats(gamma)
            _grow(s, _part(k, lo, mid, dtype), mid)
            s.assimilate(lo)
            if robust:
                sums, H1, wts = s.adapt_series_robust(float('inf'), 3, 1.0, return_loadings=True, return_weights=True)
                assert (wts.data == 1).all() and sums['downweighted'] == 0 and sums['weight_sum'] == wts.nnz
            else:
                sums, H1 = s.adapt_series(return_loadings=True)
            _, after = s.update(_part(k, mid, hi, dtype), adapt=True)          # a following plain update continues from the tables
            got.append((sums, H1, after, s.download().H.copy()))
    (ps, pH, pa, pH2), (rs, rH, ra, rH2) = got
    assert np.array_equal(pH, rH) and np.array_equal(pH2, rH2) and pa == ra
    assert all(ps[key] == rs[key] for key in ps)


# ---- 4. refused calls ---------------------------------------------------------------------------------------------------------
def _refused(s, match, H, exc=RuntimeError, **kw):
    info = s.series_stats_info()
    with pytest.raises(exc, match=match):
        s.adapt_series_robust(**kw)
    assert np.array_equal(s.download().H, H) and s.series_stats_info() == info


@pytest.mark.parametrize('dtype', DTYPES, ids=['float32', 'float64'])
def test_refused_calls_leave_the_session_as_it_was(dtype):
    k, lamI, gamma = 7, 0.5, 0.95
    H0 = OH.inputs(k)['H'].astype(dtype)
    (lo, mid), _ = ARH.BLOCKS
    for storage in ('dense', 'sparse'):                                        # the full-observation forms keep one shared S
        with _open(k, dtype, lamI, storage=storage, missing=False) as s:
            s.init_series_stats(gamma)
            s.update(_part(k, lo, mid, dtype, storage))
            _refused(s, 'shared S', H0, scale=1.0)
            s.adapt_series()
    with _open(k, dtype, lamI) as s:
        _refused(s, 'no series statistics', H0, scale=1.0)
        s.init_series_stats(gamma)
        s.update(_part(k, lo, mid, dtype))
        _refused(s, 'no scale given and no noise', H0)
        for bad in (0.0, -1.0, float('nan')):
            _refused(s, 'c must be positive', H0, c=bad, scale=1.0)
        for bad in (0, 65, -3):
            _refused(s, 'sweeps', H0, sweeps=bad, scale=1.0)
        for bad in (0.0, -1.0, float('nan'), float('inf')):
            sc = np.ones(OH.N)
            sc[5] = bad
            _refused(s, 'scale of series 5', H0, scale=sc)
        _refused(s, 'shape', H0, exc=ValueError, scale=np.ones(OH.N - 1))
        # the outputs of a refused call stay as they were
        sums = TrmfRobustAdaptSums()
        sums.entries, sums.weight_sum = 7, 0.25
        Hbuf = np.full((OH.N, k), 3, dtype=dtype)
        wptr, wrows, wts = np.full(OH.N + 1, 9, np.uint64), np.full(512, 9, np.uint32), np.full(512, 3, dtype=dtype)
        assert s.lib.trmf_session_adapt_series_robust(s.handle, -1.0, 4, None, ctypes.byref(sums), Hbuf.ctypes.data, wptr.ctypes.data, wrows.ctypes.data,
                                                      wts.ctypes.data) < 0
        assert sums.entries == 7 and sums.weight_sum == 0.25 and (Hbuf == 3).all() and (wptr == 9).all() and (wrows == 9).all() and (wts == 3).all()
        # ... and a following plain update gives what a session without the refused calls gives
        after = s.adapt_series(return_loadings=True)
        with _open(k, dtype, lamI) as t:
            t.init_series_stats(gamma)
            t.update(_part(k, lo, mid, dtype))
            want = t.adapt_series(return_loadings=True)
        assert after[0] == want[0] and np.array_equal(after[1], want[1])
        # stale tables: the message says what to do
        s.run(1)
        H2 = s.download().H.copy()
        _refused(s, 'stale.*initialise', H2, scale=1.0)


# ---- 5. sameness and untouched state --------------------------------------------------------------------------------------------
def _same(a, b):
    return all(x['sums'] == y['sums'] and np.array_equal(x['H'], y['H']) and np.array_equal(x['weights'].data, y['weights'].data) and
               np.array_equal(x['weights'].indices, y['weights'].indices) and np.array_equal(x['W'], y['W']) for x, y in zip(a, b))


def test_two_sessions_two_ranks_and_non_canonical_input(monkeypatch):
    dtype, k = np.float32, 40
    lamI, gamma = AH.CASES[1]
    one = _sequence(k, dtype, lamI, gamma)
    scales = [blk['scale'] for blk in one]
    again = _sequence(k, dtype, lamI, gamma, twin=False, scales=scales)
    assert _same(one, again)
    # unsorted columns and rows, the doubled cell's copies apart: another stored order, the same H within the bound
    shuffled = _sequence(k, dtype, lamI, gamma, seed=77, twin=False, scales=scales)
    for b, (x, y) in enumerate(zip(one, shuffled)):
        bH = ARH.bound(dtype, x['y']['dev_H'])
        got = relmax(y['H'], x['y']['H64'])
        evidence('robust online loadings non-canonical input float32 k=%d block %d: H %.3e = %.2f x its bound %.3e' % (k, b, got, got / bH, bH))
        assert got <= bH and y['sums']['entries'] == x['sums']['entries']
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    with _open(k, dtype, lamI) as s:
        assert '2 ranks' in s.describe()
    two = _sequence(k, dtype, lamI, gamma, twin=False, scales=scales)
    assert _same(one, two)


def test_mark_counter_statistics_scores_and_noise_are_untouched():
    dtype, k = np.float32, 16
    (lo, mid), _ = ARH.BLOCKS
    truth = np.random.RandomState(2).rand(4, OH.N).astype(dtype)
    with _open(k, dtype, 0.5) as s:
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
        sums = s.adapt_series_robust(1.5, 3)                                   # the scale: the resident noise
        assert sums['rows'] == 0 and sums['entries'] == 0 and sums['objective_after'] <= sums['objective_before']
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


# ---- 6. Session.update and the rolling evaluation ---------------------------------------------------------------------------------
def test_update_with_adapt_robust_equals_append_assimilate_robust_adapt_robust():
    dtype, k, gamma, scale = np.float32, 16, 0.95, 0.2
    block = lambda: _part(k, OH.FIRST, OH.T, dtype)
    with _open(k, dtype, 0.5) as s:
        s.run(2)
        s.init_series_stats(gamma)
        _grow(s, block(), OH.T)
        s.mark()
        want = (s.assimilate_robust(OH.FIRST, 2.0, 3, scale), s.adapt_series_robust(2.0, 3, scale))
        a = s.download()
        aW, aH = a.W.copy(), a.H.copy()
    with _open(k, dtype, 0.5) as s:
        s.run(2)
        got = s.update(block(), robust_c=2.0, robust_sweeps=3, scale=scale, adapt=True, forget=gamma, adapt_robust=True)
        b = s.download()
        assert s.series_stats_info() == dict(valid=True, stale=False, absorbed_rows=OH.T, forget=gamma)
        with pytest.raises(ValueError, match='adapt_robust'):
            s.update(block(), adapt=True, adapt_robust=True)
        with pytest.raises(ValueError, match='adapt_robust'):
            s.update(block(), robust_c=2.0, scale=scale, adapt_robust=True)
        assert s.rows() == OH.T
    assert got == want and np.array_equal(aW, b.W) and np.array_equal(aH, b.H) and 0 < got[1]['downweighted'] < got[1]['entries']
    # without the flag: the unweighted loading update under robust_c, as before
    with _open(k, dtype, 0.5) as s:
        s.run(2)
        s.init_series_stats(gamma)
        _grow(s, block(), OH.T)
        want_plain = (s.assimilate_robust(OH.FIRST, 2.0, 3, scale), s.adapt_series())
        c = s.download()
        cW, cH = c.W.copy(), c.H.copy()
    with _open(k, dtype, 0.5) as s:
        s.run(2)
        got_plain = s.update(block(), robust_c=2.0, robust_sweeps=3, scale=scale, adapt=True, forget=gamma)
        e = s.download()
    assert got_plain == want_plain and np.array_equal(cW, e.W) and np.array_equal(cH, e.H) and not np.array_equal(cH, aH)


GOLD_Y = np.load(OH.__file__.replace('online_helpers.py', 'golden/py_harness.npz'))['rv_Y']
ROLL = dict(k=3, window_size=8, nr_windows=3, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=4, threads=2, seed=0)
ROLL_LAGS = [1, 2, 5]


def test_rolling_validate_with_adapt_robust_equals_the_host_loop():
    dtype, gamma = np.float32, 0.95
    Y = np.array(GOLD_Y, dtype=dtype, order='C')
    win, nw = ROLL['window_size'], ROLL['nr_windows']
    start = Y.shape[0] - win * nw
    rng = np.random.RandomState(7)
    spikes = (rng.rand(win * (nw - 1), Y.shape[1]) < 0.05) & (Y[start:start + win * (nw - 1)] != 0)      # spiked cells in the windows absorbed online
    Y[start:start + win * (nw - 1)][spikes] += 20.0 * Y.std()
    kw = dict(missing=True, threshold=0, update='assimilate', robust_c=3, adapt_series=True, forget=gamma)
    got = trmf.rolling_validate(Y, ROLL_LAGS, adapt_robust=True, **dict(kw, **ROLL))
    unweighted = trmf.rolling_validate(Y, ROLL_LAGS, **dict(kw, **ROLL))
    # the host loop: window 0 trained on the device, its noise fitted on the host, every later window through Model.assimilate
    model = trmf.Model.initialize(Y[:start], ROLL_LAGS, ROLL['k'], seed=0)
    with Session(smat.csr_matrix(Y[:start]), model, missing=True, log_norms=False, timing=0, lambdaI=ROLL['lambdaI'], lambdaAR=ROLL['lambdaAR'],
                 lambdaLag=ROLL['lambdaLag']) as s:
        s.run(ROLL['max_iter']).download()
    m = make_model(model.W, model.H, model.lag_val, model.lag_set).fit_noise(smat.csr_matrix(Y[:start]), missing=True)
    m.init_series_stats(smat.csr_matrix(Y[:start]), gamma, True)
    host = [m.forecast(win, threshold=0)[0]]
    for w in range(1, nw):
        cut = start + w * win
        m = m.assimilate(smat.csr_matrix(Y[cut - win:cut]), ROLL['lambdaI'], ROLL['lambdaAR'], missing=True, robust_c=3, robust_sweeps=4, adapt=True,
                         forget=gamma, adapt_robust=True)
        assert (m.adapt_weights.data < 1).any()
        host.append(m.forecast(win, threshold=0)[0])
    want = trmf.Metrics.generate(Y[start:], np.vstack(host), missing=True)
    assert np.allclose(fields(got), fields(want), rtol=1e-4), (got, want)       # tests/test_gpu_robust.py: the forecasts' own rounding
    assert not np.allclose(fields(got), fields(unweighted), rtol=1e-6), (got, unweighted)
    on_dev = trmf.rolling_validate(Y, ROLL_LAGS, adapt_robust=True, forecast_on_device=True, **dict(kw, **ROLL))
    assert np.allclose(fields(on_dev), fields(got), rtol=1e-4), (on_dev, got)
    for bad in (dict(kw, robust_c=None), dict(kw, adapt_series=False)):
        with pytest.raises(ValueError, match='adapt_robust'):
            trmf.rolling_validate(Y, ROLL_LAGS, adapt_robust=True, **dict(bad, **ROLL))
