"""GPU (-m gpu): the sliding window on the device -- trmf_session_slide (csc_slide_count_kernel, csc_slide_kernel,
series_downdate_kernel) behind Session.slide / retire_rows / update(window=) and rolling_validate(window=).  Small shapes
(tests/slide_helpers.py): the whole file takes a few seconds.

The contract is bit-identity: after a slide the session IS the session trmf_session_create builds from the retained entries in
their stored order (slide_helpers.slid = trmf.online.slide_entries on both orientations), W[retire:] + the block's AR roll-out and
the current H and lag weights, so every later call returns the same bits on both.  Only the downdated statistics are held to a
yardstick instead (adapt_helpers.bound: 8x an fp32 NumPy twin of the same recursion against the fp64 direct ridge)."""
import numpy as np
import pytest

import adapt_helpers as AH
import online_helpers as OH
import slide_helpers as SH
import trmf
from helpers import evidence, make_model, relmax
from rawsparse_helpers import RawSparse
from trmf.model import NormalizedTransform
from trmf.rf_util import PyMatrix
from trmf.session import Session

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, 40), (np.float64, 7)]
DT_IDS = ['float32-k40', 'float64-k7']
HYPER = dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5)
SEED = 41
REACH = max(OH.LAGS)


def _model(d, dtype, W=None, H=None, theta=None):
    return make_model((d['W'] if W is None else W).astype(dtype), (d['H'] if H is None else H).astype(dtype),
                      (d['theta'] if theta is None else theta).astype(dtype), d['lag_set'])


def _rows(k, lo, hi, dtype, storage):
    """Rows lo..hi-1 as a session takes them: (what Session gets, the RawSparse behind it or None)."""
    if storage == 'dense':
        return SH.dense_rows(k, lo, hi, dtype), None
    raw = SH.raw_rows(k, lo, hi, dtype, SEED)
    return raw.pymatrix(), raw


def _after(s, T1):
    """What the contract promises equal on both sessions: three iterations (with the CG's step counts), the objective, the
    filter, the smoother and a forecast."""
    out = {}
    s.run(3)
    out['cg'] = [x['cg_iter'] for x in s.stats(3)]
    m = s.download()
    out['W'], out['H'], out['theta'] = m.W.copy(), m.H.copy(), m.lag_val.copy()
    out['J'] = np.float64(s.objective())
    out['assim'], out['Wa'] = s.assimilate(T1 - 6, return_latent=True)
    out['smooth'], out['Ws'] = s.smooth(T1 - 10, return_latent=True)
    out['Y5'], out['W5'] = s.forecast(5, return_latent=True)
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], np.ndarray) or isinstance(a[key], np.floating):
            assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


# ---- 1. equals a fresh session, bit for bit -----------------------------------------------------------------------------------
FORMS = [('sparse-missing', 'sparse', True, False), ('sparse-full', 'sparse', False, False), ('dense', 'dense', False, False),
         ('dense-transform', 'dense', False, True)]
MODES = [('retire-only', False, SH.RETIRE), ('fused', True, SH.RETIRE), ('retire-0', True, 0)]


@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('mode,with_block,retire', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('form,storage,missing,transform', FORMS, ids=[f[0] for f in FORMS])
def test_slide_equals_a_fresh_session(form, storage, missing, transform, mode, with_block, retire, dtype, k):
    """The sparse input is not canonical: neither orientation is sorted, one cell is stored twice in a retired row and one in a
    retained row.  The fresh session is created from slide_entries' output."""
    d = OH.inputs(k)
    T0, Tn = SH.T0, (OH.T - SH.T0 if with_block else 0)
    T1 = T0 - retire + Tn
    head, raw_head = _rows(k, 0, T0, dtype, storage)
    block, raw_block = _rows(k, T0, OH.T, dtype, storage) if with_block else (None, None)
    tr = NormalizedTransform(SH.dense_rows(k, 0, T0, dtype)) if transform else None
    with Session(head, _model(d, dtype, W=d['W'][:T0]), missing=missing, **HYPER) as s:
        if tr is not None:
            s.model.transform = tr
            s.set_transform(tr)
        s.run(1)
        m1 = s.download()
        W1, H1, Th1 = m1.W.copy(), m1.H.copy(), m1.lag_val.copy()
        sums = s.slide(block, retire)
        assert s.rows() == T1 and s.model.m == T1
        assert sums['rows_retired'] == retire and sums['rows_appended'] == Tn and sums['rows'] == T1
        if raw_head is not None:
            want = SH.slid(raw_head, retire, raw_block)
            assert sums['entries'] == want.nnz and sums['entries_retired'] == np.count_nonzero(raw_head.rows < retire)
            assert sums['entries_appended'] == (raw_block.nnz if with_block else 0)
        else:
            assert sums['entries'] == T1 * OH.N and sums['entries_retired'] == retire * OH.N
        m2 = s.download()
        # W[retire:] followed by the AR roll-out of the block (the bits of Model.latent_forecast); H and the lag weights stay
        warm = make_model(W1[retire:], H1, Th1, d['lag_set']).latent_forecast(Tn)
        assert np.array_equal(m2.W, warm) and np.array_equal(m2.H, H1) and np.array_equal(m2.lag_val, Th1)
        with pytest.raises(RuntimeError, match='rewind'):
            s.rewind()
        got = _after(s, T1)
        if retire == 0:             # ... and must be append_rows
            with Session(head, _model(d, dtype, W=W1, H=H1, theta=Th1), missing=missing, **HYPER) as a:
                if tr is not None:
                    a.set_transform(tr)
                a.append_rows(block)
                a.model = make_model(warm, H1, Th1, d['lag_set'])
                _assert_same(got, _after(a, T1), form + ' append_rows')
    if raw_head is not None:
        fresh_Y = SH.slid(raw_head, retire, raw_block).pymatrix()
    else:
        fresh_Y = np.ascontiguousarray(np.vstack([SH.dense_rows(k, retire, T0, dtype)] + ([block] if with_block else [])))
    with Session(fresh_Y, make_model(warm, H1, Th1, d['lag_set']), missing=missing, **HYPER) as f:
        if tr is not None:
            f.set_transform(tr)
        _assert_same(got, _after(f, T1), form + ' fresh')


# ---- 2. the column shapes of the compaction ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_every_column_shape_is_compacted_stably(dtype):
    """Columns of 0, 1, 63, 64, 65 and 130 entries (and one of 140 with repeated cells), each losing none, all and an interleaved
    part of its entries: the F-solve adds a column's entries in stored order in the element type, so the trained factors tell a
    compaction that kept another order (or lost an entry) from the fresh session's arrays."""
    raw = SH.shape_problem(np.dtype(dtype))
    T, n = raw.shape
    k = 7
    rng = np.random.RandomState(2)
    W0, H0 = rng.rand(T, k).astype(dtype), rng.rand(n, k).astype(dtype)
    Th0 = np.asfortranarray((rng.randn(2, k) / 3).astype(dtype))
    lags = [1, 3]
    outs = []
    with Session(raw.pymatrix(), make_model(W0, H0, Th0, lags), missing=True, **HYPER) as s:
        sums = s.retire_rows(SH.SHAPE_RETIRE)
        assert sums['entries'] == np.count_nonzero(raw.rows >= SH.SHAPE_RETIRE) and s.rows() == T - SH.SHAPE_RETIRE
        s.run(2); m = s.download(); outs.append((m.W.copy(), m.H.copy(), m.lag_val.copy(), s.objective()))
    want = SH.slid(raw, SH.SHAPE_RETIRE)
    lens = np.diff(want.col_ptr.astype(np.int64))
    j = 0
    for L in SH.SHAPE_LENGTHS:          # the design holds: none / all / a part of every length retired
        assert lens[j] == L and lens[j + 1] == 0 and (0 < lens[j + 2] < L or L <= 1)
        j += 3
    with Session(want.pymatrix(), make_model(W0[SH.SHAPE_RETIRE:], H0, Th0, lags), missing=True, **HYPER) as f:
        f.run(2); m = f.download(); outs.append((m.W.copy(), m.H.copy(), m.lag_val.copy(), f.objective()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---- 3. failure atomicity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage,missing', [('sparse', True), ('sparse', False), ('dense', False)], ids=['sparse-missing', 'sparse-full', 'dense'])
def test_a_refused_slide_leaves_the_session_as_it_was(storage, missing):
    from ctypes import byref
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    head, _ = _rows(k, 0, SH.T0, dtype, storage)
    block, _ = _rows(k, SH.T0, OH.T, dtype, storage)
    other, _ = _rows(k, SH.T0, OH.T, dtype, 'dense' if storage == 'sparse' else 'sparse')
    narrow = PyMatrix(np.ascontiguousarray(np.zeros((3, OH.N - 1), dtype=dtype)), dtype) if storage == 'dense' else \
        RawSparse(np.array([0]), np.array([0]), np.array([1.0]), (3, OH.N - 1), dtype).pymatrix()
    as_pm = lambda b: b if isinstance(b, PyMatrix) else PyMatrix(b, dtype=dtype)
    with Session(head, _model(d, dtype, W=d['W'][:SH.T0]), missing=missing, **HYPER) as s:
        s.run(1)
        m = s.download()
        before = (m.W.copy(), m.H.copy(), m.lag_val.copy())

        def refused(blk, retire, downdate, text):
            rc = s.lib.trmf_session_slide(s.handle, byref(as_pm(blk)) if blk is not None else None, retire, downdate, None)
            assert rc < 0 and text in s.lib.trmf_last_error().decode(), (text, s.lib.trmf_last_error().decode())
            assert s.rows() == SH.T0
            m = s.download()
            assert np.array_equal(m.W, before[0]) and np.array_equal(m.H, before[1]) and np.array_equal(m.lag_val, before[2])

        refused(None, -1, 0, 'negative')
        refused(None, SH.T0 - REACH, 0, 'largest lag + 1')                     # REACH rows left: one too few
        refused(block, SH.T0 + 1, 0, 'cannot retire')
        refused(narrow, 1, 0, 'column count')
        refused(other, 1, 0, 'storage class')
        refused(None, 1, 2, 'downdate_stats must be 0 or 1')
        refused(None, 1, 1, 'full-observation' if not missing else 'without valid series statistics')
        s.init_series_stats(1.0)
        if not missing:
            refused(None, 1, 1, 'full-observation')                            # one shared S: no per-series downdate
        else:
            s.run(1); s.sync()                                                 # stale statistics
            before = tuple(a.copy() for a in (s.download().W, s.model.H, s.model.lag_val))
            refused(None, 1, 1, 'without valid series statistics')
        with pytest.raises(ValueError, match='negative'):
            s.slide(None, -1)
        # ... and a valid slide still works: REACH + 1 rows is the fewest a session may keep
        assert s.slide(None, 1)['rows'] == SH.T0 - 1
        assert np.array_equal(s.download().W, before[0][1:])
        s.run(1).sync()
        assert s.retire_rows(SH.T0 - 1 - (REACH + 1))['rows'] == REACH + 1 == s.rows()


# ---- 4. the held-out set ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
def test_heldout_set_follows_the_slide(dtype, k):
    """Positions in retired rows are dropped, the others move up: the sums (and the predictions, in the set's order) of a fresh
    set_heldout of the shifted set.  4200 positions: more than one chunk of the compaction."""
    import scipy.sparse as smat
    d = OH.inputs(k)
    rng = np.random.RandomState(8)
    held = smat.csr_matrix((rng.rand(SH.T0, OH.N) + 0.5).astype(dtype))
    assert held.nnz == SH.T0 * OH.N > 4096
    head, raw_head = _rows(k, 0, SH.T0, dtype, 'sparse')
    block, raw_block = _rows(k, SH.T0, OH.T, dtype, 'sparse')
    with Session(head, _model(d, dtype, W=d['W'][:SH.T0]), missing=True, **HYPER) as s:
        s.run(1).set_heldout(held)
        s.slide(block, SH.RETIRE)
        got, pred = s.eval_heldout_sums(predictions=True)
        m = s.download()
        W, H, Th = m.W.copy(), m.H.copy(), m.lag_val.copy()
    with Session(SH.slid(raw_head, SH.RETIRE, raw_block).pymatrix(), make_model(W, H, Th, d['lag_set']), missing=True, **HYPER) as f:
        f.set_heldout(held[SH.RETIRE:])
        want, wpred = f.eval_heldout_sums(predictions=True)
    assert got == want and got['count'] == (SH.T0 - SH.RETIRE) * OH.N
    assert np.array_equal(pred, wpred)


# ---- 5. the statistics --------------------------------------------------------------------------------------------------------
def _stats_sequence(k, dtype, lamI, gamma, retire, downdate):
    """init on 72 rows, 12 rows absorbed, `retire` rows retired, 12 rows absorbed: (W, H, info, sums of the slide)."""
    d = OH.inputs(k)
    hyper = dict(HYPER, lambdaI=lamI)
    with Session(_rows(k, 0, OH.FIRST, dtype, 'sparse')[0], _model(d, dtype, W=d['W'][:OH.FIRST]), missing=True, **hyper) as s:
        s.init_series_stats(gamma)
        s.update(_rows(k, OH.FIRST, SH.T0, dtype, 'sparse')[0], adapt=True)
        Wold = s.download().W.copy()
        sums = None
        if retire:
            sums = s.slide(None, retire, downdate)
            info = s.series_stats_info()
            assert info['valid'] and info['absorbed_rows'] == SH.T0 - retire and info['forget'] == gamma
        s.update(_rows(k, SH.T0, OH.T, dtype, 'sparse')[0], adapt=True)
        m = s.download()
        return dict(W=m.W.copy(), H=m.H.copy(), Wold=Wold, info=s.series_stats_info(), sums=sums)


@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('gamma', [1.0, 0.95])
def test_downdated_statistics_fit_the_retained_rows(gamma, dtype, k):
    """downdate_stats=True: adapt_series after the slide against series_ridge in fp64 on the retained rows of the session's own W,
    no farther than 8x the fp32 NumPy twin of the same recursion (scaled by eps64 / eps32 for fp64).  30 of the 84 absorbed rows
    leave: fewer than half."""
    lamI = 0.5
    got = _stats_sequence(k, dtype, lamI, gamma, SH.STATS_RETIRE, True)
    assert got['info']['absorbed_rows'] == OH.T - SH.STATS_RETIRE and np.array_equal(got['W'][:SH.T0 - SH.STATS_RETIRE], got['Wold'][SH.STATS_RETIRE:])
    Wfull = np.vstack([got['Wold'][:SH.STATS_RETIRE], got['W']])              # the 96 rows as the statistics saw them
    ref = SH.downdate_direct(Wfull, k, lamI, gamma)
    yard = relmax(SH.downdate_twin(Wfull, k, np.float32, gamma).solve(lamI), ref)
    b, err = AH.bound(dtype, yard), relmax(got['H'], ref)
    evidence('sliding window downdate %s k=%d gamma=%g: relmax to the fp64 direct ridge on the retained rows %.3e = %.2f x its bound %.3e (fp32 twin %.3e)'
             % (np.dtype(dtype).name, k, gamma, err, err / b, b, yard))
    assert err <= b
    # the downdate did something: without it the retired rows still pull
    keep = _stats_sequence(k, dtype, lamI, gamma, SH.STATS_RETIRE, False)
    assert not np.array_equal(keep['H'], got['H'])


@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
def test_statistics_without_downdate_are_those_without_retirement(dtype, k):
    """downdate_stats=False: the tables keep the retired rows as forgotten history, so H after adapt_series -- the tables' ridge
    solution; the tables themselves cannot be downloaded -- and the filtered rows are bit for bit those of the same sequence
    without retirement."""
    slid = _stats_sequence(k, dtype, 0.5, 0.95, SH.STATS_RETIRE, False)
    plain = _stats_sequence(k, dtype, 0.5, 0.95, 0, False)
    assert np.array_equal(slid['H'], plain['H']) and np.array_equal(slid['W'], plain['W'][SH.STATS_RETIRE:])
    assert slid['info']['absorbed_rows'] == OH.T - SH.STATS_RETIRE and plain['info']['absorbed_rows'] == OH.T


def test_retiring_past_the_absorbed_rows_makes_the_statistics_stale():
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    with Session(_rows(k, 0, OH.FIRST, dtype, 'sparse')[0], _model(d, dtype, W=d['W'][:OH.FIRST]), missing=True, **HYPER) as s:
        s.init_series_stats(1.0)
        s.append_rows(_rows(k, OH.FIRST, SH.T0, dtype, 'sparse')[0])           # 84 rows, 72 absorbed
        s.model = _model(d, dtype, W=d['W'][:SH.T0])
        s.retire_rows(OH.FIRST - 2)
        info = s.series_stats_info()
        assert info['valid'] and info['absorbed_rows'] == 2
        s.retire_rows(3)                                                       # one row the tables never absorbed
        info = s.series_stats_info()
        assert info['stale'] and not info['valid']
        with pytest.raises(RuntimeError, match='series statistics'):
            s.adapt_series()
        s.retire_rows(1)
        assert s.series_stats_info()['stale']                                  # stale tables stay stale


# ---- 6. update(window=N) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['sparse-missing', 'dense'])
def test_update_with_a_window_is_slide_plus_assimilate(storage, missing):
    """30 ticks of one row at N = 40: rows() stays at N and the session ends bit for bit where explicit slide + assimilate calls
    end.  Device memory does not grow: the pool's live bytes after tick 10 and after tick 30 are equal (a sparse row's entry count
    changes from tick to tick by a few entries, which stays inside the pool's block granularity on this input)."""
    dtype, k, N = np.float32, 7, 40
    d = OH.inputs(k)
    ticks = [_rows(k, t, t + 1, dtype, storage)[0] for t in range(N, N + 30)]
    live = {}
    with Session(_rows(k, 0, N, dtype, storage)[0], _model(d, dtype, W=d['W'][:N]), missing=missing, **HYPER) as s:
        for i, row in enumerate(ticks, 1):
            sums = s.update(row, window=N)
            assert s.rows() == N and sums['rows'] == 1
            if i in (10, 30):
                live[i] = s.pool_live_bytes()
        m = s.download()
        got = (m.W.copy(), m.H.copy(), m.lag_val.copy())
        with pytest.raises(ValueError, match='smaller than the block'):
            s.update(ticks[0], window=REACH + 1)
        assert s.rows() == N
    evidence('sliding window %s: pool live bytes after tick 10 %d, after tick 30 %d' % (storage, live[10], live[30]))
    assert live[10] == live[30] > 0
    with Session(_rows(k, 0, N, dtype, storage)[0], _model(d, dtype, W=d['W'][:N]), missing=missing, **HYPER) as s:
        for row in ticks:
            s.slide(row, 1)
            s.assimilate(N - 1)
        m = s.download()
        assert np.array_equal(m.W, got[0]) and np.array_equal(m.H, got[1]) and np.array_equal(m.lag_val, got[2])
    assert not np.array_equal(got[0], d['W'][30:30 + N].astype(dtype))          # (the filter moved the rows)


# ---- 7. two virtual ranks -----------------------------------------------------------------------------------------------------
def test_two_virtual_ranks_slide_to_the_bits_of_one_rank(monkeypatch):
    """TRMF_DEVICES=0,0: every rank makes the same call and ends with the same bits as one rank in the tile geometry several ranks
    use (TRMF_TEST=1 TRMF_TILE=narrow, tests/test_gpu_devices.py)."""
    dtype, k = np.float32, 40
    d = OH.inputs(k)

    def once():
        with Session(_rows(k, 0, SH.T0, dtype, 'sparse')[0], _model(d, dtype, W=d['W'][:SH.T0]), missing=True, **HYPER) as s:
            s.run(2)
            s.init_series_stats(0.95)
            sums = s.slide(_rows(k, SH.T0, OH.T, dtype, 'sparse')[0], SH.RETIRE, True)
            a = s.assimilate(OH.T - SH.RETIRE - 12)
            ad = s.adapt_series()
            s.run(2)
            m = s.download()
            return sums, a, ad, m.W.copy(), m.H.copy(), m.lag_val.copy()

    monkeypatch.setenv('TRMF_TEST', '1')
    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = once()
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two = once()
    assert one[0] == two[0] and one[1] == two[1] and one[2] == two[2]
    for a, b in zip(one[3:], two[3:]):
        assert np.array_equal(a, b)


# ---- 8. rolling_validate(update='assimilate', window=N) -------------------------------------------------------------------------
def test_rolling_validate_with_a_window_is_the_loop_by_hand():
    from trmf import Metrics
    from trmf.model import Model
    rng = np.random.RandomState(4)
    T, n, k, ws, nw, N = 120, 12, 4, 6, 4, 80
    lags = [1, 2, 5]
    Y = np.ascontiguousarray((rng.rand(T, n) + 0.1).astype(np.float32))
    kw = dict(k=k, window_size=ws, nr_windows=nw, lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5, max_iter=3, missing=False, seed=3)
    got = trmf.rolling_validate(Y, lags, update='assimilate', window=N, **kw)
    grow = trmf.rolling_validate(Y, lags, update='assimilate', **kw)
    cuts = [T - nw * ws + i * ws for i in range(nw)]
    forecasts = np.zeros((nw * ws, n), dtype=Y.dtype)
    model = Model.initialize(Y[:cuts[0]], lags, k, seed=3)
    with Session(Y[:cuts[0]], model, missing=False, lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5, log_norms=False, timing=0) as s:
        s.run(3).download()
        model.forecast(ws, Ynew=forecasts[:ws], threshold=0)
        for i in range(1, nw):
            s.update(Y[cuts[i - 1]:cuts[i]], window=N)
            assert s.rows() == min(N, cuts[i])
            s.download().forecast(ws, Ynew=forecasts[i * ws:(i + 1) * ws], threshold=0)
    want = Metrics.generate(Y[T - nw * ws:], forecasts, missing=False)
    assert got == want
    assert isinstance(grow, type(got))
