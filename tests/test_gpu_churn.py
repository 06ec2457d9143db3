"""GPU (-m gpu): series churn on the device -- trmf_session_change_series (csr_churn_count_kernel, csr_churn_kernel,
csc_gather_kernel, dense_churn_kernel, row_gather_kernel and the adapt kernels over the new columns) behind Session.change_series /
add_series / retire_series.  Small shapes (tests/churn_helpers.py): T = 96, 38 resident series, 12 new ones.

The contract is bit-identity: after a churn the session IS the session trmf_session_create builds from the churned entries in their
stored order (churn_helpers.churned = trmf.churn_entries on both orientations), the current W and lag weights and
H = [H[keep]; H_new], so every later call returns the same bits on both.  Only the cold-start fit is held to a yardstick instead
(adapt_helpers.bound / row_bound: 8x an fp32 NumPy twin of the same recursion against the fp64 direct ridge)."""
import copy
from ctypes import byref

import numpy as np
import pytest

import adapt_helpers as AH
import churn_helpers as CH
import online_helpers as OH
import slide_helpers as SH
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
SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}             # tests/test_gpu_adapt.py's


def _model(d, dtype, n=CH.N0, W=None, H=None, theta=None, rows=OH.T):
    m = make_model((d['W'][:rows] if W is None else W).astype(dtype), (d['H'][:n] if H is None else H).astype(dtype),
                   (d['theta'] if theta is None else theta).astype(dtype), d['lag_set'])
    if m.k == 1:        # PyMatrix tags a (rows, 1) array column-major; the two orders are the same bytes
        m.pyW.type = m.pyH.type = PyMatrix.DENSE_ROWMAJOR
    return m


def _cols(k, lo, hi, dtype, storage):
    """Series lo..hi-1 as a session takes them: (what Session gets, the RawSparse behind it or None)."""
    if storage == 'dense':
        return CH.dense_cols(k, lo, hi, dtype), None
    raw = CH.raw_cols(k, lo, hi, dtype, SEED)
    return raw.pymatrix(), raw


# ---- 1. equals a fresh session, bit for bit -----------------------------------------------------------------------------------
FORMS = [('sparse-missing', 'sparse', True, False), ('sparse-full', 'sparse', False, False), ('dense', 'dense', False, False),
         ('dense-transform', 'dense', False, True)]
MODES = [('retire-only', True, False), ('add-only', False, True), ('both', True, True)]


def _churn_case(form, storage, missing, transform, retire, add, dtype, k, fit=True, Hgiven=None, compare=CH.after):
    """One session through run(1) + change_series, one fresh session on the churned arrays: (what the first gives, what the
    second gives, the sums)."""
    d = OH.inputs(k)
    keep = CH.keep_mask() if retire else None
    nk = int(keep.sum()) if retire else CH.N0
    head, raw_head = _cols(k, 0, CH.N0, dtype, storage)
    block, raw_block = _cols(k, CH.N0, OH.N, dtype, storage) if add else (None, None)
    tr = NormalizedTransform(CH.dense_cols(k, 0, CH.N0, dtype)) if transform else None
    trn = NormalizedTransform(CH.dense_cols(k, CH.N0, OH.N, dtype)) if transform and add else None
    with Session(head, _model(d, dtype), missing=missing, **HYPER) as s:
        if tr is not None:
            s.model.transform = tr
            s.set_transform(tr)
        s.run(1)
        m1 = s.download()
        W1, H1, Th1 = m1.W.copy(), m1.H.copy(), m1.lag_val.copy()
        s.mark()
        sums = s.change_series(keep, block, fit=fit, H=Hgiven, transform_new=trn)
        n1 = nk + (CH.M if add else 0)
        assert s.model.n == n1 and s.rows() == OH.T
        assert (sums['series_before'], sums['series_retired'], sums['series_added'], sums['series']) == (CH.N0, CH.N0 - nk, CH.M if add else 0, n1)
        assert sums['fitted'] == (add and fit) and not sums['stats_carried'] and sums['heldout_dropped'] == 0
        if raw_head is not None:
            want = CH.churned(raw_head, keep, raw_block)
            assert sums['entries'] == want.nnz and sums['entries_added'] == (raw_block.nnz if add else 0)
            assert sums['entries_retired'] == (np.count_nonzero(~keep[raw_head.cols]) if retire else 0)
        else:
            assert sums['entries'] == OH.T * n1 and sums['entries_retired'] == OH.T * (CH.N0 - nk) and sums['entries_added'] == OH.T * (n1 - nk)
        m2 = s.download()
        # W, the lag weights and the kept rows of H are the same bits
        assert np.array_equal(m2.W, W1) and np.array_equal(m2.lag_val, Th1)
        assert np.array_equal(m2.H[:nk], H1[keep] if retire else H1)
        H2 = m2.H.copy()
        if add and not fit:
            assert np.array_equal(H2[nk:], Hgiven if Hgiven is not None else np.zeros((CH.M, k), dtype))
        with pytest.raises(RuntimeError, match='rewind'):
            s.rewind()
        tr2 = s.model.transform
        got = compare(s, OH.T)
    if raw_head is not None:
        fresh_Y = CH.churned(raw_head, keep, raw_block).pymatrix()
    else:
        fresh_Y = np.ascontiguousarray(np.hstack([CH.dense_cols(k, 0, CH.N0, dtype)[:, keep if retire else slice(None)]] + ([block] if add else [])))
    with Session(fresh_Y, make_model(W1, H2, Th1, d['lag_set']), missing=missing, **HYPER) as f:
        if tr2 is not None:
            assert tr2.a.shape == (1, n1)
            f.set_transform(tr2)
        return got, compare(f, OH.T), sums


@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('mode,retire,add', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('form,storage,missing,transform', FORMS, ids=[f[0] for f in FORMS])
def test_churn_equals_a_fresh_session(form, storage, missing, transform, mode, retire, add, dtype, k):
    """The sparse input is not canonical: neither orientation is sorted, two cells are stored twice (one of them in a retired
    series).  The retired set holds the first series, the last one, two neighbours and the series with the doubled cell."""
    got, want, _ = _churn_case(form, storage, missing, transform, retire, add, dtype, k)
    CH.assert_same(got, want, form + ' ' + mode)


def _after_generic(s, T1):
    """What a session of rank above 64 offers: iterations with their CG counts, the objective, a forecast."""
    out = {}
    s.run(3)
    out['cg'] = [x['cg_iter'] for x in s.stats(3)]
    m = s.download()
    out['W'], out['H'], out['theta'] = m.W.copy(), m.H.copy(), m.lag_val.copy()
    out['J'] = np.float64(s.objective())
    out['Y5'], out['W5'] = s.forecast(5, return_latent=True)
    return out


def test_churn_at_rank_72_without_the_fit():
    """The structural change works at every rank: k = 72 runs the generic kernels; the new loadings are the caller's."""
    k = 72
    Hn = np.ascontiguousarray(np.random.RandomState(3).rand(CH.M, k).astype(np.float32))
    got, want, sums = _churn_case('sparse-missing', 'sparse', True, False, True, True, np.float32, k, fit=False, Hgiven=Hn, compare=_after_generic)
    CH.assert_same(got, want, 'k=72')
    assert sums['sq_err_new'] == 0.0 and not sums['fitted']


# ---- 2. every row shape is compacted stably -----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_every_row_shape_is_compacted_stably(dtype):
    """Rows of 0, 1, 63, 64, 65 and 130 entries (and one of 140 with repeated cells), each losing none, all and an interleaved part
    of its series, with and without a block whose rows hold 0, 1 and 65 entries: the X-side Gram adds a row's entries in stored
    order in the element type, so the trained factors tell a compaction that kept another order (or lost an entry) from the
    fresh session's arrays."""
    raw, blk = CH.shape_problem(np.dtype(dtype))
    T, n = raw.shape
    k, lags = 7, [1, 3]
    rng = np.random.RandomState(2)
    W0, H0 = rng.rand(T, k).astype(dtype), rng.rand(n, k).astype(dtype)
    Th0 = np.asfortranarray((rng.randn(2, k) / 3).astype(dtype))
    lens = np.diff(raw.row_ptr.astype(np.int64))
    assert lens.tolist() == list(CH.SHAPE_LENGTHS + CH.SHAPE_LENGTHS[1:]) + [140]
    assert np.diff(blk.row_ptr.astype(np.int64)).tolist() == list(CH.SHAPE_BLOCK_LENGTHS) * 4
    for name, keep in CH.shape_keeps().items():
        for with_block in (False, True):
            if not with_block and name in ('none', 'all'):
                continue                                    # nothing to do / refused
            want = CH.churned(raw, keep, blk if with_block else None)
            if name == 'mixed':                             # the design holds: a part of every row of more than one entry leaves
                kl = np.diff(CH.churned(raw, keep).row_ptr.astype(np.int64))
                assert all(0 < a < b for a, b in zip(kl, lens) if b > 1)
            outs = []
            with Session(raw.pymatrix(), make_model(W0, H0, Th0, lags), missing=True, **HYPER) as s:
                sums = s.change_series(keep, blk.pymatrix() if with_block else None)
                assert sums['entries'] == want.nnz and s.model.n == want.shape[1]
                H1 = s.download().H.copy()
                s.run(2); m = s.download(); outs.append((m.W.copy(), m.H.copy(), m.lag_val.copy(), s.objective()))
            with Session(want.pymatrix(), make_model(W0, H1, Th0, lags), missing=True, **HYPER) as f:
                f.run(2); m = f.download(); outs.append((m.W.copy(), m.H.copy(), m.lag_val.copy(), f.objective()))
            for a, b in zip(*outs):
                assert np.array_equal(a, b), (name, with_block)


# ---- 3. the cold-start fit ------------------------------------------------------------------------------------------------------
STORAGES = [('sparse-missing', 'sparse', True), ('sparse-full', 'sparse', False), ('dense', 'dense', False)]


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('name,storage,missing', STORAGES, ids=[s[0] for s in STORAGES])
@pytest.mark.parametrize('lamI,gamma', AH.CASES, ids=['lamI%g-gamma%g' % c for c in AH.CASES])
@pytest.mark.parametrize('k', OH.RANKS)
def test_cold_start_fit_matches_the_direct_ridge(k, lamI, gamma, name, storage, missing, dtype):
    """Designed new series -- no entry, one, exactly 64, 65, all 96, a cell stored twice -- in canonical and in random stored orders.
    gamma < 1: the session holds valid, fully absorbed statistics built with it; they are carried where they are per series (sparse
    storage with missing) and the fit then weights by gamma; on the full-observation forms they go stale and the fit is unweighted."""
    d = OH.inputs(k)
    hyper = dict(HYPER, lambdaI=lamI)
    carried = gamma != 1.0 and missing
    g_fit = gamma if carried else 1.0
    for seed in ((None, 5) if storage == 'sparse' else (None,)):
        rawn = CH.fit_raw(k, dtype, seed) if storage == 'sparse' else None
        Ynew = rawn if storage == 'sparse' else CH.fit_dense(k, dtype)
        with Session(_cols(k, 0, CH.N0, dtype, storage)[0], _model(d, dtype), missing=missing, **hyper) as s:
            if gamma != 1.0:
                s.init_series_stats(gamma)
            sums = s.add_series(rawn.pymatrix() if rawn is not None else Ynew)
            info = s.series_stats_info()
            H = s.download().H.copy()
        assert sums['fitted'] and sums['stats_carried'] == carried and sums['series'] == CH.N0 + CH.FIT_M
        if gamma != 1.0:
            assert info == (dict(valid=True, stale=False, absorbed_rows=OH.T, forget=gamma) if carried else dict(info, valid=False, stale=True))
        Hn = H[CH.N0:]
        assert np.array_equal(H[:CH.N0], d['H'][:CH.N0].astype(dtype))
        ref, yard, twin_rows = CH.fit_yardstick(d['W'], Ynew, lamI, g_fit, missing)
        b, got = AH.bound(dtype, yard), relmax(Hn, ref)
        own = AH.own_scale(Hn, ref)
        evidence('cold-start fit %s %s k=%d lambdaI=%g gamma=%g order=%s: relmax to the fp64 direct ridge %.3e = %.2f x its bound %.3e (fp32 twin %.3e); '
                 'worst designed series on its own scale %.2f x' % (name, np.dtype(dtype).name, k, lamI, g_fit, 'canonical' if seed is None else 'random', got, got / b, b,
                                                                    yard, max(own[j] / AH.row_bound(dtype, k, twin_rows[j]) for j in range(1, len(CH.FIT_LENGTHS) + 1))))
        assert got <= b, (name, seed, got, b)
        assert not Hn[0].any()                                                # no entry: h = 0 exactly (lambdaI > 0)
        for j in range(1, len(CH.FIT_LENGTHS) + 1):
            assert own[j] <= AH.row_bound(dtype, k, twin_rows[j]), (name, seed, 'series', j, own[j], AH.row_bound(dtype, k, twin_rows[j]))
        want = CH.fit_sq_err(Ynew, d['W'].astype(dtype), Hn)
        assert abs(sums['sq_err_new'] - want) <= SUM_TOL[dtype] * want, (sums['sq_err_new'], want)


@pytest.mark.parametrize('chunk', [None, '8'], ids=['whole-columns', 'items-of-8'])
@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
def test_carried_statistics_continue_as_a_fresh_init(dtype, k, chunk, monkeypatch):
    """Valid, fully absorbed tables with gamma = 0.95: after retiring and adding series they are still valid, and the next
    update(adapt=True) gives the bits of the same call on a fresh session that ran init_series_stats(0.95) on the churned data.
    TRMF_ADAPT_CHUNK=8: the init pass -- and with it the cold-start fit -- cuts every column into items of 8 entries."""
    if chunk is not None:
        monkeypatch.setenv('TRMF_ADAPT_CHUNK', chunk)
    d = OH.inputs(k)
    T0, gamma = SH.T0, 0.95
    keep = CH.keep_mask()
    series = list(np.flatnonzero(keep)) + list(range(CH.N0, OH.N))
    head = CH.raw_part(k, 0, T0, range(CH.N0), dtype, SEED)
    blk = CH.raw_part(k, 0, T0, range(CH.N0, OH.N), dtype, SEED)
    tail = CH.raw_part(k, T0, OH.T, series, dtype, SEED)
    outs = []
    with Session(head.pymatrix(), _model(d, dtype, rows=T0), missing=True, **HYPER) as s:
        s.init_series_stats(gamma)
        sums = s.change_series(keep, blk.pymatrix())
        assert sums['stats_carried'] and sums['fitted']
        assert s.series_stats_info() == dict(valid=True, stale=False, absorbed_rows=T0, forget=gamma)
        m = s.download()
        W1, H1, Th1 = m.W.copy(), m.H.copy(), m.lag_val.copy()
        a, ad = s.update(tail.pymatrix(), adapt=True)
        m = s.download()
        outs.append((a, ad, m.W.copy(), m.H.copy()))
    with Session(CH.churned(head, keep, blk).pymatrix(), make_model(W1, H1, Th1, d['lag_set']), missing=True, **HYPER) as f:
        f.init_series_stats(gamma)
        a, ad = f.update(tail.pymatrix(), adapt=True)
        m = f.download()
        outs.append((a, ad, m.W.copy(), m.H.copy()))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][2], outs[1][2]) and np.array_equal(outs[0][3], outs[1][3])
    assert not np.array_equal(outs[0][3], H1)                                  # (the update moved the loadings)


def test_statistics_that_lag_behind_go_stale():
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    with Session(CH.raw_part(k, 0, OH.FIRST, range(CH.N0), dtype, SEED).pymatrix(), _model(d, dtype, rows=OH.FIRST), missing=True, **HYPER) as s:
        s.init_series_stats(0.95)
        s.append_rows(CH.raw_part(k, OH.FIRST, SH.T0, range(CH.N0), dtype, SEED).pymatrix())      # 84 rows, 72 absorbed
        s.model = _model(d, dtype, rows=SH.T0)
        sums = s.add_series(CH.raw_part(k, 0, SH.T0, range(CH.N0, OH.N), dtype, SEED).pymatrix())
        info = s.series_stats_info()
        assert not sums['stats_carried'] and info['stale'] and not info['valid']
        with pytest.raises(RuntimeError, match='series statistics'):
            s.adapt_series()
        s.init_series_stats(0.95)                                              # ... and can be built again for the new series count
        assert s.series_stats_info()['valid'] and s.adapt_series()['series'] == OH.N


def test_a_new_series_that_cannot_be_fitted_is_refused():
    """lambdaI == 0: a new series without entries has a singular system; the message names it and nothing changes."""
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    with Session(_cols(k, 0, CH.N0, dtype, 'sparse')[0], _model(d, dtype), missing=True, **dict(HYPER, lambdaI=0.0)) as s:
        with pytest.raises(RuntimeError, match='new series 0'):
            s.add_series(CH.fit_raw(k, dtype, 5).pymatrix())
        assert s.model.n == CH.N0 and np.array_equal(s.download().H, d['H'][:CH.N0].astype(dtype))
        s.run(1).sync()


# ---- 4. held-out set, scores and noise ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
def test_heldout_scores_and_noise_follow_the_churn(dtype, k):
    """Held-out positions of retired series are dropped, the others renumbered (7296 positions: more than one chunk of the
    compaction); the score tables read zero rows; the noise must be fitted again; the mark is gone."""
    d = OH.inputs(k)
    rng = np.random.RandomState(8)
    rr, cc = np.divmod(np.arange(OH.T * CH.N0), CH.N0)
    held = RawSparse(np.tile(rr, 2), np.tile(cc, 2), rng.rand(2 * rr.size) + 0.5, (OH.T, CH.N0), dtype, seed=4)
    assert held.nnz > 4096
    keep = CH.keep_mask()
    head, raw_head = _cols(k, 0, CH.N0, dtype, 'sparse')
    block, raw_block = _cols(k, CH.N0, OH.N, dtype, 'sparse')
    truth = np.ascontiguousarray((rng.rand(3, CH.N0) + 0.1).astype(dtype))
    with Session(head, _model(d, dtype), missing=True, **HYPER) as s:
        s.run(1).set_heldout(held.pymatrix())
        s.fit_noise()
        s.forecast(3, truth=truth); s.forecast_dist(3, truth=truth)
        assert s.forecast_series_sums()[0] == 3 and s.interval_series_sums()[0] == 3
        s.mark()
        sums = s.change_series(keep, block)
        assert sums['heldout_dropped'] == np.count_nonzero(~keep[held.cols])
        got, pred = s.eval_heldout_sums(predictions=True)
        rows_f, table_f = s.forecast_series_sums()
        rows_i, table_i = s.interval_series_sums()
        assert rows_f == 0 and rows_i == 0 and not table_f.any() and not table_i.any() and table_f.shape[0] == s.model.n
        with pytest.raises(RuntimeError, match='noise'):
            s.noise()
        with pytest.raises(RuntimeError, match='noise'):
            s.forecast_dist(3)
        with pytest.raises(RuntimeError, match='rewind'):
            s.rewind()
        s.fit_noise()
        assert s.noise()[0].shape == (s.model.n,)
        m = s.download()
        W, H, Th = m.W.copy(), m.H.copy(), m.lag_val.copy()
    with Session(CH.churned(raw_head, keep, raw_block).pymatrix(), make_model(W, H, Th, d['lag_set']), missing=True, **HYPER) as f:
        none = RawSparse(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), (OH.T, CH.M), dtype)     # (the held-out set gains no cells)
        f.set_heldout(CH.churned(held, keep, none).pymatrix())
        want, wpred = f.eval_heldout_sums(predictions=True)
    assert got == want and got['count'] == 2 * OH.T * int(keep.sum())
    assert np.array_equal(pred, wpred)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def _forged(raw, **fields):
    """A PyMatrix over `raw` with header fields overwritten (the arrays stay as they are)."""
    pm = raw.pymatrix()
    for name, value in fields.items():
        setattr(pm, name, value)
    return pm


@pytest.mark.parametrize('storage,missing', [('sparse', True), ('sparse', False), ('dense', False)], ids=['sparse-missing', 'sparse-full', 'dense'])
def test_a_refused_churn_leaves_the_session_as_it_was(storage, missing):
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    head, _ = _cols(k, 0, CH.N0, dtype, storage)
    block, raw_block = _cols(k, CH.N0, OH.N, dtype, storage)
    other, _ = _cols(k, CH.N0, OH.N, dtype, 'dense' if storage == 'sparse' else 'sparse')
    short = PyMatrix(np.ascontiguousarray(np.zeros((OH.T - 1, 3), dtype=dtype)), dtype) if storage == 'dense' else \
        RawSparse(np.array([0]), np.array([0]), np.array([1.0]), (OH.T - 1, 3), dtype).pymatrix()
    as_pm = lambda b: b if isinstance(b, PyMatrix) else PyMatrix(b, dtype=dtype)
    Hn = np.zeros((CH.M, k), dtype=dtype)
    coef = np.ones(CH.M, dtype=dtype)
    zeros = np.zeros(CH.N0, dtype=np.uint8)
    with Session(head, _model(d, dtype), missing=missing, **HYPER) as s, Session(head, _model(d, dtype), missing=missing, **HYPER) as twin:
        for x in (s, twin):
            x.run(1)
            x.init_series_stats(0.95)

        def refused(keep, blk, fit, H, ta, tb, text):
            ptr = lambda a: a.ctypes.data if a is not None else None
            rc = s.lib.trmf_session_change_series(s.handle, ptr(keep), byref(as_pm(blk)) if blk is not None else None, fit, ptr(H), ptr(ta), ptr(tb), None)
            assert rc < 0 and text in s.lib.trmf_last_error().decode(), (text, s.lib.trmf_last_error().decode())

        refused(zeros, None, 1, None, None, None, 'no series would be left')
        refused(None, short, 1, None, None, None, 'rows, the session holds')
        refused(None, other, 1, None, None, None, 'storage class')
        refused(None, block, 1, Hn, None, None, 'fit together with Hnew')
        refused(None, block, 2, None, None, None, 'fit must be 0 or 1')
        refused(None, block, 1, None, coef, coef, 'no series transform is set')
        if storage == 'sparse':
            big = 1 << 32
            rp, cp = raw_block.row_ptr.copy(), raw_block.col_ptr.copy()
            rp[-1] = cp[-1] = big
            forged = _forged(raw_block, nnz=big)
            forged.py_buf = dict(forged.py_buf, row_ptr=rp, col_ptr=cp)
            ctype_of = dict(PyMatrix._fields_)
            forged.row_ptr = rp.ctypes.data_as(ctype_of['row_ptr']); forged.col_ptr = cp.ctypes.data_as(ctype_of['col_ptr'])
            refused(None, forged, 1, None, None, None, '32-bit device indices')
            refused(None, _forged(raw_block, nnz=raw_block.nnz - 1), 1, None, None, None, 'different entry counts')
            bad = copy.copy(raw_block); bad.col_idx = raw_block.col_idx.copy(); bad.col_idx[0] = CH.M
            refused(None, bad.pymatrix(), 1, None, None, None, 'outside rows() x m')
        assert s.rows() == twin.rows() == OH.T and s.series_stats_info() == twin.series_stats_info()
        a, b = s.download(), twin.download()
        assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)
        with pytest.raises(ValueError, match='flags'):
            s.change_series(np.ones(3, dtype=bool))
        noop = s.change_series()                                                                    # keep None, no block: nothing happens
        assert noop['series'] == noop['series_before'] == CH.N0 and noop['series_retired'] == noop['series_added'] == 0
        for x in (s, twin):
            x.run(1)
        a, b = s.download(), twin.download()
        assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)
        assert s.add_series(block)['series'] == OH.N                                                # ... and a valid churn still works
        s.run(1).sync()


def test_refusals_of_the_rank_and_the_transform():
    dtype = np.float32
    d72 = OH.inputs(72)
    blk = _cols(72, CH.N0, OH.N, dtype, 'sparse')[0]
    with Session(_cols(72, 0, CH.N0, dtype, 'sparse')[0], _model(d72, dtype), missing=True, **HYPER) as s:
        with pytest.raises(RuntimeError, match='ranks 1..64'):
            s.add_series(blk)
        assert s.model.n == CH.N0 and s.add_series(blk, fit=False)['series'] == OH.N
    k = 7
    d = OH.inputs(k)
    tr = NormalizedTransform(CH.dense_cols(k, 0, CH.N0, dtype))
    trn = NormalizedTransform(CH.dense_cols(k, CH.N0, OH.N, dtype))
    block = CH.dense_cols(k, CH.N0, OH.N, dtype)
    with Session(CH.dense_cols(k, 0, CH.N0, dtype), _model(d, dtype), missing=False, **HYPER) as s:
        s.model.transform = tr
        s.set_transform(tr)
        H0 = s.download().H.copy()
        with pytest.raises(RuntimeError, match='need both tr_a_new and tr_b_new'):
            s.add_series(block)
        dead = copy.copy(trn); dead.a = trn.a.copy(); dead.a[0, 2] = 0
        with pytest.raises(RuntimeError, match='is zero'):
            s.add_series(block, transform_new=dead)
        dead.a[0, 2] = np.inf
        with pytest.raises(RuntimeError, match='not finite'):
            s.add_series(block, transform_new=dead)
        assert s.model.n == CH.N0 and np.array_equal(s.download().H, H0)
        assert s.add_series(block, transform_new=trn)['series'] == OH.N and s.model.transform.a.shape == (1, OH.N)


def test_a_refused_churn_keeps_a_group_of_ranks_usable(monkeypatch):
    """TRMF_DEVICES=0,0: the validation runs on the calling thread, so a refused call does not break the group's barrier."""
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    with Session(_cols(k, 0, CH.N0, dtype, 'sparse')[0], _model(d, dtype), missing=True, **HYPER) as s:
        assert '2 ranks' in s.describe()
        s.run(1)
        with pytest.raises(RuntimeError, match='no series would be left'):
            s.change_series(np.zeros(CH.N0, dtype=bool))
        with pytest.raises(RuntimeError, match='storage class'):
            s.add_series(CH.dense_cols(k, CH.N0, OH.N, dtype))
        assert s.change_series(CH.keep_mask(), _cols(k, CH.N0, OH.N, dtype, 'sparse')[0])['series'] == OH.N - len(CH.RETIRED)
        s.run(1).sync()
        assert '2 ranks' in s.describe()


# ---- 6. determinism -----------------------------------------------------------------------------------------------------------
def test_two_sessions_and_two_virtual_ranks_give_the_same_bits(monkeypatch):
    """The add-and-retire case of test 1 twice on one rank, and on two virtual ranks of device 0 against one rank in the tile
    geometry several ranks use (TRMF_TEST=1 TRMF_TILE=narrow, tests/test_gpu_devices.py)."""
    dtype, k = np.float32, 40
    d = OH.inputs(k)
    names = []

    def once():
        with Session(_cols(k, 0, CH.N0, dtype, 'sparse')[0], _model(d, dtype), missing=True, **HYPER) as s:
            s.run(1)
            sums = s.change_series(CH.keep_mask(), _cols(k, CH.N0, OH.N, dtype, 'sparse')[0])
            names.append(s.describe())
            return sums, CH.after(s, OH.T)

    a, b = once(), once()
    assert a[0] == b[0]
    CH.assert_same(a[1], b[1], 'two sessions')
    monkeypatch.setenv('TRMF_TEST', '1')
    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = once()
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two = once()
    assert one[0] == two[0] and '2 ranks' in names[-1] and '1 rank' in names[-2]
    CH.assert_same(one[1], two[1], 'two virtual ranks')


# ---- 7. composition with the window ---------------------------------------------------------------------------------------------
def test_churn_between_the_ticks_of_a_sliding_window():
    """update(window=N) in blocks of 4 rows with a churn after the third block: the session ends bit for bit where a session
    re-created from host arrays at the churn ends."""
    dtype, k, N, step = np.float32, 7, 40, 4
    d = OH.inputs(k)
    keep = CH.keep_mask()
    before, after_ = list(range(CH.N0)), list(np.flatnonzero(keep)) + list(range(CH.N0, OH.N))
    cur = CH.raw_part(k, 0, N, before, dtype, SEED)
    ref = None
    with Session(cur.pymatrix(), _model(d, dtype, rows=N), missing=True, **HYPER) as s:
        for i, t in enumerate(range(N, N + 6 * step, step)):
            series = before if i < 3 else after_
            block = CH.raw_part(k, t, t + step, series, dtype, SEED)
            s.update(block.pymatrix(), window=N)
            cur = SH.slid(cur, step, block)
            if ref is not None:
                ref.update(block.pymatrix(), window=N)
            if i == 2:
                lo = t + step - N
                blk = CH.raw_part(k, lo, lo + N, range(CH.N0, OH.N), dtype, SEED)
                sums = s.change_series(keep, blk.pymatrix())
                cur = CH.churned(cur, keep, blk)
                assert sums['entries'] == cur.nnz and s.rows() == N
                m = s.download()
                ref = Session(cur.pymatrix(), make_model(m.W.copy(), m.H.copy(), m.lag_val.copy(), d['lag_set']), missing=True, **HYPER)
        try:
            a, b = s.download(), ref.download()
            assert a.H.shape == (len(after_), k)
            assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)
            s.run(2); ref.run(2)
            a, b = s.download(), ref.download()
            assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)
        finally:
            ref.close()
