"""GPU (-m gpu): cell revisions on the device -- trmf_session_revise (revise_count_kernel, revise_kernel, dense_revise_kernel,
series_revise_kernel) behind Session.revise / retract / update(revisions=).  Small shapes (tests/revise_helpers.py): T = 96 rows of
50 series, both orientations in random stored orders, two cells stored twice.

The contract is bit-identity: after a revise the session IS the session trmf_session_create builds from the revised entries in their
stored order (revise_helpers.revised = trmf.revise_entries on both orientations) and the current W, H and lag weights, so every
later call returns the same bits on both.  Only the revised statistics are held to a yardstick instead (adapt_helpers.bound: 8x an
fp32 NumPy twin of the same recursion against the fp64 direct ridge, the slide tests' yardstick for downdate_stats)."""
from ctypes import byref

import numpy as np
import pytest

import adapt_helpers as AH
import churn_helpers as CH
import online_helpers as OH
import revise_helpers as RH
import slide_helpers as SH
from helpers import evidence, make_model, relmax
from trmf.model import NormalizedTransform
from trmf.session import Session, TrmfReviseSums

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, 40), (np.float64, 7)]
DT_IDS = ['float32-k40', 'float64-k7']
HYPER = dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5)
SEED = 41
COUNTED = ('edits', 'inserted', 'replaced', 'deleted', 'missed', 'copies_removed', 'entries_before', 'entries', 'first_row', 'last_row')


def _model(d, dtype, W=None, H=None, theta=None, rows=OH.T):
    return make_model((d['W'][:rows] if W is None else W).astype(dtype), (d['H'] if H is None else H).astype(dtype),
                      (d['theta'] if theta is None else theta).astype(dtype), d['lag_set'])


def _Y(k, dtype, storage, rows=OH.T):
    """The first `rows` rows as a session takes them: (what Session gets, the RawSparse behind it or the dense array)."""
    if storage == 'dense':
        Y = RH.dense_all(k, dtype, 0, rows)
        return Y, Y
    raw = RH.raw_all(k, dtype, SEED, 0, rows)
    return raw.pymatrix(), raw


def _typed(ed, dtype):
    return ed[0], ed[1], np.asarray(ed[2]).astype(dtype), ed[3]


# ---- 1. equals a fresh session, bit for bit -----------------------------------------------------------------------------------
FORMS = [('sparse-missing', 'sparse', True, False), ('sparse-full', 'sparse', False, False), ('dense', 'dense', False, False),
         ('dense-transform', 'dense', False, True)]


def _revise_case(storage, missing, transform, name, dtype, k):
    """One session through run(1) + revise, one fresh session on the revised arrays: (what the first gives, what the second
    gives, the sums, the NumPy statement of the sums)."""
    d = OH.inputs(k)
    ed = _typed(RH.batch(name, k, deletes=storage == 'sparse'), dtype)
    Y, held = _Y(k, dtype, storage)
    tr = NormalizedTransform(RH.dense_all(k, dtype)) if transform else None
    with Session(Y, _model(d, dtype), missing=missing, **HYPER) as s:
        if tr is not None:
            s.model.transform = tr
            s.set_transform(tr)
        s.run(1)
        m1 = s.download()
        W1, H1, Th1 = m1.W.copy(), m1.H.copy(), m1.lag_val.copy()
        sums = s.revise(ed[0], ed[1], ed[2], ed[3] if storage == 'sparse' else None)
        m2 = s.download()
        assert np.array_equal(m2.W, W1) and np.array_equal(m2.H, H1) and np.array_equal(m2.lag_val, Th1)      # the factors are not touched
        got = CH.after(s, OH.T)
    if storage == 'sparse':
        want_Y, counts = RH.revised(held, ed, counts=True)
        fresh_Y = want_Y.pymatrix()
    else:
        fresh_Y = RH.revised_dense(held, ed)
        E = len(ed[0])
        counts = dict(edits=E, inserted=0, replaced=E, deleted=0, missed=0, copies_removed=E, entries_before=OH.T * OH.N, entries=OH.T * OH.N,
                      first_row=int(ed[0].min()), last_row=int(ed[0].max()))
    with Session(fresh_Y, make_model(W1, H1, Th1, d['lag_set']), missing=missing, **HYPER) as f:
        if tr is not None:
            f.set_transform(tr)
        return got, CH.after(f, OH.T), sums, counts


# (dense storage refuses deletes -- test_a_refused_revise_leaves_the_session_as_it_was -- so it has no delete-only case)
CASES = [f + (name,) for f in FORMS for name in RH.BATCHES if not (f[1] == 'dense' and name == 'delete-only')]


@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('form,storage,missing,transform,name', CASES, ids=[c[0] + '-' + c[4] for c in CASES])
def test_revise_equals_a_fresh_session(form, storage, missing, transform, name, dtype, k):
    """The sparse input is not canonical: neither orientation is sorted, two cells are stored twice.  The mixed batch touches row 0
    and the last row, series 0 and the last series, both copies of each doubled cell (one replaced, one deleted), the series
    without an entry and, as deletes, cells that are not stored.  Dense storage takes the same cells as sets."""
    got, want, sums, counts = _revise_case(storage, missing, transform, name, dtype, k)
    assert {key: sums[key] for key in COUNTED} == {key: counts[key] for key in COUNTED}
    assert not sums['stats_carried']
    if name == 'mixed' and storage == 'sparse':
        assert sums['first_row'] == 0 and sums['last_row'] == OH.T - 1 and sums['missed'] >= 1
        assert sums['copies_removed'] >= sums['replaced'] + sums['deleted'] + 2          # both copies of the two doubled cells
    CH.assert_same(got, want, form + ' ' + name)


# ---- 2. the compaction's row shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_every_row_shape_is_revised_stably(dtype):
    """churn_helpers.shape_problem's rows of 0, 1, 63, 64, 65 and 130 entries (and one of 140 with repeated cells) under per-row edit
    lists of 0, 1, 2, 64 and 65 cells -- the bounds of the binary search -- that drop a row's first stored entry, its last, every
    one and none, and an insert into the empty row.  The X-side Gram adds a row's entries in stored order in the element type, so
    the trained factors tell a compaction that kept another order (or lost an entry) from the fresh session's arrays."""
    raw, _ = CH.shape_problem(np.dtype(dtype))
    T, n = raw.shape
    k, lags = 7, [1, 3]
    rng = np.random.RandomState(2)
    W0, H0 = rng.rand(T, k).astype(dtype), rng.rand(n, k).astype(dtype)
    Th0 = np.asfortranarray((rng.randn(2, k) / 3).astype(dtype))
    ed = _typed(RH.shape_edits(raw), dtype)
    assert np.bincount(ed[0], minlength=T).tolist() == [1, 1, 64, 65, 2, 64, 0, 1, 0, 0, 0, 3]
    want, counts = RH.revised(raw, ed, counts=True)
    outs = []
    with Session(raw.pymatrix(), make_model(W0, H0, Th0, lags), missing=True, **HYPER) as s:
        sums = s.revise(*ed)
        assert {key: sums[key] for key in COUNTED} == {key: counts[key] for key in COUNTED}
        per_row = np.zeros(T, dtype=np.uint64)
        assert s.lib.trmf_session_row_entries(s.handle, per_row.ctypes.data) == 0
        assert np.array_equal(per_row, np.diff(want.row_ptr)) and np.array_equal(s._stored, np.diff(want.row_ptr.astype(np.int64)))
        s.run(2); m = s.download(); outs.append((m.W.copy(), m.H.copy(), m.lag_val.copy(), s.objective()))
    with Session(want.pymatrix(), make_model(W0, H0, Th0, lags), missing=True, **HYPER) as f:
        f.run(2); m = f.download(); outs.append((m.W.copy(), m.H.copy(), m.lag_val.copy(), f.objective()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---- 3. the statistics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('gamma', [1.0, 0.98])
def test_revised_statistics_fit_the_revised_entries(gamma, dtype, k):
    """init_series_stats, revise(update_stats=True) with replaces, inserts and deletes, adapt_series: H against series_ridge in fp64
    on the revised entries, no farther than 8x the fp32 NumPy twin of the same recursion (scaled by eps64 / eps32 for fp64).

    Measured on an MI355X: 0.13 (fp32, gamma 1), 0.12 (fp32, 0.98), 0.10 (fp64, 1) and 0.28 (fp64, 0.98) of the bound."""
    lamI = 0.5
    d = OH.inputs(k)
    hyper = dict(HYPER, lambdaI=lamI)
    ed = _typed(RH.batch('mixed', k), dtype)
    Y, raw = _Y(k, dtype, 'sparse')
    with Session(Y, _model(d, dtype), missing=True, **hyper) as s:
        s.init_series_stats(gamma)
        sums = s.revise(*ed, update_stats=True)
        assert sums['stats_carried'] and s.series_stats_info() == dict(valid=True, stale=False, absorbed_rows=OH.T, forget=gamma)
        ad, H = s.adapt_series(return_loadings=True)
        assert ad['rows'] == 0 and ad['series'] == OH.N
    with Session(Y, _model(d, dtype), missing=True, **hyper) as u:         # the tables left unrevised
        u.init_series_stats(gamma)
        _, Hplain = u.adapt_series(return_loadings=True)
    ref, yard = RH.stats_yardstick(d['W'], raw, ed, lamI, gamma)
    b, err = AH.bound(dtype, yard), relmax(H, ref)
    evidence('cell revisions %s k=%d gamma=%g: relmax of H after revise(update_stats) + adapt_series to the fp64 direct ridge on the revised entries '
             '%.3e = %.2f x its bound %.3e (fp32 twin %.3e)' % (np.dtype(dtype).name, k, gamma, err, err / b, b, yard))
    assert err <= b
    assert not np.array_equal(H, Hplain)                                     # the update did something
    touched = np.unique(ed[1])
    assert np.array_equal(np.delete(H, touched, axis=0), np.delete(Hplain, touched, axis=0))      # untouched series: their tables were copied


def test_statistics_without_the_update_go_stale():
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    ed = _typed(RH.batch('mixed', k), dtype)
    with Session(_Y(k, dtype, 'sparse')[0], _model(d, dtype), missing=True, **HYPER) as s:
        s.init_series_stats(0.98)
        gone = RH.batch('delete-only', k)                                    # (its last cell is not stored)
        sums = s.retract(gone[0][-1:], gone[1][-1:])
        assert sums['missed'] == 1 and sums['copies_removed'] == 0 and s.series_stats_info()['valid']      # nothing changed
        sums = s.revise(*ed)
        info = s.series_stats_info()
        assert not sums['stats_carried'] and info['stale'] and not info['valid']
        with pytest.raises(RuntimeError, match='series statistics'):
            s.adapt_series()
        s.init_series_stats(0.98)                                            # ... and can be built again
        assert s.adapt_series()['series'] == OH.N
    with Session(_Y(k, dtype, 'sparse', SH.T0)[0], _model(d, dtype, rows=SH.T0), missing=True, **HYPER) as s:
        s.init_series_stats(0.98)
        s.append_rows(SH.raw_rows(k, SH.T0, OH.T, dtype, SEED).pymatrix())    # 96 rows, 84 absorbed
        s.model = _model(d, dtype)
        sums = s.revise(*ed, update_stats=True)                              # tables that lag behind cannot follow
        assert not sums['stats_carried'] and s.series_stats_info()['stale']


# ---- 4. refusals and atomicity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage,missing', [('sparse', True), ('sparse', False), ('dense', False)], ids=['sparse-missing', 'sparse-full', 'dense'])
def test_a_refused_revise_leaves_the_session_as_it_was(storage, missing):
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    Y, _ = _Y(k, dtype, storage)
    u32 = lambda *a: np.array(a, dtype=np.uint32)
    one = np.ones(4, dtype=dtype)
    with Session(Y, _model(d, dtype), missing=missing, **HYPER) as s, Session(Y, _model(d, dtype), missing=missing, **HYPER) as twin:
        for x in (s, twin):
            x.run(1)

        def same_bits():
            a, b = s.download(), twin.download()
            assert np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H) and np.array_equal(a.lag_val, b.lag_val)
            assert np.array_equal(np.float64(s.objective()), np.float64(twin.objective()), equal_nan=True) and s.rows() == twin.rows() == OH.T

        def refused(count, rows, cols, vals, dele, update, text):
            ptr = lambda a: a.ctypes.data if a is not None else None
            rc = s.lib.trmf_session_revise(s.handle, count, ptr(rows), ptr(cols), ptr(vals), ptr(dele), update, None)
            assert rc < 0 and text in s.lib.trmf_last_error().decode(), (text, s.lib.trmf_last_error().decode())
            same_bits()

        refused(2, u32(1, OH.T), u32(2, 3), one, None, 0, 'names row %d, the session holds %d' % (OH.T, OH.T))
        refused(2, u32(1, 2), u32(OH.N, 3), one, None, 0, 'names series %d, the session holds %d' % (OH.N, OH.N))
        refused(3, u32(4, 7, 4), u32(9, 9, 9), one, None, 0, 'cell (4, 9) is named twice in one batch')
        refused(1, u32(4), u32(9), one, None, 2, 'update_stats must be 0 or 1')
        refused(1, u32(4), u32(9), None, None, 0, 'vals is needed')
        refused(1 << 32, u32(4), u32(9), one, None, 0, '32-bit device indices')
        if storage == 'dense':
            refused(2, u32(4, 5), u32(9, 9), one, np.array([0, 1], dtype=np.uint8), 0, 'a delete on dense storage')
        if missing:
            refused(1, u32(4), u32(9), one, None, 1, 'without valid series statistics')
        else:
            refused(1, u32(4), u32(9), one, None, 1, 'full-observation')
        # an empty batch returns 0 and changes nothing
        sums = TrmfReviseSums()
        assert s.lib.trmf_session_revise(s.handle, 0, None, None, None, None, 0, byref(sums)) == 0
        assert sums.edits == 0 and sums.first_row == -1 and sums.last_row == -1 and sums.entries == sums.entries_before > 0
        same_bits()
        with pytest.raises(ValueError, match='one length'):
            s.revise([1, 2], [3], [0.5, 0.5])
        for x in (s, twin):
            x.run(1)
        same_bits()
        # ... and a valid revise still works; the mark rewinds past it
        s.mark()
        before = s.download()
        W0, H0, Th0 = before.W.copy(), before.H.copy(), before.lag_val.copy()
        ed = _typed(RH.batch('replace-only', k), dtype)
        assert s.revise(ed[0], ed[1], ed[2])['replaced'] == len(ed[0])
        s.run(2)
        assert not np.array_equal(s.download().W, W0)
        s.rewind()
        back = s.download()
        assert np.array_equal(back.W, W0) and np.array_equal(back.H, H0) and np.array_equal(back.lag_val, Th0)
        s.run(1).sync()


def test_a_refused_revise_keeps_a_group_of_ranks_usable(monkeypatch):
    """TRMF_DEVICES=0,0: the validation runs on the calling thread, so a refused call does not break the group's barrier."""
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    ed = _typed(RH.batch('mixed', k), dtype)
    with Session(_Y(k, dtype, 'sparse')[0], _model(d, dtype), missing=True, **HYPER) as s:
        assert '2 ranks' in s.describe()
        s.run(1)
        with pytest.raises(RuntimeError, match='named twice'):
            s.revise([4, 4], [9, 9], [0.5, 0.25])
        with pytest.raises(RuntimeError, match='names row'):
            s.revise([OH.T], [9], [0.5])
        assert s.revise(*ed)['edits'] == len(ed[0])
        s.run(1).sync()
        assert '2 ranks' in s.describe()


# ---- 5. the front end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
def test_update_with_revisions_equals_the_calls_by_hand(dtype, k):
    """update(block, revisions=..., smooth_back=4) on 84 resident rows: the revisions are applied before the block and the smoothed
    window reaches back to the first revised row (beyond the 4 rows asked for) -- bit for bit revise + append_rows + assimilate (the
    block's filter, which update always runs) + smooth(first revised row) done by hand."""
    d = OH.inputs(k)
    T0 = SH.T0
    full = RH.batch('mixed', k, T0)
    late = (full[0] >= 60) & ~full[3]
    rev = _typed(tuple(a[late] for a in full), dtype)[:3]
    first = int(rev[0].min())
    assert rev[0].size >= 5 and 60 <= first < T0 - 4
    block = SH.raw_rows(k, T0, OH.T, dtype, SEED)
    outs = []
    with Session(_Y(k, dtype, 'sparse', T0)[0], _model(d, dtype, rows=T0), missing=True, **HYPER) as s:
        sums = s.update(block.pymatrix(), revisions=rev, smooth_back=4)
        assert sums['revise']['edits'] == rev[0].size and sums['revise']['first_row'] == first and sums['smooth']['rows'] == OH.T - first
        m = s.download()
        outs.append((m.W.copy(), m.H.copy(), m.lag_val.copy(), sums['smooth'], {key: v for key, v in sums.items() if key not in ('smooth', 'revise')}))
    with Session(_Y(k, dtype, 'sparse', T0)[0], _model(d, dtype, rows=T0), missing=True, **HYPER) as h:
        h.revise(*rev)
        h.append_rows(block.pymatrix())
        h.model = _model(d, dtype)
        a = h.assimilate(T0)
        sm = h.smooth(first)
        m = h.download()
        outs.append((m.W.copy(), m.H.copy(), m.lag_val.copy(), sm, a))
    for x, y in zip(*outs):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    with Session(_Y(k, dtype, 'sparse', T0)[0], _model(d, dtype, rows=T0), missing=True, **HYPER) as s:
        plain = s.update(block.pymatrix(), smooth_back=4)                    # without revisions the window is the 4 rows asked for
        assert plain['smooth']['rows'] == OH.T - T0 + 4 and 'revise' not in plain


def test_model_revise_agrees_with_the_session():
    """Model.revise -- the host form -- and Session.revise on the same canonical matrix hold the same entries: the objective of a
    fresh session on the host form's matrix is the revised session's, up to the summation order of the revised rows."""
    dtype, k = np.float64, 7
    d = OH.inputs(k)
    Y = RH.raw_all(k, dtype, SEED).canonical()
    ed = _typed(RH.batch('mixed', k), dtype)
    m2, Y2 = _model(d, dtype).revise(Y, *ed)
    with Session(Y, _model(d, dtype), missing=True, **HYPER) as s:
        sums = s.revise(*ed)
        J = s.objective()
    with Session(Y2, m2, missing=True, **HYPER) as f:
        assert sums['entries'] == Y2.nnz and abs(f.objective() - J) <= 1e-12 * abs(J)
    m3, Y3 = m2.revise(Y2, ed[0], ed[1], Y.toarray()[ed[0], ed[1]], Y.toarray()[ed[0], ed[1]] == 0)      # ... and back
    assert np.array_equal(Y3.toarray(), Y.toarray()) and Y3.nnz == Y.nnz


# ---- 6. determinism -----------------------------------------------------------------------------------------------------------
def test_two_sessions_and_two_virtual_ranks_give_the_same_bits(monkeypatch):
    """The mixed case of test 1 twice on one rank, and on two virtual ranks of device 0 against one rank in the tile geometry
    several ranks use (TRMF_TEST=1 TRMF_TILE=narrow, tests/test_gpu_devices.py)."""
    dtype, k = np.float32, 40
    d = OH.inputs(k)
    ed = _typed(RH.batch('mixed', k), dtype)
    names = []

    def once():
        with Session(_Y(k, dtype, 'sparse')[0], _model(d, dtype), missing=True, **HYPER) as s:
            s.run(1)
            sums = s.revise(*ed)
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
