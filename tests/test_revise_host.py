"""CPU: the host side of the cell revisions -- trmf.revise_entries (the NumPy statement of the stored-order rule of
trmf_session_revise), trmf.SeriesStats.revise (the table update), Model.revise and the designed batches of revise_helpers.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as smat

import adapt_helpers as AH
import churn_helpers as CH
import online_helpers as OH
import revise_helpers as RH
import slide_helpers as SH
import trmf
from helpers import make_model, relmax


def _lists(seed, n=9, T=7, count=60):
    """An entry list grouped by neither index, with doubled cells; row 3 is empty."""
    rng = np.random.RandomState(seed)
    r, c = rng.randint(0, T - 1, size=count), rng.randint(0, n, size=count)
    r[r >= 3] += 1
    r, c = np.concatenate([r, r[:8]]), np.concatenate([c, c[:8]])            # eight cells twice
    return r, c, rng.rand(r.size)


def _edits(r, c, seed, n=9, T=7):
    """Replaces (one of them of a doubled cell), inserts (one into the empty row), deletes and a delete that misses."""
    rng = np.random.RandomState(seed)
    stored = list(dict.fromkeys(zip(r.tolist(), c.tolist())))
    absent = [(i, j) for i in range(T) for j in range(n) if (i, j) not in set(stored)]
    cells = [(int(r[0]), int(c[0]))] + stored[10:16] + [(3, 4)] + [x for x in absent if x[0] != 3][:5]
    er, ec = np.array([x[0] for x in cells]), np.array([x[1] for x in cells])
    dl = np.zeros(er.size, dtype=bool)
    dl[[2, 4, 6]] = True                                                     # stored cells
    dl[-1] = True                                                            # not stored: a miss
    p = rng.permutation(er.size)                                             # the order of the batch must not matter
    return er[p], ec[p], rng.rand(er.size)[p], dl[p]


@pytest.mark.parametrize('major', ['row', 'col'])
def test_revise_entries_against_a_brute_force_loop(major):
    r, c, v = _lists(1)
    o = np.argsort(r if major == 'row' else c, kind='stable')                # the arrays of a session are grouped by their major index
    r, c, v = r[o], c[o], v[o]
    ed = _edits(r, c, 2)
    got = trmf.revise_entries(r, c, v, ed, major=major, return_counts=True)
    want = RH.brute_revise(r, c, v, ed, major)
    assert [(int(a), int(b), x) for a, b, x in zip(*got[:3])] == want
    cells = set(zip(ed[0].tolist(), ed[1].tolist()))
    copies = sum((int(a), int(b)) in cells for a, b in zip(r, c))
    assert got[3] == dict(inserted=5, replaced=4, deleted=3, missed=1, copies_removed=copies) and copies >= 8
    assert len(want) == r.size - copies + 9
    assert (3, 4) in [(a, b) for a, b, _ in want]                            # the empty row gained its entry
    # the order of the batch does not matter
    p = np.random.RandomState(5).permutation(len(ed[0]))
    again = trmf.revise_entries(r, c, v, tuple(a[p] for a in ed), major=major)
    assert all(np.array_equal(a, b) for a, b in zip(again, got[:3]))


def test_revise_entries_guards():
    r, c, v = _lists(1)
    with pytest.raises(ValueError, match='twice'):
        trmf.revise_entries(r, c, v, ([1, 1], [2, 2], [0.5, 0.25]))
    with pytest.raises(ValueError, match='vals is needed'):
        trmf.revise_entries(r, c, v, ([1], [2], None))
    with pytest.raises(ValueError, match='major'):
        trmf.revise_entries(r, c, v, ([1], [2], [0.5]), major='x')
    same = trmf.revise_entries(np.sort(r), c, v, (np.zeros(0, int), np.zeros(0, int), np.zeros(0)))
    assert np.array_equal(same[0], np.sort(r)) and np.array_equal(same[1], c) and np.array_equal(same[2], v)


@pytest.mark.parametrize('name', RH.BATCHES)
def test_revise_on_a_raw_pair_gives_a_consistent_pair(name):
    """Both orientations of a non-canonical pair through revise_entries: still one multiset (RawSparse.from_arrays checks it), the
    untouched rows and columns as stored, the sets at the ends of theirs in ascending order."""
    k = 7
    raw = RH.raw_all(k, np.float32, 3)
    ed = RH.batch(name, k)
    out, cnt = RH.revised(raw, ed, counts=True)
    assert cnt['entries'] == raw.nnz - cnt['copies_removed'] + cnt['inserted'] + cnt['replaced']
    assert cnt['inserted'] + cnt['replaced'] == np.count_nonzero(~ed[3]) and cnt['deleted'] + cnt['missed'] == np.count_nonzero(ed[3])
    if name == 'mixed':
        assert cnt['first_row'] == 0 and cnt['last_row'] == RH.T - 1 and cnt['missed'] >= 1 and cnt['copies_removed'] >= cnt['replaced'] + cnt['deleted'] + 2
        assert {0, RH.N - 1, AH.NO_ENTRY} <= set(ed[1].tolist())
        for cell in (RH.DOUBLED, SH.DOUBLE_GONE):
            assert np.count_nonzero((ed[0] == cell[0]) & (ed[1] == cell[1])) == 1
        assert np.count_nonzero((out.rows == RH.DOUBLED[0]) & (out.cols == RH.DOUBLED[1])) == 1
        assert not np.any((out.rows == SH.DOUBLE_GONE[0]) & (out.cols == SH.DOUBLE_GONE[1]))
    touched = set(ed[0].tolist())
    for i in range(RH.T):
        a = raw.col_idx[int(raw.row_ptr[i]):int(raw.row_ptr[i + 1])]
        b = out.col_idx[int(out.row_ptr[i]):int(out.row_ptr[i + 1])]
        if i not in touched:
            assert np.array_equal(a, b)
            continue
        mine = ed[1][ed[0] == i]
        sets = np.sort(ed[1][(ed[0] == i) & ~ed[3]])
        assert np.array_equal(b, np.concatenate([a[~np.isin(a, mine)], sets]))


@pytest.mark.parametrize('gamma', [1.0, 0.98])
def test_series_stats_revise_against_a_rebuild(gamma):
    """The revised tables against SeriesStats rebuilt from the revised entries: the same terms in another order (and a
    cancellation of the removed ones), fp64, so they agree to the rounding of the sums."""
    k = 7
    W = OH.inputs(k)['W'].astype(np.float64)
    raw = RH.raw_all(k, np.float64, 3)
    ed = RH.batch('mixed', k)
    before = CH.fit_csc(raw)
    st = trmf.SeriesStats(W, before, gamma, True).revise(W, before, ed)
    want = trmf.SeriesStats(W, CH.fit_csc(RH.revised(raw, ed)), gamma, True)
    scale = np.abs(want.S).max()
    assert np.abs(st.S - want.S).max() <= 1e-13 * scale and np.abs(st.r - want.r).max() <= 1e-13 * scale
    assert st.rows == RH.T and relmax(st.solve(0.5), want.solve(0.5)) <= 1e-11
    untouched = np.setdiff1d(np.arange(RH.N), ed[1])
    plain = trmf.SeriesStats(W, before, gamma, True)
    assert np.array_equal(st.S[untouched], plain.S[untouched]) and np.array_equal(st.r[untouched], plain.r[untouched])
    assert not np.array_equal(st.S[0], plain.S[0])
    with pytest.raises(ValueError, match='per-series'):
        trmf.SeriesStats(W, RH.dense_all(k, np.float64), gamma, False).revise(W, RH.dense_all(k, np.float64), ed)


def test_model_revise_round_trips():
    """Model.revise on a canonical sparse Y and on a dense one: the cells are set / removed, the factors carried, and revising back
    restores the matrix; with update_stats the attached statistics follow."""
    k = 7
    d = OH.inputs(k)
    m = make_model(d['W'].astype(np.float64), d['H'].astype(np.float64), d['theta'].astype(np.float64), d['lag_set'])
    Y = RH.raw_all(k, np.float64, 3).canonical()
    ed = RH.batch('mixed', k)
    m.init_series_stats(Y, 0.98, True)
    m2, Y2 = m.revise(Y, ed[0], ed[1], ed[2], ed[3], update_stats=True)
    assert np.array_equal(m2.W, m.W) and np.array_equal(m2.H, m.H) and np.array_equal(m2.lag_val, m.lag_val)
    want = Y.toarray()
    want[ed[0], ed[1]] = np.where(ed[3], 0.0, ed[2].astype(np.float64))
    assert smat.issparse(Y2) and np.array_equal(Y2.toarray(), want)
    assert Y2.nnz == Y.nnz + np.count_nonzero(~ed[3] & (Y.toarray()[ed[0], ed[1]] == 0)) - np.count_nonzero(ed[3] & (Y.toarray()[ed[0], ed[1]] != 0))
    rebuilt = trmf.SeriesStats(m.W, Y2, 0.98, True)
    assert np.abs(m2.series_stats.S - rebuilt.S).max() <= 1e-13 * np.abs(rebuilt.S).max()
    # back again: the old values of the stored cells return, the inserted cells leave
    old = Y.toarray()[ed[0], ed[1]]
    m3, Y3 = m2.revise(Y2, ed[0], ed[1], old, old == 0)
    assert np.array_equal(Y3.toarray(), Y.toarray()) and Y3.nnz == Y.nnz and getattr(m3, 'series_stats', None) is None
    # dense
    Yd = RH.dense_all(k, np.float64)
    _, Yd2 = m.revise(Yd, ed[0], ed[1], ed[2])
    assert np.array_equal(Yd2, RH.revised_dense(Yd, ed)) and not np.array_equal(Yd2, Yd)
    with pytest.raises(ValueError, match='delete on a dense'):
        m.revise(Yd, ed[0], ed[1], ed[2], ed[3])
    with pytest.raises(ValueError, match='outside'):
        m.revise(Yd, [RH.T], [0], [1.0])


def test_shape_edits_hold_their_design():
    raw, _ = CH.shape_problem(np.dtype(np.float32))
    er, ec, ev, dl = RH.shape_edits(raw)
    per_row = np.bincount(er, minlength=raw.shape[0]).tolist()
    assert per_row[:8] == [1, 1, 64, 65, 2, 64, 0, 1] and per_row[8:11] == [0, 0, 0] and per_row[11] == 3
    out, cnt = RH.revised(raw, (er, ec, ev, dl), counts=True)
    lens = np.diff(out.row_ptr.astype(np.int64))
    assert lens[0] == 1 and lens[1] == 0 and lens[3] == 64 + 52 and cnt['missed'] == 13
    assert cnt['copies_removed'] > cnt['replaced'] + cnt['deleted']          # repeated cells of the 140-entry row left together


def test_the_front_end_checks_its_arguments_without_a_library():
    from trmf.session import Session
    s = object.__new__(Session)
    s.lib = type('L', (), {'trmf_session_revise': None})()
    s.model = make_model(np.zeros((4, 2), np.float32), np.zeros((3, 2), np.float32), np.zeros((1, 2), np.float32), [1])
    s.handle = None
    with pytest.raises(ValueError, match='one length'):
        s.revise([0, 1], [0], [1.0, 2.0])
    with pytest.raises(ValueError, match='vals is needed'):
        s.revise([0], [0])
    with pytest.raises(ValueError, match='one value per cell'):
        s.revise([0], [0], [1.0, 2.0])
    with pytest.raises(ValueError, match='negative'):
        s.revise([-1], [0], [1.0])
    s.lib = object()
    with pytest.raises(RuntimeError, match='built before the cell revisions'):
        s.revise([0], [0], [1.0])
