"""CPU: the host side of series churn -- trmf.churn_entries (the NumPy statement of the stored-order rule of
trmf_session_change_series), Model.add_series / retire_series, the front end's argument checks and its behaviour against a library
built before the feature.  No GPU."""
import types

import numpy as np
import pytest

import churn_helpers as CH
import online_helpers as OH
import trmf
from helpers import make_model
from rawsparse_helpers import RawSparse
from trmf.session import Session, check_keep


def _lists(seed, n=9, T=7, count=60):
    """An unsorted entry list with doubled cells."""
    rng = np.random.RandomState(seed)
    r, c = rng.randint(0, T, size=count), rng.randint(0, n, size=count)
    r, c = np.concatenate([r, r[:8]]), np.concatenate([c, c[:8]])            # eight cells twice
    v = rng.rand(r.size)
    return r, c, v


# ---- churn_entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('major', ['row', 'col'])
@pytest.mark.parametrize('with_block', [False, True], ids=['no-block', 'block'])
def test_churn_entries_against_a_brute_force_loop(major, with_block):
    n = 9
    r, c, v = _lists(1, n)
    if with_block:                                           # the CSR / CSC arrays of a session are grouped by their major index
        o = np.argsort(r if major == 'row' else c, kind='stable')
        r, c, v = r[o], c[o], v[o]
    keep = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1], dtype=bool)
    block = _lists(2, 4) if with_block else None
    if with_block:
        o = np.argsort(block[0] if major == 'row' else block[1], kind='stable')
        block = tuple(a[o] for a in block)
    got = trmf.churn_entries(r, c, v, keep, n, block, major=major)
    want = CH.brute_churn(r, c, v, keep, n, block, major)
    assert [(int(a), int(b), x) for a, b, x in zip(*got)] == want
    assert len(want) == np.count_nonzero(keep[c]) + (len(block[0]) if with_block else 0)
    # the kept series are numbered densely in their order, the block's follow
    assert set(got[1].tolist()) <= set(range(int(keep.sum()) + (4 if with_block else 0)))


def test_churn_entries_on_a_raw_pair_gives_a_consistent_pair():
    """Both orientations of a non-canonical pair (random stored orders, doubled cells) through churn_entries: still one multiset
    (RawSparse.from_arrays checks it), every row the survivors in stored order and then the block's."""
    k = 7
    raw, blk = CH.raw_cols(k, 0, CH.N0, np.float32, 3), CH.raw_cols(k, CH.N0, OH.N, np.float32, 3)
    keep = CH.keep_mask()
    out = CH.churned(raw, keep, blk)
    assert out.shape == (OH.T, int(keep.sum()) + CH.M) and out.nnz == np.count_nonzero(keep[raw.cols]) + blk.nnz
    remap = np.cumsum(keep) - 1
    for i in (0, 5, 74, 95):
        a0, a1 = int(raw.row_ptr[i]), int(raw.row_ptr[i + 1])
        old = raw.col_idx[a0:a1].astype(np.int64)
        b0, b1 = int(blk.row_ptr[i]), int(blk.row_ptr[i + 1])
        want = np.concatenate([remap[old[keep[old]]], blk.col_idx[b0:b1].astype(np.int64) + int(keep.sum())])
        assert np.array_equal(out.col_idx[int(out.row_ptr[i]):int(out.row_ptr[i + 1])], want)
    # the CSC: kept columns as stored, then the block's columns as delivered
    q = int(remap[CH.N0 - 2])
    j0, j1 = int(raw.col_ptr[CH.N0 - 2]), int(raw.col_ptr[CH.N0 - 1])
    assert np.array_equal(out.row_idx[int(out.col_ptr[q]):int(out.col_ptr[q + 1])], raw.row_idx[j0:j1])
    assert np.array_equal(out.val[int(out.col_ptr[int(keep.sum())]):], blk.val) and np.array_equal(out.row_idx[int(out.col_ptr[int(keep.sum())]):], blk.row_idx)


def test_churn_entries_keep_all_without_a_block_is_the_identity():
    r, c, v = _lists(3)
    for keep in (None, np.ones(9, dtype=bool)):
        for major in ('row', 'col'):
            got = trmf.churn_entries(r, c, v, keep, 9, major=major)
            assert all(np.array_equal(a, b) for a, b in zip(got, (r, c, v)))
            assert got[0] is not r and got[2] is not v


def test_two_churns_compose():
    """Retiring A and adding B, then retiring C and adding D, is one churn of the union (kept series of the first call that survive
    the second, then B's survivors, then D)."""
    n = 9
    r, c, v = _lists(4, n)
    o = np.argsort(r, kind='stable'); r, c, v = r[o], c[o], v[o]
    blk1 = _lists(5, 3, count=20); o = np.argsort(blk1[0], kind='stable'); blk1 = tuple(a[o] for a in blk1)
    blk2 = _lists(6, 2, count=12); o = np.argsort(blk2[0], kind='stable'); blk2 = tuple(a[o] for a in blk2)
    keep1 = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0], dtype=bool)                # 6 kept + 3 new = 9
    keep2 = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1], dtype=bool)                # of those 9
    step = trmf.churn_entries(*trmf.churn_entries(r, c, v, keep1, n, blk1), keep2, 9, blk2)
    # in one go: the old series that survive both, the block-1 series that survive the second, then block 2
    old_keep = keep1.copy(); old_keep[np.flatnonzero(keep1)[~keep2[:6]]] = False
    b1_keep = keep2[6:]
    b1 = trmf.churn_entries(*blk1, b1_keep, 3)
    merged = trmf.churn_entries(r, c, v, old_keep, n, b1)
    once = trmf.churn_entries(*merged, None, int(old_keep.sum()) + int(b1_keep.sum()), blk2)
    assert all(np.array_equal(a, b) for a, b in zip(step, once))


def test_churn_entries_argument_errors():
    r, c, v = _lists(7)
    with pytest.raises(ValueError, match='one length'):
        trmf.churn_entries(r[:-1], c, v, None, 9)
    with pytest.raises(ValueError, match='flags'):
        trmf.churn_entries(r, c, v, np.ones(8, dtype=bool), 9)
    with pytest.raises(ValueError, match='outside'):
        trmf.churn_entries(r, c, v, None, 5)
    with pytest.raises(ValueError, match='major'):
        trmf.churn_entries(r, c, v, None, 9, major='diag')
    with pytest.raises(ValueError, match='block'):
        trmf.churn_entries(r, c, v, None, 9, (r[:3], c[:2], v[:3]))
    with pytest.raises(ValueError, match='negative'):
        trmf.churn_entries(r, c, v, None, 9, (r[:3], -c[:3] - 1, v[:3]))


# ---- Model.add_series / retire_series ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('missing', [True, False])
def test_model_add_series_is_series_ridge_on_the_new_columns(missing):
    k = 7
    d = OH.inputs(k)
    m = make_model(d['W'], d['H'][:CH.N0], d['theta'], d['lag_set'])
    Ynew = CH.fit_csc(CH.fit_raw(k, np.float32)) if missing else CH.fit_dense(k, np.float32)
    out = m.add_series(Ynew, 0.5, missing=missing, forget=0.95)
    want = trmf.series_ridge(d['W'], Ynew, 0.5, 0.95, missing)
    assert out.n == CH.N0 + CH.FIT_M and np.array_equal(out.H[:CH.N0], d['H'][:CH.N0]) and np.array_equal(out.H[CH.N0:], want)
    assert np.array_equal(out.W, d['W']) and np.array_equal(out.lag_val, d['theta']) and m.n == CH.N0
    assert not missing or not out.H[CH.N0].any()             # the series without an entry: h = 0 exactly
    with pytest.raises(ValueError, match='rows'):
        m.add_series(Ynew[:-1], 0.5, missing=missing)


def test_model_retire_series_gathers():
    from trmf.model import NormalizedTransform
    k = 7
    d = OH.inputs(k)
    m = make_model(d['W'], d['H'], d['theta'], d['lag_set'])
    m.transform = NormalizedTransform(CH.dense_cols(k, 0, OH.N, np.float32))
    keep = CH.keep_mask(OH.N)
    for which in (list(CH.RETIRED), ~keep):
        out = m.retire_series(which)
        assert np.array_equal(out.H, d['H'][keep]) and np.array_equal(out.W, d['W']) and out.n == OH.N - len(CH.RETIRED)
        assert np.array_equal(out.transform.a, m.transform.a[:, keep]) and np.array_equal(out.transform.b, m.transform.b[:, keep])
    assert m.n == OH.N and m.transform.a.shape == (1, OH.N)
    with pytest.raises(ValueError, match='no series'):
        m.retire_series(np.ones(OH.N, dtype=bool))
    grown = m.add_series(CH.fit_dense(k, np.float32), 0.5, missing=False, transform_new=NormalizedTransform(CH.fit_dense(k, np.float32)))
    assert grown.transform.a.shape == (1, OH.N + CH.FIT_M)
    with pytest.raises(ValueError, match='transform_new'):
        m.add_series(CH.fit_dense(k, np.float32), 0.5, missing=False)


# ---- check_keep -------------------------------------------------------------------------------------------------------------
def test_check_keep():
    assert check_keep(None, 4).tolist() == [True] * 4
    mask = np.array([True, False, True, True])
    got = check_keep(mask, 4)
    assert got.tolist() == mask.tolist() and got is not mask
    assert check_keep(mask, 4, retire=True).tolist() == [False, True, False, False]
    assert check_keep([3, 0], 4, retire=True).tolist() == [False, True, True, False]
    assert check_keep([], 4, retire=True).tolist() == [True] * 4
    with pytest.raises(ValueError, match='flags'):
        check_keep(np.ones(3, dtype=bool), 4)
    with pytest.raises(TypeError, match='mask'):
        check_keep([1, 0, 1, 1], 4)                          # integers are not flags
    with pytest.raises(TypeError, match='indices'):
        check_keep([0.5], 4, retire=True)
    with pytest.raises(ValueError, match='outside'):
        check_keep([4], 4, retire=True)
    with pytest.raises(ValueError, match='outside'):
        check_keep([-1], 4, retire=True)
    with pytest.raises(ValueError, match='twice'):
        check_keep([1, 1], 4, retire=True)


# ---- a library built before the feature -------------------------------------------------------------------------------------
def test_change_series_against_a_library_without_the_symbol():
    d = OH.inputs(7)
    s = object.__new__(Session)
    s.handle = None
    s.model = make_model(d['W'], d['H'], d['theta'], d['lag_set'])
    s.lib = types.SimpleNamespace()                          # no trmf_session_change_series
    for call in (lambda: s.change_series(np.ones(OH.N, dtype=bool)), lambda: s.retire_series([1]),
                 lambda: s.add_series(RawSparse(np.array([0]), np.array([0]), np.array([1.0]), (OH.T, 1), np.float32).pymatrix())):
        with pytest.raises(RuntimeError, match='built before series churn'):
            call()
    with pytest.raises(ValueError, match='flags'):           # the argument check comes first
        s.change_series(np.ones(3, dtype=bool))
    assert s.model.n == OH.N
