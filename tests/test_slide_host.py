"""CPU: the NumPy statements of the sliding window -- trmf.online.slide_entries (what the stored entries become),
trmf.SeriesStats.retire (the fp64 / fp32 downdate of the loading statistics) -- and the front-end refusals that need no device."""
import numpy as np
import pytest

import adapt_helpers as AH
import online_helpers as OH
import slide_helpers as SH
import trmf
from helpers import TOL, relmax


@pytest.mark.parametrize('retire', [0, 1, SH.RETIRE, SH.T0])
def test_slide_entries_is_slicing_the_dense_matrix(retire):
    """Stored order kept, rows reduced; scattered back (copies of a cell added) the result is the dense matrix sliced."""
    raw = SH.raw_rows(7, 0, SH.T0, np.float64, seed=3)
    dense = np.zeros(raw.shape); np.add.at(dense, (raw.rows, raw.cols), raw.vals)
    for rows, cols, vals in ((raw.rows, raw.cols, raw.vals),
                             (raw.row_idx.astype(np.int64), np.repeat(np.arange(raw.shape[1]), np.diff(raw.col_ptr.astype(np.int64))), raw.val)):
        r, c, v = trmf.slide_entries(rows, cols, vals, retire)
        got = np.zeros((raw.shape[0] - retire, raw.shape[1])); np.add.at(got, (r, c), v)
        assert np.array_equal(got, dense[retire:])
        keep = np.flatnonzero(rows >= retire)                                   # stable: the survivors in their stored order
        assert np.array_equal(r, rows[keep] - retire) and np.array_equal(c, cols[keep]) and np.array_equal(v, vals[keep])
    with pytest.raises(ValueError, match='negative'):
        trmf.slide_entries(raw.rows, raw.cols, raw.vals, -1)
    with pytest.raises(ValueError, match='one length'):
        trmf.slide_entries(raw.rows, raw.cols[:-1], raw.vals, 1)


def test_slid_arrays_are_a_consistent_pair():
    """slide_helpers.slid (the storage contract of the device test) keeps the entry multiset of the retained rows in both
    orientations (RawSparse.from_arrays checks that) and the stored order inside every column."""
    raw = SH.raw_rows(7, 0, SH.T0, np.float32, seed=3)
    tail = SH.raw_rows(7, SH.T0, OH.T, np.float32, seed=3)
    out = SH.slid(raw, SH.RETIRE, tail)
    assert out.shape == (OH.T - SH.RETIRE, OH.N) and out.nnz == np.count_nonzero(raw.rows >= SH.RETIRE) + tail.nnz
    j = AH.TWICE
    old = raw.row_idx[int(raw.col_ptr[j]):int(raw.col_ptr[j + 1])].astype(np.int64)
    new = out.row_idx[int(out.col_ptr[j]):int(out.col_ptr[j + 1])].astype(np.int64)
    kept = old[old >= SH.RETIRE] - SH.RETIRE
    assert np.array_equal(new[:kept.size], kept) and np.all(new[kept.size:] >= SH.T0 - SH.RETIRE)
    assert np.count_nonzero((raw.rows == SH.DOUBLE_GONE[0]) & (raw.cols == SH.DOUBLE_GONE[1])) >= 2      # the doubled cell that leaves


@pytest.mark.parametrize('k', [7, 40])
@pytest.mark.parametrize('gamma', [1.0, 0.95])
def test_series_stats_retire_is_the_ridge_on_the_retained_rows(k, gamma):
    """retire + solve against series_ridge computed directly on the retained rows: fp64 to rounding, and the fp32 twin -- the
    yardstick of the device test -- stays small on the chosen inputs (fewer than half of the absorbed rows leave).
    The bounds.  fp64: twin and direct sum differ by the order of at most 96 + 30 rank-1 terms per series; the entries of W lie in
    (0, 1), so ||S_j|| <= 96 k and the condition number of S_j + lambdaI I is at most kappa = (96 k + lambdaI) / lambdaI: the
    solutions agree to kappa x 126 x eps64.  fp32: the same product is no useful figure (1e-1); the twin is the yardstick of the
    device test, and 8x its error only gates anything while it stays inside the project's fp32 parity gate for factors
    (helpers.TOL, 1e-3)."""
    lamI = 0.5
    W = OH.inputs(k)['W']
    ref = SH.downdate_direct(W, k, lamI, gamma)
    h64 = SH.downdate_twin(W, k, np.float64, gamma).solve(lamI)
    h32 = SH.downdate_twin(W, k, np.float32, gamma).solve(lamI)
    e64, e32 = relmax(h64, ref), relmax(h32, ref)
    print('downdate twin k=%d gamma=%g: fp64 %.3e fp32 %.3e' % (k, gamma, e64, e32))
    kappa = (96.0 * k + lamI) / lamI
    assert e64 <= kappa * 126 * np.finfo(np.float64).eps and e32 <= TOL['float32']['factor']
    assert e64 <= AH.bound(np.float64, e32) and e32 > 0          # the twin itself passes the gate the device is held to


def test_series_stats_retire_without_downdate_keeps_the_tables():
    k = 7
    W = OH.inputs(k)['W'].astype(np.float64)
    st = trmf.SeriesStats(W[:SH.T0], SH.stats_training(k, 0, SH.T0, np.float64), 0.95, True)
    S, r = st.S.copy(), st.r.copy()
    st.retire(W, SH.stats_training(k, 0, SH.T0, np.float64), 10, downdate=False)
    assert st.rows == SH.T0 - 10 and np.array_equal(st.S, S) and np.array_equal(st.r, r)
    st.absorb(W[10:], SH.stats_training(k, SH.T0, OH.T, np.float64))            # the next block follows the retained rows
    assert st.rows == OH.T - 10
    with pytest.raises(ValueError, match='count'):
        st.retire(W, SH.stats_training(k, 0, SH.T0, np.float64), OH.T)
    with pytest.raises(ValueError, match='count'):
        st.retire(W, SH.stats_training(k, 0, SH.T0, np.float64), -1)


def test_front_end_refusals_need_no_device():
    from trmf.session import check_retire, check_window
    assert check_retire(0) == 0 and check_retire(np.int64(3)) == 3
    with pytest.raises(ValueError, match='negative'):
        check_retire(-1)
    for bad in (1.5, '2', None, True):
        with pytest.raises(TypeError, match='integer'):
            check_retire(bad)
    assert check_window(40, 1, 0, 5) == 40 and check_window(7, 1, 0, 5) == 7
    with pytest.raises(ValueError, match='smaller than the block'):
        check_window(6, 1, 0, 5)
    with pytest.raises(ValueError, match='smaller than the block'):
        check_window(20, 12, 3, 5)
    with pytest.raises(TypeError, match='integer'):
        check_window(40.0, 1, 0, 5)
    Y = np.random.RandomState(0).rand(120, 6)
    with pytest.raises(ValueError, match="window: a sliding window retires rows absorbed online"):
        trmf.rolling_validate(Y, [1, 2], k=3, window_size=4, nr_windows=3, window=40)
    with pytest.raises(ValueError, match='forecast_on_device'):
        trmf.rolling_validate(Y, [1, 2], k=3, window_size=4, nr_windows=3, update='assimilate', forecast_on_device=True, missing=False, window=40)
    with pytest.raises(ValueError, match='smaller than the block'):
        trmf.rolling_validate(Y, [1, 2], k=3, window_size=4, nr_windows=3, update='assimilate', window=6)
    m = trmf.Model.initialize(Y[:100], [1, 2], 3, seed=0)
    with pytest.raises(ValueError, match='smaller than the block'):
        m.assimilate(Y[100:104], 0.5, 0.5, missing=False, window=5)


def test_model_assimilate_window_keeps_the_last_rows():
    """The host form: the update itself is the one without a window, then the oldest rows beyond N leave."""
    Y = np.random.RandomState(1).rand(64, 6)
    m = trmf.Model.initialize(Y[:60], [1, 2], 3, seed=0)
    grown = m.assimilate(Y[60:], 0.5, 0.5, missing=False)
    win = m.assimilate(Y[60:], 0.5, 0.5, missing=False, window=50)
    assert grown.m == 64 and win.m == 50 and np.array_equal(win.W, grown.W[14:]) and np.array_equal(win.H, grown.H)
    assert m.assimilate(Y[60:], 0.5, 0.5, missing=False, window=100).m == 64
