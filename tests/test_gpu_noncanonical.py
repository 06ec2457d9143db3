"""GPU (-m gpu): sparse input that is NOT a canonical CSR/CSC pair, on every solver path.

The C ABI takes Y as two independent sets of arrays and the session uploads both exactly as the caller holds them.  Here the caller
holds what `PyMatrix(coo_matrix)` builds and more (tests/rawsparse_helpers.py): cells stored several times with different values,
stored zeros, one item column with more entries than there are timestamps and one timestamp row with more entries than there are
items, an empty row and an empty column, and a random entry order inside every row and column, drawn independently for the CSR and
the CSC.  Every index is in range and the pointers are consistent.

References: the C restatement fed the same arrays (checked on such input by tests/test_rawsparse_host.py against a per-entry NumPy
model and against the reference's build), the per-entry fp64 NumPy F-solve, and identities that need no oracle at all (another
order of the same entries; every entry twice == half the ridge weights; a stored zero is an observation).  Gates: the direct-solve
gates of tests/test_gpu_split.py for single solves, helpers.TOL for iterations.  A product that merged duplicates or skipped zeros
would be 20-55 % away (measured on the restatement, see the host tests).
"""
import functools
import os

import numpy as np
import pytest

import oracle_py as O
import trmf
from helpers import TOL, assert_within_fp32_noise, evidence, fp32_noise_yardstick, make_model, relfro, relmax
from rawsparse_helpers import RawSparse, dirty_problem, doubled, entry_fsolve, entry_objective, stacked, start_factors
from trmf import synth
from trmf._corelib import get_clib
from trmf.session import Session

pytestmark = pytest.mark.gpu
NCPU = os.cpu_count() or 8
THREADS = min(8, NCPU)
BIG = 10 ** 6
HYPER = synth.HYPER
T, N, DENSITY = 260, 150, 0.25
PATHS = {'rows': {}, 'unfused': {'TRMF_NO_HV_TILE': '1'}, 'split': {'TRMF_LONG_ROW': '24', 'TRMF_LONG_CHUNK': '32'}}
F32, F64 = np.float32, np.float64


def _py(raw):
    """What the product is handed: the raw arrays, untouched."""
    return raw.pymatrix()


def _name(dtype):
    return np.dtype(dtype).name


@functools.lru_cache(maxsize=None)
def _dirty(dtype, T=T, n=N, seed=1):
    return dirty_problem(T, n, DENSITY, dtype, seed=seed)[0]


@functools.lru_cache(maxsize=None)
def _start(dtype, k, nlag, T=T, n=N):
    return start_factors(T, n, k, nlag, dtype, seed=k + nlag)


@functools.lru_cache(maxsize=None)
def _oracle(dtype, k, lags, iters, periods=(1, 1, 2), missing=True):
    """The restatement on the standard dirty problem, computed once per case and shared (never modified by its users)."""
    raw = _dirty(dtype)
    W0, H0, Th0 = _start(dtype, k, len(lags))
    W, H, Th = W0.copy(), H0.copy(), np.asfortranarray(Th0.copy())
    log = O.train_port(raw, np.array(lags, np.uint32), W, H, Th, HYPER, max_iter=iters, periods=periods, threads=THREADS, missing=missing)
    for a in (W, H, Th):
        a.setflags(write=False)
    return W, H, Th, log


def _setenv(monkeypatch, path):
    for key, v in PATHS[path].items():
        monkeypatch.setenv(key, v)


def run_session(raw, lags, f0, iters, periods=(1, 1, 2), missing=True, hyper=HYPER):
    model = make_model(f0[0], f0[1], f0[2], lags)
    with Session(_py(raw), model, missing=missing, period_W=periods[0], period_H=periods[1], period_Lag=periods[2], **hyper) as s:
        d = s.describe()
        s.run(iters); st = s.stats(iters); J = s.objective() if missing else None; s.download()
    return model, st, J, d


def run_oneshot(raw, lags, f0, iters, periods=(1, 1, 2), hyper=HYPER):
    """The one-shot entry c_trmf_train on the raw arrays."""
    model = make_model(f0[0], f0[1], f0[2], lags)
    get_clib().train(_py(raw), model.lag_set, model.pyW, model.pyH, model.pylag_val, warm_start=True, max_iter=iters,
                     period_W=periods[0], period_H=periods[1], period_Lag=periods[2], threads=1, missing=True, **hyper)
    return model


def _assert_path(d, path, k):
    """The describe() line of the session names the path the case is about: the forced split cut rows into items, the unfused CG
    ran where it was asked for (and above rank 64, where it is the only form), the generic kernels took the ranks above 64."""
    assert ('split rows' in d) == (path == 'split'), d
    assert ('X-solve unfused' in d) == (path == 'unfused' or k > 64), d
    assert ('generic' in d) == (k > 64), d


# ---- a. the F-solve alone -----------------------------------------------------------------------------------------------------
# every rank class of the row kernels in both forms; the generic kernels (k = 80) have no split path
FSOLVE = [(d, k, p) for k in (8, 24, 40, 64) for d in (F32, F64) for p in ('rows', 'split')] + [(F32, 80, 'rows')]


@pytest.mark.parametrize('dtype,k,path', FSOLVE, ids=['%s-k%d-%s' % (_name(d), k, p) for d, k, p in FSOLVE])
def test_fsolve_alone_vs_restatement_and_per_entry_model(dtype, k, path, monkeypatch):
    """One F-solve from the random start (periods (BIG, 1, BIG)) through c_trmf_train: every rank class of the row kernels, the
    generic kernel (k = 80), and the forced split where the over-long item column is cut into items."""
    _setenv(monkeypatch, path)
    raw, lags = _dirty(dtype), (1, 2, 3)
    f0 = _start(dtype, k, 3)
    m = run_oneshot(raw, lags, f0, 1, periods=(BIG, 1, BIG))
    _, Ho, _, _ = _oracle(dtype, k, lags, 1, (BIG, 1, BIG))
    Hn = entry_fsolve(raw.cols, raw.rows, raw.vals, f0[0], f0[1], HYPER['lambdaI'])
    tight = 1e-6 if dtype == F64 else 2e-4
    evidence('noncanonical F-solve %s k=%d %s: relmax H vs restatement %.2e, vs per-entry fp64 model %.2e (gate %.0e)' % (
        _name(dtype), k, path, relmax(m.H, Ho), relmax(m.H, Hn), tight))
    assert np.array_equal(m.W, f0[0]) and np.array_equal(m.lag_val, f0[2])
    assert relmax(m.H, Ho) < tight and relmax(m.H, Hn) < tight
    with Session(_py(raw), make_model(f0[0], f0[1], f0[2], lags), missing=True, **HYPER) as s:
        _assert_path(s.describe(), path, k)


# ---- b. the X-solve alone -----------------------------------------------------------------------------------------------------
# ranks above 64 have one form of the X-solve (unfused, no split)
XSOLVE = [(d, k, p) for d, k in ((F32, 16), (F64, 16), (F32, 40), (F64, 40), (F32, 64)) for p in ('rows', 'unfused', 'split')] + [(F64, 72, 'rows')]


@pytest.mark.parametrize('dtype,k,path', XSOLVE, ids=['%s-k%d-%s' % (_name(d), k, p) for d, k, p in XSOLVE])
def test_xsolve_alone_vs_restatement(dtype, k, path, monkeypatch):
    """One X-solve from the random start (periods (1, BIG, BIG)): the Gram cache of every timestamp from entries in the caller's
    order (the over-long timestamp row included), then the CG -- fused / persistent, unfused with the packed cache, forced split."""
    _setenv(monkeypatch, path)
    raw, lags = _dirty(dtype), (1, 2, 3)
    f0 = _start(dtype, k, 3)
    m, st, _, d = run_session(raw, lags, f0, 1, periods=(1, BIG, BIG))
    Wo, _, _, log = _oracle(dtype, k, lags, 1, (1, BIG, BIG))
    gate = 1e-6 if dtype == F64 else TOL['float32']['factor']
    evidence('noncanonical X-solve %s k=%d %s (%s): relfro W %.2e (gate %.0e); CG %d vs %d' % (
        _name(dtype), k, path, d, relfro(m.W, Wo), gate, st[0]['cg_iter'], log[0]['cg_iter']))
    assert np.array_equal(m.H, f0[1])
    assert relfro(m.W, Wo) < gate
    assert abs(st[0]['cg_iter'] - log[0]['cg_iter']) <= 1
    _assert_path(d, path, k)


# ---- c. three full iterations -------------------------------------------------------------------------------------------------
ITER = [(F32, 8, 'rows'), (F64, 8, 'unfused'), (F32, 40, 'rows'), (F64, 40, 'rows'), (F32, 40, 'unfused'), (F32, 40, 'split'), (F64, 40, 'split'),
        (F64, 64, 'rows'), (F32, 64, 'split'), (F32, 80, 'rows'), (F64, 80, 'rows')]


@pytest.mark.parametrize('dtype,k,path', ITER, ids=['%s-k%d-%s' % (_name(d), k, p) for d, k, p in ITER])
def test_three_iterations_vs_restatement(dtype, k, path, monkeypatch):
    _setenv(monkeypatch, path)
    raw, lags = _dirty(dtype), (1, 2, 3, 4, 7)
    f0 = _start(dtype, k, len(lags))
    m, st, Jdev, d = run_session(raw, lags, f0, 3)
    W, H, Th, log = _oracle(dtype, k, lags, 3)
    tol = TOL[_name(dtype)]
    Jo = O.objective(raw, lags, W, H, Th, HYPER)
    Jp = O.objective(raw, lags, m.W, m.H, m.lag_val, HYPER)
    Jn = entry_objective(raw, lags, m.W, m.H, m.lag_val, HYPER)
    cg_o, cg_p = [l['cg_iter'] for l in log], [x['cg_iter'] for x in st]
    evidence('noncanonical 3 iterations %s k=%d %s (%s): relfro W %.2e H %.2e Th %.2e (gate %.0e); J rel %.2e, device J vs entry list %.2e (gate %.0e); CG %s vs %s' % (
        _name(dtype), k, path, d, relfro(m.W, W), relfro(m.H, H), relfro(m.lag_val, Th), tol['factor'], abs(Jp - Jo) / Jo, abs(Jdev - Jn) / Jn,
        tol['objective'], cg_p, cg_o))
    assert abs(Jp - Jn) <= 1e-12 * Jn                                     # the oracle's objective IS the sum over the entry list
    assert abs(Jdev - Jn) / Jn < tol['objective']
    direct = abs(Jp - Jo) / Jo < tol['objective'] and relfro(m.H, H) < tol['factor'] and relfro(m.W, W) < tol['factor'] and \
        relfro(m.lag_val, Th) < 10 * tol['factor']
    if not direct:
        # fp32 only: the truncated CG's noise floor, measured on the reference side on the same raw arrays (helpers.fp32_noise_yardstick)
        assert dtype == F32, (abs(Jp - Jo) / Jo, relfro(m.H, H), relfro(m.W, W), relfro(m.lag_val, Th))
        ys = fp32_noise_yardstick(raw, np.array(lags, np.uint32), f0[0], f0[1], f0[2], HYPER, 3, threads=THREADS)
        assert_within_fp32_noise(m, ys, np.array(lags, np.uint32), HYPER, what='noncanonical k=%d %s' % (k, path))
    assert all(abs(a - b) <= 1 for a, b in zip(cg_o, cg_p))
    _assert_path(d, path, k)


@pytest.mark.parametrize('dtype', [F32, F64])
def test_one_shot_entry_equals_the_session_on_raw_arrays(dtype):
    raw, lags = _dirty(dtype), (1, 2, 3, 4, 7)
    f0 = _start(dtype, 40, len(lags))
    a = run_oneshot(raw, lags, f0, 3)
    W, H, Th, _ = _oracle(dtype, 40, lags, 3)
    tol = TOL[_name(dtype)]['factor']
    assert relfro(a.W, W) < tol and relfro(a.H, H) < tol and relfro(a.lag_val, Th) < 10 * tol


# ---- d. identities that need no oracle ----------------------------------------------------------------------------------------
def _close(a, b, dtype, what):
    tol = TOL[_name(dtype)]['factor']
    got = (relfro(a.W, b.W), relfro(a.H, b.H), relfro(a.lag_val, b.lag_val))
    evidence('noncanonical identity %s %s: relfro W %.2e H %.2e Th %.2e (gate %.0e)' % (what, _name(dtype), got[0], got[1], got[2], tol))
    assert got[0] < tol and got[1] < tol and got[2] < 10 * tol, (what, got)


@pytest.mark.parametrize('dtype', [F32, F64])
def test_another_order_of_the_same_entries_gives_the_same_factors(dtype):
    raw, lags = _dirty(dtype), (1, 2, 5)
    f0 = _start(dtype, 24, 3)
    other = raw.reordered(4242)
    assert not np.array_equal(other.col_idx, raw.col_idx) and not np.array_equal(other.row_idx, raw.row_idx)
    a = run_session(raw, lags, f0, 3)[0]
    b = run_session(other, lags, f0, 3)[0]
    _close(a, b, dtype, 'entry order')


@pytest.mark.parametrize('path', ['rows', 'split'])
@pytest.mark.parametrize('dtype', [F32, F64])
def test_every_entry_twice_equals_half_the_ridge_weights(dtype, path, monkeypatch):
    """2 sum_e (y_e - w h)^2 + lambdaI (..) + lambdaAR (..) = 2 [ sum_e (..)^2 + lambdaI/2 (..) + lambdaAR/2 (..) ]: the duplicate-entry
    path against the product's own canonical path (a csr_matrix with sorted indices), no oracle involved."""
    _setenv(monkeypatch, path)
    p = synth.sparse_problem(n=N, T=T, k=6, nlag=3, density=DENSITY, dtype=dtype, seed=21)
    Y, lags = p['Y'], (1, 2, 3)
    coo = Y.tocoo()
    twice = doubled(RawSparse(coo.row, coo.col, coo.data, Y.shape, dtype, seed=5), seed=6)
    assert twice.nnz == 2 * Y.nnz
    f0 = _start(dtype, 40, 3)
    a, st_a, _, d = run_session(twice, lags, f0, 3)
    _assert_path(d, path, 40)
    half = dict(lambdaI=HYPER['lambdaI'] / 2, lambdaAR=HYPER['lambdaAR'] / 2, lambdaLag=HYPER['lambdaLag'])
    b = make_model(f0[0], f0[1], f0[2], lags)
    with Session(Y, b, missing=True, **half) as s:
        s.run(3); st_b = s.stats(3); s.download()
    _close(a, b, dtype, 'every entry twice (%s)' % path)
    assert all(abs(x['cg_iter'] - y['cg_iter']) <= 1 for x, y in zip(st_a, st_b))
    c = make_model(f0[0], f0[1], f0[2], lags)                             # at the full weights the doubled matrix IS another problem
    with Session(Y, c, missing=True, **HYPER) as s:
        s.run(3).download()
    assert relmax(a.H, c.H) > 1e-2


@pytest.mark.parametrize('dtype', [F32, F64])
def test_a_stored_zero_is_an_observation(dtype):
    """Zeros replaced by 1e-30 (nobody's test for `== 0` fires): the same factors.  Those entries removed: another problem."""
    raw, lags = _dirty(dtype), (1, 2, 5)
    f0 = _start(dtype, 24, 3)
    zero = raw.vals == 0
    assert 0.05 < zero.mean() < 0.15
    tiny = RawSparse.from_arrays(raw.shape, dtype, raw.row_ptr, raw.col_idx, np.where(raw.val_t == 0, dtype(1e-30), raw.val_t),
                                 raw.col_ptr, raw.row_idx, np.where(raw.val == 0, dtype(1e-30), raw.val))
    assert not np.any(tiny.val == 0) and np.count_nonzero(tiny.val != raw.val) == int(zero.sum())
    a = run_session(raw, lags, f0, 3)[0]
    b = run_session(tiny, lags, f0, 3)[0]
    c = run_session(raw.select(~zero, seed=7), lags, f0, 3)[0]
    _close(a, b, dtype, 'stored zeros vs 1e-30')
    evidence('noncanonical stored zeros dropped %s: relmax H %.2e (must exceed 1e-2)' % (_name(dtype), relmax(c.H, a.H)))
    assert relmax(c.H, a.H) > 1e-2


# ---- e. the full-observation path on a sparse Y -------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,k', [(F32, 16), (F64, 16), (F32, 70), (F64, 70)])
def test_full_observation_path_on_raw_sparse_input(dtype, k):
    """missing = 0 with the dirty sparse Y: Y^T W and Y H sum the entries as stored, sum y^2 runs over the entries."""
    raw, lags = _dirty(dtype), (1, 2, 3, 4, 7)
    f0 = _start(dtype, k, len(lags))
    m, _, _, d = run_session(raw, lags, f0, 3, missing=False)
    W, H, Th, _ = _oracle(dtype, k, lags, 3, missing=False)
    tol = TOL[_name(dtype)]['factor']
    evidence('noncanonical full-observation path %s k=%d (%s): relfro W %.2e H %.2e Th %.2e (gate %.0e)' % (
        _name(dtype), k, d, relfro(m.W, W), relfro(m.H, H), relfro(m.lag_val, Th), tol))
    assert relfro(m.W, W) < tol and relfro(m.H, H) < tol and relfro(m.lag_val, Th) < 10 * tol


# ---- f. resident-session features ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,path', [(F32, 'rows'), (F64, 'rows'), (F32, 'unfused'), (F64, 'unfused')])
def test_append_rows_of_a_dirty_block_equals_a_fresh_session_bit_for_bit(dtype, path, monkeypatch):
    """The grown CSR is the old rows then the new; every grown CSC column its old entries then the block's, shifted -- unsorted
    columns with repeats on both sides of the seam.  A fresh session over exactly those arrays continues with the same bits."""
    _setenv(monkeypatch, path)
    T0, Tn, n, k, lags = 240, 37, 60, 8, [1, 2, 6]
    head, tail = dirty_problem(T0, n, DENSITY, dtype, seed=31)[0], dirty_problem(Tn, n, DENSITY, dtype, seed=32)[0]
    whole = stacked(head, tail)
    assert whole.nnz == head.nnz + tail.nnz and whole.shape == (T0 + Tn, n)
    f0 = start_factors(T0, n, k, len(lags), dtype, seed=3)
    grown = make_model(f0[0], f0[1], f0[2], lags)
    with Session(_py(head), grown, missing=True, **HYPER) as s:
        _assert_path(s.describe(), path, k)
        s.run(3).download()
        first = make_model(grown.W, grown.H, grown.lag_val, grown.lag_set)
        s.append_rows(_py(tail))
        assert s.rows() == T0 + Tn
        grown2 = trmf.Model.initialize(whole, lags, k, seed=1, dtype=dtype, warm_start_model=first)
        s.model = grown2
        s.download()
        warm = trmf.Model.initialize(whole, lags, k, seed=1, dtype=dtype, warm_start_model=first)
        assert np.array_equal(grown2.W, warm.W) and np.array_equal(grown2.H, warm.H)
        s.run(3); st_g = s.stats(3); Jg = s.objective(); s.download()
    fresh = make_model(warm.W, warm.H, warm.lag_val, warm.lag_set)
    with Session(_py(whole), fresh, missing=True, **HYPER) as s:
        _assert_path(s.describe(), path, k)
        s.run(3); st_f = s.stats(3); Jf = s.objective(); s.download()
    assert [x['cg_iter'] for x in st_g] == [x['cg_iter'] for x in st_f] and Jg == Jf
    assert np.array_equal(grown2.W, fresh.W) and np.array_equal(grown2.H, fresh.H) and np.array_equal(grown2.lag_val, fresh.lag_val)


@pytest.mark.parametrize('dtype,k', [(F32, 16), (F64, 40), (F32, 80)])
def test_heldout_set_with_repeated_cells_and_stored_zeros(dtype, k):
    """Every stored entry of the held-out matrix is scored, a repeated cell once per copy and a stored zero as a truth of 0; the
    sums match NumPy over the entry list (tolerances of test_eval_heldout_matches_numpy_of_downloaded_factors)."""
    raw, lags = _dirty(dtype), (1, 2, 3)
    f0 = _start(dtype, k, 3)
    rng = np.random.RandomState(k)
    m = 3000
    rr, cc = rng.randint(0, T, m), rng.randint(0, N, m)
    rep = rng.randint(0, m, m // 4)                                        # a quarter again as repeats of cells already drawn
    rr, cc = np.concatenate([rr, rr[rep]]), np.concatenate([cc, cc[rep]])
    y = rng.uniform(0.5, 2.0, rr.size) * rng.choice([-1.0, 1.0], rr.size)
    y[rng.rand(rr.size) < 0.1] = 0.0
    ho = RawSparse(rr, cc, y, (T, N), dtype, seed=9)
    assert np.unique(rr * N + cc).size < ho.nnz
    model = make_model(f0[0], f0[1], f0[2], lags)
    with Session(_py(raw), model, missing=True, **HYPER) as s:
        s.run(2)
        s.set_heldout(_py(ho))
        sums, pred = s.eval_heldout_sums(predictions=True)
        s.download()
    rows = np.repeat(np.arange(T), np.diff(ho.row_ptr.astype(np.int64)))       # the set's CSR order, as stored
    cols, truth = ho.col_idx.astype(np.int64), ho.val_t.astype(np.float64)
    W, H = model.W.astype(np.float64), model.H.astype(np.float64)
    ref = np.einsum('ij,ij->i', W[rows], H[cols])
    bound = 4 * k * np.finfo(dtype).eps * np.einsum('ij,ij->i', np.abs(W[rows]), np.abs(H[cols]))
    assert pred.shape == (ho.nnz,) and np.all(np.abs(pred.astype(np.float64) - ref) <= bound + 1e-300)
    dlt, nz = ref - truth, truth != 0
    want = dict(sq_err=np.sum(dlt * dlt), abs_err=np.sum(np.abs(dlt)), abs_truth=np.sum(np.abs(truth)), rel_err=np.sum(np.abs(dlt[nz]) / np.abs(truth[nz])))
    assert sums['count'] == ho.nnz == rr.size and sums['count_nonzero'] == int(nz.sum()) < ho.nnz
    sum_tol = 1e-5 if dtype == F32 else 1e-12
    for key, v in want.items():
        assert abs(sums[key] - v) <= sum_tol * abs(v), (key, sums[key], v)


# ---- g. two ranks on one device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env', [{}, {'TRMF_FSHARD': 'shard', 'TRMF_GRAMX': 'shard'}], ids=['measured', 'sharded'])
def test_two_ranks_on_one_device_give_the_bits_of_one_rank(env, monkeypatch):
    """TRMF_DEVICES=0,0 on the dirty pattern: the F-phase cut by nnz over a col_ptr with the over-long column, the group path."""
    dtype, lags = F32, (1, 2, 3)
    raw = _dirty(dtype, 400, 300, 2)
    f0 = _start(dtype, 40, 3, 400, 300)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    monkeypatch.delenv('TRMF_DEVICES', raising=False)
    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = run_oneshot(raw, lags, f0, 3)
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two = run_oneshot(raw, lags, f0, 3)
    assert not np.array_equal(one.H, f0[1])
    assert np.array_equal(one.W, two.W) and np.array_equal(one.H, two.H) and np.array_equal(one.lag_val, two.lag_val)


# ---- h. repeated lags ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['rows', 'unfused'])
@pytest.mark.parametrize('lags', [(1, 1, 2), (1, 2, 3, 4, 4, 5, 6, 7, 9)], ids=['lags112', 'run4-then-repeat'])
@pytest.mark.parametrize('dtype', [F32, F64])
def test_repeated_lags_vs_restatement(dtype, lags, path, monkeypatch):
    """validate_problem accepts a lag set with repeats (ascending, not strictly); the reference computes with it (host tests).  The
    second set is a run of four consecutive lags followed by a repeat, which lands inside ar_lag_steps' grouping."""
    _setenv(monkeypatch, path)
    raw = _dirty(dtype)
    k = 16
    f0 = _start(dtype, k, len(lags))
    m, st, _, d = run_session(raw, lags, f0, 2)
    W, H, Th, log = _oracle(dtype, k, lags, 2)
    tol = TOL[_name(dtype)]['factor']
    evidence('noncanonical repeated lags %s %s %s (%s): relfro W %.2e H %.2e Th %.2e (gate %.0e); CG %s vs %s' % (
        _name(dtype), list(lags), path, d, relfro(m.W, W), relfro(m.H, H), relfro(m.lag_val, Th), tol,
        [x['cg_iter'] for x in st], [l['cg_iter'] for l in log]))
    _assert_path(d, path, k)
    assert np.all(np.isfinite(m.W)) and np.all(np.isfinite(m.H)) and np.all(np.isfinite(m.lag_val))
    assert relfro(m.W, W) < tol and relfro(m.H, H) < tol and relfro(m.lag_val, Th) < 10 * tol
