"""GPU (-m gpu): the online filter (trmf_session_assimilate: assim_factor_kernel, assim_chain_kernel, assim_err_kernel) on the
inputs the ALS solvers are already held to.  tests/test_gpu_online.py runs one designed input (T = 96, n = 50, lags (1, 2, 5),
values in (0, 1), a canonical CSR); here:

  A. lag-set geometry and shape edges of the chain (the LDS ring's base / wrap / seeding, the lag staging loop, ring versus global
     memory, chunks shorter than the reach, no lags, two real chunks), the ranks at the tile edges, assim_err_kernel beyond one
     256-stride trip;
  B. the per-row Cholesky solve as a direct solve: normwise backward error on an ill-conditioned problem, gated against the NumPy
     twin's own; exact scaling by 2^+-20;
  D. raw sparse arrays (cells stored several times, stored zeros, random entry order, a row longer than n, an emptied row)
     through assimilate, update and fit_noise, with the duplicate-cell reading of the training objective.

Gates of A and D: the two of test_gpu_online.py -- free-running relmax to the fp64 twin <= online_helpers.bound(dtype, the fp32
twin's distance), and the same bound per row teacher-forced (a failure names a row).  Small shapes: the file takes a few seconds.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as smat

import online_helpers as OH
from conditioning_helpers import U as UNIT
from helpers import evidence, make_model, relmax
from rawsparse_helpers import RawSparse, dirty_entries, doubled, stacked
from trmf import fit_noise, synth
from trmf.session import Session

pytestmark = pytest.mark.gpu

SUM_TOL = {np.float32: 1e-5, np.float64: 1e-12}             # tests/test_gpu_online.py's
DTYPES = [np.float32, np.float64]
IDS = ['float32', 'float64']
LAM = OH.LAMBDAS[0]


def _name(dtype):
    return np.dtype(dtype).name


def _run(d, dtype, lamI, lamAR, missing=True, storage='sparse', Y=None, W=None):
    """(downloaded model, sums, Wnew, describe) of one session over the input set after assimilate(d['first']).  Y: what the
    session trains on instead of the set's own matrix (given as the session is to hold it)."""
    model = make_model((d['W'] if W is None else W).astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    if Y is None:
        Y = d['Y'].astype(dtype)
        if storage == 'dense':
            Y = np.ascontiguousarray(Y.toarray())
    with Session(Y, model, lambdaI=lamI, lambdaAR=lamAR, lambdaLag=0.5, missing=missing) as s:
        sums, Wnew = s.assimilate(d['first'], return_latent=True)
        s.download()
        desc = s.describe()
    assert np.array_equal(Wnew, model.W[d['first']:])
    return model, sums, Wnew, desc


@functools.lru_cache(maxsize=None)
def _yard(k, density, lags, T, N, first, lamI, lamAR, missing):
    """(the fp64 twin, the fp32 twin's distance) of one generalised input, shared by the cases that use it (read only)."""
    return OH.yardstick_of(OH.inputs(k, density, lags, T, N, first), lamI, lamAR, missing, first)


def _gate(what, d, W, dtype, lamI, lamAR, missing, w64, dev32, Y=None, free=True, W0=None):
    """The two gates of tests/test_gpu_online.py::_gate; free=False prints the free-running distance without gating it."""
    first = d['first']
    b = OH.bound(dtype, dev32)
    got = relmax(W[first:], w64[first:])
    rows = OH.teacher_forced(d, W, lamI, lamAR, missing, first, Y=Y)
    worst = int(np.argmax(rows))
    evidence('online inputs %s %s lambdaI=%g lambdaAR=%g: relmax to the fp64 twin %.3e = %.2f x its bound %.3e (fp32 twin %.3e)%s; '
             'teacher-forced worst row %d: %.3e = %.2f x' % (what, _name(dtype), lamI, lamAR, got, got / b, b, dev32,
                                                             '' if free else ' [not gated]', first + worst, rows[worst], rows[worst] / b))
    assert np.array_equal(W[:first], (d['W'] if W0 is None else W0)[:first].astype(dtype))        # earlier rows keep their bits
    assert np.all(np.isfinite(W))
    if free:
        assert got <= b, (what, got, b)
    assert rows[worst] <= b, (what, 'row', first + worst, rows[worst], b)


# ---- A. lag-set geometry of the chain --------------------------------------------------------------------------------------------
WEEKLY = tuple(range(1, 25)) + tuple(range(168, 192))
# assim_chain_lds_bytes(k, nlag = 48, reach = 191) = 2 k (k + 1) s + 192 + (48 + 191) 64 s  for an element of s bytes
# (two factors of pitch k + 1; the lag set, 48 ints = 192 B, already a multiple of 16; Theta's 48 rows and the ring's 191 of 64):
#   fp64 k = 64:  66 560 + 192 + 122 368 = 189 120 B  > kLdsMax (160 KiB = 163 840 B): the global-memory form, unforced
#   fp64 k = 40:  26 240 + 192 + 122 368 = 148 800 B  a ring of 191 rows
#   fp32 k = 64:  33 280 + 192 +  61 184 =  94 656 B  a ring of 191 rows
#        name                   lags            T    first  n    (dtype, k) pairs                             environment
GEOMETRY = [
    ('lag-above-block', (1, 7, 30), 64, 40, 50, [(np.float32, 40), (np.float64, 7)], {}),          # a ring of 30 rows, 24 new rows
    ('first-row-is-reach', (1, 2, 24), 48, 24, 50, [(np.float32, 40), (np.float64, 7)], {}),       # the ring seeded from row 0
    ('lags-1-to-70', tuple(range(1, 71)), 120, 96, 50, [(d, k) for d in DTYPES for k in (7, 40)], {}),      # a second trip of l += 64
    ('weekly-global-unforced', WEEKLY, 240, 216, 50, [(np.float64, 64)], {}),
    ('weekly-ring', WEEKLY, 240, 216, 50, [(np.float64, 40), (np.float32, 64)], {}),
    ('no-lags', (), 64, 40, 50, [(np.float32, 40), (np.float64, 7)], {}),                          # reach = 0, nlag = 0
    ('repeated-lag', (1, 2, 2, 5), 96, 72, 50, [(np.float32, 40), (np.float64, 7)], {}),           # summed in lag-set order, twice
]
# (an unsorted lag set such as (5, 1, 2) never reaches the filter: trmf_session_create refuses a lag set that is not ascending --
# "lag_set must be ascending", every ALS kernel takes the last lag for the largest -- so it has no device case; the twin's order
# is checked on the host, tests/test_online_host.py)
GEOMETRY = [(n, l, T, f, N, dt, k, env) for n, l, T, f, N, pairs, env in GEOMETRY for dt, k in pairs]


@pytest.mark.parametrize('name,lags,T,first,N,dtype,k,env', GEOMETRY, ids=['%s-%s-k%d' % (g[0], _name(g[5]), g[6]) for g in GEOMETRY])
def test_lag_set_geometry_matches_the_numpy_twin(name, lags, T, first, N, dtype, k, env, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    lamI, lamAR = LAM
    d = OH.inputs(k, 0.3, lags, T, N, first)
    w64, dev32 = _yard(k, 0.3, lags, T, N, first, lamI, lamAR, True)
    model, sums, _, _ = _run(d, dtype, lamI, lamAR)
    _gate('%s k=%d' % (name, k), d, model.W, dtype, lamI, lamAR, True, w64, dev32)
    assert sums['rows'] == T - first and sums['entries'] == d['Y'][first:].nnz


def test_weekly_ring_and_forced_global_form_give_the_same_bits(monkeypatch):
    """fp64 k = 40 over the weekly lag set: TRMF_FORECAST_GLOBAL=1 reads the rows from global memory where the ring of 191 fits."""
    dtype, k, T, first = np.float64, 40, 240, 216
    lamI, lamAR = LAM
    d = OH.inputs(k, 0.3, WEEKLY, T, OH.N, first)
    w64, dev32 = _yard(k, 0.3, WEEKLY, T, OH.N, first, lamI, lamAR, True)
    ring = _run(d, dtype, lamI, lamAR)[0].W
    monkeypatch.setenv('TRMF_FORECAST_GLOBAL', '1')
    glob = _run(d, dtype, lamI, lamAR)[0].W
    _gate('weekly-global-forced k=%d' % k, d, glob, dtype, lamI, lamAR, True, w64, dev32)
    assert np.array_equal(ring, glob)


@pytest.mark.parametrize('dtype,k', [(np.float32, 40), (np.float64, 7), (np.float32, 7), (np.float64, 40)],
                         ids=['float32-k40', 'float64-k7', 'float32-k7', 'float64-k40'])
def test_chunks_shorter_than_the_reach_give_the_bits_of_one_chunk(dtype, k, monkeypatch):
    """Lags (1, 3, 24), 24 new rows: with TRMF_ASSIM_CHUNK = 7 and = 1 every pass seeds its ring of 24 rows partly from the rows
    the passes before it wrote (Wnew), partly from W, at another base = row0 % 24."""
    lags, T, first = (1, 3, 24), 72, 48
    lamI, lamAR = LAM
    d = OH.inputs(k, 0.3, lags, T, OH.N, first)
    w64, dev32 = _yard(k, 0.3, lags, T, OH.N, first, lamI, lamAR, True)
    one = _run(d, dtype, lamI, lamAR)[0].W
    _gate('chunk-below-reach unforced k=%d' % k, d, one, dtype, lamI, lamAR, True, w64, dev32)
    for chunk in ('7', '1'):
        monkeypatch.setenv('TRMF_ASSIM_CHUNK', chunk)
        got = _run(d, dtype, lamI, lamAR)[0].W
        _gate('chunk-below-reach chunk=%s k=%d' % (chunk, k), d, got, dtype, lamI, lamAR, True, w64, dev32)
        assert np.array_equal(got, one), chunk


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_two_real_chunks(dtype):
    """260 new rows, no knob: a pass of kAssimChunk = 256 rows and one of 4.  Teacher-forced gate only: GATE = 8 was sized for a
    chain of 24 rows; the free-running distance over 260 rows is printed next to the fp32 twin's."""
    lags, T, first, N, k = (1, 2, 5), 300, 40, 20, 16
    lamI, lamAR = LAM
    d = OH.inputs(k, 0.3, lags, T, N, first)
    w64, dev32 = _yard(k, 0.3, lags, T, N, first, lamI, lamAR, True)
    model, sums, _, _ = _run(d, dtype, lamI, lamAR)
    _gate('two-chunks 260 rows k=%d' % k, d, model.W, dtype, lamI, lamAR, True, w64, dev32, free=False)
    assert sums['rows'] == 260 and sums['entries'] == d['Y'][first:].nnz
    for key, W in (('sq_err_before', d['W'].astype(dtype)), ('sq_err_after', model.W)):
        want, _ = OH.sq_err(d, W, first, True)
        assert abs(sums[key] - want) <= SUM_TOL[dtype] * abs(want), (key, sums[key], want)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('k', [8, 9, 17, 33, 48, 49, 63])
def test_ranks_at_the_tile_edges(k, dtype):
    lamI, lamAR = LAM
    d = OH.inputs(k)
    w64, dev32 = OH.yardstick(k, lamI, lamAR)
    model, sums, _, _ = _run(d, dtype, lamI, lamAR)
    _gate('tile-edge k=%d' % k, d, model.W, dtype, lamI, lamAR, True, w64, dev32)
    assert sums['rows'] == OH.TN and sums['entries'] == d['Y'][OH.FIRST:].nnz


#           name            storage   missing density
ERR_MODES = [('full-dense', 'dense', False, 0.3), ('full-sparse', 'sparse', False, 0.3), ('every-cell-stored', 'sparse', True, 1.0)]


@pytest.mark.parametrize('name,storage,missing,density', ERR_MODES, ids=[m[0] for m in ERR_MODES])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('N', [300, 257])
def test_error_sums_beyond_one_trip_of_256(N, dtype, name, storage, missing, density):
    """n = 300 and n = 257: the second trip of assim_err_kernel's series loop (j += 256, missing = 0) and of its entry loop
    (p += 256, density 1.0: every new row but the two designed ones stores n entries)."""
    lags, T, first, k = OH.LAGS, 64, 40, 16
    lamI, lamAR = LAM
    d = OH.inputs(k, density, lags, T, N, first)
    w64, dev32 = _yard(k, density, lags, T, N, first, lamI, lamAR, missing)
    model, sums, _, _ = _run(d, dtype, lamI, lamAR, missing, storage)
    _gate('err-sums n=%d %s' % (N, name), d, model.W, dtype, lamI, lamAR, missing, w64, dev32)
    if missing:
        assert np.diff(d['Y'].indptr)[first:].max() == N > 256
    want_entries = d['Y'][first:].nnz if missing else (T - first) * N
    assert sums['rows'] == T - first and sums['entries'] == want_entries
    for key, W in (('sq_err_before', d['W'].astype(dtype)), ('sq_err_after', model.W)):
        want, cnt = OH.sq_err(d, W, first, missing)
        evidence('online inputs err-sums n=%d %s %s %s: device %.17g, fp64 NumPy %.17g, rel %.2e (gate %.0e)' % (
            N, name, _name(dtype), key, sums[key], want, abs(sums[key] - want) / abs(want), SUM_TOL[dtype]))
        assert cnt == want_entries and abs(sums[key] - want) <= SUM_TOL[dtype] * abs(want), (key, sums[key], want)


# ---- B. conditioning of the per-row solve ----------------------------------------------------------------------------------------
#             name          environment                  missing storage   describe() must hold
HARD_PATHS = [('rows', {}, True, 'sparse', ''),
              ('packed-gram', {'TRMF_NO_HV_TILE': '1'}, True, 'sparse', 'unfused'),
              ('full-dense', {}, False, 'dense', '')]


@pytest.mark.parametrize('scale,lamI,lamAR', OH.HARD_CASES, ids=['scale%g-lamI%g-lamAR%g' % c for c in OH.HARD_CASES])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('k', OH.HARD_RANKS)
def test_backward_error_of_the_per_row_solve(k, dtype, scale, lamI, lamAR, monkeypatch):
    """Per new row of online_helpers.hard_filter_problem: the normwise backward error eta of the device's row as a solution of
    A_i x = b_i + lambdaAR p_i (the system from exact sums of the fp64 products of the stored values, p_i in the element type from
    the device's own earlier rows).  Gate: the worst row <= 4 x max(the worst row of filter_rows in the same element type on the
    same arrays, measured the same way on its own rows; u) -- the 4 of the F- and Theta-solves, u one rounding of the stored row."""
    d = OH.hard_filter_problem(k, scale)
    u = UNIT[_name(dtype)]
    systems, twin = {}, {}
    for missing, Y in ((True, d['Y']), (False, d['Yd'])):
        systems[missing] = OH.row_systems(d, dtype, lamI, lamAR, missing)
        Wt = OH.twin(d, dtype, lamI, lamAR, missing, d['first'], Y=Y)
        twin[missing] = OH.row_backward_errors(d, systems[missing], Wt, dtype, lamAR)
    cond = max(float(np.linalg.cond(A)) for A, _ in systems[True])
    for name, env, missing, storage, must in HARD_PATHS:
        with monkeypatch.context() as mp:
            for key, v in env.items():
                mp.setenv(key, v)
            model, _, _, desc = _run(d, dtype, lamI, lamAR, missing, storage)
        assert must in desc, desc
        eta = OH.row_backward_errors(d, systems[missing], model.W, dtype, lamAR)
        worst, tw = int(np.argmax(eta)), float(twin[missing].max())
        gate = 4.0 * max(tw, u)
        evidence('online inputs conditioning %s k=%d scale=%g lambdaI=%g lambdaAR=%g %s (cond up to %.1e): device eta %.2f u (row %d, '
                 '%d entries), twin eta %.2f u, ratio %.2f (gate: 4 x max(twin, u))' % (
                     _name(dtype), k, scale, lamI, lamAR, name, cond, eta[worst] / u, d['first'] + worst,
                     OH.HARD_LENGTHS[worst] if missing else OH.HARD_N, tw / u, eta[worst] / max(tw, u)))
        assert np.array_equal(model.W[:d['first']], d['W'][:d['first']].astype(dtype))
        assert eta[worst] <= gate, (name, 'row', d['first'] + worst, eta[worst] / u, tw / u)


@pytest.mark.parametrize('storage,missing', [('sparse', True), ('dense', False)], ids=['observed', 'full'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('which', ['standard', 'hard'])
def test_scaling_the_values_by_a_power_of_two_scales_the_rows_bit_for_bit(which, dtype, storage, missing):
    """Nothing in the filter is non-linear in the observed values and W: both times 2^+-20 give the new rows times 2^+-20."""
    lamI, lamAR = (0.5, 0.5) if which == 'standard' else (1e-3, 1e-3)
    d = OH.inputs(40) if which == 'standard' else OH.hard_filter_problem(40, 1.0)
    base = _run(d, dtype, lamI, lamAR, missing, storage)[0].W
    for f in (2.0 ** 20, 2.0 ** -20):
        Y = (d['Y'] * np.float32(f)).astype(dtype)
        Y = np.ascontiguousarray(Y.toarray()) if storage == 'dense' else smat.csr_matrix(Y)
        got = _run(d, dtype, lamI, lamAR, missing, storage, Y=Y, W=d['W'] * np.float32(f))[0].W
        assert np.array_equal(got, base * dtype(f)), (which, f)


# ---- D. raw sparse arrays --------------------------------------------------------------------------------------------------------
DLAM = OH.LAMBDAS[1]                                       # (0.5, 0.5): the observations, not the prior, decide the rows
#              name           environment                                         missing  describe() must hold
DIRTY_PATHS = [('rows', {}, True, ''),
               ('split-rows', {'TRMF_LONG_ROW': '24', 'TRMF_LONG_CHUNK': '32'}, True, 'split rows'),
               ('packed-gram', {'TRMF_NO_HV_TILE': '1'}, True, 'unfused'),
               ('sparse-full', {}, False, '')]


@functools.lru_cache(maxsize=None)
def _dirty_parts():
    """A dirty history (72 x 50) and a dirty block of 24 new rows (rawsparse_helpers.dirty_entries, fp32 values uniform in (0, 1)
    like the standard input's): about 15 % of the cells stored twice with different values, 10 % stored zeros, one row with
    n + 9 entries, one emptied row (and column), a random entry order drawn independently for the CSR and the CSC."""
    rng = np.random.RandomState(77)
    mask, vals = rng.rand(OH.T, OH.N) < 0.3, rng.rand(OH.T, OH.N)
    parts = []
    for lo, hi, seed in ((0, OH.FIRST, 5), (OH.FIRST, OH.T, 6)):
        e = dirty_entries(mask[lo:hi], vals[lo:hi], seed=seed)
        parts.append(RawSparse(e['rows'], e['cols'], e['vals'], (hi - lo, OH.N), np.float32, seed=seed + 10))
        assert np.diff(parts[-1].row_ptr.astype(np.int64)).max() > OH.N and np.diff(parts[-1].row_ptr.astype(np.int64)).min() == 0
        cells = e['rows'] * OH.N + e['cols']
        assert np.unique(cells).size < cells.size and np.any(parts[-1].vals == 0)
    return tuple(parts)


def _scipy(raw, dtype):
    """The raw CSR arrays as a scipy matrix, NOT canonicalised: what filter_rows is fed."""
    Y = smat.csr_matrix((raw.val_t.astype(dtype), raw.col_idx.astype(np.int32), raw.row_ptr.astype(np.int32)), shape=raw.shape)
    assert Y.nnz == raw.nnz
    return Y


def _dirty_gate(what, d, raw, dtype, lamI, lamAR, missing, W):
    """Both references on the raw arrays: filter_rows fed the un-canonicalised CSR (the part-A gates) and the per-entry fp64 model."""
    Y = _scipy(raw, np.float32)
    w64, dev32 = OH.yardstick_of(d, lamI, lamAR, missing, d['first'], Y=Y)
    _gate(what, d, W, dtype, lamI, lamAR, missing, w64, dev32, Y=Y)
    went = OH.entry_filter(raw.rows, raw.cols, raw.vals, d['W'], d['H'], d['lag_set'], d['theta'], d['first'], lamI, lamAR, missing)
    assert relmax(went[d['first']:], w64[d['first']:]) <= 1e-10                  # the two references agree
    b = OH.bound(dtype, dev32)
    assert relmax(W[d['first']:], went[d['first']:]) <= b
    return b


@pytest.mark.parametrize('name,env,missing,must', DIRTY_PATHS, ids=[p[0] for p in DIRTY_PATHS])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('k', [7, 40])
def test_assimilate_on_raw_sparse_arrays(k, dtype, name, env, missing, must, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    lamI, lamAR = DLAM
    d = OH.inputs(k)
    head, tail = _dirty_parts()
    raw = stacked(head, tail)
    model, sums, _, desc = _run(d, dtype, lamI, lamAR, missing, Y=raw.astype(dtype).pymatrix())
    assert must in desc, desc
    _dirty_gate('dirty %s k=%d' % (name, k), d, raw, dtype, lamI, lamAR, missing, model.W)
    # the sums on the training objective's reading: every stored entry counts (missing); ||Y||^2 over the stored values (not missing)
    assert sums['rows'] == OH.TN and sums['entries'] == (tail.nnz if missing else OH.TN * OH.N)
    for key, W in (('sq_err_before', d['W'].astype(dtype)), ('sq_err_after', model.W)):
        want, cnt = OH.sq_err_entries(raw.rows, raw.cols, raw.vals, W, d['H'], OH.FIRST, OH.T, missing)
        merged, _ = OH.sq_err(d, W, OH.FIRST, missing, Y=raw.canonical())
        evidence('online inputs dirty %s k=%d %s %s: device %.17g, per-entry fp64 %.17g (rel %.2e, gate %.0e); duplicates summed first: %.17g' % (
            name, k, _name(dtype), key, sums[key], want, abs(sums[key] - want) / abs(want), SUM_TOL[dtype], merged))
        assert cnt == sums['entries'] and abs(sums[key] - want) <= SUM_TOL[dtype] * abs(want), (key, sums[key], want)
        assert abs(merged - want) > 10 * SUM_TOL[dtype] * abs(want)               # the other reading is a number this gate tells apart


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('k', [7, 40])
def test_identities_on_raw_sparse_arrays_that_need_no_oracle(k, dtype):
    lamI, lamAR = DLAM
    d = OH.inputs(k)
    head, tail = _dirty_parts()
    raw = stacked(head, tail)
    a = _run(d, dtype, lamI, lamAR, Y=raw.astype(dtype).pymatrix())[0].W
    b = _dirty_gate('dirty identities k=%d' % k, d, raw, dtype, lamI, lamAR, True, a)
    new = slice(OH.FIRST, None)
    # another order of the same entries, in both orientations
    other = stacked(head.reordered(4242), tail.reordered(4243))
    assert not np.array_equal(other.col_idx, raw.col_idx) and not np.array_equal(other.row_idx, raw.row_idx)
    o = _run(d, dtype, lamI, lamAR, Y=other.astype(dtype).pymatrix())[0].W
    # every new-row entry stored twice == half the ridge weights (the doubling is exact; the summation order differs)
    twice = stacked(head, doubled(tail, seed=9))
    assert twice.nnz == raw.nnz + tail.nnz
    t = _run(d, dtype, lamI, lamAR, Y=twice.astype(dtype).pymatrix())[0].W
    h = _run(d, dtype, lamI / 2, lamAR / 2, Y=raw.astype(dtype).pymatrix())[0].W
    # a stored zero is an observation: 1e-30 in its place gives the same rows, the entry removed gives others
    zero = raw.vals == 0
    assert 0.05 < zero[raw.rows >= OH.FIRST].mean() < 0.2
    tiny = RawSparse.from_arrays(raw.shape, np.float32, raw.row_ptr, raw.col_idx, np.where(raw.val_t == 0, np.float32(1e-30), raw.val_t),
                                 raw.col_ptr, raw.row_idx, np.where(raw.val == 0, np.float32(1e-30), raw.val))
    z = _run(d, dtype, lamI, lamAR, Y=tiny.astype(dtype).pymatrix())[0].W
    dropped = _run(d, dtype, lamI, lamAR, Y=raw.select(~zero, seed=7).astype(dtype).pymatrix())[0].W
    got = dict(order=relmax(o[new], a[new]), twice=relmax(t[new], h[new]), zeros=relmax(z[new], a[new]), dropped=relmax(dropped[new], a[new]))
    evidence('online inputs dirty identities k=%d %s: another order %.3e, every entry twice vs half the weights %.3e, zeros as 1e-30 %.3e '
             '(bound %.3e); zeros dropped %.3e' % (k, _name(dtype), got['order'], got['twice'], got['zeros'], b, got['dropped']))
    assert got['order'] <= b and got['twice'] <= b and got['zeros'] <= b
    assert got['dropped'] > 100 * b                                               # ... and that is another problem


@pytest.mark.parametrize('missing', [True, False], ids=['observed', 'sparse-full'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_update_of_a_dirty_block_equals_append_rows_then_assimilate(dtype, missing):
    k = 16
    d = OH.inputs(k)
    head, tail = (p.astype(dtype) for p in _dirty_parts())
    mk = lambda: make_model(d['W'][:OH.FIRST].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    a, b = mk(), mk()
    with Session(head.pymatrix(), a, missing=missing, **synth.HYPER) as s:
        s.run(2)
        s.append_rows(tail.pymatrix())
        rolled = make_model(np.zeros((OH.T, k), dtype), a.H, a.lag_val, a.lag_set)
        s.model = rolled
        want = s.assimilate(OH.FIRST)
        s.download()
    with Session(head.pymatrix(), b, missing=missing, **synth.HYPER) as s:
        s.run(2)
        got = s.update(tail.pymatrix())
        assert s.rows() == OH.T
        grown = s.download()
    assert got == want and got['rows'] == OH.TN and got['entries'] == (tail.nnz if missing else OH.TN * OH.N)
    assert np.array_equal(grown.W, rolled.W) and np.array_equal(grown.H, rolled.H) and np.array_equal(grown.lag_val, rolled.lag_val)
    assert np.all(np.isfinite(grown.W)) and not np.array_equal(grown.W[OH.FIRST:], np.zeros((OH.TN, k), dtype))


U52 = 2.0 ** -52                                            # tests/test_gpu_uncertainty.py's unit


def _noise_bounds(raw, W, H, mode):
    """Per series: the bound on |device sq_j - NumPy's| of tests/test_gpu_uncertainty.py::_sigma2_bounds, restated per stored
    entry: a dot product of k fp64 fmas is off by delta = (k + 2) U (|y| + |w| . |h|), a squared residual by 2 |r| delta +
    delta^2, a sum of m terms by m U sum |terms|.  On sparse storage with missing = 0 the terms are p^2 per cell and
    y (y - 2 p) per entry (3 more roundings), which cancel in part: their absolute values are summed."""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    k, T, n = W.shape[1], raw.shape[0], raw.shape[1]
    r, c, y = raw.rows, raw.cols, raw.vals.astype(np.float64)
    absdot, P = np.abs(W).dot(np.abs(H).T), W.dot(H.T)
    if mode == 'observed-sparse':
        res = y - P[r, c]
        delta = (k + 2) * U52 * (np.abs(y) + absdot[r, c])
        terms, err = res * res, 2 * np.abs(res) * delta + delta * delta
        cnt = np.bincount(c, minlength=n).astype(np.float64)
        mag = np.bincount(c, weights=terms, minlength=n)
        return np.bincount(c, weights=err, minlength=n) + cnt * U52 * mag, cnt
    if mode == 'full-sparse':
        dp = (k + 2) * U52 * absdot
        cell = (2 * np.abs(P) * dp + dp * dp).sum(axis=0)
        entry = 2 * np.abs(y) * dp[r, c] + 3 * U52 * (y * y + 2 * np.abs(y * P[r, c]))
        mag = (P * P).sum(axis=0) + np.bincount(c, weights=np.abs(y * (y - 2 * P[r, c])), minlength=n)
        m = T + np.bincount(c, minlength=n)
        return cell + np.bincount(c, weights=entry, minlength=n) + m * U52 * mag, np.full(n, float(T))
    Yd = raw.coo().toarray().astype(np.float64)                 # full-dense: the caller's array holds one value per cell
    res = Yd - P
    delta = (k + 2) * U52 * (np.abs(Yd) + absdot)
    return (2 * np.abs(res) * delta + delta * delta).sum(axis=0) + T * U52 * (res * res).sum(axis=0), np.full(n, float(T))


NOISE_MODES = [('observed-sparse', True, 'sparse'), ('full-sparse', False, 'sparse'), ('full-dense', False, 'dense')]


@pytest.mark.parametrize('name,missing,storage', NOISE_MODES, ids=[m[0] for m in NOISE_MODES])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('k', [7, 40])
def test_fit_noise_on_raw_sparse_arrays(k, dtype, name, missing, storage):
    """sigma2 of Session.fit_noise on the dirty matrix against trmf.uncertainty.fit_noise fed the same entries: one residual per
    stored entry (missing), ||Y||^2 over the stored values (sparse storage, not missing), the caller's cell values (dense)."""
    d = OH.inputs(k)
    raw = stacked(*_dirty_parts()).astype(dtype)
    dense = raw.coo().toarray()
    assert dense.dtype == dtype
    model = make_model(d['W'].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    with Session(np.ascontiguousarray(dense) if storage == 'dense' else raw.pymatrix(), model, lambdaLag=0.5, missing=missing) as s:
        stats = s.fit_noise()
        sigma2, _ = s.noise()
    ref_s2, _, info = fit_noise(model.W, model.H, model.lag_set, model.lag_val, dense if storage == 'dense' else raw.coo(), missing)
    bound, cnt = _noise_bounds(raw, model.W, model.H, name)
    assert np.array_equal(info['cnt'], cnt)
    has = cnt > 0
    ratio = np.abs(sigma2[has] - ref_s2[has]) * cnt[has] / bound[has]
    pooled_ratio = abs(stats['pooled_sigma2'] - info['pooled']) * cnt.sum() / bound.sum()
    merged = fit_noise(model.W, model.H, model.lag_set, model.lag_val, raw.canonical(), missing)[2]['sq']
    moved = np.abs(merged - info['sq'])
    other = moved.max() / info['sq'].max()
    evidence('online inputs dirty fit_noise k=%d %s %s: sigma2 measured / bound max %.3f, pooled %.3f; pooled sigma2 device %.17g NumPy %.17g; '
             'duplicates summed first moves a series sum by %.2e' % (k, _name(dtype), name, ratio.max(), pooled_ratio,
                                                                   stats['pooled_sigma2'], info['pooled'], other))
    assert ratio.max() <= 1.0 and pooled_ratio <= 1.0
    assert stats['series_pooled'] == int((~has).sum()) == info['series_pooled']
    if storage == 'sparse':
        assert moved.max() > 1e6 * bound.max()                                    # the reading matters on this input
