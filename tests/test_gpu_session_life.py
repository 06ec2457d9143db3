"""GPU (-m gpu): a resident session through a life of interleaved edits -- slide / append_rows, change_series, revise and the
update(...) front end in every order -- against the host twin of tests/session_life_helpers.py.  The sibling files test each edit
once, on a session trmf_session_create built a moment earlier; here each edit finds the state the others left: the absorbed prefixes
and the live generation of the loading statistics, the compacted held-out list, the mark, the storage generations of the pool.

The contract is the siblings': after every step the session IS the session trmf_session_create builds from the twin's arrays and
the current factors, so both return the same bits from then on.  The statistics are held to the twin's own distance from the fp64
direct ridge (adapt_helpers.bound), the held-out predictions also to the textbook bound of a dot product.  Small shapes: a window of
40 rows, 38 series and 12 to add, blocks of 4 rows, batches of 30 cells."""
import numpy as np
import pytest

import adapt_helpers as AH
import churn_helpers as CH
import online_helpers as OH
import session_life_helpers as LH
from helpers import evidence, make_model, relmax
from trmf.session import Session

pytestmark = pytest.mark.gpu

DTYPES = [(np.float32, 40), (np.float64, 7)]
DT_IDS = ['float32-k40', 'float64-k7']
HYPER = dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5)
POOL_UNIT = 256                          # bytes: what DevicePool rounds every request up to, the smallest block it hands out


def _start(tw, d, hyper=HYPER):
    """A session on the twin's first window with the design's factors."""
    dt = tw.dtype.type
    s = Session(tw.session_Y(), make_model(d['W'][:tw.T].astype(dt), d['H'][:tw.n].astype(dt), d['theta'].astype(dt), d['lag_set']),
                missing=tw.missing, **hyper)
    if tw.tr is not None:
        s.model.transform = tw.tr
        s.set_transform(tw.tr)
    return s


def _factors(s):
    m = s.download()
    return m.W.copy(), m.H.copy(), m.lag_val.copy()


def _fresh(tw, d, factors, hyper=HYPER):
    """trmf_session_create on the twin's arrays, the given factors and the twin's transform coefficients."""
    f = Session(tw.session_Y(), make_model(factors[0], factors[1], factors[2], d['lag_set']), missing=tw.missing, **hyper)
    if tw.tr is not None:
        f.set_transform(tw.tr)
    return f


def _probe(s):
    s.run(1)
    W, H, Th = _factors(s)
    return dict(W=W, H=H, theta=Th, J=np.float64(s.objective()), Y3=s.forecast(3))


def _same_counts(op, got, want):
    """The sums a call returned against the twin's counts."""
    if op.kind == 'update':
        sums, adapted = got if isinstance(got, tuple) else (got, None)
        assert sums['rows'] == want['slide']['rows_appended']
        if 'revise' in want:
            assert LH.counts_of(sums['revise'], want['revise']) == want['revise']
        if adapted is not None:
            assert LH.counts_of(adapted, want['adapt']) == want['adapt']
    elif op.kind != 'stats' or op.label == 'adapt':
        assert LH.counts_of(got, want) == want, (op, got, want)


def _refused_calls(s, tw):
    """One refused call of each kind: the session stays what it was."""
    before = _factors(s)
    with pytest.raises(RuntimeError, match='largest lag'):
        s.slide(None, tw.T - LH.REACH)                                        # REACH rows left: one too few
    with pytest.raises(ValueError, match='flags'):
        s.change_series(np.ones(tw.n + 1, dtype=bool))
    with pytest.raises(RuntimeError, match='named twice'):
        s.revise([4, 7, 4], [9, 9, 9], np.ones(3, dtype=tw.dtype))
    assert s.rows() == tw.T and s.model.n == tw.n
    for a, b in zip(before, _factors(s)):
        assert np.array_equal(a, b)


def _life(form, storage, missing, transform, dtype, k, sequence, refuse_after=None):
    """The sequence on one session; after every step a fresh session on the twin's arrays must give the same bits.  Returns the
    number of steps."""
    d = OH.inputs(k)
    tw = LH.Twin(k, dtype, storage, missing, transform)
    fresh, steps = None, 0
    with _start(tw, d) as s:
        s.run(1)
        try:
            for step, op in enumerate(sequence(tw)):
                want = tw.apply(op)
                _same_counts(op, LH.play(s, op), want)
                assert s.rows() == tw.T and s.model.n == tw.n and s.model.m == tw.T
                if fresh is not None:
                    fresh.close()
                fresh = _fresh(tw, d, _factors(s))
                CH.assert_same(_probe(s), _probe(fresh), (form, step, op.label))
                if step + 1 == refuse_after:
                    _refused_calls(s, tw)
                steps += 1
            CH.assert_same(CH.after(s, tw.T), CH.after(fresh, tw.T), (form, 'the end'))
        finally:
            if fresh is not None:
                fresh.close()
    return steps


# ---- a. every step equals a fresh session -------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('name', ['all-pairs', 'edges'])
@pytest.mark.parametrize('form,storage,missing,transform', LH.FORMS, ids=[f[0] for f in LH.FORMS])
def test_every_step_of_a_designed_life_equals_a_fresh_session(form, storage, missing, transform, name, dtype, k):
    """all-pairs: 37 ops in which every ordered pair of {slide with a block, retire only, append only, churn that retires and adds,
    churn that retires, revise} is adjacent once.  edges: a revise that deletes a cell an earlier one inserted, that replaces both
    copies of a doubled cell in a row a slide has moved, in a row the previous slide appended, in the first and the last row, in a
    series the previous churn added; a slide that retires revised rows; a retire down to the largest lag + 1 rows, then appends.
    After every step: run(1), download(), objective() and forecast(3) of the session and of a fresh one on the twin's arrays give
    the same bits; at the end churn_helpers.after of both.  The sums of every call are the twin's counts."""
    steps = _life(form, storage, missing, transform, dtype, k, LH.SEQUENCES[name])
    assert steps == {'all-pairs': 37, 'edges': 11}[name]
    evidence('session life %s %s %s: %d steps, each bit for bit a fresh session on the host twin' % (name, form, np.dtype(dtype).name, steps))


RANDOM = [f + (seed, i) for f in LH.FORMS for i, seed in enumerate(LH.SEEDS[f[0]])]


@pytest.mark.parametrize('form,storage,missing,transform,seed,i', RANDOM, ids=['%s-seed%d' % (c[0], c[4]) for c in RANDOM])
def test_every_step_of_a_random_life_equals_a_fresh_session(form, storage, missing, transform, seed, i):
    """12 random ops per seed, the arguments drawn so that the twin says each call is legal; the element types alternate."""
    dtype, k = DTYPES[i % 2]
    assert _life(form, storage, missing, transform, dtype, k, lambda tw: LH.random_life(tw, seed)) == LH.RANDOM_STEPS
    evidence('session life random seed %d %s %s: %d steps, each bit for bit a fresh session on the host twin' % (seed, form, np.dtype(dtype).name, LH.RANDOM_STEPS))


@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
def test_the_front_end_through_six_ticks_and_a_churn(dtype, k):
    """update(block, window=N, revisions=, adapt=True, downdate_stats=True): every tick revises cells of rows the same tick
    retires (revised['first_row'] - retire is negative).  Bit for bit the calls by hand on a second session -- revise(update_stats),
    slide(downdate_stats), assimilate, adapt_series -- the flags of the twin after every tick, and at the end a fresh session on the
    twin's arrays."""
    d = OH.inputs(k)
    gamma = 0.95
    tw = LH.Twin(k, dtype, 'sparse', True)
    with _start(tw, d) as s, _start(tw, d) as h:
        for step, op in enumerate(LH.frontend(tw, gamma)):
            rows_before = tw.T
            want = tw.apply(op)
            got = LH.play(s, op)
            _same_counts(op, got, want)
            if op.kind == 'update':
                if step == 0:
                    h.init_series_stats(gamma)
                rv = h.revise(op.revisions[0], op.revisions[1], op.revisions[2], update_stats=True)
                retire = rows_before + LH.STEP - LH.N
                assert rv['first_row'] - retire < 0 and rv['stats_carried']
                h.slide(op.block.pymatrix(), retire, True)
                by_hand = (dict(h.assimilate(rows_before - retire), revise=rv), h.adapt_series())
                assert got == by_hand
            else:
                assert LH.play(h, op) == got and got['stats_carried'] and got['fitted']
            info = s.series_stats_info()
            assert {key: info[key] for key in ('valid', 'stale', 'absorbed_rows')} == tw.stats_info() and info['forget'] == gamma
            assert h.series_stats_info() == info and s.rows() == tw.T == LH.N
            for a, b in zip(_factors(s), _factors(h)):
                assert np.array_equal(a, b), (step, op.label)
        with _fresh(tw, d, _factors(s)) as f:
            CH.assert_same(CH.after(s, tw.T), CH.after(f, tw.T), 'front end')
    evidence('session life front end %s k=%d: 6 ticks of update(window, revisions, adapt, downdate_stats) and a churn, each bit for bit the calls by hand; the end a fresh session'
             % (np.dtype(dtype).name, k))


# ---- b. the held-out set ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
def test_the_heldout_set_through_slides_churns_and_a_revise(dtype, k):
    """slide -> churn -> revise -> slide -> churn under a held-out set of 9120 positions (5376 at the end: several chunks of both
    compactions throughout).  After every step the sums and the predictions, in set order, are bit for bit those of a fresh
    set_heldout of the twin's list on a fresh session; and independently of any kernel the count is the twin's and every prediction
    lies within k eps sum_d |w_td h_jd| of the fp64 dot of the downloaded factors at the twin's (row, series) -- the textbook bound
    of a k-term dot product, which a position remapped wrongly misses by orders of magnitude.  The noise and the forecast scores
    stay through a slide and a revise and are reset by a churn."""
    d = OH.inputs(k)
    tw = LH.Twin(k, dtype, 'sparse', True)
    tw.set_heldout(*LH.heldout_cells(tw))
    assert len(tw.held[0]) > 4096
    eps = float(np.finfo(dtype).eps)
    worst = 0.0
    truth = np.ascontiguousarray((np.random.RandomState(8).rand(3, tw.n) + 0.1).astype(dtype))
    with _start(tw, d) as s:
        s.run(1).set_heldout(tw.heldout_matrix().pymatrix())
        s.fit_noise()
        s.forecast(3, truth=truth)
        tw.noise, tw.scored_rows = True, 3
        for step, op in enumerate(LH.heldout_life(tw)):
            want = tw.apply(op)
            _same_counts(op, LH.play(s, op), want)
            got, pred = s.eval_heldout_sums(predictions=True)
            W, H, Th = _factors(s)
            with _fresh(tw, d, (W, H, Th)) as f:
                f.set_heldout(tw.heldout_matrix().pymatrix())
                fsums, fpred = f.eval_heldout_sums(predictions=True)
            assert got == fsums and np.array_equal(pred, fpred), (step, op.label)
            hr, hc, _ = tw.held
            assert got['count'] == hr.size == pred.size and hr.size > 4096
            terms = W.astype(np.float64)[hr] * H.astype(np.float64)[hc]
            ratio = np.abs(pred.astype(np.float64) - terms.sum(axis=1)) / (k * eps * np.abs(terms).sum(axis=1))
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (step, op.label, float(ratio.max()))
            assert s.forecast_series_sums()[0] == tw.scored_rows
            if tw.noise:
                assert s.noise()[0].shape == (tw.n,)
            else:
                with pytest.raises(RuntimeError, match='noise'):
                    s.noise()
            s.run(1)                                                          # (the factors move between the steps)
        assert not tw.noise and tw.scored_rows == 0
    evidence('session life held-out set %s k=%d: %d positions left after slide, churn, revise, slide, churn; worst prediction %.3f x the dot-product bound k eps sum|w h|'
             % (np.dtype(dtype).name, k, len(tw.held[0]), worst))


# ---- c. the statistics --------------------------------------------------------------------------------------------------------
def _stats_flags(s, tw, gamma):
    info = s.series_stats_info()
    assert {key: info[key] for key in ('valid', 'stale', 'absorbed_rows')} == tw.stats_info(), (info, tw.stats_info(), tw.labels)
    assert info['forget'] == gamma


@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('gamma', [1.0, 0.95])
def test_statistics_carried_through_a_life_fit_the_final_entries(gamma, dtype, k):
    """init_series_stats, update(adapt), revise(update_stats), slide(downdate_stats) with a block, adapt_series,
    change_series(fit), revise(update_stats) in an added series, update(adapt, window, downdate_stats), no training in between: the
    flags after every step are the twin's, and H at the end is no farther from series_ridge in fp64 -- on the twin's final entries
    and the downloaded W -- than 8x the float32 NumPy twin of the same life is on the design's W (scaled by eps64 / eps32 for fp64;
    tests/test_session_life_host.py prints that value).  8 of 44 and 4 of 40 absorbed rows are retired: fewer than half."""
    from trmf import series_ridge
    d = OH.inputs(k)
    hyper = dict(HYPER, lambdaI=LH.LAM_I)
    yard, _ = LH.stats_yardstick(k, gamma)
    tw = LH.Twin(k, dtype, 'sparse', True)
    with _start(tw, d, hyper) as s:
        for op in LH.stats_life(tw, gamma):
            want = tw.apply(op)
            _same_counts(op, LH.play(s, op), want)
            _stats_flags(s, tw, gamma)
        assert len(tw.labels) == LH.STATS_STEPS and s.rows() == tw.T
        W, H, _ = _factors(s)
    ref = series_ridge(W.astype(np.float64), CH.fit_csc(tw.raw.astype(np.float64)), LH.LAM_I, gamma, True)
    b, err = AH.bound(dtype, yard), relmax(H, ref)
    evidence('session life statistics %s k=%d gamma=%g: relmax of H after the life to the fp64 direct ridge on the final entries %.3e = %.2f x its bound %.3e (fp32 twin %.3e)'
             % (np.dtype(dtype).name, k, gamma, err, err / b, b, yard))
    assert err <= b


@pytest.mark.parametrize('off', [3, 7])
def test_a_life_without_one_update_of_the_statistics_ends_stale(off):
    """The same life with the update_stats of one revise left off: the statistics are stale from there to the end -- no later slide,
    churn, revise or append makes them valid again -- every later step that needs them (slide with downdate_stats, adapt_series,
    revise with update_stats, update with adapt) is refused and leaves the session as it was, and the same step without its use of
    the statistics still works.  (Leaving a downdate_stats off does not make the tables stale, by design: test_gpu_slide.py.)"""
    dtype, k, gamma = np.float32, 7, 0.95
    d = OH.inputs(k)
    tw = LH.Twin(k, dtype, 'sparse', True)
    refused = []
    with _start(tw, d) as s:
        for step, op in enumerate(LH.stats_life(tw, gamma, off=off), 1):
            no, op = LH.stale_steps(tw, op)
            if no is not None:
                before = _factors(s)
                with pytest.raises(RuntimeError, match='series statistics'):
                    LH.play(s, no)
                assert s.rows() == tw.T and s.model.n == tw.n
                for a, b in zip(before, _factors(s)):
                    assert np.array_equal(a, b)
                refused.append(step)
            if op is not None:
                want = tw.apply(op)
                _same_counts(op, LH.play(s, op), want)
            _stats_flags(s, tw, gamma)
            assert tw.stats_info()['stale'] == (step >= off)
        assert refused == {3: [4, 5, 7, 8], 7: [8]}[off] and s.rows() == tw.T == LH.N and s.model.n == tw.n
        with pytest.raises(RuntimeError, match='series statistics'):
            s.adapt_series()
        s.run(1).sync()
    evidence('session life stale statistics, update_stats left off at step %d: stale through every later step, %d calls that need them refused' % (off, len(refused)))


# ---- d. marks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form,storage,missing,transform', [LH.FORMS[0], LH.FORMS[2]], ids=[LH.FORMS[0][0], LH.FORMS[2][0]])
def test_marks_through_a_life(form, storage, missing, transform):
    """A revise keeps the mark -- mark(); revise(); run(1); rewind() restores the marked bits -- also late in a life; after a slide
    that retires rows or a churn the mark is gone and rewind() raises (after an append it names fewer rows than the session holds and
    rewind() refuses as well); a new mark() works every time."""
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    tw = LH.Twin(k, dtype, storage, missing, transform)
    rng = np.random.RandomState(23)
    ops = [lambda: LH.revise_op(tw, rng), lambda: LH.slide_op(tw, 'slide'), lambda: LH.revise_op(tw, rng),
           lambda: LH.churn_op(tw, 'churn-add', [0, tw.n - 1], add=2), lambda: LH.revise_op(tw, rng), lambda: LH.slide_op(tw, 'append'),
           lambda: LH.slide_op(tw, 'retire'), lambda: LH.churn_op(tw, 'churn-retire', [2]), lambda: LH.revise_op(tw, rng)]
    kept = []
    with _start(tw, d) as s:
        s.run(1)
        for make in ops:
            s.mark()
            tw.mark = True
            marked = _factors(s)
            op = make()
            want = tw.apply(op)
            _same_counts(op, LH.play(s, op), want)
            s.run(1)
            kept.append(tw.mark)
            if op.kind == 'revise':
                assert tw.mark and not np.array_equal(_factors(s)[0], marked[0])
                s.rewind()
                for a, b in zip(_factors(s), marked):
                    assert np.array_equal(a, b), op
            else:       # the mark is gone -- or, after an append, names fewer rows than the session holds
                with pytest.raises(RuntimeError, match='rewind: the session has grown' if tw.mark else 'rewind: no mark'):
                    s.rewind()
            s.run(1).sync()
    assert kept == [True, False, True, False, True, True, False, False, True]
    evidence('session life marks %s: rewind restored the marked bits after each of %d revises; it refused after 2 slides that retire, 2 churns and an append'
             % (form, sum(l == 'revise' for l in tw.labels)))


# ---- e. a refused call in mid-life ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form,storage,missing,transform', [LH.FORMS[0], LH.FORMS[2]], ids=[LH.FORMS[0][0], LH.FORMS[2][0]])
def test_refused_calls_in_mid_life_change_nothing(form, storage, missing, transform):
    """After step 6 of all-pairs: a slide below the largest lag + 1 rows, a churn with a mask of the wrong length and a revise
    that names a cell twice are refused; the next probes still equal the twin's and the sequence finishes."""
    assert _life(form, storage, missing, transform, np.float32, 7, LH.all_pairs, refuse_after=6) == 37
    evidence('session life refusals %s: three refused calls after step 6 of all-pairs, the 31 steps behind them still bit for bit a fresh session' % form)


# ---- f. memory ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form,storage,missing,transform', [LH.FORMS[0], LH.FORMS[2]], ids=[LH.FORMS[0][0], LH.FORMS[2][0]])
def test_device_memory_does_not_grow_over_cycles_of_edits(form, storage, missing, transform):
    """100 cycles of slide a block, one series out and one in, a revise with as many inserts as deletes (300 edits): rows and series
    return to what they were after every cycle and the entry count is steered back to its start (session_life_helpers.memory_cycle),
    so the session asks the pool for the same sizes over and over; every edit reserves a new generation of storage and the
    previous one must go back to the pool.

    What is asserted is that the live bytes show no trend.  Two single readings cannot be compared: the figure is the pool's, not
    the session's -- every live buffer carries the unsplit remainder (below DevicePool::kSplitMin) of whichever free block was the
    best fit when it was taken, there are dozens of buffers, and which blocks are free depends on the slab and the order of the
    temporaries -- so equal shapes do not give equal readings (measured on an MI355X: the readings of the 100 cycles wander over 7.5 KB
    with sparse and 9.5 KB with dense storage, cycles 3 and 10 are 256 and 2560 bytes apart).  That wander is bounded whatever
    the number of cycles, a leak is not: the smallest block the pool hands out is POOL_UNIT = 256 bytes, so a buffer lost once per
    cycle by any of the three edits adds at least 256 bytes per cycle (a lost generation of the arrays of Y alone: 7 KB sparse,
    12 KB dense).  Compared are the medians of the readings of cycles 11..20 and 91..100, 80 cycles apart: the later one must
    exceed the earlier one by less than 80 x 256 bytes."""
    dtype, k = np.float32, 7
    d = OH.inputs(k)
    tw = LH.Twin(k, dtype, storage, missing, transform)
    tw.wrap = True                                                            # (300 edits need more rows than the design has)
    rng = np.random.RandomState(29)
    live, count = {}, {}
    entries = tw.raw.nnz if tw.sparse else tw.Y.size
    with _start(tw, d) as s:
        for cycle in range(1, LH.MEMORY_CYCLES + 1):
            for op in LH.memory_cycle(tw, rng, entries):
                want = tw.apply(op)
                _same_counts(op, LH.play(s, op), want)
            assert (s.rows(), s.model.n) == (tw.T, tw.n) == (LH.N, LH.N0)
            s.run(1).sync()
            live[cycle], count[cycle] = s.pool_live_bytes(), tw.raw.nnz if tw.sparse else tw.Y.size
    early, late = (float(np.median([live[c] for c in range(lo, lo + 10)])) for lo in (11, 91))
    evidence('session life memory %s: pool live bytes after cycle 3 %d (%d entries), after cycle 10 %d (%d entries); over %d cycles min %d max %d; '
             'median of cycles 11..20 %d, of cycles 91..100 %d: growth %d bytes, the bound %d'
             % (form, live[3], count[3], live[10], count[10], LH.MEMORY_CYCLES, min(live.values()), max(live.values()), early, late, late - early, 80 * POOL_UNIT))
    assert min(live.values()) > 0 and max(abs(c - entries) for c in count.values()) <= 4
    assert late - early < 80 * POOL_UNIT


# ---- g. two virtual ranks -------------------------------------------------------------------------------------------------------
def test_two_virtual_ranks_live_the_same_life(monkeypatch):
    """all-pairs on one rank in the tile geometry several ranks use (TRMF_TEST=1 TRMF_TILE=narrow) and on TRMF_DEVICES=0,0: the same
    sums, the same objective after an iteration behind every step, the same churn_helpers.after.  (revise and change_series
    re-arm the measured choices of both sharded phases of a group of ranks, slide only the X-side Gram's.)"""
    dtype, k = np.float32, 40
    d = OH.inputs(k)
    names = []

    def once():
        tw = LH.Twin(k, dtype, 'sparse', True)
        trail = []
        with _start(tw, d) as s:
            s.run(1)
            for op in LH.all_pairs(tw):
                want = tw.apply(op)
                got = LH.play(s, op)
                _same_counts(op, got, want)
                s.run(1)
                trail.append((op.label, got, s.objective()))
            names.append(s.describe())
            return trail, CH.after(s, tw.T)

    monkeypatch.setenv('TRMF_TEST', '1')
    monkeypatch.setenv('TRMF_TILE', 'narrow')
    one = once()
    monkeypatch.delenv('TRMF_TILE', raising=False)
    monkeypatch.setenv('TRMF_DEVICES', '0,0')
    two = once()
    assert '2 ranks' in names[-1] and '1 rank' in names[-2]
    for a, b in zip(one[0], two[0]):
        assert a == b, (a, b)
    CH.assert_same(one[1], two[1], 'two virtual ranks')
    evidence('session life two virtual ranks: %d steps of all-pairs, the sums, the objective behind every step and the end are those of one rank' % len(one[0]))
