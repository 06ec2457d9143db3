"""CPU: the host twin of a session's life (tests/session_life_helpers.py) against brute force, the yardstick of the statistics carried
through a life, and the coverage conditions of the sequences tests/test_gpu_session_life.py plays on the device."""
import itertools

import numpy as np
import pytest

import churn_helpers as CH
import online_helpers as OH
import session_life_helpers as LH
from helpers import evidence

DTYPES = [(np.float32, 40), (np.float64, 7)]
DT_IDS = ['float32-k40', 'float64-k7']
STORAGES = ['sparse', 'dense']


def _sequence(name, tw):
    if name.startswith('random-'):
        return LH.random_life(tw, int(name.split('-')[1]))
    return {'all-pairs': LH.all_pairs, 'edges': LH.edges, 'frontend': LH.frontend, 'heldout': LH.heldout_life,
            'stats': lambda t: LH.stats_life(t, 0.95)}[name](tw)


def _played(name, storage, dtype=np.float32, k=7, check=None):
    """The twin after the sequence (every step also through `check`)."""
    tw = LH.Twin(k, dtype, storage, storage == 'sparse')
    for step, op in enumerate(_sequence(name, tw)):
        sums = tw.apply(op)
        if check is not None:
            check(step, op, sums)
    return tw


# ---- 1. the twin against brute force ----------------------------------------------------------------------------------------------
ALL_SEEDS = sorted(s for seeds in LH.SEEDS.values() for s in seeds)
NAMES = ['all-pairs', 'edges', 'frontend', 'heldout', 'stats'] + ['random-%d' % s for s in ALL_SEEDS]


# (update(adapt, downdate_stats) needs per-series statistics: sparse storage only)
LIVES = [(name, storage) for name in NAMES for storage in STORAGES if not (storage == 'dense' and name in ('frontend', 'stats'))]


@pytest.mark.parametrize('name,storage', LIVES, ids=['%s-%s' % c for c in LIVES])
def test_the_twin_equals_a_life_on_plain_lists(name, storage):
    """Every sequence also on per-orientation lists of (row, col, val) tuples advanced by loops (brute_revise, brute_churn, a loop
    restating slide_entries); both orientations are compared after every step.  A sequence that draws a refusal is a bug of the
    generator: the twin asserts that each call is legal."""
    tw = LH.Twin(7, np.float64, storage, storage == 'sparse')
    brute = LH.Brute(tw)
    assert brute.same_as(tw)
    steps = 0
    for op in _sequence(name, tw):
        tw.apply(op)
        brute.apply(op)
        assert brute.same_as(tw), (name, steps, op)
        if tw.sparse:                                            # a consistent pair: from_arrays has compared the two orientations
            assert tw.raw.shape == (tw.T, tw.n)
        steps += 1
    assert steps == {'all-pairs': 37, 'edges': 11, 'frontend': 7, 'heldout': 5, 'stats': LH.STATS_STEPS}.get(name, LH.RANDOM_STEPS)
    assert tw.T >= LH.MIN_ROWS and tw.n >= LH.MIN_SERIES and tw.t0 + tw.T <= OH.T


def test_the_heldout_list_names_the_same_design_cells():
    """In design coordinates a held-out position never moves: after slide -> churn -> revise -> slide -> churn the twin's list is the
    original one without the positions of retired rows and series, in its order, and has several chunks of the compaction."""
    tw = LH.Twin(7, np.float64, 'sparse', True)
    hr, hc, hv = LH.heldout_cells(tw)
    assert hr.size > 4096 and np.all(np.diff(hr) >= 0)
    tw.set_heldout(hr, hc, hv)
    cells = [(int(r), int(c), v) for r, c, v in zip(hr, hc, hv)]          # (t0 = 0, series = 0..37: design coordinates)
    dropped = 0
    for op in LH.heldout_life(tw):
        before = len(tw.held[0])
        sums = tw.apply(op)
        if op.kind == 'churn':
            assert sums['heldout_dropped'] == before - len(tw.held[0]) > 0
            dropped += sums['heldout_dropped']
        want = [e for e in cells if e[0] >= tw.t0 and e[1] in tw.series]
        r, c, v = tw.held
        assert [(tw.t0 + int(a), tw.series[int(b)], x) for a, b, x in zip(r, c, v)] == want
        m = tw.heldout_matrix()
        assert m.nnz == len(want) and np.array_equal(m.col_idx, c) and np.array_equal(m.val_t, v)
    assert len(tw.held[0]) > 4096 and dropped > 0


# ---- 2. the yardstick of the statistics -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,k', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('gamma', [1.0, 0.95])
def test_the_statistics_twin_through_a_life(gamma, dtype, k):
    """The float32 SeriesStats through init, absorb, revise, retire with downdate, absorb, a churn with the cold-start fit, revise
    in an added series and a window tick, solved at lambdaI = 0.5, against series_ridge in fp64 on the twin's final entries.  The
    value is what the device test allows 8x of (adapt_helpers.bound); fewer than half of the absorbed rows are ever retired."""
    yard, tw = LH.stats_yardstick(k, gamma)
    evidence('session life statistics k=%d gamma=%g: the float32 twin through the life is %.3e (relmax) from the fp64 direct ridge on its final entries'
             % (k, gamma, yard))
    assert tw.stats_info() == dict(valid=True, stale=False, absorbed_rows=LH.N) and tw.T == LH.N and tw.n == LH.N0 - 3 + 4
    assert 0 < yard < 1e-4                                       # float32 rounding of a few hundred rank-1 updates, not a wrong table
    assert [t for t in tw.labels] == ['init-stats', 'update', 'revise', 'slide', 'adapt', 'churn-add', 'revise', 'update']
    assert 'in-a-series-the-previous-churn-added' in tw.tags[6]
    # a wrong table is orders of magnitude away: the same life without the downdate
    from helpers import relmax
    from trmf import series_ridge
    bad = LH.Twin(k, np.float32, 'sparse', True, W=OH.inputs(k)['W'])
    for op in LH.stats_life(bad, gamma):
        if op.kind == 'slide':
            op.downdate = False
        bad.apply(op)
    ref = series_ridge(bad.W().astype(np.float64), CH.fit_csc(bad.raw.astype(np.float64)), LH.LAM_I, gamma, True)
    assert relmax(bad.ss.solve(LH.LAM_I), ref) > 100 * yard


@pytest.mark.parametrize('off', [3, 7])
def test_a_life_without_one_update_ends_stale(off):
    """From the revise whose update_stats is left off the statistics are stale; no later slide, churn, revise or append makes them
    valid again, and every step that needs them is one the session must refuse (stale_steps)."""
    tw = LH.Twin(7, np.float32, 'sparse', True, W=OH.inputs(7)['W'])
    refused = []
    for step, op in enumerate(LH.stats_life(tw, 0.95, off=off), 1):
        no, op = LH.stale_steps(tw, op)
        if no is not None:
            refused.append(step)
        if op is not None:
            tw.apply(op)
        info = tw.stats_info()
        assert info['stale'] == (step >= off) and info['valid'] == (step < off)
    assert tw.ss is None and refused == {3: [4, 5, 7, 8], 7: [8]}[off] and len(tw.labels) == {3: 7, 7: 8}[off]
    assert tw.T == LH.N and tw.n == LH.N0 - 3 + 4                     # the structural edits all took place
    with pytest.raises(AssertionError, match='refused'):
        tw.apply(LH.Op('adapt'))


# ---- 3. the coverage conditions of the sequences ----------------------------------------------------------------------------------
def _pairs(labels):
    return set(zip(labels[:-1], labels[1:]))


@pytest.mark.parametrize('storage', STORAGES)
def test_all_pairs_holds_every_ordered_pair(storage):
    tw = _played('all-pairs', storage)
    assert _pairs(tw.labels) == set(itertools.product(LH.LABELS, LH.LABELS))
    churns = [i for i, l in enumerate(tw.labels) if LH.KIND[l] == 'churn']
    after_add = [i for i in churns if i and tw.labels[i - 1] == 'churn-add']
    assert len(after_add) == 2 and all('retires-a-series-the-previous-churn-added' in tw.tags[i] for i in after_add)
    assert not tw.pool                                           # all 12 spare series have joined


@pytest.mark.parametrize('storage', STORAGES)
def test_edges_holds_every_designed_property(storage):
    seen = {}

    def check(step, op, sums):
        seen[step] = (op, sums)

    tw = _played('edges', storage, check=check)
    tags = tw.tags
    want = [(1, 'in-a-row-the-previous-slide-appended'), (1, 'first-row'), (1, 'last-row'), (4, 'in-a-series-the-previous-churn-added'),
            (6, 'retires-revised-row'), (7, 'down-to-the-fewest-rows'), (8, 'append-at-the-fewest-rows')]
    if storage == 'sparse':
        want += [(1, 'replaces-a-doubled-cell-in-a-moved-row'), (2, 'deletes-an-inserted-cell')]
        assert seen[1][1]['copies_removed'] >= seen[1][1]['replaced'] + seen[1][1]['deleted'] + 1         # both copies of the doubled cell
        assert seen[1][1]['inserted'] >= 1 and seen[2][1]['deleted'] >= 1 and seen[4][1]['inserted'] >= 1
    for step, tag in want:
        assert tag in tags[step], (step, tag, tags[step])
    assert tw.labels[:3] == ['slide', 'revise', 'revise'] and tw.labels[7:9] == ['retire', 'append']
    assert seen[7][1]['rows'] == LH.REACH + 1


def test_frontend_retires_revised_rows_in_the_same_tick():
    tw = _played('frontend', 'sparse')
    ticks = [i for i, l in enumerate(tw.labels) if l == 'update']
    assert len(ticks) == 6 and tw.labels[3] == 'churn-add'
    assert all('a-revised-row-is-retired-by-the-same-tick' in tw.tags[i] and 'retires-revised-row' in tw.tags[i] for i in ticks)
    assert tw.stats_info() == dict(valid=True, stale=False, absorbed_rows=LH.N) and tw.T == LH.N


def test_the_random_seeds_cover_every_pair_and_every_kind():
    """Over the seeds the device test uses every one of the 36 ordered pairs of ops occurs; every seed holds each of the three kinds
    of edit at least twice (whatever the storage: the draws do not depend on it)."""
    pairs = set()
    for form, storage, missing, transform in LH.FORMS:
        for seed in LH.SEEDS[form]:
            tw = LH.Twin(7, np.float32, storage, missing, transform)
            for op in LH.random_life(tw, seed):
                tw.apply(op)
            assert len(tw.labels) == LH.RANDOM_STEPS
            kinds = [LH.KIND[l] for l in tw.labels]
            assert all(kinds.count(kind) >= 2 for kind in ('slide', 'churn', 'revise')), (form, seed, tw.labels)
            pairs |= _pairs(tw.labels)
    assert pairs == set(itertools.product(LH.LABELS, LH.LABELS)), set(itertools.product(LH.LABELS, LH.LABELS)) - pairs
    assert len(set(s for seeds in LH.SEEDS.values() for s in seeds)) == 16


@pytest.mark.parametrize('storage', STORAGES)
def test_the_memory_cycle_returns_to_the_same_shape(storage):
    """The 100 cycles of the device test: rows and series after every cycle are those of the start, every revise inserts as many
    cells as it deletes, and the entry count of sparse storage is steered back to its start -- it is off by at most 4 entries
    (64 bytes of arrays) and in fewer than one cycle in ten.  The first ten cycles also against brute force."""
    tw = LH.Twin(7, np.float32, storage, storage == 'sparse')
    tw.wrap = True
    brute = LH.Brute(tw)
    rng = np.random.RandomState(29)
    entries = tw.raw.nnz if tw.sparse else tw.Y.size
    off = []
    for cycle in range(LH.MEMORY_CYCLES):
        for op in LH.memory_cycle(tw, rng, entries):
            sums = tw.apply(op)
            if cycle < 10:
                brute.apply(op)
            if op.kind == 'revise' and tw.sparse:
                assert sums['inserted'] == sums['deleted'] == 10 and sums['replaced'] == sums['missed'] == 0
        assert cycle >= 10 or brute.same_as(tw)
        assert (tw.T, tw.n) == (LH.N, LH.N0)
        off.append(abs((tw.raw.nnz if tw.sparse else tw.Y.size) - entries))
    assert max(off) <= 4 and sum(x != 0 for x in off) < LH.MEMORY_CYCLES // 10
