"""Shared by tests/test_revise_host.py and tests/test_gpu_revise.py: the input sets of the cell-revision tests (test infrastructure).

Built on the designs of online_helpers / adapt_helpers / slide_helpers / churn_helpers: T = 96 rows of 50 series, lags (1, 2, 5),
both orientations in random stored orders, the cells (74, 30) and (5, 12) stored twice, series 3 without an entry.  `revised` is the
statement of the storage contract of trmf_session_revise: both orientations of a session's Y pass through trmf.revise_entries
(every stored copy of an edited cell removed by a stable filter, the sets behind the survivors of their row / column)."""
import functools

import numpy as np

import adapt_helpers as AH
import churn_helpers as CH
import online_helpers as OH
import slide_helpers as SH
from rawsparse_helpers import RawSparse

T, N = OH.T, OH.N
DOUBLED = (AH.TWICE_ROW, AH.TWICE)                   # (74, 30): stored twice
BATCHES = ('replace-only', 'insert-only', 'delete-only', 'mixed')


def raw_all(k, dtype, seed, lo=0, hi=T):
    return SH.raw_rows(k, lo, hi, dtype, seed)


def dense_all(k, dtype, lo=0, hi=T):
    return SH.dense_rows(k, lo, hi, dtype)


@functools.lru_cache(maxsize=None)
def _cells(k, rows=T):
    """(stored cells, unstored cells) of the first `rows` rows of the design, each as sorted (row, col) arrays."""
    r, c, _ = SH.entries(k)
    mask = np.zeros((T, N), dtype=bool)
    mask[r, c] = True
    return np.nonzero(mask[:rows]), np.nonzero(~mask[:rows])


@functools.lru_cache(maxsize=None)
def batch(name, k, rows=T, deletes=True):
    """(rows, cols, vals float32, delete mask) of a designed batch over the first `rows` rows.  `mixed` touches row 0 and the last
    row, series 0 and the last series, both copies of the doubled cell, the series without an entry, and -- as a delete -- one
    cell that is not stored.  deletes=False (dense storage): the same cells, every edit a set."""
    rng = np.random.RandomState(sum(map(ord, name)) + k)
    (sr, sc), (ur, uc) = _cells(k, rows)
    ps, pu = rng.permutation(sr.size), rng.permutation(ur.size)
    stored = lambda m: (sr[ps[:m]], sc[ps[:m]])
    unstored = lambda m: (ur[pu[:m]], uc[pu[:m]])
    if name == 'replace-only':
        er, ec = stored(40); dl = np.zeros(40, dtype=bool)
    elif name == 'insert-only':
        er, ec = unstored(40); dl = np.zeros(40, dtype=bool)
    elif name == 'delete-only':
        a, b = stored(40), unstored(1)
        er, ec = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]); dl = np.ones(41, dtype=bool)
    elif name == 'mixed':
        last = rows - 1
        pick = lambda rr, cc, cond: (int(rr[cond][0]), int(cc[cond][0]))
        gains = pick(ur, uc, uc == AH.NO_ENTRY)
        must = [pick(sr, sc, sr == 0), pick(ur, uc, ur == 0), pick(sr, sc, sr == last), pick(ur, uc, ur == last),
                pick(sr, sc, sc == 0), pick(ur, uc, uc == 0), pick(sr, sc, sc == N - 1), pick(ur, uc, uc == N - 1),
                SH.DOUBLE_GONE, gains] + ([DOUBLED] if DOUBLED[0] < rows else [])
        a, b = stored(30), unstored(30)
        cells = list(dict.fromkeys(must + list(zip(a[0].tolist(), a[1].tolist())) + list(zip(b[0].tolist(), b[1].tolist()))))
        at = {cell: i for i, cell in enumerate(cells)}
        er, ec = np.array([x[0] for x in cells]), np.array([x[1] for x in cells])
        dl = rng.rand(er.size) < 0.35
        is_stored = np.array([bool(np.any((sr == x) & (sc == y))) for x, y in cells])
        dl[np.flatnonzero(~is_stored)[:3]] = True         # cells that are not stored, as deletes (row 0's among them)
        dl[at[SH.DOUBLE_GONE]] = True                     # both copies of a doubled cell are deleted ...
        if DOUBLED[0] < rows:
            dl[at[DOUBLED]] = False                       # ... and those of the other are REPLACED by one entry
        dl[at[gains]] = False                             # the series without an entry gains one
        assert np.any(dl & is_stored) and np.any(~dl & is_stored) and np.any(~dl & ~is_stored) and np.any(dl & ~is_stored)
    else:
        raise KeyError(name)
    if not deletes:
        dl = np.zeros(er.size, dtype=bool)
    ev = (rng.rand(er.size).astype(np.float32) + np.float32(0.25))
    out = (er.astype(np.int64), ec.astype(np.int64), ev, dl)
    for a in out:
        a.setflags(write=False)
    return out


def revised(raw, edits, counts=False):
    """The arrays a session holds after revise(*edits) on a session created over `raw`: each orientation through
    trmf.revise_entries.  counts: also the NumPy statement of the call's sums."""
    from trmf import revise_entries
    Tn, n = raw.shape
    csr, csc = CH.entry_lists(raw)
    ed = (edits[0], edits[1], np.asarray(edits[2]).astype(raw.dtype), edits[3])
    r, c, v, cnt = revise_entries(*csr, ed, major='row', return_counts=True)
    r2, c2, v2, cnt2 = revise_entries(*csc, ed, major='col', return_counts=True)
    assert cnt == cnt2
    rp = np.zeros(Tn + 1, np.uint64); np.cumsum(np.bincount(r, minlength=Tn), out=rp[1:])
    cp = np.zeros(n + 1, np.uint64); np.cumsum(np.bincount(c2, minlength=n), out=cp[1:])
    out = RawSparse.from_arrays((Tn, n), raw.dtype, rp, c.astype(np.uint32), v, cp, r2.astype(np.uint32), v2)
    cnt = dict(cnt, entries=out.nnz, entries_before=raw.nnz, edits=len(edits[0]), first_row=int(np.min(edits[0])) if len(edits[0]) else -1,
               last_row=int(np.max(edits[0])) if len(edits[0]) else -1)
    return (out, cnt) if counts else out


def revised_dense(Y, edits):
    out = np.array(Y, copy=True)
    out[edits[0], edits[1]] = np.asarray(edits[2]).astype(out.dtype)
    return np.ascontiguousarray(out)


def brute_revise(rows, cols, vals, edits, major):
    """revise_entries as a loop over the entries: per major index the entries whose cell is not edited, in stored order, then the
    sets of that index by ascending minor index."""
    er, ec, ev, dl = edits
    cells = set(zip(er.tolist(), ec.tolist()))
    items = [(int(r), int(c), v) for r, c, v in zip(rows, cols, vals) if (int(r), int(c)) not in cells]
    sets = [(int(r), int(c), v) for r, c, v, d in zip(er, ec, ev, dl) if not d]
    key = (lambda e: e[0]) if major == 'row' else (lambda e: e[1])
    minor = (lambda e: e[1]) if major == 'row' else (lambda e: e[0])
    out = []
    for m in sorted(set(key(e) for e in items + sets)):
        out += [e for e in items if key(e) == m] + sorted([e for e in sets if key(e) == m], key=minor)
    return out


# ---- the row shapes of the compaction (churn_helpers.shape_problem) --------------------------------------------------------------
def shape_edits(raw, seed=3):
    """Edits over churn_helpers.shape_problem's matrix (rows of 0, 1, 63, 64, 65, 130, 1, 63, 64, 65, 130 and 140 entries):
    per-row edit lists of 0, 1, 2, 64 and 65 cells; rows that lose their first stored entry, their last, every one and none; an
    insert into the empty row; a repeated cell of the 140-entry row replaced and another deleted."""
    rng = np.random.RandomState(seed)
    Tn, n = raw.shape
    row = lambda i: raw.col_idx[int(raw.row_ptr[i]):int(raw.row_ptr[i + 1])].astype(np.int64)
    absent = lambda i: np.setdiff1d(np.arange(n), row(i))
    er, ec, dl = [], [], []

    def add(i, cols, delete):
        cols = np.atleast_1d(cols)
        er.extend([i] * cols.size); ec.extend(cols.tolist()); dl.extend(np.broadcast_to(delete, cols.shape).tolist())

    add(0, 77, False)                                         # the empty row gains an entry (a list of 1)
    add(1, row(1), True)                                      # its only entry leaves (every one; a list of 1)
    add(2, row(2), rng.rand(63) < 0.5); add(2, absent(2)[:1], False)          # all 63 leave or are replaced, one insert: a list of 64
    add(3, absent(3)[:65], np.arange(65) % 5 == 0)            # 65 cells that are not stored: none leaves, 52 inserts, 13 misses
    add(4, row(4)[0], True); add(4, row(4)[-1], False)        # the first stored entry is deleted, the last replaced
    mid = rng.permutation(row(5)[1:-1])[:64]
    add(5, mid, rng.rand(64) < 0.5)                           # 64 of the 130 from the middle, interleaved with the survivors
    add(7, row(7)[:1], False)                                 # (rows 6, 8, 9, 10: no edit, a plain copy)
    cols, cnt = np.unique(row(11), return_counts=True)
    rep = cols[cnt > 1]
    assert rep.size >= 2
    add(11, rep[0], False); add(11, rep[1], True); add(11, row(11)[-1] if row(11)[-1] not in rep[:2] else cols[cnt == 1][0], True)
    er, ec, dl = np.array(er, dtype=np.int64), np.array(ec, dtype=np.int64), np.array(dl, dtype=bool)
    ev = rng.rand(er.size).astype(np.float32) + np.float32(0.25)
    return er, ec, ev, dl


# ---- the statistics --------------------------------------------------------------------------------------------------------------
def stats_yardstick(W, raw_before, edits, lamI, gamma):
    """(H of the fp64 series_ridge on W's fp32 values over the REVISED entries, relmax of the fp32 twin -- SeriesStats over the
    entries of before the edit in their stored order, then SeriesStats.revise -- against it)."""
    from trmf import SeriesStats, series_ridge
    from helpers import relmax
    W32 = np.asarray(W).astype(np.float32)
    after = revised(raw_before, edits)
    h64 = series_ridge(W32.astype(np.float64), CH.fit_csc(after.astype(np.float64)), lamI, gamma, True)
    ed32 = (edits[0], edits[1], np.asarray(edits[2]).astype(np.float32), edits[3])
    twin = SeriesStats(W32, CH.fit_csc(raw_before.astype(np.float32)), gamma, True).revise(W32, CH.fit_csc(raw_before.astype(np.float32)), ed32)
    return h64, relmax(twin.solve(lamI), h64)
