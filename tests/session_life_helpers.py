"""Shared by tests/test_session_life_host.py and tests/test_gpu_session_life.py: a host twin of a resident session through a whole
life of interleaved edits, and the edit sequences both files play (test infrastructure).

A session lives long: it slides, gains and loses series and has cells revised, in any order, and every edit leaves state the next one
reads.  `Twin` holds what a session should hold after each call -- the stored entries of both orientations (slide_helpers.slid,
churn_helpers.churned, revise_helpers.revised: the NumPy statements of the three storage contracts), a dense matrix and its transform
coefficients, the held-out list in set order, the flags (mark, series statistics) and, when it is given the W the rows are absorbed
with, a float32 trmf.SeriesStats carried through absorb / retire / revise and gathered by a churn.  One method per Session call, the
same arguments.  `History` notes, beside the twin, which of the designed properties each op had.

The data are the designs of the sibling helpers: T = 96 rows of 50 series at rank k (slide_helpers.entries), of which a session starts
on the window of the first N = 40 rows and the 38 first series; rows 40..95 arrive in blocks of 4, series 38..49 are there to be added.
Twin.t0 and Twin.series say which rows and series of the design the window holds, so every op can be stated in design coordinates
too (the brute-force check of the host test does)."""
import copy
import functools

import numpy as np

import churn_helpers as CH
import online_helpers as OH
import revise_helpers as RH
import slide_helpers as SH

N = 40                                   # rows of the window a life starts on
N0 = CH.N0                               # 38 resident series; 38..49 can be added
STEP = 4                                 # rows of a block
REACH = max(OH.LAGS)
BATCH = 30                               # cells of a revise
SEED = 41
MIN_ROWS = REACH + 11                    # churn_helpers.after: the filter from row T - 6, the smoother from row T - 10 >= REACH ... + 1
MIN_SERIES = 8
LAM_I = 0.5
FORMS = [('sparse-missing', 'sparse', True, False), ('sparse-full', 'sparse', False, False), ('dense', 'dense', False, False),
         ('dense-transform', 'dense', False, True)]
LABELS = ('slide', 'retire', 'append', 'churn-add', 'churn-retire', 'revise')        # the six ops of the all-pairs order
KIND = {'slide': 'slide', 'retire': 'slide', 'append': 'slide', 'churn-add': 'churn', 'churn-retire': 'churn', 'revise': 'revise',
        'update': 'update', 'init-stats': 'stats', 'adapt': 'stats'}


class Op(object):
    """One call: `label` (one of LABELS, or 'update' / 'init-stats' / 'adapt'), its kind and the arguments of the Session method."""

    def __init__(self, label, **args):
        self.label, self.kind = label, KIND[label]
        self.__dict__.update(args)

    def __repr__(self):
        return 'Op({})'.format(self.label)


def _csc32(raw):
    return CH.fit_csc(raw.astype(np.float32))


class History(object):
    """Which of the designed properties each op of a life had -- what the host test's coverage conditions read.  Kept apart from
    the twin: note(tw, op) looks at the twin BEFORE the op is applied and remembers, in design coordinates, which cells revises
    have set or inserted and what the previous op appended or added."""

    def __init__(self):
        self.inserted, self.revised_cells = set(), set()
        self.last_appended, self.last_added = 0, 0         # rows / series the PREVIOUS op appended / added
        self.labels, self.tags = [], []

    def note(self, tw, op):
        tags = set()
        if op.kind == 'update':
            window = getattr(op, 'window', None)
            retire = max(0, tw.T + op.block.shape[0] - window) if window is not None else 0
            if op.revisions is not None:
                if retire and int(np.min(op.revisions[0])) < retire:
                    tags.add('a-revised-row-is-retired-by-the-same-tick')
                self._revise(tw, np.asarray(op.revisions[0]), np.asarray(op.revisions[1]), None, tags)
            self._slide(tw, retire, op.block.shape[0], tags)
        elif op.kind == 'slide':
            self._slide(tw, int(op.retire), 0 if op.block is None else op.block.shape[0], tags)
        elif op.kind == 'churn':
            keep = np.ones(tw.n, dtype=bool) if op.keep is None else np.asarray(op.keep, dtype=bool)
            if self.last_added and not keep[tw.n - self.last_added:].all():
                tags.add('retires-a-series-the-previous-churn-added')
            self.last_appended, self.last_added = 0, len(getattr(op, 'ids', ()))
        elif op.kind == 'revise':
            self._revise(tw, np.asarray(op.rows), np.asarray(op.cols), op.delete, tags)
        self.labels.append(op.label)
        self.tags.append(tags)

    def _slide(self, tw, retire, Tn, tags):
        if retire and any(tw.t0 <= r < tw.t0 + retire for r, _ in self.revised_cells):
            tags.add('retires-revised-row')
        if Tn and tw.T == REACH + 1 and retire == 0:
            tags.add('append-at-the-fewest-rows')
        if retire and tw.T - retire + Tn == REACH + 1:
            tags.add('down-to-the-fewest-rows')
        self.last_appended, self.last_added = Tn, 0

    def _revise(self, tw, er, ec, delete, tags):
        dl = np.zeros(er.shape, dtype=bool) if delete is None else np.asarray(delete, dtype=bool)
        M = tw.stored_mask()
        cells = [(tw.t0 + int(r), tw.series[int(c)]) for r, c in zip(er, ec)]
        if any(d and M[r, c] and g in self.inserted for r, c, d, g in zip(er, ec, dl, cells)):
            tags.add('deletes-an-inserted-cell')
        if tw.sparse and tw.t0 > 0:
            copies = np.zeros((tw.T, tw.n), dtype=np.int64)
            np.add.at(copies, (tw.raw.rows, tw.raw.cols), 1)
            if np.any((copies[er, ec] >= 2) & ~dl):
                tags.add('replaces-a-doubled-cell-in-a-moved-row')
        if self.last_appended and er.max() >= tw.T - self.last_appended:
            tags.add('in-a-row-the-previous-slide-appended')
        if self.last_added and ec.max() >= tw.n - self.last_added:
            tags.add('in-a-series-the-previous-churn-added')
        if er.min() == 0:
            tags.add('first-row')
        if er.max() == tw.T - 1:
            tags.add('last-row')
        for r, c, d, g in zip(er, ec, dl, cells):
            if not d:
                self.revised_cells.add(g)
                if not M[r, c]:
                    self.inserted.add(g)
            else:
                self.inserted.discard(g); self.revised_cells.discard(g)
        self.last_appended, self.last_added = 0, 0


class Twin(object):
    """What a session created on rows 0..N-1 of the N0 first series should hold.  W: the 96 design rows of W (float32) the statistics
    absorb with -- given, the twin carries a float32 SeriesStats; without, only the flags."""

    def __init__(self, k, dtype, storage='sparse', missing=True, transform=False, W=None):
        self.k, self.dtype = k, np.dtype(dtype)
        self.sparse, self.missing = storage == 'sparse', bool(missing)
        self.per_series = self.sparse and self.missing
        self.t0, self.T, self.series = 0, N, list(range(N0))
        self.wrap = False
        self.pool = list(range(N0, OH.N))
        self.raw = self.Y = self.tr = None
        if self.sparse:
            self.raw = CH.raw_part(k, 0, N, self.series, dtype, SEED)
        else:
            self.design = SH.dense_rows(k, 0, OH.T, dtype)
            self.Y = np.ascontiguousarray(self.design[:N, :N0])
            if transform:
                from trmf.model import NormalizedTransform
                self.tr = NormalizedTransform(self.Y)
        self.held = None                                   # (rows, cols, vals) in set order
        self.mark = False
        self.stats = None                                  # dict(valid, stale, absorbed_rows, forget)
        self.Wd = None if W is None else np.asarray(W, dtype=np.float32)
        self.ss = None
        self.noise = False
        self.scored_rows = 0
        self.history = History()                           # which designed properties each op had (the coverage conditions)

    # ---- what the window holds ------------------------------------------------------------------------------------------------
    @property
    def n(self):
        return len(self.series)

    labels = property(lambda self: self.history.labels)
    tags = property(lambda self: self.history.tags)
    last_added = property(lambda self: self.history.last_added)

    def W(self):
        return self.Wd[self.t0:self.t0 + self.T]

    def stored_mask(self):
        M = np.ones((self.T, self.n), dtype=bool)
        if self.sparse:
            M[:] = False
            M[self.raw.rows, self.raw.cols] = True
        return M

    def session_Y(self):
        """What Session takes."""
        return self.raw.pymatrix() if self.sparse else self.Y

    def rows_block(self, count=STEP):
        """The next `count` rows of the design over the series held (wrap: the design's rows N.. over and over, for a life
        longer than the design)."""
        lo = self.t0 + self.T
        if self.wrap:
            lo = N + (lo - N) % (OH.T - N)
        assert lo + count <= OH.T, 'the design has no rows left'
        if self.sparse:
            return CH.raw_part(self.k, lo, lo + count, self.series, self.dtype, SEED)
        return np.ascontiguousarray(self.design[lo:lo + count][:, self.series])

    def series_block(self, ids):
        """The design's series `ids` over the rows held (wrap: over as many rows of the design, from a start that stays inside it)."""
        lo = self.t0 % (OH.T - self.T + 1) if self.wrap else self.t0
        if self.sparse:
            return CH.raw_part(self.k, lo, lo + self.T, list(ids), self.dtype, SEED)
        return np.ascontiguousarray(self.design[lo:lo + self.T][:, list(ids)])

    def transform_of(self, block):
        if self.tr is None or block is None:
            return None
        from trmf.model import NormalizedTransform
        return NormalizedTransform(block)

    def heldout_matrix(self):
        """The held-out list as a matrix whose CSR arrays are the list in its order (what a fresh set_heldout takes)."""
        from rawsparse_helpers import RawSparse
        hr, hc, hv = self.held
        assert np.all(np.diff(hr) >= 0)
        rp = np.zeros(self.T + 1, np.uint64); np.cumsum(np.bincount(hr, minlength=self.T), out=rp[1:])
        o = np.argsort(hc, kind='stable')
        cp = np.zeros(self.n + 1, np.uint64); np.cumsum(np.bincount(hc, minlength=self.n), out=cp[1:])
        return RawSparse.from_arrays((self.T, self.n), self.dtype, rp, hc.astype(np.uint32), hv, cp, hr[o].astype(np.uint32), hv[o])

    def stats_info(self):
        if self.stats is None:
            return dict(valid=False, stale=False, absorbed_rows=0)
        return dict(valid=self.stats['valid'], stale=not self.stats['valid'], absorbed_rows=self.stats['absorbed_rows'])

    # ---- the calls --------------------------------------------------------------------------------------------------------------
    def apply(self, op):
        """Advance by one op; returns the sums the Session call should return (the keys that are counts)."""
        self.history.note(self, op)                        # (reads the state of before the op)
        return getattr(self, '_' + op.kind)(op)

    def set_heldout(self, rows, cols, vals):
        self.held = (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals).astype(self.dtype))

    def _stale(self):
        if self.stats is not None:
            self.stats['valid'] = False
        self.ss = None

    def _stats(self, op):
        if op.label == 'init-stats':
            self.stats = dict(valid=True, absorbed_rows=self.T, forget=op.forget)
            if self.Wd is not None:
                from trmf import SeriesStats
                self.ss = SeriesStats(self.W(), _csc32(self.raw), op.forget, True) if self.per_series else None
            return {}
        assert self.stats is not None and self.stats['valid'], 'adapt_series on statistics that are not valid: the call is refused'
        first = self.stats['absorbed_rows']
        if self.ss is not None:
            self.ss.absorb(self.W(), _csc32(SH.slid(self.raw, first)))
        self.stats['absorbed_rows'] = self.T
        return dict(series=self.n, rows=self.T - first)

    def _slide(self, op):
        block, retire, down = op.block, int(op.retire), bool(getattr(op, 'downdate', False))
        Tn = 0 if block is None else block.shape[0]
        assert 0 <= retire <= self.T and self.T - retire + Tn >= REACH + 1, 'a slide the session refuses'
        if self.stats is not None:
            ad = self.stats['absorbed_rows']
            if retire:
                if retire > ad:
                    self._stale()
                elif self.ss is not None:
                    assert not down or self.stats['valid']
                    self.ss.retire(self.W(), _csc32(self.raw), retire, downdate=down)
                self.stats['absorbed_rows'] = max(0, ad - retire)
        if self.sparse:
            gone = int(np.count_nonzero(self.raw.rows < retire))
            self.raw = SH.slid(self.raw, retire, block)
            out = dict(rows_retired=retire, entries_retired=gone, rows_appended=Tn, entries_appended=0 if block is None else block.nnz,
                       rows=self.T - retire + Tn, entries=self.raw.nnz)
        else:
            self.Y = np.ascontiguousarray(np.vstack([self.Y[retire:]] + ([block] if block is not None else [])))
            out = dict(rows_retired=retire, entries_retired=retire * self.n, rows_appended=Tn, entries_appended=Tn * self.n,
                       rows=self.T - retire + Tn, entries=self.Y.size)
        if retire and self.held is not None:
            hr, hc, hv = self.held
            stay = hr >= retire                                      # a stable filter, the rest moves up
            self.held = (hr[stay] - retire, hc[stay], hv[stay])
        if retire:
            self.mark = False
        self.t0 += retire
        self.T = self.T - retire + Tn
        return out

    def _churn(self, op):
        keep, block, fit = op.keep, op.block, bool(getattr(op, 'fit', True))
        n0 = self.n
        keep = np.ones(n0, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
        assert keep.shape == (n0,)
        ids = list(getattr(op, 'ids', ()))
        m = len(ids)
        assert (block is None) == (m == 0) and (m == 0 or block.shape == (self.T, m))
        nk = int(keep.sum())
        assert nk + m > 0 and not (nk == n0 and m == 0), 'a churn the session refuses or ignores'
        carry = self.stats is not None and self.stats['valid'] and self.stats['absorbed_rows'] == self.T and self.per_series and (m == 0 or fit)
        if self.stats is not None:
            if not carry:
                self._stale()
            elif self.ss is not None:
                self.ss.S, self.ss.r = self.ss.S[keep], self.ss.r[keep]
                if m:
                    from trmf import SeriesStats
                    new = SeriesStats(self.W(), _csc32(block), self.stats['forget'], True)
                    self.ss.S, self.ss.r = np.concatenate([self.ss.S, new.S]), np.concatenate([self.ss.r, new.r])
                self.ss.n = nk + m
        if self.sparse:
            gone = int(np.count_nonzero(~keep[self.raw.cols]))
            self.raw = CH.churned(self.raw, keep, block)
            out = dict(entries_retired=gone, entries_added=0 if block is None else block.nnz, entries=self.raw.nnz)
        else:
            self.Y = np.ascontiguousarray(np.hstack([self.Y[:, keep]] + ([block] if block is not None else [])))
            out = dict(entries_retired=self.T * (n0 - nk), entries_added=self.T * m, entries=self.Y.size)
            if self.tr is not None:
                tn = op.transform_new
                tr = copy.copy(self.tr)
                tr.a = np.concatenate([self.tr.a[:, keep]] + ([np.asarray(tn.a).reshape(1, -1)] if m else []), axis=1)
                tr.b = np.concatenate([self.tr.b[:, keep]] + ([np.asarray(tn.b).reshape(1, -1)] if m else []), axis=1)
                self.tr = tr
        dropped = 0
        if self.held is not None and nk < n0:
            hr, hc, hv = self.held
            stay = keep[hc]                                          # a stable filter, the kept series renumbered densely
            dropped = int(np.count_nonzero(~stay))
            self.held = (hr[stay], (np.cumsum(keep) - 1)[hc[stay]], hv[stay])
        out.update(series_before=n0, series_retired=n0 - nk, series_added=m, series=nk + m, heldout_dropped=dropped, fitted=bool(m and fit),
                   stats_carried=bool(carry))
        self.series = [s for s, kp in zip(self.series, keep) if kp] + ids
        self.pool = [s for s in self.pool if s not in ids]
        self.mark = False
        self.noise, self.scored_rows = False, 0
        return out

    def _revise(self, op):
        er, ec = np.asarray(op.rows, dtype=np.int64), np.asarray(op.cols, dtype=np.int64)
        ev = np.asarray(op.vals).astype(self.dtype)
        dl = np.zeros(er.shape, dtype=bool) if op.delete is None else np.asarray(op.delete, dtype=bool)
        update = bool(getattr(op, 'update_stats', False))
        assert er.size and er.min() >= 0 and er.max() < self.T and ec.min() >= 0 and ec.max() < self.n
        assert len(set(zip(er.tolist(), ec.tolist()))) == er.size, 'a cell is named twice'
        assert self.sparse or not dl.any(), 'a delete on dense storage'
        edits = (er, ec, ev, dl)
        if self.sparse:
            before = self.raw
            self.raw, out = RH.revised(before, edits, counts=True)
            changed = bool((~dl).any() or out['copies_removed'])
        else:
            self.Y = RH.revised_dense(self.Y, edits)
            E = int(er.size)
            out = dict(edits=E, inserted=0, replaced=E, deleted=0, missed=0, copies_removed=E, entries_before=self.Y.size, entries=self.Y.size,
                       first_row=int(er.min()), last_row=int(er.max()))
            changed = True
        carry = update and self.stats is not None and self.stats['valid'] and self.stats['absorbed_rows'] == self.T and self.per_series
        if self.stats is not None and changed:
            if not carry:
                self._stale()
            elif self.ss is not None:
                self.ss.revise(self.W(), _csc32(before), (er, ec, ev.astype(np.float32), dl))
        out['stats_carried'] = bool(carry)
        return out

    def _update(self, op):
        """Session.update(block, window=, revisions=, adapt=, downdate_stats=): init if there are no statistics, revise, slide,
        (the filter,) adapt_series."""
        adapt = bool(getattr(op, 'adapt', False))
        window = getattr(op, 'window', None)
        out = {}
        if adapt:
            assert self.stats is None or self.stats['valid'], 'update(adapt=True) on stale statistics: the call is refused'
            if self.stats is None:
                self._stats(Op('init-stats', forget=getattr(op, 'forget', 1.0)))
        retire = max(0, self.T + op.block.shape[0] - window) if window is not None else 0
        if op.revisions is not None:
            rv = op.revisions
            out['revise'] = self._revise(Op('revise', rows=rv[0], cols=rv[1], vals=rv[2], delete=None, update_stats=adapt and self.per_series))
        out['slide'] = self._slide(Op('slide', block=op.block, retire=retire, downdate=bool(getattr(op, 'downdate', False))))
        if adapt:
            out['adapt'] = self._stats(Op('adapt'))
        return out


# ---- playing an op on a session --------------------------------------------------------------------------------------------------
def _arg(block):
    return block.pymatrix() if hasattr(block, 'pymatrix') else block


def play(s, op):
    """The Session call of `op`; returns what it returns."""
    if op.kind == 'slide':
        return s.slide(_arg(op.block), op.retire, bool(getattr(op, 'downdate', False)))
    if op.kind == 'churn':
        return s.change_series(op.keep, _arg(op.block), fit=bool(getattr(op, 'fit', True)), transform_new=getattr(op, 'transform_new', None))
    if op.kind == 'revise':
        return s.revise(op.rows, op.cols, op.vals, op.delete, update_stats=bool(getattr(op, 'update_stats', False)))
    if op.kind == 'update':
        return s.update(_arg(op.block), window=getattr(op, 'window', None), revisions=op.revisions, adapt=bool(getattr(op, 'adapt', False)),
                        forget=getattr(op, 'forget', 1.0), downdate_stats=bool(getattr(op, 'downdate', False)))
    if op.label == 'init-stats':
        return s.init_series_stats(op.forget)
    return s.adapt_series()


def counts_of(got, want):
    """The counts of `want` as the call returned them (update: per part)."""
    return {key: got[key] for key in want}


# ---- building ops from the twin's state ------------------------------------------------------------------------------------------
def slide_op(tw, label, retire=STEP, downdate=False):
    block = tw.rows_block() if label in ('slide', 'append') else None
    return Op(label, block=block, retire=0 if label == 'append' else int(retire), downdate=downdate)


def churn_op(tw, label, retired, add=0, fit=True):
    """Retire the series at the positions `retired`, add the `add` next series of the pool."""
    keep = np.ones(tw.n, dtype=bool)
    keep[list(retired)] = False
    ids = tw.pool[:add]
    block = tw.series_block(ids) if ids else None
    return Op(label, keep=keep if len(retired) else None, block=block, ids=ids, fit=fit, transform_new=tw.transform_of(block))


def revise_op(tw, rng, must=(), count=BATCH, update_stats=False, sets_only=False):
    """About `count` cells: `must` -- (row, col, delete) triples -- first, then replaces, deletes, inserts and deletes of cells that
    are not stored (in the proportions 12 : 8 : 8 : 2) drawn from the window.  Dense storage, or sets_only: every edit a set."""
    M = tw.stored_mask()
    sets_only = sets_only or not tw.sparse
    cells = {(int(r), int(c)): bool(d) and not sets_only for r, c, d in must}
    (sr, sc), (ur, uc) = np.nonzero(M), np.nonzero(~M)
    ps, pu = rng.permutation(sr.size), rng.permutation(ur.size)
    room = max(count - len(cells), 0)
    if tw.sparse:
        parts = [(sr[ps], sc[ps], False, (room * 12) // 30), (sr[ps[::-1]], sc[ps[::-1]], True, (room * 8) // 30),
                 (ur[pu], uc[pu], False, (room * 8) // 30), (ur[pu[::-1]], uc[pu[::-1]], True, room - (room * 28) // 30)]
    else:
        parts = [(sr[ps], sc[ps], False, room)]
    for rr, cc, dele, want in parts:
        took = 0
        for r, c in zip(rr.tolist(), cc.tolist()):
            if took == want:
                break
            if (r, c) not in cells:
                cells[(r, c)] = dele and not sets_only
                took += 1
    er = np.array([x[0] for x in cells], dtype=np.int64); ec = np.array([x[1] for x in cells], dtype=np.int64)
    dl = np.array(list(cells.values()), dtype=bool)
    ev = (rng.rand(er.size).astype(np.float32) + np.float32(0.25)).astype(tw.dtype)
    return Op('revise', rows=er, cols=ec, vals=ev, delete=dl if tw.sparse and not sets_only else None, update_stats=update_stats)


def _pick(mask, cond=None):
    """The first cell of a boolean matrix (under a condition on (rows, cols)) as (row, col)."""
    r, c = np.nonzero(mask)
    if cond is not None:
        ok = cond(r, c)
        r, c = r[ok], c[ok]
    assert r.size, 'the design holds no such cell'
    return int(r[0]), int(c[0])


# ---- the designed sequences ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_pairs_order():
    """37 labels in which every ordered pair of LABELS is adjacent exactly once: an Euler circuit of the complete digraph with
    loops on six nodes (Hierholzer, the out-edges taken in a fixed order)."""
    left = {a: list(range(len(LABELS))) for a in range(len(LABELS))}
    for a in left:                                               # the loop last: a circuit that does not stall on its first node
        left[a].remove(a); left[a].append(a)
    stack, path = [0], []
    while stack:
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop(0))
        else:
            path.append(stack.pop())
    order = tuple(LABELS[v] for v in reversed(path))
    assert len(order) == 37 and len(set(zip(order[:-1], order[1:]))) == 36
    return order


def all_pairs(tw):
    """The all-pairs order on `tw` (a generator: the caller applies each op to the twin before it asks for the next).  A churn that
    follows a churn-add retires a series that one added."""
    rng = np.random.RandomState(7)
    order = all_pairs_order()
    adds = order.count('churn-add')
    for label in order:
        if KIND[label] == 'slide':
            yield slide_op(tw, label)
        elif KIND[label] == 'churn':
            retired = {tw.n - 1} if tw.last_added else {0}
            retired.add(int(rng.randint(1, tw.n - 1)))
            add = 0
            if label == 'churn-add':
                add = 2 if len(tw.pool) - 2 >= adds - 1 else 1
                adds -= 1
            yield churn_op(tw, label, sorted(retired), add)
        else:
            yield revise_op(tw, rng)


def edges(tw):
    """The designed edge cases, in an order in which each finds the state it needs."""
    rng = np.random.RandomState(11)
    yield slide_op(tw, 'slide', retire=3)                                     # design row 5 (a cell stored twice) is now row 2
    M = tw.stored_mask()
    if tw.sparse:
        copies = np.zeros(M.shape, dtype=np.int64); np.add.at(copies, (tw.raw.rows, tw.raw.cols), 1)
        twice = _pick(copies >= 2)
    else:
        twice = (SH.DOUBLE_GONE[0] - 3, SH.DOUBLE_GONE[1])
    late = _pick(~M if tw.sparse else M, lambda r, c: (r >= 10) & (r < tw.T - STEP))      # an insert (sparse) that a later revise deletes
    cell_x = (tw.t0 + late[0], tw.series[late[1]])
    yield revise_op(tw, rng, must=[twice + (False,), late + (False,), _pick(M, lambda r, c: r >= tw.T - STEP) + (False,),
                                   _pick(M, lambda r, c: r == 0) + (False,), _pick(M, lambda r, c: r == tw.T - 1) + (True,)])
    yield revise_op(tw, rng, must=[(cell_x[0] - tw.t0, tw.series.index(cell_x[1]), True)])
    yield churn_op(tw, 'churn-add', [1], add=2)
    M = tw.stored_mask()
    new = lambda r, c: c >= tw.n - 2
    yield revise_op(tw, rng, must=[_pick(M, new) + (False,), _pick(M, lambda r, c: new(r, c) & (r > 20)) + (True,)] +
                    ([_pick(~M, new) + (False,)] if tw.sparse else []))
    M = tw.stored_mask()
    yield revise_op(tw, rng, must=[_pick(M, lambda r, c: r == 1) + (False,)] + ([_pick(~M, lambda r, c: r == 2) + (False,)] if tw.sparse else []))
    yield slide_op(tw, 'slide', retire=STEP)                                  # ... and those rows are retired
    yield slide_op(tw, 'retire', retire=tw.T - (REACH + 1))                   # the fewest rows a session may keep
    for _ in range(3):
        yield slide_op(tw, 'append')


def frontend(tw, gamma=0.95):
    """Six ticks of update(block, window=N, revisions=, adapt=True, downdate_stats=True), a churn with the cold-start fit after the
    third.  Every tick revises cells of rows 0..3, which the same tick retires, and of later rows."""
    rng = np.random.RandomState(13)
    for tick in range(6):
        M = tw.stored_mask()
        rv = revise_op(tw, rng, must=[_pick(M, lambda r, c: r == 0) + (False,), _pick(~M, lambda r, c: r == STEP - 1) + (False,),
                                      _pick(M, lambda r, c: r == tw.T - 1) + (False,)], count=12, sets_only=True)
        yield Op('update', block=tw.rows_block(), window=N, revisions=(rv.rows, rv.cols, rv.vals), adapt=True, forget=gamma, downdate=True)
        if tick == 2:
            yield churn_op(tw, 'churn-add', [0, tw.n - 1], add=3, fit=True)


def heldout_life(tw):
    """slide -> churn -> revise -> slide -> churn under a held-out set."""
    rng = np.random.RandomState(17)
    yield slide_op(tw, 'slide', retire=2 * STEP)
    yield churn_op(tw, 'churn-add', [0, 7, 8, 20, tw.n - 1], add=2)
    yield revise_op(tw, rng)
    yield slide_op(tw, 'slide', retire=STEP)
    yield churn_op(tw, 'churn-add', [3, tw.n - 1], add=1)


def heldout_cells(tw, copies=6, seed=8):
    """Every cell of the window `copies` times, grouped by row in a random order inside the row: (rows, cols, vals)."""
    rng = np.random.RandomState(seed)
    rr, cc = np.divmod(np.tile(np.arange(tw.T * tw.n), copies), tw.n)
    o = np.lexsort((rng.rand(rr.size), rr))
    return rr[o], cc[o], (rng.rand(rr.size) + 0.5).astype(tw.dtype)


STATS_STEPS = 8


def stats_life(tw, gamma, off=None):
    """init_series_stats; update(adapt); revise(update_stats); slide(downdate_stats) with a block; adapt_series; change_series(fit);
    revise(update_stats) in an added series; update(adapt, window, downdate_stats).  8 of 44 and 4 of 40 absorbed rows are retired:
    fewer than half (slide_helpers.STATS_RETIRE).  off: the (1-based) step -- a revise -- whose update_stats is left off: the
    statistics are stale from there on, and the later steps go through stale_steps.  (There is no variant with a downdate_stats
    left off: the library keeps such tables valid by design, as forgotten history -- slide_helpers / test_gpu_slide.py.)"""
    rng = np.random.RandomState(19)
    yield Op('init-stats', forget=gamma)
    yield Op('update', block=tw.rows_block(), window=None, revisions=None, adapt=True, forget=gamma)
    yield revise_op(tw, rng, update_stats=off != 3)
    yield slide_op(tw, 'slide', retire=2 * STEP, downdate=True)
    yield Op('adapt')
    yield churn_op(tw, 'churn-add', [0, 14, tw.n - 1], add=4, fit=True)
    M = tw.stored_mask()
    new = lambda r, c: c >= tw.n - 4
    yield revise_op(tw, rng, must=[_pick(M, new) + (False,), _pick(~M, new) + (False,), _pick(M, lambda r, c: new(r, c) & (r > 9)) + (True,)],
                    update_stats=off != 7)
    yield Op('update', block=tw.rows_block(), window=N, revisions=None, adapt=True, forget=gamma, downdate=True)


def stale_steps(tw, op):
    """An op of a life whose statistics have gone stale: (the op as it is if the session must refuse it, else None; the op without
    its use of the statistics, which the session takes -- None for adapt_series, which is nothing else)."""
    if tw.stats is None or tw.stats['valid']:
        return None, op
    if op.label == 'adapt':
        return op, None
    plain = copy.copy(op)
    if op.kind == 'slide' and getattr(op, 'downdate', False):
        plain.downdate = False
    elif op.kind == 'revise' and getattr(op, 'update_stats', False):
        plain.update_stats = False
    elif op.kind == 'update' and (getattr(op, 'adapt', False) or getattr(op, 'downdate', False)):
        plain.adapt, plain.downdate = False, False
    else:
        return None, op
    return op, plain


@functools.lru_cache(maxsize=None)
def stats_yardstick(k, gamma):
    """The float32 twin through stats_life on the design's W, solved at LAM_I, against series_ridge in fp64 on the twin's final
    entries: (relmax, the twin).  What another rounding of the same recursion costs on this life -- no device value enters."""
    from helpers import relmax
    from trmf import series_ridge
    tw = Twin(k, np.float32, 'sparse', True, W=OH.inputs(k)['W'])
    for op in stats_life(tw, gamma):
        tw.apply(op)
    ref = series_ridge(tw.W().astype(np.float64), CH.fit_csc(tw.raw.astype(np.float64)), LAM_I, gamma, True)
    return relmax(tw.ss.solve(LAM_I), ref), tw


MEMORY_CYCLES = 100


def memory_cycle(tw, rng, entries=None):
    """A cycle after which rows and series are what they were, and (sparse storage) the entry count is steered back to `entries`:
    slide a block, one series out and one in -- the pair that brings the count closest to `entries`, exactly whenever a series holds
    as many entries as are over -- and a revise with as many inserts as deletes.  tw.wrap lets it go on past the design's rows."""
    yield slide_op(tw, 'slide', retire=STEP)
    if tw.sparse:
        per_series = np.bincount(tw.raw.cols, minlength=tw.n)
        spare = [s for s in range(OH.N) if s not in tw.series]                   # (a series that has left may come back)
        over = {s: tw.raw.nnz + tw.series_block([s]).nnz - entries for s in spare}
        miss = min(abs(int(per_series[j]) - over[s]) for s in spare for j in range(tw.n))
        fits = [(j, s) for s in spare for j in range(tw.n) if abs(int(per_series[j]) - over[s]) == miss]
        j, s = fits[int(rng.randint(len(fits)))]
        tw.pool = [s] + [x for x in tw.pool if x != s]
        yield churn_op(tw, 'churn-add', [int(j)], add=1)
        copies = np.zeros((tw.T, tw.n), dtype=np.int64); np.add.at(copies, (tw.raw.rows, tw.raw.cols), 1)
        (sr, sc), (ur, uc) = np.nonzero(copies == 1), np.nonzero(copies == 0)      # (a doubled cell would take two entries along)
        ps, pu = rng.permutation(sr.size)[:10], rng.permutation(ur.size)[:10]
        must = [(int(r), int(c), True) for r, c in zip(sr[ps], sc[ps])] + [(int(r), int(c), False) for r, c in zip(ur[pu], uc[pu])]
        yield revise_op(tw, rng, must=must, count=20)
    else:
        spare = [s for s in range(OH.N) if s not in tw.series]
        s = spare[int(rng.randint(len(spare)))]
        tw.pool = [s] + [x for x in tw.pool if x != s]
        yield churn_op(tw, 'churn-add', [int(rng.randint(tw.n))], add=1)
        yield revise_op(tw, rng, count=20)


# ---- seeded random sequences -----------------------------------------------------------------------------------------------------
RANDOM_STEPS = 12
# four seeds per form, chosen in tests/test_session_life_host.py's conditions: together they hold every ordered pair of LABELS, and
# each holds every kind of edit at least twice
SEEDS = {'sparse-missing': (2, 3, 8, 10), 'sparse-full': (14, 15, 16, 17), 'dense': (18, 20, 21, 23), 'dense-transform': (24, 25, 27, 183)}


def legal(tw, label):
    """Whether the twin says the session takes an op of this label (and the sequence can go on afterwards)."""
    if label == 'retire':
        return tw.T - 1 >= MIN_ROWS
    if label in ('slide', 'append'):
        return tw.t0 + tw.T + STEP <= OH.T
    if label == 'churn-add':
        return len(tw.pool) >= 1
    if label == 'churn-retire':
        return tw.n - 1 >= MIN_SERIES
    return True


def random_life(tw, seed, steps=RANDOM_STEPS):
    """`steps` ops drawn from LABELS; the arguments are drawn so that the twin says the call is legal: at least MIN_ROWS rows and
    MIN_SERIES series stay, no cell twice in a batch, no deletes on dense storage."""
    rng, cells = np.random.RandomState(1000 + seed), np.random.RandomState(2000 + seed)      # (the ops do not depend on the storage)
    for _ in range(steps):
        label = LABELS[rng.randint(len(LABELS))]
        while not legal(tw, label):
            label = LABELS[rng.randint(len(LABELS))]
        if label == 'slide':
            yield slide_op(tw, label, retire=int(rng.randint(0, min(2 * STEP, tw.T + STEP - MIN_ROWS) + 1)))
        elif label == 'retire':
            yield slide_op(tw, label, retire=int(rng.randint(1, min(2 * STEP, tw.T - MIN_ROWS) + 1)))
        elif label == 'append':
            yield slide_op(tw, label)
        elif label == 'churn-add':
            gone = int(rng.randint(0, min(3, tw.n - MIN_SERIES) + 1))
            yield churn_op(tw, label, sorted(rng.permutation(tw.n)[:gone].tolist()), add=int(rng.randint(1, min(3, len(tw.pool)) + 1)))
        elif label == 'churn-retire':
            gone = int(rng.randint(1, min(3, tw.n - MIN_SERIES) + 1))
            yield churn_op(tw, label, sorted(rng.permutation(tw.n)[:gone].tolist()))
        else:
            yield revise_op(tw, cells)


SEQUENCES = {'all-pairs': all_pairs, 'edges': edges}


# ---- the same life on plain lists of (row, col, val) tuples ------------------------------------------------------------------------
class Brute(object):
    """Both orientations as Python lists of (row, col, val) in stored order (sparse), or a dict over design cells (dense), advanced
    by loops over the entries: brute_revise, brute_churn and a loop restating trmf.online.slide_entries."""

    def __init__(self, tw):
        self.sparse = tw.sparse
        if tw.sparse:
            csr, csc = CH.entry_lists(tw.raw)
            self.csr, self.csc = self._tuples(csr), self._tuples(csc)
        else:
            self.cells = {(tw.t0 + i, tw.series[j]): tw.Y[i, j] for i in range(tw.T) for j in range(tw.n)}
        self.t0, self.T, self.series = tw.t0, tw.T, list(tw.series)

    @staticmethod
    def _tuples(lists):
        return [(int(r), int(c), v) for r, c, v in zip(*lists)]

    @staticmethod
    def _grouped(items, key):
        out = []
        for m in sorted(set(key(e) for e in items)):
            out += [e for e in items if key(e) == m]
        return out

    def apply(self, op):
        if op.kind == 'update':
            if op.revisions is not None:
                self.apply(Op('revise', rows=op.revisions[0], cols=op.revisions[1], vals=op.revisions[2], delete=None))
            window = getattr(op, 'window', None)
            retire = max(0, self.T + op.block.shape[0] - window) if window is not None else 0
            return self.apply(Op('slide', block=op.block, retire=retire))
        if op.kind == 'stats':
            return
        if not self.sparse:
            return self._dense(op)
        if op.kind == 'slide':
            Tk = self.T - op.retire
            for name, key in (('csr', lambda e: e[0]), ('csc', lambda e: e[1])):
                kept = []
                for r, c, v in getattr(self, name):                     # slide_entries: a stable filter, row numbers reduced
                    if r >= op.retire:
                        kept.append((r - op.retire, c, v))
                if op.block is not None:
                    blk = self._tuples(CH.entry_lists(op.block)[0 if name == 'csr' else 1])
                    kept = self._grouped(kept + [(r + Tk, c, v) for r, c, v in blk], key)
                setattr(self, name, kept)
            self.t0 += op.retire
            self.T = Tk + (op.block.shape[0] if op.block is not None else 0)
        elif op.kind == 'churn':
            n0 = len(self.series)
            keep = np.ones(n0, dtype=bool) if op.keep is None else op.keep
            for i, (name, major) in enumerate((('csr', 'row'), ('csc', 'col'))):
                L = getattr(self, name)
                blk = CH.entry_lists(op.block)[i] if op.block is not None else None
                setattr(self, name, CH.brute_churn([e[0] for e in L], [e[1] for e in L], [e[2] for e in L], keep, n0, blk, major))
            self.series = [s for s, kp in zip(self.series, keep) if kp] + list(op.ids)
        else:
            dl = np.zeros(len(op.rows), dtype=bool) if op.delete is None else op.delete
            ed = (np.asarray(op.rows), np.asarray(op.cols), np.asarray(op.vals), dl)
            for name, major in (('csr', 'row'), ('csc', 'col')):
                L = getattr(self, name)
                setattr(self, name, RH.brute_revise([e[0] for e in L], [e[1] for e in L], [e[2] for e in L], ed, major))

    def _dense(self, op):
        if op.kind == 'slide':
            for cell in [cell for cell in self.cells if cell[0] < self.t0 + op.retire]:
                del self.cells[cell]
            Tk = self.T - op.retire
            self.t0 += op.retire
            if op.block is not None:
                for i in range(op.block.shape[0]):
                    for j, s in enumerate(self.series):
                        self.cells[(self.t0 + Tk + i, s)] = op.block[i, j]
            self.T = Tk + (op.block.shape[0] if op.block is not None else 0)
        elif op.kind == 'churn':
            keep = np.ones(len(self.series), dtype=bool) if op.keep is None else op.keep
            gone = set(s for s, kp in zip(self.series, keep) if not kp)
            for cell in [cell for cell in self.cells if cell[1] in gone]:
                del self.cells[cell]
            for j, s in enumerate(op.ids):
                for i in range(self.T):
                    self.cells[(self.t0 + i, s)] = op.block[i, j]
            self.series = [s for s, kp in zip(self.series, keep) if kp] + list(op.ids)
        else:
            for r, c, v in zip(op.rows, op.cols, op.vals):
                self.cells[(self.t0 + int(r), self.series[int(c)])] = v

    def same_as(self, tw):
        """Both orientations (or every cell) equal the twin's."""
        if (self.t0, self.T, self.series) != (tw.t0, tw.T, tw.series):
            return False
        if self.sparse:
            csr, csc = CH.entry_lists(tw.raw)
            return self.csr == self._tuples(csr) and self.csc == self._tuples(csc)
        return len(self.cells) == tw.Y.size and all(self.cells[(tw.t0 + i, tw.series[j])] == tw.Y[i, j] for i in range(tw.T) for j in range(tw.n))
