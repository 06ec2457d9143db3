#!/usr/bin/env python3
"""Wall time of cell revisions on a resident session beside the route without them: re-creating the session.

    python scripts/bench_revise.py [--case c3] [--shares 0.001,0.01] [--rows 48] [--reps 5] [--out profiles/online_revise.json]

Case: synth.CONFIGS['c3'] (100 000 series x 10 000 timestamps, 1 % observed, k = 40, fp32).  One session is created on the whole
problem, trained for two iterations and given series statistics (init_series_stats(1.0)).  Then, per share and `reps` times each, a
batch of `share` x (stored cells of the whole problem) distinct cells in the LAST `rows` timestamps is revised: replaces of stored
cells (half of the batch, at most half of the cells those rows store), deletes of stored cells (a tenth, at most a quarter of
them) and inserts of unstored cells (the rest) -- late and corrected observations of the recent past.

Every repetition is timed twice from the same state and ends in the same state:

    revise    trmf_session_revise(update_stats = 1)  the library call (blocking; ends in a device synchronisation)
    recreate  what a build without it offers: close the session, create it again from host arrays of the same revised data,
              init_series_stats                      (the host arrays of the revised matrix -- both orientations, as the ABI takes
                                                      them -- are prepared BEFORE the clock starts: editing Y on the host is not
                                                      charged to this route, nor is the download of the factors)

This is the route scripts/bench_churn.py charges, without its adapt_series (revise does not refit H either).  `revise_py` is the
same call through Session.revise, which also refreshes the front end's per-row entry counts.  One untimed revise per share warms
both routes.  Host wall times of whole calls: median, min and max over the repetitions; nothing here is a target or a gate."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'exp-trmf-nips16_amd'))


def draw_batch(rng, cur, rows, count):
    """`count` distinct cells of the last `rows` rows of the canonical CSR `cur`: (rows, cols, vals, delete)."""
    import numpy as np
    T, n = cur.shape
    lo = T - rows
    tail = cur[lo:].tocoo()
    stored = tail.row.astype(np.int64) * n + tail.col.astype(np.int64)
    n_rep = min(count // 2, stored.size // 2)
    n_del = min(count // 10, stored.size // 4)
    pick = rng.permutation(stored.size)[:n_rep + n_del]
    n_ins = count - n_rep - n_del
    cand = np.unique(rng.randint(0, rows * n, size=int(n_ins * 1.2) + 16).astype(np.int64))
    cand = rng.permutation(np.setdiff1d(cand, stored))[:n_ins]
    cells = np.concatenate([stored[pick], cand])
    dele = np.zeros(cells.size, dtype=bool)
    dele[n_rep:n_rep + n_del] = True
    p = rng.permutation(cells.size)                          # the batch arrives in no particular order
    cells, dele = cells[p], dele[p]
    vals = (rng.rand(cells.size) + 0.25).astype(cur.dtype)
    return cells // n + lo, cells % n, vals, dele


def revised_host(cur, batch):
    """The canonical CSR of the revised matrix (host prep of route 2; not timed)."""
    import numpy as np
    import scipy.sparse as smat
    r, c, v, d = batch
    T, n = cur.shape
    coo = cur.tocoo()
    stay = ~np.isin(coo.row.astype(np.int64) * n + coo.col, r * n + c)
    out = smat.csr_matrix((np.concatenate([coo.data[stay], v[~d]]), (np.concatenate([coo.row[stay], r[~d]]), np.concatenate([coo.col[stay], c[~d]]))),
                          shape=cur.shape)
    out.sort_indices()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='c3')
    ap.add_argument('--shares', default='0.001,0.01')
    ap.add_argument('--rows', type=int, default=48)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    from ctypes import byref
    from trmf import synth
    from trmf.model import Model
    from trmf.rf_util import PyMatrix
    from trmf.session import Session, TrmfReviseSums
    cfg = synth.CONFIGS[args.case]
    p = synth.make(cfg, seed=0)
    dt = np.dtype(cfg['dtype'])
    hyper = cfg.get('hyper', synth.HYPER)
    cur = p['Y'].tocsr()
    cur.sort_indices()
    T, n = cur.shape
    nnz0 = int(cur.nnz)
    rng = np.random.RandomState(7)
    kw = dict(missing=True, log_norms=False, timing=0)
    kw.update(hyper)
    m0 = synth.initial_model(cur, p['lag_set'], cfg['k'], seed=0, dtype=dt)
    s = Session(cur, m0, **kw)
    s.run(2).sync()
    s.init_series_stats(1.0)
    desc = s.describe()
    shares = [float(x) for x in args.shares.split(',')]
    runs, py = [], {}
    for share in shares:
        count = max(1, int(round(share * nnz0)))
        for rep in range(-1, args.reps + 1):                 # -1: warm-up; reps: the front end's call
            batch = draw_batch(rng, cur, args.rows, count)
            r32, c32 = np.ascontiguousarray(batch[0].astype(np.uint32)), np.ascontiguousarray(batch[1].astype(np.uint32))
            vals, flags = np.ascontiguousarray(batch[2]), np.ascontiguousarray(batch[3].astype(np.uint8))
            nxt = revised_host(cur, batch)                    # host prep of the revised data: not timed
            if rep == args.reps:
                t0 = time.perf_counter()
                s.revise(batch[0], batch[1], batch[2], batch[3], update_stats=True)
                py[share] = round((time.perf_counter() - t0) * 1e3, 3)
                cur = nxt
                continue
            pm_next = PyMatrix(nxt, dtype=dt)                 # ... both orientations as the ABI takes them
            m = s.download()
            W, H, theta = m.W.copy(), m.H.copy(), m.lag_val.copy()
            # route 1: the library call
            sums = TrmfReviseSums()
            t0 = time.perf_counter()
            rc = s.lib.trmf_session_revise(s.handle, r32.size, r32.ctypes.data, c32.ctypes.data, vals.ctypes.data, flags.ctypes.data, 1, byref(sums))
            t_rev = (time.perf_counter() - t0) * 1e3
            if rc < 0:
                raise RuntimeError(s.lib.trmf_last_error().decode())
            assert sums.entries == nxt.nnz and sums.stats_carried == 1 and sums.missed == 0 and sums.edits == r32.size
            J1 = s.objective()
            # route 2: close, create again from host arrays of the same data, statistics from zero
            t0 = time.perf_counter()
            s.close()
            t_close = (time.perf_counter() - t0) * 1e3
            s = Session(pm_next, Model.from_arrays(W, H, theta, p['lag_set']), **kw)
            t_create = (time.perf_counter() - t0) * 1e3 - t_close
            s.init_series_stats(1.0)
            t_all = (time.perf_counter() - t0) * 1e3
            J2 = s.objective()
            cur = nxt
            row = dict(share=share, warmup=rep < 0, edits=int(r32.size), replaced=int(sums.replaced), inserted=int(sums.inserted), deleted=int(sums.deleted),
                       entries_after=int(nxt.nnz), revise_ms=round(t_rev, 3), recreate_ms=round(t_all, 3),
                       recreate_split_ms=dict(close=round(t_close, 3), create=round(t_create, 3), init_series_stats=round(t_all - t_close - t_create, 3)),
                       ratio_recreate_over_revise=round(t_all / t_rev, 2), objective_rel_diff_between_routes=abs(J1 - J2) / abs(J2))
            runs.append(row)
            print('{:>7.3%}{}: {} edits ({} replaced, {} inserted, {} deleted): revise {:.2f} ms, re-creation {:.2f} ms (close {:.2f}, create {:.2f}, init {:.2f}): {:.1f} x; '
                  'objectives differ by {:.1e}'.format(share, ' (warm-up)' if rep < 0 else '', r32.size, sums.replaced, sums.inserted, sums.deleted, t_rev, t_all, t_close,
                                                       t_create, t_all - t_close - t_create, t_all / t_rev, row['objective_rel_diff_between_routes']), flush=True)
    s.close()
    summary = {}
    for share in shares:
        a = [r['revise_ms'] for r in runs if r['share'] == share and not r['warmup']]
        b = [r['recreate_ms'] for r in runs if r['share'] == share and not r['warmup']]
        stat = lambda x: dict(median=float(np.median(x)), min=float(np.min(x)), max=float(np.max(x)))
        summary['%g' % share] = dict(edits=int(round(share * nnz0)), revise_ms=stat(a), recreate_ms=stat(b),
                                     ratio_recreate_over_revise=round(float(np.median(b)) / float(np.median(a)), 2), revise_py_ms=py[share])
        print('{:>7.3%}: revise median {:.2f} ms (min {:.2f}, max {:.2f}), re-creation median {:.2f} ms (min {:.2f}, max {:.2f}), ratio {:.1f}; through Session.revise {:.2f} ms'.format(
            share, np.median(a), np.min(a), np.max(a), np.median(b), np.min(b), np.max(b), np.median(b) / np.median(a), py[share]), flush=True)
    result = {'device': 'MI355X', 'what': 'host wall times of whole blocking calls; see scripts/bench_revise.py',
              'case': dict(name=args.case, T=int(T), n=int(n), k=cfg['k'], dtype=cfg['dtype'], nnz=nnz0, rows=args.rows, reps=args.reps),
              'session': desc, 'summary': summary, 'runs': runs}
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(result, indent=1) + '\n')


if __name__ == '__main__':
    main()
