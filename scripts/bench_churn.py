#!/usr/bin/env python3
"""Wall time of series churn on a resident session beside the route without it: re-creating the session.

    python scripts/bench_churn.py [--case c3] [--share 0.01] [--reps 3] [--out profiles/online_churn.json]

Case: synth.CONFIGS['c3'] (100 000 series x 10 000 timestamps, 1 % observed, k = 40, fp32).  One session is created on the whole
problem, trained for two iterations and given series statistics (init_series_stats(1.0)).  Then, `reps` times each:

    replace   `share` of the series are retired and as many new ones added    (change_series(keep, block), fit on the device)
    add       `share` of the series are added                                  (add_series(block), fit on the device)

Every repetition is timed twice from the same state and ends in the same state:

    churn     trmf_session_change_series            the library call (blocking; ends in a device synchronisation)
    recreate  what a build without it offers: close the session, create it again from host arrays of the same churned data,
              init_series_stats, adapt_series       (the host arrays of the churned matrix -- both orientations, as the ABI takes
                                                     them -- are prepared BEFORE the clock starts: editing Y on the host is not
                                                     charged to this route, nor is the download)

`churn_py` is the same call through Session.change_series, which also rebuilds the host model (a copy of H).  The new series' data
are the columns of the problem itself (the times do not depend on the values).  One untimed churn of each kind warms both routes.
Host wall times of whole calls; nothing here is a target or a gate."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'exp-trmf-nips16_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='c3')
    ap.add_argument('--share', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    import scipy.sparse as smat
    from ctypes import byref
    from trmf import synth
    from trmf.rf_util import PyMatrix
    from trmf.session import Session, TrmfChurnSums
    cfg = synth.CONFIGS[args.case]
    p = synth.make(cfg, seed=0)
    dt = np.dtype(cfg['dtype'])
    hyper = cfg.get('hyper', synth.HYPER)
    cur = p['Y'].tocsc()
    pool = cur                                              # where the new series' data come from
    T, n = cur.shape
    rng = np.random.RandomState(7)
    kw = dict(missing=True, log_norms=False, timing=0)
    kw.update(hyper)

    def open_session(Y, H, W, theta):
        from trmf.model import Model
        model = Model.from_arrays(W, H, theta, p['lag_set'])
        return Session(Y, model, **kw)

    m0 = synth.initial_model(cur, p['lag_set'], cfg['k'], seed=0, dtype=dt)
    s = Session(cur.tocsr(), m0, **kw)
    s.run(2).sync()
    s.init_series_stats(1.0)
    desc = s.describe()
    runs = []
    plan = [('replace', True), ('add', True)] + [('replace', False)] * args.reps + [('add', False)] * args.reps
    for kind, warm in plan:
        n0 = cur.shape[1]
        cnt = max(1, int(round(args.share * n0)))
        keep = np.ones(n0, dtype=bool)
        if kind == 'replace':
            keep[rng.permutation(n0)[:cnt]] = False
        block = pool[:, rng.permutation(pool.shape[1])[:cnt]].tocsc()
        nxt = smat.hstack([cur[:, np.flatnonzero(keep)], block]).tocsc()          # host prep of the churned data: not timed
        pm_next = PyMatrix(nxt.tocsr(), dtype=dt)                                  # ... both orientations as the ABI takes them
        pm_block = PyMatrix(block.tocsr(), dtype=dt)
        flags = np.ascontiguousarray(keep.astype(np.uint8))
        m = s.download()
        W, H0, theta = m.W.copy(), m.H.copy(), m.lag_val.copy()
        # route 1: the library call
        sums = TrmfChurnSums()
        t0 = time.perf_counter()
        rc = s.lib.trmf_session_change_series(s.handle, flags.ctypes.data, byref(pm_block), 1, None, None, None, byref(sums))
        t_churn = (time.perf_counter() - t0) * 1e3
        if rc < 0:
            raise RuntimeError(s.lib.trmf_last_error().decode())
        assert sums.series == nxt.shape[1] and sums.entries == nxt.nnz and sums.stats_carried == 1 and sums.fitted == 1
        # (the host model of the new size, so that the session can be downloaded)
        Hh = np.zeros((nxt.shape[1], cfg['k']), dtype=dt)
        Hh[:int(keep.sum())] = H0[keep]
        s.model = type(m).from_arrays(W, Hh, theta, p['lag_set'])
        H1 = s.download().H.copy()
        # route 2: close, create again from host arrays of the same data, statistics from zero, loadings of every series
        t0 = time.perf_counter()
        s.close()
        t_close = (time.perf_counter() - t0) * 1e3
        s = open_session(pm_next, Hh.copy(), W, theta)
        t_create = (time.perf_counter() - t0) * 1e3 - t_close
        s.init_series_stats(1.0)
        t_init = (time.perf_counter() - t0) * 1e3 - t_close - t_create
        s.adapt_series()
        t_all = (time.perf_counter() - t0) * 1e3
        Hre = s.download().H.copy()
        new = slice(int(keep.sum()), nxt.shape[1])
        dev = float(np.abs(Hre[new] - H1[new]).max() / max(np.abs(Hre[new]).max(), 1e-30))
        cur = nxt
        r = dict(kind=kind, warmup=warm, series_before=int(n0), series_changed=int(cnt), series_after=int(nxt.shape[1]), entries_after=int(nxt.nnz),
                 block_entries=int(block.nnz), churn_ms=round(t_churn, 3), recreate_ms=round(t_all, 3),
                 recreate_split_ms=dict(close=round(t_close, 3), create=round(t_create, 3), init_series_stats=round(t_init, 3),
                                        adapt_series=round(t_all - t_close - t_create - t_init, 3)),
                 ratio_recreate_over_churn=round(t_all / t_churn, 2), new_loadings_relmax_between_routes=dev)
        runs.append(r)
        print('{:>8s}{}: change_series {:.1f} ms, re-creation {:.1f} ms (close {:.1f}, create {:.1f}, init {:.1f}, adapt {:.1f}): {:.1f} x; new loadings differ by {:.1e}'.format(
            kind, ' (warm-up)' if warm else '', t_churn, t_all, t_close, t_create, t_init, t_all - t_close - t_create - t_init, t_all / t_churn, dev), flush=True)
    # the Python front end's call (also rebuilds the host model): once per kind on the final state
    py = {}
    for kind in ('replace', 'add'):
        n0 = cur.shape[1]
        cnt = max(1, int(round(args.share * n0)))
        keep = np.ones(n0, dtype=bool)
        if kind == 'replace':
            keep[rng.permutation(n0)[:cnt]] = False
        block = pool[:, rng.permutation(pool.shape[1])[:cnt]].tocsc()
        pm_block = PyMatrix(block.tocsr(), dtype=dt)
        t0 = time.perf_counter()
        s.change_series(keep if kind == 'replace' else None, pm_block)
        py[kind] = round((time.perf_counter() - t0) * 1e3, 3)
        cur = smat.hstack([cur[:, np.flatnonzero(keep)], block]).tocsc()
    s.close()
    timed = [r for r in runs if not r['warmup']]
    summary = {}
    for kind in ('replace', 'add'):
        a = [r['churn_ms'] for r in timed if r['kind'] == kind]
        b = [r['recreate_ms'] for r in timed if r['kind'] == kind]
        summary[kind] = dict(churn_ms_median=float(np.median(a)), recreate_ms_median=float(np.median(b)),
                             ratio_recreate_over_churn=round(float(np.median(b)) / float(np.median(a)), 2), churn_py_ms=py[kind])
        print('{:>8s}: median change_series {:.1f} ms, re-creation {:.1f} ms, ratio {:.1f}; through Session.change_series {:.1f} ms'.format(
            kind, summary[kind]['churn_ms_median'], summary[kind]['recreate_ms_median'], summary[kind]['ratio_recreate_over_churn'], py[kind]), flush=True)
    result = {'device': 'MI355X', 'what': 'host wall times of whole blocking calls; see scripts/bench_churn.py',
              'case': dict(name=args.case, T=int(T), n=int(n), k=cfg['k'], dtype=cfg['dtype'], nnz=int(p['Y'].nnz), share=args.share, reps=args.reps),
              'session': desc, 'summary': summary, 'runs': runs}
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(result, indent=1) + '\n')


if __name__ == '__main__':
    main()
