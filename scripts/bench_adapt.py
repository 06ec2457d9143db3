#!/usr/bin/env python3
"""Wall time of the online loading updates (Session.init_series_stats, Session.adapt_series after 1, 24 and 256 new rows) beside
one ALS iteration of the same session (run(1): its F phase from stats(), and the whole step).

    python scripts/bench_adapt.py [--reps 3] [--cases c3,imp] [--forget 0.98] [--out profiles/online_adapt.json]

Cases: synth.CONFIGS['c3'] (100 000 series x 10 000 timestamps, 1 % observed, k = 40: ~100 entries per series) and
synth.CONFIGS['imp'] (370 series x 26 304 timestamps, 80 % observed, k = 40: ~21 000 entries per series).

Per case one session is trained on all but the last reps x (1 + 24 + 256) + 1 rows.  Then, per repetition and per block size m:
init_series_stats (timed), append m rows, assimilate them, adapt_series (timed).  Every call is blocking and ends in a stream
synchronisation, so the times are host wall times of WHOLE CALLS: the upload of the start positions and weights, every kernel of
the call (the per-series kernel, the two error passes, the maximum) and the read-back.  `bytes_model` is what the per-series
kernel has to move -- both generations of the tables, the gathered rows of W, H old and new -- computed from the shapes;
`fraction_of_8TBs` is that over the call's time over 8 TB/s, a lower bound of the kernel's own share of peak because the call
holds more than the kernel.  Nothing here is a target: the numbers are recorded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'exp-trmf-nips16_amd'))

BLOCKS = (1, 24, 256)
PEAK_BYTES_PER_S = 8e12


def case(name, reps, forget):
    import numpy as np
    from trmf import synth
    from trmf.session import Session
    cfg = synth.CONFIGS[name]
    p = synth.make(cfg, seed=0)
    Y = p['Y'].tocsr()
    T, n = Y.shape
    k, size = cfg['k'], np.dtype(cfg['dtype']).itemsize
    hyper = cfg.get('hyper', synth.HYPER)
    T0 = T - reps * sum(BLOCKS) - 1
    model = synth.initial_model(Y[:T0], p['lag_set'], k, seed=0, dtype=np.dtype(cfg['dtype']))
    packed = k * (k + 1) // 2
    init_ms, adapt_ms, rows_absorbed = [], {m: [] for m in BLOCKS}, {m: [] for m in BLOCKS}
    with Session(Y[:T0], model, missing=True, log_norms=False, timing=1, **hyper) as s:
        s.run(2).sync()
        desc = s.describe()
        # config 3's synthetic panel learns lag weights that are explosive under its lambdaAR: 256 filtered rows
        # overflow W, and adapt_series rightly refuses a non-finite system.  The times do not depend on the values, so the online
        # part runs without the AR prior.
        s.set_lambdas(hyper['lambdaI'], 0.0, hyper['lambdaLag'])
        s.init_series_stats(forget)                         # warm-up: code objects, the pool's blocks
        s.update(Y[T0:T0 + 1], adapt=True)
        at = T0 + 1
        for _ in range(reps):
            for m in BLOCKS:
                t0 = time.perf_counter()
                s.init_series_stats(forget)
                t1 = time.perf_counter()
                s.update(Y[at:at + m])                      # append + assimilate: not timed here (scripts/bench_online.py)
                t2 = time.perf_counter()
                sums = s.adapt_series()
                t3 = time.perf_counter()
                init_ms.append((t1 - t0) * 1e3); adapt_ms[m].append((t3 - t2) * 1e3); rows_absorbed[m].append(sums['entries'])
                at += m
        nnz = int(Y[:at].nnz)
        s.set_lambdas(hyper['lambdaI'], hyper['lambdaAR'], hyper['lambdaLag'])
        t0 = time.perf_counter()
        s.run(1).sync()
        step_ms = (time.perf_counter() - t0) * 1e3
        st = s.stats(1)[-1]
    med = lambda v: float(np.median(v))
    out = dict(name=name, T=T, n=n, k=k, dtype=cfg['dtype'], nnz=nnz, forget=forget, reps=reps, session=desc,
               init_ms_median=med(init_ms), init_ms_all=[float(v) for v in init_ms],
               run1_step_ms=step_ms, run1_F_phase_ms=float(st['ms_F']), run1_F_kernel_ms=float(st['ms_F_kernel']), adapt=[])
    for m in BLOCKS:
        entries = med(rows_absorbed[m])
        bytes_model = (2 * n * (packed + k) + entries * k + 2 * n * k) * size + entries * 2 * 4
        t = med(adapt_ms[m]) * 1e-3
        out['adapt'].append(dict(new_rows=m, entries_median=entries, call_ms_median=med(adapt_ms[m]), call_ms_all=[float(v) for v in adapt_ms[m]],
                                 bytes_model=bytes_model, fraction_of_8TBs=bytes_model / t / PEAK_BYTES_PER_S))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cases', default='c3,imp')
    ap.add_argument('--forget', type=float, default=0.98)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    result = {'device': 'MI355X', 'what': 'host wall times of whole blocking calls; see scripts/bench_adapt.py',
              'cases': [case(name, args.reps, args.forget) for name in args.cases.split(',') if name]}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
