#!/usr/bin/env python3
"""Wall time of the robust online loading update (Session.adapt_series_robust after 1, 24 and 256 new rows) beside the plain
Session.adapt_series measured in the same run.

    python scripts/bench_adapt_robust.py [--reps 3] [--cases c3,imp] [--forget 0.98] [--c 3] [--sweeps 4] [--out profiles/online_adapt_robust.json]

Cases: synth.CONFIGS['c3'] (100 000 series x 10 000 timestamps, 1 % observed, k = 40) and synth.CONFIGS['imp'] (370 series x 26 304
timestamps, 80 % observed, k = 40), both fp32.

Per case TWO sessions are opened on the same rows with the same initial model and advanced in lock-step: per repetition and block
size m both initialise the series statistics, append the same m rows and filter them; then one runs adapt_series and the other
adapt_series_robust, both timed.  The two calls of a pair therefore see the same rows, the same tables and the same W up to what the
loadings of the pairs before have done to the filter (each session keeps the H its own calls gave it).  Every call is blocking and
ends in a stream synchronisation, so the times are host wall times of WHOLE CALLS: uploads of the start positions, thresholds and
weights, every kernel of the call (the per-series kernel with all its sweeps, the objective kernel, the two error passes, the
maximum) and the read-back of the sums and of the weights.  The scale is the resident noise (fit_noise after training).
`share_multi_sweep` is the share of the series with at least one new entry: the others run one sweep.  Nothing here is a target:
the numbers are recorded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'exp-trmf-nips16_amd'))

BLOCKS = (1, 24, 256)


def case(name, reps, forget, c, sweeps):
    import numpy as np
    from trmf import synth
    from trmf.session import Session
    cfg = synth.CONFIGS[name]
    p = synth.make(cfg, seed=0)
    Y = p['Y'].tocsr()
    T, n = Y.shape
    k = cfg['k']
    hyper = cfg.get('hyper', synth.HYPER)
    T0 = T - reps * sum(BLOCKS) - 1
    plain_ms, robust_ms = {m: [] for m in BLOCKS}, {m: [] for m in BLOCKS}
    entries, down, multi = {m: [] for m in BLOCKS}, {m: [] for m in BLOCKS}, {m: [] for m in BLOCKS}
    models = [synth.initial_model(Y[:T0], p['lag_set'], k, seed=0, dtype=np.dtype(cfg['dtype'])) for _ in range(2)]
    with Session(Y[:T0], models[0], missing=True, log_norms=False, timing=0, **hyper) as a, \
            Session(Y[:T0], models[1], missing=True, log_norms=False, timing=0, **hyper) as b:
        desc = b.describe()
        for s in (a, b):
            s.run(2).sync()
            s.fit_noise()
            # config 3's synthetic panel learns lag weights that are explosive under its lambdaAR (scripts/bench_adapt.py): the online
            # part runs without the AR prior; the times do not depend on the values
            s.set_lambdas(hyper['lambdaI'], 0.0, hyper['lambdaLag'])
            s.init_series_stats(forget)                     # warm-up: code objects, the pool's blocks
            s.update(Y[T0:T0 + 1])
        a.adapt_series()
        b.adapt_series_robust(c, sweeps)
        at = T0 + 1
        for _ in range(reps):
            for m in BLOCKS:
                for s in (a, b):
                    s.init_series_stats(forget)
                    s.update(Y[at:at + m])                  # append + assimilate: not timed here (scripts/bench_online.py)
                t0 = time.perf_counter()
                a.adapt_series()
                t1 = time.perf_counter()
                sums = b.adapt_series_robust(c, sweeps)
                t2 = time.perf_counter()
                plain_ms[m].append((t1 - t0) * 1e3); robust_ms[m].append((t2 - t1) * 1e3)
                entries[m].append(sums['entries']); down[m].append(sums['downweighted'])
                multi[m].append(float(np.count_nonzero(np.diff(Y[at:at + m].tocsc().indptr))) / n)
                at += m
    med = lambda v: float(np.median(v))
    out = dict(name=name, T=T, n=n, k=k, dtype=cfg['dtype'], forget=forget, c=c, sweeps=sweeps, reps=reps, session=desc, adapt=[])
    for m in BLOCKS:
        out['adapt'].append(dict(new_rows=m, entries_median=med(entries[m]), downweighted_median=med(down[m]), share_multi_sweep=med(multi[m]),
                                 robust_call_ms_median=med(robust_ms[m]), robust_call_ms_all=[float(v) for v in robust_ms[m]],
                                 plain_call_ms_median=med(plain_ms[m]), plain_call_ms_all=[float(v) for v in plain_ms[m]],
                                 robust_over_plain=med(robust_ms[m]) / med(plain_ms[m])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cases', default='c3,imp')
    ap.add_argument('--forget', type=float, default=0.98)
    ap.add_argument('--c', type=float, default=3.0)
    ap.add_argument('--sweeps', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    result = {'device': 'MI355X', 'what': 'host wall times of whole blocking calls; see scripts/bench_adapt_robust.py',
              'cases': [case(name, args.reps, args.forget, args.c, args.sweeps) for name in args.cases.split(',') if name]}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
