#!/usr/bin/env python3
"""Wall time of the robust fixed-interval smoother (trmf_session_smooth_robust, four sweeps) beside the plain smoother
(trmf_session_smooth) for the same window on the same session, on bench_smooth.py's own shape.

    python scripts/bench_smooth_robust.py [--reps 10] [--cases paper,imp,wide] [--out profiles/online_smooth_robust.json]
                                          [--kernel-csv paper=DIR,imp=DIR,wide=DIR]

Per case one session is trained on all but the last (reps + 1) x 24 rows and its noise fitted (the robust calls use the resident
scale, c = 3).  Then, block by block: append_rows and assimilate_robust the block, and for smooth_back in (24, 96): mark, smooth
the window (timed), rewind, smooth_robust the window with four sweeps (timed), rewind.  The calls are blocking, so the times are
host wall times of whole calls; the first block is warm-up.  The split of a sweep into its Gram build (smooth_robust_part_kernel,
smooth_robust_fold_kernel), the factors (assim_factor_kernel) and the PCG (smooth_ar / apply / update) cannot be seen from the
host: --kernel-csv names, per case, a directory with the kernel trace (csv) of a profiler run of THIS script with that one case
(`rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/bench_smooth_robust.py --reps R --cases NAME`); the kernel
times of the robust calls are summed per sweep.  Nothing here is a target: the numbers are recorded."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'exp-trmf-nips16_amd'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import bench_robust  # noqa: E402  (the three cases and their problems)

STEPS = 24
BACKS = (24, 96)
SWEEPS = 4
C = 3.0
GROUPS = {'gram': ('smooth_robust_part_kernel', 'smooth_robust_fold_kernel'), 'factor': ('assim_factor_kernel',),
          'pcg': ('smooth_ar_kernel', 'smooth_apply_kernel', 'smooth_update_kernel')}


def _kernel_split(path):
    """ms per sweep of the three parts of a robust sweep from the kernel-trace csv files under `path`.  A robust call launches the
    fold kernel once per sweep, so its dispatches count the sweeps; the factor and PCG kernels of the plain smoother's calls are
    told apart by order: only dispatches between a fold kernel and the next smooth_finish_kernel belong to a sweep."""
    rows = []
    for f in glob.glob(os.path.join(path, '**', '*kernel_trace.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                low = {key.lower(): v for key, v in row.items()}
                rows.append((int(low['start_timestamp']), int(low['end_timestamp']), low.get('kernel_name', '')))
    rows.sort()
    tot = {key: 0 for key in GROUPS}
    sweeps, inside = 0, False
    for t0, t1, name in rows:
        if any(n in name for n in GROUPS['gram']):           # only robust calls launch these
            tot['gram'] += t1 - t0
        if 'smooth_robust_fold_kernel' in name:
            sweeps += 1
            inside = True
        elif 'smooth_finish_kernel' in name:
            inside = False
        elif inside:
            for key in ('factor', 'pcg'):
                if any(n in name for n in GROUPS[key]):
                    tot[key] += t1 - t0
    if not sweeps:
        raise SystemExit('no smooth_robust_fold_kernel dispatch in the kernel traces under ' + path)
    return dict(sweeps=sweeps, ms_per_sweep={key: ns * 1e-6 / sweeps for key, ns in tot.items()},
                note='the two score-only part launches of a call are counted with its Gram builds')


def case(name, reps, kernel_csv=None):
    import numpy as np
    from trmf import synth
    from trmf.session import Session
    c = bench_robust.CASES[name]
    Y, block = bench_robust._problem(c)
    T0 = c['T'] - (reps + 1) * STEPS
    model = synth.initial_model(block(0, T0), c['lags'], c['k'], seed=0, dtype=np.dtype(c['dtype']))
    per_back = {back: dict(smooth_ms=[], robust_ms=[], sums=[], plain=[]) for back in BACKS}
    with Session(block(0, T0), model, missing=c['missing'], log_norms=False, timing=0, **c['hyper']) as s:
        s.run(c['max_iter']).sync()
        s.fit_noise()
        desc = s.describe()
        for r in range(reps + 1):
            s.append_rows(block(T0 + r * STEPS, T0 + (r + 1) * STEPS))
            first = s.rows() - STEPS
            s.assimilate_robust(first, C, SWEEPS)
            for back in BACKS:
                s.mark()
                t0 = time.perf_counter()
                plain = s.smooth(first - back)
                t1 = time.perf_counter()
                s.rewind()
                t2 = time.perf_counter()
                out = s.smooth_robust(first - back, C, SWEEPS)
                t3 = time.perf_counter()
                s.rewind()
                per_back[back]['smooth_ms'].append((t1 - t0) * 1e3)
                per_back[back]['robust_ms'].append((t3 - t2) * 1e3)
                per_back[back]['sums'].append(out)
                per_back[back]['plain'].append(plain)
    med = lambda v: float(np.median(v[1:]))
    res = dict(name=name, T=c['T'], n=c['n'], k=c['k'], nlag=len(c['lags']), dtype=c['dtype'], missing=c['missing'], block_rows=STEPS, reps=reps,
               sweeps=SWEEPS, c=C, session=desc)
    for back in BACKS:
        p = per_back[back]
        its = [o['iterations'] for o in p['sums'][1:]]
        res['smooth_back_%d' % back] = dict(
            window_rows=STEPS + back, smooth_ms_median=med(p['smooth_ms']), smooth_robust_ms_median=med(p['robust_ms']),
            smooth_robust_ms_min=float(min(p['robust_ms'][1:])), robust_over_plain=med(p['robust_ms']) / med(p['smooth_ms']),
            ms_per_sweep_wall=med(p['robust_ms']) / SWEEPS, iterations_all_sweeps=its, plain_iterations=[o['iterations'] for o in p['plain'][1:]],
            converged=[o['converged'] for o in p['sums'][1:]], downweighted_share=[o['downweighted'] / max(o['entries'], 1) for o in p['sums'][1:]],
            objective_drop=[1.0 - o['objective_after'] / o['objective_before'] for o in p['sums'][1:]])
    if kernel_csv:
        res['kernel_trace'] = _kernel_split(kernel_csv)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cases', default='paper,imp,wide')
    ap.add_argument('--kernel-csv', default='', help='NAME=DIR[,NAME=DIR...]: kernel traces of profiler runs of this script, one case each')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    traces = dict(item.split('=', 1) for item in args.kernel_csv.split(',') if item)
    result = {'device': 'MI355X', 'cases': [case(name, args.reps, traces.get(name)) for name in args.cases.split(',') if name]}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
