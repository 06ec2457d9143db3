#!/usr/bin/env python3
"""Wall time of the fixed-interval smoother (trmf_session_smooth) behind a 24-row online update, beside the forward filter
(trmf_session_assimilate) over the same range of rows on the same session.

    python scripts/bench_smooth.py [--reps 10] [--cases paper,imp,wide] [--out profiles/online_smooth.json]
                                   [--kernel-csv paper=DIR,imp=DIR,wide=DIR]

Cases: bench_robust.py's `paper` (26 304 x 370 dense, k = 60, 48 lags, missing=False), `imp` (the same panel 80 % observed, k = 40,
16 lags, missing=True) and `wide` (config 3: 100 000 series x 10 000 timestamps at 1 % density, k = 40, 16 lags).

Per case one session is trained on all but the last (reps + 1) x 24 rows.  Then, block by block: append_rows and assimilate the
block (timed: smooth_back = 0), and for smooth_back in (24, 96): mark, assimilate over the rows of the window (timed: the filter
over the same range, the cost of those rows before this feature), rewind, smooth the window (timed), rewind.  The calls are
blocking, so the times are host wall times of whole calls; the first block is warm-up.  The smoother's kernel time cannot be seen
from the host: --kernel-csv names, per case, a directory with the kernel trace (csv) of a profiler run of THIS script with that
one case (`rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/bench_smooth.py --reps R --cases NAME`); its
smooth_* rows are summed per smoother call.  The byte model per step is the Gram table plus the factor table, 2 m k^2 elements
(one k^2 on the shared-Gram forms).  Nothing here is a target: the numbers are recorded."""
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
KERNELS = ('smooth_ar_kernel', 'smooth_apply_kernel', 'smooth_update_kernel', 'smooth_finish_kernel')


def _kernel_times(path):
    """ms per smoother call of the smooth_* kernels from the kernel-trace csv files under `path`; a call launches the finish kernel
    once, so its dispatches count the calls."""
    tot = {}
    for f in glob.glob(os.path.join(path, '**', '*kernel_trace.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                low = {key.lower(): v for key, v in row.items()}
                name = low.get('kernel_name', '')
                for key in KERNELS:
                    if key in name:
                        ns, cnt = tot.get(key, (0, 0))
                        tot[key] = (ns + int(low['end_timestamp']) - int(low['start_timestamp']), cnt + 1)
    calls = tot.get('smooth_finish_kernel', (0, 0))[1]
    if not calls:
        raise SystemExit('no smooth_finish_kernel dispatch in the kernel traces under ' + path)
    return {key: dict(ms_per_call=ns * 1e-6 / calls, dispatches_per_call=cnt / calls) for key, (ns, cnt) in tot.items()}


def case(name, reps, kernel_csv=None):
    import numpy as np
    from trmf import synth
    from trmf.session import Session
    c = bench_robust.CASES[name]
    Y, block = bench_robust._problem(c)
    T0 = c['T'] - (reps + 1) * STEPS
    model = synth.initial_model(block(0, T0), c['lags'], c['k'], seed=0, dtype=np.dtype(c['dtype']))
    plain = []
    per_back = {back: dict(filter_ms=[], smooth_ms=[], sums=[]) for back in BACKS}
    with Session(block(0, T0), model, missing=c['missing'], log_norms=False, timing=0, **c['hyper']) as s:
        s.run(c['max_iter']).sync()
        desc = s.describe()
        for r in range(reps + 1):
            s.append_rows(block(T0 + r * STEPS, T0 + (r + 1) * STEPS))
            first = s.rows() - STEPS
            t0 = time.perf_counter()
            s.assimilate(first)
            plain.append((time.perf_counter() - t0) * 1e3)
            for back in BACKS:
                s.mark()
                t0 = time.perf_counter()
                s.assimilate(first - back)
                t1 = time.perf_counter()
                s.rewind()
                t2 = time.perf_counter()
                out = s.smooth(first - back)
                t3 = time.perf_counter()
                s.rewind()
                per_back[back]['filter_ms'].append((t1 - t0) * 1e3)
                per_back[back]['smooth_ms'].append((t3 - t2) * 1e3)
                per_back[back]['sums'].append(out)
    med = lambda v: float(np.median(v[1:]))
    size = np.dtype(c['dtype']).itemsize
    res = dict(name=name, T=c['T'], n=c['n'], k=c['k'], nlag=len(c['lags']), dtype=c['dtype'], missing=c['missing'], block_rows=STEPS, reps=reps,
               session=desc, smooth_back_0=dict(assimilate_ms_median=med(plain), assimilate_ms_min=float(min(plain[1:]))))
    for back in BACKS:
        p = per_back[back]
        m = STEPS + back
        its = [o['iterations'] for o in p['sums'][1:]]
        tables = (m + (1 if not c['missing'] else m)) * c['k'] * c['k'] * size        # U_i per row; G_i per row, or the one shared Gram
        res['smooth_back_%d' % back] = dict(
            window_rows=m, smooth_ms_median=med(p['smooth_ms']), smooth_ms_min=float(min(p['smooth_ms'][1:])),
            filter_same_rows_ms_median=med(p['filter_ms']), smooth_over_filter=med(p['smooth_ms']) / med(p['filter_ms']),
            iterations=its, converged=[o['converged'] for o in p['sums'][1:]], residual=[o['residual'] for o in p['sums'][1:]],
            launches_per_call=[3 * it + 7 for it in its],                            # 3 per step, 3 at the start, the last test, finish, errors, factors
            us_per_step_wall=med(p['smooth_ms']) * 1e3 / max(float(np.mean(its)), 1.0),
            table_bytes_per_step=tables,
            objective_drop=[1.0 - o['objective_after'] / o['objective_before'] for o in p['sums'][1:]])
    if kernel_csv:
        res['kernel_trace'] = _kernel_times(kernel_csv)
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
