#!/usr/bin/env python3
"""Wall time of a robust online update (trmf_session_assimilate_robust, 4 sweeps) beside the plain one (trmf_session_assimilate)
of the same build, on the same session and the same 24-row blocks.

    python scripts/bench_robust.py [--reps 10] [--cases paper,imp,wide] [--out profiles/online_robust.json]
                                   [--kernel-csv paper=DIR,imp=DIR,wide=DIR]

Cases: bench_online.py's `paper` (26 304 x 370 dense, k = 60, 48 lags, missing=False) and `imp` (the same panel 80 % observed,
k = 40, 16 lags, missing=True), and `wide`: config 3 (100 000 series x 10 000 timestamps at 1 % density, k = 40, 16 lags), rows of
~1 000 gathered entries.

Per case one session is trained on all but the last (reps + 1) x 24 rows.  Then, block by block: append_rows, mark, assimilate
(timed), rewind, assimilate_robust (timed) with the block's one-step-ahead RMSE as the scale of every series (the in-sample
residual scale of fit_noise is too small where a series has few observations for its rank: most cells are then down-weighted
and the rows follow the AR prior alone).  Both calls are blocking, so the times
are host wall times of whole calls; the first block is warm-up.  The launch count is counted from the shapes.  The part kernel's
own time cannot be seen from the host: --kernel-csv names, per case, a directory with the kernel trace (csv) of a profiler run of
THIS script with that one case (`rocprofv3 --kernel-trace --output-format csv -d DIR -- python
scripts/bench_robust.py --reps R --cases NAME`); its assim_robust_* rows are summed per call (any --reps will do) and set against the byte model
sweeps * sum |Omega_i| * (k + 2) * sizeof(real) of the part kernel.  Nothing here is a target: the numbers are recorded."""
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

import bench_online  # noqa: E402  (the paper / imp cases and their panel)

STEPS, SWEEPS, C = 24, 4, 3.0
CASES = dict(bench_online.CASES)
CASES['wide'] = dict(T=10000, n=100000, k=40, lags=list(range(1, 17)), dtype='float32', missing=True, density=0.01, max_iter=10,
                     hyper=dict(lambdaI=0.5, lambdaAR=50, lambdaLag=0.5))


def _problem(c):
    """(Y the session trains on, block(r0, r1) -> rows in the session's storage class)."""
    import scipy.sparse as smat
    if 'density' in c:
        from trmf import synth
        Y = synth.sparse_problem(c['n'], c['T'], c['k'], len(c['lags']), c['density'], dtype=c['dtype'], seed=0)['Y'].tocsr()
        return Y, lambda a, b: Y[a:b]
    Y = bench_online._panel(c)
    return Y, lambda a, b: (smat.csr_matrix(Y[a:b]) if c['missing'] else Y[a:b])


def _kernel_times(path):
    """ms per robust call of the assim_robust_* kernels from the kernel-trace csv files under `path` (a profiler run of this script
    with one case); a call launches the prior kernel once, so its dispatches count the calls."""
    tot = {}
    for f in glob.glob(os.path.join(path, '**', '*kernel_trace.csv'), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                low = {key.lower(): v for key, v in row.items()}
                name = low.get('kernel_name', '')
                for key in ('assim_robust_part_kernel', 'assim_robust_solve_kernel', 'assim_robust_prior_kernel'):
                    if key in name:
                        ns, cnt = tot.get(key, (0, 0))
                        tot[key] = (ns + int(low['end_timestamp']) - int(low['start_timestamp']), cnt + 1)
    calls = tot.get('assim_robust_prior_kernel', (0, 0))[1]
    if not calls:
        raise SystemExit('no assim_robust_prior_kernel dispatch in the kernel traces under ' + path)
    return {key: dict(ms_per_call=ns * 1e-6 / calls, dispatches_per_call=cnt / calls) for key, (ns, cnt) in tot.items()}


def case(name, reps, kernel_csv=None):
    import numpy as np
    from trmf import synth
    from trmf.session import Session
    c = CASES[name]
    Y, block = _problem(c)
    T0 = c['T'] - (reps + 1) * STEPS
    model = synth.initial_model(block(0, T0), c['lags'], c['k'], seed=0, dtype=np.dtype(c['dtype']))
    plain, robust, sums, plain_sums = [], [], [], []
    with Session(block(0, T0), model, missing=c['missing'], log_norms=False, timing=0, **c['hyper']) as s:
        s.run(c['max_iter']).sync()
        desc = s.describe()
        for r in range(reps + 1):
            s.append_rows(block(T0 + r * STEPS, T0 + (r + 1) * STEPS))
            first = s.rows() - STEPS
            s.mark()
            t0 = time.perf_counter()
            one_step = s.assimilate(first)
            t1 = time.perf_counter()
            s.rewind()
            scale = float(np.sqrt(one_step['sq_err_before'] / max(one_step['entries'], 1)))
            t2 = time.perf_counter()
            out = s.assimilate_robust(first, C, SWEEPS, scale)
            t3 = time.perf_counter()
            plain.append((t1 - t0) * 1e3); robust.append((t3 - t2) * 1e3); sums.append(out); plain_sums.append(one_step)
    med = lambda v: float(np.median(v[1:]))
    size = np.dtype(c['dtype']).itemsize
    entries = float(np.mean([o['entries'] for o in sums[1:]]))
    model_bytes = SWEEPS * entries * (c['k'] + 2) * size
    res = dict(name=name, T=c['T'], n=c['n'], k=c['k'], nlag=len(c['lags']), dtype=c['dtype'], missing=c['missing'], block_rows=STEPS, reps=reps,
               sweeps=SWEEPS, c=C, session=desc,
               assimilate_ms_median=med(plain), assimilate_ms_min=float(min(plain[1:])),
               assimilate_robust_ms_median=med(robust), assimilate_robust_ms_min=float(min(robust[1:])),
               robust_over_plain=med(robust) / med(plain),
               launches_per_robust_call=2 * SWEEPS * STEPS + 2,             # part + solve per row and sweep, the first prior, the errors
               entries_per_block=entries, part_kernel_model_bytes=model_bytes,
               downweighted_share=[o['downweighted'] / max(o['entries'], 1) for o in sums[1:]],
               one_step_ahead_rmse=[float(np.sqrt(o['sq_err_before'] / max(o['entries'], 1))) for o in sums[1:]],
               rmse_after=[float(np.sqrt(o['sq_err_after'] / max(o['entries'], 1))) for o in sums[1:]],
               rmse_after_plain=[float(np.sqrt(o['sq_err_after'] / max(o['entries'], 1))) for o in plain_sums[1:]])
    if kernel_csv:
        kt = _kernel_times(kernel_csv)
        res['kernel_trace'] = kt
        part = kt.get('assim_robust_part_kernel')
        if part and part['ms_per_call'] > 0:
            res['part_kernel_bytes_per_s'] = model_bytes / (part['ms_per_call'] * 1e-3)
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
