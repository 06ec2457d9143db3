#!/usr/bin/env python3
"""Cost of the forecast uncertainty (Session.fit_noise / Session.forecast_dist) beside the point forecast and the F-solve of the
same build, and the empirical coverage of the rolling evaluation.

    python scripts/bench_uncertainty.py [--reps 10] [--rolls 3] [--cases paper,imp,c3] [--out profiles/forecast_interval.json]

Cases:

  paper     the paper scripts' shape: 26 304 x 370 dense, fp32, k = 60, the 48 weekly lags, trained with missing=False
  imp       the same panel with 80 % of the cells observed: k = 40, 16 lags, missing=True (21 000 entries per series)
  c3        config 3 (synth.CONFIGS['c3']): 10 000 x 100 000 sparse, 1 % observed, fp32, k = 40, 16 lags (kernels only)

Two runs, because a tracer charges every launch:

  kernels   under `rocprofv3 --kernel-trace`: reps + 1 calls of fit_noise and of forecast_dist (24 steps, scored) from a session
            that has run three iterations; the dispatches of the new kernels and of the F-solve kernel are read from the trace.
            noise_resid_kernel's achieved B_N / t, B_N = nnz (4 + s + k s) + n k s, stands next to the F-solve's B_F / t
            (trmf_session_fsolve_bytes over the traced F-solve kernel time): a stream without a factorisation
  wall      not traced: host wall time of fit_noise, of one forecast_dist call and of one forecast call (blocking calls, the
            upload of the truth included), and -- paper and imp -- the 7-window rolling_validate with and without intervals,
            whose IntervalMetrics (empirical coverage of the 90 % interval among them) are recorded as an observation

Nothing here is a target: the numbers are recorded."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'exp-trmf-nips16_amd'))

WEEK = list(range(1, 25)) + list(range(7 * 24, 8 * 24))
STEPS, WINDOWS, LEVEL = 24, 7, 0.9
CASES = {
    'paper': dict(T=26304, n=370, k=60, lags=WEEK, dtype='float32', missing=False, max_iter=10,
                  hyper=dict(lambdaI=0.5, lambdaAR=125, lambdaLag=2)),
    'imp': dict(T=26304, n=370, k=40, lags=list(range(1, 17)), dtype='float32', missing=True, observed=0.8, max_iter=10,
                hyper=dict(lambdaI=0.5, lambdaAR=50, lambdaLag=0.5)),
    'c3': dict(config='c3', max_iter=3, missing=True, hyper=dict(lambdaI=0.5, lambdaAR=50, lambdaLag=0.5)),
}
NEW_KERNELS = ('noise_resid_kernel', 'noise_innov_kernel', 'forecast_psi_kernel', 'forecast_dist_kernel')


def _panel(c):
    """A dense low-rank + AR panel of the case's shape with positive levels and observation noise (the data sets are not
    redistributable); with `observed` the unobserved cells are zeros, which rolling_validate(missing=True) reads as missing."""
    import numpy as np
    from trmf import synth
    rng = np.random.RandomState(0)
    X, F, _ = synth._latent_factors(rng, c['n'], c['T'], c['k'], c['lags'], 0.01)
    dt = np.dtype(c['dtype'])
    Y = X.astype(dt).dot(F.astype(dt).T)
    Y += (0.05 * rng.randn(*Y.shape)).astype(dt)
    level = rng.lognormal(1.0, 0.5, c['n']).astype(dt)
    Y *= level
    Y += 2 * level
    if c.get('observed'):
        Y[rng.rand(*Y.shape) >= c['observed']] = 0
    return np.ascontiguousarray(Y)


def _problem(c):
    """(training matrix without the last STEPS rows, lag set, k, truth of the last STEPS rows, dense panel or None)."""
    import numpy as np
    import scipy.sparse as smat
    from trmf import synth
    if 'config' in c:
        cfg = synth.CONFIGS[c['config']]
        p = synth.make(cfg, seed=0)
        Y = p['Y'].tocsr()
        T0 = Y.shape[0] - STEPS
        return Y[:T0], [int(v) for v in p['lag_set']], cfg['k'], np.ascontiguousarray(Y[T0:].toarray()), None
    Y = _panel(c)
    T0 = c['T'] - STEPS
    head = smat.csr_matrix(Y[:T0]) if c['missing'] else Y[:T0]
    return head, c['lags'], c['k'], np.ascontiguousarray(Y[T0:]), Y


def _session(c):
    from trmf import synth
    from trmf.session import Session
    head, lags, k, truth, panel = _problem(c)
    model = synth.initial_model(head, lags, k, seed=0, dtype=truth.dtype)
    s = Session(head, model, missing=c['missing'], log_norms=False, timing=1, **c['hyper'])
    s.run(3).sync()
    return s, head, lags, k, truth, panel


def inner_kernels(names, reps, meta_path):
    meta = {'cases': []}
    for name in names:
        c = CASES[name]
        print('[kernels] ' + name, file=sys.stderr, flush=True)
        s, head, lags, k, truth, _ = _session(c)
        with s:
            nnz = int(head.nnz) if hasattr(head, 'nnz') and c['missing'] else int(head.shape[0] * head.shape[1])
            for _ in range(reps + 1):                       # (first: warm-up)
                s.fit_noise()
                s.forecast_dist(STEPS, level=LEVEL, truth=truth)
            meta['cases'].append(dict(name=name, T=int(head.shape[0]), n=int(head.shape[1]), k=k, nlag=len(lags), reach=int(lags[-1]),
                                      s=truth.dtype.itemsize, missing=c['missing'], cells=nnz, calls=reps + 1, iterations=3,
                                      fsolve_bytes=float(s.fsolve_bytes()), session=s.describe()))
    with open(meta_path, 'w') as fh:
        json.dump(meta, fh)


def inner_wall(names, reps, rolls, meta_path):
    import numpy as np
    import trmf
    meta = {'cases': []}
    for name in names:
        c = CASES[name]
        print('[wall] ' + name, file=sys.stderr, flush=True)
        s, head, lags, k, truth, panel = _session(c)
        fit, dist, point = [], [], []
        with s:
            for _ in range(reps + 1):                       # (first: warm-up)
                t0 = time.perf_counter()
                stats = s.fit_noise()
                t1 = time.perf_counter()
                s.forecast_dist(STEPS, level=LEVEL, truth=truth)
                t2 = time.perf_counter()
                s.forecast(STEPS, truth=truth)
                t3 = time.perf_counter()
                fit.append((t1 - t0) * 1e3); dist.append((t2 - t1) * 1e3); point.append((t3 - t2) * 1e3)
        out = dict(name=name, fit_noise_ms_median=float(np.median(fit[1:])), forecast_dist_ms_median=float(np.median(dist[1:])),
                   forecast_ms_median=float(np.median(point[1:])), noise=stats)
        if panel is not None:
            kw = dict(k=k, window_size=STEPS, nr_windows=WINDOWS, max_iter=c['max_iter'], missing=c['missing'], threshold=None, seed=0,
                      forecast_on_device=True, **c['hyper'])
            walls = {False: [], True: []}
            iv = None
            for _ in range(rolls + 1):                      # (first of each: warm-up)
                for with_iv in (False, True):
                    t0 = time.perf_counter()
                    res = trmf.rolling_validate(panel, lags, interval_level=LEVEL if with_iv else None, **kw)
                    walls[with_iv].append(time.perf_counter() - t0)
                    if with_iv:
                        iv = res[1]
            out['rolling_validate'] = dict(windows=WINDOWS, max_iter=c['max_iter'], level=LEVEL,
                                           wall_s_median=float(np.median(walls[False][1:])),
                                           wall_s_with_intervals_median=float(np.median(walls[True][1:])),
                                           interval_metrics={key: float(v) for key, v in iv._asdict().items()})
        meta['cases'].append(out)
    with open(meta_path, 'w') as fh:
        json.dump(meta, fh)


def _trace_rows(d):
    out = []
    for path in glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                out.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    return sorted(out)


def outer(args):
    import numpy as np
    work = tempfile.mkdtemp(prefix='bench_uncertainty_')
    me = os.path.abspath(__file__)
    kmeta, wmeta = os.path.join(work, 'kernels.json'), os.path.join(work, 'wall.json')
    subprocess.run(['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', os.path.join(work, 'trace'), '-o', 'uncertainty', '--',
                    sys.executable, me, '--inner', 'kernels', '--meta', kmeta, '--reps', str(args.reps), '--cases', args.cases], check=True, timeout=1100)
    rows = _trace_rows(os.path.join(work, 'trace'))
    by_name = {key: [(s, e) for s, e, name in rows if key in name] for key in NEW_KERNELS}
    fsolve = [(s, e) for s, e, name in rows if 'fsolve_' in name and 'long' not in name]
    fsolve_long = [(s, e) for s, e, name in rows if ('fsolve_' in name and 'long' in name) or 'gram_part_kernel' in name]
    result = {'device': 'MI355X', 'steps': STEPS, 'level': LEVEL, 'cases': []}
    cases = json.load(open(kmeta))['cases']
    calls_before = 0
    lo = 0
    for c in cases:
        rec = dict(c)
        for key in NEW_KERNELS:                             # one launch of each per call; the first call is the warm-up
            span = by_name[key][calls_before + 1:calls_before + c['calls']]
            us = np.array([(e - s) / 1e3 for s, e in span])
            rec[key + '_us_median'] = float(np.median(us)) if len(us) else None
            rec[key + '_us_min'] = float(us.min()) if len(us) else None
        calls_before += c['calls']
        per_cell = (4 if c['missing'] else 0) + c['s'] + c['k'] * c['s']          # (the dense orientation carries no index)
        rec['noise_resid_bytes'] = c['cells'] * per_cell + c['n'] * c['k'] * c['s']
        if rec['noise_resid_kernel_us_median']:
            rec['noise_resid_TBps'] = rec['noise_resid_bytes'] / (rec['noise_resid_kernel_us_median'] * 1e-6) / 1e12
        # the F-solve kernel of the case's three iterations: the traced process runs the cases in order, so they are the ones
        # between the previous case's last forecast_dist_kernel and this case's
        hi = by_name['forecast_dist_kernel'][calls_before - 1][1]
        mine = [(s, e) for s, e in fsolve if lo < s < hi]
        split = [(s, e) for s, e in fsolve_long if lo < s < hi]
        lo = hi
        if mine and not split:
            us = np.array([(e - s) / 1e3 for s, e in mine[1:]])          # (the first iteration's launch: warm-up)
            rec['fsolve_kernel_us_median'] = float(np.median(us))
            rec['fsolve_TBps'] = rec['fsolve_bytes'] / (rec['fsolve_kernel_us_median'] * 1e-6) / 1e12
        else:
            rec['fsolve_kernel_us_median'] = None
            rec['fsolve_note'] = 'no single F-solve kernel to compare with (full observation, or the split path of long rows)'
        result['cases'].append(rec)
    subprocess.run([sys.executable, me, '--inner', 'wall', '--meta', wmeta, '--reps', str(args.reps), '--rolls', str(args.rolls),
                    '--cases', args.cases], check=True, timeout=1100)
    by = {c['name']: c for c in result['cases']}
    for w in json.load(open(wmeta))['cases']:
        by[w['name']].update({key: v for key, v in w.items() if key != 'name'})
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rolls', type=int, default=3)
    ap.add_argument('--cases', default='paper,imp,c3')
    ap.add_argument('--out', default=None)
    ap.add_argument('--inner', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--meta', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    names = [x for x in args.cases.split(',') if x]
    if args.inner == 'kernels':
        inner_kernels(names, args.reps, args.meta)
    elif args.inner == 'wall':
        inner_wall(names, args.reps, args.rolls, args.meta)
    else:
        outer(args)


if __name__ == '__main__':
    main()
