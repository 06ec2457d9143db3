#!/usr/bin/env python3
"""Kernel time of an on-device forecast (trmf_session_forecast) against its byte model, and the wall time of a rolling
evaluation with the forecasts on the host and on the device.

    python scripts/bench_forecast.py [--reps 20] [--rolls 5] [--cases paper,c3] [--out profiles/forecast_eval.json]

Two child processes, one case after another in each:

  kernels   under `rocprofv3 --kernel-trace`: reps + 1 scored forecasts of 24 steps from a session that has run two iterations;
            the dispatches of forecast_rollout_kernel / forecast_score_kernel are read from the trace
  wall      not traced (a tracer charges every launch, and the two paths launch different numbers of kernels): a 7-window
            rolling_validate with forecast_on_device False and True, alternating, `rolls` times each after one warm-up call each

Cases:

  paper     the paper scripts' shape: 26 304 x 370, fp64, k = 60, the 48 lags of examples/rolling_forecast.py, transform on
  c3        config 3's shape: 10 000 timestamps x 100 000 series, fp32, k = 40, 16 lags, a dense panel trained with missing=False

Byte model of one call: the H rows n KP s, the rolled rows steps KP s, the truth steps n s, the forecast
steps n s if it is asked for (not here), the score table read and written 2 x 48 n."""
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
STEPS, WINDOWS = 24, 7
CASES = {
    'paper': dict(T=26304, n=370, k=60, lags=WEEK, dtype='float64', transform=True, max_iter=10,
                  hyper=dict(lambdaI=0.5, lambdaAR=125, lambdaLag=2)),
    'c3': dict(T=10000, n=100000, k=40, lags=list(range(1, 17)), dtype='float32', transform=None, max_iter=10,
               hyper=dict(lambdaI=0.5, lambdaAR=50, lambdaLag=0.5)),
}


def _panel(c):
    """A dense low-rank + AR panel of the case's shape with positive levels (the data sets are not redistributable)."""
    import numpy as np
    from trmf import synth
    rng = np.random.RandomState(0)
    X, F, _ = synth._latent_factors(rng, c['n'], c['T'], c['k'], c['lags'], 0.01)
    dt = np.dtype(c['dtype'])
    Y = X.astype(dt).dot(F.astype(dt).T)
    level = rng.lognormal(1.0, 0.5, c['n']).astype(dt)
    Y *= level
    Y += 2 * level
    return np.ascontiguousarray(Y)


def inner_kernels(names, reps, meta_path):
    import numpy as np
    from trmf import synth
    from trmf.model import NormalizedTransform
    from trmf.session import Session
    meta = {'cases': []}
    for name in names:
        c = CASES[name]
        Y = _panel(c)
        T0 = c['T'] - STEPS
        model = synth.initial_model(Y[:T0], c['lags'], c['k'], seed=0, dtype=Y.dtype)
        with Session(Y[:T0], model, missing=False, log_norms=False, timing=0, **c['hyper']) as s:
            if c['transform']:
                s.set_transform(NormalizedTransform(Y[:T0]))
            s.run(2).sync()
            truth = np.ascontiguousarray(Y[T0:])
            walls = []
            for _ in range(reps + 1):                       # (first: warm-up)
                t0 = time.perf_counter()
                s.forecast(STEPS, truth=truth, return_forecast=False)
                walls.append(time.perf_counter() - t0)
        meta['cases'].append(dict(name=name, T=c['T'], n=c['n'], k=c['k'], nlag=len(c['lags']), reach=c['lags'][-1], s=Y.dtype.itemsize,
                                  steps=STEPS, calls=reps + 1, call_wall_us_median=float(np.median(walls[1:]) * 1e6)))
        del Y
    with open(meta_path, 'w') as fh:
        json.dump(meta, fh)


def inner_wall(names, rolls, meta_path):
    import numpy as np
    import trmf
    meta = {'cases': []}
    for name in names:
        c = CASES[name]
        Y = _panel(c)
        kw = dict(k=c['k'], window_size=STEPS, nr_windows=WINDOWS, max_iter=c['max_iter'], missing=False, threshold=None,
                  transform=c['transform'], seed=0, **c['hyper'])
        times = {False: [], True: []}
        metrics = {}
        for r in range(rolls + 1):                          # (first of each: warm-up)
            for dev in (False, True):
                t0 = time.perf_counter()
                m = trmf.rolling_validate(Y, c['lags'], forecast_on_device=dev, **kw)
                times[dev].append(time.perf_counter() - t0)
                metrics[dev] = m._asdict()
        host, dev = np.array(times[False][1:]), np.array(times[True][1:])
        per_window = (host - dev) / WINDOWS * 1e3           # paired: the calls alternate
        meta['cases'].append(dict(name=name, rolls=rolls, windows=WINDOWS, max_iter=c['max_iter'],
                                  host_forecast_wall_s=host.tolist(), device_forecast_wall_s=dev.tolist(),
                                  host_forecast_wall_s_median=float(np.median(host)), device_forecast_wall_s_median=float(np.median(dev)),
                                  saved_per_window_ms_median=float(np.median(per_window)), saved_per_window_ms_min=float(per_window.min()),
                                  saved_per_window_ms_max=float(per_window.max()),
                                  metrics_host={k: float(v) for k, v in metrics[False].items()},
                                  metrics_device={k: float(v) for k, v in metrics[True].items()}))
        del Y
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
    work = tempfile.mkdtemp(prefix='bench_forecast_')
    me = os.path.abspath(__file__)
    kmeta, wmeta = os.path.join(work, 'kernels.json'), os.path.join(work, 'wall.json')
    subprocess.run(['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', os.path.join(work, 'trace'), '-o', 'forecast', '--',
                    sys.executable, me, '--inner', 'kernels', '--meta', kmeta, '--reps', str(args.reps), '--cases', args.cases], check=True, timeout=1100)
    rows = _trace_rows(os.path.join(work, 'trace'))
    roll = [(s, e) for s, e, name in rows if 'forecast_rollout_kernel' in name]
    score = [(s, e) for s, e, name in rows if 'forecast_score_kernel' in name]
    result = {'device': 'MI355X', 'steps': STEPS, 'cases': []}
    pos = 0
    for c in json.load(open(kmeta))['cases']:
        r, sc = roll[pos + 1:pos + c['calls']], score[pos + 1:pos + c['calls']]       # (first: warm-up)
        pos += c['calls']
        KP = (c['k'] + 15) // 16 * 16
        model = c['n'] * KP * c['s'] + c['steps'] * KP * c['s'] + c['steps'] * c['n'] * c['s'] + 2 * 48 * c['n']
        r_us, s_us = np.array([(e - s) / 1e3 for s, e in r]), np.array([(e - s) / 1e3 for s, e in sc])
        gap = np.array([(b[0] - a[0]) / 1e3 for a, b in zip(r, sc)])                # roll-out start -> score start
        both = float(np.median(r_us) + np.median(s_us))
        result['cases'].append(dict(c, rollout_kernel_us_median=float(np.median(r_us)), rollout_kernel_us_min=float(r_us.min()),
                                    score_kernel_us_median=float(np.median(s_us)), score_kernel_us_min=float(s_us.min()),
                                    launch_to_launch_us_median=float(np.median(gap)), model_bytes=model,
                                    model_us_at_8TBps=model / 8e12 * 1e6, score_effective_TBps=model / (float(np.median(s_us)) * 1e-6) / 1e12,
                                    model_fraction_of_kernel_time=(model / 8e12 * 1e6) / both))
    subprocess.run([sys.executable, me, '--inner', 'wall', '--meta', wmeta, '--rolls', str(args.rolls), '--cases', args.cases], check=True, timeout=1100)
    by = {c['name']: c for c in result['cases']}
    for w in json.load(open(wmeta))['cases']:
        by[w['name']]['rolling_validate'] = {k: v for k, v in w.items() if k != 'name'}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rolls', type=int, default=5)
    ap.add_argument('--cases', default='paper,c3')
    ap.add_argument('--out', default=None)
    ap.add_argument('--inner', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--meta', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    names = [x for x in args.cases.split(',') if x]
    if args.inner == 'kernels':
        inner_kernels(names, args.reps, args.meta)
    elif args.inner == 'wall':
        inner_wall(names, args.rolls, args.meta)
    else:
        outer(args)


if __name__ == '__main__':
    main()
