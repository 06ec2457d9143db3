#!/usr/bin/env python3
"""Kernel time of the sparse lag-weight solve (theta_lasso_kernel) against the ridge solve it replaces (theta_solve_kernel), its
sweep counts over the ALS iterations, and iterations/s with the L1 penalty on and off.

    python scripts/bench_lag_lasso.py [--iters 12] [--reps 5] [--cases paper,c3] [--out profiles/lag_lasso.json]

Two child processes, one case after another in each:

  kernels   under `rocprofv3 --kernel-trace`: from one marked initial model (random Theta), `iters` ALS iterations (period_Lag = 2)
            with the ridge solve, then with lambdaLagL1 on, then with the refit as well; the session is synchronised after every
            Theta-solve to read its record (trmf_session_lag_stats).  The dispatches of theta_solve_kernel / theta_lasso_kernel are
            read from the trace in order: the first lasso solve starts from the random Theta, the later ones are warm-started.
  wall      not traced: run(iters) + sync from the marked model, L1 off and on alternating, `reps` times each after one warm-up.

lambdaLagL1 = 0.2 median_t |b_t|_inf at the factors of the ridge run (the rule of the tests' designed inputs).

Cases:

  paper     the paper scripts' shape: 26 304 x 370, fp64, k = 60, 48 lags {1..24} u {168..191}, missing = 0
  c3        config 3: 10 000 x 100 000, 1 % observed, fp32, k = 40, 16 lags"""
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

CASES = {'paper': ('c1p', False), 'c3': ('c3', True)}        # synth.CONFIGS entry, missing


def _problem(name):
    import numpy as np
    from trmf import synth
    cfg, missing = synth.CONFIGS[CASES[name][0]], CASES[name][1]
    p = synth.make(cfg)
    model = synth.initial_model(p['Y'], p['lag_set'], cfg['k'], seed=0, dtype=np.dtype(cfg['dtype']))
    return p, model, cfg.get('hyper', synth.HYPER), missing


def _rhs_inf(W, lags):
    """|b_t|_inf per latent dimension (fp64): b[a] = sum_{i >= midx} w[i] w[i - L_a]."""
    import numpy as np
    W = W.astype(np.float64)
    T, midx = W.shape[0], int(max(lags))
    return np.max(np.abs(np.stack([(W[midx:] * W[midx - int(l):T - int(l)]).sum(axis=0) for l in lags])), axis=0)


def _penalty(sess, model, lags, iters):
    import numpy as np
    sess.rewind().set_lag_penalty(0.0, False).run(iters).download()
    return 0.2 * float(np.median(_rhs_inf(model.W, lags)))


def inner_kernels(names, iters, meta_path):
    import numpy as np
    from trmf.session import Session
    meta = {'cases': []}
    for name in names:
        p, model, hyper, missing = _problem(name)
        lags = [int(v) for v in p['lag_set']]
        with Session(p['Y'], model, missing=missing, log_norms=False, timing=0, period_Lag=2, **hyper) as s:
            s.mark()
            l1 = _penalty(s, model, lags, iters)                       # iters / 2 ridge solves in the trace
            runs = {}
            for key, refit in (('lasso', False), ('lasso_refit', True)):
                s.rewind().set_lag_penalty(l1, refit)
                rec = []
                for _ in range(iters // 2):
                    s.run(2)
                    st = s.lag_stats()
                    rec.append(dict(sweeps_max=int(st['per_dim'][:, 0].max()), sweeps_median=float(np.median(st['per_dim'][:, 0])),
                                    nonzeros_median=float(np.median(st['per_dim'][:, 1])), capped=st['capped'], refit_skipped=st['refit_skipped']))
                runs[key] = rec
            desc = s.describe()
        meta['cases'].append(dict(name=name, T=int(model.m), n=int(model.n), k=int(model.k), nlag=len(lags), dtype=str(model.W.dtype),
                                  lambdaLagL1=l1, solves=iters // 2, records=runs, describe=desc))
    with open(meta_path, 'w') as fh:
        json.dump(meta, fh)


def inner_wall(names, iters, reps, meta_path):
    import numpy as np
    from trmf.session import Session
    meta = {'cases': []}
    for name in names:
        p, model, hyper, missing = _problem(name)
        lags = [int(v) for v in p['lag_set']]
        with Session(p['Y'], model, missing=missing, log_norms=False, timing=0, period_Lag=2, **hyper) as s:
            s.mark()
            l1 = _penalty(s, model, lags, iters)
            times = {0.0: [], l1: []}
            for _ in range(reps + 1):                                   # (first of each: warm-up)
                for w in (0.0, l1):
                    s.rewind().set_lag_penalty(w, False).sync()
                    t0 = time.perf_counter()
                    s.run(iters).sync()
                    times[w].append(time.perf_counter() - t0)
        off, on = np.array(times[0.0][1:]), np.array(times[l1][1:])
        meta['cases'].append(dict(name=name, iters=iters, reps=reps, iter_per_s_l1_off=float(iters / np.median(off)),
                                  iter_per_s_l1_on=float(iters / np.median(on)), ms_per_iteration_l1_off=float(np.median(off) / iters * 1e3),
                                  ms_per_iteration_l1_on=float(np.median(on) / iters * 1e3)))
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
    work = tempfile.mkdtemp(prefix='bench_lag_lasso_')
    me = os.path.abspath(__file__)
    kmeta, wmeta = os.path.join(work, 'kernels.json'), os.path.join(work, 'wall.json')
    common = ['--iters', str(args.iters), '--cases', args.cases]
    subprocess.run(['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', os.path.join(work, 'trace'), '-o', 'lag', '--',
                    sys.executable, me, '--inner', 'kernels', '--meta', kmeta] + common, check=True, timeout=1100)
    rows = _trace_rows(os.path.join(work, 'trace'))
    us = lambda key: [(e - s) / 1e3 for s, e, name in rows if key in name]
    # 'theta_solve_': theta_solve_kernel or theta_solve_reg_kernel<N>, one per ridge solve
    ridge, lasso, gram = us('theta_solve_'), us('theta_lasso_kernel'), us('theta_gram_kernel')
    result = {'device': 'MI355X', 'cases': []}
    rp = lp = gp = 0
    for c in json.load(open(kmeta))['cases']:
        n = c['solves']
        r = ridge[rp:rp + n]; rp += n
        a, b = lasso[lp:lp + n], lasso[lp + n:lp + 2 * n]; lp += 2 * n
        g = gram[gp:gp + 3 * n]; gp += 3 * n
        warm = lambda v: v[2:] if len(v) > 2 else v[-1:]               # solve i runs in iteration 2 (i + 1): iterations >= 6
        result['cases'].append(dict(c, theta_gram_kernel_us_median=float(np.median(g)),
                                    theta_solve_kernel_us_median=float(np.median(r)),
                                    theta_lasso_kernel_us=a, theta_lasso_refit_kernel_us=b,
                                    theta_lasso_first_solve_us=a[0], theta_lasso_warm_us_median=float(np.median(warm(a))),
                                    theta_lasso_refit_first_solve_us=b[0], theta_lasso_refit_warm_us_median=float(np.median(warm(b)))))
    subprocess.run([sys.executable, me, '--inner', 'wall', '--meta', wmeta, '--reps', str(args.reps)] + common, check=True, timeout=1100)
    by = {c['name']: c for c in result['cases']}
    for w in json.load(open(wmeta))['cases']:
        by[w['name']]['als_loop'] = {k: v for k, v in w.items() if k != 'name'}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cases', default='paper,c3')
    ap.add_argument('--out', default=None)
    ap.add_argument('--inner', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--meta', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    names = [x for x in args.cases.split(',') if x]
    if args.inner == 'kernels':
        inner_kernels(names, args.iters, args.meta)
    elif args.inner == 'wall':
        inner_wall(names, args.iters, args.reps, args.meta)
    else:
        outer(args)


if __name__ == '__main__':
    main()
