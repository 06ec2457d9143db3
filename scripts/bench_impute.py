#!/usr/bin/env python3
"""Kernel time of held-out evaluation (trmf_session_eval_heldout) against its byte model, and one grid_impute step.

    python scripts/bench_impute.py [--reps 20] [--out profiles/impute_eval.json]

runs itself under `rocprofv3 --kernel-trace` (a child process) and reads the dispatches of heldout_eval_kernel /
heldout_reduce_kernel from the trace, case by case:

  imp       20 % of the 26 304 x 370 imputation panel held out (~1.95 M entries), k = 40, fp32
  c3        config 3's shape (100 000 x 10 000 timestamps, k = 40, fp32), 1 M uniform held-out entries
  c3zipf    the same count drawn with Zipf-like weights over series and timestamps (the `zipf` pattern)
  grid      at `imp`: one lambda step of grid_impute (rewind, set_lambdas, run(10), eval) against impute() from scratch (wall)

Byte model per entry: position + truth 8 + s, the prediction s when asked for, the gathered H row KP s
(from L2 / MALL: H is 71 KB at imp, 19 MB at config 3), plus the W row KP s once per timestamp run of the sorted set."""
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


def _zipf_cells(T, n, count, seed, alpha_items=0.8, alpha_time=0.6):
    import numpy as np
    rng = np.random.RandomState(seed)
    wi = (1.0 + np.arange(n)) ** -alpha_items
    wt = (1.0 + np.arange(T)) ** -alpha_time
    pi_, pt_ = rng.permutation(n), rng.permutation(T)
    ci, ct = np.cumsum(wi / wi.sum()), np.cumsum(wt / wt.sum())
    keys = np.zeros(0, dtype=np.int64)
    while keys.size < count:
        m = 2 * (count - keys.size)
        r = pt_[np.minimum(np.searchsorted(ct, rng.rand(m)), T - 1)]
        c = pi_[np.minimum(np.searchsorted(ci, rng.rand(m)), n - 1)]
        keys = np.unique(np.concatenate([keys, r.astype(np.int64) * n + c]))
    return np.sort(rng.choice(keys, count, replace=False))


def _cells(keys, n, T, dtype, seed):
    import numpy as np
    from trmf.impute import _cells_matrix
    rng = np.random.RandomState(seed)
    rows, cols = keys // n, keys % n
    return _cells_matrix(rng.randn(keys.size), rows, cols, (T, n), dtype), rows


def inner(reps, meta_path):
    import numpy as np
    from trmf import impute, synth
    from trmf.impute import training_matrix
    from trmf.session import Session
    meta = {'cases': []}
    dt = np.float32

    def evals(sess, name, held, rows, k, T, n):
        sess.set_heldout(held)
        sess.eval_heldout()                                   # warm-up (not counted)
        for _ in range(reps):
            sess.eval_heldout()
        meta['cases'].append(dict(name=name, entries=int(held.nnz), row_runs=int(np.count_nonzero(np.diff(rows)) + 1), k=k, T=T, n=n,
                                  s=4, evals=reps + 1))

    # imp: the panel, 80 % observed (training), the other 20 % held out
    cfg = synth.CONFIGS['imp']
    T, n, k = cfg['T'], cfg['n'], cfg['k']
    full = synth.imputation_problem(n, T, k, list(range(1, cfg['nlag'] + 1)), observed=1.0, dtype=dt, seed=0)['Y'].toarray()
    mask = np.random.RandomState(1).rand(T, n) < 0.8
    lags = list(range(1, cfg['nlag'] + 1))
    Ytr = training_matrix(full, mask, dt)
    keys = np.flatnonzero(~mask.ravel())
    held, rows = _cells(keys, n, T, dt, 2)
    held.data[:] = full.ravel()[keys]
    model = synth.initial_model(Ytr, lags, k, seed=0, dtype=dt)
    with Session(Ytr, model, missing=True, log_norms=False, timing=0, **synth.HYPER) as s:
        s.mark().run(2)
        evals(s, 'imp', held, rows, k, T, n)
        # one grid step (wall): rewind to the initial model, new weights, 10 iterations, evaluation -- the same model as impute() below
        t0 = time.perf_counter()
        s.rewind().set_lambdas(2.0, 5.0, 0.5).run(10)
        m = s.eval_heldout()
        meta['grid_step_s'] = time.perf_counter() - t0
        meta['grid_step_metrics'] = m._asdict()
    t0 = time.perf_counter()
    _, m2, _ = impute(full, mask, lags, k=k, lambdaI=2.0, lambdaAR=5.0, lambdaLag=0.5, max_iter=10, seed=0)
    meta['impute_scratch_s'] = time.perf_counter() - t0
    meta['impute_scratch_metrics'] = m2._asdict()

    # config 3's shape: uniform and Zipf-weighted held-out sets of 1 M entries
    cfg = synth.CONFIGS['c3']
    p = synth.make(cfg)
    T, n, k = cfg['T'], cfg['n'], cfg['k']
    model = synth.initial_model(p['Y'], p['lag_set'], k, seed=0, dtype=dt)
    with Session(p['Y'], model, missing=True, log_norms=False, timing=0, **synth.HYPER) as s:
        s.run(1)
        uni = np.unique(np.random.RandomState(3).randint(0, T * n, size=1030000).astype(np.int64))[:1000000]
        held, rows = _cells(uni, n, T, dt, 4)
        evals(s, 'c3', held, rows, k, T, n)
        held, rows = _cells(_zipf_cells(T, n, 1000000, 5), n, T, dt, 6)
        evals(s, 'c3zipf', held, rows, k, T, n)
    with open(meta_path, 'w') as fh:
        json.dump(meta, fh)


def _trace_rows(d):
    paths = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    out = []
    for path in paths:
        with open(path) as fh:
            for r in csv.DictReader(fh):
                out.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    return sorted(out)


def outer(args):
    import numpy as np
    work = tempfile.mkdtemp(prefix='bench_impute_')
    meta_path = os.path.join(work, 'meta.json')
    cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', os.path.join(work, 'trace'), '-o', 'impute', '--',
           sys.executable, os.path.abspath(__file__), '--inner', meta_path, '--reps', str(args.reps)]
    subprocess.run(cmd, check=True, timeout=1200)
    meta = json.load(open(meta_path))
    rows = _trace_rows(os.path.join(work, 'trace'))
    ev = [(e - s) / 1000.0 for s, e, name in rows if 'heldout_eval_kernel' in name]
    red = [(e - s) / 1000.0 for s, e, name in rows if 'heldout_reduce_kernel' in name]
    result = {'device': 'MI355X', 'cases': [], 'grid_step_s': meta['grid_step_s'], 'impute_scratch_s': meta['impute_scratch_s']}
    pos = 0
    for c in meta['cases']:
        seg, rseg = ev[pos + 1:pos + c['evals']], red[pos + 1:pos + c['evals']]     # (first: warm-up)
        pos += c['evals']
        KP = (c['k'] + 15) // 16 * 16
        s = c['s']
        b_entry = c['entries'] * (8 + s + KP * s)
        b_w = c['row_runs'] * KP * s
        b_hbm = c['entries'] * (8 + s) + min(c['row_runs'], c['T']) * KP * s      # positions, truths, W rows once
        med = float(np.median(seg))
        result['cases'].append(dict(c, eval_kernel_us_median=med, eval_kernel_us_min=float(np.min(seg)), reduce_kernel_us_median=float(np.median(rseg)),
                                    model_bytes_total=b_entry + b_w, model_bytes_hbm=b_hbm, gathered_H_bytes=c['entries'] * KP * s,
                                    effective_TBps_total=(b_entry + b_w) / (med * 1e-6) / 1e12, effective_TBps_hbm=b_hbm / (med * 1e-6) / 1e12))
    by = {c['name']: c for c in result['cases']}
    if 'c3' in by and 'c3zipf' in by:
        result['zipf_over_uniform'] = by['c3zipf']['eval_kernel_us_median'] / by['c3']['eval_kernel_us_median']
    result['grid_step_speedup_vs_scratch'] = meta['impute_scratch_s'] / meta['grid_step_s']
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--inner', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.inner:
        inner(args.reps, args.inner)
    else:
        outer(args)


if __name__ == '__main__':
    main()
