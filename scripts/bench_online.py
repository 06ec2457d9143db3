#!/usr/bin/env python3
"""Wall time of an online update (Session.update: append_rows + trmf_session_assimilate) beside retraining on the grown prefix
(append_rows + run(max_iter)) of the same build, and the rolling scores of rolling_validate(update='assimilate') beside
update='retrain'.

    python scripts/bench_online.py [--reps 10] [--cases paper,imp] [--out profiles/online_update.json]

Cases:

  paper     the paper scripts' shape: 26 304 x 370 dense, fp32, k = 60, the 48 weekly lags, trained with missing=False
  imp       the same panel with 80 % of the cells observed (synth.CONFIGS['imp']): k = 40, 16 lags, missing=True

Per case two sessions are trained alike on all but the last reps x 24 rows; then, block by block of 24 rows, one absorbs the block
with update(), the other with append_rows + run(max_iter).  Every call is blocking, so the times are host wall times of whole
calls (the upload of the block and append_rows' re-tuning included on both sides); `assimilate_ms` is the filter's own share.
Nothing here is a target: the numbers are recorded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'exp-trmf-nips16_amd'))

WEEK = list(range(1, 25)) + list(range(7 * 24, 8 * 24))
STEPS, WINDOWS = 24, 7
CASES = {
    'paper': dict(T=26304, n=370, k=60, lags=WEEK, dtype='float32', missing=False, max_iter=10,
                  hyper=dict(lambdaI=0.5, lambdaAR=125, lambdaLag=2)),
    'imp': dict(T=26304, n=370, k=40, lags=list(range(1, 17)), dtype='float32', missing=True, observed=0.8, max_iter=10,
                hyper=dict(lambdaI=0.5, lambdaAR=50, lambdaLag=0.5)),
}


def _panel(c):
    """A dense low-rank + AR panel of the case's shape with positive levels (the data sets are not redistributable); with
    `observed` the unobserved cells are zeros, which rolling_validate(missing=True) reads as missing."""
    import numpy as np
    from trmf import synth
    rng = np.random.RandomState(0)
    X, F, _ = synth._latent_factors(rng, c['n'], c['T'], c['k'], c['lags'], 0.01)
    dt = np.dtype(c['dtype'])
    Y = X.astype(dt).dot(F.astype(dt).T)
    level = rng.lognormal(1.0, 0.5, c['n']).astype(dt)
    Y *= level
    Y += 2 * level
    if c.get('observed'):
        Y[rng.rand(*Y.shape) >= c['observed']] = 0
    return np.ascontiguousarray(Y)


def _train(Y, c, rows):
    import scipy.sparse as smat
    from trmf import synth
    from trmf.session import Session
    head = smat.csr_matrix(Y[:rows]) if c['missing'] else Y[:rows]
    model = synth.initial_model(Y[:rows], c['lags'], c['k'], seed=0, dtype=Y.dtype)
    s = Session(head, model, missing=c['missing'], log_norms=False, timing=0, **c['hyper'])
    s.run(c['max_iter']).sync()
    return s


def case(name, reps):
    import numpy as np
    import scipy.sparse as smat
    import trmf
    c = CASES[name]
    Y = _panel(c)
    T0 = c['T'] - (reps + 1) * STEPS                        # (the first block of each side: warm-up)
    block = lambda r: (smat.csr_matrix(Y[T0 + r * STEPS:T0 + (r + 1) * STEPS]) if c['missing'] else Y[T0 + r * STEPS:T0 + (r + 1) * STEPS])
    upd, app, asm, ret, run_ms, sums = [], [], [], [], [], []
    with _train(Y, c, T0) as s:
        desc = s.describe()
        for r in range(reps + 1):
            b = block(r)
            t0 = time.perf_counter()
            s.append_rows(b)
            t1 = time.perf_counter()
            out = s.assimilate(s.rows() - STEPS)
            t2 = time.perf_counter()
            app.append((t1 - t0) * 1e3); asm.append((t2 - t1) * 1e3); upd.append((t2 - t0) * 1e3); sums.append(out)
    with _train(Y, c, T0) as s:
        for r in range(reps + 1):
            b = block(r)
            t0 = time.perf_counter()
            s.append_rows(b)
            t1 = time.perf_counter()
            s.run(c['max_iter']).sync()
            t2 = time.perf_counter()
            ret.append((t2 - t0) * 1e3); run_ms.append((t2 - t1) * 1e3)
    med = lambda v: float(np.median(v[1:]))
    kw = dict(k=c['k'], window_size=STEPS, nr_windows=WINDOWS, max_iter=c['max_iter'], missing=c['missing'], threshold=None, seed=0,
              forecast_on_device=not c['missing'], **c['hyper'])
    rolling = {}
    for mode in ('retrain', 'assimilate'):
        t0 = time.perf_counter()
        m = trmf.rolling_validate(Y, c['lags'], update=mode, **kw)
        rolling[mode] = dict(wall_s=time.perf_counter() - t0, **{key: float(v) for key, v in m._asdict().items()})
    return dict(name=name, T=c['T'], n=c['n'], k=c['k'], nlag=len(c['lags']), reach=c['lags'][-1], dtype=c['dtype'], missing=c['missing'],
                max_iter=c['max_iter'], block_rows=STEPS, reps=reps, session=desc,
                update_ms_median=med(upd), append_rows_ms_median=med(app), assimilate_ms_median=med(asm), assimilate_ms_min=float(min(asm[1:])),
                retrain_ms_median=med(ret), retrain_run_ms_median=med(run_ms),
                speedup_of_the_update=med(ret) / med(upd), speedup_without_append_rows=med(run_ms) / med(asm),
                one_step_ahead_rmse_of_the_blocks=[float(np.sqrt(o['sq_err_before'] / max(o['entries'], 1))) for o in sums[1:]],
                rmse_after_the_update=[float(np.sqrt(o['sq_err_after'] / max(o['entries'], 1))) for o in sums[1:]],
                rolling_validate=rolling)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cases', default='paper,imp')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    result = {'device': 'MI355X', 'cases': [case(name, args.reps) for name in args.cases.split(',') if name]}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
