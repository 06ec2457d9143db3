#!/usr/bin/env python3
"""An online forecaster that runs indefinitely: a SLIDING window on one resident GPU session.

    python examples/sliding_online.py [--window 400] [--ticks 600] [--block 4] [--rank 4] [--forget 1.0]

`Session.update` alone only ever grows the resident problem: every tick costs a little more than the one before, device memory
grows without bound and the loading statistics carry rows that are arbitrarily old.  With `window=N` the append becomes a slide
-- the block's rows come in, the oldest rows beyond N leave, in one pass on the device -- so a tick costs the same after a
million ticks as after ten, and with `downdate_stats=True` the statistics behind `adapt=True` describe exactly the rows the window
holds (a rectangular window; with `forget < 1` and no downdate they are the usual exponentially forgotten history instead).

The stream: a low-rank + autoregressive panel whose loadings drift linearly after the training window, half of the cells observed.
Three forecasters see the same blocks: loadings frozen, loadings adapted on a growing session, loadings adapted on a sliding window
with the statistics downdated.  Printed: the 4-step forecast RMSE over all cells, the rows each session holds at the end and the
median time of a tick over the first and the last fifth of the stream."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as smat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'exp-trmf-nips16_amd'))
import trmf  # noqa: E402
from trmf.session import Session  # noqa: E402

LAGS = [1, 2, 5]
HYPER = dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5)


def stream(T, T0, n, k, seed):
    """(clean values T x n, observed sparse matrix): AR(1)-like factors, loadings drifting linearly after T0."""
    rng = np.random.RandomState(seed)
    X = np.zeros((T, k))
    X[0] = rng.randn(k)
    for t in range(1, T):
        X[t] = 0.9 * X[t - 1] + 0.3 * rng.randn(k)
    F0, F1 = rng.randn(n, k), rng.randn(n, k)
    drift = np.clip((np.arange(T) - T0) / float(T - T0), 0.0, 1.0)[:, None, None]
    clean = np.einsum('tk,tnk->tn', X, F0[None] + drift * (F1 - F0)[None])
    seen = rng.rand(T, n) < 0.5
    noisy = (clean + 0.05 * rng.randn(T, n)).astype(np.float32)
    noisy[noisy == 0] = 1e-3
    return clean.astype(np.float32), smat.csr_matrix(np.where(seen, noisy, np.float32(0)))


def replay(Y, clean, T0, block, rank, steps, **how):
    model = trmf.Model.initialize(Y[:T0], LAGS, rank, seed=0, dtype=np.float32)
    err, ms = [], []
    with Session(Y[:T0], model, missing=True, log_norms=False, timing=0, **HYPER) as s:
        s.run(20).sync()
        for lo in range(T0, Y.shape[0] - steps, block):
            t0 = time.perf_counter()
            s.update(Y[lo:lo + block], **how)
            ms.append((time.perf_counter() - t0) * 1e3)
            f = s.forecast(steps)
            err.append(((f - clean[lo + block:lo + block + steps][:f.shape[0]]) ** 2).mean())
        rows = s.rows()
    fifth = max(1, len(ms) // 5)
    return float(np.sqrt(np.mean(err))), rows, float(np.median(ms[:fifth])), float(np.median(ms[-fifth:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=int, default=400)
    ap.add_argument('--ticks', type=int, default=600, help='timestamps replayed online')
    ap.add_argument('--block', type=int, default=4)
    ap.add_argument('--rank', type=int, default=4)
    ap.add_argument('--series', type=int, default=30)
    ap.add_argument('--forget', type=float, default=1.0)
    args = ap.parse_args()
    T0 = args.window
    T = T0 + args.ticks + args.block
    clean, Y = stream(T, T0, args.series, args.rank, seed=0)
    cases = [('frozen loadings, growing session', dict()),
             ('adapted loadings, growing session', dict(adapt=True, forget=args.forget)),
             ('adapted loadings, window of %d rows' % args.window, dict(adapt=True, forget=args.forget, window=args.window, downdate_stats=True))]
    for name, how in cases:
        rmse, rows, first, last = replay(Y, clean, T0, args.block, args.rank, args.block, **how)
        print('{:42s}: forecast RMSE {:.4f}; {} rows resident at the end; tick {:.2f} ms at the start, {:.2f} ms at the end'.format(name, rmse, rows, first, last))


if __name__ == '__main__':
    main()
