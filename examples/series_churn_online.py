#!/usr/bin/env python3
"""An online forecaster whose fleet changes: series join and leave a sliding window on one resident GPU session.

    python examples/series_churn_online.py [--window 300] [--ticks 480] [--block 4] [--rank 4] [--every 60] [--swap 3]

`Session.update(window=N)` keeps the TIME axis of a resident problem at a fixed size; `Session.change_series` does the same for the
SERIES axis.  Every `--every` rows the `--swap` longest-serving series are withdrawn and as many new ones are installed.  A new
series arrives with the little history it has -- the rows since its sensor was switched on, `--history` of them -- as a block over
the window's rows; its loadings are fitted on the device from the resident W (a cold-start ridge over its own entries), so it is
forecast from its first tick.  Only the block crosses PCIe; the session is never re-created.

The stream: a low-rank + autoregressive panel, half of the cells observed.  Two forecasters see the same blocks and the same
churn: new loadings fitted by the call (`fit=True`) and new loadings left at zero until the online loading update has seen enough
of the series (`fit=False`).  Both adapt their loadings online (`update(adapt=True)` with the statistics carried across every
churn).  Printed: the 4-step forecast RMSE over the series that joined during their first `--every` rows, over all other series,
and the series resident at the end."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as smat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'exp-trmf-nips16_amd'))
import trmf  # noqa: E402
from trmf.session import Session  # noqa: E402

LAGS = [1, 2, 5]
HYPER = dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5)


def stream(T, n, k, seed):
    """(clean values T x n, observed values with zeros for unobserved cells)."""
    rng = np.random.RandomState(seed)
    X = np.zeros((T, k))
    X[0] = rng.randn(k)
    for t in range(1, T):
        X[t] = 0.9 * X[t - 1] + 0.3 * rng.randn(k)
    clean = X.dot(rng.randn(n, k).T)
    seen = rng.rand(T, n) < 0.5
    noisy = (clean + 0.05 * rng.randn(T, n)).astype(np.float32)
    noisy[noisy == 0] = 1e-3
    return clean.astype(np.float32), np.where(seen, noisy, np.float32(0))


def replay(obs, clean, args, fit):
    N, block, steps = args.window, args.block, args.block
    fleet = list(range(args.series))                        # the series resident now, in the session's order
    joined = {}                                             # series -> the row it joined at
    nxt = args.series
    model = trmf.Model.initialize(smat.csr_matrix(obs[:N, fleet]), LAGS, args.rank, seed=0, dtype=np.float32)
    err_new, err_old = [], []
    with Session(smat.csr_matrix(obs[:N, fleet]), model, missing=True, log_norms=False, timing=0, **HYPER) as s:
        s.run(20).sync()
        s.init_series_stats(args.forget)
        for lo in range(N, N + args.ticks, block):
            s.update(smat.csr_matrix(obs[lo:lo + block, fleet]), adapt=True, window=N)
            now = lo + block                                # rows [now - N, now) are resident
            if (lo - N) % args.every == 0 and lo > N and nxt + args.swap <= obs.shape[1]:
                keep = np.ones(len(fleet), dtype=bool)
                keep[:args.swap] = False                    # the longest-serving series leave
                new = list(range(nxt, nxt + args.swap))
                hist = np.zeros((N, args.swap), dtype=np.float32)
                hist[N - args.history:] = obs[now - args.history:now, new]      # a new sensor has a short history
                sums = s.change_series(keep, smat.csr_matrix(hist), fit=fit)
                assert sums['stats_carried'] == fit and s.rows() == N
                if not fit:
                    s.init_series_stats(args.forget)        # (zero loadings: the statistics start again with the new fleet)
                fleet = [j for j, k in zip(fleet, keep) if k] + new
                joined.update({j: now for j in new})
                nxt += args.swap
            f = s.forecast(steps)
            truth = clean[now:now + steps][:, fleet]
            fresh = np.array([j in joined and now - joined[j] < args.every for j in fleet])
            e = (f[:truth.shape[0]] - truth) ** 2
            if fresh.any():
                err_new.append(e[:, fresh].mean())
            err_old.append(e[:, ~fresh].mean())
        return float(np.sqrt(np.mean(err_new))), float(np.sqrt(np.mean(err_old))), s.model.n, len(joined)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=int, default=300)
    ap.add_argument('--ticks', type=int, default=480, help='timestamps replayed online')
    ap.add_argument('--block', type=int, default=4)
    ap.add_argument('--rank', type=int, default=4)
    ap.add_argument('--series', type=int, default=30)
    ap.add_argument('--every', type=int, default=60, help='rows between two churns')
    ap.add_argument('--swap', type=int, default=3, help='series replaced per churn')
    ap.add_argument('--history', type=int, default=40, help='rows of history a new series arrives with')
    ap.add_argument('--forget', type=float, default=1.0)
    args = ap.parse_args()
    total = args.series + args.swap * (args.ticks // args.every + 1)
    clean, obs = stream(args.window + args.ticks + 2 * args.block, total, args.rank, seed=0)
    for name, fit in (('new loadings fitted by change_series', True), ('new loadings left at zero', False)):
        new, old, n, count = replay(obs, clean, args, fit)
        print('{:38s}: forecast RMSE {:.4f} over the {} series that joined (their first {} rows), {:.4f} over the others; {} series resident'.format(
            name, new, count, args.every, old, n))


if __name__ == '__main__':
    main()
