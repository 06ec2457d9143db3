#!/usr/bin/env python3
"""A deployed forecaster's loop -- forecast, observe, update -- on ONE resident GPU session, without retraining.

    python examples/online_forecast.py [--data series.npy] [--hours 168] [--iters 20] [--retrain-every 0]

The model is trained once on the history.  Then, for every block of 24 new timestamps: forecast the block, see what really
happened, and absorb it with `Session.update` (append the rows, then a forward filter over them: each new latent row is solved
from its own observations and the AR prior of the rows before it; H and the lag weights stay as they are).  `sq_err_before` of an
update is the one-step-ahead error of the block -- the number to watch in production; --retrain-every N runs a few ALS
iterations after every N-th block.  Every forecast comes with a 90 % interval (`Session.fit_noise` after the training and after
every update, `Session.forecast_dist`): a plug-in interval from in-sample residuals, so read its coverage before trusting its
width.  Without --data a synthetic low-rank + autoregressive panel is generated."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'exp-trmf-nips16_amd'))
import trmf  # noqa: E402
from trmf.session import Session  # noqa: E402

LAGS = list(range(1, 25)) + list(range(7 * 24, 8 * 24))              # one day back, and the same day a week before
STEP = 24
LEVEL = 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--data', help='.npy file, timestamps x series')
    ap.add_argument('--hours', type=int, default=168, help='timestamps to replay online (a multiple of 24)')
    ap.add_argument('--iters', type=int, default=20, help='ALS iterations of the initial training')
    ap.add_argument('--retrain-every', type=int, default=0, help='run 2 ALS iterations after every N-th update (0: never)')
    ap.add_argument('--rank', type=int, default=40)
    args = ap.parse_args()
    if args.data:
        Y = np.ascontiguousarray(np.load(args.data), dtype=np.float32)
    else:
        d = trmf.Model.syn_gen(4000, 200, args.rank, LAGS, seed=0, dtype=np.float32)
        level = np.random.RandomState(0).lognormal(1.0, 0.5, 200).astype(np.float32)
        Y = np.ascontiguousarray(d['Y'] * level + 2 * level)
    blocks = args.hours // STEP
    T0 = Y.shape[0] - blocks * STEP
    hyper = dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5)
    model = trmf.Model.initialize(Y[:T0], LAGS, args.rank, seed=0)
    with Session(Y[:T0], model, missing=False, log_norms=False, timing=0, **hyper) as sess:
        sess.run(args.iters).sync()
        sess.fit_noise()
        for b in range(blocks):
            lo = T0 + b * STEP
            truth = Y[lo:lo + STEP]
            forecast = sess.forecast(STEP, truth=truth)                  # scored into the resident per-series table as well
            _, low, high = sess.forecast_interval(STEP, level=LEVEL, truth=truth)       # the same forecast with its interval
            inside = np.mean((truth >= low) & (truth <= high))
            t0 = time.perf_counter()
            sums = sess.update(truth, iters=2 if args.retrain_every and (b + 1) % args.retrain_every == 0 else 0)
            ms = (time.perf_counter() - t0) * 1e3
            nd = np.abs(forecast - truth).sum() / np.abs(truth).sum()
            sess.fit_noise()                                             # the model has moved: refit the variances behind the next interval
            print('block {:3d}: forecast ND {:.4f}, {:.0f} % interval holds {:.1f} % (mean width {:.3g}); update {:.2f} ms, latent rmse {:.4f} -> {:.4f}'.format(
                b, nd, 100 * LEVEL, 100 * inside, float(np.mean(high - low)), ms,
                np.sqrt(sums['sq_err_before'] / sums['entries']), np.sqrt(sums['sq_err_after'] / sums['entries'])))
        print(sess.forecast_scores())
        print(sess.interval_scores(LEVEL))


if __name__ == '__main__':
    main()
