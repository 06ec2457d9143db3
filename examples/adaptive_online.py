#!/usr/bin/env python3
"""Online updates on a stream whose series loadings drift: frozen H beside H refitted online, on the GPU.

    python examples/adaptive_online.py [--steps 20] [--drift 1.0] [--forget 1.0,0.98,0.95] [--seeds 5]

Synthetic AR data (k = 4, 30 series, half the cells observed).  A model is trained once on a history with constant loadings;
after the training window the true loadings drift linearly.  The stream is then replayed in blocks of 10 timestamps from the
same trained state: once with `Session.update(block)`, which absorbs the block into new rows of W and keeps H as it was trained,
and once per forgetting factor with `Session.update(block, adapt=True, forget=gamma)`, which also refits every row of H from
the resident per-series statistics (`Session.adapt_series`: recursive least squares with forgetting, O(new data)).  Before each
block every session forecasts it; the RMSE is taken over all cells of the block, observed or not.  With `--drift 0` the two
agree: adapting does no harm where nothing moves."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as smat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'exp-trmf-nips16_amd'))
import trmf  # noqa: E402
from trmf.session import Session  # noqa: E402

LAGS = [1, 2, 3]
STEP, K, N, T0 = 10, 4, 30, 400


def stream(seed, steps, drift):
    """(truth (T x n), observed mask): AR latent rows, loadings H0 up to T0 and H0 + drift * (t - T0) / (steps * STEP) * D after."""
    rng = np.random.RandomState(1000 + seed)
    T = T0 + steps * STEP
    W = np.zeros((T, K))
    W[0] = rng.randn(K)
    for t in range(1, T):                                   # persistent factors: a 10-step forecast keeps 3/4 of the signal
        W[t] = 0.97 * W[t - 1] + 0.25 * rng.randn(K)
    H, D = rng.randn(N, K), rng.randn(N, K)
    ramp = np.clip((np.arange(T) - T0) / float(steps * STEP), 0, None)
    Y = W.dot(H.T) + drift * ramp[:, None] * W.dot(D.T) + 0.1 * rng.randn(T, N)
    return np.ascontiguousarray(Y.astype(np.float32)), rng.rand(T, N) < 0.5


def observed(Y, mask, lo, hi):
    return smat.csr_matrix(np.where(mask[lo:hi], Y[lo:hi], np.float32(0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='online blocks of 10 timestamps')
    ap.add_argument('--drift', type=float, default=1.0, help='size of the drift of the loadings over the stream (0: none)')
    ap.add_argument('--forget', default='1.0,0.98,0.95', help='forgetting factors to compare')
    ap.add_argument('--seeds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=30)
    args = ap.parse_args()
    gammas = [float(g) for g in args.forget.split(',') if g]
    names = ['frozen H'] + ['forget %g' % g for g in gammas]
    hyper = dict(lambdaI=0.5, lambdaAR=2.0, lambdaLag=0.5)
    sq = {name: 0.0 for name in names}
    cells = 0
    for seed in range(args.seeds):
        Y, mask = stream(seed, args.steps, args.drift)
        sessions = {}
        for name in names:
            model = trmf.Model.initialize(observed(Y, mask, 0, T0), LAGS, K, seed=0)
            sessions[name] = Session(observed(Y, mask, 0, T0), model, missing=True, log_norms=False, timing=0, **hyper)
            sessions[name].run(args.iters).sync()
        for b in range(args.steps):
            lo = T0 + b * STEP
            block = observed(Y, mask, lo, lo + STEP)
            for name, sess in sessions.items():
                sq[name] += float(((sess.forecast(STEP) - Y[lo:lo + STEP]) ** 2).sum())
                if name == 'frozen H':
                    sess.update(block)
                else:
                    sess.update(block, adapt=True, forget=gammas[names.index(name) - 1])
            cells += STEP * N
        for sess in sessions.values():
            sess.close()
    for name in names:
        print('{:>12s}: 10-step forecast RMSE {:.4f}'.format(name, float(np.sqrt(sq[name] / cells))))


if __name__ == '__main__':
    main()
