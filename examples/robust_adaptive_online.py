#!/usr/bin/env python3
"""Online updates on a spiked stream whose loadings drift: frozen H, H refitted unweighted and H refitted with Huber weights.

    python examples/robust_adaptive_online.py [--steps 20] [--drift 1.0] [--spikes 0.03] [--forget 0.98] [--seeds 5]

The stream of examples/adaptive_online.py (synthetic AR data, k = 4, 30 series, half the cells observed, loadings that drift after
the training window) with `--spikes` of the observed online cells hit by +-40 sigma.  All three sessions absorb a block with the
robust filter (`robust_c=3`), so a spiked cell is kept out of its row of W.  They differ in the loadings:

    frozen H       Session.update(block, robust_c=3)                                    H stays as trained
    plain adapt    Session.update(block, robust_c=3, adapt=True)                        the spike enters S_j, r_j, h_j at full weight
    robust adapt   Session.update(block, robust_c=3, adapt=True, adapt_robust=True)     Session.adapt_series_robust: Huber weights

Before each block every session forecasts it; the RMSE is taken against the CLEAN values over all cells of the block."""
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
SIGMA = 0.5                                                 # observation noise; a spike is +-40 sigma = 20, ten times the signal's spread


def stream(seed, steps, drift, spikes):
    """(clean truth (T x n), the observed values with spikes, observed mask)."""
    rng = np.random.RandomState(1000 + seed)
    T = T0 + steps * STEP
    W = np.zeros((T, K))
    W[0] = rng.randn(K)
    for t in range(1, T):                                   # persistent factors: a 10-step forecast keeps 3/4 of the signal
        W[t] = 0.97 * W[t - 1] + 0.25 * rng.randn(K)
    H, D = rng.randn(N, K), rng.randn(N, K)
    ramp = np.clip((np.arange(T) - T0) / float(steps * STEP), 0, None)
    Y = W.dot(H.T) + drift * ramp[:, None] * W.dot(D.T) + SIGMA * rng.randn(T, N)
    mask = rng.rand(T, N) < 0.5
    hit = mask & (rng.rand(T, N) < spikes) & (np.arange(T)[:, None] >= T0)
    seen = Y + np.where(hit, 40.0 * SIGMA * np.sign(rng.randn(T, N)), 0.0)
    return np.ascontiguousarray(Y.astype(np.float32)), np.ascontiguousarray(seen.astype(np.float32)), mask


def observed(Y, mask, lo, hi):
    return smat.csr_matrix(np.where(mask[lo:hi], Y[lo:hi], np.float32(0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='online blocks of 10 timestamps')
    ap.add_argument('--drift', type=float, default=1.0, help='size of the drift of the loadings over the stream (0: none)')
    ap.add_argument('--spikes', type=float, default=0.03, help='share of the observed online cells hit by +-40 sigma')
    ap.add_argument('--forget', type=float, default=0.98)
    ap.add_argument('--seeds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=30)
    args = ap.parse_args()
    modes = {'frozen H': {}, 'plain adapt': dict(adapt=True, forget=args.forget), 'robust adapt': dict(adapt=True, forget=args.forget, adapt_robust=True)}
    hyper = dict(lambdaI=0.5, lambdaAR=2.0, lambdaLag=0.5)
    sq = {name: 0.0 for name in modes}
    cells = 0
    for seed in range(args.seeds):
        Y, seen, mask = stream(seed, args.steps, args.drift, args.spikes)
        sessions = {}
        for name in modes:
            model = trmf.Model.initialize(observed(seen, mask, 0, T0), LAGS, K, seed=0)
            sessions[name] = Session(observed(seen, mask, 0, T0), model, missing=True, log_norms=False, timing=0, **hyper)
            sessions[name].run(args.iters).sync()
            sessions[name].fit_noise()                      # the scale of the Huber weights: the in-sample residuals
        for b in range(args.steps):
            lo = T0 + b * STEP
            block = observed(seen, mask, lo, lo + STEP)
            for name, sess in sessions.items():
                sq[name] += float(((sess.forecast(STEP) - Y[lo:lo + STEP]) ** 2).sum())
                sess.update(block, robust_c=3.0, **modes[name])
            cells += STEP * N
        for sess in sessions.values():
            sess.close()
    for name in modes:
        print('{:>12s}: 10-step forecast RMSE against the clean values {:.4f}'.format(name, float(np.sqrt(sq[name] / cells))))


if __name__ == '__main__':
    main()
