#!/usr/bin/env python3
"""Online updates on dirty data: the plain filter + smoother, the robust filter, and the robust filter + robust smoother, on the GPU.

    python examples/robust_smoothed_online.py [--hours 192] [--back 24] [--spikes 0.03] [--rank 10]

Synthetic AR data with a known latent factor.  A model is trained once on a clean history and its noise fitted.  Then the stream is
replayed in blocks of 24 timestamps, three times from the same trained state: `Session.update(block, smooth_back=back)` (every cell
weighted fully), `Session.update(block, robust_c=3)` (Huber weights, a filter: the tail rows are not the minimiser of the window's
objective) and `Session.update(block, robust_c=3, smooth_back=back, smooth_robust=True)`, which smooths the block and the `back`
rows before it on the Huber loss.  A share `--spikes` of the new cells is spiked by +-20 noise scales.

Reported per block: the error of the block's latent rows against the known factor (through W H^T) and the forecast RMSE of the NEXT
block, made from those rows, against the noise-free truth."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as smat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'exp-trmf-nips16_amd'))
import trmf  # noqa: E402
from trmf.session import Session  # noqa: E402

LAGS = [1, 2, 3, 24]
STEP = 24
MODES = {'smoother': dict(), 'robust filter': dict(robust_c=3.0), 'robust filter + robust smoother': dict(robust_c=3.0, smooth_robust=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hours', type=int, default=192, help='timestamps to replay online (a multiple of 24)')
    ap.add_argument('--back', type=int, default=24, help='rows before each block that the smoothers revisit')
    ap.add_argument('--spikes', type=float, default=0.03, help='share of the new cells that is spiked')
    ap.add_argument('--rank', type=int, default=10)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    d = trmf.Model.syn_gen(2000, 200, args.rank, LAGS, seed=0, noise=0.1, dtype=np.float32)
    signal = d['Y']                                                  # W* H*^T, noise-free
    sigma = 0.3
    seen = signal + sigma * rng.randn(*signal.shape).astype(np.float32)
    blocks = args.hours // STEP
    T0 = signal.shape[0] - (blocks + 1) * STEP                       # one more block is kept as the last forecast's truth
    observed = rng.rand(*signal.shape) < 0.6
    hit = observed & (rng.rand(*signal.shape) < args.spikes)
    hit[:T0] = False                                                 # the history is clean
    seen = seen + np.where(hit, 20 * sigma * np.sign(rng.randn(*signal.shape)), 0).astype(np.float32)
    Y = np.where(observed, seen, 0).astype(np.float32)                # zeros are missing (missing=True)
    hyper = dict(lambdaI=0.5, lambdaAR=20.0, lambdaLag=0.5)
    sessions = {}
    for name in MODES:
        model = trmf.Model.initialize(Y[:T0], LAGS, args.rank, seed=0)
        sessions[name] = Session(smat.csr_matrix(Y[:T0]), model, missing=True, log_norms=False, timing=0, **hyper)
        sessions[name].run(args.iters).sync()
        sessions[name].fit_noise()                                   # the residual scale of every series: the robust calls' default
    latent, ahead = {n: [] for n in sessions}, {n: [] for n in sessions}
    for b in range(blocks):
        lo = T0 + b * STEP
        block = smat.csr_matrix(Y[lo:lo + STEP])
        print('block {:2d}: {} spiked cells of {}'.format(b, int(hit[lo:lo + STEP].sum()), block.nnz))
        for name, sess in sessions.items():
            kw = dict(MODES[name])
            if name != 'robust filter':
                kw['smooth_back'] = args.back
            sums = sess.update(block, **kw)
            m = sess.download()
            fitted = m.W[lo:lo + STEP].dot(m.H.T)
            latent[name].append(float(np.sqrt(np.mean((fitted - signal[lo:lo + STEP]) ** 2))))
            forecast = sess.forecast(STEP)
            ahead[name].append(float(np.sqrt(np.mean((forecast - signal[lo + STEP:lo + 2 * STEP]) ** 2))))
            extra = ''
            if 'smooth' in sums:
                sm = sums['smooth']
                extra = ' ({} rows, {} CG steps'.format(sm['rows'], sm['iterations'])
                if 'downweighted' in sm:
                    extra += ' in {} sweeps, {} cells down-weighted'.format(sm['sweeps'], sm['downweighted'])
                extra += ', objective {:.1f} -> {:.1f})'.format(sm['objective_before'], sm['objective_after'])
            print('   {:>32}: rows RMSE {:.4f}, next block {:.4f}{}'.format(name, latent[name][-1], ahead[name][-1], extra))
    for sess in sessions.values():
        sess.close()
    for name in sessions:
        print('{:>32}: mean RMSE of the block\'s rows {:.4f}, of the next block\'s forecast {:.4f}'.format(
            name, float(np.mean(latent[name])), float(np.mean(ahead[name]))))


if __name__ == '__main__':
    main()
