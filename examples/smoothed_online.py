#!/usr/bin/env python3
"""Online updates with sparsely observed tail rows: the forward filter beside filter + fixed-interval smoother, on the GPU.

    python examples/smoothed_online.py [--hours 192] [--back 48] [--sparse 0.02] [--rank 10]

Synthetic AR data with a known latent factor.  A model is trained once on a well-observed history.  Then the stream is replayed
in blocks of 24 timestamps, twice from the same trained state: once with `Session.update(block)` (the forward filter: a row sees
its own observations and the rows before it), once with `Session.update(block, smooth_back=back)`, which afterwards makes the
block and the `back` rows before it the joint minimiser of the model's objective, so that a row also takes from the rows after it.
In every block the first rows are observed on only a share `--sparse` of the series; the rest of the block is well observed.

Reported per block: the error of the block's latent rows against the known factor (compared through W H^T, which is unique
where W and H are not), and the forecast RMSE of the NEXT block, made from those rows, against the noise-free truth."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hours', type=int, default=192, help='timestamps to replay online (a multiple of 24)')
    ap.add_argument('--back', type=int, default=48, help='rows before each block that the smoother revisits')
    ap.add_argument('--sparse', type=float, default=0.02, help='observed share of the series in the sparsely observed rows')
    ap.add_argument('--thin', type=int, default=16, help='rows at the START of each block that are sparsely observed')
    ap.add_argument('--rank', type=int, default=10)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    d = trmf.Model.syn_gen(2000, 200, args.rank, LAGS, seed=0, noise=0.1, dtype=np.float32)
    signal = d['Y']                                                  # W* H*^T, noise-free
    seen = signal + 0.3 * rng.randn(*signal.shape).astype(np.float32)
    blocks = args.hours // STEP
    T0 = signal.shape[0] - (blocks + 1) * STEP                       # one more block is kept as the last forecast's truth
    observed = rng.rand(*signal.shape) < 0.6
    for b in range(blocks):
        lo = T0 + b * STEP
        observed[lo:lo + args.thin] = rng.rand(args.thin, signal.shape[1]) < args.sparse
    Y = np.where(observed, seen, 0).astype(np.float32)                # zeros are missing (missing=True)
    hyper = dict(lambdaI=0.5, lambdaAR=20.0, lambdaLag=0.5)
    sessions = {}
    for name in ('filter', 'filter + smoother'):
        model = trmf.Model.initialize(Y[:T0], LAGS, args.rank, seed=0)
        sessions[name] = Session(smat.csr_matrix(Y[:T0]), model, missing=True, log_norms=False, timing=0, **hyper)
        sessions[name].run(args.iters).sync()
    latent, ahead = {n: [] for n in sessions}, {n: [] for n in sessions}
    for b in range(blocks):
        lo = T0 + b * STEP
        block = smat.csr_matrix(Y[lo:lo + STEP])
        line = []
        for name, sess in sessions.items():
            sums = sess.update(block, smooth_back=args.back if 'smoother' in name else 0)
            m = sess.download()
            fitted = m.W[lo:lo + STEP].dot(m.H.T)
            latent[name].append(float(np.sqrt(np.mean((fitted - signal[lo:lo + STEP]) ** 2))))
            forecast = sess.forecast(STEP)
            ahead[name].append(float(np.sqrt(np.mean((forecast - signal[lo + STEP:lo + 2 * STEP]) ** 2))))
            extra = ''
            if 'smooth' in sums:
                sm = sums['smooth']
                extra = ' ({} rows, {} CG steps, J_win {:.1f} -> {:.1f})'.format(sm['rows'], sm['iterations'], sm['objective_before'], sm['objective_after'])
            line.append('{}: rows RMSE {:.4f}, next block {:.4f}{}'.format(name, latent[name][-1], ahead[name][-1], extra))
        print('block {:2d}: {}'.format(b, '; '.join(line)))
    for sess in sessions.values():
        sess.close()
    for name in sessions:
        print('{:>18}: mean RMSE of the block\'s rows {:.4f}, of the next block\'s forecast {:.4f}'.format(
            name, float(np.mean(latent[name])), float(np.mean(ahead[name]))))


if __name__ == '__main__':
    main()
