#!/usr/bin/env python3
"""Online updates when a share of the readings arrives late: ignoring the late cells beside revising them in, on the GPU.

    python examples/late_data_online.py [--hours 192] [--late 0.5] [--delay 12] [--rank 10]

Synthetic AR data with a known latent factor.  A model is trained once on a history.  Then the stream is replayed in blocks of
24 timestamps, twice from the same trained state.  In every block a share `--late` of the observed cells is held back: those
readings arrive `--delay` rows late, i.e. together with a later block.  One session ignores them (`Session.update(block)`: what a
feed without cell revisions can do short of re-creating the session); the other hands them over as they arrive,
`Session.update(block, revisions=(rows, cols, vals), smooth_back=4)`: the cells are inserted into the rows they belong to
(`Session.revise`) and the smoother's window reaches back to the first revised row, so that those rows of W are re-solved from
all the data now known.

Reported per block: the error of the last `delay + 24` latent rows against the known factor (compared through W H^T), and the
forecast RMSE of the NEXT block against the noise-free truth."""
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
    ap.add_argument('--late', type=float, default=0.5, help='share of the observed cells of a block that arrives late')
    ap.add_argument('--delay', type=int, default=12, help='rows by which a late reading is late (at most 24)')
    ap.add_argument('--rank', type=int, default=10)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    if not 0 < args.delay <= STEP:
        ap.error('--delay must lie in 1..24')
    rng = np.random.RandomState(0)
    d = trmf.Model.syn_gen(2000, 200, args.rank, LAGS, seed=0, noise=0.1, dtype=np.float32)
    signal = d['Y']                                                  # W* H*^T, noise-free
    seen = signal + 0.3 * rng.randn(*signal.shape).astype(np.float32)
    blocks = args.hours // STEP
    T0 = signal.shape[0] - (blocks + 1) * STEP                       # one more block is kept as the last forecast's truth
    observed = rng.rand(*signal.shape) < 0.3
    late = observed & (rng.rand(*signal.shape) < args.late)
    late[:T0] = False                                                # the history is complete
    Y = np.where(observed, seen, 0).astype(np.float32)                # zeros are missing (missing=True)
    on_time = np.where(late, 0, Y).astype(np.float32)
    hyper = dict(lambdaI=0.5, lambdaAR=20.0, lambdaLag=0.5)
    sessions = {}
    for name in ('late cells ignored', 'late cells revised in'):
        model = trmf.Model.initialize(Y[:T0], LAGS, args.rank, seed=0)
        sessions[name] = Session(smat.csr_matrix(Y[:T0]), model, missing=True, log_norms=False, timing=0, **hyper)
        sessions[name].run(args.iters).sync()
    span = args.delay + STEP
    latent, ahead = {n: [] for n in sessions}, {n: [] for n in sessions}
    for b in range(blocks):
        lo = T0 + b * STEP
        block = smat.csr_matrix(on_time[lo:lo + STEP])
        # what has arrived by now of the readings held back: those of rows lo - delay .. lo + STEP - delay - 1
        r, c = np.nonzero(late[max(lo - args.delay, T0):lo + STEP - args.delay])
        r = r + max(lo - args.delay, T0)
        due = r < lo                                                 # rows the session already holds (the rest would ride in a later call)
        # (a late reading of a row INSIDE this block simply joins the block)
        inside = smat.csr_matrix((Y[r[~due], c[~due]], (r[~due] - lo, c[~due])), shape=(STEP, Y.shape[1]), dtype=np.float32)
        line = []
        for name, sess in sessions.items():
            if 'revised' in name:
                sums = sess.update(block + inside, revisions=(r[due], c[due], Y[r[due], c[due]]), smooth_back=4)
            else:
                sums = sess.update(block, smooth_back=4)
            m = sess.download()
            hi = lo + STEP
            fitted = m.W[hi - span:hi].dot(m.H.T)
            latent[name].append(float(np.sqrt(np.mean((fitted - signal[hi - span:hi]) ** 2))))
            forecast = sess.forecast(STEP)
            ahead[name].append(float(np.sqrt(np.mean((forecast - signal[hi:hi + STEP]) ** 2))))
            extra = ''
            if 'revise' in sums:
                extra = ' ({} late cells inserted from row {}, {} rows smoothed)'.format(sums['revise']['inserted'], sums['revise']['first_row'], sums['smooth']['rows'])
            line.append('{}: last {} rows RMSE {:.4f}, next block {:.4f}{}'.format(name, span, latent[name][-1], ahead[name][-1], extra))
        print('block {:2d}: {}'.format(b, '; '.join(line)))
    for sess in sessions.values():
        sess.close()
    for name in sessions:
        print('{:>22}: mean RMSE of the last {} rows {:.4f}, of the next block\'s forecast {:.4f}'.format(
            name, span, float(np.mean(latent[name])), float(np.mean(ahead[name]))))


if __name__ == '__main__':
    main()
