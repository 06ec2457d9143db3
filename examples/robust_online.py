#!/usr/bin/env python3
"""Online updates on a stream with spiked readings: the plain forward filter beside the Huber-weighted one, on the GPU.

    python examples/robust_online.py [--hours 168] [--spikes 0.03] [--size 40] [--c 3.0] [--sweeps 4]

A model is trained once on a clean history and its noise is fitted (`Session.fit_noise`: the residual scale per series).  Then
the stream is replayed in blocks of 24 timestamps in which a share of the readings is spiked by +-`size` residual scales, twice
from the same trained state: once absorbing every block with `Session.update(block)`, which trusts every value, once with
`Session.update(block, robust_c=c)`, which down-weights a cell whose residual lies beyond c scales and reports the weights.
Before each block both sessions forecast it; the error is taken against the UNSPIKED truth.  The cells with a weight below 1 are
the anomaly report: compared here with the cells that were really spiked."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'exp-trmf-nips16_amd'))
import trmf  # noqa: E402
from trmf.session import Session  # noqa: E402

LAGS = [1, 2, 3, 24]
STEP = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hours', type=int, default=168, help='timestamps to replay online (a multiple of 24)')
    ap.add_argument('--spikes', type=float, default=0.03, help='share of the new readings that is spiked')
    ap.add_argument('--size', type=float, default=40.0, help='size of a spike in residual scales')
    ap.add_argument('--c', type=float, default=3.0, help="Huber's threshold in residual scales")
    ap.add_argument('--sweeps', type=int, default=4)
    ap.add_argument('--rank', type=int, default=20)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    d = trmf.Model.syn_gen(2000, 200, args.rank, LAGS, seed=0, dtype=np.float32)
    clean = np.ascontiguousarray(d['Y'] + 0.5 * rng.randn(*d['Y'].shape).astype(np.float32))
    blocks = args.hours // STEP
    T0 = clean.shape[0] - blocks * STEP
    hyper = dict(lambdaI=0.5, lambdaAR=2.0, lambdaLag=0.5)
    sessions = {}
    for name in ('plain', 'robust'):
        model = trmf.Model.initialize(clean[:T0], LAGS, args.rank, seed=0)
        sessions[name] = Session(clean[:T0], model, missing=False, log_norms=False, timing=0, **hyper)
        sessions[name].run(args.iters).sync()
    sessions['robust'].fit_noise()
    scale = np.sqrt(sessions['robust'].noise()[0])
    print('residual scale per series: median {:.3f}'.format(float(np.median(scale))))
    err = {'plain': [], 'robust': []}
    hits = found = false_alarms = 0
    for b in range(blocks):
        lo = T0 + b * STEP
        truth = clean[lo:lo + STEP]
        spiked_cells = rng.rand(STEP, truth.shape[1]) < args.spikes
        seen = np.ascontiguousarray(truth + np.where(spiked_cells, args.size * scale * np.sign(rng.randn(*truth.shape)), 0.0).astype(np.float32))
        for name, sess in sessions.items():
            forecast = sess.forecast(STEP)
            err[name].append(np.abs(forecast - truth).sum() / np.abs(truth).sum())
        sessions['plain'].update(seen)
        # update(seen, robust_c=...) is append_rows + assimilate_robust; spelled out here to get the weights of the block as well
        # (dense storage: one per cell).  A weight below 1 = a flagged cell.
        sessions['robust'].append_rows(seen)
        sums, weights = sessions['robust'].assimilate_robust(lo, args.c, args.sweeps, return_weights=True)
        flagged = weights < 1
        hits += int(spiked_cells.sum()); found += int((flagged & spiked_cells).sum()); false_alarms += int((flagged & ~spiked_cells).sum())
        print('block {:2d}: forecast ND plain {:.4f} robust {:.4f}; {} of {} cells down-weighted, {} of {} spikes among them'.format(
            b, err['plain'][-1], err['robust'][-1], sums['downweighted'], sums['entries'], int((flagged & spiked_cells).sum()), int(spiked_cells.sum())))
    for sess in sessions.values():
        sess.close()
    print('mean forecast ND after the first block: plain {:.4f}, robust {:.4f}'.format(float(np.mean(err['plain'][1:])), float(np.mean(err['robust'][1:]))))
    print('spiked cells flagged: {} of {}; other cells flagged: {}'.format(found, hits, false_alarms))


if __name__ == '__main__':
    main()
