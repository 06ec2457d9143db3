#!/usr/bin/env python3
"""Wall time per online tick of a resident session that slides (fixed window) beside one that grows.

    python scripts/bench_slide.py [--ticks 300] [--case c3] [--modes window,grow,slide,append] [--label this] [--out profiles/online_slide.json]

Case: synth.CONFIGS['c3'] (100 000 series x 10 000 timestamps, 1 % observed, k = 40: ~1000 entries per timestamp).  Per mode one
session is created on all but the last `ticks` rows and trained for two iterations; then every tick hands over ONE new row:

    window   Session.update(row, window=T0)     slide (append + retire one row) + assimilate: the resident problem keeps T0 rows
    grow     Session.update(row)                append_rows + assimilate: the resident problem grows by a row per tick
    slide    trmf_session_slide(row, 1)         the storage step of `window` alone: the library call
    append   Session.append_rows(row)           the storage step of `grow` alone: the library call

(`Session.update` and `Session.slide` also rebuild the host model of the new size -- a copy of H, 16 MB at this shape, about a
millisecond -- which `window` and `grow` therefore both contain and `slide` and `append` do not.)

`append` uses nothing newer than trmf_session_append_rows, so the same script run with TRMF_CORELIB_DIR pointing at a build of the
parent commit records the parent's time for the same rows (`--modes append --label parent`; `--merge` adds the series to an
existing file).  Every call is blocking and ends in a stream synchronisation: host wall times of whole calls.  Both series are
recorded tick by tick; nothing here is a target or a gate."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'exp-trmf-nips16_amd'))


def run_mode(mode, p, cfg, ticks):
    import numpy as np
    from ctypes import byref
    from trmf import synth
    from trmf.rf_util import PyMatrix
    from trmf.session import Session
    Y = p['Y']
    T = Y.shape[0]
    T0 = T - ticks
    hyper = cfg.get('hyper', synth.HYPER)
    model = synth.initial_model(Y[:T0], p['lag_set'], cfg['k'], seed=0, dtype=np.dtype(cfg['dtype']))
    ms, rows, live = [], [], []
    with Session(Y[:T0], model, missing=True, log_norms=False, timing=0, **hyper) as s:
        s.run(2).sync()
        desc = s.describe()
        # config 3's synthetic panel learns lag weights that are explosive under its lambdaAR: hundreds of
        # filtered rows overflow W.  The times do not depend on the values, so the online part runs without the AR prior.
        s.set_lambdas(hyper['lambdaI'], 0.0, hyper['lambdaLag'])
        for t in range(T0, T):
            row = Y[t:t + 1]
            t0 = time.perf_counter()
            if mode == 'window':
                s.update(row, window=T0)
            elif mode == 'grow':
                s.update(row)
            elif mode == 'slide':
                block = PyMatrix(row, dtype=model.W.dtype)
                if s.lib.trmf_session_slide(s.handle, byref(block), 1, 0, None) < 0:
                    raise RuntimeError(s.lib.trmf_last_error().decode())
            else:
                s.append_rows(row)
            ms.append((time.perf_counter() - t0) * 1e3)
            rows.append(int(s.rows()))
            if hasattr(s, 'pool_live_bytes') and hasattr(s.lib, 'trmf_device_pool_live_bytes'):
                live.append(s.pool_live_bytes())
    med = lambda v: float(np.median(v))
    third = max(1, ticks // 3)
    return dict(mode=mode, ticks=ticks, rows_first=rows[0], rows_last=rows[-1], session=desc, ms_median=med(ms), ms_median_first_third=med(ms[:third]),
                ms_median_last_third=med(ms[-third:]), ms_all=[round(float(v), 4) for v in ms],
                pool_live_bytes_first=live[0] if live else None, pool_live_bytes_last=live[-1] if live else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=300)
    ap.add_argument('--case', default='c3')
    ap.add_argument('--modes', default='window,grow,slide,append')
    ap.add_argument('--label', default='this', help='which build the series belong to (this / parent)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--merge', action='store_true', help='add the series to the runs of an existing --out file')
    args = ap.parse_args()
    from trmf import synth
    cfg = synth.CONFIGS[args.case]
    p = synth.make(cfg, seed=0)
    p['Y'] = p['Y'].tocsr()
    result = {'device': 'MI355X', 'what': 'host wall times of whole blocking calls, one new row per tick; see scripts/bench_slide.py',
              'case': dict(name=args.case, T=int(p['Y'].shape[0]), n=int(p['Y'].shape[1]), k=cfg['k'], dtype=cfg['dtype'], nnz=int(p['Y'].nnz)), 'runs': []}
    if args.merge and args.out and os.path.exists(args.out):
        with open(args.out) as fh:
            result = json.load(fh)
    for mode in [m for m in args.modes.split(',') if m]:
        r = run_mode(mode, p, cfg, args.ticks)
        r['build'] = args.label
        result['runs'].append(r)
        print('{:>7s} [{}]: median {:.3f} ms per tick (first third {:.3f}, last third {:.3f}), rows {} -> {}'.format(
            mode, args.label, r['ms_median'], r['ms_median_first_third'], r['ms_median_last_third'], r['rows_first'], r['rows_last']), flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(result, indent=1) + '\n')


if __name__ == '__main__':
    main()
