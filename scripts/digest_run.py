"""SHA-256 digests of the factors AND of every iteration's TRON line after a few ALS iterations at several shapes -- run with
TRMF_CORELIB_DIR pointing at two builds to check that a change is bit-neutral (usage: python scripts/digest_run.py).  The two fused
sparse cases are repeated under every form of the X-solve (persistent kernel, launch per step, wide tiles, unfused, two virtual ranks
with each transport): the forms share the scalar arithmetic of a TRON step (csrc/cg_kernels.hpp, tron_start .. tron_record)."""
import hashlib, os, struct, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'exp-trmf-nips16_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
os.environ.setdefault('TRMF_TEST', '1')
import numpy as np
from helpers import make_model
from trmf import session, synth
TRON = ('f', 'fnew', 'actred', 'prered', 'gnorm', 'cg_rnorm', 'cg_iter', 'accepted', 'delta')
def dig(model, st):
    h = hashlib.sha256()
    for a in (model.W, model.H, model.lag_val): h.update(np.ascontiguousarray(a).tobytes())
    for rec in st: h.update(struct.pack('<6d2id', *[rec[key] for key in TRON[:6]], rec['cg_iter'], rec['accepted'], rec['delta']))
    return h.hexdigest()[:16]
FORMS = [('', {}),
         ('TRMF_PERSIST=0', {'TRMF_PERSIST': '0'}),
         ('TRMF_TILE=wide', {'TRMF_TILE': 'wide'}),
         ('TRMF_TILE=wide TRMF_PERSIST=0', {'TRMF_TILE': 'wide', 'TRMF_PERSIST': '0'}),
         ('TRMF_NO_HV_TILE=1', {'TRMF_NO_HV_TILE': '1'}),
         ('TRMF_DEVICES=0,0 TRMF_CG=timeshard', {'TRMF_DEVICES': '0,0', 'TRMF_CG': 'timeshard'}),
         ('TRMF_DEVICES=0,0 TRMF_CG=p2p', {'TRMF_DEVICES': '0,0', 'TRMF_CG': 'p2p'}),
         ('TRMF_DEVICES=0,0 TRMF_CG=persist', {'TRMF_DEVICES': '0,0', 'TRMF_CG': 'persist', 'TRMF_PERSIST_TIMEOUT_MS': '120000'})]
seen = set()
def run(name, Y, m0, lag_set, missing, forms):
    for label, env in forms:
        for dtype in (np.float32, np.float64):
            model = make_model(m0.W.astype(dtype), m0.H.astype(dtype), np.asfortranarray(m0.lag_val.astype(dtype)), lag_set)
            os.environ.update(env)
            try:
                with session.Session(Y.astype(dtype), model, missing=missing, **synth.HYPER) as s:
                    s.run(5); st = s.stats(5); s.download()
            finally:
                for key in env: del os.environ[key]
            cg = [x['cg_iter'] for x in st]
            seen.update(cg)
            print('%-30s %-8s %s  f %s  cg %s%s' % (name, np.dtype(dtype).name, dig(model, st), repr(st[-1]['f']), cg, '  | ' + label if label else ''), flush=True)
cases = [('sparse k40 fused', dict(n=3000, T=1200, k=40, nlag=16, density=0.04), None, FORMS),
         ('sparse k16', dict(n=2000, T=2500, k=16, nlag=8, density=0.02), None, FORMS),
         ('sparse k64', dict(n=1500, T=700, k=64, nlag=6, density=0.05), None, FORMS[:1]),
         ('sparse long reach (unfused)', dict(n=500, T=1500, k=8, nlag=4, density=0.05), [1, 2, 24, 191], FORMS[:1]),
         ('sparse k80 (generic)', dict(n=600, T=500, k=80, nlag=4, density=0.2), None, FORMS[:1])]
for name, c, lags, forms in cases:
    p = synth.sparse_problem(n=c['n'], T=c['T'], k=c['k'], nlag=c['nlag'], density=c['density'], dtype=np.float64, seed=41)
    if lags: p['lag_set'] = np.array(lags, dtype=np.uint32)
    run(name, p['Y'], synth.initial_model(p['Y'], p['lag_set'], c['k'], seed=41), p['lag_set'], True, forms)
pd = synth.dense_problem(60, 1200, 6, [1, 2, 24, 168, 191], dtype=np.float64, seed=13)
run('dense full-observation', pd['Y'], synth.initial_model(pd['Y'], pd['lag_set'], 6, seed=7), pd['lag_set'], False, FORMS[:1])
# both exits of the CG have to be among the solves above: the tolerance (cg_iter below the cap of 20) and the cap
tol, cap = any(c < 20 for c in seen), 20 in seen
print('CG exits covered: on the tolerance %s, at the cap %s' % (tol, cap))
sys.exit(0 if tol and cap else 1)
