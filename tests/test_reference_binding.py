"""CPU: a caller laid out like the reference's Python package -- <pkg>/trmf.py loading <pkg>/corelib/trmf_float{32,64}*.so by
glob, c_trmf_train with its 17-argument prototype, PyMatrix arguments (INTEGRATION.md route A) -- in a fresh process, on a scratch
copy of the package with THIS build's libraries in its corelib/ directory.  The caller is the package's own front end, which
mirrors the reference's wrapper name for name (the reference's sources are not part of this repository).  Without a GPU the call
must come back with the "no HIP device" diagnostic and untouched factors, which proves the loader glob, the symbol, the
17-argument prototype and the PyMatrix layout line up."""
import os
import shutil
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'exp-trmf-nips16_amd', 'trmf')

SCRIPT = textwrap.dedent('''
    import os, sys, numpy as np
    sys.path.insert(0, sys.argv[1])
    import trmf                                            # the scratch copy of the package
    from trmf import _corelib
    assert os.path.dirname(os.path.abspath(trmf.__file__)) == os.path.join(sys.argv[1], 'trmf')
    assert os.path.abspath(_corelib.corelib_path).startswith(os.path.join(sys.argv[1], 'trmf'))
    import scipy.sparse as smat
    Y = smat.random(60, 40, density=0.2, random_state=np.random.RandomState(0), format='csr', dtype=np.float32)
    for dtype in (np.float32, np.float64):
        m = trmf.Model.initialize(Y.astype(dtype), [1, 2, 5], 6, seed=0)
        W0, H0, T0 = m.W.copy(), m.H.copy(), m.lag_val.copy()
        trmf.train(Y.astype(dtype), m, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5, max_iter=3, missing=True, threads=2, verbose=0)
        assert np.array_equal(m.W, W0) and np.array_equal(m.H, H0) and np.array_equal(m.lag_val, T0)
    print('BINDING_OK')
''')


def test_reference_wrapper_binds_to_this_library(tmp_path):
    from trmf import session
    import numpy as np
    if session.lib_for(np.float32).trmf_device_count() > 0:
        pytest.skip('a GPU is present: the call would train; this test checks the no-device contract')
    pkg = tmp_path / 'trmf'
    shutil.copytree(PKG, pkg, ignore=shutil.ignore_patterns('__pycache__', 'corelib'))
    os.makedirs(str(pkg / 'corelib'))
    for name in ('trmf_float32.so', 'trmf_float64.so'):
        shutil.copy(os.path.join(PKG, 'corelib', name), str(pkg / 'corelib' / name))
    env = {k: v for k, v in os.environ.items() if k != 'TRMF_CORELIB_DIR'}
    res = subprocess.run([sys.executable, '-c', SCRIPT, str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert 'BINDING_OK' in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    assert res.stderr.count('no HIP device') >= 2          # one diagnostic per element-type library
