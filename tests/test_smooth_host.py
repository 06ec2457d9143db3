"""CPU: the fixed-interval smoother on the host -- trmf.smooth_rows (the NumPy statement trmf_session_smooth is held to), the
PCG twin of the device tests, the front end's guards and the ABI's layout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as smat

import online_helpers as OH
import smooth_helpers as SH
from helpers import make_model, relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, 'include')
K = 7


def _gradient(d, W, lamI, lamAR, missing, first):
    """g_i of every window row in fp64, formed entry by entry from the definition (the head rows are W's own)."""
    H, theta, back = d['H'].astype(np.float64), d['theta'].astype(np.float64), d['lag_set'].astype(int)
    Yd = np.asarray(d['Y'].todense(), dtype=np.float64)
    stored = np.zeros(Yd.shape, dtype=bool)
    c = d['Y'].tocoo()
    stored[c.row, c.col] = True
    T, k = W.shape
    e = {i: W[i] - sum(theta[l] * W[i - back[l]] for l in range(len(back))) for i in range(first, T)}
    g = np.zeros((T - first, k))
    scale = 0.0
    for i in range(first, T):
        A = lamI * np.eye(k)
        b = np.zeros(k)
        for j in range(H.shape[0]):
            if stored[i, j] or not missing:
                A += np.outer(H[j], H[j])
                b += Yd[i, j] * H[j]
        a = e[i].copy()
        for l in range(len(back)):
            if i + back[l] < T:
                a -= theta[l] * e[i + back[l]]
        g[i - first] = A.dot(W[i]) - b + lamAR * a
        scale = max(scale, np.abs(b).max(), np.abs(A).max() * np.abs(W[i]).max())
    return g, scale


def _smooth(d, lamI, lamAR, first, missing, storage='sparse', dtype=np.float64):
    from trmf import smooth_rows
    return smooth_rows(d['W'].astype(dtype), d['H'].astype(dtype), d['lag_set'], d['theta'].astype(dtype),
                       SH.window_rows(d, first, dtype, missing, storage), first, lamI, lamAR, missing)


CASES = [(missing, storage) for missing in (True, False) for storage in ('sparse', 'dense')]


@pytest.mark.parametrize('first', SH.FIRSTS)
@pytest.mark.parametrize('lamI,lamAR', OH.LAMBDAS)
@pytest.mark.parametrize('missing,storage', CASES)
def test_smooth_rows_zeroes_the_gradient_of_every_window_row(missing, storage, lamI, lamAR, first):
    d = OH.inputs(K)
    W = _smooth(d, lamI, lamAR, first, missing, storage)
    assert np.array_equal(W[:first], d['W'][:first].astype(np.float64))             # earlier rows are not touched
    g, scale = _gradient(d, W, lamI, lamAR, missing, first)
    assert np.abs(g).max() <= 1e-10 * scale, (np.abs(g).max(), scale)
    # ... and it does not raise J_win above the filter's rows
    filtered = OH.twin(d, np.float64, lamI, lamAR, missing, first)
    Js, Jf = SH.objective_of(d, W, lamI, lamAR, first, missing), SH.objective_of(d, filtered, lamI, lamAR, first, missing)
    assert Js <= Jf * (1 + 1e-13), (Js, Jf)


@pytest.mark.parametrize('missing', [True, False])
def test_a_window_of_one_row_is_the_filters_row(missing):
    d = OH.inputs(K)
    for lamI, lamAR in OH.LAMBDAS:
        first = OH.T - 1
        assert relmax(_smooth(d, lamI, lamAR, first, missing)[first:], OH.twin(d, np.float64, lamI, lamAR, missing, first)[first:]) <= 1e-12


def test_lags_at_least_the_window_give_the_filter_on_every_row():
    d = OH.inputs(K, lags=(30, 40))
    for lamI, lamAR in OH.LAMBDAS:
        got, want = _smooth(d, lamI, lamAR, OH.FIRST, True), OH.twin(d, np.float64, lamI, lamAR, True, OH.FIRST)
        assert relmax(got[OH.FIRST:], want[OH.FIRST:]) <= 1e-12


def test_noise_free_ar_data_with_the_exact_rows_stays_fixed():
    """Y = W* H^T with W* following the AR model exactly and lambdaI = 0: the exact rows have a zero gradient."""
    from trmf import smooth_rows
    rng = np.random.RandomState(3)
    k, n, T0, Tn = 5, 30, 40, 12
    lags = np.array([1, 2, 5], dtype=np.uint32)
    theta = rng.randn(3, k)
    theta = theta / (np.abs(theta).sum(axis=0) + 0.1)
    model = make_model(rng.rand(T0, k), rng.rand(n, k), theta, lags)
    Wstar = model.latent_forecast(Tn)
    Ynew = Wstar[T0:].dot(model.H.T)
    for missing, Yrows in ((False, Ynew), (True, smat.csr_matrix(Ynew * (rng.rand(Tn, n) < 0.5)))):
        got = smooth_rows(Wstar, model.H, lags, model.lag_val, Yrows, T0, 0.0, 2.0, missing)
        assert relmax(got[T0:], Wstar[T0:]) <= 1e-12, missing
        start = np.vstack([model.W, np.zeros((Tn, k))])                           # ... and they are reached from anywhere
        assert relmax(smooth_rows(start, model.H, lags, model.lag_val, Yrows, T0, 0.0, 2.0, missing)[T0:], Wstar[T0:]) <= 1e-10, missing


def test_guards_raise_where_filter_rows_does():
    from trmf import filter_rows, smooth_rows
    d = OH.inputs(K)
    W64, H64, th64 = d['W'].astype(np.float64), d['H'].astype(np.float64), d['theta'].astype(np.float64)
    bad = [(np.array([0, 1, 2], dtype=np.uint32), d['Y'][OH.FIRST:], OH.FIRST, 0.5, 0.5, 'lag 0'),
           (d['lag_set'], d['Y'][4:], 4, 0.5, 0.5, 'largest lag'),
           (d['lag_set'], d['Y'][:0], OH.T + 1, 0.5, 0.5, 'outside'),
           (d['lag_set'], d['Y'][OH.FIRST + 1:], OH.FIRST, 0.5, 0.5, 'were expected'),
           (d['lag_set'], d['Y'][OH.FIRST:], OH.FIRST, 0.0, 0.0, 'row %d' % OH.EMPTY_ROW)]
    for lags, Yrows, first, lamI, lamAR, match in bad:
        for fn in (filter_rows, smooth_rows):
            with pytest.raises(ValueError, match=match):
                fn(W64, H64, lags, th64, Yrows, first, lamI, lamAR, True)
    assert np.array_equal(smooth_rows(W64, H64, d['lag_set'], th64, d['Y'][OH.T:], OH.T, 0.5, 0.5, True), W64)     # nothing to do


def test_the_twin_converges_on_every_input_of_the_device_tests():
    """What keeps the device gate (8 x the twin's own distance, steps within 2 of the twin's) meaningful: the twin itself converges
    within the tests' max_iter everywhere, and in fp64 it reaches the direct solve."""
    worst = {}
    for name, kw in SH.gpu_inputs():
        want, dist, steps, converged = SH.yardstick(**kw)
        assert converged and steps < SH.MAX_ITER, (name, kw, steps)
        assert np.isfinite(dist) and dist > 0, (name, kw, dist)
        key = kw['dtype'].name
        worst[key] = max(worst.get(key, (0.0, 0)), (dist, steps))
        assert dist <= (1e-2 if kw['dtype'] == np.float32 else 1e-6), (name, kw, dist)      # loose on purpose: a twin that solved another system would be off by O(1)
    print('twin distance from the direct fp64 solve, worst (distance, steps):', worst)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_model_assimilate_smooth_back_is_filter_then_smoother(dtype):
    from trmf import filter_rows, smooth_rows
    d = OH.inputs(K)
    lamI, lamAR = OH.LAMBDAS[1]
    Y = d['Y'].astype(dtype)
    base = make_model(d['W'][:OH.FIRST].astype(dtype), d['H'].astype(dtype), d['theta'].astype(dtype), d['lag_set'])
    grown = base.assimilate(Y[OH.FIRST:], lamI, lamAR, smooth_back=8, Yback=Y[OH.FIRST - 8:OH.FIRST])
    W = np.vstack([base.W, np.zeros((OH.TN, K), dtype=dtype)])
    W = filter_rows(W, base.H, base.lag_set, base.lag_val, Y[OH.FIRST:], OH.FIRST, lamI, lamAR, True)
    W = smooth_rows(W, base.H, base.lag_set, base.lag_val, Y[OH.FIRST - 8:], OH.FIRST - 8, lamI, lamAR, True)
    assert np.array_equal(grown.W, W) and not np.array_equal(grown.W[OH.FIRST - 8:OH.FIRST], base.W[OH.FIRST - 8:])
    assert np.array_equal(base.assimilate(Y[OH.FIRST:], lamI, lamAR).W, base.assimilate(Y[OH.FIRST:], lamI, lamAR, smooth_back=0).W)
    with pytest.raises(ValueError, match='Yback'):
        base.assimilate(Y[OH.FIRST:], lamI, lamAR, smooth_back=8)
    with pytest.raises(ValueError, match='Huber'):
        base.assimilate(Y[OH.FIRST:], lamI, lamAR, smooth_back=8, Yback=Y[OH.FIRST - 8:OH.FIRST], robust_c=3.0, scale=1.0)


def test_update_refuses_smooth_back_with_robust_c_before_anything_is_touched():
    from trmf.session import Session
    s = Session.__new__(Session)                             # no device: the refusal comes before the first native call
    s.handle = None
    with pytest.raises(ValueError, match='Huber'):
        s.update(None, robust_c=3.0, smooth_back=8)
    with pytest.raises(ValueError, match='negative'):
        s.update(None, smooth_back=-1)
    with pytest.raises(ValueError, match='stale'):
        s.update(None, adapt=True, smooth_back=8)


def test_rolling_validate_still_refuses_update_smooth_and_says_where_smooth_back_applies():
    import trmf
    Y = np.abs(np.random.RandomState(0).randn(120, 6)) + 0.5
    kw = dict(k=3, window_size=8, nr_windows=3, max_iter=2)
    with pytest.raises(ValueError, match='retrain'):
        trmf.rolling_validate(Y, [1, 2, 5], update='smooth', **kw)
    with pytest.raises(ValueError, match="update='assimilate'"):
        trmf.rolling_validate(Y, [1, 2, 5], smooth_back=8, **kw)
    with pytest.raises(ValueError, match='Huber'):
        trmf.rolling_validate(Y, [1, 2, 5], update='assimilate', robust_c=3.0, smooth_back=8, **kw)
    with pytest.raises(ValueError, match='Huber'):
        trmf.grid_search(Y, [1, 2, 5], {'lambdaI': [0.5]}, update='assimilate', robust_c=3.0, smooth_back=8, **kw)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_libraries_export_the_smooth_entry_point(dtype):
    from trmf import session
    lib = session.lib_for(dtype)
    assert hasattr(lib, 'trmf_session_smooth')
    assert lib.trmf_session_smooth.restype is ctypes.c_int32 and len(lib.trmf_session_smooth.argtypes) == 6


def test_smooth_sums_layout_matches_header(tmp_path):
    from trmf.session import TrmfSmoothSums
    names = [name for name, _ in TrmfSmoothSums._fields_]
    assert names == ['rows', 'entries', 'iterations', 'converged', 'residual', 'sq_err_before', 'sq_err_after', 'objective_before', 'objective_after']
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trmf_abi.h"\n'
                   'int main(void) { printf("%zu", sizeof(TrmfSmoothSums));\n'
                   + ''.join(' printf(" %%zu", offsetof(TrmfSmoothSums, %s));\n' % name for name in names)
                   + ' printf("\\n"); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run(['cc', '-I', HEADER_DIR, str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(TrmfSmoothSums)] + [getattr(TrmfSmoothSums, name).offset for name in names]
