#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the REAL reference.

Runs only in the build container: needs oracle/_ref/ (built by `make -C oracle ref` from the
reference sources where they lie under /root/reference).  The reference ships no tests or golden
vectors of its own, so every fixture here is captured from its c_trmf_train:
inputs (sparse Y, lag_set, initial W/H/Theta, hyper-parameters) and outputs (final W/H/Theta, the
per-half-step norms it prints on stderr at verbose>=1, and the CG step count / objective of the TRON
line it prints on stdout at verbose>=2).

    python tests/golden/make_golden.py             # rewrites tests/golden/*.npz
    python tests/golden/make_golden.py ref_build   # rewrites tests/golden/ref_build/*.npz only
"""
import os
import re
import sys
import tempfile

import numpy as np
import scipy.sparse as smat

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'exp-trmf-nips16_amd'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import oracle_py as O          # noqa: E402
from trmf import synth         # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
LAST_TRON = None      # act, pre, delta, |g|, CG residual norm of every TRON line of the last reference run (rf_tron.h:219)


class capture_fds(object):
    """Capture what C code writes to fd 1 and fd 2."""

    def __enter__(self):
        sys.stdout.flush(); sys.stderr.flush()
        self.saved = [os.dup(1), os.dup(2)]
        self.tmp = [tempfile.TemporaryFile(), tempfile.TemporaryFile()]
        os.dup2(self.tmp[0].fileno(), 1); os.dup2(self.tmp[1].fileno(), 2)
        return self

    def __exit__(self, *exc):
        import ctypes
        ctypes.CDLL(None).fflush(None)
        os.dup2(self.saved[0], 1); os.dup2(self.saved[1], 2)
        self.out, self.err = [], []
        for t, dst in zip(self.tmp, (self.out, self.err)):
            t.seek(0); dst.extend(t.read().decode().splitlines()); t.close()
        for fd in self.saved:
            os.close(fd)


def run_reference(Y, lag_set, W0, H0, Th0, hyper, max_iter, periods=(1, 1, 2), missing=True):
    W, H, Th = W0.copy(), H0.copy(), np.asfortranarray(Th0.copy())
    with capture_fds() as cap:
        O.train_ref(Y, lag_set, W, H, Th, hyper, max_iter=max_iter, periods=periods, threads=4, missing=missing, verbose=2)
    normF = np.full(max_iter, -1.0); normX = np.full(max_iter, -1.0); normLV = np.full(max_iter, -1.0)
    for line in cap.err:
        m = re.match(r'>> iter (\d+) (F|X|LV) (\S+)$', line.strip())
        if m:
            {'F': normF, 'X': normX, 'LV': normLV}[m.group(2)][int(m.group(1)) - 1] = float(m.group(3))
    cg, fx, tron = [], [], []
    for line in cap.out:
        m = re.match(r'iter\s+\d+ act (\S+) pre (\S+) delta (\S+) f (\S+) \|g\| (\S+) CG\s+(\d+) \|g\| (\S+)', line.strip())
        if m:
            fx.append(float(m.group(4))); cg.append(int(m.group(6)))
            tron.append([float(m.group(i)) for i in (1, 2, 3, 5, 7)])          # act, pre, delta, |g|, CG residual norm
    global LAST_TRON
    LAST_TRON = np.array(tron)
    return W, H, Th, normF, normX, normLV, np.array(cg, dtype=np.int32), np.array(fx)


def make_full_case(name, n, T, k, lag_set, dtype, max_iter, seed=0, hyper=None, sparse_density=None, order='C'):
    """missing=0 (full-observation path, trmf.cpp:155-215,299-351): dense Y, or sparse Y whose zeros count."""
    hyper = dict(hyper or synth.HYPER)
    from trmf import Model
    lag_set = np.array(sorted(lag_set), dtype=np.uint32)
    d = Model.syn_gen(T, n, k, lag_set, seed=seed, dtype=dtype)
    Yd = d['Y'] + np.asarray(0.05 * np.random.RandomState(seed).randn(T, n), dtype=dtype)
    if sparse_density is not None:
        mask = np.random.RandomState(seed + 1).rand(T, n) < sparse_density
        Y = smat.csr_matrix(np.where(mask, Yd, 0).astype(dtype)); Y.sort_indices()
    else:
        Y = np.asarray(Yd, dtype=dtype, order=order)
    model = synth.initial_model(Y, lag_set, k, seed=seed, dtype=dtype)
    W0, H0, Th0 = model.W.copy(), model.H.copy(), np.asfortranarray(model.lag_val.copy())
    W, H, Th, nF, nX, nLV, cg, fx = run_reference(Y, lag_set, W0, H0, Th0, hyper, max_iter, missing=False)
    path = os.path.join(OUT, name + '.npz')
    common = dict(shape=np.array([T, n]), lag_set=lag_set, W0=W0, H0=H0, Th0=Th0, W=W, H=H, Th=Th,
                  normF=nF, normX=nX, normLV=nLV, cg_iter=cg, f_x=fx, tron=LAST_TRON, objective=np.array(np.nan), missing=np.array(0),
                  lambdaI=hyper['lambdaI'], lambdaAR=hyper['lambdaAR'], lambdaLag=hyper['lambdaLag'], max_iter=np.array(max_iter))
    if sparse_density is not None:
        np.savez_compressed(path, Y_indptr=Y.indptr.astype(np.int64), Y_indices=Y.indices.astype(np.int32), Y_data=Y.data, **common)
    else:
        np.savez_compressed(path, Y_dense=Y, Y_order=np.array(order), **common)
    print('{:>14s}: T={} n={} k={} full {} {} iters={} cg={} ({} KB)'.format(
        name, T, n, k, 'sparse' if sparse_density is not None else 'dense-' + order, np.dtype(dtype).name, max_iter,
        cg.tolist(), os.path.getsize(path) // 1024))


def make_case(name, n, T, k, lag_set, density, dtype, max_iter, seed=0, hyper=None, drop_rows=(), drop_cols=()):
    hyper = dict(hyper or synth.HYPER)
    prob = synth.sparse_problem(n, T, k, 3, density, dtype=dtype, seed=seed)   # nlag only shapes the data
    Y = prob['Y'].tolil()
    for r in drop_rows:
        Y[r, :] = 0
    for c in drop_cols:
        Y[:, c] = 0
    Y = smat.csr_matrix(Y); Y.eliminate_zeros(); Y.sort_indices()
    lag_set = np.array(sorted(lag_set), dtype=np.uint32)
    model = synth.initial_model(Y, lag_set, k, seed=seed)
    W0, H0, Th0 = model.W.copy(), model.H.copy(), np.asfortranarray(model.lag_val.copy())
    W, H, Th, nF, nX, nLV, cg, fx = run_reference(Y, lag_set, W0, H0, Th0, hyper, max_iter)
    J = O.objective(Y, lag_set, W, H, Th, hyper)
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(
        path, Y_indptr=Y.indptr.astype(np.int64), Y_indices=Y.indices.astype(np.int32), Y_data=Y.data,
        shape=np.array([T, n]), lag_set=lag_set, W0=W0, H0=H0, Th0=Th0, W=W, H=H, Th=Th,
        normF=nF, normX=nX, normLV=nLV, cg_iter=cg, f_x=fx, tron=LAST_TRON, objective=np.array(J),
        lambdaI=hyper['lambdaI'], lambdaAR=hyper['lambdaAR'], lambdaLag=hyper['lambdaLag'],
        max_iter=np.array(max_iter))
    print('{:>14s}: T={} n={} k={} nnz={} {} iters={} cg={} J={:.6g} ({} KB)'.format(
        name, T, n, k, Y.nnz, np.dtype(dtype).name, max_iter, cg.tolist(), J, os.path.getsize(path) // 1024))


def make_cold_case(name, dtype, n=90, T=120, k=6, lag_set=(1, 2, 5), density=0.2, max_iter=4, seed=9):
    """warm_start = 0 (quirk Q1): the reference trains a PRIVATE model drawn from its own generator (mt19937 seeded 0,
    trmf.cpp:547-558) and leaves the caller's arrays alone; what a caller can observe of that run are the ">> iter" norm
    lines under verbose.  Captured: those lines, and that the caller's arrays came back unchanged."""
    prob = synth.sparse_problem(n, T, k, 3, density, dtype=dtype, seed=seed)
    Y = smat.csr_matrix(prob['Y']); Y.sort_indices()
    lag_set = np.array(sorted(lag_set), dtype=np.uint32)
    model = synth.initial_model(Y, lag_set, k, seed=seed, dtype=dtype)
    W0, H0, Th0 = model.W.copy(), model.H.copy(), np.asfortranarray(model.lag_val.copy())
    W, H, Th = W0.copy(), H0.copy(), np.asfortranarray(Th0.copy())
    hyper = dict(synth.HYPER)
    with capture_fds() as cap:
        O.train_ref(Y, lag_set, W, H, Th, hyper, max_iter=max_iter, threads=2, missing=True, verbose=1, warm_start=0)
    assert np.array_equal(W, W0) and np.array_equal(H, H0) and np.array_equal(Th, Th0)
    normF = np.full(max_iter, -1.0); normX = np.full(max_iter, -1.0); normLV = np.full(max_iter, -1.0)
    for line in cap.err:
        m = re.match(r'>> iter (\d+) (F|X|LV) (\S+)$', line.strip())
        if m:
            {'F': normF, 'X': normX, 'LV': normLV}[m.group(2)][int(m.group(1)) - 1] = float(m.group(3))
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, Y_indptr=Y.indptr.astype(np.int64), Y_indices=Y.indices.astype(np.int32), Y_data=Y.data,
                        shape=np.array([T, n]), lag_set=lag_set, W0=W0, H0=H0, Th0=Th0, normF=normF, normX=normX, normLV=normLV,
                        lambdaI=hyper['lambdaI'], lambdaAR=hyper['lambdaAR'], lambdaLag=hyper['lambdaLag'], max_iter=np.array(max_iter))
    print('{:>14s}: cold start {} F {} X {} LV {}'.format(name, np.dtype(dtype).name, normF.tolist(), normX.tolist(), normLV.tolist()))


def make_ref_build_case(dtype):
    """The fresh-seed case of tests/test_oracle_golden.py::test_port_matches_reference_build (same generator calls, same
    arguments): the reference's final W, H and Theta after 5 iterations, in tests/golden/ref_build/ (outside the solver cases
    that golden_names() lists)."""
    p = synth.sparse_problem(n=350, T=260, k=12, nlag=5, density=0.07, dtype=dtype, seed=11)
    m = synth.initial_model(p['Y'], p['lag_set'], 12, seed=11)
    W, H, Th = m.W.copy(), m.H.copy(), np.asfortranarray(m.lag_val.copy())
    O.train_ref(p['Y'], p['lag_set'], W, H, Th, synth.HYPER, max_iter=5)
    os.makedirs(os.path.join(OUT, 'ref_build'), exist_ok=True)
    path = os.path.join(OUT, 'ref_build', 'seed11_{}.npz'.format(np.dtype(dtype).name))
    np.savez_compressed(path, W=W, H=H, Th=Th)
    print('{:>14s}: 350 x 260, k=12, 5 iterations ({} KB)'.format(os.path.basename(path), os.path.getsize(path) // 1024))


def main():
    if O.ref(np.float32) is None:
        sys.exit('oracle/_ref is missing: run `make -C oracle ref` first (build container only)')
    if 'ref_build' in sys.argv:                 # only the fresh-seed outputs of test_port_matches_reference_build
        make_ref_build_case(np.float32)
        make_ref_build_case(np.float64)
        return
    make_case('tiny_f32', n=300, T=200, k=8, lag_set=[1, 2, 3], density=0.05, dtype=np.float32, max_iter=6)
    make_case('tiny_f64', n=300, T=200, k=8, lag_set=[1, 2, 3], density=0.05, dtype=np.float64, max_iter=6)
    # ragged: empty timestamps and empty items; lag 0 in the lag set (legal, trmf.py:354); k not a multiple of 8
    make_case('ragged_f64', n=120, T=150, k=5, lag_set=[0, 1, 7], density=0.08, dtype=np.float64, max_iter=4,
              drop_rows=(0, 17, 149), drop_cols=(3, 64, 119), seed=3)
    make_case('k16_f32', n=400, T=250, k=16, lag_set=list(range(1, 9)), density=0.06, dtype=np.float32, max_iter=4, seed=1)
    make_case('k40_f32', n=500, T=300, k=40, lag_set=list(range(1, 17)), density=0.2, dtype=np.float32, max_iter=4, seed=2)
    make_case('k64_f64', n=260, T=220, k=64, lag_set=[1, 2, 4, 8, 16, 32], density=0.45, dtype=np.float64, max_iter=3, seed=4)
    make_case('one_iter_f64', n=300, T=200, k=24, lag_set=[1, 2, 24], density=0.15, dtype=np.float64, max_iter=1, seed=5)
    # full-observation path (missing=0): electricity-like tall dense matrix (BASELINE config 1 shape class), F order, sparse
    make_full_case('full_dense_f64', n=37, T=520, k=4, lag_set=[1, 2, 3], dtype=np.float64, max_iter=5, seed=6)
    make_full_case('full_dense_f32', n=60, T=300, k=20, lag_set=[1, 2, 24], dtype=np.float32, max_iter=4, seed=7, order='F')
    make_full_case('full_sparse_f64', n=150, T=200, k=9, lag_set=[0, 1, 5], dtype=np.float64, max_iter=4, seed=8, sparse_density=0.2)
    if 'cold' in sys.argv or len(sys.argv) == 1:
        make_cold_case('py_cold_f64', np.float64)
        make_cold_case('py_cold_f32', np.float32)


if __name__ == '__main__':
    main()
