"""GPU (-m gpu): the fp32 quad F-solve (fsolve_quad_kernel / fsolve_quad_long_kernel, four item rows per wavefront, one per 16-lane
row; gram_kernels.hpp quad_factor_solve).  The trailing update of the four factorisations shares one matrix instruction whose A operand
is broadcast inside each 16-lane row: a wrong broadcast group would mix the four systems of a wavefront.  So

  * a row's solution must not depend on its quad neighbours: the same problem with its item rows permuted (every row gets other
    neighbours) must give the same rows BIT FOR BIT;
  * every row must solve its own normal equations: against an fp64 NumPy solve at the fp32 F-solve gate of tests/test_gpu_parity.py
    (2e-4, max |d| / max |ref|).

One F-solve only (period_W, period_Lag > max_iter), every NT / KMAX instantiation (ranks 8 .. 64: with and without the right-hand side
in the pad column), through the row kernel and through the split-row kernel (TRMF_LONG_ROW: rows of >= 56 entries)."""
import numpy as np
import pytest
import scipy.sparse as smat

import trmf
from helpers import evidence, make_model, relmax
from trmf import synth

pytestmark = pytest.mark.gpu

BIG = 10 ** 6
N, T = 203, 240                       # n is not a multiple of 4: the last wavefront holds three systems and an idle lane row
EMPTY = (0, 57, 58, 130, 202)         # item rows without entries (left untouched, trmf.cpp:374); 57, 58: two in one quad
SCALED = 77                           # one row 1e3 times its neighbours


def problem(k):
    p = synth.sparse_problem(n=N, T=T, k=k, nlag=2, density=0.25, dtype=np.float32, seed=23)
    Y = smat.lil_matrix(p['Y'])
    for j in EMPTY:
        Y[:, j] = 0
    Y = smat.csc_matrix(Y)
    Y.data[Y.indptr[SCALED]:Y.indptr[SCALED + 1]] *= np.float32(1e3)
    Y = smat.csr_matrix(Y); Y.eliminate_zeros(); Y.sort_indices()
    m0 = synth.initial_model(Y, p['lag_set'], k, seed=23)
    return Y, p['lag_set'], m0


def one_fsolve(Y, lags, W0, H0, Th0):
    model = make_model(W0, H0, Th0, lags)
    trmf.train(Y, model, max_iter=1, period_W=BIG, period_H=1, period_Lag=BIG, missing=True, **synth.HYPER)
    assert np.array_equal(model.W, W0) and np.array_equal(model.lag_val, Th0)      # untouched phases
    return model.H


def quads_of(order):
    """order[p] = the row at position p -> for every row the set of rows that share its wavefront (positions 4q .. 4q+3)."""
    return {int(r): frozenset(int(x) for x in order[p - p % 4:p - p % 4 + 4]) for p, r in enumerate(order)}


def fp64_rows(Y, W0, H0, lam):
    """Every item row from its own normal equations in fp64; rows without entries keep their initial values (trmf.cpp:374)."""
    Yc = smat.csc_matrix(Y)
    k = W0.shape[1]
    H = H0.astype(np.float64)
    for i in range(Y.shape[1]):
        tt = Yc.indices[Yc.indptr[i]:Yc.indptr[i + 1]]
        if len(tt) == 0:
            continue
        P = W0[tt].astype(np.float64); y = Yc.data[Yc.indptr[i]:Yc.indptr[i + 1]].astype(np.float64)
        H[i] = np.linalg.solve(P.T @ P + lam * np.eye(k), P.T @ y)
    return H


@pytest.mark.parametrize('path', ['rows', 'split'])
@pytest.mark.parametrize('k', [8, 16, 24, 32, 40, 48, 56, 64])
def test_row_solution_is_independent_of_its_quad_neighbours(k, path, monkeypatch):
    if path == 'split':     # rows of >= 56 entries (about two thirds of them) become split rows: fsolve_quad_long_kernel, four per wavefront
        monkeypatch.setenv('TRMF_LONG_ROW', '56')
        monkeypatch.setenv('TRMF_LONG_CHUNK', '32')
    Y, lags, m0 = problem(k)
    lens = np.diff(smat.csc_matrix(Y).indptr)
    assert all(lens[j] == 0 for j in EMPTY) and (lens > 0).sum() == N - len(EMPTY)
    assert (lens >= 56).sum() >= 40 and ((lens > 0) & (lens < 56)).sum() >= 40     # both kernels get many quads on the split path

    H = one_fsolve(Y, lags, m0.W, m0.H, m0.lag_val)

    perm = np.random.RandomState(1234).permutation(N)                 # row perm[p] moves to position p
    before, after = quads_of(np.arange(N)), quads_of(perm)
    assert all(before[r] != after[r] for r in range(N))               # every row gets other neighbours in the row kernel
    if path == 'split':                                               # ... and in the list of split rows (ascending row ids)
        lb, la = quads_of(np.flatnonzero(lens >= 56)), quads_of(perm[lens[perm] >= 56])
        assert sum(lb[r] != la[r] for r in lb) >= len(lb) - 4
    Yp = smat.csr_matrix(smat.csc_matrix(Y)[:, perm]); Yp.sort_indices()
    Hp = one_fsolve(Yp, lags, m0.W, np.ascontiguousarray(m0.H[perm]), m0.lag_val)
    back = np.empty_like(Hp); back[perm] = Hp

    same = np.array_equal(back, H)
    differing = np.flatnonzero((back != H).any(axis=1))
    evidence('quad F-solve k=%d %s: rows that change with their quad neighbours: %d of %d%s' % (
        k, path, len(differing), N, '' if same else ' (first %s, max |d| %.3e)' % (differing[:8].tolist(), np.abs(back - H).max())))

    # fp64 normal equations of every row; the scaled row on its own as well, so that it cannot hide the others (or hide behind them)
    ref = fp64_rows(Y, m0.W, m0.H, synth.HYPER['lambdaI'])
    rest = np.array([i for i in range(N) if i != SCALED])
    errs = (relmax(H, ref), relmax(H[rest], ref[rest]), relmax(H[SCALED:SCALED + 1], ref[SCALED:SCALED + 1]))
    evidence('quad F-solve k=%d %s: relmax vs fp64 normal equations: all rows %.2e, without the scaled row %.2e, the scaled row %.2e' % ((k, path) + errs))

    assert same
    for j in EMPTY:
        assert np.array_equal(H[j], m0.H[j])
    assert np.abs(ref[SCALED]).max() > 100 * np.abs(ref[rest]).max()   # the systems of that quad do differ by orders of magnitude
    assert max(errs) < 2e-4
