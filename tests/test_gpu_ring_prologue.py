"""GPU (-m gpu): the prologue and the row ends of the Gram ring (gram_kernels.hpp gram_ring) in the F-solve kernels -- the fp32 quad
kernel (four item rows per wavefront, one stream over the quad's rows) and the fp64 kernel (one row per wavefront, the row's last
iteration behind the loop).  The ring requests the entries of iteration 1 and the slices of iteration 0 before its loop and keeps
slots across iterations and rows; a slot left over from the prologue or from the previous row would show in a row that starts a
quad, follows an empty row or ends inside an iteration.  One F-solve (period_W, period_Lag > max_iter) through the session, n = 64
item rows over T = 48 timestamps, row lengths that put every such case somewhere:

  * an empty first row of a quad, an all-empty quad, a quad whose only non-empty row is its last;
  * rows of 1, 3, 4, 15, 16, 17, 32 and 33 entries (around the 4-entry group and the 16-entry iteration);
  * rows of 48 entries: three ring iterations.

Every row of H against the fp64 normal equations solved in NumPy at the F-solve gate of tests/test_gpu_parity.py
(max |d| / max |ref| < 2e-4 in fp32, < 1e-6 in fp64), and BIT FOR BIT the same rows when one dummy row is put in front, which
moves every row to another lane row of another quad (fp32) / to another wavefront of another workgroup (fp64)."""
import numpy as np
import pytest
import scipy.sparse as smat

from helpers import evidence, make_model, relmax
from trmf import session, synth

pytestmark = pytest.mark.gpu

BIG = 10 ** 6
N, T = 64, 48
LAGS = np.array([1, 2], dtype=np.uint32)
RANKS = (8, 40, 56, 64)               # fp32: <1,8>, <3,40> and <4,56> (both with group-granular row ends, gram_ring ROWEND), <4,64>
#        quad 0: empty first row      quad 1: all empty   quad 2                quad 3              quad 4: only the last row
LENGTHS = [0, 1, 3, 4,                0, 0, 0, 0,         15, 16, 17, 32,       33, 48, 1, 3,       0, 0, 0, 17,
           48, 0, 48, 5,              4, 4, 4, 4,         16, 16, 16, 16,       1, 0, 1, 0,         47, 2, 31, 18,
           0, 33, 0, 0,               12, 13, 14, 15,     17, 0, 0, 0,          32, 32, 33, 1,
           48, 48, 48, 48,            7, 8, 9, 0]
assert len(LENGTHS) == N


def pattern():
    """Y (T x N, fp32-representable values) with LENGTHS[i] entries in item column i, and the same behind one dummy column."""
    rs = np.random.RandomState(5)
    cols = []
    for L in [5] + LENGTHS:                                  # column 0 of the shifted problem: the dummy row
        col = np.zeros(T, dtype=np.float32)
        tt = np.sort(rs.permutation(T)[:L])
        col[tt] = (rs.randn(L) + 3.0 * np.sign(rs.randn(L))).astype(np.float32)     # no entry is zero
        cols.append(col)
    shifted = np.stack(cols, axis=1)
    return smat.csr_matrix(shifted[:, 1:]), smat.csr_matrix(shifted)


def one_fsolve(Y, W0, H0, Th0, dtype):
    model = make_model(W0.astype(dtype), H0.astype(dtype), np.asfortranarray(Th0.astype(dtype)), LAGS)
    with session.Session(Y.astype(dtype), model, period_W=BIG, period_H=1, period_Lag=BIG, missing=True, **synth.HYPER) as s:
        s.run(1)
        s.download()
    assert np.array_equal(model.W, W0.astype(dtype))         # untouched phase
    return model.H


def fp64_rows(Y, W0, H0, lam):
    """Every item row from its own normal equations in fp64; rows without entries keep their initial values (trmf.cpp:374)."""
    Yc = smat.csc_matrix(Y)
    H = H0.astype(np.float64)
    for i in range(Y.shape[1]):
        tt = Yc.indices[Yc.indptr[i]:Yc.indptr[i + 1]]
        if len(tt):
            P = W0[tt].astype(np.float64)
            H[i] = np.linalg.solve(P.T @ P + lam * np.eye(W0.shape[1]), P.T @ Yc.data[Yc.indptr[i]:Yc.indptr[i + 1]].astype(np.float64))
    return H


@pytest.fixture(scope='module')
def problems():
    Y, Ys = pattern()
    assert np.diff(smat.csc_matrix(Y).indptr).tolist() == LENGTHS
    assert np.diff(smat.csc_matrix(Ys).indptr).tolist() == [5] + LENGTHS
    out = {}
    for k in RANKS:
        m0 = synth.initial_model(Ys, LAGS, k, seed=11, dtype=np.float32)       # fp32 values: the fp64 runs start from the same numbers
        W0, Hs0, Th0 = m0.W.copy(), m0.H.copy(), m0.lag_val.copy()
        out[k] = dict(Y=Y, Ys=Ys, W0=W0, H0=Hs0[1:].copy(), Hs0=Hs0, Th0=Th0,
                      ref=fp64_rows(Y, W0, Hs0[1:], synth.HYPER['lambdaI']))
    return out


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('k', RANKS)
def test_rows_at_the_prologue_and_at_row_ends(k, dtype, problems):
    p = problems[k]
    H = one_fsolve(p['Y'], p['W0'], p['H0'], p['Th0'], dtype)
    Hs = one_fsolve(p['Ys'], p['W0'], p['Hs0'], p['Th0'], dtype)

    ref = p['ref']
    tol = 1e-6 if dtype == np.float64 else 2e-4              # tests/test_gpu_parity.py: max|d| / max|ref| of one F-solve
    err_rows = np.abs(H.astype(np.float64) - ref).max(axis=1) / np.abs(ref).max()
    own = np.abs(H.astype(np.float64) - ref).max(axis=1) / np.abs(ref).max(axis=1)
    worst = int(np.argmax(err_rows))
    differing = np.flatnonzero((Hs[1:] != H).any(axis=1))
    evidence('ring prologue k=%d %s: max|d|/max|ref| %.2e (row %d, %d entries), worst row against its own max %.2e (row %d, %d entries); '
             'rows that change behind a dummy row: %d of %d%s' % (
                 k, np.dtype(dtype).name, err_rows.max(), worst, LENGTHS[worst], own.max(), int(np.argmax(own)), LENGTHS[int(np.argmax(own))],
                 len(differing), N, '' if not len(differing) else ' (first %s, lengths %s)' % (differing[:8].tolist(), [LENGTHS[i] for i in differing[:8]])))

    for i, L in enumerate(LENGTHS):
        if L == 0:
            assert np.array_equal(H[i], p['H0'][i].astype(dtype)), i           # rows without entries stay untouched
    assert np.all(err_rows < tol), np.flatnonzero(err_rows >= tol).tolist()
    assert relmax(H, ref) < tol
    assert H.tobytes() == np.ascontiguousarray(Hs[1:]).tobytes()
