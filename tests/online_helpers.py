"""Shared by tests/test_online_host.py and tests/test_gpu_online.py: the designed input set of the online-update tests, its
fp32 / fp64 NumPy twins and the yardstick the device is gated by (test infrastructure)."""
import functools

import numpy as np
import scipy.sparse as smat

from helpers import relmax

LAGS = (1, 2, 5)
T, N, TN = 96, 50, 24
FIRST = T - TN
RANKS = (1, 7, 16, 40, 64)                                  # every NT, with and without pad columns
LAMBDAS = ((0.5, 50.0), (0.5, 0.5), (0.0, 1.0))
EMPTY_ROW, SINGLE_ROW = FIRST + 5, FIRST + 11               # a new row without observations, one with a single entry
EPS_SCALE = float(np.finfo(np.float64).eps / np.finfo(np.float32).eps)
GATE = 8.0                                                  # a different summation order across a 24-row chain


@functools.lru_cache(maxsize=None)
def inputs(k, density=0.3, lags=LAGS):
    """fp32 values throughout (the fp64 runs use the same values, widened): W and H uniform in (0, 1), Theta's columns scaled
    contractive as Model.syn_gen does, observed values uniform in (0, 1) on about `density` of the cells.  The values are drawn
    independently of W H^T on purpose: the rounding error of a row is ~ eps |b_i| / lambda_min(A_i), and values of the model's own
    size (~ k / 4) make the right-hand sides k / 4 times larger -- the fp32 twin then drifts up to 7e-5 from the fp64 twin at
    k = 64 with (lambdaI, lambdaAR) = (0.5, 0.5), a yardstick too loose to gate anything by."""
    rng = np.random.RandomState(1000 + k)
    W = rng.rand(T, k).astype(np.float32)
    H = rng.rand(N, k).astype(np.float32)
    theta = rng.randn(len(lags), k)
    theta = np.asfortranarray((theta / (np.abs(theta).sum(axis=0) + 0.1)).astype(np.float32))
    mask = rng.rand(T, N) < density
    mask[EMPTY_ROW] = False
    mask[SINGLE_ROW] = False
    mask[SINGLE_ROW, 17] = True
    vals = rng.rand(T, N).astype(np.float32)
    vals[vals == 0] = 0.5                                   # a stored entry is a non-zero
    Y = smat.csr_matrix(np.where(mask, vals, np.float32(0)).astype(np.float32))
    return dict(W=W, H=H, theta=theta, lag_set=np.array(lags, dtype=np.uint32), Y=Y, k=k)


def twin(d, dtype, lamI, lamAR, missing=True, first=FIRST, W=None, Y=None):
    """filter_rows on the input set in `dtype`: the whole W with the rows first.. re-solved (Y: the training values, where they
    are not the input set's own)."""
    from trmf import filter_rows
    W = d['W'] if W is None else W
    Y = d['Y'] if Y is None else Y
    return filter_rows(W.astype(dtype), d['H'].astype(dtype), d['lag_set'], d['theta'].astype(dtype), Y[first:].astype(dtype),
                       first, lamI, lamAR, missing)


def yardstick_of(d, lamI, lamAR, missing=True, first=FIRST, Y=None):
    """(the fp64 twin's W, relmax of the fp32 twin's new rows against its): what a different rounding of the same chain costs."""
    w64 = twin(d, np.float64, lamI, lamAR, missing, first, Y=Y)
    w32 = twin(d, np.float32, lamI, lamAR, missing, first, Y=Y)
    return w64, relmax(w32[first:], w64[first:])


@functools.lru_cache(maxsize=None)
def yardstick(k, lamI, lamAR, missing=True, density=0.3, first=FIRST):
    return yardstick_of(inputs(k, density), lamI, lamAR, missing, first)


def bound(dtype, dev32):
    return GATE * dev32 * (1.0 if np.dtype(dtype) == np.float32 else EPS_SCALE)


def teacher_forced(d, Wdev, lamI, lamAR, missing=True, first=FIRST, Y=None):
    """Per row i >= first: relmax of the device's row against the fp64 twin's solve of that row alone, its prior formed from the
    device's own earlier rows."""
    from trmf import filter_rows
    Y = d['Y'] if Y is None else Y
    out = []
    W64 = np.asarray(Wdev, dtype=np.float64)
    for i in range(first, W64.shape[0]):
        ref = filter_rows(W64[:i + 1], d['H'].astype(np.float64), d['lag_set'], d['theta'].astype(np.float64),
                          Y[i:i + 1].astype(np.float64), i, lamI, lamAR, missing)[i]
        out.append(relmax(W64[i], ref))
    return out


def sq_err(d, W, first, missing=True, Y=None):
    """sum over Omega of (y - w_i . h_j)^2 over the rows first.. in fp64 NumPy."""
    Y = d['Y'] if Y is None else Y
    W = np.asarray(W, dtype=np.float64)
    P = W[first:].dot(d['H'].astype(np.float64).T)
    Yd = np.asarray(Y[first:].todense() if smat.issparse(Y) else Y[first:], dtype=np.float64)
    E = (Yd - P) ** 2
    if missing:
        M = np.zeros(E.shape, dtype=bool)
        Yc = Y[first:].tocoo()
        M[Yc.row, Yc.col] = True
        return float(E[M].sum()), int(M.sum())
    return float(E.sum()), E.size
