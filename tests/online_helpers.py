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
def inputs(k, density=0.3, lags=LAGS, T=T, N=N, first=FIRST):
    """fp32 values throughout (the fp64 runs use the same values, widened): W and H uniform in (0, 1), Theta's columns scaled
    contractive as Model.syn_gen does, observed values uniform in (0, 1) on about `density` of the cells.  The values are drawn
    independently of W H^T on purpose: the rounding error of a row is ~ eps |b_i| / lambda_min(A_i), and values of the model's own
    size (~ k / 4) make the right-hand sides k / 4 times larger -- the fp32 twin then drifts up to 7e-5 from the fp64 twin at
    k = 64 with (lambdaI, lambdaAR) = (0.5, 0.5), a yardstick too loose to gate anything by.
    (T, N, first): another shape, with the two designed rows at first + 5 (no observation) and first + 11 (one); the defaults give
    the arrays every earlier caller gets."""
    rng = np.random.RandomState(1000 + k)
    W = rng.rand(T, k).astype(np.float32)
    H = rng.rand(N, k).astype(np.float32)
    theta = rng.randn(len(lags), k)
    theta = np.asfortranarray((theta / (np.abs(theta).sum(axis=0) + 0.1)).astype(np.float32))
    mask = rng.rand(T, N) < density
    empty, single = first + (EMPTY_ROW - FIRST), first + (SINGLE_ROW - FIRST)
    mask[empty] = False
    mask[single] = False
    mask[single, 17] = True
    vals = rng.rand(T, N).astype(np.float32)
    vals[vals == 0] = 0.5                                   # a stored entry is a non-zero
    Y = smat.csr_matrix(np.where(mask, vals, np.float32(0)).astype(np.float32))
    return dict(W=W, H=H, theta=theta, lag_set=np.array(lags, dtype=np.uint32), Y=Y, k=k, T=T, N=N, first=first)


def rows_of(Y, lo, hi, dtype):
    """Rows lo..hi-1 of Y in `dtype` with the stored entries exactly as they are: scipy's own astype adds the entries of a cell
    stored several times first (tests/rawsparse_helpers.py); on a canonical matrix this is Y[lo:hi].astype(dtype)."""
    if not smat.issparse(Y):
        return Y[lo:hi].astype(dtype)
    Y = Y.tocsr()
    p0, p1 = int(Y.indptr[lo]), int(Y.indptr[hi])
    return smat.csr_matrix((Y.data[p0:p1].astype(dtype), Y.indices[p0:p1].copy(), Y.indptr[lo:hi + 1] - p0), shape=(hi - lo, Y.shape[1]))


def twin(d, dtype, lamI, lamAR, missing=True, first=FIRST, W=None, Y=None):
    """filter_rows on the input set in `dtype`: the whole W with the rows first.. re-solved (Y: the training values, where they
    are not the input set's own)."""
    from trmf import filter_rows
    W = d['W'] if W is None else W
    Y = d['Y'] if Y is None else Y
    return filter_rows(W.astype(dtype), d['H'].astype(dtype), d['lag_set'], d['theta'].astype(dtype), rows_of(Y, first, Y.shape[0], dtype),
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
                          rows_of(Y, i, i + 1, np.float64), i, lamI, lamAR, missing)[i]
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


# ---- per-entry statements: a cell stored several times, stored zeros (tests/rawsparse_helpers.py) -------------------------------
def sq_err_entries(rows, cols, vals, W, H, first, T, missing=True):
    """(sum, count) of the squared errors of rows first..T-1 from an ENTRY LIST, in fp64, on the training objective's reading:
    every stored entry is an observation of its own.  missing: sum_e (y_e - p_e)^2 over the entries.  Not missing (sparse
    storage): ||Y||^2 is the sum of squares of the stored values and Y . P adds the entries of a cell, so the sum is
    sum_cells p^2 + sum_e y_e (y_e - 2 p_e) -- what assim_err_kernel forms -- and not (sum_e y_e - p)^2 per cell."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    keep = (rows >= first) & (rows < T)
    r, c, y = rows[keep], cols[keep], np.asarray(vals, dtype=np.float64)[keep]
    W64, H64 = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    p = np.einsum('ed,ed->e', W64[r], H64[c])
    if missing:
        return float(((y - p) ** 2).sum()), int(r.size)
    P = W64[first:T].dot(H64.T)
    return float((P * P).sum() + (y * (y - 2.0 * p)).sum()), int(P.size)


def entry_filter(rows, cols, vals, W, H, lag_set, theta, first, lamI, lamAR, missing=True):
    """fp64 model of the filter from an ENTRY LIST (absolute row numbers): each stored entry of a new row is one observation
    (missing); every series counts once and the entries of a cell add up in the right-hand side, as the Y H product of training
    adds them (not missing).  The prior is summed in lag-set order."""
    rows, cols, y = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    out = np.array(W, dtype=np.float64)
    H64, th = np.asarray(H, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    back = np.asarray(lag_set).astype(np.int64)
    k = out.shape[1]
    G = H64.T.dot(H64)
    for i in range(first, out.shape[0]):
        e = np.flatnonzero(rows == i)
        He = H64[cols[e]]
        A = (He.T.dot(He) if missing else G) + (lamI + lamAR) * np.eye(k)
        p = np.zeros(k)
        for l in range(len(back)):
            p = p + out[i - back[l]] * th[l]
        out[i] = np.linalg.solve(A, He.T.dot(y[e]) + lamAR * p)
    return out


# ---- the per-row solve as a direct solve: backward error on ill-conditioned rows (tests/conditioning_helpers.py) ----------------
HARD_N, HARD_T0 = 96, 16
HARD_LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 96] * 2
HARD_T = HARD_T0 + len(HARD_LENGTHS)
HARD_RANKS = (7, 40, 64)
HARD_CASES = ((8.0, 0.5, 0.0), (1.0, 1e-2, 0.0), (1.0, 0.0, 1e-2), (1.0 / 64, 0.5, 0.5), (1.0, 1e-3, 1e-3), (1.0, 0.5, 50.0))
#            (scale, lambdaI, lambdaAR)


@functools.lru_cache(maxsize=None)
def hard_filter_problem(k, scale, seed=3):
    """conditioning_helpers.hard_fsolve_problem with the roles swapped: H (96 x k) nearly of rank 3, times `scale`; 32 new rows
    whose HARD_LENGTHS entries sit on a random subset of the series with values (N(0,1) + 3 sign) * scale^2 (no entry is zero);
    a random history of 16 rows of the new rows' own size (~ scale) with a few observations of its own, and a contractive Theta
    over the lags (1, 2, 5).  Everything rounded to fp32.  'Yd' is the same matrix dense, for the full-observation path."""
    rs = np.random.RandomState(seed)
    n, T, first = HARD_N, HARD_T, HARD_T0
    H = ((rs.randn(n, 3).dot(rs.randn(3, k)) + 1e-3 * rs.randn(n, k)) * scale).astype(np.float32)
    Yd = np.zeros((T, n), dtype=np.float32)
    for r, L in enumerate(HARD_LENGTHS):
        jj = np.sort(rs.permutation(n)[:L])
        Yd[first + r, jj] = ((rs.randn(L) + 3.0 * np.sign(rs.randn(L))) * scale * scale).astype(np.float32)
    hist = rs.rand(first, n) < 0.3
    Yd[:first] = np.where(hist, ((rs.randn(first, n) + 3.0 * np.sign(rs.randn(first, n))) * scale * scale), 0.0).astype(np.float32)
    W = np.zeros((T, k), dtype=np.float32)
    W[:first] = (rs.randn(first, k) * scale).astype(np.float32)
    theta = rs.randn(len(LAGS), k)
    theta = np.asfortranarray((theta / (np.abs(theta).sum(axis=0) + 0.1)).astype(np.float32))
    Y = smat.csr_matrix(Yd)
    assert np.diff(Y.indptr)[first:].tolist() == HARD_LENGTHS
    for a in (W, H, theta, Yd):
        a.setflags(write=False)
    return dict(W=W, H=H, theta=theta, lag_set=np.array(LAGS, dtype=np.uint32), Y=Y, Yd=Yd, k=k, T=T, N=n, first=first)


def row_systems(d, dtype, lamI, lamAR, missing=True, first=None):
    """(A_i, b_i) of every row first.. in fp64 WITHOUT the prior: A_i = sum_j h_j h_j^T + lam I and b_i = sum_j y_ij h_j over the
    stored entries of the row (missing) or over every series (not missing), from the fp64 products of the stored fp32 values
    (exact) added by conditioning_helpers.exact_sum (one rounding); lam = lambdaI + lambdaAR added in `dtype`, as the device and
    filter_rows add them."""
    from conditioning_helpers import exact_sum
    dt = np.dtype(dtype).type
    first = d['first'] if first is None else first
    H = d['H'].astype(np.float64)
    k = H.shape[1]
    lam = float(dt(lamI) + dt(lamAR))
    Y = d['Y'].tocsr()
    Yd = np.asarray(Y.todense(), dtype=np.float64)
    full = None
    out = []
    for i in range(first, Y.shape[0]):
        if missing:
            cols = Y.indices[Y.indptr[i]:Y.indptr[i + 1]]
            Hi, y = H[cols], Y.data[Y.indptr[i]:Y.indptr[i + 1]].astype(np.float64)
            A = exact_sum(Hi[:, :, None] * Hi[:, None, :]) + lam * np.eye(k)
        else:
            if full is None:
                full = exact_sum(H[:, :, None] * H[:, None, :]) + lam * np.eye(k)
            Hi, y, A = H, Yd[i], full
        out.append((A, exact_sum(Hi * y[:, None]) if len(y) else np.zeros(k)))
    return out


def prior_of(W, i, lag_set, theta):
    """p_i in W's element type from W's own rows before i, as Model.latent_forecast and the device form it: every product
    rounded to the element type, added in lag-set order from zero."""
    theta = np.asarray(theta, dtype=W.dtype)
    acc = np.zeros(W.shape[1], dtype=W.dtype)
    for l, lag in enumerate(np.asarray(lag_set).astype(np.int64)):
        acc = acc + W[i - lag] * theta[l]
    return acc


def row_backward_errors(d, systems, Wgot, dtype, lamAR, first=None):
    """Per new row: the normwise backward error of Wgot's row as a solution of A_i x = b_i + lambdaAR p_i, teacher-forced: p_i
    from Wgot's own earlier rows (prior_of)."""
    from conditioning_helpers import backward_error
    dt = np.dtype(dtype).type
    first = d['first'] if first is None else first
    Wgot = np.asarray(Wgot, dtype=dtype)
    la = float(dt(lamAR))
    eta = []
    for r, (A, b) in enumerate(systems):
        p = prior_of(Wgot, first + r, d['lag_set'], d['theta']).astype(np.float64)
        eta.append(backward_error(A, b + la * p, Wgot[first + r])[0])
    return np.array(eta)
