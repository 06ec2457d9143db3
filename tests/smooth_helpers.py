"""Shared by tests/test_smooth_host.py and tests/test_gpu_smooth.py: the inputs of the smoother tests, the fp64 truth
(trmf.smooth_rows, a direct solve), and the PCG twin -- the device's iteration in NumPy, in the element type and in the device's
order of operations -- whose own distance from the truth is the yardstick the device is gated by (test infrastructure)."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as smat

import online_helpers as OH

RTOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-10}
MAX_ITER = 400
GATE = 8.0                                                   # the project's margin for summation order; also a stop one step apart
ITER_SLACK = 2
FIRSTS = (72, 40)                                            # windows of 24 and 56 rows; both hold the empty and the single-entry row
OBJ_TOL = {np.dtype(np.float32): 1e-6, np.dtype(np.float64): 1e-12}
WIDE = dict(lags=tuple(range(1, 71)), T=120, N=50, first=96)  # the 70-lag set of tests/test_gpu_online_inputs.py


def measure(x, xstar):
    """max |x - x*| / max |x*| over the window's rows."""
    x, xstar = np.asarray(x, dtype=np.float64), np.asarray(xstar, dtype=np.float64)
    return float(np.abs(x - xstar).max() / np.abs(xstar).max())


def window_rows(d, first, dtype, missing=True, storage='sparse'):
    """The rows first.. of the input set's matrix as smooth_rows / filter_rows take them."""
    rows = OH.rows_of(d['Y'], first, d['Y'].shape[0], dtype)
    return rows if storage == 'sparse' else np.ascontiguousarray(rows.toarray())


def truth_of(d, lamI, lamAR, first, missing=True, W=None):
    """trmf.smooth_rows in fp64 on the input set (W: the rows as the session holds them, where they are not the set's own)."""
    from trmf import smooth_rows
    W = d['W'] if W is None else W
    return smooth_rows(np.asarray(W, dtype=np.float64), d['H'].astype(np.float64), d['lag_set'], d['theta'].astype(np.float64),
                       window_rows(d, first, np.float64), first, lamI, lamAR, missing)


def objective_of(d, W, lamI, lamAR, first, missing=True):
    from trmf import window_objective
    return window_objective(W, d['H'], d['lag_set'], d['theta'], window_rows(d, first, np.float64), first, lamI, lamAR, missing)


def _fold(partials):
    """The m row partials (element type) summed in fp64 in the device's order: lane c adds the rows c, c + 64, ... ascending, then
    the lanes are added by a butterfly (v + v[lane ^ 32], ^ 16, ... ^ 1)."""
    lanes = np.zeros(64, dtype=np.float64)
    for r, v in enumerate(partials):
        lanes[r & 63] += float(v)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ off]
    return float(lanes[0])


def _row_dots(a, b):
    """Per row the dot product in the element type by the device's butterfly over 64 lanes (lanes >= k hold zero)."""
    m, k = a.shape
    v = np.zeros((m, 64), dtype=a.dtype)
    v[:, :k] = a * b
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ off]
    return v[:, 0]


def pcg_twin(W, H, lag_set, lag_val, Yrows, first, lamI, lamAR, missing, dtype, rtol, max_iter):
    """The device's preconditioned conjugate gradients (csrc/smooth_kernels.hpp) in NumPy, everything in `dtype` but the sums across
    rows and the scalars alpha, beta, which are formed in fp64 and cast.  Returns (W with the window replaced, steps taken,
    converged, sqrt(r.z / (r.z)_0))."""
    dt = np.dtype(dtype)
    W = np.asarray(W, dtype=dt)
    H = np.asarray(H, dtype=dt)
    T, k = W.shape
    back = np.asarray(lag_set).astype(np.int64)
    theta = np.asarray(lag_val, dtype=dt).reshape(len(back), k)
    lamI, lamAR = dt.type(lamI), dt.type(lamAR)
    m = T - first
    sparse = smat.issparse(Yrows)
    Yr = Yrows.tocsr() if sparse else np.asarray(Yrows)
    G = np.zeros((m, k, k), dtype=dt)
    b = np.zeros((m, k), dtype=dt)
    chol = []
    for r in range(m):
        if sparse:
            cols, y = Yr.indices[Yr.indptr[r]:Yr.indptr[r + 1]], Yr.data[Yr.indptr[r]:Yr.indptr[r + 1]].astype(dt)
            if not missing:
                full = np.zeros(H.shape[0], dtype=dt)
                np.add.at(full, cols, y)
                cols, y = slice(None), full
        elif missing:
            cols = np.nonzero(Yr[r])[0]
            y = Yr[r, cols].astype(dt)
        else:
            cols, y = slice(None), Yr[r].astype(dt)
        Hi = H[cols]
        G[r] = Hi.T.dot(Hi)
        b[r] = Hi.T.dot(y)
        chol.append(np.linalg.cholesky(G[r] + (lamI + lamAR) * np.eye(k, dtype=dt)))

    def ar(v, head):                                         # e = B v; head: the rows before the window, or None for zeros
        e = v.copy()
        for l, lag in enumerate(back):
            if lag < m:
                e[lag:] -= theta[l] * v[:m - lag]
            if head is not None:
                h = min(lag, m)
                e[:h] -= theta[l] * head[first - lag:first - lag + h]
        return e

    def apply(v, e):                                         # (G + lambdaI I) v + lambdaAR (e - sum_l theta_l o e_{i + lag_l})
        a = e.copy()
        for l, lag in enumerate(back):
            if lag < m:
                a[:m - lag] -= theta[l] * e[lag:]
        return np.einsum('rcs,rs->rc', G, v) + lamI * v + lamAR * a

    def precond(r):
        return np.stack([scipy.linalg.cho_solve((chol[i], True), r[i], check_finite=False) for i in range(m)]).astype(dt)

    x = W[first:].copy()
    r = b - apply(x, ar(x, W))
    z = precond(r)
    rz = _fold(_row_dots(r, z))
    rz0, tol2 = rz, float(rtol) ** 2
    p = z.copy()
    steps, converged, spent, replaced = max_iter, False, False, False
    for j in range(max_iter + 1):
        hit = rz <= 0.0 if replaced else rz <= tol2 * rz0    # after the replacement one step is always taken from the true r
        replaced = False
        if hit:
            if j == 0 or spent or j == max_iter:
                steps, converged = j, True
                break
            # the call's one residual replacement: this step recomputes r from x (real head rows) instead of stepping
            spent = replaced = True
            r = b - apply(x, ar(x, W))
            z = precond(r)
            rz = _fold(_row_dots(r, z))
            p = z.copy()
            continue
        if j == max_iter:
            break
        q = apply(p, ar(p, None))
        alpha = dt.type(rz / _fold(_row_dots(p, q)))
        x = x + alpha * p
        r = r - alpha * q
        z = precond(r)
        rz_new = _fold(_row_dots(r, z))
        p = z + dt.type(rz_new / rz) * p
        rz = rz_new
    out = W.copy()
    out[first:] = x
    return out, steps, converged, float(np.sqrt(max(rz, 0.0) / rz0)) if rz0 > 0 else 0.0


@functools.lru_cache(maxsize=None)
def inputs(k, density=0.3, lags=OH.LAGS, T=OH.T, N=OH.N, first=OH.FIRST):
    return OH.inputs(k, density, lags, T, N, first)


@functools.lru_cache(maxsize=None)
def yardstick(k, lamI, lamAR, first, dtype, missing=True, density=0.3, lags=OH.LAGS, T=OH.T, N=OH.N, ifirst=OH.FIRST):
    """(the fp64 truth, the twin's distance from it, the twin's steps, whether it converged) on one input: shared, read only.
    `dtype` is the element type the twin iterates in; `ifirst` places the input set's two designed rows (OH.inputs)."""
    dt = np.dtype(dtype)
    d = inputs(k, density, lags, T, N, ifirst)
    want = truth_of(d, lamI, lamAR, first, missing)
    got, steps, converged, _ = pcg_twin(d['W'], d['H'], d['lag_set'], d['theta'], window_rows(d, first, dt), first, lamI, lamAR, missing,
                                        dt, RTOL[dt], MAX_ITER)
    want.setflags(write=False)
    return want, measure(got[first:], want[first:]), steps, converged


# every input a device test runs the solver to convergence on, as (name, yardstick arguments): the host test asserts that the twin
# converges within MAX_ITER on each, which is what keeps the device gate meaningful
PARITY = [(k, lamI, lamAR, first) for k in OH.RANKS for lamI, lamAR in OH.LAMBDAS for first in FIRSTS]
GEOMETRY = [
    ('reach-window', dict(k=7, first=5)),                                                   # first_row = the largest lag: 91 rows
    ('lags-1-24', dict(k=16, first=88, lags=(1, 24))),                                      # an 8-row window
    ('lags-1-to-70', dict(k=7, first=WIDE['first'], lags=WIDE['lags'], T=WIDE['T'], N=WIDE['N'], ifirst=WIDE['first'])),
    ('lags-1-to-70-k40', dict(k=40, first=WIDE['first'], lags=WIDE['lags'], T=WIDE['T'], N=WIDE['N'], ifirst=WIDE['first'])),
    ('full', dict(k=16, first=72, missing=False)),                                          # the one shared Gram
]
GEOMETRY_LAMBDAS = OH.LAMBDAS[1]


def gpu_inputs():
    for dtype in (np.float32, np.float64):
        for k, lamI, lamAR, first in PARITY:
            yield 'parity', dict(k=k, lamI=lamI, lamAR=lamAR, first=first, dtype=np.dtype(dtype))
        for name, kw in GEOMETRY:
            yield name, dict(kw, lamI=GEOMETRY_LAMBDAS[0], lamAR=GEOMETRY_LAMBDAS[1], dtype=np.dtype(dtype))
