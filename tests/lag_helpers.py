"""fp64 NumPy restatement of the sparse lag-weight solve (theta_lasso_kernel) -- the yardstick of tests/test_lag_lasso_host.py and
tests/test_gpu_lag_lasso.py.  There is no compiled reference for this feature (the reference's lasso lives in its MATLAB trainer),
so the checks are optimality conditions plus this restatement.

For a latent series w = W[:, t], lags L (ascending), midx = max L:
    G[a, b] = sum_{i = midx}^{T-1} w[i - L_a] w[i - L_b]        b[a] = sum_i w[i] w[i - L_a]
each product rounded to W's element type, the sums in fp64 (l2r_autoregressive_solver::lagged_inner_product, trmf.cpp:447-453) --
no lambdaLag on the diagonal.  The solve is
    theta = argmin 1/2 th^T G th - b^T th + 1/2 lambdaLag |th|^2 + lambdaL1 |th|_1 .
"""
import numpy as np

# kLassoEps / kLassoMaxSweeps of csrc/theta_kernels.hpp, by element type of the library (test_lag_lasso_host.py reads the header)
LASSO_EPS = {'float32': 1e-7, 'float64': 1e-13}
LASSO_MAX_SWEEPS = 1000
U64 = np.finfo(np.float64).eps / 2


def gram_rhs(W, lag_set, absolute=False):
    """(G, b): k x |L| x |L| and k x |L| float64.  ``absolute``: the same sums over |products| (what a rounding bound needs)."""
    W = np.asarray(W)
    lags = np.asarray(lag_set, dtype=np.int64)
    T, k = W.shape
    midx = int(lags.max())
    cur = W[midx:]                                                       # (T - midx) x k
    lagged = np.stack([W[midx - l:T - l] for l in lags])               # |L| x (T - midx) x k, element type of W
    G = np.empty((k, len(lags), len(lags)))
    b = np.empty((k, len(lags)))
    for a in range(len(lags)):
        pb = lagged[a] * cur                                             # rounded to W's element type
        b[:, a] = (np.abs(pb) if absolute else pb).astype(np.float64).sum(axis=0)
        for c in range(a, len(lags)):
            pg = lagged[a] * lagged[c]
            G[:, a, c] = G[:, c, a] = (np.abs(pg) if absolute else pg).astype(np.float64).sum(axis=0)
    return G, b


def soft(rho, l1):
    return rho - l1 if rho > l1 else rho + l1 if rho < -l1 else 0.0


def lasso_cd(G, b, lam, l1, theta0, tol=1e-13, max_sweeps=100000):
    """Cyclic coordinate descent with covariance updates on ONE dimension's system, coordinates ascending, from theta0, until a
    sweep moves no coordinate by more than ``tol``.  Returns (theta, sweeps)."""
    th = np.array(theta0, dtype=np.float64)
    r = b - G.dot(th)
    n = len(b)
    for sweep in range(1, max_sweeps + 1):
        dmax = 0.0
        for j in range(n):
            den = G[j, j] + lam
            tn = soft(r[j] + G[j, j] * th[j], l1) / den if (den > 0 and np.isfinite(den)) else 0.0
            d = tn - th[j]
            if d != 0.0:
                r -= d * G[j]
                th[j] = tn
            dmax = max(dmax, abs(d))
        if dmax <= tol:
            return th, sweep
    raise AssertionError('the restatement did not converge')


def kkt(G, b, lam, l1, theta):
    """(gradient of the smooth part g = G th - b + lam th, KKT residual per coordinate: |g_j + l1 sign th_j| on the support,
    max(|g_j| - l1, 0) off it) -- fp64."""
    th = np.asarray(theta, dtype=np.float64)
    g = G.dot(th) - b + lam * th
    res = np.where(th != 0, np.abs(g + l1 * np.sign(th)), np.maximum(np.abs(g) - l1, 0.0))
    return g, res


def refit(G, b, lam, theta):
    """The ridge solution on the support of ``theta`` (numpy.linalg.solve), exact 0 elsewhere; also cond_2 of the support system."""
    S = np.flatnonzero(np.asarray(theta) != 0)
    out = np.zeros(len(b))
    if len(S) == 0:
        return out, 1.0
    A = G[np.ix_(S, S)] + lam * np.eye(len(S))
    out[S] = np.linalg.solve(A, b[S])
    return out, float(np.linalg.cond(A))


def kkt_bound(G, b, Gabs, babs, lam, theta, theta0, n_sum, sweeps, dtype):
    """B_j: how far the KKT conditions, evaluated in fp64 with the Gram of gram_rhs() at the DOWNLOADED theta, may be from exact
    for a correct theta_lasso_kernel.  Derived, not tuned; three terms (u = unit roundoff = eps / 2).  The feature's specification
    names the first two; the THIRD is an addition of this file, for what fp64 itself loses (summation order, in-place residual
    updates).  In the fp64 library it is the largest of the three (2.5e-8 against 6.7e-10 at 160 lags), and its sweep-count factor
    widens the bound for exactly the dimensions that converge slowly -- the GPU tests therefore also assert B <= 1e-3 lambdaL1, so
    that the bound can never decide a support:

      1. one sweep's residual   kLassoEps max(1, |th|_inf) sum_i |G_ji|
         coordinate j was exact when it was last updated; the coordinates after it in the last sweep moved by at most
         kLassoEps max(1, |th|_inf) each and shift g_j by |G_ji| times that.
      2. theta's one rounding to the element type   u_real (sum_i |G_ji| |th_i| + lam |th_j|)
         i.e. the multiple 1/2 of eps(real) (sum_i |G_ji| |th_i| + ...): one correctly rounded store, |delta_i| <= u_real |th_i|.
      3. fp64 arithmetic   u64 [2 n_sum (sum_i Gabs_ji |th_i| + babs_j) + (2 sweeps |L| + |L| + 4) (M sum_i |G_ji| + |b_j|)]
         the device and gram_rhs() add the same n_sum rounded products in different orders (each sum is within n_sum u64 of the
         exact one, relative to the sum of the |products|: Gabs, babs; a fused multiply-add on the device is inside that);
         the residual r = b - G th is formed once (|L| terms) and then updated in place 'sweeps |L|' times, each update rounding
         twice at magnitudes <= |b_j| + M sum_i |G_ji| with M = max(1, |th0|_inf, |th|_inf); 4 for the coordinate's own quotient.
    """
    th = np.abs(np.asarray(theta, dtype=np.float64))
    ureal = np.finfo(dtype).eps / 2
    M = max(1.0, float(np.abs(theta0).max()), float(th.max()))
    absG = np.abs(G)
    rowsum = absG.sum(axis=1)
    nl = len(b)
    t1 = LASSO_EPS[np.dtype(dtype).name] * max(1.0, float(th.max())) * rowsum
    t2 = ureal * (absG.dot(th) + lam * th)
    t3 = U64 * (2.0 * n_sum * (Gabs.dot(th) + babs) + (2.0 * sweeps * nl + nl + 4) * (M * rowsum + np.abs(b)))
    return t1 + t2 + t3


def ar_latent(T, k, rng, weights=((1, 0.5), (24, 0.4)), innovation=0.3):
    """T x k noisy AR process (fp64): every column follows w_i = sum weight * w_{i - lag} + innovation * N(0, 1)."""
    reach = max(l for l, _ in weights)
    W = np.zeros((T + reach, k))
    W[:reach] = innovation * rng.standard_normal((reach, k))
    noise = innovation * rng.standard_normal((T + reach, k))
    for i in range(reach, T + reach):
        W[i] = noise[i]
        for l, c in weights:
            W[i] += c * W[i - l]
    return W[reach:]


# the designed inputs of tests/test_gpu_lag_lasso.py and tests/test_lag_lasso_host.py: (T, k, lag set)
SHAPES = {
    'lags24': (400, 4, list(range(1, 25))),
    'gap': (600, 3, list(range(1, 13)) + list(range(24, 30))),
    'scratch160': (900, 2, list(range(1, 161))),          # (160^2 + 3 * 160) * 8 B = 205 KB: the global-scratch form
    'rank70': (300, 70, [1, 2, 3, 6, 12, 24]),
}


def designed(name, dtype):
    """W (a noisy AR process on lags {1: 0.5, 24: 0.4}, innovation 0.3, default_rng(1)), its Gram / rhs, lambdaLag = 0.5 and
    lambdaL1 = 0.2 median_t |b_t|_inf."""
    T, k, lags = SHAPES[name]
    W = ar_latent(T, k, np.random.default_rng(1)).astype(dtype)
    G, b = gram_rhs(W, lags)
    return dict(T=T, k=k, lags=lags, W=W, G=G, b=b, lam=0.5, l1=0.2 * float(np.median(np.abs(b).max(axis=1))))
