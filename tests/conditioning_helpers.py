"""Backward error of the direct solves on ill-conditioned and badly scaled inputs (test infrastructure) -- shared by
tests/test_conditioning_host.py and tests/test_gpu_conditioning.py.

A forward gate (distance to the exact solution) grows with the condition number and says nothing at cond 1e6.  The backward error

    normwise       eta  = ||A x - b||_inf / (||A||_inf ||x||_inf + ||b||_inf)
    componentwise  eta_c = max_i |A x - b|_i / (|A| |x| + |b|)_i

of a backward-stable solve stays at about one unit roundoff u whatever the conditioning, so it stays a tight measure there.  Every
system is rebuilt here in fp64 from the very arrays the solver is given (element-type values, exact in fp64):

    F-solve, sparse   per item row   A = P^T P + lambda I,  b = P^T y     over the row's entries (P = the rows of W they name)
    F-solve, full     one shared     A = W^T W + lambda I,  b_i = W^T y_i
    Theta-solve       per dimension  the sums of lag_helpers.gram_rhs(W, lags) plus lambdaLag on the diagonal

`|A|`, `|b|` of the componentwise figure are the same sums over the absolute values of the products.  The sums themselves are
formed by exact_sum() below (one rounding), so that a system carries no summation order of its own.
"""
import functools

import numpy as np
import scipy.sparse as smat

BIG = 10 ** 6
U = {'float32': 2.0 ** -24, 'float64': 2.0 ** -53}                        # unit roundoff


def backward_error(A, b, x, Aabs=None, babs=None):
    """(normwise, componentwise) backward error of x as a solution of A x = b; all inputs fp64.  `Aabs`, `babs`: |A|, |b| as sums of
    the absolute products A and b were accumulated from (default: the absolute values of A and b themselves)."""
    A, b, x = (np.asarray(v, dtype=np.float64) for v in (A, b, x))
    if not np.all(np.isfinite(x)):
        return float('inf'), float('inf')
    Aabs = np.abs(A) if Aabs is None else Aabs
    babs = np.abs(b) if babs is None else babs
    r = np.abs(A.dot(x) - b)
    norm = r.max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())
    den = Aabs.dot(np.abs(x)) + babs
    comp = np.where(r == 0, 0.0, r / np.where(den > 0, den, 1e-300)).max()
    return float(norm), float(comp)


# ---- the fp64 systems ----------------------------------------------------------------------------------------------------------
def exact_sum(P):
    """Sum of the fp64 array P over its first axis, correct to ONE rounding of the result.  A system whose entries are plain fp64
    sums carries the rounding of those sums in their order -- a few u, as much as the fp64 solves under test lose, and shared with
    whichever side happens to add in the same order (NumPy reduces the leading axis of a 2-D array sequentially, exactly as the
    restatement's loops do, and then sees a restatement without error and a device with twice its own).  Every term is cut at 2^-26
    of the largest one: the upper parts are multiples of one quantum below 2^27 quanta each, so up to 2^26 of them add exactly; the
    lower parts (exact differences) are 2^-26 smaller, and the rounding of THEIR sum is below 2^-79 of the result."""
    P = np.asarray(P, dtype=np.float64)
    top = np.abs(P).max() if P.size else 0.0
    if top == 0:
        return P.sum(axis=0)
    assert len(P) <= 2 ** 26
    q = 2.0 ** (np.floor(np.log2(top)) - 26)
    hi = np.round(P / q) * q
    return hi.sum(axis=0) + (P - hi).sum(axis=0)


def fsolve_row_systems(Y, W0, lam):
    """Per item column of the sparse Y (T x n): A (n, k, k), b (n, k), their absolute-product twins and the row lengths.  Rows
    without entries get the identity and a zero right-hand side (nothing is solved there)."""
    Yc = smat.csc_matrix(Y)
    n, k = Y.shape[1], W0.shape[1]
    W = W0.astype(np.float64)
    A = np.empty((n, k, k)); Aabs = np.empty((n, k, k)); b = np.zeros((n, k)); babs = np.zeros((n, k))
    lens = np.diff(Yc.indptr).astype(np.int64)
    for i in range(n):
        tt = Yc.indices[Yc.indptr[i]:Yc.indptr[i + 1]]
        y = Yc.data[Yc.indptr[i]:Yc.indptr[i + 1]].astype(np.float64)
        P = W[tt]
        PP, Py = P[:, :, None] * P[:, None, :], P * y[:, None]                # products of fp32 values: exact in fp64
        A[i] = exact_sum(PP) + lam * np.eye(k)
        Aabs[i] = exact_sum(np.abs(PP)) + lam * np.eye(k)
        b[i] = exact_sum(Py); babs[i] = exact_sum(np.abs(Py))
    return dict(A=A, b=b, Aabs=Aabs, babs=babs, lens=lens)


def fsolve_full_systems(Yd, W0, lam):
    """The full-observation F-solve: one shared A (k, k) and b (n, k), every row of T entries."""
    W, Y = W0.astype(np.float64), np.asarray(Yd, dtype=np.float64)
    k = W.shape[1]
    WW, Wy = W[:, :, None] * W[:, None, :], Y[:, :, None] * W[:, None, :]     # T x k x k, T x n x k
    return dict(A=exact_sum(WW) + lam * np.eye(k), b=exact_sum(Wy), Aabs=exact_sum(np.abs(WW)) + lam * np.eye(k),
                babs=exact_sum(np.abs(Wy)), lens=np.full(Y.shape[1], Y.shape[0], dtype=np.int64))


def theta_systems(W, lags, lam):
    """Per latent dimension: A (k, |L|, |L|) = Gram + lambdaLag I and b (k, |L|) -- the sums of lag_helpers.gram_rhs (over
    i = midx .. T-1, each product rounded to W's element type, as the reference and the device both form them), added up by
    exact_sum instead of in fp64 in one particular order."""
    W = np.asarray(W)
    lags = np.asarray(lags, dtype=np.int64)
    T, k = W.shape
    midx, nl = int(lags.max()), len(lags)
    cur = W[midx:]
    lagged = [W[midx - l:T - l] for l in lags]
    A = np.empty((k, nl, nl)); Aabs = np.empty((k, nl, nl)); b = np.empty((k, nl)); babs = np.empty((k, nl))
    for a in range(nl):
        pb = (lagged[a] * cur).astype(np.float64)                            # rounded to W's element type first
        b[:, a], babs[:, a] = exact_sum(pb), exact_sum(np.abs(pb))
        for c in range(a, nl):
            pg = (lagged[a] * lagged[c]).astype(np.float64)
            A[:, a, c] = A[:, c, a] = exact_sum(pg)
            Aabs[:, a, c] = Aabs[:, c, a] = exact_sum(np.abs(pg))
    eye = lam * np.eye(nl)
    return dict(A=A + eye, b=b, Aabs=Aabs + eye, babs=babs, lens=np.full(k, T - midx, dtype=np.int64))


def _sys(S, i):
    shared = S['A'].ndim == 2
    return (S['A'] if shared else S['A'][i]), S['b'][i], (S['Aabs'] if shared else S['Aabs'][i]), S['babs'][i]


def conds(S, rows=None):
    """cond_2 of every system (of the rows named); a shared system is measured once."""
    if S['A'].ndim == 2:
        return np.full(len(S['b']) if rows is None else len(rows), float(np.linalg.cond(S['A'])))
    return np.array([float(np.linalg.cond(S['A'][i])) for i in (range(len(S['b'])) if rows is None else rows)])


def measure(S, X, rows=None):
    """Per system of S (the rows named) against the rows of X: normwise eta, componentwise eta_c, forward error
    ||x - x*||_inf / ||x*||_inf against numpy.linalg.solve."""
    rows = list(range(len(S['b']))) if rows is None else list(rows)
    X = np.asarray(X, dtype=np.float64)
    eta = np.empty(len(rows)); comp = np.empty(len(rows)); fwd = np.empty(len(rows))
    for j, i in enumerate(rows):
        A, b, Aabs, babs = _sys(S, i)
        eta[j], comp[j] = backward_error(A, b, X[i], Aabs, babs)
        xs = np.linalg.solve(A, b)
        fwd[j] = np.abs(X[i] - xs).max() / max(np.abs(xs).max(), 1e-300) if np.all(np.isfinite(X[i])) else np.inf
    return dict(rows=rows, eta=eta, comp=comp, fwd=fwd, lens=S['lens'][rows])


def line(side, m):
    """One side's figures for an evidence line: worst eta, its row and length, componentwise, forward error."""
    w = int(np.argmax(m['eta']))
    return '%s eta %.2e (row %d, %d entries) eta_c %.2e fwd %.2e' % (side, m['eta'][w], m['rows'][w], m['lens'][w], m['comp'].max(), m['fwd'].max())


# ---- 3(a), 3(b): the hard F-solve problem ----------------------------------------------------------------------------------------
HARD_T, HARD_N = 96, 64
HARD_LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 96] * 4       # around the 4-entry group and the 16-entry ring iteration
HARD_LAGS = np.array([1, 2], dtype=np.uint32)
FSOLVE_RANKS = (8, 24, 40, 64, 80)                                        # the register-tiled classes and the generic kernel
FSOLVE_HARD = {'float32': [(8.0, 0.5), (1.0, 1e-2), (1.0 / 64, 0.5)]}     # (scale, lambdaI)
FSOLVE_HARD['float64'] = FSOLVE_HARD['float32'] + [(1.0, 1e-6)]


def hard_fsolve_problem(k, scale, seed=3):
    """A nearly rank-3 W0 (T x k) times `scale` and item rows of HARD_LENGTHS entries with values (N(0,1) + 3 sign) * scale on a
    random subset of timestamps; everything rounded to fp32, so that the fp64 runs start from the same numbers.  A quad of item
    rows holds mixed lengths (four items share each length, sixteen apart)."""
    rs = np.random.RandomState(seed)
    T, n = HARD_T, HARD_N
    W0 = ((rs.randn(T, 3).dot(rs.randn(3, k)) + 1e-3 * rs.randn(T, k)) * scale).astype(np.float32)
    cols = []
    for L in HARD_LENGTHS:
        col = np.zeros(T, dtype=np.float32)
        tt = np.sort(rs.permutation(T)[:L])
        col[tt] = ((rs.randn(L) + 3.0 * np.sign(rs.randn(L))) * scale).astype(np.float32)      # no entry is zero
        cols.append(col)
    Yd = np.stack(cols, axis=1)
    Y = smat.csr_matrix(Yd)
    assert np.diff(smat.csc_matrix(Y).indptr).tolist() == HARD_LENGTHS
    H0 = rs.rand(n, k).astype(np.float32)
    Th0 = np.asfortranarray(rs.randn(len(HARD_LAGS), k).astype(np.float32))
    return dict(Y=Y, Yd=np.ascontiguousarray(Yd), W0=W0, H0=H0, Th0=Th0, lags=HARD_LAGS, lengths=list(HARD_LENGTHS))


@functools.lru_cache(maxsize=None)
def hard_case(k, scale, lam, full=False):
    """The hard problem with its fp64 systems and their condition numbers -- built once per case and shared (read only)."""
    p = hard_fsolve_problem(k, scale)
    p['sys'] = fsolve_full_systems(p['Yd'], p['W0'], lam) if full else fsolve_row_systems(p['Y'], p['W0'], lam)
    p['cond'] = conds(p['sys'])
    for v in (p['W0'], p['H0'], p['Th0'], p['Yd'], p['cond']) + tuple(p['sys'].values()):
        v.setflags(write=False)
    return p


def restated_fsolve(p, lam, dtype, full=False):
    """H of the C restatement after one F-solve, in `dtype`, from the problem's start."""
    import oracle_py as O
    H = p['H0'].astype(dtype)
    if not full:
        return O.fsolve_port(smat.csr_matrix(p['Y'].T), p['W0'].astype(dtype), H, lam)
    W, Th = p['W0'].astype(dtype), np.asfortranarray(p['Th0'].astype(dtype))
    O.train_port(np.ascontiguousarray(p['Yd'].astype(dtype)), p['lags'], W, H, Th, dict(lambdaI=lam, lambdaAR=50.0, lambdaLag=0.5),
                 max_iter=1, periods=(BIG, 1, BIG), missing=False)
    assert np.array_equal(W, p['W0'].astype(dtype))
    return H


def fsolve_cases():
    """(dtype name, k, path, scale, lambdaI) of 3(a): rows and full observation at every rank they have, the forced split at the
    register-tiled ranks."""
    out = []
    for name in ('float32', 'float64'):
        for scale, lam in FSOLVE_HARD[name]:
            out += [(name, k, 'rows', scale, lam) for k in FSOLVE_RANKS]
            out += [(name, k, 'split', scale, lam) for k in FSOLVE_RANKS if k <= 64]
            out += [(name, k, 'full', scale, lam) for k in (40, 80)]
    return out


# ---- 3(c): the Theta-solve on a smooth series -------------------------------------------------------------------------------------
THETA_T = 400
THETA_RANKS = (8, 40)
THETA_LAGS = {'L16': tuple(range(1, 17)), 'L32': tuple(range(1, 33)), 'L33': tuple(range(1, 34)), 'gap': (1, 2, 3, 7, 24)}
THETA_LAMS = (0.5, 1e-2, 1e-4)


@functools.lru_cache(maxsize=None)
def smooth_series(k, seed=7):
    """cumsum(N(0,1)) * 0.2 + 1 (fp32 values): the lagged copies of a random walk are nearly collinear."""
    W = (np.cumsum(np.random.RandomState(seed).randn(THETA_T, k), axis=0) * 0.2 + 1.0).astype(np.float32)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def theta_case(k, lagname, lam, dtype_name):
    """The systems of one Theta case (the products are rounded to the element type the solve runs in) and their condition numbers."""
    W = smooth_series(k).astype(dtype_name)
    S = theta_systems(W, THETA_LAGS[lagname], lam)
    return dict(W=W, lags=THETA_LAGS[lagname], sys=S, cond=conds(S))


def theta_y(T, n=20):
    return smat.random(T, n, density=0.2, random_state=np.random.RandomState(5), format='csr', dtype=np.float64)


def restated_theta(W, lags, lam):
    """Theta (|L| x k) of the C restatement: the lag-weight phase alone (periods (BIG, BIG, 1)) in W's element type."""
    import oracle_py as O
    dtype = W.dtype
    Wc = np.ascontiguousarray(W.copy())
    H = np.zeros((20, W.shape[1]), dtype=dtype)
    Th = np.asfortranarray(np.zeros((len(lags), W.shape[1]), dtype=dtype))
    O.train_port(theta_y(W.shape[0]).astype(dtype), np.array(lags, np.uint32), Wc, H, Th, dict(lambdaI=0.5, lambdaAR=50.0, lambdaLag=lam),
                 max_iter=1, periods=(BIG, BIG, 1))
    assert np.array_equal(Wc, W)
    return Th


def theta_cases():
    return [(name, k, lagname, lam) for name in ('float32', 'float64') for k in THETA_RANKS for lagname in THETA_LAGS for lam in THETA_LAMS]


# ---- 3(d): one item row whose factorisation breaks down ---------------------------------------------------------------------------
BREAK_T, BREAK_N, BREAK_LAM = 256, 12, 2.0 ** -30
BREAK_RANKS = (40, 64)


@functools.lru_cache(maxsize=None)
def breakdown_problem(k, pos, seed=9):
    """fp32.  Eight timestamps of W0 hold one small-integer vector v; item 4 + pos (position `pos` of the second quad) observes only
    those: its Gram 8 v v^T has rank 1 and the ridge 2^-30 is below the rounding of its diagonal, so a pivot of its Cholesky
    factorisation is not positive.  Every other item (and the benign column that replaces the degenerate one in `Yb`) observes at
    least 3k of the other timestamps, whose rows of W0 are uniform random: well conditioned without a ridge."""
    rs = np.random.RandomState(seed + k)
    T, n = BREAK_T, BREAK_N
    W0 = rs.rand(T, k).astype(np.float32)
    same = np.sort(rs.permutation(T)[:8])
    W0[same] = rs.randint(1, 4, size=k).astype(np.float32)
    rest = np.setdiff1d(np.arange(T), same)
    cols = []
    for _ in range(n):
        col = np.zeros(T, dtype=np.float32)
        tt = rs.permutation(rest)[:rs.randint(3 * k, len(rest) + 1)]
        col[tt] = (rs.randn(len(tt)) + 3.0 * np.sign(rs.randn(len(tt)))).astype(np.float32)
        cols.append(col)
    benign = np.stack(cols, axis=1)
    deg = 4 + pos
    broken = benign.copy()
    broken[:, deg] = 0
    broken[same, deg] = (rs.randn(8) + 3.0 * np.sign(rs.randn(8))).astype(np.float32)
    Y, Yb = smat.csr_matrix(broken), smat.csr_matrix(benign)
    H0 = rs.rand(n, k).astype(np.float32)
    Th0 = np.asfortranarray(rs.randn(len(HARD_LAGS), k).astype(np.float32))
    others = [i for i in range(n) if i != deg]
    S = fsolve_row_systems(Y, W0, BREAK_LAM)
    assert S['lens'][deg] == 8 and S['lens'][others].min() >= 3 * k
    return dict(Y=Y, Yb=Yb, W0=W0, H0=H0, Th0=Th0, lags=HARD_LAGS, deg=deg, others=others, sys=S, cond=conds(S, others),
                rhs=S['b'][deg].copy())


# ---- 4: three iterations at the hyper-parameter and data-scale extremes -----------------------------------------------------------
EXT_T, EXT_N = 200, 60
EXT_LAGS = np.array([1, 2, 3, 7], dtype=np.uint32)
EXTREMES = {                                                              # name: ((lambdaI, lambdaAR, lambdaLag), factor on Y)
    'base': ((0.5, 50.0, 0.5), 1.0),
    'lambdaAR-0': ((0.5, 0.0, 0.5), 1.0),
    'lambdaAR-1e-3': ((0.5, 1e-3, 0.5), 1.0),
    'lambdaAR-1e4': ((0.5, 1e4, 0.5), 1.0),
    'lambdaI-1e-2': ((1e-2, 50.0, 0.5), 1.0),
    'lambdaLag-1e-3': ((0.5, 50.0, 1e-3), 1.0),
    'lambdaLag-1e3': ((0.5, 50.0, 1e3), 1.0),
    'Y-x1024': ((0.5, 50.0, 0.5), 1024.0),
    'Y-div1024': ((0.5, 50.0, 0.5), 1.0 / 1024),
    'all-small': ((1e-2, 1e-3, 1e-3), 1.0),
}
EXT_RANKS = [('float32', 16), ('float64', 16), ('float32', 40), ('float64', 64)]


@functools.lru_cache(maxsize=None)
def extreme_data(seed=13):
    """cumsum(N(0,1)) * 0.1 (T x 4) times N(0,1) (4 x n) plus 0.05 N(0,1), 30 % of the cells observed; fp32 values."""
    rs = np.random.RandomState(seed)
    D = (np.cumsum(rs.randn(EXT_T, 4), axis=0) * 0.1).dot(rs.randn(EXT_N, 4).T) + 0.05 * rs.randn(EXT_T, EXT_N)
    D = np.where(rs.rand(EXT_T, EXT_N) < 0.3, D, 0.0).astype(np.float32)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def extreme_start(k, seed=17):
    rs = np.random.RandomState(seed + k)
    out = (rs.rand(EXT_T, k).astype(np.float32), rs.rand(EXT_N, k).astype(np.float32),
           np.asfortranarray(rs.randn(len(EXT_LAGS), k).astype(np.float32)))
    for a in out:
        a.setflags(write=False)
    return out


def extreme_problem(case, dtype, dense=False):
    """(Y, hyper) of one case: the sparse matrix (missing = 1) or the same matrix dense with zeros in the unobserved cells."""
    (lamI, lamAR, lamLag), factor = EXTREMES[case]
    D = (extreme_data() * np.float32(factor)).astype(dtype)                # a power of two: exact
    Y = np.ascontiguousarray(D) if dense else smat.csr_matrix(D)
    return Y, dict(lambdaI=lamI, lambdaAR=lamAR, lambdaLag=lamLag)


def all_cells(Yd):
    """The dense matrix as a CSR that stores every cell (the objective of the full-observation path sums over all of them)."""
    T, n = Yd.shape
    return smat.csr_matrix((np.asarray(Yd).ravel(), np.tile(np.arange(n), T), np.arange(0, T * n + 1, n)), shape=(T, n))
