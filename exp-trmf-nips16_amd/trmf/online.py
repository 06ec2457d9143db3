"""Online updates on the host: the forward filter that ``trmf_session_assimilate`` runs on the device, as plain NumPy.

New timestamps are absorbed without ALS iterations over the history: H and the lag weights stay fixed, and each new row of W,
in ascending order, is the minimiser of its own observations plus the AR prior from the rows before it::

    Omega_i = the stored entries of row i (missing)  |  every series, an absent entry reading as 0 (not missing)
    A_i     = sum_{j in Omega_i} h_j h_j^T + (lambdaI + lambdaAR) I
    p_i     = sum_l lag_val[l] * W[i - lag_set[l]]          (rows < i as already updated; Model.latent_forecast's expression)
    W[i]    = A_i^-1 (sum_{j in Omega_i} y_ij h_j + lambdaAR p_i)

A filter, not a smoother: rows before ``first_row`` never see the new data.  ``filter_rows`` is the specification the device
tests compare against and the host path of ``Model.assimilate``.  ``smooth_rows`` is the smoother (``trmf_session_smooth``): the
joint minimiser over a window of tail rows, which also counts the AR penalties of the later rows a row appears in.  ``robust_filter_rows`` is the same filter with Huber weights
(``trmf_session_assimilate_robust``): a cell far outside its series' residual scale is down-weighted, and the weights are returned.
``robust_smooth_rows`` is the smoother on the same Huber loss (``trmf_session_smooth_robust``).
``series_ridge`` / ``SeriesStats`` refit the loadings H from new rows (``trmf_session_adapt_series``), ``SeriesStats.absorb_robust``
with Huber weights on the new entries (``trmf_session_adapt_series_robust``; ``robust_series_objective`` is its objective).
"""
import numpy as np
import scipy.linalg
import scipy.sparse as smat


def filter_rows(W, H, lag_set, lag_val, Yrows, first_row, lambdaI, lambdaAR, missing):
    """A copy of ``W`` (T x k) whose rows ``first_row .. T-1`` are re-solved in ascending order; ``Yrows`` holds the
    ``T - first_row`` rows of the training matrix that belong to them (a ``scipy.sparse`` matrix or an array; with
    ``missing`` the stored entries of a sparse matrix, the non-zeros of an array, are the observations).  All arithmetic is
    in the dtype of ``W``; each weight is cast to it before the two are added.  ``ValueError`` for a lag set with lag 0, a
    ``first_row`` below the largest lag or above T, a row count that does not match, or a row whose system is not positive
    definite (possible only with ``lambdaI + lambdaAR == 0``); the message names the row."""
    W = np.asarray(W)
    dt = W.dtype
    T, k = W.shape
    back = np.asarray(lag_set).astype(np.int64)
    if back.size and back.min() == 0:
        raise ValueError('filter_rows: the lag set contains lag 0 (a row would be its own prior)')
    reach = int(back.max()) if back.size else 0
    first_row = int(first_row)
    if first_row < reach or first_row > T:
        raise ValueError('filter_rows: first_row {} outside [{} (the largest lag), {} (rows)]'.format(first_row, reach, T))
    if Yrows.shape[0] != T - first_row or (T > first_row and Yrows.shape[1] != H.shape[0]):
        raise ValueError('filter_rows: Yrows is {}, rows {}..{} of {} series were expected'.format(Yrows.shape, first_row, T, H.shape[0]))
    H = np.asarray(H, dtype=dt)
    theta = np.asarray(lag_val, dtype=dt)
    lamAR = dt.type(lambdaAR)
    lam = dt.type(lambdaI) + lamAR
    sparse = smat.issparse(Yrows)
    Yr = Yrows.tocsr() if sparse else np.asarray(Yrows)
    out = W.copy()
    eye = np.eye(k, dtype=dt)
    for i in range(first_row, T):
        r = i - first_row
        if sparse:
            lo, hi = Yr.indptr[r], Yr.indptr[r + 1]
            cols, y = Yr.indices[lo:hi], Yr.data[lo:hi].astype(dt)
            if not missing:                                  # every series counts: absent entries read as 0
                full = np.zeros(H.shape[0], dtype=dt)
                np.add.at(full, cols, y)
                cols, y = slice(None), full
        elif missing:
            cols = np.nonzero(Yr[r])[0]
            y = Yr[r, cols].astype(dt)
        else:
            cols, y = slice(None), Yr[r].astype(dt)
        Hi = H[cols]
        A = Hi.T.dot(Hi) + lam * eye
        prior = np.sum(out[i - back] * theta, axis=0) if back.size else np.zeros(k, dtype=dt)
        b = Hi.T.dot(y) + lamAR * prior
        try:
            if not np.all(np.isfinite(A)):
                raise np.linalg.LinAlgError('not finite')
            L = np.linalg.cholesky(A)
            if not (np.all(np.isfinite(L)) and np.all(np.diagonal(L) > 0)):
                raise np.linalg.LinAlgError('pivot')
        except np.linalg.LinAlgError:
            raise ValueError('filter_rows: row {}: G + (lambdaI + lambdaAR) I is not positive definite'.format(i))
        out[i] = scipy.linalg.cho_solve((L, True), b, check_finite=False)
    return out


def robust_filter_rows(W, H, lag_set, lag_val, Yrows, first_row, lambdaI, lambdaAR, missing, scale, c=3.0, sweeps=4):
    """``filter_rows`` with Huber weights: the specification of ``trmf_session_assimilate_robust``.  A cell whose residual is
    beyond ``c * scale[j]`` of its series enters its row's system with the weight ``c * scale[j] / |r|`` instead of 1::

        w^0 = p_i;  for s = 1 .. sweeps:   r_j = y_ij - w^{s-1} . h_j,   omega_j = t_j / |r_j| if |r_j| > t_j else 1   (t_j = c scale_j)
                                           w^s = (sum omega_j h_j h_j^T + lam I)^-1 (sum omega_j y_ij h_j + lambdaAR p_i)

    (iteratively reweighted least squares on Huber's loss; a fixed number of sweeps, no convergence test).  Returns
    ``(W_out, weights)``: the weights of the LAST sweep (formed from ``w^{sweeps-1}``), one per stored entry in CSR order for a
    sparse ``Yrows`` with ``missing``, a ``(T - first_row) x n`` matrix for an array (a cell that is no observation reads 1).
    ``c = inf`` is the plain filter.  Sparse rows without ``missing`` are refused: an absent entry there is an observation
    without a slot to report a weight in.  ``ValueError`` in ``filter_rows``' cases and for a scale that is not finite and
    positive, ``c`` not positive, ``sweeps < 1``, a row whose weighted system is not positive definite."""
    W = np.asarray(W)
    dt = W.dtype
    T, k = W.shape
    back = np.asarray(lag_set).astype(np.int64)
    if back.size and back.min() == 0:
        raise ValueError('robust_filter_rows: the lag set contains lag 0 (a row would be its own prior)')
    reach = int(back.max()) if back.size else 0
    first_row = int(first_row)
    if first_row < reach or first_row > T:
        raise ValueError('robust_filter_rows: first_row {} outside [{} (the largest lag), {} (rows)]'.format(first_row, reach, T))
    if Yrows.shape[0] != T - first_row or (T > first_row and Yrows.shape[1] != H.shape[0]):
        raise ValueError('robust_filter_rows: Yrows is {}, rows {}..{} of {} series were expected'.format(Yrows.shape, first_row, T, H.shape[0]))
    sparse = smat.issparse(Yrows)
    if sparse and not missing:
        raise ValueError('robust_filter_rows: sparse rows without missing are not covered (an absent entry would be an observation '
                         'without a slot to report its weight in); pass the rows as an array')
    n = H.shape[0]
    scale = np.asarray(scale, dtype=np.float64)
    if scale.ndim == 0:
        scale = np.full(n, float(scale))
    if scale.shape != (n,):
        raise ValueError('robust_filter_rows: scale has shape {}, one value per series ({}) was expected'.format(scale.shape, n))
    bad = np.flatnonzero(~(np.isfinite(scale) & (scale > 0)))
    if bad.size:
        raise ValueError('robust_filter_rows: scale[{}] = {!r} is not finite and positive'.format(int(bad[0]), float(scale[bad[0]])))
    c = float(c)
    if not c > 0:
        raise ValueError('robust_filter_rows: c must be positive (inf: the plain filter), not {!r}'.format(c))
    sweeps = int(sweeps)
    if sweeps < 1:
        raise ValueError('robust_filter_rows: sweeps must be at least 1, not {}'.format(sweeps))
    H = np.asarray(H, dtype=dt)
    theta = np.asarray(lag_val, dtype=dt)
    lamAR = dt.type(lambdaAR)
    lam = dt.type(lambdaI) + lamAR
    thr = dt.type(c) * scale.astype(dt)
    Yr = Yrows.tocsr() if sparse else np.asarray(Yrows)
    out = W.copy()
    weights = np.ones(Yr.data.shape[0] if sparse else (T - first_row, n), dtype=dt)
    eye = np.eye(k, dtype=dt)
    for i in range(first_row, T):
        r = i - first_row
        if sparse:
            lo, hi = Yr.indptr[r], Yr.indptr[r + 1]
            cols, y = Yr.indices[lo:hi], Yr.data[lo:hi].astype(dt)
        elif missing:
            cols = np.nonzero(Yr[r])[0]
            y = Yr[r, cols].astype(dt)
        else:
            cols, y = np.arange(n), Yr[r].astype(dt)
        Hi, ti = H[cols], thr[cols]
        prior = np.sum(out[i - back] * theta, axis=0) if back.size else np.zeros(k, dtype=dt)
        w = prior
        om = np.ones(len(y), dtype=dt)
        for _ in range(sweeps):
            res = np.abs(y - Hi.dot(w))
            om = np.ones(len(y), dtype=dt)
            far = res > ti
            om[far] = ti[far] / res[far]
            Hw = Hi * om[:, None]
            A = Hw.T.dot(Hi) + lam * eye
            b = Hw.T.dot(y) + lamAR * prior
            try:
                if not np.all(np.isfinite(A)):
                    raise np.linalg.LinAlgError('not finite')
                L = np.linalg.cholesky(A)
                if not (np.all(np.isfinite(L)) and np.all(np.diagonal(L) > 0)):
                    raise np.linalg.LinAlgError('pivot')
            except np.linalg.LinAlgError:
                raise ValueError('robust_filter_rows: row {}: the weighted G + (lambdaI + lambdaAR) I is not positive definite'.format(i))
            w = scipy.linalg.cho_solve((L, True), b, check_finite=False)
        out[i] = w
        if sparse:
            weights[lo:hi] = om
        else:
            weights[r, cols] = om
    return out, weights


# ---- the fixed-interval smoother: the window's rows as the joint minimiser (trmf_session_smooth) ---------------------------------
def _window_guards(what, W, H, lag_set, Yrows, first_row):
    """filter_rows' guards under another name: (T, k, lags as int64, reach, first_row)."""
    T, k = W.shape
    back = np.asarray(lag_set).astype(np.int64)
    if back.size and back.min() == 0:
        raise ValueError('{}: the lag set contains lag 0 (a row would be its own prior)'.format(what))
    reach = int(back.max()) if back.size else 0
    first_row = int(first_row)
    if first_row < reach or first_row > T:
        raise ValueError('{}: first_row {} outside [{} (the largest lag), {} (rows)]'.format(what, first_row, reach, T))
    if Yrows.shape[0] != T - first_row or (T > first_row and Yrows.shape[1] != H.shape[0]):
        raise ValueError('{}: Yrows is {}, rows {}..{} of {} series were expected'.format(what, Yrows.shape, first_row, T, H.shape[0]))
    return T, k, back, reach, first_row


def _row_observations(Yr, r, sparse, missing, n, dt):
    """(columns, values) of row r of the window as filter_rows reads them."""
    if sparse:
        lo, hi = Yr.indptr[r], Yr.indptr[r + 1]
        cols, y = Yr.indices[lo:hi], Yr.data[lo:hi].astype(dt)
        if not missing:                                      # every series counts: absent entries read as 0
            full = np.zeros(n, dtype=dt)
            np.add.at(full, cols, y)
            cols, y = slice(None), full
        return cols, y
    if missing:
        cols = np.nonzero(Yr[r])[0]
        return cols, Yr[r, cols].astype(dt)
    return slice(None), Yr[r].astype(dt)


def _ar_operator(back, theta, m):
    """B as k banded m x m matrices (k, m, m): (B x)_i = x_i - sum_{l : i - lag_l >= 0} theta_l o x_{i - lag_l}, window indices."""
    k = theta.shape[1]
    B = np.zeros((k, m, m), dtype=theta.dtype)
    idx = np.arange(m)
    B[:, idx, idx] = 1
    for l, lag in enumerate(back):
        rows = idx[idx >= lag]
        if rows.size:
            B[:, rows, rows - lag] -= theta[l][:, None]
    return B


def smooth_rows(W, H, lag_set, lag_val, Yrows, first_row, lambdaI, lambdaAR, missing):
    """A copy of ``W`` (T x k) whose rows ``first_row .. T-1`` are the JOINT minimiser of the training objective restricted to
    them, with H, the lag weights and every earlier row fixed: the specification of ``trmf_session_smooth`` ::

        J_win = 1/2 sum_{i>=f} sum_{j in Omega_i} (y_ij - w_i . h_j)^2 + 1/2 lambdaI sum_{i>=f} |w_i|^2 + 1/2 lambdaAR sum_{i>=f} |e_i|^2
        e_i   = w_i - sum_l lag_val[l] * w_{i - lag_set[l]}                    (rows < f enter e_i as constants)

    Where ``filter_rows`` fits a row to its own observations and the rows before it, this also counts the AR penalties of the
    later rows in which the row appears.  The gradient is linear: with ``D`` the block diagonal of ``G_i + lambdaI I``, ``B`` the
    banded AR operator of the window and ``h`` the head rows' share of ``e``, the rows solve ``(D + lambdaAR B^T B) x = b +
    lambdaAR B^T h``; the system is assembled and solved directly by a (banded) Cholesky factorisation.  ``Yrows``, ``missing``,
    the dtype rule and the guards are ``filter_rows``'; a row whose ``G_i + (lambdaI + lambdaAR) I`` is not positive definite is
    refused by name as there (the device preconditions with these blocks)."""
    W = np.asarray(W)
    dt = W.dtype
    T, k, back, reach, first_row = _window_guards('smooth_rows', W, H, lag_set, Yrows, first_row)
    out = W.copy()
    m = T - first_row
    if m == 0:
        return out
    H = np.asarray(H, dtype=dt)
    theta = np.asarray(lag_val, dtype=dt).reshape(len(back), k)
    sparse = smat.issparse(Yrows)
    Yr = Yrows.tocsr() if sparse else np.asarray(Yrows)
    obs = [_row_observations(Yr, r, sparse, missing, H.shape[0], dt) for r in range(m)]
    out[first_row:] = _solve_window('smooth_rows', W, H, back, theta, reach, first_row, obs, None, dt.type(lambdaI), dt.type(lambdaAR))
    return out


def _solve_window(what, W, H, back, theta, reach, first_row, obs, omega, lamI, lamAR):
    """The window's rows (m x k) solving ``(D + lambdaAR B^T B) x = b + lambdaAR B^T h`` by a banded Cholesky factorisation, with
    ``G_i = sum_j omega_ij h_j h_j^T`` and ``b_i = sum_j omega_ij y_ij h_j`` (``omega`` None: every weight 1).  ``obs[r]``: (columns,
    values) of window row r; ``omega[r]``: its weights."""
    dt = W.dtype
    T, k = W.shape
    m = T - first_row
    eye = np.eye(k, dtype=dt)
    A4 = np.zeros((m, k, m, k), dtype=dt)
    rhs = np.zeros((m, k), dtype=dt)
    head = np.zeros((m, k), dtype=dt)                        # the head rows' share of e: e = B x - head
    for r in range(m):
        i = first_row + r
        cols, y = obs[r]
        Hi = H[cols]
        Hw = Hi if omega is None else Hi * omega[r][:, None]
        G = Hw.T.dot(Hi)
        block = G + (lamI + lamAR) * eye
        try:
            if not np.all(np.isfinite(block)):
                raise np.linalg.LinAlgError('not finite')
            L = np.linalg.cholesky(block)
            if not (np.all(np.isfinite(L)) and np.all(np.diagonal(L) > 0)):
                raise np.linalg.LinAlgError('pivot')
        except np.linalg.LinAlgError:
            raise ValueError('{}: row {}: {}G + (lambdaI + lambdaAR) I is not positive definite'.format(what, i, '' if omega is None else 'the weighted '))
        A4[r, :, r, :] = G + lamI * eye
        rhs[r] = Hw.T.dot(y)
        for l, lag in enumerate(back):
            if r - lag < 0:
                head[r] += theta[l] * W[i - lag]
    B = _ar_operator(back, theta, m)
    dims = np.arange(k)
    A4[:, dims, :, dims] += lamAR * np.einsum('cji,cjl->cil', B, B)
    rhs += lamAR * np.einsum('cji,jc->ic', B, head)
    N = m * k
    A = A4.reshape(N, N)
    u = min(N - 1, reach * k + k - 1)                        # the half bandwidth in (row, dimension) order
    ab = np.zeros((u + 1, N), dtype=dt)
    for d in range(u + 1):
        ab[u - d, d:] = np.diagonal(A, d)
    try:
        cb = scipy.linalg.cholesky_banded(ab, lower=False, check_finite=True)
    except (np.linalg.LinAlgError, ValueError):
        raise ValueError('{}: the system of rows {}..{} is not positive definite'.format(what, first_row, T))
    return scipy.linalg.cho_solve_banded((cb, False), rhs.reshape(N), check_finite=False).reshape(m, k)


def window_objective(W, H, lag_set, lag_val, Yrows, first_row, lambdaI, lambdaAR, missing):
    """``J_win`` of ``smooth_rows`` for the rows of ``W`` as they are, in float64 (``objective_before`` / ``objective_after`` of
    ``trmf_session_smooth``; canonical rows: no cell stored twice)."""
    W = np.asarray(W, dtype=np.float64)
    T, k, back, reach, first_row = _window_guards('window_objective', W, H, lag_set, Yrows, first_row)
    H = np.asarray(H, dtype=np.float64)
    theta = np.asarray(lag_val, dtype=np.float64).reshape(len(back), k)
    sparse = smat.issparse(Yrows)
    Yr = Yrows.tocsr() if sparse else np.asarray(Yrows)
    fit = ridge = ar = 0.0
    for i in range(first_row, T):
        cols, y = _row_observations(Yr, i - first_row, sparse, missing, H.shape[0], np.dtype(np.float64))
        res = y - H[cols].dot(W[i])
        e = W[i] - np.sum(W[i - back] * theta, axis=0) if back.size else W[i]
        fit += float(res.dot(res)); ridge += float(W[i].dot(W[i])); ar += float(e.dot(e))
    return 0.5 * (fit + float(lambdaI) * ridge + float(lambdaAR) * ar)


# ---- the robust fixed-interval smoother: the smoother on Huber's loss (trmf_session_smooth_robust) --------------------------------
def _robust_guards(what, n, Yrows, missing, scale, c, sweeps):
    """robust_filter_rows' guards under another name: (scale as float64 (n,), c, sweeps)."""
    if smat.issparse(Yrows) and not missing:
        raise ValueError('{}: sparse rows without missing are not covered (an absent entry would be an observation '
                         'without a slot to report its weight in); pass the rows as an array'.format(what))
    scale = np.asarray(scale, dtype=np.float64)
    if scale.ndim == 0:
        scale = np.full(n, float(scale))
    if scale.shape != (n,):
        raise ValueError('{}: scale has shape {}, one value per series ({}) was expected'.format(what, scale.shape, n))
    bad = np.flatnonzero(~(np.isfinite(scale) & (scale > 0)))
    if bad.size:
        raise ValueError('{}: scale[{}] = {!r} is not finite and positive'.format(what, int(bad[0]), float(scale[bad[0]])))
    c = float(c)
    if not c > 0:
        raise ValueError('{}: c must be positive (inf: every cell weighted fully), not {!r}'.format(what, c))
    sweeps = int(sweeps)
    if sweeps < 1:
        raise ValueError('{}: sweeps must be at least 1, not {}'.format(what, sweeps))
    return scale, c, sweeps


def robust_smooth_rows(W, H, lag_set, lag_val, Yrows, first_row, lambdaI, lambdaAR, missing, scale, c=3.0, sweeps=4):
    """``smooth_rows`` on Huber's loss: the specification of ``trmf_session_smooth_robust``.  With ``t_j = c * scale[j]`` ::

        J_rob = sum_{i>=f} sum_{j in Omega_i} rho_{t_j}(y_ij - w_i . h_j) + 1/2 lambdaI sum_{i>=f} |w_i|^2 + 1/2 lambdaAR sum_{i>=f} |e_i|^2
        rho_t(r) = 1/2 r^2 if |r| <= t,  t |r| - 1/2 t^2 otherwise
        x^0 = the rows f .. as they stand;  for s = 1 .. sweeps:
            omega_ij = t_j / |r_ij| if |r_ij| > t_j else 1,   r_ij = y_ij - x^{s-1}_i . h_j
            x^s = smooth_rows' system with G_i = sum_j omega_ij h_j h_j^T, b_i = sum_j omega_ij y_ij h_j, solved directly

    (iteratively reweighted least squares: every sweep minimises a quadratic majoriser of ``J_rob``, so ``J_rob`` never rises; a
    fixed number of sweeps, no convergence test).  Returns ``(W_out, weights)``: the weights of the LAST sweep (formed from
    ``x^{sweeps-1}``) in ``robust_filter_rows``' layout.  ``c = inf`` is ``smooth_rows``.  The guards are ``smooth_rows``' and
    ``robust_filter_rows``'."""
    W = np.asarray(W)
    dt = W.dtype
    T, k, back, reach, first_row = _window_guards('robust_smooth_rows', W, H, lag_set, Yrows, first_row)
    n = H.shape[0]
    scale, c, sweeps = _robust_guards('robust_smooth_rows', n, Yrows, missing, scale, c, sweeps)
    sparse = smat.issparse(Yrows)
    Yr = Yrows.tocsr() if sparse else np.asarray(Yrows)
    m = T - first_row
    out = W.copy()
    weights = np.ones(Yr.data.shape[0] if sparse else (m, n), dtype=dt)
    if m == 0:
        return out, weights
    H = np.asarray(H, dtype=dt)
    theta = np.asarray(lag_val, dtype=dt).reshape(len(back), k)
    thr = dt.type(c) * scale.astype(dt)
    obs = []
    for r in range(m):
        cols, y = _row_observations(Yr, r, sparse, missing, n, dt)
        obs.append((np.arange(n) if isinstance(cols, slice) else cols, y))
    omega = None
    for _ in range(sweeps):
        omega = []
        for r, (cols, y) in enumerate(obs):
            res = np.abs(y - H[cols].dot(out[first_row + r]))
            om = np.ones(len(y), dtype=dt)
            far = res > thr[cols]
            om[far] = thr[cols][far] / res[far]
            omega.append(om)
        out[first_row:] = _solve_window('robust_smooth_rows', out, H, back, theta, reach, first_row, obs, omega, dt.type(lambdaI), dt.type(lambdaAR))
    for r, (cols, y) in enumerate(obs):
        if sparse:
            weights[Yr.indptr[r]:Yr.indptr[r + 1]] = omega[r]
        else:
            weights[r, cols] = omega[r]
    return out, weights


def robust_window_objective(W, H, lag_set, lag_val, Yrows, first_row, lambdaI, lambdaAR, missing, scale, c=3.0):
    """``J_rob`` of ``robust_smooth_rows`` for the rows of ``W`` as they are, in float64 (``objective_before`` / ``objective_after``
    of ``trmf_session_smooth_robust``).  ``c = inf`` is ``window_objective``."""
    W = np.asarray(W, dtype=np.float64)
    T, k, back, reach, first_row = _window_guards('robust_window_objective', W, H, lag_set, Yrows, first_row)
    n = H.shape[0]
    scale, c, _ = _robust_guards('robust_window_objective', n, Yrows, missing, scale, c, 1)
    H = np.asarray(H, dtype=np.float64)
    theta = np.asarray(lag_val, dtype=np.float64).reshape(len(back), k)
    thr = c * scale
    sparse = smat.issparse(Yrows)
    Yr = Yrows.tocsr() if sparse else np.asarray(Yrows)
    fit = ridge = ar = 0.0
    for i in range(first_row, T):
        cols, y = _row_observations(Yr, i - first_row, sparse, missing, n, np.dtype(np.float64))
        res = np.abs(y - H[cols].dot(W[i]))
        t = thr[cols]
        with np.errstate(invalid='ignore'):
            rho = np.where(res > t, t * res - 0.5 * t * t, 0.5 * res * res)
        e = W[i] - np.sum(W[i - back] * theta, axis=0) if back.size else W[i]
        fit += float(rho.sum()); ridge += float(W[i].dot(W[i])); ar += float(e.dot(e))
    return fit + 0.5 * (float(lambdaI) * ridge + float(lambdaAR) * ar)


# ---- the sliding window (trmf_session_slide) ------------------------------------------------------------------------------------
def slide_entries(rows, cols, vals, retire):
    """What a stored list of entries becomes when the ``retire`` oldest rows leave: the entries with ``rows >= retire`` in their
    STORED order (a stable filter -- the lists need not be sorted and a cell may be stored twice), row numbers reduced by
    ``retire``.  Applied to the (row index, column index, value) arrays of either orientation of a session's Y it gives the arrays
    of the session after ``slide``.  Returns ``(rows, cols, vals)`` as new arrays."""
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals)
    retire = int(retire)
    if retire < 0:
        raise ValueError('slide_entries: retire must not be negative, not {}'.format(retire))
    if not (rows.shape == cols.shape == vals.shape and rows.ndim == 1):
        raise ValueError('slide_entries: rows, cols and vals must be one-dimensional arrays of one length')
    keep = rows >= retire
    return rows[keep] - rows.dtype.type(retire), cols[keep].copy(), vals[keep].copy()


# ---- series churn (trmf_session_change_series) -----------------------------------------------------------------------------------
def churn_entries(rows, cols, vals, keep, n, block=None, major='row'):
    """What a stored list of entries becomes when series leave and a block of new series joins: the stored-order rule of
    ``trmf_session_change_series``.  ``keep`` is a mask of ``n`` flags (``None``: every series stays); the kept series keep their
    relative order and are renumbered densely from 0.  The entries of kept series survive in their STORED order with the new
    numbers (a stable filter -- the lists need not be sorted and a cell may be stored twice).  ``block = (rows, cols, vals)``
    holds the entries of the new series, numbered from 0 within the block, in the stored order of the same orientation: they
    get the numbers ``n_kept + cols`` and are merged stably behind the survivors of the same ``major`` index -- ``major='row'``
    (the CSR arrays: every row is its survivors, then the block's entries of that row) or ``major='col'`` (the CSC arrays: the
    kept columns in order, each as stored, then the block's columns as delivered).  Without a block the survivors are returned
    as filtered, whatever their order.  Returns ``(rows, cols, vals)`` as new arrays."""
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals)
    n = int(n)
    if not (rows.shape == cols.shape == vals.shape and rows.ndim == 1):
        raise ValueError('churn_entries: rows, cols and vals must be one-dimensional arrays of one length')
    if major not in ('row', 'col'):
        raise ValueError("churn_entries: major must be 'row' or 'col', not {!r}".format(major))
    if keep is None:
        keep = np.ones(n, dtype=bool)
    keep = np.asarray(keep)
    if keep.shape != (n,):
        raise ValueError('churn_entries: keep must hold {} flags, not {}'.format(n, keep.shape))
    keep = keep.astype(bool)
    if cols.size and (cols.min() < 0 or cols.max() >= n):
        raise ValueError('churn_entries: a column index lies outside 0..{}'.format(n - 1))
    remap = np.cumsum(keep) - 1
    stay = keep[cols] if cols.size else np.zeros(0, dtype=bool)
    r, c, v = rows[stay].copy(), remap[cols[stay]].astype(cols.dtype), vals[stay].copy()
    if block is None:
        return r, c, v
    br, bc, bv = (np.asarray(a) for a in block)
    if not (br.shape == bc.shape == bv.shape and br.ndim == 1):
        raise ValueError('churn_entries: the block must be three one-dimensional arrays of one length')
    if bc.size and bc.min() < 0:
        raise ValueError('churn_entries: a column index of the block is negative')
    nk = int(np.count_nonzero(keep))
    r = np.concatenate([r, br.astype(r.dtype)]); c = np.concatenate([c, (bc + nk).astype(c.dtype)]); v = np.concatenate([v, bv.astype(v.dtype)])
    order = np.argsort(r if major == 'row' else c, kind='stable')
    return r[order], c[order], v[order]


# ---- cell revisions (trmf_session_revise) -----------------------------------------------------------------------------------------
def _revise_edits(edits, what):
    """``edits`` as ``(rows, cols, vals, delete)``: int64 cells, values (zeros where none were given), a boolean mask."""
    if len(edits) not in (3, 4):
        raise ValueError('{}: edits must be (rows, cols, vals) or (rows, cols, vals, delete)'.format(what))
    er, ec = np.asarray(edits[0]).astype(np.int64), np.asarray(edits[1]).astype(np.int64)
    dl = np.zeros(er.shape, dtype=bool) if len(edits) == 3 or edits[3] is None else np.asarray(edits[3]).astype(bool)
    ev = np.zeros(er.shape) if edits[2] is None else np.asarray(edits[2])
    if not (er.shape == ec.shape == ev.shape == dl.shape and er.ndim == 1):
        raise ValueError('{}: the edits must be one-dimensional arrays of one length'.format(what))
    if edits[2] is None and not dl.all():
        raise ValueError('{}: vals is needed (the batch holds sets)'.format(what))
    if er.size and (er.min() < 0 or ec.min() < 0):
        raise ValueError('{}: an edit names a negative index'.format(what))
    if np.unique(np.stack([er, ec]), axis=1).shape[1] != er.size:
        raise ValueError('{}: a cell is named twice in one batch'.format(what))
    return er, ec, ev, dl


def revise_entries(rows, cols, vals, edits, major='row', return_counts=False):
    """What a stored list of entries becomes when cells are set or deleted: the stored-order rule of ``trmf_session_revise``.
    ``edits = (rows, cols, vals)`` or ``(rows, cols, vals, delete)`` names distinct cells; ``delete`` flags the ones that leave
    (``None``: every edit is a set; ``vals`` may be ``None`` when all are deletes).  EVERY stored copy of an edited cell is
    removed -- a stable filter: the other entries keep their stored order, the lists need not be sorted and a cell may be stored
    twice -- and each set then places one entry behind the survivors of its ``major`` index: ``major='row'`` (the CSR arrays: the
    sets of a row follow it in ascending column order) or ``major='col'`` (the CSC arrays: the sets of a column follow it in
    ascending row order).  The result therefore depends on the set of edits, not on their order.  The lists are expected in the
    stored order of that orientation (grouped by the major index).  Returns ``(rows, cols, vals)`` as new arrays; with
    ``return_counts`` also ``{'inserted', 'replaced', 'deleted', 'missed', 'copies_removed'}``: a set of a stored cell replaces,
    of an unstored one inserts; a delete of an unstored cell is a no-op counted in ``missed``; ``copies_removed`` counts the
    stored entries that left (a cell stored twice counts twice)."""
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals)
    if not (rows.shape == cols.shape == vals.shape and rows.ndim == 1):
        raise ValueError('revise_entries: rows, cols and vals must be one-dimensional arrays of one length')
    if major not in ('row', 'col'):
        raise ValueError("revise_entries: major must be 'row' or 'col', not {!r}".format(major))
    er, ec, ev, dl = _revise_edits(edits, 'revise_entries')
    span = int(max(cols.max() if cols.size else 0, ec.max() if ec.size else 0)) + 1
    key, ekey = rows.astype(np.int64) * span + cols.astype(np.int64), er * span + ec
    order = np.argsort(ekey, kind='stable')
    pos = np.searchsorted(ekey[order], key)
    hit = (pos < ekey.size) & (ekey[order][np.minimum(pos, max(ekey.size - 1, 0))] == key) if ekey.size else np.zeros(key.shape, dtype=bool)
    stay = ~hit
    sets = np.flatnonzero(~dl)
    sets = sets[np.lexsort((ec[sets], er[sets]) if major == 'row' else (er[sets], ec[sets]))]
    r = np.concatenate([rows[stay], er[sets].astype(rows.dtype)])
    c = np.concatenate([cols[stay], ec[sets].astype(cols.dtype)])
    v = np.concatenate([vals[stay], ev[sets].astype(vals.dtype)])
    merged = np.argsort(r if major == 'row' else c, kind='stable')
    out = (r[merged], c[merged], v[merged])
    if not return_counts:
        return out
    copies = np.bincount(pos[hit], minlength=ekey.size)[np.argsort(order, kind='stable')] if ekey.size else np.zeros(0, dtype=np.int64)
    stored = copies > 0
    counts = {'inserted': int(np.count_nonzero(~dl & ~stored)), 'replaced': int(np.count_nonzero(~dl & stored)),
              'deleted': int(np.count_nonzero(dl & stored)), 'missed': int(np.count_nonzero(dl & ~stored)), 'copies_removed': int(copies.sum())}
    return out + (counts,)


# ---- online loading updates: the rows of H refitted from new rows (trmf_session_series_stats_init / _adapt_series) ---------------
def _series_entries(Y, missing):
    """Per series the (timestamps, values) of its observations in stored order.  Sparse ``Y``: the stored entries of the column
    (a cell stored twice is two observations); an array: its non-zeros with ``missing``, every row without."""
    n = Y.shape[1]
    if smat.issparse(Y):
        Yc = Y if Y.format == 'csc' else Y.tocsc()
        return [(Yc.indices[Yc.indptr[j]:Yc.indptr[j + 1]].astype(np.int64), Yc.data[Yc.indptr[j]:Yc.indptr[j + 1]]) for j in range(n)]
    Ya = np.asarray(Y)
    if missing:
        return [(np.nonzero(Ya[:, j])[0], Ya[np.nonzero(Ya[:, j])[0], j]) for j in range(n)]
    rows = np.arange(Ya.shape[0])
    return [(rows, Ya[:, j]) for j in range(n)]


def _check_forget(forget, what):
    forget = float(forget)
    if not (0.0 < forget <= 1.0):
        raise ValueError('{}: forget must lie in (0, 1], not {!r}'.format(what, forget))
    return forget


def _ridge_solve(S, r, lam, j, what):
    """(S + lam I)^-1 r.  The Cholesky factorisation decides whether the system is positive definite (the device's test); the
    solution is LAPACK's general solve (LU with partial pivoting, residual-stable row by row), which on the ridge-conditioned
    systems of a series with fewer entries than unknowns lands closer to the exact solution than the two triangular solves do."""
    A = S + lam * np.eye(S.shape[0], dtype=S.dtype)
    try:
        if not np.all(np.isfinite(A)):
            raise np.linalg.LinAlgError('not finite')
        L = np.linalg.cholesky(A)
        if not (np.all(np.isfinite(L)) and np.all(np.diagonal(L) > 0)):
            raise np.linalg.LinAlgError('pivot')
    except np.linalg.LinAlgError:
        raise ValueError('{}: series {}: S + lambdaI I is not positive definite'.format(what, j))
    return np.linalg.solve(A, r)


def series_ridge(W, Y, lambdaI, forget=1.0, missing=True):
    """The loadings the history asks for with ``W`` (T x k) as it is: the specification of ``trmf_session_adapt_series``.  Per
    series ``j`` the weighted ridge ::

        S_j = sum_t om_t w_t w_t^T,   r_j = sum_t om_t y_tj w_t,   om_t = forget^(T - 1 - t),   h_j = (S_j + lambdaI I)^-1 r_j

    over the stored entries of column ``j`` of a sparse ``Y`` (a cell stored twice is two observations) or the non-zeros of an
    array (``missing``); without ``missing`` ``S`` is shared, the sum over every row, an absent entry reading as 0.
    ``forget == 1`` is the training F-solve for the current ``W``.  All arithmetic is in the dtype of ``W``; ``lambdaI`` is cast
    to it, and the ridge is not decayed.  Returns H (n x k).  ``ValueError`` for ``forget`` outside (0, 1], a row count that does
    not match, or a series whose system is not positive definite (possible only with ``lambdaI == 0``; the message names it)."""
    W = np.asarray(W)
    dt = W.dtype
    T, k = W.shape
    forget = _check_forget(forget, 'series_ridge')
    if Y.shape[0] != T:
        raise ValueError('series_ridge: Y has {} rows, W {}'.format(Y.shape[0], T))
    lam = dt.type(lambdaI)
    om = (forget ** (T - 1 - np.arange(T, dtype=np.float64))).astype(dt)
    H = np.zeros((Y.shape[1], k), dtype=dt)
    Sall = (W * om[:, None]).T.dot(W) if not missing else None
    for j, (rows, y) in enumerate(_series_entries(Y, missing)):
        Wj = W[rows] * om[rows][:, None]
        S = Wj.T.dot(W[rows]) if missing else Sall
        H[j] = _ridge_solve(S, Wj.T.dot(np.asarray(y, dtype=dt)), lam, j, 'series_ridge')
    return H


class SeriesStats(object):
    """``series_ridge`` as a recursion -- recursive least squares with forgetting, the form the device keeps resident: ``S_j`` and
    ``r_j`` per series (one shared ``S`` without ``missing``), built over ``Y`` with ``W`` as it is, then grown block by block ::

        S <- forget^m S + sum_new forget^(T - 1 - t) w_t w_t^T        (r likewise; m new rows, T the new row count)

    one rank-1 update per entry in stored order, as the device adds them, all in the dtype of ``W``.  ``solve(lambdaI)`` gives
    the loadings.  With
    ``forget == 1`` it equals ``series_ridge`` over the grown matrix up to the summation order; in float32 it is the yardstick
    the device is held to."""

    def __init__(self, W, Y, forget=1.0, missing=True):
        W = np.asarray(W)
        self.forget = _check_forget(forget, 'SeriesStats')
        self.missing = bool(missing)
        self.dtype = W.dtype
        self.k = W.shape[1]
        self.n = Y.shape[1]
        self.rows = 0
        self.S = np.zeros((self.n if self.missing else 1, self.k, self.k), dtype=self.dtype)
        self.r = np.zeros((self.n, self.k), dtype=self.dtype)
        self.absorb(W, Y)

    def absorb(self, W, Ynew):
        """Absorb the rows ``self.rows .. T-1`` of ``W`` (T x k, as it is now) with their observations ``Ynew`` (T - self.rows rows)."""
        W = np.asarray(W)
        T = W.shape[0]
        m = T - self.rows
        if W.shape[1] != self.k or W.dtype != self.dtype:
            raise ValueError('SeriesStats.absorb: W is {} {}, {} columns of {} were expected'.format(W.shape, W.dtype, self.k, self.dtype))
        if m < 0 or Ynew.shape[0] != m or Ynew.shape[1] != self.n:
            raise ValueError('SeriesStats.absorb: Ynew is {}, rows {}..{} of {} series were expected'.format(Ynew.shape, self.rows, T, self.n))
        dt = self.dtype
        decay = dt.type(self.forget ** m)
        self.S *= decay
        self.r *= decay
        om = (self.forget ** (m - 1 - np.arange(m, dtype=np.float64))).astype(dt)
        Wn = W[self.rows:]
        if not self.missing:
            for t in range(m):
                self.S[0] += np.outer(om[t] * Wn[t], Wn[t])
        for j, (rows, y) in enumerate(_series_entries(Ynew, self.missing)):
            y = np.asarray(y, dtype=dt)
            for e, t in enumerate(rows):
                aw = om[t] * Wn[t]
                if self.missing:
                    self.S[j] += np.outer(aw, Wn[t])
                self.r[j] += aw * y[e]
        self.rows = T
        return self

    def retire(self, W, Y, count, downdate=True):
        """The sliding-window form (``trmf_session_slide``): the ``count`` oldest of the absorbed rows leave.  ``W`` (``self.rows``
        x k or longer) and ``Y`` (at least ``count`` rows) are the factor and the observations of BEFORE the retirement, row 0 the
        oldest.  With ``downdate`` every retired entry's term is subtracted, ::

            S_j <- S_j - om_t w_t w_t^T,   r_j <- r_j - om_t y_tj w_t,   om_t = forget^(rows - 1 - t),   t < count

        one rank-1 update per entry in stored order (the absorb step with the sign of the weight flipped), in the dtype of ``W``:
        the tables then describe the retained rows alone.  Without it the tables keep the retired rows as exponentially forgotten
        history (recursive least squares as usually run, the natural choice for ``forget < 1``).  Either way ``self.rows`` drops by
        ``count``, so that the next ``absorb`` takes the rows after the retained ones."""
        W = np.asarray(W)
        count = int(count)
        if count < 0 or count > self.rows:
            raise ValueError('SeriesStats.retire: count {} outside 0..{} (the absorbed rows)'.format(count, self.rows))
        if W.shape[1] != self.k or W.dtype != self.dtype or W.shape[0] < count:
            raise ValueError('SeriesStats.retire: W is {} {}, at least {} rows of {} columns of {} were expected'.format(W.shape, W.dtype, count, self.k, self.dtype))
        if Y.shape[0] < count or Y.shape[1] != self.n:
            raise ValueError('SeriesStats.retire: Y is {}, at least {} rows of {} series were expected'.format(Y.shape, count, self.n))
        if downdate and count:
            dt = self.dtype
            om = (-(self.forget ** (self.rows - 1 - np.arange(count, dtype=np.float64)))).astype(dt)
            if not self.missing:
                for t in range(count):
                    self.S[0] += np.outer(om[t] * W[t], W[t])
            for j, (rows, y) in enumerate(_series_entries(Y, self.missing)):
                y = np.asarray(y, dtype=dt)
                for e, t in enumerate(rows):
                    if t >= count:
                        continue
                    aw = om[t] * W[t]
                    if self.missing:
                        self.S[j] += np.outer(aw, W[t])
                    self.r[j] += aw * y[e]
        self.rows -= count
        return self

    def revise(self, W, Y, edits):
        """The cell-revision form (``trmf_session_revise`` with ``update_stats``): cells of the absorbed rows are set or deleted.
        ``W`` (``self.rows`` x k, as it is now) and ``Y`` (the observations of BEFORE the edit, every row absorbed) as for
        ``retire``; ``edits = (rows, cols, vals)`` or ``(rows, cols, vals, delete)`` as for ``trmf.revise_entries``.  Per touched
        series every stored entry of an edited cell is subtracted in stored order, then the sets are added in ascending row order ::

            S_j <- S_j -/+ om_t w_t w_t^T,   r_j <- r_j -/+ om_t y w_t,   om_t = forget^(rows - 1 - t)

        one rank-1 update per entry in the dtype of ``W`` (the absorb step; the sign of the weight flipped for the removed
        entries): the tables then describe the revised matrix.  Per-series tables only (``missing``)."""
        W = np.asarray(W)
        if not self.missing:
            raise ValueError('SeriesStats.revise: per-series statistics only (missing); the full-observation forms share one S')
        if W.shape != (self.rows, self.k) or W.dtype != self.dtype:
            raise ValueError('SeriesStats.revise: W is {} {}, {} x {} of {} was expected'.format(W.shape, W.dtype, self.rows, self.k, self.dtype))
        if Y.shape != (self.rows, self.n):
            raise ValueError('SeriesStats.revise: Y is {}, {} x {} (every row absorbed) was expected'.format(Y.shape, self.rows, self.n))
        er, ec, ev, dl = _revise_edits(edits, 'SeriesStats.revise')
        if er.size and (er.max() >= self.rows or ec.max() >= self.n):
            raise ValueError('SeriesStats.revise: an edit lies outside {} x {}'.format(self.rows, self.n))
        dt = self.dtype
        om = (self.forget ** (self.rows - 1 - np.arange(self.rows, dtype=np.float64))).astype(dt)
        columns = _series_entries(Y, True)
        for j in np.unique(ec):
            mine = np.flatnonzero(ec == j)
            mine = mine[np.argsort(er[mine], kind='stable')]
            rows, y = columns[j]
            y = np.asarray(y, dtype=dt)
            gone = set(int(t) for t in er[mine])
            for e, t in enumerate(rows):
                if int(t) in gone:
                    aw = -om[t] * W[t]
                    self.S[j] += np.outer(aw, W[t])
                    self.r[j] += aw * y[e]
            for e in mine:
                if not dl[e]:
                    t = er[e]
                    aw = om[t] * W[t]
                    self.S[j] += np.outer(aw, W[t])
                    self.r[j] += aw * dt.type(ev[e])
        return self

    def solve(self, lambdaI):
        lam = self.dtype.type(lambdaI)
        H = np.zeros((self.n, self.k), dtype=self.dtype)
        for j in range(self.n):
            H[j] = _ridge_solve(self.S[j if self.missing else 0], self.r[j], lam, j, 'SeriesStats.solve')
        return H

    def _robust_block(self, what, W, Ynew, H):
        """The guards of ``absorb_robust`` / ``robust_series_objective``: (W, H in the tables' dtype, m, decay, om, W's new rows)."""
        if not self.missing:
            raise ValueError('{}: the full-observation form keeps one shared S for all series; a weight per cell needs a table per '
                             'series (missing=True)'.format(what))
        W = np.asarray(W)
        T = W.shape[0]
        m = T - self.rows
        if W.shape[1] != self.k or W.dtype != self.dtype:
            raise ValueError('{}: W is {} {}, {} columns of {} were expected'.format(what, W.shape, W.dtype, self.k, self.dtype))
        if m < 0 or Ynew.shape[0] != m or Ynew.shape[1] != self.n:
            raise ValueError('{}: Ynew is {}, rows {}..{} of {} series were expected'.format(what, Ynew.shape, self.rows, T, self.n))
        H = np.asarray(H)
        if H.shape != (self.n, self.k):
            raise ValueError('{}: H is {}, {} were expected'.format(what, H.shape, (self.n, self.k)))
        dt = self.dtype
        decay = dt.type(self.forget ** m)
        om = (self.forget ** (m - 1 - np.arange(m, dtype=np.float64))).astype(dt)
        return W, H, m, decay, om, W[self.rows:]

    def absorb_robust(self, W, Ynew, H, lambdaI, scale, c=3.0, sweeps=4):
        """``absorb`` + ``solve`` with Huber weights on the new entries: the specification of ``trmf_session_adapt_series_robust``.
        Per series ``j``, with ``d = forget^m``, ``om_t`` as in ``absorb``, ``tau_j = c * scale[j]`` and ``h^0 = H[j]`` ::

            for s = 1 .. sweeps:   res_e = y_e - w_t . h^{s-1},   u_e = 1 if |res_e| <= tau_j else tau_j / |res_e|      (e: the new entries)
                                   S^s = d S_j + sum_e (u_e om_t) w_t w_t^T,   r^s = d r_j + sum_e (u_e om_t) y_e w_t
                                   h^s = (S^s + lambdaI I)^-1 r^s

        Every sweep restarts from the decayed old tables; only the new entries are reweighted (iteratively reweighted least
        squares: ``robust_series_objective`` never rises).  The tables become those of the last sweep, so that ``solve(lambdaI)``
        returns the loadings returned here and a later ``absorb`` continues from them.  One rank-1 update per entry in stored
        order, all in the dtype of ``W``.  Returns ``(Hnew, weights)``: the weights of the last sweep as a CSC matrix of shape
        ``m x n`` holding one value per stored entry of ``Ynew`` (a cell stored twice keeps two).  ``c = inf`` is ``absorb`` +
        ``solve``, bit for bit.  A series without a new entry runs one sweep.  ``ValueError`` in ``absorb``'s cases, for tables
        without ``missing``, and for ``scale``, ``c``, ``sweeps`` as ``robust_filter_rows``."""
        W, H, m, decay, om, Wn = self._robust_block('SeriesStats.absorb_robust', W, Ynew, H)
        scale, c, sweeps = _robust_guards('SeriesStats.absorb_robust', self.n, Ynew, True, scale, c, sweeps)
        dt = self.dtype
        H = H.astype(dt)
        thr = dt.type(c) * scale.astype(dt)
        Hnew = np.zeros((self.n, self.k), dtype=dt)
        lam = dt.type(lambdaI)
        S_out, r_out = np.empty_like(self.S), np.empty_like(self.r)
        indptr, rows_out, data = np.zeros(self.n + 1, dtype=np.int64), [], []
        for j, (rows, y) in enumerate(_series_entries(Ynew, True)):
            y = np.asarray(y, dtype=dt)
            h = H[j]
            u = np.ones(len(y), dtype=dt)
            for _ in range(sweeps if len(y) else 1):
                res = np.abs(y - Wn[rows].dot(h)) if len(y) else np.zeros(0, dtype=dt)
                u = np.ones(len(y), dtype=dt)
                far = res > thr[j]
                u[far] = thr[j] / res[far]
                S, r = self.S[j] * decay, self.r[j] * decay
                for e, t in enumerate(rows):
                    aw = (u[e] * om[t]) * Wn[t]
                    S += np.outer(aw, Wn[t])
                    r += aw * y[e]
                h = _ridge_solve(S, r, lam, j, 'SeriesStats.absorb_robust')
            S_out[j], r_out[j], Hnew[j] = S, r, h
            indptr[j + 1] = indptr[j] + len(y)
            rows_out.append(np.asarray(rows, dtype=np.int64)); data.append(u)
        self.S, self.r, self.rows = S_out, r_out, W.shape[0]
        weights = smat.csc_matrix((np.concatenate(data) if data else np.zeros(0, dtype=dt),
                                   np.concatenate(rows_out).astype(np.int32) if rows_out else np.zeros(0, dtype=np.int32), indptr.astype(np.int32)), shape=(m, self.n))
        return Hnew, weights


def robust_series_objective(stats, W, Ynew, H, lambdaI, scale, c=3.0):
    """``sum_j J_j(H[j])`` of ``SeriesStats.absorb_robust`` in float64, for tables ``stats`` that have NOT yet absorbed the rows
    ``stats.rows .. T-1`` of ``W`` with their observations ``Ynew`` (``objective_before`` / ``objective_after`` of
    ``trmf_session_adapt_series_robust``) ::

        J_j(h) = h^T (d S_j + lambdaI I) h - 2 h . (d r_j) + sum_e om_t rho_tau(y_e - w_t . h),   rho_tau(x) = x^2 (|x| <= tau), 2 tau |x| - tau^2

    The decayed tables ``d S_j``, ``d r_j`` are formed in the tables' dtype, as the update reads them.  ``c = inf``: the weighted
    least-squares objective of ``absorb`` + ``solve`` (up to the constant ``sum y^2`` of the history)."""
    W, H, m, decay, om, Wn = stats._robust_block('robust_series_objective', W, Ynew, H)
    scale, c, _ = _robust_guards('robust_series_objective', stats.n, Ynew, True, scale, c, 1)
    tau = c * scale
    lam = float(stats.dtype.type(lambdaI))
    H64, W64 = np.asarray(H, dtype=np.float64), np.asarray(Wn, dtype=np.float64)
    total = 0.0
    for j, (rows, y) in enumerate(_series_entries(Ynew, True)):
        h = H64[j]
        S, r = (stats.S[j] * decay).astype(np.float64), (stats.r[j] * decay).astype(np.float64)
        J = float(h.dot(S.dot(h)) + lam * h.dot(h) - 2.0 * h.dot(r))
        if len(y):
            res = np.abs(np.asarray(y, dtype=np.float64) - W64[rows].dot(h))
            with np.errstate(invalid='ignore'):
                rho = np.where(res > tau[j], 2.0 * tau[j] * res - tau[j] * tau[j], res * res)
            J += float((om[rows].astype(np.float64) * rho).sum())
        total += J
    return total
