"""Shared by tests/test_smooth_robust_host.py and tests/test_gpu_smooth_robust.py: the inputs of the robust smoother's tests, the
fp64 truth (trmf.robust_smooth_rows: every sweep solved directly) and the IRLS twin -- the device's computation in NumPy in the
element type, every sweep solved by the smoother's PCG with the weighted blocks -- whose own distance from the truth is the
yardstick the device is gated by (test infrastructure).

The inputs are the ones the robust filter and the smoother are held to: robust_helpers.case_a (every rank, the three lambda pairs,
windows from rows 72 and 40), robust_helpers.case_b (designed row lengths, a window from row 16, run with slices of 64), one dense
missing=False case and the 70-lag geometry; c = 1.5, four sweeps, scale = plain_scale, started from the set's own W."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as smat

import online_helpers as OH
import robust_helpers as RH
import smooth_helpers as SH

C, SWEEPS = RH.C, RH.SWEEPS
BORDER = RH.BORDER
DOWN_MIN, DOWN_MAX, BORDER_MAX = 0.01, 0.97, 0.01            # what a case must meet to check anything


def _rows(d, first, dtype, storage):
    rows = OH.rows_of(d['Y'], first, d['Y'].shape[0], dtype)
    return rows if storage == 'sparse' else np.ascontiguousarray(rows.toarray())


def statement(d, dtype, lamI, lamAR, first, scale, c=C, sweeps=SWEEPS, missing=True, storage='sparse', W=None):
    """(W with the window replaced, weights) of trmf.robust_smooth_rows on the input set in `dtype`."""
    from trmf import robust_smooth_rows
    W = d['W'] if W is None else W
    return robust_smooth_rows(np.asarray(W, dtype=dtype), d['H'].astype(dtype), d['lag_set'], d['theta'].astype(dtype),
                              _rows(d, first, dtype, storage), first, lamI, lamAR, missing, scale, c, sweeps)


def objective_of(d, W, lamI, lamAR, first, scale, c=C, missing=True, storage='sparse'):
    from trmf import robust_window_objective
    return robust_window_objective(W, d['H'], d['lag_set'], d['theta'], _rows(d, first, np.float64, storage), first, lamI, lamAR, missing,
                                   scale, c)


def _observations(Yr, r, missing, n, dt):
    if smat.issparse(Yr):
        return Yr.indices[Yr.indptr[r]:Yr.indptr[r + 1]], Yr.data[Yr.indptr[r]:Yr.indptr[r + 1]].astype(dt)
    if missing:
        cols = np.nonzero(Yr[r])[0]
        return cols, Yr[r, cols].astype(dt)
    return np.arange(n), Yr[r].astype(dt)


def weighted_pcg(W, x0, G, b, back, theta, first, lamI, lamAR, rtol, max_iter):
    """smooth_helpers.pcg_twin's iteration on given blocks G (m x k x k) and right-hand sides b (m x k), started from x0 (m x k):
    the device's PCG (csrc/smooth_kernels.hpp) in the arrays' element type, the sums across rows and alpha, beta in fp64.  Returns
    (x, steps taken, converged, sqrt(r.z / (r.z)_0))."""
    dt = x0.dtype
    m, k = x0.shape
    chol = [np.linalg.cholesky(G[r] + (lamI + lamAR) * np.eye(k, dtype=dt)) for r in range(m)]

    def ar(v, head):                                         # e = B v; head: the rows before the window, or None for zeros
        e = v.copy()
        for l, lag in enumerate(back):
            if lag < m:
                e[lag:] -= theta[l] * v[:m - lag]
            if head is not None:
                h = min(lag, m)
                e[:h] -= theta[l] * head[first - lag:first - lag + h]
        return e

    def apply(v, e):
        a = e.copy()
        for l, lag in enumerate(back):
            if lag < m:
                a[:m - lag] -= theta[l] * e[lag:]
        return np.einsum('rcs,rs->rc', G, v) + lamI * v + lamAR * a

    def precond(r):
        return np.stack([scipy.linalg.cho_solve((chol[i], True), r[i], check_finite=False) for i in range(m)]).astype(dt)

    x = x0.copy()
    r = b - apply(x, ar(x, W))
    z = precond(r)
    rz = SH._fold(SH._row_dots(r, z))
    rz0, tol2 = rz, float(rtol) ** 2
    p = z.copy()
    steps, converged, spent, replaced = max_iter, False, False, False
    for j in range(max_iter + 1):
        hit = rz <= 0.0 if replaced else rz <= tol2 * rz0
        replaced = False
        if hit:
            if j == 0 or spent or j == max_iter:
                steps, converged = j, True
                break
            spent = replaced = True                          # the sweep's one residual replacement
            r = b - apply(x, ar(x, W))
            z = precond(r)
            rz = SH._fold(SH._row_dots(r, z))
            p = z.copy()
            continue
        if j == max_iter:
            break
        q = apply(p, ar(p, None))
        alpha = dt.type(rz / SH._fold(SH._row_dots(p, q)))
        x = x + alpha * p
        r = r - alpha * q
        z = precond(r)
        rz_new = SH._fold(SH._row_dots(r, z))
        p = z + dt.type(rz_new / rz) * p
        rz = rz_new
    return x, steps, converged, float(np.sqrt(max(rz, 0.0) / rz0)) if rz0 > 0 else 0.0


def irls_twin(W, H, lag_set, lag_val, Yrows, first, lamI, lamAR, missing, scale, c, sweeps, dtype, rtol, max_iter):
    """The device's robust smoother in NumPy: `sweeps` rounds of Huber weights formed in `dtype` from the rows of the round before,
    each round's system solved by weighted_pcg from those rows.  Returns (W with the window replaced, the last sweep's weights in
    robust_filter_rows' layout, steps per sweep, whether every sweep converged)."""
    dt = np.dtype(dtype)
    W = np.asarray(W, dtype=dt)
    H = np.asarray(H, dtype=dt)
    T, k = W.shape
    n = H.shape[0]
    back = np.asarray(lag_set).astype(np.int64)
    theta = np.asarray(lag_val, dtype=dt).reshape(len(back), k)
    lamI, lamAR = dt.type(lamI), dt.type(lamAR)
    m = T - first
    sparse = smat.issparse(Yrows)
    Yr = Yrows.tocsr() if sparse else np.asarray(Yrows)
    sc = np.full(n, float(scale)) if np.ndim(scale) == 0 else np.asarray(scale, dtype=np.float64)
    thr = dt.type(c) * sc.astype(dt)
    obs = [_observations(Yr, r, missing, n, dt) for r in range(m)]
    x = W[first:].copy()
    steps, converged, omega = [], True, None
    for _ in range(sweeps):
        G = np.zeros((m, k, k), dtype=dt)
        b = np.zeros((m, k), dtype=dt)
        omega = []
        for r, (cols, y) in enumerate(obs):
            Hi = H[cols]
            res = np.abs(y - Hi.dot(x[r]))
            om = np.ones(len(y), dtype=dt)
            far = res > thr[cols]
            om[far] = thr[cols][far] / res[far]
            Hw = Hi * om[:, None]
            G[r] = Hw.T.dot(Hi)
            b[r] = Hw.T.dot(y)
            omega.append(om)
        x, st, conv, _ = weighted_pcg(W, x, G, b, back, theta, first, lamI, lamAR, rtol, max_iter)
        steps.append(st)
        converged = converged and conv
    out = W.copy()
    out[first:] = x
    weights = np.ones(Yr.data.shape[0] if sparse else (m, n), dtype=dt)
    for r, (cols, _) in enumerate(obs):
        if sparse:
            weights[Yr.indptr[r]:Yr.indptr[r + 1]] = omega[r]
        else:
            weights[r, cols] = omega[r]
    return out, weights, steps, converged


def margins(d, first, lamI, lamAR, scale, c, sweeps, missing, storage):
    """Per observation of the window, in the order of the weights: | |r| / t - 1 | in fp64 with r the residual the last sweep's
    weight of the fp64 statement is formed from (x^{sweeps-1})."""
    prev = statement(d, np.float64, lamI, lamAR, first, scale, c, sweeps - 1, missing, storage)[0] if sweeps > 1 else d['W'].astype(np.float64)
    H = d['H'].astype(np.float64)
    Yr = _rows(d, first, np.float64, storage)
    n = H.shape[0]
    sc = np.full(n, float(scale)) if np.ndim(scale) == 0 else np.asarray(scale, dtype=np.float64)
    sparse = smat.issparse(Yr)
    out = np.full(Yr.data.shape[0] if sparse else Yr.shape, np.inf)
    for r in range(Yr.shape[0]):
        cols, y = _observations(Yr, r, missing, n, np.dtype(np.float64))
        mg = np.abs(np.abs(y - H[cols].dot(prev[first + r])) / (float(c) * sc[cols]) - 1.0)
        if sparse:
            out[Yr.indptr[r]:Yr.indptr[r + 1]] = mg
        else:
            out[r, cols] = mg
    return out


# ---- the cases: name -> how to build the input set and run it ---------------------------------------------------------------------
def _case_a(k, lamI, lamAR, first):
    return dict(kind='a', k=k, lamI=lamI, lamAR=lamAR, first=first, missing=True, storage='sparse', slice=None)


def _case_b(k, lamI, lamAR):
    return dict(kind='b', k=k, lamI=lamI, lamAR=lamAR, first=RH.B_T0, missing=True, storage='sparse', slice=RH.SLICE)


CASES = {}
for _k in OH.RANKS:
    for _lI, _lAR in OH.LAMBDAS:
        for _f in SH.FIRSTS:
            CASES['a-k%d-%g-%g-first%d' % (_k, _lI, _lAR, _f)] = _case_a(_k, _lI, _lAR, _f)
for _k in RH.B_RANKS:
    for _lI, _lAR in OH.LAMBDAS:
        CASES['b-k%d-%g-%g' % (_k, _lI, _lAR)] = _case_b(_k, _lI, _lAR)
CASES['dense-full-k16'] = dict(kind='a', k=16, lamI=OH.LAMBDAS[0][0], lamAR=OH.LAMBDAS[0][1], first=72, missing=False, storage='dense', slice=None)
CASES['lags-1-to-70-k7'] = dict(kind='wide', k=7, lamI=SH.GEOMETRY_LAMBDAS[0], lamAR=SH.GEOMETRY_LAMBDAS[1], first=SH.WIDE['first'], missing=True,
                                storage='sparse', slice=None)


@functools.lru_cache(maxsize=None)
def case(name):
    """(input set, scale) of a case: shared, read only."""
    spec = CASES[name]
    if spec['kind'] == 'b':
        d = RH.inputs_b(spec['k'])
    elif spec['kind'] == 'wide':
        d = SH.inputs(spec['k'], 0.3, lags=SH.WIDE['lags'], T=SH.WIDE['T'], N=SH.WIDE['N'], first=SH.WIDE['first'])
    else:
        d = OH.inputs(spec['k'])
    return d, RH.plain_scale(d, spec['lamI'], spec['lamAR'], spec['missing'])


@functools.lru_cache(maxsize=None)
def truth(name):
    """dict of the fp64 statement on a case: rows, weights, the borderline mask, the shares down-weighted / borderline."""
    spec = CASES[name]
    d, scale = case(name)
    w64, om64 = statement(d, np.float64, spec['lamI'], spec['lamAR'], spec['first'], scale, missing=spec['missing'], storage=spec['storage'])
    mg = margins(d, spec['first'], spec['lamI'], spec['lamAR'], scale, C, SWEEPS, spec['missing'], spec['storage'])
    border = mg <= BORDER
    cells = np.isfinite(mg)
    w64.setflags(write=False); om64.setflags(write=False)
    return dict(w64=w64, om64=om64, border=border, down=float((om64[cells] < 1).mean()), border_share=float(border[cells].mean()))


@functools.lru_cache(maxsize=None)
def yardstick(name, dtype):
    """dict of the IRLS twin in `dtype` on a case: its distance from the truth's rows (SH.measure) and weights (max abs difference
    outside borderline cells), its steps per sweep and whether every sweep converged."""
    dt = np.dtype(dtype)
    spec = CASES[name]
    d, scale = case(name)
    t = truth(name)
    first = spec['first']
    got, om, steps, converged = irls_twin(d['W'], d['H'], d['lag_set'], d['theta'], _rows(d, first, dt, spec['storage']), first, spec['lamI'],
                                          spec['lamAR'], spec['missing'], scale, C, SWEEPS, dt, SH.RTOL[dt], SH.MAX_ITER)
    keep = ~t['border']
    return dict(rows=SH.measure(got[first:], t['w64'][first:]), weights=float(np.abs(om.astype(np.float64) - t['om64'])[keep].max()) if keep.any() else 0.0,
                steps=steps, converged=converged)


# ---- the spiked panels of the quality check -----------------------------------------------------------------------------------------
QUALITY = dict(T=120, n=48, k=8, lags=(1, 2, 7), new_rows=24, back=8, observed=0.6, sigma=0.5, c=2.0, sweeps=4, lamI=0.5, lamAR=2.0)
QUALITY_SEEDS = (5, 6, 7)


@functools.lru_cache(maxsize=None)
def quality_panel(seed):
    """A robust_helpers.spiked_panel of 8 + 24 tail rows: the 8 rows before the new block keep their clean values, 3 % of the new
    block's cells are spiked.  Returns dict: the factors, the window's clean and dirty rows (sparse, fp64), `first` (the window)
    and `new` (the block), and in fp64 the rows the four methods leave and the clean-data smoothed rows they are measured against."""
    from trmf import filter_rows, robust_filter_rows, robust_smooth_rows, smooth_rows
    q = QUALITY
    W, H, lag_set, lag_val, clean, spiked, first, _ = RH.spiked_panel(q['T'], q['n'], q['k'], q['lags'], q['new_rows'] + q['back'], q['observed'], seed,
                                                                      sigma=q['sigma'])
    new = first + q['back']
    dirty = smat.vstack([clean[:q['back']], spiked[q['back']:]]).tocsr()
    args = (H, lag_set, lag_val)
    lam = (q['lamI'], q['lamAR'], True)
    W0 = filter_rows(W[:new], *args, clean[:q['back']], first, *lam)            # the rows before the block: filtered on their own clean data
    grow = lambda: np.vstack([W0, np.zeros((q['new_rows'], q['k']))])
    ref = smooth_rows(filter_rows(grow(), *args, clean[q['back']:], new, *lam), *args, clean, first, *lam)
    plain_f = filter_rows(grow(), *args, dirty[q['back']:], new, *lam)
    plain_s = smooth_rows(plain_f, *args, dirty, first, *lam)
    robust_f = robust_filter_rows(grow(), *args, dirty[q['back']:], new, *lam, q['sigma'], q['c'], q['sweeps'])[0]
    robust_s = robust_smooth_rows(robust_f, *args, dirty, first, *lam, q['sigma'], q['c'], q['sweeps'])[0]
    return dict(H=H, lag_set=lag_set, lag_val=lag_val, clean=clean, dirty=dirty, first=first, new=new, ref=ref, plain_f=plain_f, plain_s=plain_s,
                robust_f=robust_f, robust_s=robust_s)


def rms_distance(W, ref, new):
    """RMS distance of the new rows to the rows smoothed on the clean data."""
    return float(np.sqrt(np.mean((np.asarray(W, dtype=np.float64)[new:] - ref[new:]) ** 2)))
