"""Shared by tests/test_robust_host.py and tests/test_gpu_robust.py: the input sets of the robust online update, their fp32 / fp64
NumPy statements (trmf.robust_filter_rows) and the yardsticks the device is gated by (test infrastructure).

Set (a) is online_helpers.inputs(k) with c = 1.5 and 4 sweeps; the scale is one value per case, the pooled RMS of the fp64 plain
filter's residuals over the new block, so a good part of the cells lies beyond the threshold and both branches of the weight are
exercised.  Set (b) has 160 series and new rows of designed lengths, run with slices of 64 entries: rows of 0, 1, exactly 1, 1+ and
2+ slices."""
import functools

import numpy as np
import scipy.sparse as smat

import online_helpers as OH
from helpers import relmax

C, SWEEPS = 1.5, 4
BORDER = 1e-4                                               # a cell this close (relative) to its threshold may fall on either side
SLICE = 64
B_N, B_T0 = 160, 16
B_LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 160] + [80] * 11
B_T = B_T0 + len(B_LENGTHS)
B_RANKS = (7, 40, 64)


@functools.lru_cache(maxsize=None)
def inputs_b(k):
    """Set (b): like online_helpers.inputs (values drawn independently of W H^T), 16 rows of history at density 0.3 and 24 new
    rows whose B_LENGTHS entries sit on a random subset of the 160 series."""
    rng = np.random.RandomState(2000 + k)
    W = rng.rand(B_T, k).astype(np.float32)
    H = rng.rand(B_N, k).astype(np.float32)
    theta = rng.randn(len(OH.LAGS), k)
    theta = np.asfortranarray((theta / (np.abs(theta).sum(axis=0) + 0.1)).astype(np.float32))
    mask = np.zeros((B_T, B_N), dtype=bool)
    mask[:B_T0] = rng.rand(B_T0, B_N) < 0.3
    for r, L in enumerate(B_LENGTHS):
        mask[B_T0 + r, rng.permutation(B_N)[:L]] = True
    vals = rng.rand(B_T, B_N).astype(np.float32)
    vals[vals == 0] = 0.5
    Y = smat.csr_matrix(np.where(mask, vals, np.float32(0)).astype(np.float32))
    assert np.diff(Y.indptr)[B_T0:].tolist() == B_LENGTHS
    return dict(W=W, H=H, theta=theta, lag_set=np.array(OH.LAGS, dtype=np.uint32), Y=Y, k=k, T=B_T, N=B_N, first=B_T0)


def plain_scale(d, lamI, lamAR, missing=True, Y=None):
    """One value for every series: the pooled RMS of the fp64 plain filter's residuals over the new block."""
    first = d['first']
    w64 = OH.twin(d, np.float64, lamI, lamAR, missing, first, Y=Y)
    sq, cnt = OH.sq_err(d, w64, first, missing, Y=Y)
    return float(np.sqrt(sq / cnt))


def statement(d, dtype, lamI, lamAR, scale, c=C, sweeps=SWEEPS, missing=True, first=None, W=None, Y=None):
    """(W with the rows first.. re-solved, weights) of trmf.robust_filter_rows on the input set in `dtype`."""
    from trmf import robust_filter_rows
    first = d['first'] if first is None else first
    W = d['W'] if W is None else W
    Y = d['Y'] if Y is None else Y
    rows = OH.rows_of(Y, first, Y.shape[0], dtype)
    return robust_filter_rows(W.astype(dtype), d['H'].astype(dtype), d['lag_set'], d['theta'].astype(dtype), rows, first, lamI, lamAR,
                              missing, scale, c, sweeps)


def margins(d, w64, lamI, lamAR, scale, c=C, sweeps=SWEEPS, missing=True, first=None, Y=None):
    """Per observation of the new block, in the order of the weights: | |r| / t - 1 | in fp64 with r the residual the last sweep's
    weight is formed from (w^{sweeps-1}, teacher-forced: the row's earlier rows are w64's)."""
    from trmf import robust_filter_rows
    first = d['first'] if first is None else first
    Y = d['Y'] if Y is None else Y
    H = d['H'].astype(np.float64)
    th = d['theta'].astype(np.float64)
    sc = np.full(H.shape[0], float(scale)) if np.ndim(scale) == 0 else np.asarray(scale, dtype=np.float64)
    out = []
    for i in range(first, w64.shape[0]):
        row = OH.rows_of(Y, i, i + 1, np.float64)
        if sweeps > 1:
            prev = robust_filter_rows(w64[:i + 1], H, d['lag_set'], th, row, i, lamI, lamAR, missing, sc, c, sweeps - 1)[0][i]
        else:
            prev = OH.prior_of(w64, i, d['lag_set'], th)
        if smat.issparse(row):
            cols, y = row.indices, row.data
        else:
            cols, y = np.arange(H.shape[0]), np.asarray(row[0], dtype=np.float64)
        res = np.abs(y - H[cols].dot(prev))
        out.append(np.abs(res / (float(c) * sc[cols]) - 1.0))
    return np.concatenate(out) if out else np.zeros(0)


def yardstick_of(d, lamI, lamAR, scale, c=C, sweeps=SWEEPS, missing=True, Y=None):
    """dict: the fp64 statement's W and weights, the fp32 statement's distances to them (relmax of the new rows / max abs
    difference of the weights) and the borderline mask of the observations."""
    first = d['first']
    w64, om64 = statement(d, np.float64, lamI, lamAR, scale, c, sweeps, missing, Y=Y)
    w32, om32 = statement(d, np.float32, lamI, lamAR, scale, c, sweeps, missing, Y=Y)
    border = margins(d, w64, lamI, lamAR, scale, c, sweeps, missing, Y=Y) <= BORDER if np.isfinite(c) else np.zeros(om64.size, dtype=bool)
    return dict(w64=w64, om64=om64, w32=w32, om32=om32, dev_rows=relmax(w32[first:], w64[first:]),
                dev_weights=float(np.abs(om32.astype(np.float64) - om64).max()) if om64.size else 0.0, border=border.reshape(om64.shape))


@functools.lru_cache(maxsize=None)
def case_a(k, lamI, lamAR):
    d = OH.inputs(k)
    scale = plain_scale(d, lamI, lamAR)
    return d, scale, yardstick_of(d, lamI, lamAR, scale)


@functools.lru_cache(maxsize=None)
def case_b(k, lamI, lamAR):
    d = inputs_b(k)
    scale = plain_scale(d, lamI, lamAR)
    return d, scale, yardstick_of(d, lamI, lamAR, scale)


def exercised(y):
    """The conditions a case must meet to check anything: between 3 % and 97 % of the cells down-weighted by the fp64 statement,
    at most 1 % of them borderline.  Returns (share down-weighted, share borderline)."""
    om = y['om64'].ravel()
    return float((om < 1).mean()), float(y['border'].mean())


# ---- the spiked panels of the quality check ---------------------------------------------------------------------------------------
def spiked_panel(T, n, k, lags, new_rows, observed, seed, sigma=0.5, spike=40.0, share=0.03):
    """A Model.syn_gen panel with observation noise sigma on `observed` of the cells; `share` of the observed NEW cells spiked by
    +-spike sigma.  Returns (W, H, lag_set, lag_val, clean new rows, spiked new rows, first) in fp64, sparse rows."""
    from trmf import Model
    g = Model.syn_gen(T, n, k, lags, seed=seed, dtype=np.float64)
    rng = np.random.RandomState(seed + 1)
    first = T - new_rows
    Y = g['Y'] + sigma * rng.randn(T, n)
    mask = rng.rand(new_rows, n) < observed
    clean = np.where(mask, Y[first:], 0.0)
    hit = mask & (rng.rand(new_rows, n) < share)
    spiked = clean + np.where(hit, spike * sigma * np.sign(rng.randn(new_rows, n)), 0.0)
    rows, cols = np.nonzero(mask)
    to_csr = lambda A: smat.csr_matrix((A[rows, cols], (rows, cols)), shape=A.shape)
    return g['W'], g['H'], g['lag_set'], g['lag_val'], to_csr(clean), to_csr(spiked), first, to_csr(hit.astype(np.float64))
