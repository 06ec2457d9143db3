"""Forecast uncertainty of a TRMF model: the NumPy statement of ``trmf_session_fit_noise`` / ``trmf_session_forecast_dist``
(host side, pure NumPy -- the device path is ``Session.fit_noise`` / ``Session.forecast_dist``).

TRMF read as a linear-Gaussian state-space model: ``y_ij = w_i . h_j + eps_ij`` with ``eps_ij ~ N(0, sigma_j^2)``, and every
latent dimension an AR process ``w_i[d] = sum_l Theta(l, d) w_{i - L_l}[d] + eta_i[d]`` with ``eta_i[d] ~ N(0, q_d)``.  Then
the forecast of series j, s + 1 steps ahead, has the variance

    V[s][j] = sigma_j^2 + sum_d H[j][d]^2 v_d[s],      v_d[s] = q_d sum_{u <= s} psi_d[u]^2,

where ``psi_d`` is the impulse response of dimension d's AR recursion (``psi_d[0] = 1``).  All variance arithmetic is fp64.

This is a PLUG-IN interval: it ignores the estimation error of H, of the lag weights and of the last rows of W, and
``sigma_j^2`` / ``q_d`` are in-sample residual variances, so it is too narrow where the model overfits.  A caller who has
out-of-sample variances (for example ``sq_err`` of ``Session.forecast_series_sums`` over earlier windows) substitutes them with
``Session.set_noise``.

``m = max(lag_set)``, ``T = rows of W``.  A lag 0 contributes nothing, as in ``Model.latent_forecast`` (the row being formed
reads as zero).
"""
import collections
import math

import numpy as np
import scipy.sparse as smat
from scipy.special import ndtri

_SQRT2, _SQRT_PI, _SQRT_2PI = math.sqrt(2.0), math.sqrt(math.pi), math.sqrt(2.0 * math.pi)


def _lags(lag_set):
    return [int(v) for v in np.asarray(lag_set).ravel()]


def _sequential_sum(values):
    """Added one by one in the order given (``np.sum`` adds pairwise)."""
    total = 0.0
    for v in values:
        total += float(v)
    return total


def fit_noise(W, H, lag_set, lag_val, Y, missing=True):
    """``(sigma2, q, info)`` of the factors on the training matrix ``Y`` (T x n, in the scale the factors were trained on).

    ``sigma2[j] = (1 / |Omega_j|) sum_{i in Omega_j} (y_ij - w_i . h_j)^2`` over the stored entries of series j (``missing``;
    ``Y`` must be sparse), or over every timestamp with an absent entry of a sparse ``Y`` reading as 0 (``missing=False``).
    A cell that a sparse ``Y`` stores several times is read as the training objective reads it: with ``missing`` every stored
    entry is a residual of its own (and counts in ``|Omega_j|``); without, ``||Y||^2`` is the sum of squares of the stored
    values and ``Y . W H^T`` adds them, so the cell contributes ``p^2 + sum_e y_e (y_e - 2 p)`` and counts once -- not
    ``(sum_e y_e - p)^2``, which a caller gets by summing duplicates first.
    Products, dot product, difference, square and sum are fp64, formed from the stored values of W, H and Y.  A series without
    a stored entry takes the pooled value ``sum_j sq_j / sum_j cnt_j`` (both summed in series order).

    ``q[d] = (1 / (T - m)) sum_{i >= m} (w_i[d] - p_i[d])^2`` with ``p_i[d] = sum_l W[i - L_l][d] Theta(l, d)`` formed as
    ``Model.latent_forecast`` forms it (products rounded to the element type, added in ascending lag order); difference,
    square and sum are fp64: the residual is the one-step latent forecast error of the code that forecasts.

    ``info``: ``{'pooled', 'sq', 'cnt', 'series_pooled'}``."""
    W, H, lag_val = np.asarray(W), np.asarray(H), np.asarray(lag_val)
    T, k = W.shape
    n = H.shape[0]
    lags = _lags(lag_set)
    m = max(lags) if lags else 0
    if T <= m:
        raise ValueError('fit_noise: {} timestamps do not reach past the largest lag {}'.format(T, m))
    if Y.shape != (T, n):
        raise ValueError('fit_noise: Y is {} x {}, the factors describe {} x {}'.format(Y.shape[0], Y.shape[1], T, n))
    W64, H64 = W.astype(np.float64), H.astype(np.float64)
    if missing:
        if not smat.issparse(Y):
            raise ValueError('fit_noise: missing=True needs a sparse Y (its stored entries are the observations)')
        coo = Y.tocoo()
        pred = np.einsum('ed,ed->e', W64[coo.row], H64[coo.col])
        res = coo.data.astype(np.float64) - pred
        sq = np.bincount(coo.col, weights=res * res, minlength=n).astype(np.float64)
        cnt = np.bincount(coo.col, minlength=n).astype(np.float64)
    else:
        if smat.issparse(Y):
            # the stored entries as they are (scipy's own astype would add repeated cells first, in Y's element type)
            coo = Y.tocoo()
            y = coo.data.astype(np.float64)
            dense = smat.coo_matrix((y, (coo.row, coo.col)), shape=Y.shape).toarray()
        else:
            dense = np.asarray(Y, dtype=np.float64)
        res = dense - W64.dot(H64.T)
        cell = res * res
        if smat.issparse(Y):
            # a cell stored several times: (sum_e y_e - p)^2 less the cross terms (sum_e y_e)^2 - sum_e y_e^2 (exactly 0 for a
            # cell stored once, so a canonical matrix keeps its bits)
            cell = cell - (dense * dense - smat.coo_matrix((y * y, (coo.row, coo.col)), shape=Y.shape).toarray())
        sq = cell.sum(axis=0)
        cnt = np.full(n, float(T))
    total_cnt = _sequential_sum(cnt)
    if total_cnt == 0:
        raise ValueError('fit_noise: Y has no stored entry')
    pooled = _sequential_sum(sq) / total_cnt
    with np.errstate(divide='ignore', invalid='ignore'):
        sigma2 = np.where(cnt > 0, sq / cnt, pooled)
    # one-step latent forecasts in the element type, like _ar_rollout
    pred = np.zeros((T - m, k), dtype=W.dtype)
    for l, lag in enumerate(lags):
        if lag > 0:
            pred = pred + W[m - lag:T - lag] * lag_val[l]
    inn = W64[m:] - pred.astype(np.float64)
    q = (inn * inn).sum(axis=0) / float(T - m)
    return sigma2, q, dict(pooled=pooled, sq=sq, cnt=cnt, series_pooled=int((cnt == 0).sum()))


def impulse_response(lag_set, lag_val, steps):
    """``psi`` (steps x k, fp64): ``psi[0] = 1``, ``psi[s] = sum_{l: L_l <= s} Theta(l, d) psi[s - L_l]``, added in ascending
    lag order from the element-type lag weights."""
    theta = np.asarray(lag_val).astype(np.float64)
    lags = _lags(lag_set)
    steps = int(steps)
    if steps < 1:
        raise ValueError('impulse_response: steps must be at least 1')
    psi = np.zeros((steps, theta.shape[1]), dtype=np.float64)
    psi[0] = 1.0
    with np.errstate(over='ignore', invalid='ignore'):          # (explosive lag weights are the caller's to judge: forecast_var refuses them)
        for s in range(1, steps):
            acc = np.zeros(theta.shape[1], dtype=np.float64)
            for l, lag in enumerate(lags):
                if 0 < lag <= s:
                    acc = acc + theta[l] * psi[s - lag]
            psi[s] = acc
    return psi


def latent_forecast_var(lag_set, lag_val, q, steps):
    """``v`` (steps x k, fp64): ``v[s] = q sum_{u <= s} psi[u]^2``; row 0 is one step ahead."""
    psi = impulse_response(lag_set, lag_val, steps)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(q, dtype=np.float64) * np.cumsum(psi * psi, axis=0)


def forecast_var(H, lag_set, lag_val, sigma2, q, steps):
    """``V`` (steps x n, fp64) in the training scale: ``sigma2[j] + sum_d H[j][d]^2 v_d[s]``."""
    sigma2, q = np.asarray(sigma2, dtype=np.float64), np.asarray(q, dtype=np.float64)
    H64 = np.asarray(H).astype(np.float64)
    if sigma2.shape != (H64.shape[0],) or q.shape != (H64.shape[1],):
        raise ValueError('forecast_var: sigma2 must have n = {} values and q k = {}'.format(H64.shape[0], H64.shape[1]))
    if not (np.isfinite(sigma2).all() and np.isfinite(q).all() and (sigma2 >= 0).all() and (q >= 0).all()):
        raise ValueError('forecast_var: variances must be finite and not negative')
    v = latent_forecast_var(lag_set, lag_val, q, steps)
    if not np.isfinite(v).all():
        raise ValueError('lag weights explosive over this horizon')
    return sigma2[None, :] + v.dot((H64 * H64).T)


def forecast_std(H, lag_set, lag_val, sigma2, q, steps, transform=None, dtype=None):
    """Predictive standard deviation (steps x n) of the forecast: ``sqrt(V)``, divided by ``|a_j|`` under a series transform
    ``y -> a_j y + b_j`` (the forecast is reported in raw units), rounded once to ``dtype`` (default: H's)."""
    sd = np.sqrt(forecast_var(H, lag_set, lag_val, sigma2, q, steps))
    if transform is not None:
        sd = sd / np.abs(np.asarray(transform.a, dtype=np.float64).reshape(1, -1))
    return sd.astype(np.asarray(H).dtype if dtype is None else dtype)


def z_of_level(level):
    """The two-sided normal quantile of a central interval: ``ndtri((1 + level) / 2)``."""
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError('the interval level must lie strictly between 0 and 1, not {!r}'.format(level))
    return float(ndtri((1.0 + level) / 2.0))


def interval_terms(truth, mean, sd, zq):
    """Per cell, fp64: ``(covered, sd, |truth|, z^2, nll, crps)`` of a normal predictive distribution; ``e = truth - mean``,
    ``z = e / sd``, ``nll = log(2 pi sd^2) / 2 + z^2 / 2``, ``crps = sd (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi))``."""
    from scipy.special import erf
    truth, mean, sd = (np.asarray(a, dtype=np.float64) for a in (truth, mean, sd))
    e = truth - mean
    z = e / sd
    z2 = z * z
    covered = (np.abs(e) <= zq * sd).astype(np.float64)
    nll = 0.5 * np.log(2.0 * math.pi * (sd * sd)) + 0.5 * z2
    crps = sd * (z * erf(z / _SQRT2) + 2.0 * (np.exp(-0.5 * z2) / _SQRT_2PI) - 1.0 / _SQRT_PI)
    return covered, sd, np.abs(truth), z2, nll, crps


_IV_FIELDS = ('coverage', 'width', 'z2', 'nll', 'crps', 'm_coverage')


class IntervalMetrics(collections.namedtuple('IntervalMetrics', _IV_FIELDS)):
    """Scores of a normal predictive distribution over the scored cells: ``coverage`` the share of truths inside the central
    interval, ``width`` the mean interval width over the mean ``|truth|``, ``z2`` the mean squared standardised error (1 for a
    calibrated model), ``nll`` the mean negative log likelihood, ``crps`` the mean continuous ranked probability score,
    ``m_coverage`` the per-series coverage averaged over the series."""
    __slots__ = ()

    def __str__(self):
        return ' '.join('{}={:.4g}'.format(name, value) for name, value in zip(self._fields, self))

    @classmethod
    def from_series_sums(cls, table, level):
        """From the n x 7 table of ``TrmfIntervalSums`` (cells, covered, sd_sum, abs_truth, z2_sum, nll_sum, crps_sum per
        series); pooled sums are the per-series sums added in series order."""
        table = np.asarray(table, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 7:
            raise ValueError('IntervalMetrics.from_series_sums: an n x 7 table is required')
        zq = z_of_level(level)
        cells, covered, sd_sum, abs_truth, z2, nll, crps = (_sequential_sum(table[:, c]) for c in range(7))
        if cells <= 0:
            raise ValueError('IntervalMetrics.from_series_sums: no scored cell')
        scored = table[:, 0] > 0
        with np.errstate(divide='ignore', invalid='ignore'):
            return cls(coverage=covered / cells, width=(2.0 * zq * sd_sum) / abs_truth, z2=z2 / cells, nll=nll / cells,
                       crps=crps / cells, m_coverage=float((table[scored, 1] / table[scored, 0]).mean()))

    @classmethod
    def series_sums(cls, truth, mean, sd, level):
        """The n x 7 table of the cells of ``truth`` / ``mean`` / ``sd`` (steps x n each), every series summed in step order."""
        truth = np.asarray(truth)
        if truth.ndim != 2 or np.asarray(mean).shape != truth.shape or np.asarray(sd).shape != truth.shape:
            raise ValueError('IntervalMetrics: truth, mean and sd must be steps x n arrays of one shape')
        terms = interval_terms(truth, mean, sd, z_of_level(level))
        table = np.zeros((truth.shape[1], 7), dtype=np.float64)
        for i in range(truth.shape[0]):
            table[:, 0] += 1.0
            for c, term in enumerate(terms):
                table[:, c + 1] += term[i]
        return table

    @classmethod
    def generate(cls, truth, mean, sd, level=0.9):
        return cls.from_series_sums(cls.series_sums(truth, mean, sd, level), level)
