"""Missing-value imputation -- the second task of the TRMF paper -- with the held-out cells scored on the device.

``impute(Y, observed, lag_set, ...)`` trains on exactly the observed cells of a dense panel (observed zeros included: the
training matrix is built from the mask, not from the non-zeros) and fills the other cells with W.H^T, evaluated by the
library at the resident held-out positions (``Session.set_heldout`` / ``Session.eval_heldout``): the factors never leave
the card to score a model.  ``grid_impute`` runs the paper's grid protocol with one resident session per rank ``k``: the
held-out set is uploaded once, the initial model is marked, and every weight combination is ``rewind()``,
``set_lambdas()``, ``run()``, ``eval_heldout()``.

Scores over the held-out cells with finite truth y and predictions y^ (``ImputeMetrics``; N cells, N' of them with y != 0):

    mse   = sum (y^ - y)^2 / N
    nrmse = sqrt(mse) / (sum |y| / N)
    nd    = sum |y^ - y| / sum |y|
    mape  = sum over y != 0 of |y^ - y| / |y|  /  N'        (zero truths left out, as in metrics.py)
"""
import collections
import math

import numpy as np
import scipy.sparse as smat

from .model import Model
from .validate import _grid_points

_FIELDS = ('nd', 'nrmse', 'mse', 'mape', 'count')
_DEFAULTS = dict(k=40, lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5, max_iter=10, seed=0, dtype=None, lambdaLagL1=0.0, lag_refit=False)
_GRID_KEYS = ('k', 'lambdaI', 'lambdaAR', 'lambdaLag', 'lambdaLagL1')


def _ratio(num, den):
    if den == 0:
        return math.nan if num == 0 else math.inf
    return num / den


class ImputeMetrics(collections.namedtuple('ImputeMetrics', _FIELDS)):
    __slots__ = ()

    def __str__(self):
        return ' '.join('{}={:.4g}'.format(name, value) for name, value in zip(self._fields, self))

    @classmethod
    def from_sums(cls, sums):
        """From the six sums of a held-out evaluation (``TrmfHeldoutSums`` fields, as a dict or an object)."""
        get = sums.get if isinstance(sums, dict) else (lambda name: getattr(sums, name))
        count, nonzero = int(get('count')), int(get('count_nonzero'))
        sq, ab, truth, rel = float(get('sq_err')), float(get('abs_err')), float(get('abs_truth')), float(get('rel_err'))
        mse = _ratio(sq, count)
        return cls(nd=_ratio(ab, truth), nrmse=_ratio(math.sqrt(mse), _ratio(truth, count)) if count else math.nan,
                   mse=mse, mape=_ratio(rel, nonzero), count=count)

    @classmethod
    def generate(cls, truth, pred):
        """The same scores from host arrays (float64): the yardstick of the device's sums."""
        y = np.asarray(truth, dtype=np.float64).ravel()
        d = np.asarray(pred, dtype=np.float64).ravel() - y
        nz = y != 0
        return cls.from_sums(dict(count=y.size, count_nonzero=int(nz.sum()), sq_err=float(np.sum(d * d)), abs_err=float(np.sum(np.abs(d))),
                                  abs_truth=float(np.sum(np.abs(y))), rel_err=float(np.sum(np.abs(d[nz]) / np.abs(y[nz])))))


def _cells_matrix(values, rows, cols, shape, dtype):
    """CSR matrix whose stored entries are exactly the cells (rows, cols) -- given in row-major order -- holding ``values``;
    zeros stay stored entries."""
    indptr = np.zeros(shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=shape[0]), out=indptr[1:])
    return smat.csr_matrix((np.asarray(values, dtype=dtype), cols.astype(np.int32), indptr), shape=shape)


def training_matrix(Y, observed, dtype=None):
    """The observed cells of the dense ``Y`` as a COO matrix of exactly ``observed.sum()`` entries, zeros included (the form
    ``train(..., missing=True)`` and ``impute`` train on)."""
    Y = np.asarray(Y)
    observed = np.asarray(observed, dtype=bool)
    assert observed.shape == Y.shape, 'mask shape {} differs from Y {}'.format(observed.shape, Y.shape)
    rows, cols = np.nonzero(observed)
    return smat.coo_matrix((np.asarray(Y[rows, cols], dtype=dtype or Y.dtype), (rows, cols)), shape=Y.shape)


def _setup(Y, observed, dtype):
    Y = np.asarray(Y)
    if Y.ndim != 2:
        raise ValueError('impute: Y must be a T x n array')
    observed = np.asarray(observed, dtype=bool)
    if observed.shape != Y.shape:
        raise ValueError('impute: mask shape {} differs from Y {}'.format(observed.shape, Y.shape))
    if dtype is None:
        dtype = Y.dtype if Y.dtype in (np.float32, np.float64) else np.float64
    dtype = np.dtype(dtype)
    rows, cols = np.nonzero(~observed)                      # held-out cells, row-major = the CSR order of the set
    finite = np.isfinite(Y[rows, cols])
    return Y, observed, dtype, rows, cols, finite


def _session(Ytr, lag_set, k, seed, dtype, hyper):
    from .session import Session
    model = Model.initialize(Ytr, lag_set, k, seed=seed, dtype=dtype)
    # the settings of a c_trmf_train call (no norm records, no phase events): the same iterates as train()
    return Session(Ytr, model, missing=True, log_norms=False, timing=0, **hyper), model


def impute(Y, observed, lag_set, k=40, lambdaI=0.5, lambdaAR=50.0, lambdaLag=0.5, max_iter=10, seed=0, dtype=None,
           lambdaLagL1=0.0, lag_refit=False):
    """Train on the observed cells of the dense T x n ``Y`` (boolean mask ``observed``) and fill in the others
    (``lambdaLagL1`` / ``lag_refit``: sparse lag weights, ``Session.set_lag_penalty``).

    Returns ``(filled, metrics, model)``: ``Y`` with every unobserved cell replaced by the model's prediction, the
    ``ImputeMetrics`` over the unobserved cells whose ``Y`` is finite (``None`` when there is none), and the trained ``Model``."""
    Y, observed, dtype, rows, cols, finite = _setup(Y, observed, dtype)
    Ytr = training_matrix(Y, observed, dtype)
    filled = np.array(Y, copy=True)
    metrics = None
    hyper = dict(lambdaI=lambdaI, lambdaAR=lambdaAR, lambdaLag=lambdaLag)
    if lambdaLagL1 or lag_refit:
        hyper.update(lambdaLagL1=lambdaLagL1, lag_refit=lag_refit)
    sess, model = _session(Ytr, lag_set, k, seed, dtype, hyper)
    with sess:
        sess.run(max_iter)
        if rows.size:
            truth = Y[rows, cols]
            # every unobserved cell gets a prediction; a non-finite truth would poison the sums, so those cells are scored apart
            sess.set_heldout(_cells_matrix(np.where(finite, truth, 0), rows, cols, Y.shape, dtype))
            metrics, pred = sess.eval_heldout(predictions=True)
            filled[rows, cols] = pred
            if not finite.all():
                metrics = None
                if finite.any():
                    sess.set_heldout(_cells_matrix(truth[finite], rows[finite], cols[finite], Y.shape, dtype))
                    metrics = sess.eval_heldout()
        sess.download()
    return filled, metrics, model


def grid_impute(Y, observed, lag_set, grid_params, **kw):
    """Every combination of ``grid_params`` (keys among k, lambdaI, lambdaAR, lambdaLag, lambdaLagL1) scored like ``impute`` with
    the remaining settings from ``kw`` (max_iter, seed, dtype, lag_refit and the fixed values of the grid keys).  One resident session per
    ``k``: the held-out cells are uploaded once and the initial model is marked; each weight combination then rewinds to it,
    sets the weights and trains -- no factor is downloaded.  Returns ``(results, best_by_nrmse, best_by_nd)``: a list of
    ``{'kws': settings, 'metrics': ImputeMetrics}`` in grid order and the two best entries of it."""
    unknown = set(grid_params) - set(_GRID_KEYS)
    if unknown:
        raise ValueError('grid_impute: cannot vary {} (grid keys: {})'.format(sorted(unknown), ', '.join(_GRID_KEYS)))
    unknown = set(kw) - set(_DEFAULTS)
    if unknown:
        raise ValueError('grid_impute: unknown settings {}'.format(sorted(unknown)))
    base = dict(_DEFAULTS, **kw)
    from .session import check_lag_penalty
    for l1 in list(grid_params.get('lambdaLagL1', ())) + [base['lambdaLagL1']]:
        check_lag_penalty(l1, base['lag_refit'])
    sparse_lags = bool(base['lag_refit']) or any(float(v) > 0 for v in list(grid_params.get('lambdaLagL1', ())) + [base['lambdaLagL1']])
    Y, observed, dtype, rows, cols, finite = _setup(Y, observed, base['dtype'])
    if not finite.any():
        raise ValueError('grid_impute: no unobserved cell with a finite value to score')
    Ytr = training_matrix(Y, observed, dtype)
    held = _cells_matrix(Y[rows[finite], cols[finite]], rows[finite], cols[finite], Y.shape, dtype)
    points = [dict(base, **point) for point in _grid_points(grid_params)]
    results = [None] * len(points)
    by_k = collections.OrderedDict()
    for idx, settings in enumerate(points):
        by_k.setdefault(settings['k'], []).append(idx)
    for k, members in by_k.items():
        first = points[members[0]]
        sess, _ = _session(Ytr, lag_set, k, first['seed'], dtype, {name: first[name] for name in ('lambdaI', 'lambdaAR', 'lambdaLag')})
        with sess:
            sess.set_heldout(held).mark()
            for idx in members:
                st = points[idx]
                sess.rewind().set_lambdas(st['lambdaI'], st['lambdaAR'], st['lambdaLag'])
                if sparse_lags:
                    sess.set_lag_penalty(st['lambdaLagL1'], st['lag_refit'])
                sess.run(st['max_iter'])
                results[idx] = {'kws': st, 'metrics': sess.eval_heldout()}
    best_by_nrmse = min(results, key=lambda r: r['metrics'].nrmse)
    best_by_nd = min(results, key=lambda r: r['metrics'].nd)
    return results, best_by_nrmse, best_by_nd
