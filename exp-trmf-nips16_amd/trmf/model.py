"""The TRMF model object of the Python front end (host side, pure NumPy -- no GPU code here).

API contract (names, signatures, defaults, array layouts, RNG call order, file names), pinned by
tests/test_python_frontend.py; the reference's counterpart is python/trmf/trmf.py:82-251:

* ``Model``: ``W`` (T x k, C order), ``H`` (n x k, C order), ``lag_val`` (|L| x k, F order) wrapped as
  ``PyMatrix`` views (``pyW``, ``pyH``, ``pylag_val``) that the C ABI updates in place; ``lag_set`` sorted uint32.
* ``Model.initialize`` draws ``rand`` W, ``rand`` H, ``randn`` lag_val, in that order, after ``np.random.seed(seed)``;
  a ``warm_start_model`` replaces them by the previous model rolled forward.
* ``Model.save`` / ``Model.load``: ``arrays.npz`` (W, H, lag_val, lag_set) + ``other.pkl`` ({'transform': ...}).
* ``NormalizedTransform``: per-series affine map ``y -> a*y + b`` to zero mean / unit variance.
"""
import os
import pickle

import numpy as np
import scipy.sparse as smat

from .rf_util import PyMatrix

_ARRAYS, _EXTRA = 'arrays.npz', 'other.pkl'


class NormalizedTransform(object):
    """z-score per series: ``preprocess`` applies ``a*y + b`` with a = 1/std, b = -mean/std; ``postprocess`` undoes it.
    Constant series (std = 0) keep a unit scale."""

    def __init__(self, Y):
        dense = Y.toarray() if smat.issparse(Y) else np.asarray(Y)
        center = dense.mean(axis=0, keepdims=True)
        spread = dense.std(axis=0, keepdims=True)
        spread = np.where(spread == 0, 1.0, spread)
        self.a = 1.0 / spread
        self.b = -self.a * center

    def _check(self, Y):
        assert Y.shape[1] == self.a.shape[1], 'series count differs from the fitted transform'

    def preprocess(self, Y):
        self._check(Y)
        return Y * self.a + self.b

    def postprocess(self, Y):
        self._check(Y)
        return (Y - self.b) / self.a


def _sorted_lags(lag_set):
    return np.array(sorted(lag_set), dtype=np.uint32)


def _empty_factors(m, n, k, nlag, dtype):
    """Zero-filled (W, H, lag_val) in the memory orders the C ABI requires (trmf.cpp:583-594)."""
    return (np.zeros((m, k), dtype=dtype, order='C'), np.zeros((n, k), dtype=dtype, order='C'),
            np.zeros((nlag, k), dtype=dtype, order='F'))


def _ar_rollout(W, first, last, lag_set, lag_val):
    """In place: W[i] = sum_l lag_val[l] * W[i - lag_set[l]] for i = first .. last-1, in time order."""
    back = lag_set.astype(np.int64)
    for i in range(first, last):
        np.sum(W[i - back] * lag_val, axis=0, out=W[i])


class Model(object):

    def __init__(self, pyW=None, pyH=None, pylag_val=None, lag_set=None, transform=None):
        self.pyW, self.pyH, self.pylag_val = pyW, pyH, pylag_val
        self.lag_set = lag_set
        self.transform = transform

    @classmethod
    def from_arrays(cls, W, H, lag_val, lag_set, transform=None, dtype=None):
        dtype = W.dtype if dtype is None else dtype
        return cls(PyMatrix(np.ascontiguousarray(W), dtype), PyMatrix(np.ascontiguousarray(H), dtype),
                   PyMatrix(np.asfortranarray(lag_val), dtype), lag_set=lag_set, transform=transform)

    # the arrays the C side reads and writes are the ones pinned inside the PyMatrix views
    @property
    def W(self):
        return self.pyW.py_buf['val']

    @property
    def H(self):
        return self.pyH.py_buf['val']

    @property
    def lag_val(self):
        return self.pylag_val.py_buf['val']

    @property
    def m(self):
        return self.W.shape[0]

    @property
    def n(self):
        return self.H.shape[0]

    @property
    def k(self):
        return self.W.shape[1]

    # ---- persistence ---------------------------------------------------------------------------
    def save(self, path_to_folder):
        os.makedirs(path_to_folder, exist_ok=True)
        np.savez(os.path.join(path_to_folder, _ARRAYS), W=self.W, H=self.H, lag_val=self.lag_val, lag_set=self.lag_set)
        with open(os.path.join(path_to_folder, _EXTRA), 'wb') as fh:
            pickle.dump({'transform': self.transform}, fh)

    @classmethod
    def load(cls, path_to_folder, dtype=None):
        assert os.path.isdir(path_to_folder), path_to_folder
        with np.load(os.path.join(path_to_folder, _ARRAYS)) as stored:
            parts = {name: stored[name] for name in ('W', 'H', 'lag_val', 'lag_set')}
        with open(os.path.join(path_to_folder, _EXTRA), 'rb') as fh:
            extra = pickle.load(fh)
        return cls.from_arrays(parts['W'], parts['H'], parts['lag_val'], parts['lag_set'],
                               transform=extra['transform'], dtype=dtype)

    # ---- forecasting -----------------------------------------------------------------------------
    def latent_forecast(self, window, Wnew=None):
        """W extended by ``window`` timestamps through the AR model; the first ``m`` rows are W itself."""
        total = self.m + window
        if Wnew is None:
            Wnew = np.zeros((total, self.k), dtype=self.W.dtype, order='C')
        assert Wnew.shape == (total, self.k) and Wnew.dtype == self.W.dtype and Wnew.flags.c_contiguous
        Wnew[:self.m] = self.W
        _ar_rollout(Wnew, self.m, total, self.lag_set, self.lag_val)
        return Wnew

    def forecast(self, window, Ynew=None, threshold=None):
        """(Ynew, Wnew): the next ``window`` rows of Y and of W; values below ``threshold`` are clipped before the
        transform (if any) is undone."""
        Wnew = self.latent_forecast(window)[self.m:]
        if Ynew is None:
            Ynew = np.zeros((window, self.n), dtype=self.W.dtype, order='C')
        Ynew[:] = Wnew.dot(self.H.T)
        if threshold is not None:
            np.maximum(Ynew, threshold, out=Ynew)
        if self.transform is not None:
            Ynew[:] = self.transform.postprocess(Ynew)
        return Ynew, Wnew

    # ---- forecast uncertainty ----------------------------------------------------------------------
    def fit_noise(self, Y, missing=True):
        """Fit the observation noise per series and the innovation variance per latent dimension of this model on its
        training matrix ``Y`` (raw values; a transform of this model is applied first) and keep them as ``self.noise =
        (sigma2, q)`` (``trmf.uncertainty.fit_noise``; the host form of ``Session.fit_noise``).  Returns ``self``."""
        from .uncertainty import fit_noise
        if self.transform is not None:
            if smat.issparse(Y):
                raise ValueError('fit_noise: a series transform needs a dense Y')
            Y = self.transform.preprocess(np.asarray(Y)).astype(self.W.dtype)
            if missing:
                Y = smat.csr_matrix(Y)
        sigma2, q, _ = fit_noise(self.W, self.H, self.lag_set, self.lag_val, Y, missing)
        self.noise = (sigma2, q)
        return self

    def forecast_std(self, window):
        """Predictive standard deviation (window x n) of ``forecast(window)``, in the units ``forecast`` reports; needs
        ``fit_noise`` first.  A plug-in estimate: see ``trmf.uncertainty``."""
        from .uncertainty import forecast_std
        noise = getattr(self, 'noise', None)
        if noise is None:
            raise ValueError('forecast_std: no noise fitted (Model.fit_noise)')
        return forecast_std(self.H, self.lag_set, self.lag_val, noise[0], noise[1], window, transform=self.transform)

    # ---- online update ----------------------------------------------------------------------------
    def assimilate(self, Ynew, lambdaI, lambdaAR, missing=True, robust_c=None, robust_sweeps=4, scale=None, adapt=False, forget=1.0,
                   smooth_back=0, Yback=None, smooth_robust=False, adapt_robust=False, window=None):
        """A new ``Model`` grown by the ``Ynew.shape[0]`` timestamps of ``Ynew`` (raw values; a transform of this model is
        applied first): H, the lag weights and the rows this model has stay as they are, every new row of W is solved from its
        own observations and the AR prior of the rows before it (``trmf.online.filter_rows``; the host form of
        ``Session.update``).  This model is left untouched.  With ``robust_c`` the rows are solved with Huber weights
        (``trmf.online.robust_filter_rows``: ``robust_sweeps`` rounds, ``scale`` per series, default ``sqrt(self.noise[0])`` of
        ``fit_noise``); the last sweep's weights are kept as ``robust_weights`` of the new model, whose ``noise`` is this model's.
        With ``adapt`` the loadings follow (the host form of ``Session.update(adapt=True)``): this model must carry
        ``series_stats`` (``init_series_stats``); a copy of them absorbs the new rows of the filtered W (unweighted, also under
        ``robust_c``) and the new model's H is their ridge solution with ``lambdaI`` (``trmf.online.series_ridge`` as a recursion).
        ``forget`` is fixed when the statistics are built: a different value here is refused.
        With ``smooth_back > 0`` the new rows and the ``smooth_back`` rows before them (clipped at the largest lag) are then
        smoothed (``trmf.online.smooth_rows``; the host form of ``Session.update(smooth_back=)``): a model keeps no training
        matrix, so ``Yback`` must hold the last ``smooth_back`` rows this model was trained on (raw values, like ``Ynew``).
        Together with ``robust_c`` that is refused (the smoother weights every cell fully) unless ``smooth_robust=True``: the
        window is then smoothed on Huber's loss (``trmf.online.robust_smooth_rows`` with the same ``robust_c``, ``scale`` and
        ``robust_sweeps``; the host form of ``Session.update(smooth_robust=True)``), and ``robust_weights`` of the new model are the
        smoother's, one per cell of the window.  ``smooth_robust=True`` without both ``robust_c`` and ``smooth_back > 0`` is refused.
        ``adapt_robust=True`` (needs both ``robust_c`` and ``adapt``): the statistics absorb the block with Huber weights of their
        own (``trmf.online.SeriesStats.absorb_robust`` with the same ``robust_c``, ``scale`` and ``robust_sweeps``; the host form
        of ``Session.update(adapt_robust=True)``) and ``adapt_weights`` of the new model are its weights; without the flag the
        cells enter unweighted, as before.
        ``window=N`` (the host form of ``Session.update(window=N)``): the new model keeps the last N rows only -- the oldest
        ``max(0, m + Tn - N)`` rows of W are dropped after the update, and series statistics drop their absorbed rows by as many
        (their tables keep the retired rows as exponentially forgotten history; a model holds no training matrix to downdate
        from).  An N smaller than the block + ``smooth_back`` + the largest lag + 1 is refused."""
        from .online import filter_rows, robust_filter_rows, smooth_rows, robust_smooth_rows
        if window is not None:
            from .session import check_window
            window = check_window(window, Ynew.shape[0], int(smooth_back), int(self.lag_set.max()) if len(self.lag_set) else 0)
        if adapt_robust and (robust_c is None or not adapt):
            raise ValueError('assimilate: adapt_robust=True needs both robust_c and adapt (it refits the loadings with the Huber threshold of '
                             'the robust filter)')
        smooth_back = int(smooth_back)
        if smooth_back < 0:
            raise ValueError('assimilate: smooth_back must not be negative, not {}'.format(smooth_back))
        if smooth_robust and (robust_c is None or smooth_back <= 0):
            raise ValueError('assimilate: smooth_robust=True needs both robust_c and smooth_back > 0 (it back-smooths with the Huber weights '
                             'of the robust filter)')
        if smooth_back > 0:
            if robust_c is not None and not smooth_robust:
                raise ValueError('assimilate: smooth_back together with robust_c is refused: the smoother weights every cell fully and '
                                 'would undo the Huber weights of the robust filter')
            if adapt:
                raise ValueError('assimilate: smooth_back together with adapt is refused: the rows before the block are the ones the series statistics have absorbed: smoothing them makes the statistics stale')
            if Yback is None or Yback.shape != (smooth_back, self.n):
                raise ValueError('assimilate: smooth_back needs Yback, the last {} rows of the training matrix ({} series)'.format(smooth_back, self.n))
            if smat.issparse(Yback) != smat.issparse(Ynew):
                raise ValueError('assimilate: Yback and Ynew must both be sparse or both be arrays')
        if self.transform is not None:
            if smat.issparse(Ynew):
                raise ValueError('assimilate: a series transform needs dense rows')
            Ynew = self.transform.preprocess(np.asarray(Ynew)).astype(self.W.dtype)
            if smooth_back > 0:
                Yback = self.transform.preprocess(np.asarray(Yback)).astype(self.W.dtype)
        grown = np.zeros((self.m + Ynew.shape[0], self.k), dtype=self.W.dtype, order='C')
        grown[:self.m] = self.W
        weights = None
        if robust_c is None:
            grown = filter_rows(grown, self.H, self.lag_set, self.lag_val, Ynew, self.m, lambdaI, lambdaAR, missing)
        else:
            if scale is None:
                noise = getattr(self, 'noise', None)
                if noise is None:
                    raise ValueError('assimilate: robust_c needs a scale per series or a fitted noise (Model.fit_noise)')
                scale = np.sqrt(np.asarray(noise[0], dtype=np.float64))
            grown, weights = robust_filter_rows(grown, self.H, self.lag_set, self.lag_val, Ynew, self.m, lambdaI, lambdaAR, missing,
                                                scale, robust_c, robust_sweeps)
        if smooth_back > 0:
            first = max(self.m - smooth_back, int(self.lag_set.max()) if len(self.lag_set) else 0)
            tail = Yback[smooth_back - (self.m - first):] if first < self.m else Yback[:0]
            span = smat.vstack([smat.csr_matrix(tail), smat.csr_matrix(Ynew)]).tocsr() if smat.issparse(Ynew) else np.vstack([np.asarray(tail), np.asarray(Ynew)])
            if smooth_robust:
                grown, weights = robust_smooth_rows(grown, self.H, self.lag_set, self.lag_val, span, first, lambdaI, lambdaAR, missing,
                                                    scale, robust_c, robust_sweeps)
            else:
                grown = smooth_rows(grown, self.H, self.lag_set, self.lag_val, span, first, lambdaI, lambdaAR, missing)
        retire = max(0, grown.shape[0] - window) if window is not None else 0
        out = Model.from_arrays(np.ascontiguousarray(grown[retire:]), self.H.copy(), self.lag_val.copy(), self.lag_set.copy(), transform=self.transform)
        stats = getattr(self, 'series_stats', None)
        if adapt:
            import copy
            if stats is None:
                raise ValueError('assimilate: adapt needs series statistics (Model.init_series_stats) before the first block')
            if float(forget) != stats.forget:
                raise ValueError('assimilate: forget {!r} differs from the {!r} the series statistics were built with'.format(forget, stats.forget))
            if bool(missing) != stats.missing:
                raise ValueError('assimilate: missing differs from the setting the series statistics were built with')
            if adapt_robust:
                stats = copy.deepcopy(stats)
                out.H[:], out.adapt_weights = stats.absorb_robust(grown, Ynew, self.H, lambdaI, scale, robust_c, robust_sweeps)
            else:
                stats = copy.deepcopy(stats).absorb(grown, Ynew)
                out.H[:] = stats.solve(lambdaI)
            if retire:
                stats.rows -= min(retire, stats.rows)          # (the tables keep the retired rows: forgotten history)
            out.series_stats = stats
        if weights is not None:
            out.robust_weights = weights
            if getattr(self, 'noise', None) is not None:
                out.noise = self.noise
        return out

    def init_series_stats(self, Y, forget=1.0, missing=True):
        """Attach the per-series statistics of ``assimilate(adapt=True)`` (``trmf.online.SeriesStats``), built over the training
        matrix ``Y`` (raw values; a transform of this model is applied first) with W as it is.  H is not changed."""
        from .online import SeriesStats
        if self.transform is not None:
            if smat.issparse(Y):
                raise ValueError('init_series_stats: a series transform needs dense rows')
            Y = self.transform.preprocess(np.asarray(Y)).astype(self.W.dtype)
        self.series_stats = SeriesStats(self.W, Y, forget, missing)
        return self

    # ---- series churn ------------------------------------------------------------------------------
    def _transform_of(self, a, b):
        import copy
        tr = copy.copy(self.transform)
        tr.a, tr.b = a, b
        return tr

    def retire_series(self, which):
        """A new ``Model`` without the series ``which`` (a list of indices or a mask of ``n`` flags): the kept rows of H in their
        order, W, the lag weights and the lag set as they are, the transform's coefficients gathered (the host form of
        ``Session.retire_series``).  Series statistics and a fitted noise are not carried."""
        from .session import check_keep
        keep = check_keep(which, self.n, retire=True)
        if not keep.any():
            raise ValueError('retire_series: no series would be left')
        tr = None if self.transform is None else self._transform_of(np.asarray(self.transform.a)[:, keep], np.asarray(self.transform.b)[:, keep])
        return Model.from_arrays(self.W.copy(), np.ascontiguousarray(self.H[keep]), self.lag_val.copy(), self.lag_set.copy(), transform=tr)

    def add_series(self, Ynew, lambdaI, missing=True, forget=1.0, transform_new=None):
        """A new ``Model`` grown by the ``Ynew.shape[1]`` series of ``Ynew`` (``m`` rows: the new series over every timestamp of
        this model; raw values): their loadings are the cold-start ridge ``trmf.series_ridge(W, Ynew, lambdaI, forget, missing)``
        with W as it is, appended behind the rows of H (the host form of ``Session.add_series``).  A model with a transform needs
        ``transform_new`` (an object with ``a``, ``b`` of the new series, e.g. ``NormalizedTransform(Ynew)``), which is applied to
        ``Ynew`` first and appended to the model's."""
        from .online import series_ridge
        if Ynew.shape[0] != self.m:
            raise ValueError('add_series: Ynew has {} rows, the model {}'.format(Ynew.shape[0], self.m))
        tr = None
        if self.transform is not None:
            if transform_new is None:
                raise ValueError('add_series: this model has a series transform: the new series need transform_new')
            if smat.issparse(Ynew):
                raise ValueError('add_series: a series transform needs dense rows')
            Ynew = transform_new.preprocess(np.asarray(Ynew)).astype(self.W.dtype)
            tr = self._transform_of(np.concatenate([np.asarray(self.transform.a), np.asarray(transform_new.a)], axis=1),
                                    np.concatenate([np.asarray(self.transform.b), np.asarray(transform_new.b)], axis=1))
        elif transform_new is not None:
            raise ValueError('add_series: transform_new given, but this model has no series transform')
        Hn = series_ridge(self.W, Ynew, lambdaI, forget, missing)
        return Model.from_arrays(self.W.copy(), np.ascontiguousarray(np.vstack([self.H, Hn])), self.lag_val.copy(), self.lag_set.copy(), transform=tr)

    # ---- cell revisions ----------------------------------------------------------------------------
    def revise(self, Y, rows, cols, vals=None, delete=None, update_stats=False):
        """The host form of ``Session.revise``: ``(model, Y_revised)`` for the training matrix ``Y`` (raw values) with the cells
        ``(rows[i], cols[i])`` set to ``vals[i]`` or, where ``delete[i]`` is set, removed.  A sparse ``Y`` comes back as a
        ``scipy.sparse.csr_matrix`` holding ``trmf.revise_entries`` of its entries in CSR order (every stored copy of an edited
        cell removed, the sets at the end of their rows); an array comes back as a copy with the cells overwritten (deletes are
        refused, as on the device).  The factors are carried over.  ``update_stats``: attached series statistics follow by
        ``SeriesStats.revise`` (values in the trained scale); without it they are not carried, as the device leaves them stale."""
        from .online import revise_entries, _revise_edits
        import copy
        if Y.shape != (self.m, self.n):
            raise ValueError('revise: Y is {}, the model {} x {}'.format(Y.shape, self.m, self.n))
        er, ec, ev, dl = _revise_edits((rows, cols, vals, delete), 'revise')
        if er.size and (er.max() >= self.m or ec.max() >= self.n):
            raise ValueError('revise: a cell lies outside {} x {}'.format(self.m, self.n))
        out = Model.from_arrays(self.W.copy(), self.H.copy(), self.lag_val.copy(), self.lag_set.copy(), transform=self.transform)
        stats = getattr(self, 'series_stats', None)
        if smat.issparse(Y):
            Yr = Y.tocsr()
            r0 = np.repeat(np.arange(self.m, dtype=np.int64), np.diff(Yr.indptr))
            r, c, v = revise_entries(r0, Yr.indices.astype(np.int64), Yr.data, (er, ec, ev, dl), major='row')
            ptr = np.zeros(self.m + 1, dtype=np.int64)
            np.cumsum(np.bincount(r, minlength=self.m), out=ptr[1:])
            Y2 = smat.csr_matrix((v, c, ptr), shape=Y.shape)
            trained, tv = Y, ev
        else:
            if dl.any():
                raise ValueError('revise: a delete on a dense Y (every cell is observed; set a value instead)')
            Y2 = np.array(Y, copy=True)
            Y2[er, ec] = ev.astype(Y2.dtype)
            trained, tv = Y, ev
            if self.transform is not None:
                trained = self.transform.preprocess(np.asarray(Y)).astype(self.W.dtype)
                tv = self.transform.preprocess(np.asarray(Y2)).astype(self.W.dtype)[er, ec]
        if update_stats:
            if stats is None:
                raise ValueError('revise: update_stats needs series statistics (Model.init_series_stats)')
            out.series_stats = copy.deepcopy(stats).revise(self.W, trained, (er, ec, tv, dl))
        return out, Y2

    # ---- construction ------------------------------------------------------------------------------
    @staticmethod
    def syn_gen(m, n, k, lag_set, seed=None, noise=0.01, dtype=np.float32):
        """A low-rank matrix whose temporal factor follows an AR model over ``lag_set``.  Random draws in this order:
        W, H, lag_val (standard normal), then the innovation noise of rows midx.. of W."""
        if seed is not None:
            np.random.seed(seed)
        lags = _sorted_lags(lag_set)
        W, H, theta = _empty_factors(m, n, k, len(lags), dtype)
        for target in (W, H, theta):
            target[:] = np.random.randn(*target.shape)
        theta = theta.dot(np.diag(1.0 / (np.abs(theta).sum(axis=0) + 0.1)))      # contractive columns
        start = int(lags.max())
        _ar_rollout(W, start, m, lags, theta)
        W[start:] += noise * np.random.randn(m - start, k)
        Y = np.zeros((m, n), dtype=dtype, order='C')
        Y[:] = W.dot(H.T)
        return {'W': W, 'H': H, 'lag_val': theta, 'lag_set': lags, 'Y': Y, 'k': k}

    @classmethod
    def initialize(cls, Y, lag_set, k, warm_start_model=None, seed=None, dtype=None, transform=None):
        if seed is not None:
            np.random.seed(seed)
        dtype = Y.dtype if dtype is None else dtype
        m, n = Y.shape
        lags = _sorted_lags(lag_set)
        W, H, theta = _empty_factors(m, n, k, len(lags), dtype)
        W[:] = np.random.rand(m, k)
        H[:] = np.random.rand(n, k)
        theta[:] = np.random.randn(len(lags), k)
        prev = warm_start_model
        if prev is not None:
            assert (prev.k, prev.n) == (k, n) and prev.m <= m and len(prev.lag_set) == len(lags)
            W[:] = prev.latent_forecast(m - prev.m)
            H[:] = prev.H
            theta[:] = prev.lag_val
            transform = prev.transform
        if transform is not None:                       # any request for a transform: fit a fresh one on this Y
            transform = NormalizedTransform(Y)
        return cls(PyMatrix(W, dtype), PyMatrix(H, dtype), PyMatrix(theta, dtype), lag_set=lags, transform=transform)

    def selected_lags(self, tol=0):
        """Per latent dimension, the lags of ``lag_set`` whose weight has ``|theta| > tol`` (a list of k uint32 arrays): with
        sparse lag weights (``train(..., lambdaLagL1=...)``) the lags the data uses."""
        if tol < 0:
            raise ValueError('selected_lags: tol must not be negative')
        used = np.abs(self.lag_val) > tol
        return [self.lag_set[used[:, t]] for t in range(self.k)]

    def fit(self, Y, **kw):
        """``model.fit(Y, ...)`` is ``train(Y, model, ...)``, ``lambdaLagL1`` and ``lag_refit`` included."""
        from .trmf import train
        return train(Y, self, **kw)
