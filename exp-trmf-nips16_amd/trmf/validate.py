"""Rolling-window evaluation and hyper-parameter grid of the Python front end.

Contract (same call signatures and results as the reference's python/trmf/trmf.py:303-346): the last
``nr_windows * window_size`` timestamps of ``Y`` are forecast window by window; for window ``i`` the model is
trained on the prefix that ends where the window starts, warm-started from the previous window's model rolled
forward by the AR recursion, and its ``window_size``-step forecast is stored.  The result is ``Metrics`` of all
forecasts against the truth.

What is different here is where the data lives.  The reference re-wraps the whole growing prefix for every
window; on the GPU that would be a fresh upload of everything per window.  ``rolling_validate`` instead keeps ONE
HBM-resident session for all windows (``trmf.session.Session``): the first prefix is uploaded once, each later
window only appends its new timestamps (``Session.append_rows`` -> ``trmf_session_append_rows``: CSR rows
appended, CSC rebuilt on the device, W extended on the device by the same AR recursion, H and the lag weights
stay where they are).  A per-window ``NormalizedTransform`` (the paper scripts' ``transform=True``) rescales
every entry of the prefix: the session then keeps the RAW dense matrix and applies each window's refitted
coefficients on the device (``Session.set_transform`` -> ``trmf_session_set_series_transform``), so only 2n numbers
per window are uploaded.  ``resident=False`` forces a fresh upload per window through ``train``.

``update='assimilate'`` is the online form of the same evaluation: window 0 is trained with ``max_iter`` iterations, every
later window only appends its rows and absorbs them with the forward filter (``Session.update``), H and the lag weights
staying as window 0 left them.
"""
import itertools
import pickle

import numpy as np
import scipy.sparse as smat

from .metrics import Metrics
from .model import Model, NormalizedTransform


def _as_training_matrix(block, missing):
    """Observed-entries training takes a sparse matrix whose stored entries are the non-zeros of the block."""
    return smat.csr_matrix(block) if missing else block


def _train_windows_resident(Y, lag_set, k, cuts, seed, hyper, max_iter, missing, transform, verbose, lag=None, assimilate=False, robust=None, adapt=None, smooth_back=0, window=None):
    """Yield the trained model of every window from one resident session.  With a transform (dense Y, full
    observation) the session holds the RAW matrix and applies each window's refitted coefficients on the device."""
    from .session import Session
    model = Model.initialize(Y[:cuts[0]], lag_set, k, seed=seed, transform=transform)
    with Session(_as_training_matrix(Y[:cuts[0]], missing), model, missing=missing, verbose=verbose,
                 log_norms=bool(verbose), timing=0, **dict(hyper, **(lag or {}))) as sess:      # (nobody reads per-phase times here: no phase events)
        if model.transform is not None:
            sess.set_transform(model.transform)
        sess.run(max_iter).download()
        yield model
        if robust is not None:
            _ensure_noise(sess)
        for prev_cut, cut in zip(cuts[:-1], cuts[1:]):
            if assimilate:      # online: the new rows are filtered in, nothing is retrained
                sess.update(_as_training_matrix(Y[prev_cut:cut], missing), **dict(robust or {}, **dict(adapt or {}, **dict({'smooth_back': smooth_back} if smooth_back else {}, **({'window': window} if window is not None else {})))))
                yield sess.download()
                continue
            # host-side model of the new size: same warm start the device applies, same RNG consumption as the
            # reference, and (if asked for) a transform refitted on the grown prefix
            model = Model.initialize(Y[:cut], lag_set, k, seed=seed, warm_start_model=model, transform=transform)
            sess.append_rows(_as_training_matrix(Y[prev_cut:cut], missing))
            if model.transform is not None:
                sess.set_transform(model.transform)
            sess.model = model
            sess.run(max_iter).download()
            yield model


def _ensure_noise(sess):
    """The robust filter's default scale: fitted once on window 0's model unless a table is already resident."""
    try:
        sess.noise()
    except RuntimeError:
        sess.fit_noise()


def _score_windows_on_device(Y, lag_set, k, cuts, window_size, seed, hyper, max_iter, missing, threshold, transform, verbose, lag=None,
                             assimilate=False, interval_level=None, robust=None, adapt=None, smooth_back=0):
    """The whole rolling evaluation from one resident session: every window is trained, forecast and scored on the device
    (``Session.forecast`` with the window's truth), the next window's rows are appended and, if asked for, a transform
    refitted on the grown prefix is handed over.  No factor is downloaded and no host model is rebuilt between windows.  With an
    ``interval_level`` every window also refits the noise (``Session.fit_noise``) and scores its predictive distribution
    (``Session.forecast_dist``) next to the point forecast; the result is then ``(Metrics, IntervalMetrics)``."""
    from .session import Session
    model = Model.initialize(Y[:cuts[0]], lag_set, k, seed=seed, transform=transform)
    with Session(_as_training_matrix(Y[:cuts[0]], missing), model, missing=missing, verbose=verbose,
                 log_norms=bool(verbose), timing=0, **dict(hyper, **(lag or {}))) as sess:
        if model.transform is not None:
            sess.set_transform(model.transform)
        for i, cut in enumerate(cuts):
            if i > 0:
                sess.append_rows(_as_training_matrix(Y[cuts[i - 1]:cut], missing))
                if transform is not None:
                    sess.set_transform(NormalizedTransform(Y[:cut]))
            if assimilate and i > 0:      # online: the appended rows are filtered in, nothing is retrained
                if robust is None:
                    sess.assimilate(cuts[i - 1])
                else:
                    sess.assimilate_robust(cuts[i - 1], robust['robust_c'], robust['robust_sweeps'])
                if smooth_back:           # ... the block and the rows before it smoothed
                    first = max(cuts[i - 1] - smooth_back, max(lag_set))
                    if robust is not None:    # (only with smooth_robust=True: the pair is refused otherwise)
                        sess.smooth_robust(first, robust['robust_c'], robust['robust_sweeps'])
                    else:
                        sess.smooth(first)
                if adapt is not None:     # ... and the loadings follow
                    if adapt.get('adapt_robust'):
                        sess.adapt_series_robust(robust['robust_c'], robust['robust_sweeps'])
                    else:
                        sess.adapt_series()
            else:
                sess.run(max_iter)
                if assimilate and adapt is not None:
                    sess.init_series_stats(adapt['forget'])
                if robust is not None:
                    _ensure_noise(sess)
            truth = np.ascontiguousarray(Y[cut:cut + window_size])
            sess.forecast(window_size, threshold=threshold, truth=truth, return_forecast=False)
            if interval_level is not None:
                sess.fit_noise()
                sess.forecast_dist(window_size, level=interval_level, threshold=threshold, truth=truth)
        if interval_level is not None:
            return sess.forecast_scores(), sess.interval_scores(interval_level)
        return sess.forecast_scores()


def _train_windows_fresh(Y, lag_set, k, cuts, seed, hyper, max_iter, missing, transform, threads, verbose, lag=None):
    """Yield the trained model of every window, each from its own upload (needed with a per-window transform)."""
    from .trmf import train
    model = None
    for cut in cuts:
        prefix = _as_training_matrix(Y[:cut], missing)
        model = Model.initialize(prefix, lag_set, k, seed=seed, warm_start_model=model, transform=transform)
        train(prefix, model, max_iter=max_iter, missing=missing, threads=threads, verbose=verbose, **dict(hyper, **(lag or {})))
        yield model


def rolling_validate(Y, lag_set, k=40, window_size=24, nr_windows=7, lambdaI=0.5, lambdaAR=50, lambdaLag=0.5,
                     max_iter=20, missing=True, threshold=0, transform=None, threads=16, verbose=0, seed=0,
                     resident=True, forecast_on_device=False, lambdaLagL1=0.0, lag_refit=False, update='retrain', interval_level=None,
                     robust_c=None, robust_sweeps=4, adapt_series=False, forget=1.0, smooth_back=0, smooth_robust=False,
                     adapt_robust=False, window=None):
    """``interval_level`` (e.g. 0.9; needs ``forecast_on_device=True``): every window also fits the noise of its trained model and
    scores the predictive distribution of its forecast on the device; the result is ``(Metrics, IntervalMetrics)``, the ``Metrics``
    being exactly those of the call without it.
    ``update='assimilate'``: window 0 is trained with ``max_iter`` iterations, every later window appends its rows and
    absorbs them by the forward filter (``Session.update``) instead of retraining; it needs the resident path and refuses a
    per-window transform (a refitted transform rescales the whole history, which an online update does not revisit).
    ``robust_c`` (with ``update='assimilate'`` only): the later windows are absorbed by the Huber-weighted filter
    (``Session.assimilate_robust`` with ``robust_sweeps`` rounds); the noise is fitted once after window 0 unless a table is
    already resident, and its square roots are the scale.
    ``adapt_series`` (with ``update='assimilate'`` only): after every absorbed window the loadings H are refitted from the
    resident series statistics (``Session.adapt_series``; initialised after window 0 with ``forget``), so that H follows the
    data as well; the default leaves H as window 0 trained it.
    ``smooth_back`` (with ``update='assimilate'`` only, not with ``robust_c``): after every absorbed window the block and the
    ``smooth_back`` rows before it become the joint minimiser of the objective over that window (``Session.smooth``), so that the rows
    a forecast starts from also count the rows after them; 0 leaves the filter's rows.
    ``smooth_robust=True`` (needs both ``robust_c`` and ``smooth_back > 0``): the pair is accepted and the back-smoothing is
    ``Session.smooth_robust`` with the same ``robust_c`` and ``robust_sweeps``, on Huber's loss like the filter before it.
    ``adapt_robust=True`` (needs both ``robust_c`` and ``adapt_series``): the loadings are refitted by ``Session.adapt_series_robust``
    with the same ``robust_c`` and ``robust_sweeps``, so that a spiked cell is kept out of H as it is kept out of W; without it the
    loading update takes every cell unweighted.
    ``window=N`` (with ``update='assimilate'`` only; not with ``forecast_on_device``): the session is a sliding window -- every
    absorbed block retires the oldest rows beyond N (``Session.update(window=N)``) instead of growing the resident problem; the
    default is the expanding window.
    ``lambdaLagL1`` / ``lag_refit``: sparse lag weights (``Session.set_lag_penalty``) on every path.
    ``forecast_on_device=True`` keeps the forecasts and their scoring on the device as well (one session, no download and no
    host model per window); it needs the resident path and a dense ``Y``, and says so where that does not hold."""
    T, n = Y.shape
    horizon = nr_windows * window_size
    assert T > horizon, 'series too short for {} windows of {}'.format(nr_windows, window_size)
    cuts = [T - horizon + i * window_size for i in range(nr_windows)]        # training prefix of window i = Y[:cuts[i]]
    hyper = dict(lambdaI=lambdaI, lambdaAR=lambdaAR, lambdaLag=lambdaLag)
    from .session import check_lag_penalty
    lambdaLagL1, lag_refit = check_lag_penalty(lambdaLagL1, lag_refit)
    lag = dict(lambdaLagL1=lambdaLagL1, lag_refit=lag_refit) if (lambdaLagL1 > 0 or lag_refit) else None     # None: the calls of before
    if update not in ('retrain', 'assimilate'):
        raise ValueError("update must be 'retrain' or 'assimilate', not {!r}".format(update))
    online = update == 'assimilate'
    robust = None
    if robust_c is not None:
        if not online:
            raise ValueError("robust_c: the robust filter absorbs new rows online (update='assimilate'); retraining solves plain least squares")
        robust = dict(robust_c=float(robust_c), robust_sweeps=int(robust_sweeps))
    adapt = None
    if adapt_series:
        if not online:
            raise ValueError("adapt_series: the loadings are refitted from rows absorbed online (update='assimilate'); retraining refits them anyway")
        if not (0.0 < float(forget) <= 1.0):
            raise ValueError('adapt_series: forget must lie in (0, 1], not {!r}'.format(forget))
        adapt = dict(adapt=True, forget=float(forget))
    if adapt_robust:
        if robust_c is None or not adapt_series:
            raise ValueError('adapt_robust=True needs both robust_c and adapt_series (it refits the loadings with the Huber threshold of the robust filter)')
        adapt['adapt_robust'] = True        # (Session.update's keyword)
    smooth_back = int(smooth_back)
    if smooth_back < 0:
        raise ValueError('smooth_back must not be negative, not {}'.format(smooth_back))
    if smooth_robust and (robust_c is None or smooth_back <= 0):
        raise ValueError('smooth_robust=True needs both robust_c and smooth_back > 0 (it back-smooths with the Huber weights of the robust filter)')
    if smooth_back > 0:
        if not online:
            raise ValueError("smooth_back: the smoother revisits rows absorbed online (update='assimilate'); retraining solves them jointly anyway")
        if robust is not None and not smooth_robust:
            raise ValueError('smooth_back together with robust_c is refused: the smoother weights every cell fully and would undo the Huber weights')
        if adapt is not None:
            raise ValueError('smooth_back together with adapt_series is refused: the rows before the block are the ones the series statistics have absorbed: smoothing them makes the statistics stale')
    if smooth_robust:
        robust['smooth_robust'] = True      # (Session.update's keyword)
    if window is not None:
        if not online:
            raise ValueError("window: a sliding window retires rows absorbed online (update='assimilate'); retraining uses the growing prefix")
        if forecast_on_device:
            raise ValueError('window: not together with forecast_on_device (its loop addresses rows of the growing prefix)')
        from .session import check_window
        window = check_window(window, window_size, smooth_back, max(lag_set) if len(lag_set) else 0)
    if online:
        if transform is not None:
            raise ValueError("update='assimilate': a per-window transform rescales the whole history, which an online update does not revisit")
        if not resident or not isinstance(Y, np.ndarray):
            raise ValueError("update='assimilate': needs the resident path (resident=True and a dense NumPy Y)")
    if interval_level is not None:
        from .uncertainty import z_of_level
        z_of_level(interval_level)
        if not forecast_on_device:
            raise ValueError('interval_level: the intervals are fitted and scored on the device (forecast_on_device=True)')
    if forecast_on_device:
        if not isinstance(Y, np.ndarray):
            raise ValueError('forecast_on_device: needs a dense NumPy Y (a sparse Y has no resident rolling evaluation)')
        if Y.dtype not in (np.float32, np.float64):
            raise ValueError('forecast_on_device: Y is {}, the device forecasts in float32 or float64'.format(Y.dtype))
        if not resident:
            raise ValueError('forecast_on_device: needs the resident path (resident=True)')
        if transform is not None and missing:
            raise ValueError('forecast_on_device: a transform with missing=True is refitted on the host per window; '
                             'the device applies one only to dense full-observation training (missing=False)')
        return _score_windows_on_device(Y, lag_set, k, cuts, window_size, seed, hyper, max_iter, missing, threshold, transform, verbose, lag, online,
                                        interval_level, robust, adapt, smooth_back)
    # resident: a NumPy Y, and a transform only where the device can apply it (dense full-observation training)
    if resident and isinstance(Y, np.ndarray) and (transform is None or (not missing and Y.dtype in (np.float32, np.float64))):
        models = _train_windows_resident(Y, lag_set, k, cuts, seed, hyper, max_iter, missing, transform, verbose, lag, online, robust, adapt, smooth_back, window)
    else:
        models = _train_windows_fresh(Y, lag_set, k, cuts, seed, hyper, max_iter, missing, transform, threads, verbose, lag)
    forecasts = np.zeros((horizon, n), dtype=Y.dtype, order='C')
    for i, model in enumerate(models):
        model.forecast(window_size, Ynew=forecasts[i * window_size:(i + 1) * window_size], threshold=threshold)
    return Metrics.generate(Y[T - horizon:], forecasts, missing=missing)


def _grid_points(grid_params):
    names = list(grid_params)
    for combo in itertools.product(*(grid_params[name] for name in names)):
        yield dict(zip(names, combo))


def grid_search(Y, lag_set, grid_params, pkl_file=None, **kw_args):
    """Every combination of ``grid_params`` through ``rolling_validate``; returns (all results, best by m_nd).
    Each improvement is printed; with ``pkl_file`` the result list is re-written after every combination."""
    results, best = [], Metrics.default()
    for point in _grid_points(grid_params):
        settings = dict(kw_args, **point)
        score = rolling_validate(Y, lag_set, **settings)
        results.append({'kws': settings, 'metrics': score})
        if score.m_nd < best.m_nd:
            best = score
            print(score, point)
        if pkl_file is not None:
            with open(pkl_file, 'wb') as fh:
                pickle.dump(results, fh)
    return results, best
