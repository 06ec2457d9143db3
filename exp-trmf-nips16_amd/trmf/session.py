"""HBM-resident solver sessions: ctypes wrapper over section 2 of include/trmf_abi.h.

A session uploads Y and the factors once, runs ALS iterations asynchronously on the GPU and
exposes per-iteration statistics (norms, CG counts, HIP-event phase times).  ``trmf.train`` /
``c_trmf_train`` are the stateless one-shot form of the same loop.  No reference counterpart
(SURVEY.md 8(f) rank 4).
"""
import ctypes
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int32, c_uint32, c_uint64, c_void_p

import numpy as np
import scipy.sparse as smat

from ._corelib import get_clib
from .rf_util import PyMatrix


class TrmfIterStats(ctypes.Structure):
    _fields_ = [('normF', c_double), ('normX', c_double), ('normLV', c_double),
                ('f', c_double), ('fnew', c_double), ('actred', c_double), ('prered', c_double),
                ('gnorm', c_double), ('cg_rnorm', c_double),
                ('cg_iter', c_int32), ('accepted', c_int32),
                ('ms_F', c_float), ('ms_X', c_float), ('ms_LV', c_float), ('ms_F_kernel', c_float),
                ('delta', c_double), ('cg_rnorm_direct', c_double), ('ms_X_gram', c_float), ('reserved_', c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfHeldoutSums(ctypes.Structure):
    """Sums of a held-out evaluation (include/trmf_abi.h); ``ImputeMetrics.from_sums`` turns them into scores."""
    _fields_ = [('count', c_uint64), ('count_nonzero', c_uint64), ('sq_err', c_double), ('abs_err', c_double),
                ('abs_truth', c_double), ('rel_err', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfSeriesSums(ctypes.Structure):
    """One series' sums over the scored forecasts (include/trmf_abi.h); ``Metrics.from_series_sums`` turns the table into scores."""
    _fields_ = [('abs_err', c_double), ('sq_err', c_double), ('abs_truth', c_double), ('abs_dtruth', c_double),
                ('rel_err', c_double), ('count_nonzero', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfAssimilateSums(ctypes.Structure):
    """Sums of an online update (include/trmf_abi.h): rows re-solved, their observed entries, the squared error before / after."""
    _fields_ = [('rows', c_uint64), ('entries', c_uint64), ('sq_err_before', c_double), ('sq_err_after', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfRobustSums(ctypes.Structure):
    """Sums of a robust online update (include/trmf_abi.h): those of ``TrmfAssimilateSums``, the number of down-weighted entries
    and the sum of the weights."""
    _fields_ = [('rows', c_uint64), ('entries', c_uint64), ('downweighted', c_uint64), ('weight_sum', c_double),
                ('sq_err_before', c_double), ('sq_err_after', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfSmoothSums(ctypes.Structure):
    """Sums of a smoother call (include/trmf_abi.h): those of ``TrmfAssimilateSums``, the CG steps taken, whether the stop test held,
    the relative preconditioned residual at the end and the window objective before / after."""
    _fields_ = [('rows', c_uint64), ('entries', c_uint64), ('iterations', c_int32), ('converged', c_int32), ('residual', c_double),
                ('sq_err_before', c_double), ('sq_err_after', c_double), ('objective_before', c_double), ('objective_after', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfRobustSmoothSums(ctypes.Structure):
    """Sums of a robust smoother call (include/trmf_abi.h): those of ``TrmfSmoothSums`` over all sweeps (``objective_*`` are the
    Huber objective), the number of down-weighted entries and the sum of the weights of the last sweep."""
    _fields_ = [('rows', c_uint64), ('entries', c_uint64), ('downweighted', c_uint64), ('sweeps', c_int32), ('iterations', c_int32),
                ('converged', c_int32), ('reserved', c_int32), ('residual', c_double), ('weight_sum', c_double), ('sq_err_before', c_double),
                ('sq_err_after', c_double), ('objective_before', c_double), ('objective_after', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != 'reserved'}


class TrmfAdaptSums(ctypes.Structure):
    """Sums of an online loading update (include/trmf_abi.h): series refitted, rows and entries absorbed, the squared error of the
    absorbed entries with H as it was / as it is, the largest change of an element of H."""
    _fields_ = [('series', c_uint64), ('rows', c_uint64), ('entries', c_uint64), ('sq_err_before', c_double), ('sq_err_after', c_double),
                ('max_abs_change', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfSlideSums(ctypes.Structure):
    _fields_ = [('rows_retired', c_uint64), ('entries_retired', c_uint64), ('rows_appended', c_uint64), ('entries_appended', c_uint64),
                ('rows', c_uint64), ('entries', c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class TrmfChurnSums(ctypes.Structure):
    _fields_ = [('series_before', c_uint64), ('series_retired', c_uint64), ('series_added', c_uint64), ('series', c_uint64),
                ('entries_retired', c_uint64), ('entries_added', c_uint64), ('entries', c_uint64), ('heldout_dropped', c_uint64),
                ('fitted', c_int32), ('stats_carried', c_int32), ('sq_err_new', c_double)]

    def as_dict(self):
        out = {name: int(getattr(self, name)) for name, _ in self._fields_[:8]}
        out.update(fitted=bool(self.fitted), stats_carried=bool(self.stats_carried), sq_err_new=float(self.sq_err_new))
        return out


class TrmfReviseSums(ctypes.Structure):
    _fields_ = [('edits', c_uint64), ('inserted', c_uint64), ('replaced', c_uint64), ('deleted', c_uint64), ('missed', c_uint64),
                ('copies_removed', c_uint64), ('entries_before', c_uint64), ('entries', c_uint64), ('first_row', c_int32), ('last_row', c_int32),
                ('stats_carried', c_int32)]

    def as_dict(self):
        out = {name: int(getattr(self, name)) for name, _ in self._fields_[:10]}
        out.update(stats_carried=bool(self.stats_carried))
        return out


class TrmfRobustAdaptSums(ctypes.Structure):
    """Sums of a robust online loading update (include/trmf_abi.h): those of ``TrmfAdaptSums``, the number of down-weighted
    entries and the sum of the weights of the last sweep, the Huber objective ``sum_j J_j`` before / after."""
    _fields_ = [('series', c_uint64), ('rows', c_uint64), ('entries', c_uint64), ('downweighted', c_uint64), ('sq_err_before', c_double),
                ('sq_err_after', c_double), ('max_abs_change', c_double), ('weight_sum', c_double), ('objective_before', c_double),
                ('objective_after', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfNoiseStats(ctypes.Structure):
    """Summary of a noise fit (include/trmf_abi.h)."""
    _fields_ = [('pooled_sigma2', c_double), ('sigma2_min', c_double), ('sigma2_max', c_double), ('series_pooled', c_uint64),
                ('q_min', c_double), ('q_max', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfIntervalSums(ctypes.Structure):
    """One series' interval sums over the scored forecasts (include/trmf_abi.h); ``IntervalMetrics.from_series_sums`` turns the
    table into scores."""
    _fields_ = [('cells', c_double), ('covered', c_double), ('sd_sum', c_double), ('abs_truth', c_double), ('z2_sum', c_double),
                ('nll_sum', c_double), ('crps_sum', c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TrmfTrainProfile(ctypes.Structure):
    """Split of the last c_trmf_train call of this process (include/trmf_abi.h)."""
    _fields_ = [('total_s', c_double), ('setup_s', c_double), ('upload_s', c_double), ('compute_s', c_double),
                ('download_s', c_double), ('teardown_s', c_double), ('bytes_h2d', c_double), ('bytes_d2h', c_double),
                ('iters', c_int32), ('device_mallocs', c_int32), ('pool_reused', c_int32), ('failed', c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


ALLGATHERV_FN = ctypes.CFUNCTYPE(c_int32, c_void_p, POINTER(c_uint64), c_int32, c_void_p)
_prototyped = set()


def bind(lib):
    """Attach argtypes/restypes of the build-owned entry points to a loaded library (idempotent)."""
    if id(lib) in _prototyped:
        return lib
    P = POINTER(PyMatrix)
    lib.trmf_sizeof_real.restype = c_int32
    lib.trmf_device_count.restype = c_int32
    lib.trmf_set_device.argtypes = [c_int32]; lib.trmf_set_device.restype = c_int32
    lib.trmf_last_error.restype = c_char_p
    lib.trmf_device_free_bytes.restype = ctypes.c_int64
    lib.trmf_last_train_profile.argtypes = [POINTER(TrmfTrainProfile)]; lib.trmf_last_train_profile.restype = c_int32
    lib.trmf_release_cached.restype = c_int32
    lib.trmf_session_create.argtypes = [P, POINTER(c_uint32), c_uint32, P, P, P, c_double, c_double, c_double,
                                        c_int32, c_int32, c_int32, c_int32, c_int32]
    lib.trmf_session_create.restype = c_void_p
    lib.trmf_session_run.argtypes = [c_void_p, c_int32]; lib.trmf_session_run.restype = c_int32
    lib.trmf_session_log_norms.argtypes = [c_void_p, c_int32]; lib.trmf_session_log_norms.restype = c_int32
    lib.trmf_session_set_timing.argtypes = [c_void_p, c_int32]; lib.trmf_session_set_timing.restype = c_int32
    lib.trmf_session_sync.argtypes = [c_void_p]; lib.trmf_session_sync.restype = c_int32
    if hasattr(lib, 'trmf_session_mark'):      # (absent from libraries built before round 6: scripts/ab_builds.sh loads those side by side)
        lib.trmf_session_mark.argtypes = [c_void_p]; lib.trmf_session_mark.restype = c_int32
        lib.trmf_session_rewind.argtypes = [c_void_p]; lib.trmf_session_rewind.restype = c_int32
    lib.trmf_session_append_rows.argtypes = [c_void_p, P]; lib.trmf_session_append_rows.restype = c_int32
    lib.trmf_session_rows.argtypes = [c_void_p]; lib.trmf_session_rows.restype = c_int32
    lib.trmf_session_set_series_transform.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.trmf_session_set_series_transform.restype = c_int32
    lib.trmf_session_download.argtypes = [c_void_p, P, P, P]; lib.trmf_session_download.restype = c_int32
    lib.trmf_session_stats.argtypes = [c_void_p, POINTER(TrmfIterStats), c_int32]
    lib.trmf_session_stats.restype = c_int32
    lib.trmf_session_objective.argtypes = [c_void_p]; lib.trmf_session_objective.restype = c_double
    lib.trmf_session_fsolve_bytes.argtypes = [c_void_p]; lib.trmf_session_fsolve_bytes.restype = c_double
    lib.trmf_session_describe.argtypes = [c_void_p, ctypes.c_char_p, c_int32]; lib.trmf_session_describe.restype = c_int32
    lib.trmf_session_destroy.argtypes = [c_void_p]; lib.trmf_session_destroy.restype = None
    if hasattr(lib, 'trmf_session_set_heldout'):      # (absent from libraries built before held-out evaluation)
        lib.trmf_session_set_heldout.argtypes = [c_void_p, P]; lib.trmf_session_set_heldout.restype = c_int32
        lib.trmf_session_eval_heldout.argtypes = [c_void_p, POINTER(TrmfHeldoutSums), c_void_p]
        lib.trmf_session_eval_heldout.restype = c_int32
        lib.trmf_session_set_lambdas.argtypes = [c_void_p, c_double, c_double, c_double]
        lib.trmf_session_set_lambdas.restype = c_int32
    if hasattr(lib, 'trmf_session_forecast'):         # (absent from libraries built before on-device forecasting)
        lib.trmf_session_forecast.argtypes = [c_void_p, c_int32, c_int32, c_double, P, c_void_p, c_void_p]
        lib.trmf_session_forecast.restype = c_int32
        lib.trmf_session_forecast_scores.argtypes = [c_void_p, POINTER(c_uint64), c_void_p]
        lib.trmf_session_forecast_scores.restype = c_int32
        lib.trmf_session_forecast_reset.argtypes = [c_void_p]; lib.trmf_session_forecast_reset.restype = c_int32
    if hasattr(lib, 'trmf_session_set_lag_penalty'):  # (absent from libraries built before the sparse lag weights)
        lib.trmf_session_set_lag_penalty.argtypes = [c_void_p, c_double, c_int32]; lib.trmf_session_set_lag_penalty.restype = c_int32
        lib.trmf_session_solve_lags.argtypes = [c_void_p]; lib.trmf_session_solve_lags.restype = c_int32
        lib.trmf_session_lag_stats.argtypes = [c_void_p, c_void_p, POINTER(c_int32), POINTER(c_int32)]
        lib.trmf_session_lag_stats.restype = c_int32
    if hasattr(lib, 'trmf_session_assimilate'):       # (absent from libraries built before the online updates)
        lib.trmf_session_assimilate.argtypes = [c_void_p, c_int32, POINTER(TrmfAssimilateSums), c_void_p]
        lib.trmf_session_assimilate.restype = c_int32
    if hasattr(lib, 'trmf_session_assimilate_robust'):    # (absent from libraries built before the robust online updates)
        lib.trmf_session_assimilate_robust.argtypes = [c_void_p, c_int32, c_double, c_int32, c_void_p, POINTER(TrmfRobustSums), c_void_p, c_void_p]
        lib.trmf_session_assimilate_robust.restype = c_int32
    if hasattr(lib, 'trmf_session_smooth'):           # (absent from libraries built before the smoother)
        lib.trmf_session_smooth.argtypes = [c_void_p, c_int32, c_double, c_int32, POINTER(TrmfSmoothSums), c_void_p]
        lib.trmf_session_smooth.restype = c_int32
    if hasattr(lib, 'trmf_session_smooth_robust'):    # (absent from libraries built before the robust smoother)
        lib.trmf_session_smooth_robust.argtypes = [c_void_p, c_int32, c_double, c_int32, c_void_p, c_double, c_int32, POINTER(TrmfRobustSmoothSums),
                                                   c_void_p, c_void_p]
        lib.trmf_session_smooth_robust.restype = c_int32
    if hasattr(lib, 'trmf_session_adapt_series'):     # (absent from libraries built before the online loading updates)
        lib.trmf_session_series_stats_init.argtypes = [c_void_p, c_double]; lib.trmf_session_series_stats_init.restype = c_int32
        lib.trmf_session_adapt_series.argtypes = [c_void_p, POINTER(TrmfAdaptSums), c_void_p]; lib.trmf_session_adapt_series.restype = c_int32
        lib.trmf_session_series_stats_info.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_double)]
        lib.trmf_session_series_stats_info.restype = c_int32
    if hasattr(lib, 'trmf_session_adapt_series_robust'):      # (absent from libraries built before the robust online loading updates)
        lib.trmf_session_adapt_series_robust.argtypes = [c_void_p, c_double, c_int32, c_void_p, POINTER(TrmfRobustAdaptSums), c_void_p, c_void_p,
                                                         c_void_p, c_void_p]
        lib.trmf_session_adapt_series_robust.restype = c_int32
    if hasattr(lib, 'trmf_session_slide'):            # (absent from libraries built before the sliding window)
        lib.trmf_session_slide.argtypes = [c_void_p, P, c_int32, c_int32, POINTER(TrmfSlideSums)]; lib.trmf_session_slide.restype = c_int32
        lib.trmf_device_pool_live_bytes.restype = ctypes.c_int64
    if hasattr(lib, 'trmf_session_change_series'):    # (absent from libraries built before series churn)
        lib.trmf_session_change_series.argtypes = [c_void_p, c_void_p, P, c_int32, c_void_p, c_void_p, c_void_p, POINTER(TrmfChurnSums)]
        lib.trmf_session_change_series.restype = c_int32
        lib.trmf_session_row_entries.argtypes = [c_void_p, c_void_p]; lib.trmf_session_row_entries.restype = c_int32
    if hasattr(lib, 'trmf_session_revise'):           # (absent from libraries built before the cell revisions)
        lib.trmf_session_revise.argtypes = [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, POINTER(TrmfReviseSums)]
        lib.trmf_session_revise.restype = c_int32
    if hasattr(lib, 'trmf_session_fit_noise'):        # (absent from libraries built before the forecast uncertainty)
        lib.trmf_session_fit_noise.argtypes = [c_void_p, POINTER(TrmfNoiseStats)]; lib.trmf_session_fit_noise.restype = c_int32
        lib.trmf_session_noise.argtypes = [c_void_p, c_void_p, c_void_p]; lib.trmf_session_noise.restype = c_int32
        lib.trmf_session_set_noise.argtypes = [c_void_p, c_void_p, c_void_p]; lib.trmf_session_set_noise.restype = c_int32
        lib.trmf_session_forecast_dist.argtypes = [c_void_p, c_int32, c_int32, c_double, c_double, P, c_void_p, c_void_p, c_void_p]
        lib.trmf_session_forecast_dist.restype = c_int32
        lib.trmf_session_interval_scores.argtypes = [c_void_p, POINTER(c_uint64), c_void_p]
        lib.trmf_session_interval_scores.restype = c_int32
        lib.trmf_session_interval_reset.argtypes = [c_void_p]; lib.trmf_session_interval_reset.restype = c_int32
    lib.trmf_dist_get_unique_id.argtypes = [c_void_p]; lib.trmf_dist_get_unique_id.restype = c_int32
    lib.trmf_dist_init.argtypes = [c_int32, c_int32, c_void_p]; lib.trmf_dist_init.restype = c_int32
    lib.trmf_dist_init_callback.argtypes = [c_int32, c_int32, ALLGATHERV_FN, c_void_p]
    lib.trmf_dist_init_callback.restype = c_int32
    lib.trmf_dist_init_solo.argtypes = [c_int32, c_int32]; lib.trmf_dist_init_solo.restype = c_int32
    lib.trmf_dist_rank.restype = c_int32
    lib.trmf_dist_world.restype = c_int32
    lib.trmf_dist_finalize.restype = None
    lib.trmf_partition_by_nnz.argtypes = [c_uint64, POINTER(c_uint64), c_int32, POINTER(c_uint64)]
    lib.trmf_partition_by_nnz.restype = c_int32
    _prototyped.add(id(lib))
    return lib


def lib_for(dtype):
    return bind(get_clib().lib_for(dtype))


def train_profile(dtype):
    """Split of the last ``c_trmf_train`` call made through the library of ``dtype`` (None if there was none)."""
    prof = TrmfTrainProfile()
    return prof.as_dict() if lib_for(dtype).trmf_last_train_profile(byref(prof)) == 0 else None


def _stored_per_row(pm):
    """Stored entries per row of a sparse ``PyMatrix`` (None for a dense one): ``Session`` keeps them to size the weights that
    ``assimilate_robust`` reports per stored entry."""
    if pm.type != PyMatrix.SPARSE:
        return None
    return np.diff(np.ctypeslib.as_array(pm.row_ptr, shape=(int(pm.rows) + 1,)).astype(np.int64))


def check_retire(retire):
    """The front end's argument check of ``slide``: ``retire`` as an int that is not negative."""
    if isinstance(retire, bool) or not isinstance(retire, (int, np.integer)):
        raise TypeError('retire must be an integer, not {!r}'.format(retire))
    if retire < 0:
        raise ValueError('retire must not be negative, not {}'.format(retire))
    return int(retire)


def check_keep(keep, n, retire=False):
    """The front end's argument check of ``change_series``: ``keep`` as a boolean mask of ``n`` flags (``None``: all set).  A mask is
    an array of ``n`` booleans; with ``retire`` the argument names the series that LEAVE instead -- such a mask, or a list of distinct
    indices in ``0..n-1`` -- and the complement is returned."""
    n = int(n)
    if keep is None:
        return np.ones(n, dtype=bool)
    a = np.asarray(keep)
    if a.dtype == bool:
        if a.shape != (n,):
            raise ValueError('a mask of {} flags was expected, not one of shape {}'.format(n, a.shape))
        return ~a if retire else a.copy()
    if not retire:
        raise TypeError('keep must be a boolean mask of {} flags, not {!r}'.format(n, a.dtype))
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise TypeError('which must be a boolean mask or a list of integer indices, not {!r}'.format(keep))
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= n):
        raise ValueError('a series index lies outside 0..{}'.format(n - 1))
    if np.unique(a).size != a.size:
        raise ValueError('a series index is listed twice')
    mask = np.ones(n, dtype=bool)
    mask[a] = False
    return mask


def check_window(window, block_rows, smooth_back, reach):
    """The front end's argument check of ``update(window=N)``: N holds at least the block, the rows smoothed back and the largest
    lag + 1."""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)):
        raise TypeError('window must be an integer, not {!r}'.format(window))
    need = int(block_rows) + int(smooth_back) + int(reach) + 1
    if window < need:
        raise ValueError('update: window={} is smaller than the block ({}) + smooth_back ({}) + the largest lag ({}) + 1 = {}'.format(
            window, block_rows, smooth_back, reach, need))
    return int(window)


def check_lag_penalty(lambdaLagL1, lag_refit=False):
    """The front end's argument check of the sparse lag weights: a finite ``lambdaLagL1 >= 0`` as a float, ``lag_refit`` as a bool."""
    try:
        l1 = float(lambdaLagL1)
    except (TypeError, ValueError):
        raise TypeError('lambdaLagL1 must be a number, not {!r}'.format(lambdaLagL1))
    if not np.isfinite(l1) or l1 < 0:
        raise ValueError('lambdaLagL1 must be finite and not negative, not {!r}'.format(lambdaLagL1))
    return l1, bool(lag_refit)


class Session(object):
    """``Session(Y, model, **hyper).run(iters)``; the model's arrays are refreshed by ``download()``.

    ``lambdaLagL1 > 0`` makes the lag weights sparse (an L1 penalty next to the ridge ``lambdaLag``), ``lag_refit`` re-solves
    them on the selected support; the defaults are the reference's ridge solve."""

    def __init__(self, Y, model, lambdaI=0.1, lambdaAR=0.1, lambdaLag=0.1,
                 period_W=1, period_H=1, period_Lag=2, missing=True, verbose=0, log_norms=True, timing=1,
                 lambdaLagL1=0.0, lag_refit=False):
        lambdaLagL1, lag_refit = check_lag_penalty(lambdaLagL1, lag_refit)
        self.handle = None
        self.model = model
        self.lib = lib_for(model.W.dtype)
        self.pyY = Y if isinstance(Y, PyMatrix) else PyMatrix(Y, dtype=model.W.dtype)
        self.handle = self.lib.trmf_session_create(
            byref(self.pyY), model.lag_set.ctypes.data_as(POINTER(c_uint32)), len(model.lag_set),
            byref(model.pyW), byref(model.pyH), byref(model.pylag_val),
            lambdaI, lambdaAR, lambdaLag, period_W, period_H, period_Lag, int(missing), verbose)
        if not self.handle:
            raise RuntimeError('trmf_session_create failed: ' + self.lib.trmf_last_error().decode())
        self._stored = _stored_per_row(self.pyY)
        self._per_series_stats = self._stored is not None and bool(missing)      # (the full-observation forms share one S)
        if not log_norms:       # the reference computes the ||.||^2 log lines only under verbose
            self.lib.trmf_session_log_norms(self.handle, 0)
        if timing != 1:         # phase events (ms_* of stats()) on every `timing`-th iteration only / never (0): they cost ~25 us apiece
            self._check(self.lib.trmf_session_set_timing(self.handle, int(timing)), 'trmf_session_set_timing')
        if lambdaLagL1 > 0 or lag_refit:
            try:
                self.set_lag_penalty(lambdaLagL1, lag_refit)
            except Exception:
                self.close()            # nobody else holds the native handle yet
                raise

    def _check(self, rc, what):
        if rc < 0:
            raise RuntimeError('{} failed: {}'.format(what, self.lib.trmf_last_error().decode()))
        return rc

    def run(self, iters=1):
        self._check(self.lib.trmf_session_run(self.handle, iters), 'trmf_session_run')
        return self

    def sync(self):
        self._check(self.lib.trmf_session_sync(self.handle), 'trmf_session_sync')
        return self

    def mark(self):
        """Checkpoint (W, H, lag_val, iteration counter) on the device; ``rewind()`` returns to it."""
        self._check(self.lib.trmf_session_mark(self.handle), 'trmf_session_mark')
        return self

    def rewind(self):
        self._check(self.lib.trmf_session_rewind(self.handle), 'trmf_session_rewind')
        return self

    def append_rows(self, Ynew):
        """Append the timestamps of ``Ynew`` (Tn x n, same storage class as the session's Y) to the resident problem;
        W is extended on the device by the AR recursion, H and the lag weights are kept.  ``self.model`` must be
        replaced by a model with ``rows()`` timestamps before the next ``download()``."""
        block = Ynew if isinstance(Ynew, PyMatrix) else PyMatrix(Ynew, dtype=self.model.W.dtype)
        self._check(self.lib.trmf_session_append_rows(self.handle, byref(block)), 'trmf_session_append_rows')
        if self._stored is not None:
            self._stored = np.concatenate([self._stored, _stored_per_row(block)])
        return self

    def slide(self, Ynew=None, retire=0, downdate_stats=False):
        """The sliding window: append the timestamps of ``Ynew`` (as ``append_rows`` does; ``None``: nothing) and retire the
        ``retire`` oldest rows of the resident problem, in one pass on the device.  Afterwards the session is the one a fresh
        ``Session`` would be on the retained entries in their stored order (``trmf.online.slide_entries``), ``W[retire:]`` followed
        by the AR roll-out of the block, and the current H, lag weights and transform; row numbers of every later call count from
        the new first row.  Held-out positions in retired rows are dropped, the others move up; the mark is invalidated.  Series
        statistics: their absorbed rows drop by ``retire``; with ``downdate_stats`` the retired entries' terms are also subtracted
        from ``S_j`` and ``r_j`` (``trmf.SeriesStats.retire``; sparse storage with ``missing`` only) so that the next
        ``adapt_series`` fits the retained rows alone, without it they stay as exponentially forgotten history.  ``self.model``
        is replaced by a host model of ``rows()`` timestamps (W shifted; H, lag weights, lag set and transform carried over).
        Returns ``{'rows_retired', 'entries_retired', 'rows_appended', 'entries_appended', 'rows', 'entries'}``.  A refused call
        (negative ``retire``, more than the rows held before the call, fewer than the largest lag + 1 rows left, whatever
        ``append_rows`` refuses, ``downdate_stats`` without valid per-series statistics) raises and leaves the session as it was."""
        retire = check_retire(retire)
        if not hasattr(self.lib, 'trmf_session_slide'):
            raise RuntimeError('slide: the loaded library was built before the sliding window')
        block = None
        if Ynew is not None:
            block = Ynew if isinstance(Ynew, PyMatrix) else PyMatrix(Ynew, dtype=self.model.W.dtype)
        before = self.rows()
        sums = TrmfSlideSums()
        self._check(self.lib.trmf_session_slide(self.handle, byref(block) if block is not None else None, retire, 1 if downdate_stats else 0,
                                                byref(sums)), 'trmf_session_slide')
        if self._stored is not None:
            self._stored = np.concatenate([self._stored[retire:]] + ([_stored_per_row(block)] if block is not None else []))
        if retire and getattr(self, '_heldout_rows', None) is not None:
            if getattr(self, '_heldout_cols', None) is not None:
                self._heldout_cols = self._heldout_cols[self._heldout_rows >= retire]
            self._heldout_rows = self._heldout_rows[self._heldout_rows >= retire] - retire
            self._heldout_nnz = int(self._heldout_rows.size)
        old = self.model
        moved = np.zeros((self.rows(), old.k), dtype=old.W.dtype, order='C')
        kept = old.W[retire:min(before, old.m)]
        moved[:len(kept)] = kept
        self.model = type(old).from_arrays(moved, old.H.copy(), old.lag_val.copy(), old.lag_set.copy(), transform=old.transform)
        return sums.as_dict()

    def retire_rows(self, count, downdate_stats=False):
        """``slide`` without a block: retire the ``count`` oldest rows."""
        return self.slide(None, count, downdate_stats)

    def change_series(self, keep=None, Ynew=None, fit=True, H=None, transform_new=None):
        """Series churn on the device: retire the series whose flag in ``keep`` (a boolean mask of n flags; ``None``: keep all) is
        unset and add the series of ``Ynew`` (``rows()`` x m, the new series over every timestamp held, same storage class as the
        session's Y, raw values; ``None``: nothing).  Kept series keep their order and are renumbered densely from 0, the new ones
        follow.  Afterwards the session is the one a fresh ``Session`` would be on the churned entries in their stored order
        (``trmf.churn_entries``), the current W and lag weights and ``H = [H[keep]; H_new]``.  ``fit`` (ranks up to 64): the new
        loadings are the cold-start ridge ``trmf.series_ridge(W, Ynew, lambdaI, forget, missing)`` computed on the device, ``forget``
        that of the series statistics when they are carried (valid, per series, every row absorbed) and 1 otherwise; without it
        -- or with ``H`` given, which takes the fit's place -- they are ``H`` (m x k) or zeros.  ``transform_new`` (``a``, ``b`` of the new series): needed iff a series transform is
        set.  Held-out positions of retired series are dropped; the forecast and interval scores are reset; a fitted noise is
        invalidated (``fit_noise`` again); the mark is released.  ``self.model`` is replaced by a host model of the new series
        count (H rows gathered, new rows zero until ``download()``).  Returns the sums as a dict.  A refused call raises and leaves
        the session as it was."""
        n = self.model.n
        mask = None if keep is None else check_keep(keep, n)
        if not hasattr(self.lib, 'trmf_session_change_series'):
            raise RuntimeError('change_series: the loaded library was built before series churn')
        dt = self.model.W.dtype
        block = None
        if Ynew is not None:
            block = Ynew if isinstance(Ynew, PyMatrix) else PyMatrix(Ynew, dtype=dt)
        m = int(block.cols) if block is not None else 0
        fit = bool(fit) and block is not None and H is None
        Hn = None
        if H is not None:
            Hn = np.ascontiguousarray(np.asarray(H))
            if Hn.dtype != dt or Hn.shape != (m, self.model.k):
                raise ValueError('change_series: H is {} {}, {} x {} of {} was expected'.format(Hn.shape, Hn.dtype, m, self.model.k, dt))
        ta = tb = None
        if transform_new is not None:
            ta = np.ascontiguousarray(np.asarray(transform_new.a).ravel())
            tb = np.ascontiguousarray(np.asarray(transform_new.b, dtype=dt).ravel())
            if ta.dtype != dt or ta.shape != (m,) or tb.shape != (m,):
                raise ValueError('change_series: transform_new must hold {} coefficients of {}'.format(m, dt))
        flags = None if mask is None else np.ascontiguousarray(mask.astype(np.uint8))
        sums = TrmfChurnSums()
        self._check(self.lib.trmf_session_change_series(
            self.handle, flags.ctypes.data if flags is not None else None, byref(block) if block is not None else None, 1 if fit else 0,
            Hn.ctypes.data if Hn is not None else None, ta.ctypes.data if ta is not None else None, tb.ctypes.data if tb is not None else None,
            byref(sums)), 'trmf_session_change_series')
        if mask is None and block is None:
            return sums.as_dict()
        if mask is None:
            mask = np.ones(n, dtype=bool)
        if self._stored is not None:       # sparse storage: the survivors of a row are known to the library
            per_row = np.zeros(self.rows(), dtype=np.uint64)
            self._check(self.lib.trmf_session_row_entries(self.handle, per_row.ctypes.data), 'trmf_session_row_entries')
            self._stored = per_row.astype(np.int64)
        if getattr(self, '_heldout_cols', None) is not None and not mask.all():
            stay = mask[self._heldout_cols]
            self._heldout_rows = self._heldout_rows[stay]
            self._heldout_cols = (np.cumsum(mask) - 1)[self._heldout_cols[stay]]
            self._heldout_nnz = int(self._heldout_rows.size)
        old = self.model
        Hhost = np.zeros((int(sums.series), old.k), dtype=dt, order='C')
        Hhost[:int(mask.sum())] = old.H[mask]
        if Hn is not None:
            Hhost[int(mask.sum()):] = Hn
        tr = old.transform
        if tr is not None:
            import copy
            tr = copy.copy(tr)
            a_old, b_old = np.asarray(old.transform.a), np.asarray(old.transform.b)
            tr.a = np.concatenate([a_old[:, mask]] + ([np.asarray(transform_new.a).reshape(1, -1)] if m else []), axis=1)
            tr.b = np.concatenate([b_old[:, mask]] + ([np.asarray(transform_new.b).reshape(1, -1)] if m else []), axis=1)
        self.model = type(old).from_arrays(old.W.copy(), Hhost, old.lag_val.copy(), old.lag_set.copy(), transform=tr)
        self.model.pyW.type, self.model.pyH.type = old.pyW.type, old.pyH.type      # (a (rows, 1) array is both memory orders: keep the tag)
        return sums.as_dict()

    def add_series(self, Ynew, fit=True, H=None, transform_new=None):
        """``change_series`` that only adds: the series of ``Ynew`` join behind the resident ones."""
        return self.change_series(None, Ynew, fit, H, transform_new)

    def retire_series(self, which):
        """``change_series`` that only retires: ``which`` is a list of series indices or a boolean mask of the series that leave."""
        return self.change_series(check_keep(which, self.model.n, retire=True))

    def revise(self, rows, cols, vals=None, delete=None, update_stats=False):
        """Cell revisions on the device: set the cells ``(rows[i], cols[i])`` of the resident problem to ``vals[i]`` -- a reading
        that arrives late, a provisional value that is corrected -- or, where ``delete[i]`` is set, retract them.  The cells of one
        batch are distinct and lie inside the rows and series the session holds; ``vals`` are raw values (a series transform is
        applied on the device) and may be ``None`` when every edit is a delete.  Sparse storage: every stored copy of an edited cell
        leaves both orientations, the other entries keep their stored order, and each set places one entry at the end of its row
        and of its column (``trmf.revise_entries`` is the same statement in NumPy), so the result does not depend on the order
        of the batch.  Dense storage: sets overwrite the cell; deletes are refused.  Afterwards the session is the one a fresh
        ``Session`` would be on the revised entries with the current W, H, lag weights and transform.  W, H and the lag weights are
        not touched -- ``smooth``, ``assimilate``, ``adapt_series`` or ``run`` is the caller's next call -- the mark stays valid, the
        noise and score tables stay, and the held-out set is untouched: a revised cell that is also held out stays held out.
        ``update_stats`` (sparse storage with ``missing``, valid series statistics): the removed entries' terms leave ``S_j`` and
        ``r_j`` and the sets' terms join them (``trmf.SeriesStats.revise``), so the next ``adapt_series`` refits on the revised
        data; without it -- or when the statistics have not absorbed every row -- statistics whose columns changed become stale.
        Returns ``{'edits', 'inserted', 'replaced', 'deleted', 'missed', 'copies_removed', 'entries_before', 'entries', 'first_row',
        'last_row', 'stats_carried'}``.  A refused call (a cell outside the session, a cell named twice, a delete on dense storage,
        ``update_stats`` without valid per-series statistics, sizes beyond the 32-bit device indices) raises and leaves the session
        as it was."""
        if not hasattr(self.lib, 'trmf_session_revise'):
            raise RuntimeError('revise: the loaded library was built before the cell revisions')
        dt = self.model.W.dtype
        r, c = np.asarray(rows), np.asarray(cols)
        if r.ndim != 1 or r.shape != c.shape or (r.size and not (np.issubdtype(r.dtype, np.integer) and np.issubdtype(c.dtype, np.integer))):
            raise ValueError('revise: rows and cols must be one-dimensional integer arrays of one length')
        if r.size and (r.min() < 0 or c.min() < 0 or r.max() >= 2 ** 32 or c.max() >= 2 ** 32):
            raise ValueError('revise: a cell index is negative or does not fit 32 bits')
        r32, c32 = np.ascontiguousarray(r.astype(np.uint32)), np.ascontiguousarray(c.astype(np.uint32))
        flags = None
        if delete is not None:
            d = np.asarray(delete)
            if d.shape != r.shape:
                raise ValueError('revise: delete must hold one flag per cell')
            flags = np.ascontiguousarray(d.astype(bool).astype(np.uint8))
        v = None
        if vals is not None:
            v = np.ascontiguousarray(np.asarray(vals, dtype=dt))
            if v.shape != r.shape:
                raise ValueError('revise: vals must hold one value per cell')
        elif flags is None or not flags.all():
            raise ValueError('revise: vals is needed (the batch holds sets)')
        sums = TrmfReviseSums()
        self._check(self.lib.trmf_session_revise(self.handle, int(r32.size), self._ptr(r32), self._ptr(c32), self._ptr(v), self._ptr(flags),
                                                 1 if update_stats else 0, byref(sums)), 'trmf_session_revise')
        if self._stored is not None and r32.size:      # sparse storage: the entries of a row are known to the library
            per_row = np.zeros(self.rows(), dtype=np.uint64)
            self._check(self.lib.trmf_session_row_entries(self.handle, per_row.ctypes.data), 'trmf_session_row_entries')
            self._stored = per_row.astype(np.int64)
        return sums.as_dict()

    def retract(self, rows, cols, update_stats=False):
        """``revise`` that only deletes: the cells ``(rows[i], cols[i])`` leave the resident problem (sparse storage)."""
        return self.revise(rows, cols, None, np.ones(np.asarray(rows).shape, dtype=bool), update_stats)

    def pool_live_bytes(self):
        """Bytes of device memory that live buffers of this process hold in the library's pool right now."""
        return int(self.lib.trmf_device_pool_live_bytes())

    # ---- what the online calls share: scale normalisation, output buffers, pointers, the returned tuple --------------------------
    def _series_scales(self, what, scale):
        """``scale`` as n float64 values (one value stands for all series); ``None`` stays ``None`` (the resident noise)."""
        if scale is None:
            return None
        n = self.model.n
        sc = np.asarray(scale, dtype=np.float64)
        if sc.ndim == 0:
            sc = np.full(n, float(sc))
        if sc.shape != (n,):
            raise ValueError('{}: scale has shape {}, one value per series ({}) was expected'.format(what, sc.shape, n))
        return np.ascontiguousarray(sc)

    def _row_weight_buffer(self, first_row, nr, dt):
        """Room for one weight per stored entry of rows ``first_row ..`` in CSR order, or ``nr`` x n under dense storage."""
        if self._stored is not None:
            return np.empty(int(self._stored[first_row:].sum()) if nr and first_row >= 0 else 0, dtype=dt)
        return np.empty((nr, self.model.n), dtype=dt)

    @staticmethod
    def _ptr(a):
        return a.ctypes.data if a is not None and a.size else None

    @staticmethod
    def _pack(sums, *extras):
        """``sums`` alone, or a tuple of it and every ``value`` whose ``wanted`` is set."""
        out = (sums,) + tuple(value for wanted, value in extras if wanted)
        return out if len(out) > 1 else out[0]

    def assimilate(self, first_row, return_latent=False):
        """Online update on the device: rows ``first_row .. rows()-1`` of W are re-solved in ascending order from their own
        observations and the AR prior of the rows before them, with H and the lag weights fixed (``trmf.online.filter_rows``
        is the same computation in NumPy).  Returns ``{'rows', 'entries', 'sq_err_before', 'sq_err_after'}`` -- right after
        ``append_rows`` the third is the one-step-ahead forecast error of the block -- or ``(sums, Wnew)`` with
        ``return_latent``.  The session's arrays are taken as they are: a cell stored several times is several observations
        with ``missing`` (each in the row's system, in ``entries`` and in the squared errors); without, its values add up in
        the right-hand side and the squared error of the cell is ``p^2 + sum_e y_e (y_e - 2 p)``, as in the training objective
        (``||Y||^2`` is the sum of squares of the stored values), not ``(sum_e y_e - p)^2``.  A refused call (lag 0 in the lag set, rank above 64, ``first_row`` below the largest lag, a row
        whose system is not positive definite) raises and leaves the session as it was."""
        first_row = int(first_row)
        sums = TrmfAssimilateSums()
        Wnew = None
        if return_latent:
            Wnew = np.empty((max(self.rows() - first_row, 0), self.model.k), dtype=self.model.W.dtype)
        self._check(self.lib.trmf_session_assimilate(self.handle, first_row, byref(sums), self._ptr(Wnew)),
                    'trmf_session_assimilate')
        return self._pack(sums.as_dict(), (return_latent, Wnew))

    def assimilate_robust(self, first_row, c=3.0, sweeps=4, scale=None, return_latent=False, return_weights=False):
        """``assimilate`` with Huber weights (``trmf.online.robust_filter_rows`` is the same computation in NumPy): an entry whose
        residual lies beyond ``c * scale[j]`` of its series enters its row's system with the weight ``c * scale[j] / |r|``
        instead of 1, over ``sweeps`` rounds of reweighting per row.  ``scale``: n positive values (or one for all), default the
        square roots of the resident noise table (``fit_noise`` / ``set_noise``), which is the in-sample residual scale: ``c``
        below about 2 then flags ordinary cells.  Returns ``{'rows', 'entries', 'downweighted', 'weight_sum', 'sq_err_before',
        'sq_err_after'}``, followed by ``Wnew`` with ``return_latent`` and by the last sweep's weights with ``return_weights``:
        one per stored entry of the rows in CSR order (``missing``), or a ``(rows() - first_row) x n`` matrix (dense storage
        without ``missing``).  A weight below 1 marks an anomalous cell.  A refused call (everything ``assimilate`` refuses; no
        scale and no resident noise; a scale that is not finite and positive; ``c`` not positive; ``sweeps`` outside 1..64; sparse
        storage without ``missing``) raises and leaves the session as it was."""
        first_row = int(first_row)
        dt = self.model.W.dtype
        nr = max(self.rows() - first_row, 0)
        sc = self._series_scales('assimilate_robust', scale)
        sums = TrmfRobustSums()
        Wnew = np.empty((nr, self.model.k), dtype=dt) if return_latent else None
        weights = self._row_weight_buffer(first_row, nr, dt) if return_weights else None
        self._check(self.lib.trmf_session_assimilate_robust(self.handle, first_row, float(c), int(sweeps), self._ptr(sc), byref(sums), self._ptr(Wnew), self._ptr(weights)),
                    'trmf_session_assimilate_robust')
        return self._pack(sums.as_dict(), (return_latent, Wnew), (return_weights, weights))

    def smooth(self, first_row, rtol=None, max_iter=None, return_latent=False):
        """Fixed-interval smoother on the device: rows ``first_row .. rows()-1`` of W become the JOINT minimiser of the training
        objective restricted to them, with H, the lag weights and every earlier row fixed (``trmf.online.smooth_rows`` is the same
        statement in NumPy, solved directly) -- what the X-solve would give for those rows if nothing else moved, by preconditioned
        conjugate gradients over the window.  ``rtol``: the stop ``r.z <= rtol^2 (r.z)_0`` (default 1e-5 in float32, 2e-14 in
        float64); ``max_iter`` (default 500): a call that reaches it still commits, with ``converged == 0``.  Returns ``{'rows',
        'entries', 'iterations', 'converged', 'residual', 'sq_err_before', 'sq_err_after', 'objective_before', 'objective_after'}``,
        or ``(sums, Wnew)`` with ``return_latent``.  A refused call (everything ``assimilate`` refuses, a window of more than 1024
        rows, an ``rtol`` that is not finite) raises and leaves the session as it was."""
        first_row = int(first_row)
        sums = TrmfSmoothSums()
        Wnew = None
        if return_latent:
            Wnew = np.empty((max(self.rows() - first_row, 0), self.model.k), dtype=self.model.W.dtype)
        self._check(self.lib.trmf_session_smooth(self.handle, first_row, 0.0 if rtol is None else float(rtol), 0 if max_iter is None else int(max_iter),
                                                 byref(sums), self._ptr(Wnew)), 'trmf_session_smooth')
        return self._pack(sums.as_dict(), (return_latent, Wnew))

    def smooth_robust(self, first_row, c=3.0, sweeps=4, scale=None, rtol=None, max_iter=None, return_latent=False, return_weights=False):
        """``smooth`` on Huber's loss (``trmf.online.robust_smooth_rows`` is the same statement in NumPy, every sweep solved
        directly): ``sweeps`` rounds of reweighting, each one the smoother's system with every cell weighted by ``c * scale[j] /
        |r|`` where its residual at the rows of the round before lies beyond ``c * scale[j]``, solved by the smoother's PCG from
        those rows.  ``c``, ``sweeps``, ``scale`` as for ``assimilate_robust``; ``rtol``, ``max_iter`` as for ``smooth``, per sweep.
        The Huber objective never rises, also when a sweep stops at ``max_iter`` (``converged == 0``; the call still commits).
        Returns ``{'rows', 'entries', 'downweighted', 'sweeps', 'iterations', 'converged', 'residual', 'weight_sum', 'sq_err_before',
        'sq_err_after', 'objective_before', 'objective_after'}`` (``iterations`` over all sweeps, ``residual`` of the last), followed
        by ``Wnew`` with ``return_latent`` and by the last sweep's weights with ``return_weights`` (the layout of
        ``assimilate_robust``).  A refused call (everything ``smooth`` and ``assimilate_robust`` refuse) raises and leaves the
        session as it was."""
        first_row = int(first_row)
        dt = self.model.W.dtype
        nr = max(self.rows() - first_row, 0)
        sc = self._series_scales('smooth_robust', scale)
        sums = TrmfRobustSmoothSums()
        Wnew = np.empty((nr, self.model.k), dtype=dt) if return_latent else None
        weights = self._row_weight_buffer(first_row, nr, dt) if return_weights else None
        self._check(self.lib.trmf_session_smooth_robust(self.handle, first_row, float(c), int(sweeps), self._ptr(sc), 0.0 if rtol is None else float(rtol),
                                                        0 if max_iter is None else int(max_iter), byref(sums), self._ptr(Wnew), self._ptr(weights)),
                    'trmf_session_smooth_robust')
        return self._pack(sums.as_dict(), (return_latent, Wnew), (return_weights, weights))

    def _reach(self):
        return int(self.model.lag_set.max()) if len(self.model.lag_set) else 0

    def init_series_stats(self, forget=1.0):
        """Build the resident per-series statistics ``S_j``, ``r_j`` of ``adapt_series`` over all rows with W as it is, weighted by
        ``forget ** (rows() - 1 - t)`` (``forget`` in (0, 1]; 1: no forgetting).  One pass as heavy as an F-solve; H is not
        changed.  The tables cost ``n k (k + 1) / 2`` reals twice (one shared ``S`` without ``missing``)."""
        self._check(self.lib.trmf_session_series_stats_init(self.handle, float(forget)), 'trmf_session_series_stats_init')

    def adapt_series(self, return_loadings=False):
        """Online loading update on the device: the rows appended since the statistics were last brought up to date are absorbed
        into them (``S <- forget^m S + sum_new forget^(rows-1-t) w_t w_t^T`` with W as it is now, ``r`` likewise) and every row of H
        is refitted, ``h_j = (S_j + lambdaI I)^-1 r_j`` (``trmf.online.series_ridge`` is the same computation in NumPy, a direct
        sum).  W and the lag weights stay.  Huber weights of ``assimilate_robust`` are not part of the statistics: the cells enter
        unweighted (``adapt_series_robust`` is the weighted update).  Returns ``{'series', 'rows', 'entries', 'sq_err_before', 'sq_err_after', 'max_abs_change'}``, or ``(sums,
        Hnew)`` with ``return_loadings``.  A refused call (no statistics, or stale ones after ``run``, ``rewind``, ``assimilate``
        below the absorbed rows or a new transform; rank above 64; a series whose system is not positive definite, possible only
        with ``lambdaI == 0``) raises and leaves the session as it was."""
        sums = TrmfAdaptSums()
        Hnew = np.empty((self.model.n, self.model.k), dtype=self.model.W.dtype) if return_loadings else None
        self._check(self.lib.trmf_session_adapt_series(self.handle, byref(sums), self._ptr(Hnew)),
                    'trmf_session_adapt_series')
        return self._pack(sums.as_dict(), (return_loadings, Hnew))

    def adapt_series_robust(self, c=3.0, sweeps=4, scale=None, return_loadings=False, return_weights=False):
        """``adapt_series`` with Huber weights on the entries it absorbs (``trmf.online.SeriesStats.absorb_robust`` is the same
        statement in NumPy): over ``sweeps`` rounds every new entry whose residual against the loadings of the round before lies
        beyond ``c * scale[j]`` enters ``S_j`` and ``r_j`` with the weight ``c * scale[j] / |r|`` instead of 1; every round restarts
        from the decayed old tables, and the last round's tables and loadings are kept.  ``c``, ``sweeps``, ``scale`` as for
        ``assimilate_robust``.  The weights are this call's own (residuals against H with W as it is now), not the filter's.
        Sparse storage with ``missing`` only.  Returns ``{'series', 'rows', 'entries', 'downweighted', 'sq_err_before',
        'sq_err_after', 'max_abs_change', 'weight_sum', 'objective_before', 'objective_after'}`` (the objectives:
        ``trmf.robust_series_objective``), followed by ``Hnew`` with ``return_loadings`` and by the last sweep's weights with
        ``return_weights``: a ``scipy.sparse.csc_matrix`` of shape (rows absorbed) x n with one value per absorbed entry (a cell
        stored twice keeps two).  A refused call (everything ``adapt_series`` refuses; no scale and no resident noise; a scale that
        is not finite and positive; ``c`` not positive; ``sweeps`` outside 1..64; dense storage or no ``missing``, which keep one
        shared S) raises and leaves the session as it was."""
        dt = self.model.W.dtype
        n = self.model.n
        sc = self._series_scales('adapt_series_robust', scale)
        sums = TrmfRobustAdaptSums()
        Hnew = np.empty((n, self.model.k), dtype=dt) if return_loadings else None
        row0 = self.series_stats_info()['absorbed_rows']
        m = max(self.rows() - row0, 0)
        wptr = wrows = weights = None
        if return_weights:
            cap = int(self._stored[row0:].sum()) if self._stored is not None and m else 0
            wptr, wrows, weights = np.zeros(n + 1, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.ones(cap, dtype=dt)
        self._check(self.lib.trmf_session_adapt_series_robust(self.handle, float(c), int(sweeps), self._ptr(sc), byref(sums), self._ptr(Hnew), self._ptr(wptr), self._ptr(wrows),
                                                              self._ptr(weights)), 'trmf_session_adapt_series_robust')
        wmat = smat.csc_matrix((weights, wrows.astype(np.int64) - row0, wptr.astype(np.int64)), shape=(m, n)) if return_weights else None
        return self._pack(sums.as_dict(), (return_loadings, Hnew), (return_weights, wmat))

    def series_stats_info(self):
        """``{'valid', 'stale', 'absorbed_rows', 'forget'}`` of the resident series statistics (absent ones: neither valid nor stale)."""
        v, rows, g = c_int32(0), c_int32(0), c_double(1.0)
        self._check(self.lib.trmf_session_series_stats_info(self.handle, byref(v), byref(rows), byref(g)), 'trmf_session_series_stats_info')
        return {'valid': v.value == 1, 'stale': v.value == -1, 'absorbed_rows': int(rows.value), 'forget': float(g.value)}

    def update(self, Ynew, iters=0, robust_c=None, robust_sweeps=4, scale=None, adapt=False, forget=1.0, smooth_back=0, smooth_robust=False,
               adapt_robust=False, window=None, downdate_stats=False, revisions=None):
        """Absorb the new timestamps ``Ynew`` (as for ``append_rows``): append them, assimilate the new block, run ``iters``
        ALS iterations if asked for.  ``self.model`` is replaced by a host model of ``rows()`` timestamps (H, lag weights, lag
        set and transform carried over; its arrays are filled by the next ``download()``).  Returns the sums of ``assimilate``;
        with ``robust_c`` the block is absorbed by ``assimilate_robust(before, robust_c, robust_sweeps, scale)`` and its sums
        are returned.  With ``adapt`` the loadings follow: the series statistics are initialised with ``forget`` before the
        append if the session has none (existing ones keep their own), ``adapt_series`` runs after the block has been assimilated
        and ``(sums, adapt_sums)`` is returned.  With ``smooth_back > 0`` the block and the ``smooth_back`` rows before it are then
        smoothed, ``smooth(before - smooth_back)`` clipped at the largest lag; its sums are returned as ``sums['smooth']``.  Together with ``robust_c`` that is refused (the smoother
        weights every cell fully and would undo the Huber weights) unless ``smooth_robust=True`` is passed: the back-smoothing
        is then ``smooth_robust`` with the same ``robust_c``, ``scale`` and ``robust_sweeps``.  ``smooth_robust=True`` without both
        ``robust_c`` and ``smooth_back > 0`` is refused.  ``smooth_back`` with ``adapt`` is refused: the rows before the block are the
        ones the series statistics have absorbed.  Under ``robust_c`` the loading update of ``adapt`` still takes every cell
        unweighted unless ``adapt_robust=True`` is passed: the block's loading update is then ``adapt_series_robust`` with the same
        ``robust_c``, ``scale`` and ``robust_sweeps``.  ``adapt_robust=True`` without both ``robust_c`` and ``adapt`` is refused.  With ``window=N`` the session is a
        sliding window of at most N rows: the append becomes ``slide(Ynew, max(0, rows() + Tn - N), downdate_stats)`` and every later
        step runs on the shifted row numbers; an N smaller than the block + ``smooth_back`` + the largest lag + 1 is refused before the
        session is touched.  Without ``window`` the session grows as before.  ``revisions=(rows, cols, vals)``: late or corrected
        cells of the rows already held, applied by ``revise`` BEFORE the block is appended (under ``adapt`` with ``update_stats`` where the
        statistics are per series, so that they follow); with ``smooth_back`` the smoothed window is widened back to the first revised row (clipped at
        the largest lag), and a window beyond the smoother's cap raises the smoother's own error.  Its sums are returned as
        ``sums['revise']``."""
        smooth_back = int(smooth_back)
        if smooth_back < 0:
            raise ValueError('update: smooth_back must not be negative, not {}'.format(smooth_back))
        if adapt_robust and (robust_c is None or not adapt):
            raise ValueError('update: adapt_robust=True needs both robust_c and adapt (it refits the loadings with the Huber threshold of '
                             'the robust filter)')
        if smooth_robust and (robust_c is None or smooth_back <= 0):
            raise ValueError('update: smooth_robust=True needs both robust_c and smooth_back > 0 (it back-smooths with the Huber weights '
                             'of the robust filter)')
        if smooth_back > 0 and robust_c is not None and not smooth_robust:
            raise ValueError('update: smooth_back together with robust_c is refused: the smoother weights every cell fully and would '
                             'undo the Huber weights of the robust filter')
        if smooth_back > 0 and adapt:
            raise ValueError('update: smooth_back together with adapt is refused: the rows before the block are the ones the series statistics have absorbed: smoothing them makes the statistics stale')
        before = self.rows()
        retire = 0
        if window is not None:
            block = Ynew if isinstance(Ynew, PyMatrix) else PyMatrix(Ynew, dtype=self.model.W.dtype)
            Ynew = block
            retire = max(0, before + int(block.rows) - check_window(window, int(block.rows), smooth_back, self._reach()))
        elif downdate_stats:
            raise ValueError('update: downdate_stats needs window')
        if adapt:
            info = self.series_stats_info()
            if info['stale']:       # before anything is appended: a refused update leaves the session as it was
                raise RuntimeError('update: the series statistics are stale (run, rewind, assimilate below the absorbed rows or a new '
                                   'transform since they were built); initialise them again (init_series_stats)')
            if not info['valid']:
                self.init_series_stats(forget)
        revised = None
        if revisions is not None:
            if len(revisions) != 3:
                raise ValueError('update: revisions must be (rows, cols, vals)')
            revised = self.revise(revisions[0], revisions[1], revisions[2], update_stats=bool(adapt) and getattr(self, '_per_series_stats', False))
        if window is not None:
            self.slide(Ynew, retire, downdate_stats)
            before -= retire                                 # the block's first row, counted from the new first row
        else:
            self.append_rows(Ynew)
            old = self.model
            grown = np.zeros((self.rows(), old.k), dtype=old.W.dtype, order='C')
            grown[:min(before, old.m)] = old.W[:before]
            self.model = type(old).from_arrays(grown, old.H.copy(), old.lag_val.copy(), old.lag_set.copy(), transform=old.transform)
        sums = self.assimilate(before) if robust_c is None else self.assimilate_robust(before, robust_c, robust_sweeps, scale)
        if smooth_back > 0:
            first = before - smooth_back
            if revised is not None and revised['first_row'] >= 0:
                first = min(first, revised['first_row'] - retire)     # the window reaches back to the first revised row
            first = max(first, self._reach())
            sums['smooth'] = self.smooth_robust(first, robust_c, robust_sweeps, scale) if smooth_robust else self.smooth(first)
        if adapt_robust:
            adapted = self.adapt_series_robust(robust_c, robust_sweeps, scale)
        else:
            adapted = self.adapt_series() if adapt else None
        if revised is not None:
            sums['revise'] = revised
        if iters:
            self.run(int(iters))
        return (sums, adapted) if adapt else sums

    def set_transform(self, transform):
        """Train on ``transform.preprocess`` of the raw dense Y held by the session (``None``: the raw values); the
        coefficients (``a``, ``b`` of a ``NormalizedTransform``, which have the dtype of the Y they were fitted on)
        are applied on the device in the session's element type, as NumPy evaluates ``Y * a + b``."""
        if transform is None:
            rc = self.lib.trmf_session_set_series_transform(self.handle, None, None)
        else:
            dt = self.model.W.dtype
            if np.asarray(transform.a).dtype != dt:
                raise TypeError('transform coefficients are {}, the session trains in {}'.format(np.asarray(transform.a).dtype, dt))
            a = np.ascontiguousarray(np.asarray(transform.a).ravel())
            b = np.ascontiguousarray(np.asarray(transform.b, dtype=dt).ravel())
            rc = self.lib.trmf_session_set_series_transform(self.handle, a.ctypes.data, b.ctypes.data)
        self._check(rc, 'trmf_session_set_series_transform')
        return self

    def rows(self):
        return self._check(self.lib.trmf_session_rows(self.handle), 'trmf_session_rows')

    def set_lambdas(self, lambdaI, lambdaAR, lambdaLag):
        """New regularisation weights for the iterations run from now on (with ``rewind()``: a grid over the weights
        from one resident problem and one initial model)."""
        self._check(self.lib.trmf_session_set_lambdas(self.handle, lambdaI, lambdaAR, lambdaLag), 'trmf_session_set_lambdas')
        return self

    def set_lag_penalty(self, lambdaLagL1, lag_refit=False):
        """L1 weight of the lag weights (and the refit on the selected support) for the lag-weight solves run from now on;
        ``(0, False)`` restores the ridge solve exactly.  The library refuses a negative or non-finite weight and stays usable."""
        self._check(self.lib.trmf_session_set_lag_penalty(self.handle, float(lambdaLagL1), int(bool(lag_refit))), 'trmf_session_set_lag_penalty')
        return self

    def solve_lags(self):
        """Recompute the lag weights from the session's current W with the current penalties (the lag-weight phase on its own)."""
        self._check(self.lib.trmf_session_solve_lags(self.handle), 'trmf_session_solve_lags')
        return self

    def lag_stats(self):
        """Record of the last lag-weight solve: ``{'per_dim': k x 4 int32 (sweeps, non-zeros, capped, refit skipped), 'capped': int,
        'refit_skipped': int}``; all zero after a ridge solve."""
        per_dim = np.zeros((self.model.k, 4), dtype=np.int32)
        capped, skipped = c_int32(0), c_int32(0)
        self._check(self.lib.trmf_session_lag_stats(self.handle, per_dim.ctypes.data, byref(capped), byref(skipped)), 'trmf_session_lag_stats')
        return {'per_dim': per_dim, 'capped': int(capped.value), 'refit_skipped': int(skipped.value)}

    def set_heldout(self, Ytest):
        """Upload the held-out positions and truths: a sparse T' x n matrix (T' <= rows()) whose STORED entries, explicit
        zeros included, are the cells to score, in the scale the session trains on.  ``None`` drops the set."""
        if Ytest is None:
            self._check(self.lib.trmf_session_set_heldout(self.handle, None), 'trmf_session_set_heldout')
            self._heldout_nnz = self._heldout_rows = self._heldout_cols = None
            return self
        if isinstance(Ytest, PyMatrix):
            pyT = Ytest
        elif smat.issparse(Ytest):
            pyT = PyMatrix(Ytest, dtype=self.model.W.dtype)
        else:
            raise TypeError('set_heldout: a scipy.sparse matrix is required (its stored entries are the held-out cells)')
        self._check(self.lib.trmf_session_set_heldout(self.handle, byref(pyT)), 'trmf_session_set_heldout')
        self._heldout_nnz = int(pyT.nnz)
        self._heldout_rows = np.repeat(np.arange(int(pyT.rows), dtype=np.int64), _stored_per_row(pyT))     # (slide drops the retired rows' cells)
        self._heldout_cols = np.ctypeslib.as_array(pyT.col_idx, shape=(int(pyT.nnz),)).astype(np.int64) if pyT.nnz else np.zeros(0, np.int64)     # (change_series drops the retired series' cells)
        return self

    def eval_heldout_sums(self, predictions=False):
        """The six sums of the held-out set (a dict), plus the predictions in the set's CSR order if asked for."""
        sums = TrmfHeldoutSums()
        pred = None
        if predictions:
            nnz = getattr(self, '_heldout_nnz', None)
            pred = np.empty(nnz or 0, dtype=self.model.W.dtype)
        self._check(self.lib.trmf_session_eval_heldout(self.handle, byref(sums), pred.ctypes.data if pred is not None and pred.size else None),
                    'trmf_session_eval_heldout')
        return (sums.as_dict(), pred) if predictions else sums.as_dict()

    def eval_heldout(self, predictions=False):
        """``ImputeMetrics`` of the current model on the held-out set (computed on the device); with ``predictions=True`` a
        pair (metrics, predictions in the set's CSR order)."""
        from .impute import ImputeMetrics
        if predictions:
            sums, pred = self.eval_heldout_sums(True)
            return ImputeMetrics.from_sums(sums), pred
        return ImputeMetrics.from_sums(self.eval_heldout_sums())

    def _truth_matrix(self, truth, what):
        """The truth of a forecast as a PyMatrix of the session's dtype (``None`` stays ``None``)."""
        dt = np.dtype(self.model.W.dtype)
        if truth is None or isinstance(truth, PyMatrix):
            return truth
        if smat.issparse(truth):
            return PyMatrix(truth, dtype=dt)               # refused by the library: the truth of a forecast is dense
        truth = np.asarray(truth)
        if truth.dtype != dt:
            raise TypeError('{}: the truth is {}, the session forecasts in {}'.format(what, truth.dtype, dt))
        if truth.ndim != 2:
            raise ValueError('{}: the truth must be a steps x n array'.format(what))
        return PyMatrix(truth, dtype=dt)

    def forecast(self, steps, threshold=None, truth=None, return_forecast=True, return_latent=False):
        """The next ``steps`` timestamps from the current factors, on the device: W rolled forward by the AR model (the bits of
        ``Model.latent_forecast``), times H, clipped from below at ``threshold`` if one is given, mapped back through the session's
        series transform if one is active.  With ``truth`` (``steps x n``, raw values of the session's dtype) the forecast is also
        scored into the resident per-series table (``forecast_scores``).  Returns ``Ynew``, ``(Ynew, Wnew)`` with
        ``return_latent``, ``Wnew`` alone without ``return_forecast``, or ``None``.  Nothing the training sees is changed."""
        dt = np.dtype(self.model.W.dtype)
        n, k = self.model.n, self.model.k
        steps = int(steps)
        pyT = self._truth_matrix(truth, 'forecast')
        Ynew = np.empty((max(steps, 0), n), dtype=dt) if return_forecast else None
        Wnew = np.empty((max(steps, 0), k), dtype=dt) if return_latent else None
        self._check(self.lib.trmf_session_forecast(
            self.handle, steps, int(threshold is not None), float(threshold) if threshold is not None else 0.0,
            byref(pyT) if pyT is not None else None,
            Ynew.ctypes.data if Ynew is not None else None, Wnew.ctypes.data if Wnew is not None else None), 'trmf_session_forecast')
        if return_forecast and return_latent:
            return Ynew, Wnew
        return Ynew if return_forecast else Wnew

    def forecast_series_sums(self):
        """(rows scored since the last reset, n x 6 float64 table in ``TrmfSeriesSums`` order)."""
        rows = c_uint64(0)
        table = np.zeros((self.model.n, len(TrmfSeriesSums._fields_)), dtype=np.float64)
        self._check(self.lib.trmf_session_forecast_scores(self.handle, byref(rows), table.ctypes.data), 'trmf_session_forecast_scores')
        return int(rows.value), table

    def forecast_scores(self):
        """``Metrics`` of every forecast scored since the last reset (the sums were formed on the device)."""
        from .metrics import Metrics
        return Metrics.from_series_sums(*self.forecast_series_sums())

    def reset_forecast_scores(self):
        self._check(self.lib.trmf_session_forecast_reset(self.handle), 'trmf_session_forecast_reset')
        return self

    # ---- forecast uncertainty (trmf.uncertainty is the same computation in NumPy) ------------------------------------------
    def fit_noise(self):
        """Fit the observation noise per series and the innovation variance per latent dimension on the session's current factors
        and training matrix, on the device, into resident tables (``trmf.uncertainty.fit_noise``).  Later ``run`` /
        ``assimilate`` / ``append_rows`` / ``rewind`` calls neither refit nor invalidate them: call again when the model has
        moved.  A cell that sparse storage holds several times counts as the training objective counts it (one residual per
        stored entry with ``missing``; ``p^2 + sum_e y_e (y_e - 2 p)`` without).
        Returns ``{'pooled_sigma2', 'sigma2_min', 'sigma2_max', 'series_pooled', 'q_min', 'q_max'}``."""
        stats = TrmfNoiseStats()
        self._check(self.lib.trmf_session_fit_noise(self.handle, byref(stats)), 'trmf_session_fit_noise')
        return stats.as_dict()

    def noise(self):
        """``(sigma2, q)``: the resident variances, n and k float64 values."""
        sigma2, q = np.zeros(self.model.n, dtype=np.float64), np.zeros(self.model.k, dtype=np.float64)
        self._check(self.lib.trmf_session_noise(self.handle, sigma2.ctypes.data, q.ctypes.data), 'trmf_session_noise')
        return sigma2, q

    def set_noise(self, sigma2, q):
        """Replace the resident variances (finite, not negative), e.g. by out-of-sample ones."""
        sigma2 = np.ascontiguousarray(sigma2, dtype=np.float64).ravel()
        q = np.ascontiguousarray(q, dtype=np.float64).ravel()
        if sigma2.shape != (self.model.n,) or q.shape != (self.model.k,):
            raise ValueError('set_noise: sigma2 must have n = {} values and q k = {}'.format(self.model.n, self.model.k))
        self._check(self.lib.trmf_session_set_noise(self.handle, sigma2.ctypes.data, q.ctypes.data), 'trmf_session_set_noise')
        return self

    def forecast_dist(self, steps, level=0.9, threshold=None, truth=None, return_latent=False):
        """``(Ynew, Ysd)`` -- or ``(Ynew, Ysd, Wnew)`` -- of the next ``steps`` timestamps: ``Ynew`` (and ``Wnew``) exactly as
        ``forecast`` returns them, ``Ysd`` the predictive standard deviation in the same units.  Needs ``fit_noise`` or
        ``set_noise`` first.  With ``truth`` the cells are scored into the resident interval table (``interval_scores``), the
        central ``level`` interval deciding ``coverage``.  A plug-in estimate: see ``trmf.uncertainty``."""
        from .uncertainty import z_of_level
        dt = np.dtype(self.model.W.dtype)
        n, k = self.model.n, self.model.k
        steps = int(steps)
        zq = z_of_level(level)
        pyT = self._truth_matrix(truth, 'forecast_dist')
        Ynew = np.empty((max(steps, 0), n), dtype=dt)
        Ysd = np.empty((max(steps, 0), n), dtype=dt)
        Wnew = np.empty((max(steps, 0), k), dtype=dt) if return_latent else None
        self._check(self.lib.trmf_session_forecast_dist(
            self.handle, steps, int(threshold is not None), float(threshold) if threshold is not None else 0.0, zq,
            byref(pyT) if pyT is not None else None, Ynew.ctypes.data, Ysd.ctypes.data,
            Wnew.ctypes.data if Wnew is not None else None), 'trmf_session_forecast_dist')
        return (Ynew, Ysd, Wnew) if return_latent else (Ynew, Ysd)

    def forecast_interval(self, steps, level=0.9, threshold=None, truth=None):
        """``(Ynew, lo, hi)``: the forecast and its central ``level`` interval ``Ynew -+ zq Ysd`` (``lo`` clipped from below at
        ``threshold`` when one is given)."""
        from .uncertainty import z_of_level
        Ynew, Ysd = self.forecast_dist(steps, level=level, threshold=threshold, truth=truth)
        half = Ysd * Ynew.dtype.type(z_of_level(level))
        lo, hi = Ynew - half, Ynew + half
        if threshold is not None:
            np.maximum(lo, Ynew.dtype.type(threshold), out=lo)
        return Ynew, lo, hi

    def interval_series_sums(self):
        """(rows scored by ``forecast_dist`` since the last reset, n x 7 float64 table in ``TrmfIntervalSums`` order)."""
        rows = c_uint64(0)
        table = np.zeros((self.model.n, len(TrmfIntervalSums._fields_)), dtype=np.float64)
        self._check(self.lib.trmf_session_interval_scores(self.handle, byref(rows), table.ctypes.data), 'trmf_session_interval_scores')
        return int(rows.value), table

    def interval_scores(self, level=0.9):
        """``IntervalMetrics`` of every cell scored since the last reset; ``level`` must be the one the calls were scored with."""
        from .uncertainty import IntervalMetrics
        return IntervalMetrics.from_series_sums(self.interval_series_sums()[1], level)

    def reset_interval_scores(self):
        self._check(self.lib.trmf_session_interval_reset(self.handle), 'trmf_session_interval_reset')
        return self

    def download(self):
        m = self.model
        self._check(self.lib.trmf_session_download(self.handle, byref(m.pyW), byref(m.pyH), byref(m.pylag_val)),
                    'trmf_session_download')
        return m

    def stats(self, last=64):
        buf = (TrmfIterStats * last)()
        cnt = self._check(self.lib.trmf_session_stats(self.handle, buf, last), 'trmf_session_stats')
        return [buf[i].as_dict() for i in range(cnt)]

    def objective(self):
        return self.lib.trmf_session_objective(self.handle)

    def fsolve_bytes(self):
        return self.lib.trmf_session_fsolve_bytes(self.handle)

    def describe(self):
        """One line: which phases are sharded, the form of the X-solve the measure-once rule chose (with the measured
        X-phase time of every candidate) and whether the peer-to-peer transport is available."""
        buf = ctypes.create_string_buffer(1024)
        self._check(self.lib.trmf_session_describe(self.handle, buf, len(buf)), 'trmf_session_describe')
        return buf.value.decode()

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.trmf_session_destroy(self.handle)
            self.handle = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def partition_by_nnz(ptr, world, dtype=np.float32):
    """Row partition used by the sharded solver (host logic of the library, for tests/tools)."""
    ptr = np.ascontiguousarray(ptr, dtype=np.uint64)
    bounds = np.zeros(world + 1, dtype=np.uint64)
    lib = lib_for(dtype)
    rc = lib.trmf_partition_by_nnz(len(ptr) - 1, ptr.ctypes.data_as(POINTER(c_uint64)), world,
                                   bounds.ctypes.data_as(POINTER(c_uint64)))
    if rc != 0:
        raise RuntimeError(lib.trmf_last_error().decode())
    return bounds
