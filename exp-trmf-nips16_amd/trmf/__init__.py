"""MI355X-native TRMF (temporal regularized matrix factorization) -- Python front end.

Importable exactly like the reference package (python/trmf/__init__.py:1-6):
``from trmf import Model, Metrics, train, rolling_validate, grid_search``; imputation (the paper's second task) adds
``impute``, ``grid_impute`` and ``ImputeMetrics``; online updates add ``filter_rows``, ``robust_filter_rows`` (and ``Model.assimilate``, ``Session.update``);
online loading updates add ``series_ridge``, ``SeriesStats`` (and ``Session.adapt_series``, ``Session.update(adapt=True)``);
the fixed-interval smoother adds ``smooth_rows``, ``window_objective`` (and ``Session.smooth``, ``Session.update(smooth_back=)``);
the robust smoother adds ``robust_smooth_rows``, ``robust_window_objective`` (and ``Session.smooth_robust``, ``smooth_robust=True``);
robust online loading updates add ``robust_series_objective`` (and ``SeriesStats.absorb_robust``, ``Session.adapt_series_robust``, ``adapt_robust=True``);
the sliding window adds ``slide_entries`` (and ``SeriesStats.retire``, ``Session.slide``, ``Session.retire_rows``, ``Session.update(window=)``);
series churn adds ``churn_entries`` (and ``Session.change_series``, ``Session.add_series``, ``Session.retire_series``, ``Model.add_series``, ``Model.retire_series``);
cell revisions add ``revise_entries`` (and ``SeriesStats.revise``, ``Session.revise``, ``Session.retract``, ``Session.update(revisions=)``, ``Model.revise``);
forecast uncertainty adds ``fit_noise``, ``impulse_response``, ``forecast_std`` and ``IntervalMetrics`` (and ``Model.fit_noise``,
``Model.forecast_std``, ``Session.forecast_dist``).
"""
from .trmf import Model, Metrics
from .trmf import train, fit, rolling_validate, grid_search
from .impute import ImputeMetrics, impute, grid_impute
from .online import (filter_rows, robust_filter_rows, series_ridge, SeriesStats, smooth_rows, window_objective, robust_smooth_rows,
                     robust_window_objective, robust_series_objective, slide_entries, churn_entries, revise_entries)
from .uncertainty import IntervalMetrics, fit_noise, forecast_std, impulse_response

__all__ = ['Model', 'Metrics', 'train', 'fit', 'rolling_validate', 'grid_search', 'ImputeMetrics', 'impute', 'grid_impute', 'filter_rows', 'robust_filter_rows', 'series_ridge', 'SeriesStats', 'smooth_rows', 'window_objective', 'robust_smooth_rows', 'robust_window_objective', 'robust_series_objective', 'slide_entries', 'churn_entries', 'revise_entries',
           'fit_noise', 'impulse_response', 'forecast_std', 'IntervalMetrics']
