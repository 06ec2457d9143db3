"""NumPy restatements shared by the forecast tests (test infrastructure)."""
import numpy as np


def series_sums(truth, pred, prev=None):
    """The table one scored call adds (n x 6, TrmfSeriesSums order), formed in fp64; ``prev`` is the truth row before the block."""
    y = np.asarray(truth).astype(np.float64)
    e = np.asarray(pred).astype(np.float64) - y
    steps = np.diff(y, axis=0) if prev is None else np.diff(np.vstack([np.asarray(prev).astype(np.float64)[None], y]), axis=0)
    nz = y != 0
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(nz, np.abs(e) / np.abs(y), 0.0)
    return np.stack([np.abs(e).sum(0), (e * e).sum(0), np.abs(y).sum(0), np.abs(steps).sum(0), rel.sum(0), nz.sum(0).astype(np.float64)], axis=1)


def fields(metrics):
    return np.array([getattr(metrics, f) for f in metrics._fields])
