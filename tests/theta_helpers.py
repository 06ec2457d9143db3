"""Model builder of tests/test_gpu_theta_lean.py (test infrastructure)."""
import numpy as np

from trmf import Model
from trmf.rf_util import PyMatrix


class _RowMajor(PyMatrix):
    """A dense PyMatrix over a C-ordered array, tagged row-major whatever its shape.  PyMatrix tests f_contiguous first (the
    reference's quirk Q2, kept and tested in tests/test_abi.py), so a (T, 1) array -- C- and F-contiguous at once, the same bytes
    either way -- comes out column-major and the libraries' dimension check rejects a rank-1 W or H built from it."""

    def __init__(self, A, dtype):
        super().__init__(np.ascontiguousarray(A), dtype)
        self.type = PyMatrix.DENSE_ROWMAJOR


def lag_model(W, n_items, lags):
    """A model over a copy of W (T x k, any k >= 1) with zero H (n_items x k) and zero Theta (|L| x k)."""
    T, k = W.shape
    dtype = W.dtype.type
    return Model(pyW=_RowMajor(W.copy(), dtype), pyH=_RowMajor(np.zeros((n_items, k), dtype=dtype), dtype),
                 pylag_val=PyMatrix(np.asfortranarray(np.zeros((len(lags), k), dtype=dtype)), dtype), lag_set=np.array(lags, dtype=np.uint32))
