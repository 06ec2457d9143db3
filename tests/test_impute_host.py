"""CPU: the host side of imputation -- ImputeMetrics from the device's six sums, the mask-built training matrix, the three new
C entry points and the layout of TrmfHeldoutSums.  No compute is launched here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, 'include')


def _sums(y, p):
    d = p - y
    nz = y != 0
    return dict(count=y.size, count_nonzero=int(nz.sum()), sq_err=float(np.sum(d * d)), abs_err=float(np.sum(np.abs(d))),
                abs_truth=float(np.sum(np.abs(y))), rel_err=float(np.sum(np.abs(d[nz]) / np.abs(y[nz]))))


def test_impute_metrics_from_sums_match_numpy():
    from trmf import ImputeMetrics
    rng = np.random.RandomState(3)
    y = rng.randn(5000)
    y[rng.rand(y.size) < 0.1] = 0.0                         # zero truths: left out of MAPE only
    p = y + 0.3 * rng.randn(y.size)
    m = ImputeMetrics.from_sums(_sums(y, p))
    d = p - y
    mse = np.mean(d ** 2)
    assert m.count == y.size
    assert np.isclose(m.mse, mse, rtol=1e-13)
    assert np.isclose(m.nrmse, np.sqrt(mse) / np.mean(np.abs(y)), rtol=1e-13)
    assert np.isclose(m.nd, np.sum(np.abs(d)) / np.sum(np.abs(y)), rtol=1e-13)
    nz = y != 0
    assert np.isclose(m.mape, np.mean(np.abs(d[nz]) / np.abs(y[nz])), rtol=1e-13)
    assert ImputeMetrics.generate(y, p) == m
    assert m._fields == ('nd', 'nrmse', 'mse', 'mape', 'count')


def test_impute_metrics_without_nonzero_truth():
    from trmf import ImputeMetrics
    m = ImputeMetrics.from_sums(dict(count=3, count_nonzero=0, sq_err=3.0, abs_err=3.0, abs_truth=0.0, rel_err=0.0))
    assert np.isnan(m.mape) and np.isinf(m.nd) and m.mse == 1.0


def test_training_matrix_from_mask_keeps_observed_zeros():
    from trmf.impute import training_matrix
    from trmf.rf_util import PyMatrix
    rng = np.random.RandomState(0)
    Y = rng.randn(50, 20)
    mask = rng.rand(50, 20) < 0.7
    Y[mask & (rng.rand(50, 20) < 0.2)] = 0.0                # observed true zeros
    Y[~mask] = np.nan                                       # whatever the unobserved cells hold is never read
    A = training_matrix(Y, mask, np.float32)
    assert A.nnz == int(mask.sum())
    assert np.array_equal(np.sort(A.row * 20 + A.col), np.flatnonzero(mask))
    assert np.array_equal(A.data, Y[A.row, A.col].astype(np.float32))
    assert (A.data == 0).sum() == int((mask & (Y == 0)).sum()) > 0
    py = PyMatrix(A, dtype=np.float32)                      # what the library receives: every observed cell, zeros included
    assert py.nnz == int(mask.sum())


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_libraries_export_heldout_entry_points(dtype):
    from trmf import session
    lib = session.lib_for(dtype)
    for name in ('trmf_session_set_heldout', 'trmf_session_eval_heldout', 'trmf_session_set_lambdas'):
        assert hasattr(lib, name), name


def test_heldout_sums_layout_matches_header(tmp_path):
    from trmf.session import TrmfHeldoutSums
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trmf_abi.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(TrmfHeldoutSums),\n'
                   ' offsetof(TrmfHeldoutSums, count), offsetof(TrmfHeldoutSums, count_nonzero), offsetof(TrmfHeldoutSums, sq_err),\n'
                   ' offsetof(TrmfHeldoutSums, abs_err), offsetof(TrmfHeldoutSums, abs_truth), offsetof(TrmfHeldoutSums, rel_err));\n'
                   ' return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run(['cc', '-I', HEADER_DIR, str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(TrmfHeldoutSums)] + [getattr(TrmfHeldoutSums, name).offset for name, _ in TrmfHeldoutSums._fields_]
    assert got == want
