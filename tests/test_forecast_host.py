"""CPU: the host side of on-device forecasting -- Metrics from the device's per-series sums, the three new C entry points, the
layout of TrmfSeriesSums and the refusals of rolling_validate(forecast_on_device=True).  No compute is launched here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as smat

from forecast_helpers import fields as _fields, series_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, 'include')
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'py_harness.npz'))


@pytest.mark.parametrize('pieces', [1, 3])
def test_metrics_from_series_sums_match_generate_and_the_reference_capture(pieces):
    from trmf import Metrics
    pred = GOLD['met_pred']
    for true, want, upto in ((GOLD['met_true'], GOLD['met_values'], 6), (GOLD['met2_true'], GOLD['met2_values'], 7)):
        table, prev, rows = np.zeros((true.shape[1], 6)), None, 0
        for part in np.array_split(np.arange(true.shape[0]), pieces):       # the MASE term is carried over the seams
            table += series_sums(true[part], pred[part], prev)
            prev, rows = true[part[-1]], rows + len(part)
        got = Metrics.from_series_sums(rows, table)
        assert got._fields == Metrics._fields
        assert np.allclose(_fields(got), _fields(Metrics.generate(true, pred)), rtol=1e-12, atol=0)
        assert np.allclose(_fields(got)[:upto], want[:upto], rtol=1e-12, atol=0)


def test_metrics_from_series_sums_skip_series_without_a_finite_ratio():
    from trmf import Metrics
    rng = np.random.RandomState(0)
    true = rng.randn(20, 5)
    true[:, 2] = 0.0                                        # a series of zeros: no scale, left out of the m_ fields and of MAPE
    pred = true + 0.1 * rng.randn(20, 5)
    got = Metrics.from_series_sums(20, series_sums(true, pred))
    assert np.allclose(_fields(got), _fields(Metrics.generate(true, pred)), rtol=1e-12, atol=0)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_libraries_export_forecast_entry_points(dtype):
    from trmf import session
    lib = session.lib_for(dtype)
    for name in ('trmf_session_forecast', 'trmf_session_forecast_scores', 'trmf_session_forecast_reset'):
        assert hasattr(lib, name), name
    assert lib.trmf_session_forecast.restype is ctypes.c_int32 and len(lib.trmf_session_forecast.argtypes) == 7


def test_series_sums_layout_matches_header(tmp_path):
    from trmf.session import TrmfSeriesSums
    names = [name for name, _ in TrmfSeriesSums._fields_]
    assert names == ['abs_err', 'sq_err', 'abs_truth', 'abs_dtruth', 'rel_err', 'count_nonzero']
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trmf_abi.h"\n'
                   'int main(void) { printf("%zu", sizeof(TrmfSeriesSums));\n'
                   + ''.join(' printf(" %%zu", offsetof(TrmfSeriesSums, %s));\n' % name for name in names)
                   + ' printf("\\n"); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.run(['cc', '-I', HEADER_DIR, str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(TrmfSeriesSums)] + [getattr(TrmfSeriesSums, name).offset for name in names]


def test_forecast_on_device_says_where_it_does_not_apply():
    import trmf
    Y = np.abs(np.random.RandomState(0).randn(120, 6)) + 0.5
    kw = dict(k=3, window_size=8, nr_windows=3, max_iter=2)
    with pytest.raises(ValueError, match='sparse'):
        trmf.rolling_validate(smat.csr_matrix(Y), [1, 2, 5], forecast_on_device=True, **kw)
    with pytest.raises(ValueError, match='missing=True'):
        trmf.rolling_validate(Y, [1, 2, 5], forecast_on_device=True, transform=True, missing=True, **kw)
    with pytest.raises(ValueError, match='resident'):
        trmf.rolling_validate(Y, [1, 2, 5], forecast_on_device=True, resident=False, **kw)
    with pytest.raises(ValueError, match='sparse'):
        trmf.grid_search(smat.csr_matrix(Y), [1, 2, 5], {'lambdaI': [0.5]}, forecast_on_device=True, **kw)
