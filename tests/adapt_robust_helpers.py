"""Shared by tests/test_adapt_robust_host.py and tests/test_gpu_adapt_robust.py: the cases of the robust online loading update on
adapt_helpers' designed matrix, their fp32 / fp64 NumPy statements (trmf.online.SeriesStats.absorb_robust) and the yardstick the
device is gated by (test infrastructure).

A case is one block of 12 rows absorbed into tables that hold the rows before it.  Its scale is one value for every series: the
pooled RMS, over the block, of the residuals the fp64 PLAIN update (absorb + solve) leaves -- not the residual RMS at the input H:
with that, sweeps 2..4 down-weight nothing for k >= 7 and a case would test only the plain path.  With c = 1.5 and 4 sweeps a good
part of the block's entries then lies beyond the threshold in the last sweep and both branches of the weight are exercised.

The yardstick.  H and the weights are checked teacher-forced: against the fp64 statement on the W the session itself holds and the
H it held before the call.  An fp32 session may be no farther from it than 8x (online_helpers.GATE) the fp32 statement is from the
fp64 statement on the same fp32 values, an fp64 session no farther than that scaled by eps64 / eps32."""
import copy

import numpy as np
import scipy.sparse as smat

import adapt_helpers as AH
import online_helpers as OH
import robust_helpers as RH
from helpers import relmax

C, SWEEPS = RH.C, RH.SWEEPS
BLOCKS = ((OH.FIRST, AH.MID), (AH.MID, OH.T))


def cast(Y, dtype):
    """A CSC copy of Y in `dtype` with the stored entries exactly as they are (online_helpers.rows_of: scipy's own astype may add the
    copies of a cell stored twice)."""
    Yc = Y if Y.format == 'csc' else Y.tocsc()
    return smat.csc_matrix((Yc.data.astype(dtype), Yc.indices.copy(), Yc.indptr.copy()), shape=Yc.shape)


def block_entries(Ynew):
    """(rows, cols, values) of a block's stored entries series-major in stored order: the order of the weights."""
    Yc = Ynew.tocsc() if Ynew.format != 'csc' else Ynew
    cols = np.repeat(np.arange(Yc.shape[1]), np.diff(Yc.indptr))
    return Yc.indices.astype(np.int64), cols, Yc.data


def plain_scale(stats64, W, Ynew, lamI):
    """The pooled RMS over the block of the residuals the fp64 plain update leaves (stats64: fp64 tables of the rows before the block;
    they are not changed)."""
    W64 = np.asarray(W, dtype=np.float64)
    H = copy.deepcopy(stats64).absorb(W64, Ynew).solve(lamI)
    r, c, y = block_entries(Ynew)
    res = y.astype(np.float64) - np.einsum('ed,ed->e', W64[stats64.rows:][r], H[c])
    return float(np.sqrt((res ** 2).mean()))


def margins(stats64, W, Ynew, Hin, lamI, scale, c=C, sweeps=SWEEPS):
    """Per entry of the block, in the order of the weights: | |res| / tau - 1 | in fp64 with res the residual the last sweep's weight
    is formed from (against h^{sweeps-1})."""
    W64 = np.asarray(W, dtype=np.float64)
    Hprev = np.asarray(Hin, dtype=np.float64)
    if sweeps > 1:
        Hprev = copy.deepcopy(stats64).absorb_robust(W64, Ynew, Hprev, lamI, scale, c, sweeps - 1)[0]
    r, cols, y = block_entries(Ynew)
    res = np.abs(y.astype(np.float64) - np.einsum('ed,ed->e', W64[stats64.rows:][r], Hprev[cols]))
    sc = np.full(Ynew.shape[1], float(scale)) if np.ndim(scale) == 0 else np.asarray(scale, dtype=np.float64)
    return np.abs(res / (float(c) * sc[cols]) - 1.0)


class Twin(object):
    """The NumPy statements side by side over one sequence of blocks, their tables built on the rows before the first block:
    `ref`, fp64 on the values handed in as they are (what the device is compared with), and the pair the yardstick is measured
    on, fp32 and fp64 on the same values rounded to fp32 (for fp32 input the fp64 one of the pair is `ref`)."""

    def __init__(self, W, Yhead, gamma):
        from trmf import SeriesStats
        W = np.asarray(W)
        rows = Yhead.shape[0]
        self.exact = W.dtype == np.float32
        W32 = W.astype(np.float32)
        self.ref = SeriesStats(W[:rows].astype(np.float64), cast(Yhead, np.float64), gamma, True)
        self.st32 = SeriesStats(W32[:rows], cast(Yhead, np.float32), gamma, True)
        self.st64 = self.ref if self.exact else SeriesStats(W32[:rows].astype(np.float64), cast(Yhead, np.float64), gamma, True)

    def block(self, W, Ynew, Hin, lamI, scale=None, c=C, sweeps=SWEEPS):
        """Absorb the block (rows ref.rows..len(W)-1 of W with their observations Ynew, a CSC that keeps a doubled cell's copies)
        from the loadings Hin.  Returns a dict: scale; H64, om64, rows, indptr (the reference's loadings and its weights
        series-major as a CSC's arrays); dev_H / dev_weights, the fp32 statement's distances from its fp64 twin (relmax / largest
        absolute difference); border, the mask of the entries within robust_helpers.BORDER of their threshold; before, the
        reference's tables as they were (for trmf.robust_series_objective)."""
        W, Hin = np.asarray(W), np.asarray(Hin)
        W32, H32in = W.astype(np.float32), Hin.astype(np.float32)
        Y64, Y32 = cast(Ynew, np.float64), cast(Ynew, np.float32)
        before = copy.deepcopy(self.ref)
        if scale is None:
            scale = plain_scale(before, W, Y64, lamI)
        border = margins(before, W, Y64, Hin, lamI, scale, c, sweeps) <= RH.BORDER if np.isfinite(c) else np.zeros(Y64.nnz, dtype=bool)
        H64, om64 = self.ref.absorb_robust(W.astype(np.float64), Y64, Hin.astype(np.float64), lamI, scale, c, sweeps)
        if self.exact:
            Hy, omy = H64, om64
        else:
            Hy, omy = self.st64.absorb_robust(W32.astype(np.float64), Y64, H32in.astype(np.float64), lamI, scale, c, sweeps)
        H32, om32 = self.st32.absorb_robust(W32, Y32, H32in, lamI, scale, c, sweeps)
        assert np.array_equal(om64.indices, om32.indices) and np.array_equal(om64.indptr, om32.indptr)
        return dict(scale=scale, H64=H64, om64=om64.data, rows=om64.indices, indptr=om64.indptr, H32=H32, om32=om32.data, dev_H=relmax(H32, Hy),
                    dev_weights=float(np.abs(om32.data.astype(np.float64) - omy.data).max()) if om64.nnz else 0.0, border=border, before=before)


def host_sequence(k, lamI, gamma, c=C, sweeps=SWEEPS):
    """The two blocks of the designed matrix absorbed one after the other on online_helpers.inputs(k)'s own W, from its H: a list of
    Twin.block results (with 'W', 'Ynew', 'Hin' added)."""
    d = OH.inputs(k)
    W = d['W']
    tw = Twin(W, AH.csc_of(k, 0, OH.FIRST, np.float32), gamma)
    H = d['H']
    out = []
    for lo, hi in BLOCKS:
        Ynew = AH.csc_of(k, lo, hi, np.float32)
        y = tw.block(W[:hi], Ynew, H, lamI, None, c, sweeps)
        y.update(W=W[:hi], Ynew=Ynew, Hin=H)
        out.append(y)
        H = y['H64'].astype(np.float32)
    return out


def exercised(y):
    """robust_helpers.exercised on a Twin.block result: (share down-weighted by the fp64 statement, share borderline)."""
    return RH.exercised(dict(om64=y['om64'], border=y['border']))


def bound(dtype, dev32):
    return OH.GATE * dev32 * (1.0 if np.dtype(dtype) == np.float32 else OH.EPS_SCALE)
