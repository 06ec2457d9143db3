"""Sparse input as a caller may hold it (test infrastructure): two independent sets of compressed arrays, not a canonical CSR/CSC pair.

The C ABI takes Y as CSR (row_ptr, col_idx, val_t) and CSC (col_ptr, row_idx, val) and uploads both as they are (DESIGN.md
section 4.10).  `RawSparse` builds such a pair from an ENTRY LIST: a cell may be stored several times (each copy is an observation
of its own, as the reference's coo path keeps them, rf_util.py:98-118), a stored value may be exactly 0 (an observation of 0), and
the order of the entries inside a row and inside a column is a seeded random permutation, drawn independently for the two
orientations -- so the CSC is not the transpose order of the CSR and neither has ascending indices.

Also here: the standard "dirty" pattern of the non-canonical tests, and an fp64 NumPy model of one F-solve from the entry list.
Every index a `RawSparse` holds is in range and its pointers are consistent; the constructor asserts it.
"""
import numpy as np
import scipy.sparse as smat

from trmf.rf_util import PyMatrix

ARRAYS = ('row_ptr', 'col_idx', 'val_t', 'col_ptr', 'row_idx', 'val')


def _compress(major, minor, vals, n_major, rng):
    """Compressed arrays of one orientation; the order inside a major index is a random permutation."""
    order = np.lexsort((rng.rand(len(major)), major))
    ptr = np.zeros(n_major + 1, dtype=np.uint64)
    np.cumsum(np.bincount(major, minlength=n_major), out=ptr[1:])
    return ptr, minor[order].astype(np.uint32), vals[order], order


class RawSparse(object):
    """T x n sparse matrix as the six arrays of the C ABI, built from the entry list (rows[e], cols[e], vals[e])."""

    def __init__(self, rows, cols, vals, shape, dtype, seed=0):
        rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64)
        self.shape = (int(shape[0]), int(shape[1]))
        self.dtype = np.dtype(dtype)
        assert rows.ndim == 1 and rows.shape == cols.shape == np.shape(vals)
        assert rows.size == 0 or (rows.min() >= 0 and rows.max() < self.shape[0] and cols.min() >= 0 and cols.max() < self.shape[1])
        self.rows, self.cols = rows, cols
        self.vals = np.asarray(vals).astype(self.dtype)
        self.nnz = int(rows.size)
        rng = np.random.RandomState(seed)
        self.row_ptr, self.col_idx, self.val_t, self.csr_order = _compress(rows, cols, self.vals, self.shape[0], rng)
        self.col_ptr, self.row_idx, self.val, self.csc_order = _compress(cols, rows, self.vals, self.shape[1], rng)
        self._check()

    def _check(self):
        T, n = self.shape
        for ptr, idx, val, nmaj, nmin in ((self.row_ptr, self.col_idx, self.val_t, T, n), (self.col_ptr, self.row_idx, self.val, n, T)):
            assert ptr.dtype == np.uint64 and idx.dtype == np.uint32 and val.dtype == self.dtype
            assert ptr.shape == (nmaj + 1,) and ptr[0] == 0 and int(ptr[-1]) == self.nnz and np.all(ptr[1:] >= ptr[:-1])
            assert idx.shape == val.shape == (self.nnz,) and (self.nnz == 0 or int(idx.max()) < nmin)

    @classmethod
    def from_arrays(cls, shape, dtype, row_ptr, col_idx, val_t, col_ptr, row_idx, val):
        """Over the six arrays themselves (checked like any other); the entry list is read off the CSR."""
        out = object.__new__(cls)
        out.shape, out.dtype = (int(shape[0]), int(shape[1])), np.dtype(dtype)
        out.row_ptr, out.col_idx, out.val_t = np.asarray(row_ptr, np.uint64), np.asarray(col_idx, np.uint32), np.asarray(val_t, out.dtype)
        out.col_ptr, out.row_idx, out.val = np.asarray(col_ptr, np.uint64), np.asarray(row_idx, np.uint32), np.asarray(val, out.dtype)
        out.nnz = int(out.row_ptr[-1])
        out.rows = np.repeat(np.arange(out.shape[0], dtype=np.int64), np.diff(out.row_ptr.astype(np.int64)))
        out.cols, out.vals = out.col_idx.astype(np.int64), out.val_t
        out.csr_order = out.csc_order = None
        out._check()
        a = np.lexsort((out.val_t, out.cols, out.rows))
        cc = np.repeat(np.arange(out.shape[1], dtype=np.int64), np.diff(out.col_ptr.astype(np.int64)))
        b = np.lexsort((out.val, cc, out.row_idx))
        assert np.array_equal(out.rows[a], out.row_idx[b]) and np.array_equal(out.cols[a], cc[b]) and np.array_equal(out.val_t[a], out.val[b])
        return out

    def astype(self, dtype):
        """The same arrays in the same order in another element type."""
        out = object.__new__(RawSparse)
        out.__dict__.update(self.__dict__)
        out.dtype = np.dtype(dtype)
        out.vals, out.val_t, out.val = self.vals.astype(dtype), self.val_t.astype(dtype), self.val.astype(dtype)
        out._check()
        return out

    def reordered(self, seed):
        """The same entry multiset in another order, in both orientations."""
        return RawSparse(self.rows, self.cols, self.vals, self.shape, self.dtype, seed=seed)

    def pymatrix(self):
        """A trmf.rf_util.PyMatrix over these arrays (they are kept alive in its py_buf)."""
        m = PyMatrix(None)
        m.rows, m.cols, m.nnz = self.shape[0], self.shape[1], self.nnz
        m.dtype = self.dtype.type
        m.type = PyMatrix.SPARSE
        m.py_buf = {name: getattr(self, name) for name in ARRAYS}
        ctype_of = dict(PyMatrix._fields_)
        for name, arr in m.py_buf.items():
            setattr(m, name, arr.ctypes.data_as(ctype_of[name]))
        return m

    def coo(self):
        """scipy coo_matrix of the entry list (duplicates and stored zeros kept, as scipy's coo format does)."""
        return smat.coo_matrix((self.vals, (self.rows, self.cols)), shape=self.shape)

    def canonical(self):
        """What a canonicalising caller would train on instead: duplicates summed, stored zeros dropped (csr_matrix)."""
        Y = self.coo().tocsr()
        Y.eliminate_zeros(); Y.sort_indices()
        return Y

    def select(self, keep, seed=0):
        """The entries where `keep` holds, as a new RawSparse (new random orders from `seed`)."""
        keep = np.asarray(keep)
        return RawSparse(self.rows[keep], self.cols[keep], self.vals[keep], self.shape, self.dtype, seed=seed)


def dirty_entries(mask, values, seed=0, long_col=True, long_row=True):
    """The standard dirty entry list from a T x n observation mask and values:
      * one timestamp row and one item column are emptied;
      * about 15 % of the observed cells are stored a second time with a different value;
      * about 10 % of the stored values are exactly 0;
      * one item column holds more entries than T and one timestamp row more than n (random repeats of in-range cells).
    Returns dict(rows, cols, vals (float64), empty_row, empty_col, long_col, long_row)."""
    rng = np.random.RandomState(seed)
    T, n = mask.shape
    mask = mask.copy()
    er, ec = int(rng.randint(T)), int(rng.randint(n))
    mask[er, :] = False; mask[:, ec] = False
    r, c = np.nonzero(mask)
    v = np.asarray(values, dtype=np.float64)[r, c]
    scale = max(float(np.abs(v).std()), 1e-3)
    dup = np.flatnonzero(rng.rand(r.size) < 0.15)
    rows, cols, vals = [r, r[dup]], [c, c[dup]], [v, v[dup] + scale * rng.uniform(0.5, 1.5, dup.size) * rng.choice([-1.0, 1.0], dup.size)]
    lc = lr = None
    if long_col:
        lc = int((ec + 1 + rng.randint(n - 1)) % n)
        tt = rng.choice(np.setdiff1d(np.arange(T), [er]), size=T + 9)
        rows.append(tt); cols.append(np.full(tt.size, lc)); vals.append(scale * rng.randn(tt.size))
    if long_row:
        lr = int((er + 1 + rng.randint(T - 1)) % T)
        jj = rng.choice(np.setdiff1d(np.arange(n), [ec]), size=n + 9)
        rows.append(np.full(jj.size, lr)); cols.append(jj); vals.append(scale * rng.randn(jj.size))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    vals[rng.rand(vals.size) < 0.10] = 0.0
    assert rows.min() >= 0 and rows.max() < T and cols.min() >= 0 and cols.max() < n
    if long_col: assert np.count_nonzero(cols == lc) > T
    if long_row: assert np.count_nonzero(rows == lr) > n
    assert not np.any(rows == er) and not np.any(cols == ec)
    return dict(rows=rows, cols=cols, vals=vals, empty_row=er, empty_col=ec, long_col=lc, long_row=lr)


def dirty_problem(T, n, density, dtype, seed=0, **kw):
    """A low-rank + AR panel (trmf.synth) observed on the dirty pattern: (RawSparse, the dict of dirty_entries)."""
    from trmf import synth
    rng = np.random.RandomState(seed)
    X, F, _ = synth._latent_factors(rng, n, T, 4, [1, 2, 3], 0.01)
    values = X @ F.T + 0.05 * rng.randn(T, n)
    d = dirty_entries(rng.rand(T, n) < density, values, seed=seed + 1, **kw)
    return RawSparse(d['rows'], d['cols'], d['vals'], (T, n), dtype, seed=seed + 2), d


def start_factors(T, n, k, nlag, dtype, seed=0):
    """Random initial (W, H, Theta) as Model.initialize draws them: rand W and H (row-major), randn Theta (column-major)."""
    rng = np.random.RandomState(seed)
    return (np.ascontiguousarray(rng.rand(T, k).astype(dtype)), np.ascontiguousarray(rng.rand(n, k).astype(dtype)),
            np.asfortranarray(rng.randn(nlag, k).astype(dtype)))


def doubled(raw, seed=0):
    """Every entry stored twice."""
    return RawSparse(np.tile(raw.rows, 2), np.tile(raw.cols, 2), np.tile(raw.vals, 2), raw.shape, raw.dtype, seed=seed)


def stacked(head, tail):
    """The arrays a session holds after append_rows(tail) on a session created over `head` (csrc/session_online.hpp append_rows): the
    CSR is the old rows followed by the new ones; every column of the CSC is its old entries followed by the block's entries of
    that column with their timestamps shifted."""
    T0, n = head.shape
    assert tail.shape[1] == n and tail.dtype == head.dtype
    row_ptr = np.concatenate([head.row_ptr, head.row_ptr[-1] + tail.row_ptr[1:]])
    col_idx, val_t = np.concatenate([head.col_idx, tail.col_idx]), np.concatenate([head.val_t, tail.val_t])
    col_ptr = head.col_ptr + tail.col_ptr
    row_idx, val = np.empty(head.nnz + tail.nnz, np.uint32), np.empty(head.nnz + tail.nnz, head.dtype)
    for j in range(n):
        h0, h1, t0, t1, d0 = (int(x) for x in (head.col_ptr[j], head.col_ptr[j + 1], tail.col_ptr[j], tail.col_ptr[j + 1], col_ptr[j]))
        row_idx[d0:d0 + h1 - h0] = head.row_idx[h0:h1]; val[d0:d0 + h1 - h0] = head.val[h0:h1]
        row_idx[d0 + h1 - h0:d0 + h1 - h0 + t1 - t0] = tail.row_idx[t0:t1] + T0; val[d0 + h1 - h0:d0 + h1 - h0 + t1 - t0] = tail.val[t0:t1]
    return RawSparse.from_arrays((T0 + tail.shape[0], n), head.dtype, row_ptr, col_idx, val_t, col_ptr, row_idx, val)


def entry_fsolve(major, minor, vals, X, F0, lam):
    """fp64 model of one F-solve from the entry list: for every index i of `major` that holds entries,
    (sum_e x_e x_e^T + lam I) f_i = sum_e y_e x_e with x_e = X[minor[e]]; rows without entries keep F0 (trmf.cpp:374)."""
    X = np.asarray(X, dtype=np.float64)
    F = np.array(F0, dtype=np.float64)
    vals = np.asarray(vals, dtype=np.float64)
    k = X.shape[1]
    order = np.argsort(major, kind='stable')
    bounds = np.searchsorted(major[order], np.arange(F.shape[0] + 1))
    for i in range(F.shape[0]):
        e = order[bounds[i]:bounds[i + 1]]
        if e.size == 0:
            continue
        Xe = X[minor[e]]
        F[i] = np.linalg.solve(Xe.T @ Xe + lam * np.eye(k), Xe.T @ vals[e])
    return F


def entry_objective(raw, lag_set, W, H, theta, hyper):
    """fp64 NumPy objective over the entry list (the sum the restatement's oracle_objective_sparse forms over the CSR)."""
    W, H, th = (np.asarray(a, dtype=np.float64) for a in (W, H, theta))
    d = raw.vals.astype(np.float64) - np.einsum('ij,ij->i', W[raw.rows], H[raw.cols])
    lags = np.asarray(lag_set, dtype=np.int64)
    ar = 0.0
    if lags.size:
        midx = int(lags[-1])
        res = W[midx:].copy()
        for l, lag in enumerate(lags):
            res -= th[l] * W[midx - lag:W.shape[0] - lag]
        ar = float((res * res).sum())
    return 0.5 * float(d @ d) + 0.5 * hyper['lambdaI'] * float((W * W).sum() + (H * H).sum()) + 0.5 * hyper['lambdaAR'] * ar
