// churn_kernels.hpp -- series churn of an HBM-resident problem (trmf_session_change_series): series (columns of Y, rows of H) are
// retired and a block of new ones is added without the data crossing PCIe again.  slide_kernels.hpp moves the window along the
// time axis; this is the other axis.  The kept series keep their relative order and are renumbered densely from 0 (remap[old] = new,
// or kChurnGone), the block's series follow them.  The stored order of every row and column survives -- it is the summation order
// of the F-solve and of the X-side Gram -- so each compaction is stable.
//
//   csr_churn_count_kernel    one wavefront per row, 64 entries per step: the entries whose series is kept, counted with a ballot
//                             and a population count.  The host turns the counts into the new row pointers.
//   csr_churn_kernel          one wavefront per row: the STABLE compaction of (remap[series], value) -- ballot, then each surviving
//                             lane's rank among the survivors below it -- followed by the block's entries of that row at
//                             series + n_kept.  remap == nullptr: every series is kept (a plain copy in front of the block's
//                             entries).  An optional second index array travels with the entries: the held-out set (COO in CSR
//                             order, cut into pseudo-rows of kSlideChunk entries) is compacted by the same kernel.
//   csc_gather_kernel         one wavefront per KEPT column copies the column, coalesced, to its new place (the block's columns
//                             arrive behind them by plain copies).
//   dense_churn_kernel        T x n0 -> T x n1 row-major: a workgroup owns 256 consecutive columns of the result and a band of rows;
//                             each thread reads its source column's index ONCE, then walks the band (reads of a row are contiguous
//                             within runs of kept columns, stores are contiguous).  Columns >= n_kept come from the block (T x m).
//   row_gather_kernel         dst row q = src row list[q], one wavefront per row: the n x KP table of H, n-vectors (row length 1),
//                             the packed S_j / r_j tables, the n x T orientation of a dense Y.
//
// Streaming kernels: no LDS, no atomics, four wavefronts per 256-thread workgroup (csc_slide_kernel's shape).
#pragma once

#include "common.hpp"

namespace trmf {

constexpr uint32_t kChurnGone = 0xffffffffu;    // remap[series] of a retired series
constexpr int kChurnBand = 64;                  // rows of one dense_churn_kernel workgroup

struct ChurnArgs {
    const uint32_t *optr, *oidx;       // the rows before the call: row i at [optr[i], optr[i + 1]), oidx = the series
    const real *oval;
    const uint32_t *oaux;              // nullptr, or a second index per entry that moves with it (held-out set: the timestamp)
    const uint32_t *remap;             // per old series: its new number or kChurnGone; nullptr: every series keeps its number
    const uint32_t *wptr, *widx;       // the block's rows (series numbered within the block), or nullptr
    const real *wval;
    const uint32_t *nptr;              // the rows after the call (csr_churn_kernel)
    uint32_t *nidx;
    real *nval;
    uint32_t *naux;
    uint32_t *kept;                    // per row: entries of kept series (csr_churn_count_kernel)
    int nrows;
    uint32_t shift;                    // the block's first series after the call (the number of kept series)
};

struct CscGatherArgs {
    const uint32_t *optr, *oidx;       // the columns before the call
    const real *oval;
    const uint32_t *list;              // nkept old column numbers, ascending
    const uint32_t *nptr;              // the columns after the call (the first nkept of them)
    uint32_t *nidx;
    real *nval;
    int nkept;
};

struct DenseChurnArgs {
    const real *src;                   // rows x n0 row-major
    const uint32_t *list;              // nkept old column numbers
    const real *blk;                   // rows x m row-major, or nullptr (m == 0)
    real *dst;                         // rows x (nkept + m) row-major
    int rows, n0, nkept, m;
};

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
__global__ void csr_churn_count_kernel(ChurnArgs a);
__global__ void csr_churn_kernel(ChurnArgs a);
__global__ void csc_gather_kernel(CscGatherArgs a);
__global__ void dense_churn_kernel(DenseChurnArgs a);
__global__ void row_gather_kernel(const real *src, const uint32_t *list, int nrows, size_t rowlen, real *dst);
#else
__global__ __launch_bounds__(256) void csr_churn_count_kernel(ChurnArgs a) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= a.nrows) return;                               // wave-uniform
    const uint32_t o0 = a.optr[i], on = a.optr[i + 1] - o0;
    uint32_t cnt = 0;
    for (uint32_t base = 0; base < on; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        const bool keep = e < on && a.remap[a.oidx[o0 + e]] != kChurnGone;
        cnt += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane == 0) a.kept[i] = cnt;
}

__global__ __launch_bounds__(256) void csr_churn_kernel(ChurnArgs a) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= a.nrows) return;                               // wave-uniform
    const uint32_t o0 = a.optr[i], on = a.optr[i + 1] - o0, d0 = a.nptr[i];
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t out = 0;                                       // survivors written so far (the same in every lane)
    for (uint32_t base = 0; base < on; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        const bool valid = e < on;
        const uint32_t j = valid ? a.oidx[o0 + e] : 0u;
        const real y = valid ? a.oval[o0 + e] : real(0);
        const uint32_t x = (valid && a.oaux) ? a.oaux[o0 + e] : 0u;
        const uint32_t jn = !valid ? kChurnGone : a.remap ? a.remap[j] : j;
        const bool keep = jn != kChurnGone;
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const uint32_t d = d0 + out + (uint32_t)__popcll(mask & below);
            a.nidx[d] = jn;
            a.nval[d] = y;
            if (a.naux) a.naux[d] = x;
        }
        out += (uint32_t)__popcll(mask);
    }
    if (a.wptr) {
        const uint32_t w0 = a.wptr[i], wn = a.wptr[i + 1] - w0;
        for (uint32_t e = lane; e < wn; e += 64u) { a.nidx[d0 + out + e] = a.widx[w0 + e] + a.shift; a.nval[d0 + out + e] = a.wval[w0 + e]; }
    }
}

__global__ __launch_bounds__(256) void csc_gather_kernel(CscGatherArgs a) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= a.nkept) return;                               // wave-uniform
    const uint32_t j = a.list[q];
    const uint32_t o0 = a.optr[j], on = a.optr[j + 1] - o0, d0 = a.nptr[q];
    for (uint32_t e = lane; e < on; e += 64u) { a.nidx[d0 + e] = a.oidx[o0 + e]; a.nval[d0 + e] = a.oval[o0 + e]; }
}

__global__ __launch_bounds__(256) void dense_churn_kernel(DenseChurnArgs a) {
    const int q = blockIdx.x * 256 + threadIdx.x, n1 = a.nkept + a.m;
    if (q >= n1) return;
    const int r0 = blockIdx.y * kChurnBand, r1 = min(r0 + kChurnBand, a.rows);
    const bool old = q < a.nkept;
    const real *col = old ? a.src + a.list[q] : a.blk + (q - a.nkept);
    const size_t pitch = old ? (size_t)a.n0 : (size_t)a.m;
    for (int t = r0; t < r1; t++) a.dst[(size_t)t * n1 + q] = col[(size_t)t * pitch];
}

__global__ __launch_bounds__(256) void row_gather_kernel(const real *__restrict__ src, const uint32_t *__restrict__ list, int nrows, size_t rowlen,
                                                         real *__restrict__ dst) {
    const int lane = threadIdx.x & 63;
    for (int q = blockIdx.x * 4 + (threadIdx.x >> 6); q < nrows; q += gridDim.x * 4) {      // wave-uniform
        const real *s = src + (size_t)list[q] * rowlen;
        real *d = dst + (size_t)q * rowlen;
        for (size_t e = lane; e < rowlen; e += 64u) d[e] = s[e];
    }
}
#endif

}  // namespace trmf
