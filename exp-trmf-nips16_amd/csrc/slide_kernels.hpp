// slide_kernels.hpp -- a sliding window over an HBM-resident problem (trmf_session_slide): the oldest timestamps of a session are
// retired -- and, in the same pass, a block of new ones appended -- without the data crossing PCIe again.  The CSR side of a sparse
// Y, a dense Y and W are suffix copies (device-to-device); what needs kernels is the CSC side, whose columns each lose entries
// ANYWHERE in their stored order (the input need not be canonical: a column's timestamps may be unsorted and a cell may be stored
// twice), and the loading statistics of adapt_kernels.hpp, which lose the retired entries' rank-1 terms.
//
//   csc_slide_count_kernel    one wavefront per column, 64 entries per step: the entries with timestamp >= retire, counted with a
//                             ballot and a population count.  The host turns the n counts into the new column pointers.
//   csc_slide_kernel          one wavefront per column: the STABLE compaction of (timestamp - retire, value) into the new column --
//                             ballot, then each surviving lane's rank among the survivors below it -- followed by the block's entries
//                             of that column at their new timestamps (csc_append_kernel's second half).  Loads are coalesced within
//                             a column; no atomics, no LDS.  An optional second index array travels with the entries: the held-out
//                             set (COO in CSR order) is compacted by the same kernel, cut into pseudo-columns of kSlideChunk entries.
//   series_downdate_kernel<NT>  sparse storage with missing != 0: one wavefront per series subtracts om_t w_t w_t^T from S_j and
//                             om_t y w_t from r_j for every retired entry among the column's absorbed ones, in stored order -- the
//                             rank-1 update of adapt_series_kernel with the sign of the weight flipped (adapt_rank1, shared).  Reads
//                             the storage and the W of BEFORE the slide and the active generation of the tables, writes the other.
//
// Every sum runs in stored order in the element type; no floating-point atomics.
#pragma once

#include "adapt_kernels.hpp"

namespace trmf {

constexpr uint32_t kSlideChunk = 4096;      // entries per pseudo-column when a COO list (the held-out set) is compacted

struct SlideArgs {
    const uint32_t *optr, *oidx;       // the columns before the slide: column j at [optr[j], optr[j + 1]), oidx = the timestamp
    const real *oval;
    const uint32_t *oaux;              // nullptr, or a second index per entry that moves with it (held-out set: the series)
    const uint32_t *wptr, *widx;       // the appended block's columns (timestamps relative to the block), or nullptr
    const real *wval;
    const uint32_t *nptr;              // the columns after the slide (csc_slide_kernel)
    uint32_t *nidx;
    real *nval;
    uint32_t *naux;
    uint32_t *kept;                    // per column: entries with timestamp >= retire (csc_slide_count_kernel)
    int ncols;
    uint32_t retire, shift;            // shift: the block's first timestamp after the slide (rows before - retire)
};

struct DowndateArgs {
    const uint32_t *ptr, *idx;         // CSC before the slide
    const real *val;
    const uint32_t *absorbed;          // per series: how many of the column's first entries the tables hold
    const real *W;                     // before the slide, rows x KP, column-interleaved
    const real *omega;                 // MINUS the weight of timestamp t at omega[t], t < retire; nullptr: -1 (gamma == 1)
    const real *Sin, *rin;             // the active generation
    real *Sout, *rout;                 // the inactive generation
    uint32_t retire;
    int n, k, KP;
};

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
__global__ void csc_slide_count_kernel(SlideArgs a);
__global__ void csc_slide_kernel(SlideArgs a);
template <int NT>
__global__ void series_downdate_kernel(DowndateArgs a);
#else
__global__ __launch_bounds__(256) void csc_slide_count_kernel(SlideArgs a) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= a.ncols) return;                               // wave-uniform
    const uint32_t o0 = a.optr[j], on = a.optr[j + 1] - o0;
    uint32_t cnt = 0;
    for (uint32_t base = 0; base < on; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        const bool keep = e < on && a.oidx[o0 + e] >= a.retire;
        cnt += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane == 0) a.kept[j] = cnt;
}

__global__ __launch_bounds__(256) void csc_slide_kernel(SlideArgs a) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= a.ncols) return;                               // wave-uniform
    const uint32_t o0 = a.optr[j], on = a.optr[j + 1] - o0, d0 = a.nptr[j];
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t out = 0;                                       // survivors written so far (the same in every lane)
    for (uint32_t base = 0; base < on; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        const bool valid = e < on;
        const uint32_t t = valid ? a.oidx[o0 + e] : 0u;
        const real y = valid ? a.oval[o0 + e] : real(0);
        const uint32_t x = (valid && a.oaux) ? a.oaux[o0 + e] : 0u;
        const bool keep = valid && t >= a.retire;
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const uint32_t d = d0 + out + (uint32_t)__popcll(mask & below);
            a.nidx[d] = t - a.retire;
            a.nval[d] = y;
            if (a.naux) a.naux[d] = x;
        }
        out += (uint32_t)__popcll(mask);
    }
    if (a.wptr) {
        const uint32_t w0 = a.wptr[j], wn = a.wptr[j + 1] - w0;
        for (uint32_t e = lane; e < wn; e += 64u) { a.nidx[d0 + out + e] = a.widx[w0 + e] + a.shift; a.nval[d0 + out + e] = a.wval[w0 + e]; }
    }
}

template <int NT>
__global__ __launch_bounds__(64) void series_downdate_kernel(DowndateArgs a) {
    constexpr int KMAX = kTile * NT;
    const int c = threadIdx.x, k = a.k;
    const int j = blockIdx.x;
    if (j >= a.n) return;
    const bool on = c < k;
    const int cp = colpos(on ? c : k - 1, NT);
    const size_t PK = adapt_packed(k);
    real col[KMAX], rr = 0;
    const real *Sj = a.Sin + (size_t)j * PK;
#pragma unroll
    for (int s = 0; s < KMAX; s++) col[s] = (on && s <= c) ? Sj[s * k - s * (s - 1) / 2 + c - s] : real(0);
    if (on) rr = a.rin[(size_t)j * k + c];
    const uint32_t e0 = a.ptr[j], e1 = e0 + a.absorbed[j];
    for (uint32_t base = e0; base < e1; base += 64u) {
        const uint32_t e = base + (uint32_t)c;
        const bool valid = e < e1;
        const uint32_t t = valid ? a.idx[e] : a.retire;
        const bool gone = t < a.retire;
        const real y = gone ? a.val[e] : real(0);
        const real om = gone ? (a.omega ? a.omega[t] : real(-1)) : real(0);
        unsigned long long mask = __ballot(gone);           // wave-uniform: the retired entries of this batch, in stored order
        while (mask) {
            const int l = (int)__builtin_ctzll(mask);
            mask &= mask - 1ull;
            const int tq = adapt_bcast((int)t, l);
            const real wq = a.W[(size_t)tq * a.KP + cp];
            adapt_rank1<KMAX>(col, rr, on ? wq : real(0), adapt_bcast(om, l), adapt_bcast(y, l));
        }
    }
    if (on) {
        real *So = a.Sout + (size_t)j * PK;
#pragma unroll
        for (int s = 0; s < KMAX; s++)
            if (s <= c) So[s * k - s * (s - 1) / 2 + c - s] = col[s];
        a.rout[(size_t)j * k + c] = rr;
    }
}
#endif

}  // namespace trmf
