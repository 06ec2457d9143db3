// revise_kernels.hpp -- cell revisions of an HBM-resident problem (trmf_session_revise): cells INSIDE the rows and series a session
// holds are set (a late or corrected observation) or deleted (a retracted one) without the data crossing PCIe again.
// slide_kernels.hpp edits the time axis and churn_kernels.hpp the series axis; this is the third structural edit.  Every stored
// copy of an edited cell leaves both orientations -- the input need not be canonical: a row's series may be unsorted and a cell may
// be stored twice -- and each set then places ONE entry at the end of its row and of its column.  The stored order of the other
// entries survives (it is the summation order of the F-solve and of the X-side Gram), so the compaction is stable.
//
// One pair of kernels serves BOTH orientations.  The major index (a row of the CSR side, a column of the CSC side) owns the sorted
// list of the minor indices it loses or gains, [eptr[i], eptr[i + 1]) of (eidx, eval, edel): the host uploads the batch bucketed
// twice, by row with the series ascending and by column with the timestamps ascending.
//
//   revise_count_kernel       one wavefront per major index, 64 entries per step: each lane binary-searches its entry's minor index
//                             in the major's edit list; the survivors are counted with a ballot and a population count, and the
//                             stored copies each edit removes are added to hits[edit] by the lane edit % 64 (a plain read-modify-write:
//                             the wavefront owns the major index and with it the edits, the steps run in program order).  The host
//                             turns the counts into the new pointers and the hits into replaced / inserted / deleted / missed.
//   revise_kernel             one wavefront per major index: the STABLE compaction of the survivors -- ballot, then each surviving
//                             lane's rank among the survivors below it -- followed by the major's sets in list order (its deletes
//                             skipped by the same ballot and rank).  A major index without edits is a plain coalesced copy.
//   dense_revise_kernel       dense storage: the E cells scattered into the T x n copy (the raw copy under a transform) and, where
//                             given, into the n x T copy.  The cells of a batch are distinct, so no two threads write one address.
//   series_revise_kernel<NT>  sparse storage with missing != 0: one wavefront per TOUCHED series subtracts om_t w_t w_t^T / om_t y w_t
//                             of every removed entry of the column in stored order, then adds those of the column's sets in
//                             ascending timestamp (adapt_rank1, shared).  Reads the storage of BEFORE the edit and the active
//                             generation of the tables, writes the other (series_downdate_kernel's scheme); the host copies the
//                             untouched series' tables.
//
// Streaming kernels: no LDS, no atomics, four wavefronts per 256-thread workgroup (csc_slide_kernel's shape).
#pragma once

#include "adapt_kernels.hpp"

namespace trmf {

struct ReviseArgs {
    const uint32_t *optr, *oidx;       // before the call: major index i at [optr[i], optr[i + 1]), oidx = the minor index
    const real *oval;
    const uint32_t *eptr;              // nmajor + 1: the edits of major index i are [eptr[i], eptr[i + 1]), minor indices ascending
    const uint32_t *eidx;
    const real *eval;                  // the value of a set
    const uint8_t *edel;               // non-zero: a delete
    const uint32_t *nptr;              // after the call (revise_kernel)
    uint32_t *nidx;
    real *nval;
    uint32_t *kept;                    // per major index: the surviving entries (revise_count_kernel)
    uint32_t *hits;                    // per edit: stored copies removed (revise_count_kernel; zero on entry), or nullptr
    int nmajor;
};

struct DenseReviseArgs {
    const uint32_t *rows, *cols;       // E distinct cells
    const real *vals;
    real *tn;                          // T x n row-major
    real *nt;                          // n x T row-major, or nullptr
    uint32_t count;
    int T, n;
};

struct SeriesReviseArgs {
    const uint32_t *ptr, *idx;         // CSC before the edit
    const real *val;
    const uint32_t *list;              // ntouched series, ascending
    const uint32_t *eptr, *eidx;       // the batch bucketed by column (n + 1 pointers; timestamps ascending)
    const real *eval;
    const uint8_t *edel;
    const real *W;                     // rows x KP, column-interleaved
    const real *omega;                 // the weight of timestamp t at omega[t]; nullptr: 1 (gamma == 1)
    const real *Sin, *rin;             // the active generation
    real *Sout, *rout;                 // the inactive generation
    int ntouched, k, KP;
};

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
__global__ void revise_count_kernel(ReviseArgs a);
__global__ void revise_kernel(ReviseArgs a);
__global__ void dense_revise_kernel(DenseReviseArgs a);
template <int NT>
__global__ void series_revise_kernel(SeriesReviseArgs a);
#else
// the position of `key` in the ascending list ed[0, ne), or ne when it is not there
__device__ __forceinline__ uint32_t revise_find(const uint32_t *ed, uint32_t ne, uint32_t key) {
    uint32_t lo = 0, hi = ne;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ed[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < ne && ed[lo] == key) ? lo : ne;
}

__global__ __launch_bounds__(256) void revise_count_kernel(ReviseArgs a) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= a.nmajor) return;                              // wave-uniform
    const uint32_t o0 = a.optr[i], on = a.optr[i + 1] - o0;
    const uint32_t e0 = a.eptr[i], ne = a.eptr[i + 1] - e0;
    if (ne == 0) { if (lane == 0) a.kept[i] = on; return; }
    uint32_t cnt = 0;
    for (uint32_t base = 0; base < on; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        const bool valid = e < on;
        const uint32_t q = valid ? revise_find(a.eidx + e0, ne, a.oidx[o0 + e]) : ne;
        const bool hit = q < ne;
        cnt += (uint32_t)__popcll(__ballot(valid && !hit));
        if (a.hits) {
            unsigned long long mask = __ballot(hit);        // wave-uniform: the removed entries of this step
            while (mask) {
                const int l = (int)__builtin_ctzll(mask);
                const uint32_t qq = (uint32_t)__builtin_amdgcn_readlane((int)q, l);
                const unsigned long long same = __ballot(hit && q == qq);
                mask &= ~same;
                if (lane == (int)(qq & 63u)) a.hits[e0 + qq] += (uint32_t)__popcll(same);
            }
        }
    }
    if (lane == 0) a.kept[i] = cnt;
}

__global__ __launch_bounds__(256) void revise_kernel(ReviseArgs a) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= a.nmajor) return;                              // wave-uniform
    const uint32_t o0 = a.optr[i], on = a.optr[i + 1] - o0, d0 = a.nptr[i];
    const uint32_t e0 = a.eptr[i], ne = a.eptr[i + 1] - e0;
    if (ne == 0) {                                          // no edit: a plain copy
        for (uint32_t e = lane; e < on; e += 64u) { a.nidx[d0 + e] = a.oidx[o0 + e]; a.nval[d0 + e] = a.oval[o0 + e]; }
        return;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t out = 0;                                       // entries written so far (the same in every lane)
    for (uint32_t base = 0; base < on; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        const bool valid = e < on;
        const uint32_t j = valid ? a.oidx[o0 + e] : 0u;
        const real y = valid ? a.oval[o0 + e] : real(0);
        const bool keep = valid && revise_find(a.eidx + e0, ne, j) == ne;
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const uint32_t d = d0 + out + (uint32_t)__popcll(mask & below);
            a.nidx[d] = j;
            a.nval[d] = y;
        }
        out += (uint32_t)__popcll(mask);
    }
    for (uint32_t base = 0; base < ne; base += 64u) {       // the sets follow the survivors, in list order
        const uint32_t e = base + (uint32_t)lane;
        const bool set = e < ne && a.edel[e0 + e] == 0;
        const unsigned long long mask = __ballot(set);
        if (set) {
            const uint32_t d = d0 + out + (uint32_t)__popcll(mask & below);
            a.nidx[d] = a.eidx[e0 + e];
            a.nval[d] = a.eval[e0 + e];
        }
        out += (uint32_t)__popcll(mask);
    }
}

__global__ __launch_bounds__(256) void dense_revise_kernel(DenseReviseArgs a) {
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < a.count; e += gridDim.x * 256u) {
        const uint32_t t = a.rows[e], j = a.cols[e];
        if (t >= (uint32_t)a.T || j >= (uint32_t)a.n) continue;        // (the host has refused such a batch)
        const real y = a.vals[e];
        a.tn[(size_t)t * a.n + j] = y;
        if (a.nt) a.nt[(size_t)j * a.T + t] = y;
    }
}

template <int NT>
__global__ __launch_bounds__(64) void series_revise_kernel(SeriesReviseArgs a) {
    constexpr int KMAX = kTile * NT;
    const int c = threadIdx.x, k = a.k;
    if ((int)blockIdx.x >= a.ntouched) return;
    const uint32_t j = a.list[blockIdx.x];
    const bool on = c < k;
    const int cp = colpos(on ? c : k - 1, NT);
    const size_t PK = adapt_packed(k);
    real col[KMAX], rr = 0;
    const real *Sj = a.Sin + (size_t)j * PK;
#pragma unroll
    for (int s = 0; s < KMAX; s++) col[s] = (on && s <= c) ? Sj[s * k - s * (s - 1) / 2 + c - s] : real(0);
    if (on) rr = a.rin[(size_t)j * k + c];
    const uint32_t q0 = a.eptr[j], ne = a.eptr[j + 1] - q0;
    // the removed entries: every stored copy of an edited cell, in stored order, with the sign of the weight flipped
    const uint32_t e0 = a.ptr[j], e1 = a.ptr[j + 1];
    for (uint32_t base = e0; base < e1; base += 64u) {
        const uint32_t e = base + (uint32_t)c;
        const bool valid = e < e1;
        const uint32_t t = valid ? a.idx[e] : 0u;
        const bool gone = valid && revise_find(a.eidx + q0, ne, t) < ne;
        const real y = gone ? a.val[e] : real(0);
        const real om = gone ? -(a.omega ? a.omega[t] : real(1)) : real(0);
        unsigned long long mask = __ballot(gone);           // wave-uniform: the removed entries of this batch, in stored order
        while (mask) {
            const int l = (int)__builtin_ctzll(mask);
            mask &= mask - 1ull;
            const int tq = adapt_bcast((int)t, l);
            const real wq = a.W[(size_t)tq * a.KP + cp];
            adapt_rank1<KMAX>(col, rr, on ? wq : real(0), adapt_bcast(om, l), adapt_bcast(y, l));
        }
    }
    // the sets of the column, timestamps ascending
    for (uint32_t base = 0; base < ne; base += 64u) {
        const uint32_t e = base + (uint32_t)c;
        const bool set = e < ne && a.edel[q0 + e] == 0;
        const uint32_t t = set ? a.eidx[q0 + e] : 0u;
        const real y = set ? a.eval[q0 + e] : real(0);
        const real om = set ? (a.omega ? a.omega[t] : real(1)) : real(0);
        unsigned long long mask = __ballot(set);
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
