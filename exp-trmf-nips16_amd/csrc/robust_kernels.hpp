// robust_kernels.hpp -- outlier-robust online updates (trmf_session_assimilate_robust): the forward filter of online_kernels.hpp
// with Huber weights.  Row i of W, in ascending order, is `sweeps` rounds of iteratively reweighted least squares from the prior
// p_i (H, Theta and the earlier rows fixed):
//
//     w^0 = p_i;   r_j = y_ij - w^{s-1} . h_j,   omega_j = t_j / |r_j| if |r_j| > t_j else 1      (t_j = c scale_j, j in Omega_i)
//                  w^s = (sum_j omega_j h_j h_j^T + (lambdaI + lambdaAR) I)^-1 (sum_j omega_j y_ij h_j + lambdaAR p_i)
//
// The weights depend on the iterate, so nothing of the Gram cache can be reused: every sweep gathers the row's h_j again.  Two
// launches per row and sweep, all on the session's stream, no host synchronisation in between:
//
//   assim_robust_part_kernel<NT>    one workgroup per slice of the row's entries (stored entries, or series on the dense path).
//                                   w^{s-1} is staged in LDS; a 16-lane group owns one entry and forms r and omega (stored to the
//                                   weights scratch); four entries are one K = 4 slice of the 16x16x4 MFMA with omega h as the A
//                                   operand and h as the B operand, so the upper tiles of sum omega h h^T grow as in the Gram
//                                   builders.  The four wavefronts fold their tiles, right-hand sides, counts of omega < 1 and
//                                   fp64 sums of omega in wavefront order through LDS into the workgroup's own slot of a slab.
//   assim_robust_solve_kernel<NT>   one workgroup: adds the slots in slice order, adds the ridge, factors with lane c holding column
//                                   c (assim_factor_kernel's scheme) and substitutes with one unknown per lane (assim_chain_kernel's).
//                                   A pivot that is not positive and finite raises the flag with the row's index.  On the last sweep
//                                   it also writes the row to the scratch of new rows and forms p_{i+1} from global memory
//                                   (assim_rhs_global's rounding: contraction off, ascending lag order).
//   assim_robust_prior_kernel       p of the first row.
//
// No floating-point atomics and no workgroup waits for another: every sum has a fixed order, so repeated calls and every rank end
// with the same bits.
#pragma once

#include "common.hpp"
#include "gram_kernels.hpp"

namespace trmf {

// entries per workgroup of the part kernel (TRMF_TEST + TRMF_ASSIM_ROBUST_SLICE overrides).  A wavefront's entries are a chain of
// dependent gathers (index -> row of H -> residual), 16 entries of the slice per trip: 256 keeps a workgroup to four trips.  Measured
// with slices of 1024: 43 us per dispatch on rows of ~1000 entries, 14-18 us on rows of 300-370
constexpr int kAssimRobustSlice = 256;
constexpr int kAssimRobustMaxSweeps = 64;

struct AssimRobustArgs {
    const uint32_t *ptr, *idx;         // CSR of the training matrix (sparse storage), or nullptr
    const real *val;
    const real *Yd;                    // dense T x n row-major training matrix, or nullptr
    const real *H;
    const real *W;                     // the session's W: rows < first_row are read from here
    real *Wnew;                        // rows first_row .. : (rows - first_row) x KP, column-interleaved, pads zero
    real *flat;                        // nullptr, or (rows - first_row) x k row-major
    real *wcur;                        // KP: w^{s-1}, column-interleaved, pads zero
    real *prior;                       // KP: p_i, column-interleaved
    const real *thr;                   // n: c * scale_j in the element type
    real *weights;                     // one per stored entry of rows first_row .. in CSR order / (rows - first_row) x n
    real *slab;                        // per slice: the upper tiles of sum omega h h^T as KP x KP logical row-major, then KP right-hand sides
    double *slab_d;                    // per slice: count of omega < 1, sum of omega
    double *rowsum;                    // per row: the same two of the last sweep
    const uint32_t *lag_set;
    const real *theta;                 // Theta(l, t) at t * nlag + l
    int *flag;
    real lam, lamAR;
    int first_row, T, i, n, k, KP, nlag;
    int slice, nslices, last;
};

__host__ __device__ inline size_t assim_robust_slot_reals(int KP) { return (size_t)KP * KP + KP; }

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
template <int NT>
__global__ void assim_robust_part_kernel(AssimRobustArgs a);
template <int NT>
__global__ void assim_robust_solve_kernel(AssimRobustArgs a);
__global__ void assim_robust_prior_kernel(AssimRobustArgs a);
#else
__device__ constexpr int assim_robust_tile(int ti, int tj, int NT) { return ti * NT - ti * (ti - 1) / 2 + (tj - ti); }     // upper tiles, row-major
__device__ __forceinline__ void assim_robust_wave_sync() {          // LDS operations of one wavefront retire in order
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// p_i for latent dimension t: products rounded to the element type and summed in ascending lag order, like Model.latent_forecast
__device__ __forceinline__ real assim_robust_prior(const AssimRobustArgs &a, int i, int t, int tp) {
#pragma clang fp contract(off)
    real acc = 0;
    for (int l = 0; l < a.nlag; l++) {
        const int src = i - (int)a.lag_set[l];              // >= 0: first_row >= the largest lag
        const real w = src >= a.first_row ? a.Wnew[(size_t)(src - a.first_row) * a.KP + tp] : a.W[(size_t)src * a.KP + tp];
        const real prod = w * a.theta[(size_t)t * a.nlag + l];
        acc = acc + prod;
    }
    return acc;
}
__device__ __forceinline__ real assim_robust_rhs(real b, real lamAR, real p) {
#pragma clang fp contract(off)
    const real pen = lamAR * p;
    return b + pen;
}

__global__ __launch_bounds__(64) void assim_robust_prior_kernel(AssimRobustArgs a) {
    const int t = threadIdx.x;
    if (t >= a.k) return;
    const int tp = colpos(t, a.KP / kTile);
    const real p = assim_robust_prior(a, a.i, t, tp);
    a.prior[tp] = p;
    a.wcur[tp] = p;
}

template <int NT>
__global__ __launch_bounds__(256) void assim_robust_part_kernel(AssimRobustArgs a) {
    using M = Mfma16<real>;
    using acc_t = typename M::acc_t;
    constexpr int KP = kTile * NT, NTT = NT * (NT + 1) / 2;
    __shared__ real wl[KP];                                 // w^{s-1}, column-interleaved like a row of H
    __shared__ real fold[NTT * 256];                        // [tile][register][lane]
    __shared__ real bfold[KP];                              // logical columns
    __shared__ double dfold[2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    if (tid < KP) wl[tid] = a.wcur[tid];
    __syncthreads();
    // this workgroup's entries: positions [e0, e1) of the CSR arrays, or series [e0, e1) of the dense row
    uint32_t e0, e1, wbase;
    if (a.ptr) {
        const uint32_t p0 = a.ptr[a.i], p1 = a.ptr[a.i + 1];
        e0 = p0 + (uint32_t)blockIdx.x * (uint32_t)a.slice;
        e1 = min(p1, e0 + (uint32_t)a.slice);
        wbase = a.ptr[a.first_row];                         // weights[e - wbase]
    } else {
        e0 = (uint32_t)blockIdx.x * (uint32_t)a.slice;
        e1 = min((uint32_t)a.n, e0 + (uint32_t)a.slice);
        wbase = 0;
    }
    real *wrow = a.ptr ? a.weights : a.weights + (size_t)(a.i - a.first_row) * a.n;
    const real *yrow = a.ptr ? a.val : a.Yd + (size_t)a.i * a.n;
    acc_t acc[NTT];
    real b[NT];
#pragma unroll
    for (int t = 0; t < NTT; t++) acc[t] = acc_t{0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < NT; q++) b[q] = 0;
    double cnt = 0, sw = 0;
    // wavefront w takes the groups w, w + 4, ... of four consecutive entries; lane group g owns entry g of the group
    for (uint32_t base = e0 + 4u * (uint32_t)wave; base < e1; base += 16u) {
        const uint32_t e = base + (uint32_t)g;
        const bool valid = e < e1;
        const uint32_t j = valid ? (a.ptr ? a.idx[e] : e) : 0u;
        const real y = valid ? yrow[e] : real(0);
        const RealVec<NT> xv = *reinterpret_cast<const RealVec<NT> *>(a.H + (size_t)j * KP + NT * c);
        real x[NT], part = 0;
#pragma unroll
        for (int q = 0; q < NT; q++) {
            x[q] = valid ? xv.v[q] : real(0);
            part = fma(wl[NT * c + q], x[q], part);
        }
        const real dot = row16_allsum(part);                // the same bits in the 16 lanes of the group
        const real res = fabs(y - dot), t = a.thr[j];
        const real om = res > t ? t / res : real(1);
        if (valid && c == 0) {
            wrow[e - wbase] = om;
            cnt += om < real(1) ? 1.0 : 0.0;
            sw += (double)om;
        }
        real ax[NT];
#pragma unroll
        for (int q = 0; q < NT; q++) {
            ax[q] = om * x[q];
            b[q] = fma(ax[q], y, b[q]);
        }
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
            for (int tj = ti; tj < NT; tj++) {
                const int t_ = assim_robust_tile(ti, tj, NT);
                acc[t_] = M::mma(ax[ti], x[tj], acc[t_]);
            }
    }
    // the four entries of a group, then the four wavefronts in order
#pragma unroll
    for (int q = 0; q < NT; q++) {
        b[q] += __shfl_xor(b[q], 16, kWave);
        b[q] += __shfl_xor(b[q], 32, kWave);
    }
    cnt += __shfl_xor(cnt, 16, kWave); cnt += __shfl_xor(cnt, 32, kWave);
    sw += __shfl_xor(sw, 16, kWave); sw += __shfl_xor(sw, 32, kWave);
    for (int w = 0; w < 4; w++) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < NTT; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    real *dst = fold + t * 256 + r * 64 + lane;
                    *dst = w == 0 ? acc[t][r] : *dst + acc[t][r];
                }
            if (lane < 16) {
#pragma unroll
                for (int q = 0; q < NT; q++) bfold[16 * q + lane] = w == 0 ? b[q] : bfold[16 * q + lane] + b[q];
            }
            if (lane == 0) {
                dfold[0] = w == 0 ? cnt : dfold[0] + cnt;
                dfold[1] = w == 0 ? sw : dfold[1] + sw;
            }
        }
        __syncthreads();
    }
    real *slot = a.slab + (size_t)blockIdx.x * assim_robust_slot_reals(KP);
    // thread (wave, lane) copies register `wave` of every tile: row M::row(lane, wave), column lane & 15 of the tile
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = ti; tj < NT; tj++) {
            const int t_ = assim_robust_tile(ti, tj, NT);
            slot[(size_t)(16 * ti + M::row(lane, wave)) * KP + 16 * tj + c] = fold[t_ * 256 + wave * 64 + lane];
        }
    if (tid < KP) slot[(size_t)KP * KP + tid] = bfold[tid];
    if (tid < 2) a.slab_d[2 * (size_t)blockIdx.x + tid] = dfold[tid];
}

template <int NT>
__global__ __launch_bounds__(256) void assim_robust_solve_kernel(AssimRobustArgs a) {
    constexpr int KP = kTile * NT, KMAX = KP, SP = KP + 1;   // odd pitch: column reads spread over the banks
    __shared__ real S[KP * SP];                             // the summed upper tiles, then the factor U
    __shared__ real bs[KP];
    const int tid = threadIdx.x, wave = tid >> 6, c = tid & 63;
    const int k = a.k, i = a.i;
    const size_t stride = assim_robust_slot_reals(KP);
    // the slots in slice order; only the upper tiles are defined
    for (int e = tid; e < KP * KP + KP; e += 256) {
        const int row = e / KP, col = e % KP;
        if (row < KP && (row >> 4) > (col >> 4)) continue;
        real v = 0;
        for (int s = 0; s < a.nslices; s++) v += a.slab[(size_t)s * stride + e];
        if (row < KP) S[row * SP + col] = v;
        else bs[col] = v;
    }
    if (a.last && tid == 64) {
        double cnt = 0, sw = 0;
        for (int s = 0; s < a.nslices; s++) { cnt += a.slab_d[2 * (size_t)s]; sw += a.slab_d[2 * (size_t)s + 1]; }
        a.rowsum[2 * (size_t)(i - a.first_row)] = cnt;
        a.rowsum[2 * (size_t)(i - a.first_row) + 1] = sw;
    }
    __syncthreads();
    if (wave > 0) return;                                   // one wavefront from here on: no block barrier below
    // lane c keeps column c of A (the upper triangle mirrored); rows and columns >= k are padded with the identity
    real col[KMAX];
#pragma unroll
    for (int s = 0; s < KMAX; s++) {
        real v = (s == c) ? real(1) : real(0);
        if (s < k && c < k) {
            v = s <= c ? S[s * SP + c] : S[c * SP + s];
            if (s == c) v += a.lam;
        }
        col[s] = v;
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < KMAX; j++) {
        const real piv = lane_bcast(col[j], j);
        bad = bad || !(piv > real(0) && piv < real(INFINITY));
        const real d = sqrt(piv);
        const real u = (c == j) ? d : col[j] / d;
        col[j] = u;
#pragma unroll
        for (int s = j + 1; s < KMAX; s++) {
            col[s] = fma(-lane_bcast(u, s), u, col[s]);
            if ((s & 15) == 15) __builtin_amdgcn_sched_barrier(0);       // bound the scalar operands in flight
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (bad && c == 0) atomicMin(a.flag, i);
    assim_robust_wave_sync();                                        // every lane has read its column of A
    if (c < k) {
#pragma unroll
        for (int s = 0; s < KMAX; s++)
            if (s < k) S[s * SP + c] = s <= c ? col[s] : real(0);
    }
    assim_robust_wave_sync();
    const bool on = c < k;
    const int t = on ? c : k - 1;                           // idle lanes shadow the last unknown and store nothing
    const int tp = colpos(t, NT);
    real x = assim_robust_rhs(bs[t], a.lamAR, a.prior[tp]);
    // column-oriented substitutions, one unknown per lane (assim_chain_kernel)
    for (int q = 0; q < k; q++) {                           // U^T z = b
        const real zq = lane_bcast(x, q) / S[q * SP + q];
        if (c == q) x = zq;
        else if (c > q) x -= S[q * SP + t] * zq;
    }
    for (int q = k - 1; q >= 0; q--) {                      // U x = z
        const real xq = lane_bcast(x, q) / S[q * SP + q];
        if (c == q) x = xq;
        else if (c < q) x -= S[t * SP + q] * xq;
    }
    if (!on) return;
    a.wcur[tp] = x;
    if (a.last) {
        a.Wnew[(size_t)(i - a.first_row) * a.KP + tp] = x;
        if (a.flat) a.flat[(size_t)(i - a.first_row) * k + t] = x;
        if (i + 1 < a.T) {                                  // the next row starts from its prior (this lane reads its own column only)
            const real p = assim_robust_prior(a, i + 1, t, tp);
            a.prior[tp] = p;
            a.wcur[tp] = p;
        }
    }
}
#endif

}  // namespace trmf
