// smooth_robust_kernels.hpp -- the robust fixed-interval smoother (trmf_session_smooth_robust): the smoother of smooth_kernels.hpp
// on the Huber form of its objective, by iteratively reweighted least squares around its PCG.  With t_j = c scale_j:
//
//     J_rob = sum_{i>=f} sum_{j in Omega_i} rho_{t_j}(y_ij - w_i . h_j) + 1/2 lambdaI sum |w_i|^2 + 1/2 lambdaAR sum |e_i|^2
//     x^0 = the rows as they stand;   sweep s:  omega_ij = t_j / |r_ij| if |r_ij| > t_j else 1,  r_ij = y_ij - x^{s-1}_i . h_j
//                                               G_i = sum_j omega_ij h_j h_j^T,  b_i = sum_j omega_ij y_ij h_j
//                                               x^s = the smoother's system with these G_i, b_i, by its PCG from x^{s-1}
//
// The weights depend on the iterate, so neither the Gram cache nor (on dense storage) the shared H^T H is of use: every sweep
// gathers the h_j of every window row again.  Two launches per sweep build all G_i, b_i of the window:
//
//   smooth_robust_part_kernel<NT>   ONE launch for the whole window, one workgroup per item.  An item is one row and a span of its
//                                   entries (stored entries, or series on the dense path); the host cuts the items from the row
//                                   lengths alone (smooth_robust_span).  assim_robust_part_kernel's scheme: x^{s-1}_i staged in LDS; a
//                                   16-lane group owns one entry and forms r and omega (stored to the weights scratch); four entries
//                                   are one K = 4 slice of the 16x16x4 MFMA with omega h as the A operand and h as the B operand;
//                                   the four wavefronts fold their tiles, right-hand sides, counts of omega < 1 and fp64 sums of
//                                   omega in wavefront order through LDS into the item's own slot of a slab.  An item of more
//                                   entries than one slice walks them in several trips of the same loop.
//                                   Score-only mode (a.score): no MFMA, no weights; the item's fp64 sum of rho and of r^2 with the
//                                   dot products in fp64 (assim_err_kernel's reading of an entry).
//   smooth_robust_fold_kernel<NT>   one workgroup per row: adds the row's slots in item order, writes G_i as a full k x k block
//                                   (the upper triangle mirrored) and b_i (KP logical columns) to scratch of the call's own, and
//                                   the row's count of omega < 1 and sum of omega in fp64.  A row without entries gets zeros.
//
// After the fold each sweep runs assim_factor_kernel and the smooth_* kernels unchanged.  No floating-point atomics and no
// workgroup waits for another; every sum has a fixed order GIVEN the slice, so repeated calls and every rank end with the same
// bits.  A different slice (TRMF_TEST + TRMF_SMOOTH_ROBUST_SLICE) cuts the sums differently: the bits are NOT guaranteed to be
// those of the default slice, only the result to rounding.
#pragma once

#include "common.hpp"
#include "gram_kernels.hpp"

namespace trmf {

constexpr int kSmoothRobustSlice = 256;         // entries per item (robust_kernels.hpp: four trips of a workgroup)
constexpr int kSmoothRobustMaxItems = 8;        // the cap on the items of one row: bounds the slab at 8 (KP^2 + KP) reals per row
constexpr int kSmoothRobustMaxSweeps = 64;

// entries per item of a row of `len` entries: the slice, or for rows beyond kSmoothRobustMaxItems slices the smallest multiple of
// the slice that keeps the row within the cap.  Depends on the row's length only.
__host__ __device__ inline uint64_t smooth_robust_span(uint64_t len, int slice) {
    const uint64_t cap = (uint64_t)kSmoothRobustMaxItems * (uint64_t)slice;
    if (len <= cap) return (uint64_t)slice;
    const uint64_t per = (len + kSmoothRobustMaxItems - 1) / kSmoothRobustMaxItems;
    return (per + slice - 1) / slice * slice;
}
__host__ __device__ inline size_t smooth_robust_slot_reals(int KP) { return (size_t)KP * KP + KP; }
constexpr int kSmoothRobustSlotD = 4;           // per item in fp64: count of omega < 1, sum of omega, sum of rho, sum of r^2

struct SmoothRobustArgs {
    const uint32_t *ptr, *idx;         // CSR of the training matrix (sparse storage), or nullptr
    const real *val;
    const real *Yd;                    // dense T x n row-major training matrix, or nullptr
    const real *H;
    const real *xc;                    // x^{s-1}: m x KP, column-interleaved, pads zero
    const real *thr;                   // n: c * scale_j in the element type
    real *weights;                     // one per stored entry of rows first_row .. in CSR order / m x n
    const uint32_t *items;             // per item: window row, first entry, end entry (CSR positions, or series on the dense path)
    const uint32_t *row_item;          // m + 1: the first item of every window row
    real *slab;                        // per item: the upper tiles of sum omega h h^T as KP x KP logical row-major, then KP right-hand sides
    double *slab_d;                    // per item: kSmoothRobustSlotD sums
    real *G;                           // m x (k x k)
    real *Bv;                          // m x KP, logical columns
    double *rowsum;                    // per row: count of omega < 1, sum of omega
    int first_row, m, n, k, KP;
    int score;
};

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
template <int NT>
__global__ void smooth_robust_part_kernel(SmoothRobustArgs a);
template <int NT>
__global__ void smooth_robust_fold_kernel(SmoothRobustArgs a);
#else
__device__ constexpr int smooth_robust_tile(int ti, int tj, int NT) { return ti * NT - ti * (ti - 1) / 2 + (tj - ti); }     // upper tiles, row-major

template <int NT>
__global__ __launch_bounds__(256) void smooth_robust_part_kernel(SmoothRobustArgs a) {
    using M = Mfma16<real>;
    using acc_t = typename M::acc_t;
    constexpr int KP = kTile * NT, NTT = NT * (NT + 1) / 2;
    __shared__ real wl[KP];                                 // x^{s-1}_i, column-interleaved like a row of H
    __shared__ real fold[NTT * 256];                        // [tile][register][lane]
    __shared__ real bfold[KP];                              // logical columns
    __shared__ double dfold[kSmoothRobustSlotD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const uint32_t r = a.items[3 * (size_t)blockIdx.x], e0 = a.items[3 * (size_t)blockIdx.x + 1], e1 = a.items[3 * (size_t)blockIdx.x + 2];
    const int i = a.first_row + (int)r;
    if (tid < KP) wl[tid] = a.xc[(size_t)r * KP + tid];
    __syncthreads();
    const uint32_t wbase = a.ptr ? a.ptr[a.first_row] : 0u;                     // weights[e - wbase]
    real *wrow = a.ptr ? a.weights : a.weights + (size_t)r * a.n;
    const real *yrow = a.ptr ? a.val : a.Yd + (size_t)i * a.n;
    double cnt = 0, sw = 0, srho = 0, sr2 = 0;
    real *slot = a.slab + (size_t)blockIdx.x * smooth_robust_slot_reals(KP);
    if (a.score) {
        // wavefront w takes the groups w, w + 4, ... of four consecutive entries; lane group g owns entry g of the group
        for (uint32_t base = e0 + 4u * (uint32_t)wave; base < e1; base += 16u) {
            const uint32_t e = base + (uint32_t)g;
            const bool valid = e < e1;
            const uint32_t j = valid ? (a.ptr ? a.idx[e] : e) : 0u;
            const double y = valid ? (double)yrow[e] : 0.0;
            const RealVec<NT> xv = *reinterpret_cast<const RealVec<NT> *>(a.H + (size_t)j * KP + NT * c);
            double part = 0;
#pragma unroll
            for (int q = 0; q < NT; q++) part = fma((double)wl[NT * c + q], (double)xv.v[q], part);
            const double dot = row16_allsum(part);
            const double res = fabs(y - dot), t = (double)a.thr[j];
            if (valid && c == 0) {
                srho += res > t ? t * res - 0.5 * t * t : 0.5 * res * res;
                sr2 += res * res;
            }
        }
    } else {
        acc_t acc[NTT];
        real b[NT];
#pragma unroll
        for (int t = 0; t < NTT; t++) acc[t] = acc_t{0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < NT; q++) b[q] = 0;
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
                    const int t_ = smooth_robust_tile(ti, tj, NT);
                    acc[t_] = M::mma(ax[ti], x[tj], acc[t_]);
                }
        }
        // the four entries of a group, then the four wavefronts in order
#pragma unroll
        for (int q = 0; q < NT; q++) {
            b[q] += __shfl_xor(b[q], 16, kWave);
            b[q] += __shfl_xor(b[q], 32, kWave);
        }
        for (int w = 0; w < 4; w++) {
            if (wave == w) {
#pragma unroll
                for (int t = 0; t < NTT; t++)
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) {
                        real *dst = fold + t * 256 + rr * 64 + lane;
                        *dst = w == 0 ? acc[t][rr] : *dst + acc[t][rr];
                    }
                if (lane < 16) {
#pragma unroll
                    for (int q = 0; q < NT; q++) bfold[16 * q + lane] = w == 0 ? b[q] : bfold[16 * q + lane] + b[q];
                }
            }
            __syncthreads();
        }
        // thread (wave, lane) copies register `wave` of every tile: row M::row(lane, wave), column lane & 15 of the tile
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
            for (int tj = ti; tj < NT; tj++) {
                const int t_ = smooth_robust_tile(ti, tj, NT);
                slot[(size_t)(16 * ti + M::row(lane, wave)) * KP + 16 * tj + c] = fold[t_ * 256 + wave * 64 + lane];
            }
        if (tid < KP) slot[(size_t)KP * KP + tid] = bfold[tid];
    }
    cnt += __shfl_xor(cnt, 16, kWave); cnt += __shfl_xor(cnt, 32, kWave);
    sw += __shfl_xor(sw, 16, kWave); sw += __shfl_xor(sw, 32, kWave);
    srho += __shfl_xor(srho, 16, kWave); srho += __shfl_xor(srho, 32, kWave);
    sr2 += __shfl_xor(sr2, 16, kWave); sr2 += __shfl_xor(sr2, 32, kWave);
    for (int w = 0; w < 4; w++) {
        if (wave == w && lane == 0) {
            dfold[0] = w == 0 ? cnt : dfold[0] + cnt;
            dfold[1] = w == 0 ? sw : dfold[1] + sw;
            dfold[2] = w == 0 ? srho : dfold[2] + srho;
            dfold[3] = w == 0 ? sr2 : dfold[3] + sr2;
        }
        __syncthreads();
    }
    if (tid < kSmoothRobustSlotD) a.slab_d[(size_t)kSmoothRobustSlotD * blockIdx.x + tid] = dfold[tid];
}

template <int NT>
__global__ __launch_bounds__(256) void smooth_robust_fold_kernel(SmoothRobustArgs a) {
    constexpr int KP = kTile * NT;
    const int tid = threadIdx.x, r = blockIdx.x, k = a.k;
    const uint32_t i0 = a.row_item[r], i1 = a.row_item[r + 1];
    const size_t stride = smooth_robust_slot_reals(KP);
    real *Gi = a.G + (size_t)r * k * k;
    // element (s, t) of G_i from the upper triangle of the slots, the slots in item order
    for (int e = tid; e < k * k; e += 256) {
        const int s = e / k, t = e % k;
        const int lo = s < t ? s : t, hi = s < t ? t : s;
        real v = 0;
        for (uint32_t it = i0; it < i1; it++) v += a.slab[(size_t)it * stride + (size_t)lo * KP + hi];
        Gi[e] = v;
    }
    for (int t = tid; t < KP; t += 256) {
        real v = 0;
        for (uint32_t it = i0; it < i1; it++) v += a.slab[(size_t)it * stride + (size_t)KP * KP + t];
        a.Bv[(size_t)r * KP + t] = t < k ? v : real(0);
    }
    if (tid < 2) {
        double v = 0;
        for (uint32_t it = i0; it < i1; it++) v += a.slab_d[(size_t)kSmoothRobustSlotD * it + tid];
        a.rowsum[2 * (size_t)r + tid] = v;
    }
}
#endif

}  // namespace trmf
