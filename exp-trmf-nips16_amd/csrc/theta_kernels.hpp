// theta_kernels.hpp -- lag-weight (Theta) update on device: trmf.cpp:447-484
// (l2r_autoregressive_solver::{lagged_inner_product, solve}).
//
// Per latent dimension t: |L| x |L| Gram of lagged inner products of the series W[:,t] over
// i in [midx, T) with double accumulators, + lambdaLag on the diagonal, Cholesky solve in val_type.
// Kept on device so that the ALS loop never round-trips W to the host.
#pragma once

#include "common.hpp"

namespace trmf {

constexpr int kThetaChunk = 512;    // timestamps per workgroup of theta_gram_kernel (2048 -> 512: 92 us -> ~40 us at config 3)
constexpr int kMaxLags = 1024;      // beyond ~140 (fp64) / 200 (fp32) lags the |L| x |L| systems of theta_solve_kernel no longer fit LDS: global scratch

// pair index p in [0, npairs): p < nlag -> rhs entry y[p] = <s_i, s_{i-L_p}>;
// otherwise the upper-triangle entry (a, b), a <= b, in row-major order.
__device__ __forceinline__ void theta_decode_pair(int p, int nlag, int &a, int &b, bool &rhs) {
    if (p < nlag) { rhs = true; a = p; b = p; return; }
    rhs = false;
    int q = p - nlag, row = 0, len = nlag;
    while (q >= len) { q -= len; row++; len--; }
    a = row; b = row + q;
}

// grid (k, nchunk), 256 threads, dynamic LDS = theta_gram_lds_bytes(midx, nlag).
// Register tiling: a thread owns a 4 x 4 block of lag pairs (a in ta, b in tb, tb >= ta; the "zero lag" series s_i
// against a block of four lags for the right-hand side) and, when there are fewer blocks than threads, one of S time
// slices of the chunk -- per timestamp it reads 8 series values from LDS for 16 products (0.5 reads per product instead
// of 2).  Products are rounded to val_type, sums are double (trmf.cpp:447-453); the S slice sums of a block are added
// in fixed order through LDS.  The lag set is staged in LDS beside the series.
constexpr int kThetaTile = 4;
constexpr int kThetaRows = 4;     // consecutive timestamps per pass of the sliding-window path
// Slice sums in LDS: entry e of thread x at red[e * kThetaRedStride + x].  Neighbouring lanes store neighbouring doubles (thread-major
// rows of 16 doubles put every second lane of a store on the same banks); the odd stride keeps the 16 entries of a block, which the
// closing reduction reads side by side, on different banks (the blocks of a wavefront, S doubles apart, may still share some).
constexpr int kThetaRedStride = 257;
__host__ __device__ inline size_t theta_gram_series_bytes(int midx) {
    return ((size_t)(kThetaChunk + midx + kThetaRows) * sizeof(real) + 15) / 16 * 16;   // + window slack
}
__host__ __device__ inline size_t theta_gram_lds_bytes(int midx, int nlag) {        // series | red | blocks of a pass | lag set
    return theta_gram_series_bytes(midx) + (size_t)16 * kThetaRedStride * sizeof(double) + (size_t)(256 + nlag) * sizeof(int);
}
// block q of the row-major upper triangle of NA x NA blocks (row r starts at r NA - r (r - 1) / 2) -> (row, column).  The root is
// taken of an integer that fp32 holds exactly ((2 NA + 1)^2 <= 2^24 up to kMaxLags), so the estimate is off by one row at most.
__device__ __forceinline__ void theta_decode_tile(int q, int NA, int &ta, int &tb) {
    const float h = (float)(2 * NA + 1);
    int r = min(NA - 1, max(0, (int)((h - sqrtf(h * h - 8.0f * (float)q)) * 0.5f)));
    while (r > 0 && r * NA - r * (r - 1) / 2 > q) r--;
    while ((r + 1) * NA - (r + 1) * r / 2 <= q) r++;
    ta = r; tb = r + (q - (r * NA - r * (r - 1) / 2));
}
__global__ __launch_bounds__(256) void theta_gram_kernel(const real *__restrict__ W, int T, int KP,
                                                         const uint32_t *__restrict__ lag_set,
                                                         int nlag, int midx, int npairs,
                                                         double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    real *series = reinterpret_cast<real *>(smem_raw);
    double *red = reinterpret_cast<double *>(smem_raw + theta_gram_series_bytes(midx));
    int *blocks = reinterpret_cast<int *>(red + 16 * kThetaRedStride);     // (row | column << 16) of the blocks of a pass, for its closing reduction
    int *lags = blocks + 256;
    const int t = blockIdx.x, ch = blockIdx.y, nchunk = gridDim.y;
    const int i0 = midx + ch * kThetaChunk;
    const int i1 = min(T, i0 + kThetaChunk);
    const int lo = i0 - midx;                           // first timestamp staged
    const int tp = colpos(t, KP / kTile);                 // column-interleaved factor layout
    for (int i = threadIdx.x; i < nlag; i += 256) lags[i] = (int)lag_set[i];
    for (int i = lo + threadIdx.x; i < i1; i += 4 * 256) {      // four loads of a thread in flight
        real w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) w[u] = i + u * 256 < i1 ? W[(size_t)(i + u * 256) * KP + tp] : real(0);
#pragma unroll
        for (int u = 0; u < 4; u++) if (i + u * 256 < i1) series[i + u * 256 - lo] = w[u];
    }
    __syncthreads();
    const int NA = (nlag + kThetaTile - 1) / kThetaTile;
    const int ntri = NA * (NA + 1) / 2;
    const int ntiles = ntri + NA;                       // upper-triangle blocks, then the rhs blocks
    const int S = max(1, 256 / ntiles);                 // time slices per block of pairs
    double *out = part + ((size_t)t * nchunk + ch) * npairs;
    for (int base = 0; base < ntiles; base += 256 / S) {
        const int tile = base + (int)threadIdx.x / S, slice = (int)threadIdx.x % S;
        const bool live = tile < ntiles && (int)threadIdx.x < (256 / S) * S;
        int ta = 0, tb = 0;
        bool rhs = false;
        if (live) {
            if (tile >= ntri) { rhs = true; tb = tile - ntri; }
            else theta_decode_tile(tile, NA, ta, tb);
        }
        int la[kThetaTile], lb[kThetaTile];
#pragma unroll
        for (int u = 0; u < kThetaTile; u++) {
            la[u] = rhs ? 0 : lags[min(kThetaTile * ta + u, nlag - 1)];
            lb[u] = lags[min(kThetaTile * tb + u, nlag - 1)];
        }
        double acc[kThetaTile][kThetaTile];
#pragma unroll
        for (int u = 0; u < kThetaTile; u++)
#pragma unroll
            for (int v = 0; v < kThetaTile; v++) acc[u][v] = 0;
        // Blocks whose four lags are consecutive integers on both sides (all of the paper's lag set, every 1..|L| set):
        // a thread then takes kThetaRows consecutive timestamps per pass -- the operands of neighbouring rows and lags
        // overlap, so two windows of kThetaRows + 3 LDS reads feed 16 kThetaRows products (0.22 reads per product
        // instead of 0.5; the kernel is LDS-bound).  Other blocks take the general loop below.
        bool runs = live;
#pragma unroll
        for (int u = 1; u < kThetaTile; u++)
            runs = runs && (rhs || la[u] == la[0] + u) && lb[u] == lb[0] + u;
        if (runs) {
            constexpr int R = kThetaRows, Wn = R + kThetaTile - 1;
            for (int i = i0 + slice * R; i < i1; i += S * R) {
                real wa[Wn], wb[Wn];
                const real *pa = series + (i - la[0] - (kThetaTile - 1) - lo), *pb = series + (i - lb[0] - (kThetaTile - 1) - lo);
#pragma unroll
                for (int m = 0; m < Wn; m++) { wb[m] = pb[m]; wa[m] = rhs ? series[i - lo + min(m, R - 1)] : pa[m]; }
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if (i + r >= i1) break;
#pragma unroll
                    for (int u = 0; u < kThetaTile; u++) {
                        if (rhs && u > 0) break;
                        const real su = rhs ? wa[r] : wa[r - u + kThetaTile - 1];       // s_{i+r-la[u]}
#pragma unroll
                        for (int v = 0; v < kThetaTile; v++) {
                            const real prod = su * wb[r - v + kThetaTile - 1];           // val_type product
                            acc[u][v] += (double)prod;                                 // double accumulate
                        }
                    }
                }
            }
        } else if (live) {
            const int nrow = rhs ? 1 : kThetaTile;
            for (int i = i0 + slice; i < i1; i += S) {
                real sa[kThetaTile], sb[kThetaTile];
#pragma unroll
                for (int u = 0; u < kThetaTile; u++) { sa[u] = series[i - la[u] - lo]; sb[u] = series[i - lb[u] - lo]; }
#pragma unroll
                for (int u = 0; u < kThetaTile; u++)
                    if (u < nrow) {
#pragma unroll
                        for (int v = 0; v < kThetaTile; v++) {
                            const real prod = sa[u] * sb[v];                           // val_type product
                            acc[u][v] += (double)prod;                                 // double accumulate
                        }
                    }
            }
        }
        // slice sums -> LDS -> sixteen threads per block, one per entry, add the S slice sums of their entry in slice order
        // (from 0.0, ascending: the order is part of the result) and store the block's pairs
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kThetaTile; u++)
#pragma unroll
            for (int v = 0; v < kThetaTile; v++) red[(u * kThetaTile + v) * kThetaRedStride + (int)threadIdx.x] = acc[u][v];
        if (live && slice == 0) blocks[tile - base] = ta | (tb << 16);
        __syncthreads();
        for (int o = threadIdx.x; o < (256 / S) * 16; o += 256) {
            const int tl = o >> 4, e = o & 15, rt = base + tl;
            if (rt >= ntiles) break;
            const int u = e / kThetaTile, v = e % kThetaTile;
            const bool rr = rt >= ntri;                 // a rhs block
            const int ra = blocks[tl] & 0xffff, rb = blocks[tl] >> 16;
            const int a = kThetaTile * ra + u, b = kThetaTile * rb + v;
            if (b >= nlag || (!rr && (a >= nlag || a > b)) || (rr && u > 0)) continue;
            const double *src = red + e * kThetaRedStride + tl * S;
            double sum = 0;
            for (int sl = 0; sl < S; sl++) sum += src[sl];
            // pair index: p < nlag -> rhs entry y[b]; otherwise upper-triangle (a, b) in row-major order
            const int p = rr ? b : nlag + a * nlag - a * (a - 1) / 2 + (b - a);
            out[p] = sum;
        }
    }
}

// sum over the time chunks of pair p of latent dimension t, in the fixed chunk order (shared by the ridge and the lasso solve)
__device__ __forceinline__ double theta_sum_pair(const double *__restrict__ part, int nchunk, int npairs, int t, int p) {
    double acc = 0;
#pragma unroll 8
    for (int ch = 0; ch < nchunk; ch++) acc += part[((size_t)t * nchunk + ch) * npairs + p];   // fixed order
    return acc;
}

// a - u c of the Cholesky's trailing update and of the substitutions, as ONE fused multiply-add: what the compiler made of the
// plain expression in theta_chol_solve (fp contraction), written out so that the LDS form and the register form cannot drift apart.
template <typename E> __device__ __forceinline__ E theta_nmsub(E a, E u, E c) { return fma(-u, c, a); }

// A x = y for the symmetric positive definite n x n system A ((i,j) at A[i*n+j], upper triangle read), x left in y; one wavefront
// (lane = 0..63), LDS or -- with the workgroup barriers ordering the accesses -- global scratch.  CHECK: a pivot that is not
// positive and finite ends the factorisation and returns false (A and y are then void); without it nothing is tested.
template <typename E, bool CHECK> __device__ __forceinline__ bool theta_chol_solve(E *A, E *y, int nlag, int lane) {
    // upper Cholesky A = U^T U, row by row (posv 'U', rf_matrix.h:3008-3014).  One wavefront: LDS accesses
    // retire in program order, the barriers are wave-local.  Same operations on every element, in the same j order,
    // as the row-by-row loop.
    for (int j = 0; j < nlag; j++) {
        if (CHECK) { const E piv = A[j * nlag + j]; if (!(piv > E(0)) || !isfinite(piv)) return false; }
        const E ajj = sqrt(A[j * nlag + j]);
        __syncthreads();
        for (int c = j + lane; c < nlag; c += 64) A[j * nlag + c] = (c == j) ? ajj : A[j * nlag + c] / ajj;
        __syncthreads();
        // trailing update, a lane per column (two for more than 64 lags): rows s = j+1 .. c of its column
        for (int c = j + 1 + lane; c < nlag; c += 64) {
            const E ujc = A[j * nlag + c];
            int s = j + 1;
            for (; s + 3 <= c; s += 4) {                 // four independent rows per pass: reads first, then writes
                E u[4], a[4];
#pragma unroll
                for (int q = 0; q < 4; q++) { u[q] = A[j * nlag + s + q]; a[q] = A[(s + q) * nlag + c]; }
#pragma unroll
                for (int q = 0; q < 4; q++) A[(s + q) * nlag + c] = theta_nmsub(a[q], u[q], ujc);
            }
            for (; s <= c; s++) A[s * nlag + c] = theta_nmsub(A[s * nlag + c], A[j * nlag + s], ujc);
        }
        __syncthreads();
    }
    // substitutions, column-oriented: after step q every remaining unknown has had its U(.,.)*z_q term removed:
    // |L| steps of one parallel pass instead of |L|^2/2 dependent LDS round trips on a single lane.  Forward:
    // the same subtractions in the same order as the row-oriented loop; backward: the terms of a row are
    // subtracted in descending instead of ascending q (a last-bit difference in Theta)
    for (int q = 0; q < nlag; q++) {                    // U^T z = y
        if (lane == 0) y[q] = y[q] / A[q * nlag + q];
        __syncthreads();
        for (int i = q + 1 + lane; i < nlag; i += 64) y[i] = theta_nmsub(y[i], A[q * nlag + i], y[q]);
        __syncthreads();
    }
    for (int q = nlag - 1; q >= 0; q--) {               // U x = z
        if (lane == 0) y[q] = y[q] / A[q * nlag + q];
        __syncthreads();
        for (int i = lane; i < q; i += 64) y[i] = theta_nmsub(y[i], A[i * nlag + q], y[q]);
        __syncthreads();
    }
    return true;
}

// one workgroup per latent dimension; dynamic LDS = (nlag*nlag + nlag) * sizeof(real).  All 256 threads add up the
// time-chunk partials (a single wavefront streaming nchunk * npairs doubles is latency-bound: 125 us of the former
// 187 us at 48 lags); the |L| x |L| solve itself is one wavefront's work, the other three retire after the sum.
// `scratch` != null: the systems live there ((nlag*nlag + nlag) reals per latent dimension, L2-resident) instead of LDS -- lag sets
// too long for LDS (the reference has no limit on |L|: trmf.cpp:425-484); same code, workgroup barriers order the accesses.
__global__ __launch_bounds__(256) void theta_solve_kernel(const double *__restrict__ part, int nchunk,
                                                         int nlag, int npairs, double lambdaLag,
                                                         real *__restrict__ theta, real *__restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    real *A = scratch ? scratch + (size_t)blockIdx.x * ((size_t)nlag * nlag + nlag) : reinterpret_cast<real *>(smem_raw);   // nlag x nlag, (i,j) at A[i*nlag+j]
    real *y = A + nlag * nlag;
    const int t = blockIdx.x, lane = threadIdx.x;
    for (int p = threadIdx.x; p < npairs; p += 256) {
        const double acc = theta_sum_pair(part, nchunk, npairs, t, p);
        int a, b; bool rhs;
        theta_decode_pair(p, nlag, a, b, rhs);
        if (rhs) y[a] = (real)acc;
        else {
            real v = (real)acc;                                              // trmf.cpp:473
            if (a == b) v = (real)((double)v + lambdaLag);                   // trmf.cpp:480
            A[a * nlag + b] = v;
            A[b * nlag + a] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;                      // the barriers below only count the wavefront that is left
    theta_chol_solve<real, false>(A, y, nlag, lane);
    for (int a = lane; a < nlag; a += 64) theta[(size_t)t * nlag + a] = y[a];
}

// ---- the register form of the ridge solve: |L| <= kThetaRegMax ------------------------------------------------------------------
// One wavefront holds the system: lane c owns column c, row s is register col[s] (statically indexed, N = the rank class >= |L|),
// the right-hand side is one value per lane.  Pivots and row values travel by v_readlane; there is no LDS access and no barrier in
// the factorisation or the substitutions.  Every element of the upper triangle and of y receives the operations of
// theta_chol_solve in its order: sqrt and true division on row j, the trailing updates in ascending pivot order, the forward
// substitution's terms in ascending q, the backward's in descending q.  What lies below the diagonal (and in lanes >= |L|) is
// updated along with the rest and never read.
constexpr int kThetaRegMax = 32;
__device__ __forceinline__ float theta_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double theta_lane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
template <typename E, int N> __device__ __forceinline__ E theta_chol_solve_reg(E (&col)[N], E yv, int nlag, int lane) {
#pragma unroll
    for (int j = 0; j < N; j++)
        if (j < nlag) {                                 // (wave-uniform)
            const E ajj = sqrt(theta_lane(col[j], j));
            col[j] = lane == j ? ajj : col[j] / ajj;
            const E ujc = col[j];
#pragma unroll
            for (int s = j + 1; s < N; s++) col[s] = theta_nmsub(col[s], theta_lane(ujc, s), ujc);
        }
#pragma unroll
    for (int q = 0; q < N; q++)                         // U^T z = y: lane i keeps y[i]
        if (q < nlag) {
            const E zq = theta_lane(yv, q) / theta_lane(col[q], q);
            yv = lane == q ? zq : lane > q ? theta_nmsub(yv, col[q], zq) : yv;
        }
    // U x = z: U(i,q) is register i of lane q, so the unknowns are kept in every lane (x[i], wave-uniform) and row q's column
    // arrives by N readlanes
    E x[N];
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = theta_lane(yv, i);
#pragma unroll
    for (int q = N - 1; q >= 0; q--)
        if (q < nlag) {
            x[q] = x[q] / theta_lane(col[q], q);
#pragma unroll
            for (int i = 0; i < q; i++) x[i] = theta_nmsub(x[i], theta_lane(col[i], q), x[q]);
        }
    E out = E(0);
#pragma unroll
    for (int i = 0; i < N; i++) out = lane == i ? x[i] : out;
    return out;
}

// theta_sum_pair with the chunk partials of a pair requested 32 at a time before the first add (same adds, same order)
__device__ __forceinline__ double theta_sum_pair_wide(const double *__restrict__ part, int nchunk, int npairs, int t, int p) {
    double acc = 0;
    for (int c0 = 0; c0 < nchunk; c0 += 32) {
        double v[32];
#pragma unroll
        for (int u = 0; u < 32; u++) v[u] = c0 + u < nchunk ? part[((size_t)t * nchunk + c0 + u) * npairs + p] : 0.0;
#pragma unroll
        for (int u = 0; u < 32; u++) if (c0 + u < nchunk) acc += v[u];                          // fixed order
    }
    return acc;
}

// one workgroup per latent dimension, static LDS: the packed pairs.  All 256 threads add up the chunk partials; one wavefront
// then loads its columns (rounding to `real`, then lambdaLag on the diagonal: trmf.cpp:473, 480) and solves in registers.
template <int N>
__global__ __launch_bounds__(256) void theta_solve_reg_kernel(const double *__restrict__ part, int nchunk, int nlag, int npairs,
                                                             double lambdaLag, real *__restrict__ theta) {
    __shared__ real sm[N * (N + 1) / 2 + N];
    const int t = blockIdx.x, lane = threadIdx.x;
    for (int p = threadIdx.x; p < npairs; p += 256) sm[p] = (real)theta_sum_pair_wide(part, nchunk, npairs, t, p);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    real col[N];
#pragma unroll
    for (int s = 0; s < N; s++) {
        real v = real(0);
        if (s < nlag && lane < nlag) {
            const int a = min(s, lane), b = max(s, lane);
            v = sm[nlag + a * nlag - a * (a - 1) / 2 + (b - a)];
            if (s == lane) v = (real)((double)v + lambdaLag);
        }
        col[s] = v;
    }
    const real yv = lane < nlag ? sm[lane] : real(0);
    const real x = theta_chol_solve_reg<real, N>(col, yv, nlag, lane);
    if (lane < nlag) theta[(size_t)t * nlag + lane] = x;
}

// ---- sparse lag weights: L1-penalised Theta-solve (the reference's MATLAB trainer, do_lasso; no counterpart in trmf.cpp) ----------
//   theta_t = argmin 1/2 th^T G_t th - b_t^T th + 1/2 lambdaLag |th|^2 + lambdaL1 |th|_1
// by cyclic coordinate descent with covariance updates, warm-started from the session's current Theta, then (refit != 0) the ridge
// solution on the support the lasso selected.  Everything in fp64 in both libraries; Theta is rounded to `real` on the final store.
#if defined(TRMF_F32)
constexpr double kLassoEps = 1e-7;       // a sweep that moves no coordinate by more than kLassoEps * max(1, |theta|_inf) is the last
#else
constexpr double kLassoEps = 1e-13;      // (1e-10 would leave Theta ~cond * 1e-10 from the minimiser: above the fp64 Cholesky's own error in the ridge limit)
#endif
constexpr int kLassoMaxSweeps = 1000;    // a dimension that gets here keeps its iterate and is counted (TrmfLagStats: capped)
constexpr int kLagRec = 4;               // per-dimension record: sweeps, non-zeros, hit the cap, refit skipped
__host__ __device__ inline size_t theta_lasso_doubles(int nlag) { return (size_t)nlag * nlag + 3 * (size_t)nlag; }   // G, b, r, theta

__device__ __forceinline__ double lasso_soft(double rho, double l1) { return rho > l1 ? rho - l1 : rho < -l1 ? rho + l1 : 0.0; }

// grid k, 256 threads, dynamic LDS = theta_lasso_doubles(nlag) * 8, or (GLOB) 0 and `scratch` of that many doubles per latent dimension.
// All threads sum the chunk partials (theta_sum_pair) into the full symmetric G, into b, and form r = b - G theta; one wavefront
// does the sweeps -- LDS accesses of one wavefront retire in program order; on global scratch the (then wave-local) workgroup
// barrier orders them, as in theta_chol_solve.  Per coordinate j, ascending: rho = r_j + G_jj th_j, th_j' = soft(rho, l1) / (G_jj +
// lambdaLag) (0 where that denominator is not positive and finite), r -= (th_j' - th_j) G[j, :] -- row j is column j, contiguous.
// A fixed order of operations, no atomics: the same bits every time.
// GLOB: the two forms are two instantiations, so that the LDS form addresses LDS as LDS (not through generic pointers).
template <bool GLOB>
__global__ __launch_bounds__(256) void theta_lasso_kernel(const double *__restrict__ part, int nchunk, int nlag, int npairs,
                                                         double lambdaLag, double lambdaL1, int refit, real *__restrict__ theta,
                                                         double *__restrict__ scratch, int *__restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr bool glob = GLOB;
    double *G = GLOB ? scratch + (size_t)blockIdx.x * theta_lasso_doubles(nlag) : reinterpret_cast<double *>(smem_raw);
    double *b = G + (size_t)nlag * nlag, *r = b + nlag, *th = r + nlag;
    const int t = blockIdx.x, lane = threadIdx.x;
    for (int p = threadIdx.x; p < npairs; p += 256) {
        const double acc = theta_sum_pair(part, nchunk, npairs, t, p);
        int a, c; bool rhs;
        theta_decode_pair(p, nlag, a, c, rhs);
        if (rhs) b[a] = acc;
        else { G[a * nlag + c] = acc; G[c * nlag + a] = acc; }
    }
    for (int i = threadIdx.x; i < nlag; i += 256) {
        const double v = (double)theta[(size_t)t * nlag + i];
        th[i] = isfinite(v) ? v : 0.0;                  // (a warm start that is not a number is no warm start)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nlag; i += 256) {
        double acc = b[i];
        for (int j = 0; j < nlag; j++) acc -= G[j * nlag + i] * th[j];      // column i = row i; ascending j
        r[i] = acc;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;                      // the barriers below only count the wavefront that is left
    int sweeps = 0, capped = 0;
    for (;;) {
        double dmax = 0, tmax = 0;
        for (int j = 0; j < nlag; j++) {
            const double gjj = G[j * nlag + j], thj = th[j], den = gjj + lambdaLag;
            double tn = (den > 0 && isfinite(den)) ? lasso_soft(r[j] + gjj * thj, lambdaL1) / den : 0.0;
            if (!isfinite(tn)) tn = 0.0;
            const double delta = tn - thj;
            // No barrier in the LDS form: besides the in-order retirement of one wavefront's LDS accesses this needs the compiler to
            // keep program order between the lanes' stores to r[] / th[] and the next coordinate's loads of r[j + 1], th[j + 1] -- it
            // does, because they go through the same may-aliasing pointers.  Do not mark r / th / G __restrict__ or cache them in
            // registers across coordinates.
            if (delta != 0) {                           // (uniform: every lane has read the same three values)
                if (glob) __syncthreads();              // ... before any lane overwrites r[j]
                for (int i = lane; i < nlag; i += 64) r[i] -= delta * G[j * nlag + i];
                if (lane == 0) th[j] = tn;
                if (glob) __syncthreads();
            }
            dmax = fmax(dmax, fabs(delta)); tmax = fmax(tmax, fabs(tn));
        }
        sweeps++;
        if (dmax <= kLassoEps * fmax(1.0, tmax)) break;
        if (sweeps >= kLassoMaxSweeps) { capped = 1; break; }
    }
    // the support is what survives the rounding to the element type (so that the record, the refit and the stored Theta agree)
    int *idx = reinterpret_cast<int *>(r);              // r is no longer needed: ascending indices of the support
    int m = 0;
    __syncthreads();
    for (int base = 0; base < nlag; base += 64) {
        const bool on = base + lane < nlag && (real)th[base + lane] != real(0);
        const unsigned long long mask = __ballot(on);
        if (on) idx[m + __popcll(mask & ((1ull << lane) - 1ull))] = base + lane;
        m += __popcll(mask);
    }
    __syncthreads();
    int skipped = 0;
    if (refit && m > 0) {
        // G_SS + lambdaLag I and b_S compacted in place: target (p, q) of the m x m system lies at or before its source
        // (idx[p] >= p, idx[q] >= q, m <= nlag) and strictly before the source of every later target, so 64 targets at a time --
        // all read, then all written -- never overwrite an entry that is still to be read
        for (int base = 0; base < m * m; base += 64) {
            const int o = base + lane, p = o / m, q = o - p * m;
            double v = 0;
            if (o < m * m) v = G[idx[p] * nlag + idx[q]] + (p == q ? lambdaLag : 0.0);
            __syncthreads();
            if (o < m * m) G[o] = v;
            __syncthreads();
        }
        for (int base = 0; base < m; base += 64) {
            const int p = base + lane;
            double v = 0;
            if (p < m) v = b[idx[p]];
            __syncthreads();
            if (p < m) b[p] = v;
            __syncthreads();
        }
        bool ok = theta_chol_solve<double, true>(G, b, m, lane);
        __syncthreads();
        if (ok)
            for (int base = 0; base < m; base += 64)
                if (__ballot(base + lane < m && !isfinite(b[base + lane]))) ok = false;
        if (ok) { for (int p = lane; p < m; p += 64) th[idx[p]] = b[p]; }
        else skipped = 1;                               // the lasso's own solution stays
        __syncthreads();
    }
    int nnz = 0;
    for (int base = 0; base < nlag; base += 64) {
        const int a = base + lane;
        real v = real(0);
        if (a < nlag) {
            v = (real)th[a];
            if (v == real(0)) v = real(0);              // exact +0 off the support
            theta[(size_t)t * nlag + a] = v;
        }
        nnz += __popcll(__ballot(a < nlag && v != real(0)));
    }
    if (lane < kLagRec) rec[t * kLagRec + lane] = lane == 0 ? sweeps : lane == 1 ? nnz : lane == 2 ? capped : skipped;
}

}  // namespace trmf
