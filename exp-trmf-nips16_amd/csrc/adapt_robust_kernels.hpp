// adapt_robust_kernels.hpp -- robust online loading updates (trmf_session_adapt_series_robust): adapt_series with Huber weights on
// the entries not yet absorbed, the last cell of the {W, H} x {plain, robust} table of the online features.  Sparse storage with
// missing != 0 only (per-series tables).  Per series j, with d = gamma^m, om_t = gamma^(rows - 1 - t), tau_j = c scale_j and
// h^0 = H[j]:
//
//     for s = 1 .. sweeps:   res_e = y_e - w_t . h^{s-1},   u_e = 1 if |res_e| <= tau_j else tau_j / |res_e|      (e over the tail)
//                            S^s = d S_j + sum_e (u_e om_t) w_t w_t^T,   r^s = d r_j + sum_e (u_e om_t) y_e w_t     (stored order)
//                            h^s = (S^s + lambdaI I)^-1 r^s
//
// Every sweep restarts from the decayed OLD tables; only the new entries are reweighted.  The last sweep's tables, h and u_e are
// the result.  No floating-point atomics; every sum has a fixed order.
//
//   adapt_robust_series_kernel<NT>   adapt_series_kernel's shape: one wavefront (one 64-thread workgroup) per series, lane c holding
//                                    column c of S_j in registers.  Per sweep the packed tables are reloaded times d (the
//                                    factorisation destroyed the registers; a coalesced read that is hot in L2), the tail is
//                                    walked in batches of 64 entries with the rows of W gathered four at a time, and each entry's
//                                    residual is formed by a FIXED 64-LANE BUTTERFLY of w_c h_c (lane c holds h_c from the sweep
//                                    before; idle lanes add 0) whose result is then broadcast from lane 0, so every lane forms the
//                                    same weight from the same bits -- the rows gathered for the rank-1 update are reused, no
//                                    second pass over W and no LDS for h.  The update is adapt_rank1 with om replaced by u om; the
//                                    ridge, the factorisation and the substitutions are adapt_factor_solve, the code adapt_series_kernel
//                                    runs, so with c = inf (u = 1 exactly) the two kernels execute the same operations in the same order.
//                                    The last sweep stores the tables of the inactive generation and the weights at
//                                    wptr[j] + position in the tail.  A series without a new entry runs one sweep.
//   adapt_robust_objective_kernel    J_j(h) = h^T (d S_j + lambdaI I) h - 2 h . (d r_j) + sum_e om_t rho_tau(y_e - w_t . h) per series
//                                    in fp64, for the old and for the new H: one wavefront per series, fixed orders.  Not hot.
#pragma once

#include "adapt_kernels.hpp"

namespace trmf {

constexpr int kAdaptRobustMaxSweeps = 64;

struct AdaptRobustArgs {
    const uint32_t *ptr, *idx;         // CSC of the training matrix: column j at [ptr[j], ptr[j + 1]), idx = the timestamp
    const real *val;
    const uint32_t *start;             // per series: the first entry not yet absorbed
    const real *W;                     // rows x KP, column-interleaved
    const real *omega;                 // weight of timestamp t at omega[t - row0]; nullptr: 1 (gamma == 1)
    const real *Sin, *rin;             // the active generation (n x packed, n x k)
    real *Sout, *rout;                 // the inactive generation
    const real *Hold;                  // the session's H (n x KP, column-interleaved)
    real *Hnew;                        // scratch of the same shape (the pads are the caller's: zero)
    real *change;                      // per series: max_c |h_new - h_old|
    int *flag;
    const real *thr;                   // per series: tau_j = c scale_j in the element type (inf: every weight 1)
    const uint32_t *wptr;              // n + 1: the weights of series j at [wptr[j], wptr[j + 1]) (= its tail, in stored order)
    real *weights;                     // the last sweep's u_e
    uint32_t *wrows;                   // the timestamp of each of them
    double *obj;                       // adapt_robust_objective_kernel: 2 n values, J_j at Hold then at Hnew
    real decay, lam;                   // gamma^m; lambdaI
    int row0, n, k, KP, NT, sweeps;
};

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
template <int NT>
__global__ void adapt_robust_series_kernel(AdaptRobustArgs a);
__global__ void adapt_robust_objective_kernel(AdaptRobustArgs a);
#else
// adapt_walk with a weight per entry.  h: lane c's component of the loadings the residuals are formed against (0 on idle lanes).
// The dot product of an entry is a butterfly over all 64 lanes in a fixed order, broadcast from lane 0.
template <int KMAX>
__device__ __forceinline__ void adapt_robust_walk(const AdaptRobustArgs &a, uint32_t e0, uint32_t e1, int c, int cp, bool on, real h, real tau,
                                                  bool last, uint32_t wpos, real (&col)[KMAX], real &rr) {
    for (uint32_t base = e0; base < e1; base += 64u) {
        const uint32_t e = base + (uint32_t)c;
        const bool valid = e < e1;
        const int t = valid ? (int)a.idx[e] : a.row0;
        const real y = valid ? a.val[e] : real(0);
        const real om = valid ? (a.omega ? a.omega[max(t - a.row0, 0)] : real(1)) : real(0);
        const int cnt = (int)min(64u, e1 - base);
        real ul = 1;                                                     // lane l: the weight of entry base + l
        for (int g = 0; g < cnt; g += 4) {
            real w[4], oy[4], oo[4], dot[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int l = min(g + q, cnt - 1);                       // (a short last group repeats its last entry with weight 0)
                const int tq = adapt_bcast(t, l);
                const real wq = a.W[(size_t)tq * a.KP + cp];
                w[q] = on ? wq : real(0);
                oy[q] = adapt_bcast(y, l);
                oo[q] = g + q < cnt ? adapt_bcast(om, l) : real(0);
                dot[q] = w[q] * h;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
                for (int q = 0; q < 4; q++) dot[q] += __shfl_xor(dot[q], o, kWave);
            }
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (g + q < cnt) {
                    const real ar = fabs(oy[q] - adapt_bcast(dot[q], 0));
                    const real u = ar <= tau ? real(1) : tau / ar;
                    if (c == g + q) ul = u;
                    adapt_rank1<KMAX>(col, rr, w[q], u * oo[q], oy[q]);
                }
        }
        if (last && valid) {
            a.weights[wpos + (e - e0)] = ul;
            a.wrows[wpos + (e - e0)] = (uint32_t)t;
        }
    }
}

template <int NT>
__global__ __launch_bounds__(64) void adapt_robust_series_kernel(AdaptRobustArgs a) {
    constexpr int KMAX = kTile * NT, SP = KMAX + 1;         // odd pitch: column reads spread over the banks
    __shared__ real Us[KMAX * SP];
    const int c = threadIdx.x, k = a.k;
    const int j = blockIdx.x;
    if (j >= a.n) return;
    const bool on = c < k;
    const int t = on ? c : k - 1;                           // idle lanes shadow the last unknown and store nothing
    const int cp = colpos(t, NT);
    const size_t PK = adapt_packed(k);
    const uint32_t e0 = a.start[j], e1 = a.ptr[j + 1];
    const int nsw = e1 > e0 ? a.sweeps : 1;                 // nothing to reweight: every sweep would repeat the first
    const real tau = a.thr[j];
    const uint32_t wpos = a.wptr[j];
    const real *Sj = a.Sin + (size_t)j * PK;
    const real hold = on ? a.Hold[(size_t)j * a.KP + cp] : real(0);
    real x = hold;
    bool bad = false;
    for (int sw = 1; sw <= nsw; sw++) {
        real col[KMAX], rr = 0;
#pragma unroll
        for (int s = 0; s < KMAX; s++) col[s] = 0;
#pragma unroll
        for (int s = 0; s < KMAX; s++)
            if (on && s <= c) col[s] = a.decay * Sj[s * k - s * (s - 1) / 2 + c - s];
        if (on) rr = a.decay * a.rin[(size_t)j * k + c];
        adapt_robust_walk<KMAX>(a, e0, e1, c, cp, on, x, tau, sw == nsw, wpos, col, rr);
        if (on && sw == nsw) {
            real *So = a.Sout + (size_t)j * PK;
#pragma unroll
            for (int s = 0; s < KMAX; s++)
                if (s <= c) So[s * k - s * (s - 1) / 2 + c - s] = col[s];
            a.rout[(size_t)j * k + c] = rr;
        }
        x = adapt_factor_solve<KMAX>(col, rr, a.lam, on, c, t, k, Us, bad);
        x = on ? x : real(0);
        __syncthreads();                                    // the next sweep writes the factor the substitutions have just read
    }
    if (bad && c == 0) atomicMin(a.flag, j);
    real d = 0;
    if (on) {
        d = fabs(x - hold);
        a.Hnew[(size_t)j * a.KP + cp] = x;
    }
    d = adapt_wave_max(d);
    if (c == 0) a.change[j] = d;
}

// fp64 sum over the 64 lanes in a fixed order; every lane gets lane 0's bits
__device__ __forceinline__ double adapt_robust_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return adapt_bcast(v, 0);
}

// J_j at Hold (obj[2 j]) and at Hnew (obj[2 j + 1]): lane c forms h_c (sum_s (d S)(s, c) h_s + lambdaI h_c - 2 d r_c), lane l the
// Huber terms of the tail entries l, l + 64, ...; the decayed tables are rounded to the element type as the update reads them
__global__ __launch_bounds__(64) void adapt_robust_objective_kernel(AdaptRobustArgs a) {
    __shared__ double hs[2][kMaxRank];                      // the series' row of Hold, of Hnew: the tables and W are read once for both
    const int c = threadIdx.x, k = a.k;
    const int j = blockIdx.x;
    if (j >= a.n) return;
    const bool on = c < k;
    const size_t PK = adapt_packed(k);
    const real *Sj = a.Sin + (size_t)j * PK;
    const double tau = (double)a.thr[j];
    if (on) {
        hs[0][c] = (double)a.Hold[(size_t)j * a.KP + colpos(c, a.NT)];
        hs[1][c] = (double)a.Hnew[(size_t)j * a.KP + colpos(c, a.NT)];
    }
    __syncthreads();
    double quad[2] = {0, 0}, rho[2] = {0, 0};
    if (on) {
        double acc[2] = {0, 0};
        for (int s = 0; s < k; s++) {
            const int lo = min(s, c), hi = max(s, c);
            const double ds = (double)(a.decay * Sj[lo * k - lo * (lo - 1) / 2 + hi - lo]);
            acc[0] += ds * hs[0][s];
            acc[1] += ds * hs[1][s];
        }
        const double dr = (double)(a.decay * a.rin[(size_t)j * k + c]);
        for (int v = 0; v < 2; v++) quad[v] = hs[v][c] * (acc[v] + (double)a.lam * hs[v][c] - 2.0 * dr);
    }
    for (uint32_t e = a.start[j] + (uint32_t)c; e < a.ptr[j + 1]; e += 64u) {
        const int t = (int)a.idx[e];
        const real *w = a.W + (size_t)t * a.KP;
        double p[2] = {0, 0};
        for (int s = 0; s < k; s++) {
            const double ws = (double)w[colpos(s, a.NT)];
            p[0] += ws * hs[0][s];
            p[1] += ws * hs[1][s];
        }
        const double y = (double)a.val[e];
        const double om = a.omega ? (double)a.omega[max(t - a.row0, 0)] : 1.0;
        for (int v = 0; v < 2; v++) {
            const double ar = fabs(y - p[v]);
            rho[v] += om * (ar <= tau ? ar * ar : 2.0 * tau * ar - tau * tau);
        }
    }
    for (int v = 0; v < 2; v++) {
        const double total = adapt_robust_wave_sum(quad[v]) + adapt_robust_wave_sum(rho[v]);
        if (c == 0) a.obj[2 * j + v] = total;
    }
}
#endif

}  // namespace trmf
