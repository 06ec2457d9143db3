// forecast_kernels.hpp -- the next `steps` timestamps of a resident model (trmf_session_forecast): the forecasting protocol of
// the paper rolls W forward by the AR model, multiplies by H and scores the result against the truth.
//
//   forecast_rollout_kernel     Wnew[i][t] = sum_l W[i - L_l][t] * Theta(l, t), i = T .. T+steps-1 (Model.latent_forecast)
//   forecast_score_kernel<NT>   y = Wnew[i] . H[j] (+ clip, + inverse series transform), the forecast if asked for, and the six
//                               fp64 sums of TrmfSeriesSums per series if a truth is given
//
// Roll-out: latent dimensions are independent, one thread per dimension in ceil(k / 64) workgroups of one wavefront; the only
// serial chain is over the rows.  A row reaches back at most `reach` = max lag rows, so the last `reach` rows of the thread's
// column live in a ring in LDS (row i in slot i mod reach; the slot a new row overwrites holds the row that has just gone out of
// reach), next to the lags and the workgroup's columns of Theta: the chain runs at LDS latency.  Where that does not fit the LDS
// budget everything is read from global memory -- the history from W, new rows from the output, which the same thread wrote.
// Arithmetic of latent_forecast_kernel (resident_kernels.hpp): products rounded to the element type, summed in ascending lag
// order, no contraction.
//
// Scoring: one series per thread, consecutive series on consecutive lanes, so truth[i][.] and Ynew[i][.] (row-major steps x n)
// are coalesced.  The rolled rows sit in LDS in the column-interleaved layout and are read as broadcasts: the dot product is
// invariant under the common permutation and the pads are zero on both sides.  For k <= 64 the thread's H row stays in
// registers; the generic form walks it in slices of 16 for a few rows at a time.  Each series belongs to one thread for a whole
// call: no atomics, a fixed order, the same bits every time.  The table is read from one buffer and written to another, so the
// host publishes a call's sums only once everything has succeeded.
#pragma once

#include "common.hpp"

namespace trmf {

constexpr int kFcSums = 6;             // abs_err, sq_err, abs_truth, abs_dtruth, rel_err, count_nonzero (TrmfSeriesSums order)
constexpr int kFcLdsReals = 6144;      // rolled rows held in LDS per pass of the score kernel (24 KB fp32 / 48 KB fp64)
constexpr int kFcGenRows = 6;          // rows per pass of the generic form: 6 x 1024 reals

struct RolloutArgs {
    const real *W;                     // the session's W: T rows of KP reals
    real *roll;                        // steps rows of KP reals, column-interleaved (the pads are the caller's: zero)
    real *flat;                        // nullptr, or steps x k row-major
    const uint32_t *lag_set;
    const real *theta;                 // Theta(l, t) at t * nlag + l
    int T, steps, KP, NT, k, nlag;
    int reach;                         // ring rows in LDS (the largest lag, at most T), 0: the form that reads global memory
};

struct ScoreArgs {
    const real *H;                     // n rows of KP reals
    const real *roll;                  // steps rows of KP reals
    const real *truth;                 // nullptr, or steps x n row-major
    real *Y;                           // nullptr, or steps x n row-major
    const real *tr_a, *tr_b;           // nullptr, or the series transform y -> a y + b that is undone
    const double *table_in;            // n x kFcSums
    double *table_out;
    const real *prev_in;               // the last truth row of the previous scored call
    real *prev_out;
    real threshold;
    int clip, have_prev;
    int n, steps, KP, NT, rows_per_pass;
};

// LDS of the roll-out's LDS form: the lags, 64 columns of Theta, the ring of `reach` rows of 64 columns
__host__ __device__ inline size_t rollout_lag_bytes(int nlag) { return ((size_t)nlag * sizeof(int) + 15) / 16 * 16; }
inline size_t rollout_lds_bytes(int nlag, int reach) { return rollout_lag_bytes(nlag) + ((size_t)nlag + reach) * 64 * sizeof(real); }
inline int forecast_rows_per_pass(int KP, bool generic) { return generic ? kFcGenRows : kFcLdsReals / KP; }

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
__global__ void forecast_rollout_kernel(RolloutArgs a);
template <int NT>
__global__ void forecast_score_kernel(ScoreArgs a);
#else
__global__ __launch_bounds__(64) void forecast_rollout_kernel(RolloutArgs a) {
#pragma clang fp contract(off)      // product and sum are rounded separately, like the NumPy expression (hipcc contracts by default)
    extern __shared__ __align__(16) unsigned char fc_lds_raw[];
    const int c = threadIdx.x, t = blockIdx.x * 64 + c, R = a.reach;
    const bool on = t < a.k;
    const int tp = colpos(on ? t : 0, a.NT);
    if (R > 0) {
        // LDS form: the lags, this workgroup's 64 columns of Theta (lag-major) and the ring of the last R rows; the inner loop
        // touches LDS only, and its iterations depend on each other through the running sum alone
        int *lag = reinterpret_cast<int *>(fc_lds_raw);
        real *th = reinterpret_cast<real *>(fc_lds_raw + rollout_lag_bytes(a.nlag));
        real *ring = th + (size_t)a.nlag * 64;
        for (int l = c; l < a.nlag; l += 64) lag[l] = (int)a.lag_set[l];
        for (int l = 0; l < a.nlag; l++) th[l * 64 + c] = on ? a.theta[(size_t)t * a.nlag + l] : real(0);
        int base = a.T % R;                                     // slot of row T (and of row T - R, which it replaces)
        for (int r = 0, slot = base; r < R; r++) {
            ring[slot * 64 + c] = on ? a.W[(size_t)(a.T - R + r) * a.KP + tp] : real(0);
            slot = slot + 1 == R ? 0 : slot + 1;
        }
        __syncthreads();                                        // the lags are shared; everything else is the thread's own
        for (int s = 0; s < a.steps; s++) {
            real acc = 0;
#pragma unroll 8
            for (int l = 0; l < a.nlag; l++) {
                const int lg = lag[l];                          // 0 <= lg <= R
                int slot = base - lg;
                slot += slot < 0 ? R : 0;
                const real w = lg > 0 ? ring[slot * 64 + c] : real(0);     // (lag 0 reads the row being formed: zero so far)
                const real prod = w * th[l * 64 + c];
                acc = acc + prod;
            }
            ring[base * 64 + c] = acc;
            base = base + 1 == R ? 0 : base + 1;
            if (on) {
                a.roll[(size_t)s * a.KP + tp] = acc;
                if (a.flat) a.flat[(size_t)s * a.k + t] = acc;
            }
        }
        return;
    }
    if (!on) return;
    const real *th = a.theta + (size_t)t * a.nlag;
    for (int s = 0; s < a.steps; s++) {
        const int i = a.T + s;
        real acc = 0;
        for (int l = 0; l < a.nlag; l++) {
            const int src = i - (int)a.lag_set[l];
            real w = 0;
            if (src >= 0) w = src >= a.T ? a.roll[(size_t)(src - a.T) * a.KP + tp] : a.W[(size_t)src * a.KP + tp];
            const real prod = w * th[l];
            acc = acc + prod;
        }
        a.roll[(size_t)s * a.KP + tp] = acc;
        if (a.flat) a.flat[(size_t)s * a.k + t] = acc;
    }
}

// one forecast value -> the thread's running sums
struct FcSums {
    double abs_err = 0, sq_err = 0, abs_truth = 0, abs_dtruth = 0, rel_err = 0, count_nonzero = 0;
};

// clip, inverse transform, store, score: what every form does with a finished dot product
__device__ __forceinline__ void forecast_finish(const ScoreArgs &a, int j, int i, real y, real ta, real tb, bool tr, FcSums &s, real &yprev, bool &have) {
#pragma clang fp contract(off)      // (y - b) / a with both operations rounded, like NormalizedTransform.postprocess
    if (a.clip) y = y < a.threshold ? a.threshold : y;
    if (tr) {
        const real d = y - tb;
        y = d / ta;
    }
    const size_t e = (size_t)i * a.n + j;
    if (a.Y) a.Y[e] = y;
    if (a.truth) {
        const real tv = a.truth[e];
        const double yt = (double)tv, err = (double)y - yt, ae = fabs(err), at = fabs(yt);
        s.abs_err += ae; s.sq_err += err * err; s.abs_truth += at;
        if (have) s.abs_dtruth += fabs(yt - (double)yprev);
        if (yt != 0) { s.rel_err += ae / at; s.count_nonzero += 1.0; }
        yprev = tv; have = true;
    }
}

// NT = 1..4: k <= 64 (KP = 16 NT); NT = 0: 64 < k <= 1024
template <int NT>
__global__ __launch_bounds__(256) void forecast_score_kernel(ScoreArgs a) {
    __shared__ __align__(16) real sw[kFcLdsReals];
    const int j0 = blockIdx.x * 256 + threadIdx.x;
    const bool on = j0 < a.n;
    const int j = on ? j0 : a.n - 1;                            // idle lanes of the last workgroup follow along and store nothing
    const int KP = NT > 0 ? kTile * NT : a.KP;
    const real *hrow = a.H + (size_t)j * KP;
    const bool tr = a.tr_a != nullptr;
    const real ta = tr ? a.tr_a[j] : real(1), tb = tr ? a.tr_b[j] : real(0);
    FcSums s;
    real yprev = (a.truth && a.have_prev) ? a.prev_in[j] : real(0);
    bool have = a.have_prev != 0;

    constexpr int NH = NT > 0 ? kTile * NT : kTile;
    real h[NH];
    if constexpr (NT > 0) {
#pragma unroll
        for (int q = 0; q < NH / 4; q++) {
            const Quad<real> v = reinterpret_cast<const Quad<real> *>(hrow)[q];
#pragma unroll
            for (int u = 0; u < 4; u++) h[4 * q + u] = v.v[u];
        }
    }
    for (int r0 = 0; r0 < a.steps; r0 += a.rows_per_pass) {
        const int rows = a.steps - r0 < a.rows_per_pass ? a.steps - r0 : a.rows_per_pass;
        __syncthreads();                                        // the previous pass has been read
        for (int e = threadIdx.x; e < rows * KP; e += 256) sw[e] = a.roll[(size_t)r0 * KP + e];
        __syncthreads();
        if constexpr (NT > 0) {
            for (int r = 0; r < rows; r++) {
                const real *w = sw + r * KP;
                real d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
                for (int q = 0; q < NH / 4; q++) {
                    const Quad<real> v = reinterpret_cast<const Quad<real> *>(w)[q];       // every lane reads the same address
                    d0 = fma(h[4 * q], v.v[0], d0); d1 = fma(h[4 * q + 1], v.v[1], d1);
                    d2 = fma(h[4 * q + 2], v.v[2], d2); d3 = fma(h[4 * q + 3], v.v[3], d3);
                }
                const real y = (d0 + d1) + (d2 + d3);
                if (on) forecast_finish(a, j, r0 + r, y, ta, tb, tr, s, yprev, have);
            }
        } else {
            real d[kFcGenRows];
#pragma unroll
            for (int r = 0; r < kFcGenRows; r++) d[r] = 0;
            for (int p = 0; p < KP; p += kTile) {
#pragma unroll
                for (int q = 0; q < kTile / 4; q++) {
                    const Quad<real> v = reinterpret_cast<const Quad<real> *>(hrow + p)[q];
#pragma unroll
                    for (int u = 0; u < 4; u++) h[4 * q + u] = v.v[u];
                }
#pragma unroll
                for (int r = 0; r < kFcGenRows; r++) {
                    if (r < rows) {
                        const real *w = sw + r * KP + p;
#pragma unroll
                        for (int q = 0; q < kTile; q++) d[r] = fma(h[q], w[q], d[r]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < kFcGenRows; r++)
                if (r < rows && on) forecast_finish(a, j, r0 + r, d[r], ta, tb, tr, s, yprev, have);
        }
    }
    if (on && a.truth) {
        const double *ti = a.table_in + (size_t)j * kFcSums;
        double *to = a.table_out + (size_t)j * kFcSums;
        to[0] = ti[0] + s.abs_err; to[1] = ti[1] + s.sq_err; to[2] = ti[2] + s.abs_truth;
        to[3] = ti[3] + s.abs_dtruth; to[4] = ti[4] + s.rel_err; to[5] = ti[5] + s.count_nonzero;
        a.prev_out[j] = yprev;
    }
}
#endif

}  // namespace trmf
