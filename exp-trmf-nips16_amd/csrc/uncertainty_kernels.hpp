// uncertainty_kernels.hpp -- the predictive distribution of a forecast (trmf_session_fit_noise / _forecast_dist): TRMF read as a
// linear-Gaussian state-space model, y_ij = w_i . h_j + eps, every latent dimension an AR process.  The NumPy statement is
// trmf/uncertainty.py; all variance arithmetic is fp64.
//
//   noise_resid_kernel<NT>      per work item (a fixed chunk of one series' entries), the count and the fp64 sum of
//                               (y - w_i . h_j)^2: the F-solve's stream without the factorisation
//   noise_series_kernel         the items of a series added in ascending item order -> (sq_j, cnt_j)
//   noise_pool_kernel           the pooled sum in series order, then sigma2_j = sq_j / cnt_j (or the pooled value)
//   noise_innov_kernel          per (latent dimension, chunk of time) the fp64 sum of (w_i[d] - p_i[d])^2, p_i formed as
//                               forecast_rollout_kernel forms it;  noise_q_kernel adds the chunks in ascending order
//   forecast_psi_kernel         the impulse response psi_d of every dimension as an fp64 chain over the steps, and
//                               v_d[s] = q_d sum_{u <= s} psi_d[u]^2
//   forecast_dist_kernel<NT>    mean (the bits of forecast_score_kernel), V = sigma2_j + sum_d H[j][d]^2 v_d[s], the standard
//                               deviation, and -- with a truth -- the seven fp64 sums of TrmfIntervalSums per series
//
// A PLUG-IN interval: the estimation error of H, Theta and the last rows of W is ignored and the residuals are in-sample.
//
// Residual pass.  A series' entries are cut into chunks of a fixed length and a chunk is one wavefront's work item (the split
// path's item lists, gram_kernels.hpp): the 370 x 26 304 panel would otherwise put 21 000 entries on each of 370 wavefronts.
// Within an item lane c = lane & 15 owns the NT column slices of h_j (heldout_eval_kernel's scheme: one vector load of the
// column-interleaved row serves a lane); the four 16-lane groups take entries 4 it + g and gather the W row slice.  Each group
// reduces its dot product over its 16 lanes by a fixed butterfly and accumulates e^2 in entry order; the four group sums are
// added as (g0 + g1) + (g2 + g3).  No atomics: the chunk length and these orders are the contract, the same bits on every call
// and on every rank.  An item's kind says where y comes from:
//     kNzStored    stored entries of the item-major CSR: (y - p)^2
//     kNzDense     positions of the dense n x T orientation (index = position): (y - p)^2
//     kNzZero      every timestamp with y = 0 (sparse storage, missing == 0): p^2
//     kNzCorrect   the stored entries on top of kNzZero: (y - p)^2 - p^2 = y (y - 2 p)   (assim_err_kernel's identity)
#pragma once

#include "common.hpp"

namespace trmf {

constexpr int kIvSums = 7;             // cells, covered, sd_sum, abs_truth, z2_sum, nll_sum, crps_sum (TrmfIntervalSums order)
constexpr int kFdLdsReals = 2048;      // rolled rows (and as many doubles of v) held in LDS per pass of the dist kernel
constexpr int kFdGenRows = 2;          // rows per pass of the generic form: 2 x 1024
constexpr int kNzChunk = 1024;         // entries per item of the residual pass
constexpr int kNzBatch = 4;            // entries of a 16-lane group in flight at a time
constexpr int kNzInnovChunk = 32;      // timestamps per chunk of the innovation pass (a chunk is one wavefront's chain of rows x lags loads)
enum { kNzStored = 0, kNzDense = 1, kNzZero = 2, kNzCorrect = 3 };

struct NoiseItem { uint32_t series, begin, end, kind; };

struct NoiseResidArgs {
    const NoiseItem *items;
    uint32_t nitems;
    const uint32_t *idx;               // item-major CSR: timestamp of every stored entry (kNzStored / kNzCorrect)
    const real *val;                   // ... and its value
    const real *Ynt;                   // dense n x T row-major training matrix (kNzDense)
    const real *W, *H;
    double *part;                      // per item: sq at [2 e], the counted cells at [2 e + 1]
    int T, KP, NT;
};

struct NoiseInnovArgs {
    const real *W;
    const uint32_t *lag_set;
    const real *theta;                 // Theta(l, t) at t * nlag + l
    double *part;                      // nchunks x k
    int T, m, k, KP, NT, nlag;
    int lds;                           // lags and the workgroup's Theta columns staged in LDS
};

struct PsiArgs {
    const uint32_t *lag_set;
    const real *theta;
    const double *q;
    double *v;                         // steps x KP, column-interleaved (the pads are the caller's: zero)
    double *psi_glob;                  // steps x k scratch of the global-memory form
    int *flag;                         // raised when a v is not finite
    int steps, k, KP, NT, nlag;
    int reach;                         // ring entries in LDS (the largest lag), 0: the form that reads global memory
};

struct DistArgs {
    const real *H;
    const real *roll;                  // steps rows of KP reals
    const double *v;                   // steps rows of KP doubles
    const double *sigma2;              // n
    const real *truth;                 // nullptr, or steps x n row-major
    real *Y, *Ysd;                     // nullptr, or steps x n row-major
    const real *tr_a, *tr_b;
    const double *table_in;            // n x kIvSums
    double *table_out;
    real threshold;
    double zq;
    int clip;
    int n, steps, KP, NT, rows_per_pass;
};

__host__ __device__ inline size_t nz_lag_bytes(int nlag) { return ((size_t)nlag * sizeof(int) + 15) / 16 * 16; }
inline size_t innov_lds_bytes(int nlag) { return nz_lag_bytes(nlag) + (size_t)nlag * 64 * sizeof(real); }
__host__ __device__ inline size_t psi_theta_bytes(int nlag) { return ((size_t)nlag * 64 * sizeof(real) + 15) / 16 * 16; }
inline size_t psi_lds_bytes(int nlag, int reach) { return nz_lag_bytes(nlag) + psi_theta_bytes(nlag) + (size_t)reach * 64 * sizeof(double); }
inline int dist_rows_per_pass(int KP, bool generic) { return generic ? kFdGenRows : kFdLdsReals / KP; }

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
template <int NT>
__global__ void noise_resid_kernel(NoiseResidArgs a);
__global__ void noise_series_kernel(const double *part, const uint32_t *first, int n, double *sq, double *cnt);
__global__ void noise_pool_kernel(const double *sq, const double *cnt, int n, double *sigma2, double *pooled);
__global__ void noise_innov_kernel(NoiseInnovArgs a);
__global__ void noise_q_kernel(const double *part, int nchunks, int k, double denom, double *q);
__global__ void forecast_psi_kernel(PsiArgs a);
template <int NT>
__global__ void forecast_dist_kernel(DistArgs a);
#else
// NT = 1..4: k <= 64 (KP = 16 NT), the lane's slice of h_j in registers; NT = 0: 64 < k <= 1024, slices of a.NT read per entry
template <int NT>
__global__ __launch_bounds__(256) void noise_resid_kernel(NoiseResidArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const uint32_t item = blockIdx.x * 4u + (uint32_t)wave;
    if (item >= a.nitems) return;                             // wave-uniform; no block barrier below
    const NoiseItem it = a.items[item];
    const int nt = NT > 0 ? NT : a.NT;
    const size_t KP = NT > 0 ? (size_t)kTile * NT : (size_t)a.KP;
    const real *h = a.H + (size_t)it.series * KP + (size_t)nt * c;
    constexpr int NH = NT > 0 ? NT : 1;
    double hs[NH];
    if constexpr (NT > 0) {
#pragma unroll
        for (int q = 0; q < NT; q++) hs[q] = (double)h[q];
    }
    // kNzBatch entries of a group are in flight at a time (their index loads, then their gathers, are issued together); every
    // group still adds its e^2 in ascending entry order
    double acc = 0;
    const bool stored = it.kind == kNzStored || it.kind == kNzCorrect;
    for (uint32_t e0 = it.begin; e0 < it.end; e0 += 4u * kNzBatch) {
        uint32_t i[kNzBatch];
        double y[kNzBatch], dot[kNzBatch];
        bool on[kNzBatch];
#pragma unroll
        for (int u = 0; u < kNzBatch; u++) {
            const uint32_t e = e0 + 4u * u + (uint32_t)g;
            on[u] = e < it.end;                               // uniform over the 16 lanes of a group
            i[u] = 0; y[u] = 0;
            if (on[u]) {
                if (stored) { i[u] = a.idx[e]; y[u] = (double)a.val[e]; }
                else { i[u] = e; if (it.kind == kNzDense) y[u] = (double)a.Ynt[(size_t)it.series * a.T + e]; }
            }
        }
#pragma unroll
        for (int u = 0; u < kNzBatch; u++) {
            const real *w = a.W + (size_t)i[u] * KP + (size_t)nt * c;
            dot[u] = 0;
            if constexpr (NT > 0) {
#pragma unroll
                for (int q = 0; q < NT; q++) dot[u] = fma((double)w[q], hs[q], dot[u]);
            } else {
                for (int q = 0; q < nt; q++) dot[u] = fma((double)w[q], (double)h[q], dot[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kNzBatch; u++) {
            double d = dot[u];
            d += __shfl_xor(d, 1, kWave);                     // the 16 lanes of the group, a fixed tree
            d += __shfl_xor(d, 2, kWave);
            d += __shfl_xor(d, 4, kWave);
            d += __shfl_xor(d, 8, kWave);
            if (on[u]) {
                const double r = y[u] - d;
                acc += it.kind == kNzCorrect ? y[u] * (y[u] - 2.0 * d) : r * r;
            }
        }
    }
    const double g1 = __shfl(acc, 16, kWave), g2 = __shfl(acc, 32, kWave), g3 = __shfl(acc, 48, kWave);
    if (lane == 0) {
        a.part[2 * (size_t)item] = (acc + g1) + (g2 + g3);
        a.part[2 * (size_t)item + 1] = it.kind == kNzCorrect ? 0.0 : (double)(it.end - it.begin);
    }
}

// one thread per series: its items in ascending order
__global__ __launch_bounds__(256) void noise_series_kernel(const double *__restrict__ part, const uint32_t *__restrict__ first, int n,
                                                           double *__restrict__ sq, double *__restrict__ cnt) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0, c = 0;
    for (uint32_t e = first[j]; e < first[j + 1]; e++) { s += part[2 * (size_t)e]; c += part[2 * (size_t)e + 1]; }
    sq[j] = s; cnt[j] = c;
}

// one workgroup: the pooled sums in series order (staged through LDS 256 series at a time, added by thread 0), then every
// series' variance.  pooled[0] = sum sq, pooled[1] = sum cnt.
__global__ __launch_bounds__(256) void noise_pool_kernel(const double *__restrict__ sq, const double *__restrict__ cnt, int n,
                                                         double *__restrict__ sigma2, double *__restrict__ pooled) {
    __shared__ double ss[256], sc[256], tot[2];
    const int tid = threadIdx.x;
    double ps = 0, pc = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + tid;
        ss[tid] = j < n ? sq[j] : 0.0;
        sc[tid] = j < n ? cnt[j] : 0.0;
        __syncthreads();
        if (tid == 0) {
            const int m = n - j0 < 256 ? n - j0 : 256;
            for (int u = 0; u < m; u++) { ps += ss[u]; pc += sc[u]; }
        }
        __syncthreads();
    }
    if (tid == 0) { tot[0] = ps; tot[1] = pc; pooled[0] = ps; pooled[1] = pc; }
    __syncthreads();
    const double pv = tot[0] / tot[1];
    for (int j = tid; j < n; j += 256) sigma2[j] = cnt[j] > 0 ? sq[j] / cnt[j] : pv;
}

// grid (chunks of time, ceil(k / 64)): one thread per latent dimension, rows m + chunk * kNzInnovChunk .. in ascending order
__global__ __launch_bounds__(64) void noise_innov_kernel(NoiseInnovArgs a) {
#pragma clang fp contract(off)      // product and sum are rounded separately, like the roll-out
    extern __shared__ __align__(16) unsigned char nz_lds_raw[];
    const int c = threadIdx.x, t = blockIdx.y * 64 + c;
    const bool on = t < a.k;
    const int tl = on ? t : a.k - 1;                          // idle lanes shadow the last dimension and store nothing
    const int tp = colpos(tl, a.NT);
    int *lag = reinterpret_cast<int *>(nz_lds_raw);
    real *th = reinterpret_cast<real *>(nz_lds_raw + nz_lag_bytes(a.nlag));
    if (a.lds) {
        for (int l = c; l < a.nlag; l += 64) lag[l] = (int)a.lag_set[l];
        for (int l = 0; l < a.nlag; l++) th[l * 64 + c] = a.theta[(size_t)tl * a.nlag + l];
        __syncthreads();
    }
    const int i0 = a.m + (int)blockIdx.x * kNzInnovChunk;
    const int i1 = i0 + kNzInnovChunk < a.T ? i0 + kNzInnovChunk : a.T;
    double s = 0;
    for (int i = i0; i < i1; i++) {
        real acc = 0;
        for (int l = 0; l < a.nlag; l++) {
            const int lg = a.lds ? lag[l] : (int)a.lag_set[l];      // 0 <= lg <= m <= i
            const real thv = a.lds ? th[l * 64 + c] : a.theta[(size_t)tl * a.nlag + l];
            const real w = lg > 0 ? a.W[(size_t)(i - lg) * a.KP + tp] : real(0);
            const real prod = w * thv;
            acc = acc + prod;
        }
        const double r = (double)a.W[(size_t)i * a.KP + tp] - (double)acc;
        const double r2 = r * r;
        s = s + r2;
    }
    if (on) a.part[(size_t)blockIdx.x * a.k + t] = s;
}

// the chunks of a dimension in ascending order (theta_gram_kernel's rule)
__global__ __launch_bounds__(64) void noise_q_kernel(const double *__restrict__ part, int nchunks, int k, double denom, double *__restrict__ q) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= k) return;
    double s = 0;
    for (int ch = 0; ch < nchunks; ch++) s += part[(size_t)ch * k + t];
    q[t] = s / denom;
}

// psi[0] = 1, psi[s] = sum_{l: 0 < L_l <= s} Theta(l, d) psi[s - L_l] in fp64, ascending lag order, no contraction (the bits of
// trmf.uncertainty.impulse_response); v[s] = q (psi[0]^2 + .. + psi[s]^2).  One thread per dimension, ceil(k / 64) workgroups of
// one wavefront; psi[s] lives in slot s mod reach of a ring in LDS (the roll-out's shape), or in global memory where that does
// not fit.
__global__ __launch_bounds__(64) void forecast_psi_kernel(PsiArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char ps_lds_raw[];
    const int c = threadIdx.x, t = blockIdx.x * 64 + c, R = a.reach;
    const bool on = t < a.k;
    const int tl = on ? t : a.k - 1;
    const int tp = colpos(tl, a.NT);
    const double qd = a.q[tl];
    double cum = 0;
    bool bad = false;
    if (R > 0) {
        int *lag = reinterpret_cast<int *>(ps_lds_raw);
        real *th = reinterpret_cast<real *>(ps_lds_raw + nz_lag_bytes(a.nlag));
        double *ring = reinterpret_cast<double *>(ps_lds_raw + nz_lag_bytes(a.nlag) + psi_theta_bytes(a.nlag));
        for (int l = c; l < a.nlag; l += 64) lag[l] = (int)a.lag_set[l];
        for (int l = 0; l < a.nlag; l++) th[l * 64 + c] = a.theta[(size_t)tl * a.nlag + l];
        for (int r = 0; r < R; r++) ring[r * 64 + c] = 0.0;
        __syncthreads();                                        // the lags are shared; everything else is the thread's own
        int base = 0;                                           // slot of step s
        for (int s = 0; s < a.steps; s++) {
            double acc = 0;
            if (s == 0) acc = 1.0;
            else {
                for (int l = 0; l < a.nlag; l++) {
                    const int lg = lag[l];                      // 0 <= lg <= R
                    if (lg > 0 && lg <= s) {
                        int slot = base - lg;
                        slot += slot < 0 ? R : 0;
                        const double prod = (double)th[l * 64 + c] * ring[slot * 64 + c];
                        acc = acc + prod;
                    }
                }
            }
            ring[base * 64 + c] = acc;
            base = base + 1 == R ? 0 : base + 1;
            const double p2 = acc * acc;
            cum = cum + p2;
            const double v = qd * cum;
            bad = bad || !(v == v && fabs(v) < (double)INFINITY);
            if (on) a.v[(size_t)s * a.KP + tp] = v;
        }
    } else {
        const real *th = a.theta + (size_t)tl * a.nlag;
        double *psi = a.psi_glob;
        for (int s = 0; s < a.steps; s++) {
            double acc = 0;
            if (s == 0) acc = 1.0;
            else {
                for (int l = 0; l < a.nlag; l++) {
                    const int lg = (int)a.lag_set[l];
                    if (lg > 0 && lg <= s) {
                        const double prod = (double)th[l] * psi[(size_t)(s - lg) * a.k + tl];
                        acc = acc + prod;
                    }
                }
            }
            if (on) psi[(size_t)s * a.k + t] = acc;             // (idle lanes read the last dimension's entries and write nothing)
            const double p2 = acc * acc;
            cum = cum + p2;
            const double v = qd * cum;
            bad = bad || !(v == v && fabs(v) < (double)INFINITY);
            if (on) a.v[(size_t)s * a.KP + tp] = v;
        }
    }
    if (on && bad) atomicOr(a.flag, 1);
}

// the thread's running interval sums
struct IvSums {
    double cells = 0, covered = 0, sd_sum = 0, abs_truth = 0, z2_sum = 0, nll_sum = 0, crps_sum = 0;
};

// clip, inverse transform, the standard deviation, stores, interval sums: what every form does with a finished dot product and a
// finished variance.  The mean is forecast_finish's (forecast_kernels.hpp), operation for operation.
__device__ __forceinline__ void dist_finish(const DistArgs &a, int j, int i, real y, double V, real ta, real tb, bool tr, IvSums &s) {
#pragma clang fp contract(off)      // (y - b) / a with both operations rounded, like NormalizedTransform.postprocess
    if (a.clip) y = y < a.threshold ? a.threshold : y;
    double sdd = sqrt(V);
    if (tr) {
        const real d = y - tb;
        y = d / ta;
        sdd = sdd / fabs((double)ta);
    }
    const real sdr = (real)sdd;                                 // rounded once to the element type
    const size_t e = (size_t)i * a.n + j;
    if (a.Y) a.Y[e] = y;
    if (a.Ysd) a.Ysd[e] = sdr;
    if (a.truth) {
        const double yt = (double)a.truth[e], sd = (double)sdr, err = yt - (double)y;
        const double z = err / sd, z2 = z * z;
        const double hw = a.zq * sd;
        s.cells = s.cells + 1.0;
        if (fabs(err) <= hw) s.covered = s.covered + 1.0;
        s.sd_sum = s.sd_sum + sd;
        s.abs_truth = s.abs_truth + fabs(yt);
        s.z2_sum = s.z2_sum + z2;
        const double sd2 = sd * sd;
        const double lg = log(6.283185307179586 * sd2);
        const double nll = 0.5 * lg + 0.5 * z2;
        s.nll_sum = s.nll_sum + nll;
        const double zs = z / 1.4142135623730951;
        const double t1 = z * erf(zs);
        const double ph = exp(-0.5 * z2) / 2.5066282746310002;
        const double in = (t1 + 2.0 * ph) - 0.5641895835477563;
        const double crps = sd * in;
        s.crps_sum = s.crps_sum + crps;
    }
}

// NT = 1..4: k <= 64 (KP = 16 NT); NT = 0: 64 < k <= 1024.  The dot product of the mean is forecast_score_kernel's, fma for fma.
template <int NT>
__global__ __launch_bounds__(256) void forecast_dist_kernel(DistArgs a) {
    __shared__ __align__(16) real sw[kFdLdsReals];
    __shared__ __align__(16) double sv[kFdLdsReals];
    const int j0 = blockIdx.x * 256 + threadIdx.x;
    const bool on = j0 < a.n;
    const int j = on ? j0 : a.n - 1;                            // idle lanes of the last workgroup follow along and store nothing
    const int KP = NT > 0 ? kTile * NT : a.KP;
    const real *hrow = a.H + (size_t)j * KP;
    const bool tr = a.tr_a != nullptr;
    const real ta = tr ? a.tr_a[j] : real(1), tb = tr ? a.tr_b[j] : real(0);
    const double s2 = a.sigma2[j];
    IvSums s;

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
        for (int e = threadIdx.x; e < rows * KP; e += 256) {
            sw[e] = a.roll[(size_t)r0 * KP + e];
            sv[e] = a.v[(size_t)r0 * KP + e];
        }
        __syncthreads();
        if constexpr (NT > 0) {
            for (int r = 0; r < rows; r++) {
                const real *w = sw + r * KP;
                const double *vr = sv + r * KP;
                real d0 = 0, d1 = 0, d2 = 0, d3 = 0;
                double V = 0;
#pragma unroll
                for (int q = 0; q < NH / 4; q++) {
                    const Quad<real> v = reinterpret_cast<const Quad<real> *>(w)[q];       // every lane reads the same address
                    d0 = fma(h[4 * q], v.v[0], d0); d1 = fma(h[4 * q + 1], v.v[1], d1);
                    d2 = fma(h[4 * q + 2], v.v[2], d2); d3 = fma(h[4 * q + 3], v.v[3], d3);
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const double hd = (double)h[4 * q + u];
                        V = fma(hd * hd, vr[4 * q + u], V);
                    }
                }
                const real y = (d0 + d1) + (d2 + d3);
                if (on) dist_finish(a, j, r0 + r, y, s2 + V, ta, tb, tr, s);
            }
        } else {
            real d[kFdGenRows];
            double V[kFdGenRows];
#pragma unroll
            for (int r = 0; r < kFdGenRows; r++) { d[r] = 0; V[r] = 0; }
            for (int p = 0; p < KP; p += kTile) {
#pragma unroll
                for (int q = 0; q < kTile / 4; q++) {
                    const Quad<real> v = reinterpret_cast<const Quad<real> *>(hrow + p)[q];
#pragma unroll
                    for (int u = 0; u < 4; u++) h[4 * q + u] = v.v[u];
                }
#pragma unroll
                for (int r = 0; r < kFdGenRows; r++) {
                    if (r < rows) {
                        const real *w = sw + r * KP + p;
                        const double *vr = sv + r * KP + p;
#pragma unroll
                        for (int q = 0; q < kTile; q++) {
                            d[r] = fma(h[q], w[q], d[r]);
                            const double hd = (double)h[q];
                            V[r] = fma(hd * hd, vr[q], V[r]);
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < kFdGenRows; r++)
                if (r < rows && on) dist_finish(a, j, r0 + r, d[r], s2 + V[r], ta, tb, tr, s);
        }
    }
    if (on && a.truth) {
        const double *ti = a.table_in + (size_t)j * kIvSums;
        double *to = a.table_out + (size_t)j * kIvSums;
        to[0] = ti[0] + s.cells; to[1] = ti[1] + s.covered; to[2] = ti[2] + s.sd_sum; to[3] = ti[3] + s.abs_truth;
        to[4] = ti[4] + s.z2_sum; to[5] = ti[5] + s.nll_sum; to[6] = ti[6] + s.crps_sum;
    }
}
#endif

}  // namespace trmf
