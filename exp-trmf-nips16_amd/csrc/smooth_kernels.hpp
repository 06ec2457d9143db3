// smooth_kernels.hpp -- the fixed-interval smoother of the online rows (trmf_session_smooth): rows f .. T-1 of W become the joint
// minimiser of the training objective restricted to them, with H, Theta and every row before f fixed:
//
//     J_win = 1/2 sum_{i>=f} sum_{j in Omega_i} (y_ij - w_i . h_j)^2 + 1/2 lambdaI sum_{i>=f} |w_i|^2 + 1/2 lambdaAR sum_{i>=f} |e_i|^2
//     e_i   = w_i - sum_l Theta(l, .) o w_{i - L_l}                                  (rows < f enter e_i as constants)
//     g_i   = (G_i + lambdaI I) w_i - b_i + lambdaAR (e_i - sum_{l : i + L_l < T} Theta(l, .) o e_{i + L_l})
//
// g is linear in the rows: one SPD system of order m k (m = T - f).  It is solved for the correction d = x - x0 (x0: the rows as
// they stand) by preconditioned conjugate gradients; the preconditioner is block-Jacobi with the forward filter's own blocks
// A_i = G_i + (lambdaI + lambdaAR) I, whose factors assim_factor_kernel (online_kernels.hpp) writes for the whole window at once.
// G_i / b_i come from the X-side Gram builders, as for the filter.
//
// Every vector of the iteration (x, r, z, p twice, q, e) is m x 64 in logical column order, lane c of a row's wavefront owning
// latent dimension c; lanes >= k hold zeros.  Three launches per step, one wavefront per row, no workgroup waiting for another:
//
//   smooth_ar_kernel       the step's prologue and e = B p.  Every wavefront folds the row partials of r.z in a fixed order (fp64: a
//                          lane adds the rows lane, lane + 64, ..., then a butterfly over the lanes), takes the stop test
//                          r.z <= rtol^2 (r.z)_0 and beta = (r.z)_j / (r.z)_{j-1}; the first wavefront records them (and tells the
//                          host through a pinned word).  p_j = z + beta p_{j-1} goes to the other of two p buffers, so a row may form
//                          the p of its lagged rows itself while their wavefronts write them.  Theta and the lags are staged in LDS.
//                          INIT: e of x0 with the real head rows (the one application whose head is not zero).
//   smooth_apply_kernel    q_i = (G_i + lambdaI I) p_i + lambdaAR (e_i - sum_l Theta_l o e_{i + L_l}) with G_i read as column c per
//                          lane from any of the three layouts (k x k, packed upper triangle, one shared Gram), p_s broadcast from
//                          lane s; the row's partial of p.q to its slot.  INIT: r = b - q (minus the gradient at x0).
//   smooth_update_kernel   folds the partials of p.q, alpha = (r.z) / (p.q), x += alpha p, r -= alpha q, z_i = U_i^-1 U_i^-T r_i with
//                          U_i staged in LDS at pitch k + 1 and one unknown per lane (assim_chain_kernel's substitutions), the row's
//                          partial of r.z to its slot.  INIT: z and the partial only.
//   smooth_finish_kernel   the rows in the session's column-interleaved layout (and flat), and per row |w_i|^2 and |e_i|^2 of the
//                          rows as they were and as they are, in fp64 (the ridge and AR parts of J_win).
//
// Residual replacement, once per call.  The recursion r -= alpha q drifts from b - A x by the rounding of every product A p, and
// a start far from the minimiser leaves an error of eps |A| |x0| in the very first residual that the recursion never sees.  So
// the FIRST time the stop test holds, the step that follows is spent on the true residual instead: e = B x with the real head
// rows, r = b - A x, z = M^-1 r, and the iteration goes on from p = z for at least one step (one step of iterative refinement
// where the preconditioner is exact: a window of one row, lags beyond the window); the stop test is taken again after it.  A
// second replacement is never made (a tolerance below what the element type can resolve would otherwise loop).
//
// Once the stop test holds (or the factor kernel has flagged a bad pivot) every later launch returns at once, so the result does
// not depend on how far ahead the host had enqueued.  No floating-point atomics; every sum has a fixed order: the same bits on
// every call and every rank.
#pragma once

#include "common.hpp"

namespace trmf {

constexpr int kSmoothMaxRows = 1024;            // the cap on the window: the factor table is m k^2 reals (32 MB at k = 64 in fp64)
constexpr int kSmoothNoBadRow = 0x7f7f7f7f;     // the factor kernel's idle flag (online_kernels.hpp: kAssimNoBadRow)
constexpr int kSmoothDefaultMaxIter = 500;
constexpr int kSmoothMaxIter = 16383;           // the pinned word carries the step in 14 bits
#if defined(TRMF_F32)
constexpr double kSmoothDefaultRtol = 1e-5;     // ~ 84 eps
#else
constexpr double kSmoothDefaultRtol = 2e-14;    // ~ 90 eps
#endif

enum { SMOOTH_INIT = 0, SMOOTH_STEP = 1, SMOOTH_LAST = 2 };

struct SmoothState {
    double rz0;                        // (r.z) at the start
    double rz[2];                      // (r.z)_j at [j & 1]
    int iters;                         // steps taken when the stop test held
    int done;                          // 1: the stop test held (or a factor is bad)
    int refine[2];                     // at [j & 1]: step j replaces the residual (recomputes it from x) instead of stepping
    int refined[2];                    // at [j & 1]: the call's one replacement has been spent by step j
};

struct SmoothArgs {
    const real *W;                     // the session's W (column-interleaved, pitch KP): the head rows
    const real *x0;                    // the window's starting rows, m x KP column-interleaved (trmf_session_smooth: W + first_row * KP)
    const real *Bv;                    // b_i: rows x KP, logical columns
    const real *G;                     // the Gram cache (or the one shared Gram)
    size_t gstride;                    // elements between the Grams of consecutive rows; 0: one shared Gram
    int packed;
    int grow;                          // the row of G / Bv that window row 0 reads (trmf_session_smooth: first_row; 0: tables of the window's own)
    const real *U;                     // m x (k x k) upper factors of A_i, row-major
    const uint32_t *lag_set;
    const real *theta;                 // Theta(l, t) at t * nlag + l
    real *x, *r, *z, *q, *e;           // m x 64 each
    real *p[2];
    real *part_rz, *part_pq;           // m row partials each
    SmoothState *st;
    const int *flag;                   // the factor kernel's flag
    unsigned int *note;                // pinned host word: (seq << 15) | (step << 1) | stopped
    unsigned int note_seq;
    double tol2;                       // rtol^2
    real lamI, lamAR;
    int first_row, m, k, KP, NT, nlag;
    int lds_theta;                     // Theta and the lags staged in LDS (0: read from global memory)
};

struct SmoothFinishArgs {
    const real *W;
    const real *x;
    const uint32_t *lag_set;
    const real *theta;
    real *Wnew;                        // m x KP column-interleaved (the pads are the caller's: zero)
    real *flat;                        // nullptr, or m x k row-major
    double *out;                       // per row: |w|^2, |e|^2 as they were, |w|^2, |e|^2 as they are
    int first_row, m, k, KP, NT, nlag;
};

__host__ __device__ inline size_t smooth_lag_bytes(int nlag) { return ((size_t)nlag * sizeof(int) + 15) / 16 * 16; }
inline size_t smooth_theta_lds_bytes(int nlag) { return smooth_lag_bytes(nlag) + (size_t)nlag * 64 * sizeof(real); }
inline size_t smooth_update_lds_bytes(int k) { return (size_t)k * (k + 1) * sizeof(real); }

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
__global__ void smooth_ar_kernel(SmoothArgs a, int mode, int j);
__global__ void smooth_apply_kernel(SmoothArgs a, int mode, int j);
__global__ void smooth_update_kernel(SmoothArgs a, int mode, int j);
__global__ void smooth_finish_kernel(SmoothFinishArgs a);
#else
__device__ __forceinline__ float smooth_bcast(float v, int src_lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}
__device__ __forceinline__ double smooth_bcast(double v, int src_lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), src_lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src_lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// the sum over the 64 lanes, the same bits in every lane: v + v[lane ^ 32], then ^ 16, ... ^ 1
template <typename V> __device__ __forceinline__ V smooth_wave_sum(V v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// the m row partials in fp64: lane c adds the rows c, c + 64, ... in ascending order, then the butterfly
__device__ __forceinline__ double smooth_fold(const real *part, int m, int c) {
    double acc = 0;
    for (int r = c; r < m; r += 64) acc += (double)part[r];
    return smooth_wave_sum(acc);
}
// Theta(l, c) and the lags for this wavefront's lane: from LDS (staged once per workgroup) or straight from global memory
struct SmoothTheta {
    const real *th;                    // Theta(l, c) at th[l * ths]
    const int *lag;
    int ths;
};
__device__ __forceinline__ SmoothTheta smooth_stage_theta(const uint32_t *lag_set, const real *theta, int nlag, int k, int lds_theta, unsigned char *raw) {
    const int tid = threadIdx.x, c = tid & 63;
    const int t = c < k ? c : k - 1;
    if (!lds_theta) return SmoothTheta{theta + (size_t)t * nlag, reinterpret_cast<const int *>(lag_set), 1};
    int *lag = reinterpret_cast<int *>(raw);
    real *th = reinterpret_cast<real *>(raw + smooth_lag_bytes(nlag));
    for (int l = tid; l < nlag; l += blockDim.x) lag[l] = (int)lag_set[l];
    for (int e = tid; e < nlag * 64; e += blockDim.x) {
        const int l = e >> 6, cc = e & 63;
        th[e] = cc < k ? theta[(size_t)cc * nlag + l] : real(0);
    }
    __syncthreads();
    return SmoothTheta{th + c, lag, 64};
}

__global__ __launch_bounds__(256) void smooth_ar_kernel(SmoothArgs a, int mode, int j) {
    extern __shared__ __align__(16) unsigned char sm_ar_raw[];
    // `done` is set by an earlier launch, or by the first wavefront of THIS launch when the stop holds at this step; a wavefront that
    // already reads it here returns a few instructions before it would have taken the same decision below: nothing is written either way
    if (mode != SMOOTH_INIT && a.st->done) return;
    const int wave = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int k = a.k, f = a.first_row;
    const bool on = c < k;
    real beta = 0;
    bool refine = false;
    if (mode != SMOOTH_INIT) {
        // every wavefront takes the same decision from the same numbers
        const double rz = smooth_fold(a.part_rz, a.m, c);
        const double rz0 = j == 0 ? rz : a.st->rz0;
        const bool replaced = j > 0 && a.st->refine[(j + 1) & 1];           // the step before recomputed r: this r.z is the true one
        const bool spent = j > 0 && a.st->refined[(j + 1) & 1];
        const bool hit = replaced ? rz <= 0.0 : rz <= a.tol2 * rz0;        // after a replacement one step is always taken from the true r
        refine = hit && j > 0 && !spent && mode != SMOOTH_LAST;
        const bool stop = (hit && !refine) || *a.flag != kSmoothNoBadRow;
        if (j > 0 && !replaced) beta = (real)(rz / a.st->rz[(j + 1) & 1]);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.st->rz[j & 1] = rz;
            a.st->refine[j & 1] = refine && !stop ? 1 : 0;
            a.st->refined[j & 1] = spent || refine ? 1 : 0;
            if (j == 0) a.st->rz0 = rz;
            if (stop) { a.st->iters = j; a.st->done = 1; }
            if (a.note) __hip_atomic_store(a.note, (a.note_seq << 15) | ((unsigned int)j << 1) | (stop ? 1u : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (stop || mode == SMOOTH_LAST) return;
    }
    const SmoothTheta th = smooth_stage_theta(a.lag_set, a.theta, a.nlag, k, a.lds_theta, sm_ar_raw);
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.m) return;                                   // wave-uniform; no block barrier below
    const int tp = colpos(on ? c : 0, a.NT);
    const real *pold = a.p[(j + 1) & 1], *zz = a.z;
    real *pnew = a.p[j & 1];
    real own;
    if (mode == SMOOTH_INIT) own = on ? a.x0[(size_t)r * a.KP + tp] : real(0);
    else if (refine) own = a.x[(size_t)r * 64 + c];
    else own = on ? fma(beta, pold[(size_t)r * 64 + c], zz[(size_t)r * 64 + c]) : real(0);
    real acc = 0;
    for (int l = 0; l < a.nlag; l++) {
        const int src = r - th.lag[l];                      // window row of the lagged row; < 0: a head row
        real v = 0;
        if (mode == SMOOTH_INIT && src >= 0) {
            if (on) v = a.x0[(size_t)src * a.KP + tp];
        } else if (mode == SMOOTH_INIT || (refine && src < 0)) {
            if (on) v = a.W[(size_t)(f + src) * a.KP + tp];  // f + src >= 0: first_row >= the largest lag
        } else if (refine) v = a.x[(size_t)src * 64 + c];
        else if (src >= 0 && on) v = fma(beta, pold[(size_t)src * 64 + c], zz[(size_t)src * 64 + c]);
        acc = fma(th.th[l * th.ths], v, acc);
    }
    if (mode == SMOOTH_INIT) a.x[(size_t)r * 64 + c] = own;
    else if (!refine) pnew[(size_t)r * 64 + c] = own;
    a.e[(size_t)r * 64 + c] = on ? own - acc : real(0);
}

__global__ __launch_bounds__(256) void smooth_apply_kernel(SmoothArgs a, int mode, int j) {
    extern __shared__ __align__(16) unsigned char sm_ap_raw[];
    if (mode != SMOOTH_INIT && a.st->done) return;
    const int wave = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int k = a.k;
    const bool on = c < k;
    const SmoothTheta th = smooth_stage_theta(a.lag_set, a.theta, a.nlag, k, a.lds_theta, sm_ap_raw);
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.m) return;
    const int t = on ? c : 0;
    if (mode != SMOOTH_INIT && a.st->refine[j & 1]) mode = SMOOTH_INIT;      // a replacement step: r = b - A x, like the start
    const real *v = mode == SMOOTH_INIT ? a.x : a.p[j & 1];
    const real pv = v[(size_t)r * 64 + c];
    const real *Gi = a.G + (size_t)(a.grow + r) * a.gstride;
    // (G p)_c with lane c walking column c of the symmetric G_i: consecutive lanes read consecutive addresses
    real acc = 0;
    if (a.packed) {
        for (int s = 0; s < k; s++) {
            const int lo = s < t ? s : t, hi = s < t ? t : s;
            acc = fma(Gi[lo * k - lo * (lo - 1) / 2 + hi - lo], smooth_bcast(pv, s), acc);
        }
    } else {
        for (int s = 0; s < k; s++) acc = fma(Gi[s * k + t], smooth_bcast(pv, s), acc);
    }
    real ar = a.e[(size_t)r * 64 + c];
    for (int l = 0; l < a.nlag; l++) {
        const int dst = r + th.lag[l];
        if (dst < a.m) ar = fma(-th.th[l * th.ths], a.e[(size_t)dst * 64 + c], ar);
    }
    real qv = fma(a.lamAR, ar, fma(a.lamI, pv, acc));
    if (!on) qv = 0;
    if (mode == SMOOTH_INIT) {
        a.r[(size_t)r * 64 + c] = on ? a.Bv[(size_t)(a.grow + r) * a.KP + c] - qv : real(0);
        return;
    }
    a.q[(size_t)r * 64 + c] = qv;
    const real dot = smooth_wave_sum(pv * qv);
    if (c == 0) a.part_pq[r] = dot;
}

// one wavefront per workgroup: U_i in LDS at pitch k + 1 (odd for the even ranks: column reads spread over the banks)
__global__ __launch_bounds__(64) void smooth_update_kernel(SmoothArgs a, int mode, int j) {
    extern __shared__ __align__(16) unsigned char sm_up_raw[];
    if (mode != SMOOTH_INIT && a.st->done) return;
    real *Uc = reinterpret_cast<real *>(sm_up_raw);
    const int c = threadIdx.x, r = blockIdx.x;
    const int k = a.k, UP = k + 1;
    const bool on = c < k;
    const int t = on ? c : k - 1;                           // idle lanes shadow the last unknown and store nothing
    const real *Ur = a.U + (size_t)r * k * k;
    if (on)
        for (int s = 0; s < k; s++) Uc[s * UP + c] = Ur[s * k + c];
    real rv = a.r[(size_t)r * 64 + c];
    if (mode != SMOOTH_INIT && a.st->refine[j & 1]) mode = SMOOTH_INIT;      // a replacement step: z and the partial only
    if (mode != SMOOTH_INIT) {
        const double pq = smooth_fold(a.part_pq, a.m, c);   // (every lane takes part in the butterfly)
        const real alpha = (real)(a.st->rz[j & 1] / pq);
        if (on) {
            const real pv = a.p[j & 1][(size_t)r * 64 + c];
            a.x[(size_t)r * 64 + c] = fma(alpha, pv, a.x[(size_t)r * 64 + c]);
            rv = fma(-alpha, a.q[(size_t)r * 64 + c], rv);
            a.r[(size_t)r * 64 + c] = rv;
        }
    }
    __syncthreads();
    real x = rv;                                            // (zero in the idle lanes; nothing reads them)
    for (int q = 0; q < k; q++) {                         // U^T y = r
        const real zq = smooth_bcast(x, q) / Uc[q * UP + q];
        if (c == q) x = zq;
        else if (c > q) x -= Uc[q * UP + t] * zq;
    }
    for (int q = k - 1; q >= 0; q--) {                      // U z = y
        const real xq = smooth_bcast(x, q) / Uc[q * UP + q];
        if (c == q) x = xq;
        else if (c < q) x -= Uc[t * UP + q] * xq;
    }
    const real zv = on ? x : real(0);
    a.z[(size_t)r * 64 + c] = zv;
    const real dot = smooth_wave_sum(rv * zv);
    if (c == 0) a.part_rz[r] = dot;
}

__global__ __launch_bounds__(256) void smooth_finish_kernel(SmoothFinishArgs a) {
    const int wave = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.m) return;
    const int k = a.k, f = a.first_row;
    const bool on = c < k;
    const int t = on ? c : 0, tp = colpos(t, a.NT);
    const real xv = a.x[(size_t)r * 64 + c];
    const double wa = on ? (double)a.W[(size_t)(f + r) * a.KP + tp] : 0.0, wb = on ? (double)xv : 0.0;
    double ea = wa, eb = wb;
    for (int l = 0; l < a.nlag; l++) {
        const int src = r - (int)a.lag_set[l];
        const double th = on ? (double)a.theta[(size_t)t * a.nlag + l] : 0.0;
        const double old = on ? (double)a.W[(size_t)(f + src) * a.KP + tp] : 0.0;
        const double now = src >= 0 ? (double)a.x[(size_t)src * 64 + c] : old;
        ea = fma(-th, old, ea);
        eb = fma(-th, now, eb);
    }
    if (on) {
        a.Wnew[(size_t)r * a.KP + tp] = xv;
        if (a.flat) a.flat[(size_t)r * k + c] = xv;
    }
    const double s0 = smooth_wave_sum(wa * wa), s1 = smooth_wave_sum(ea * ea), s2 = smooth_wave_sum(wb * wb), s3 = smooth_wave_sum(eb * eb);
    if (c == 0) { a.out[4 * r] = s0; a.out[4 * r + 1] = s1; a.out[4 * r + 2] = s2; a.out[4 * r + 3] = s3; }
}
#endif

}  // namespace trmf
