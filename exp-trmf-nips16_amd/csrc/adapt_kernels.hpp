// adapt_kernels.hpp -- online loading updates (trmf_session_series_stats_init / trmf_session_adapt_series): the rows of H refitted from
// new timestamps in O(new data), the other half of online_kernels.hpp (which refits rows of W with H fixed).  The F-solve of series
// j depends on the history only through
//
//     S_j = sum_t om_t w_t w_t^T,   r_j = sum_t om_t y_tj w_t   (t over the stored entries of column j),   h_j = (S_j + lambdaI I)^-1 r_j
//
// so S_j (the packed upper triangle, assim_factor_kernel's packed layout) and r_j stay resident and a new entry costs one rank-1
// update: recursive least squares with forgetting, om_t = gamma^(rows - 1 - t).  Every sum runs in stored order in the element type;
// no floating-point atomics.
//
//   adapt_series_kernel<NT>   one wavefront (one 64-thread workgroup) per series, lane c holding column c of S_j in registers
//                             (assim_factor_kernel's scheme): loads the tables of the active generation (or starts from zero: the
//                             init pass), scales them by gamma^m, walks the column's unabsorbed tail -- 64 entries are fetched at a
//                             time, their rows of W gathered four at a time (k coalesced reals each) -- or adds the partial tables
//                             of the column's items in item order, stores the tables of the inactive generation, adds the ridge,
//                             factors S_j + lambdaI I = U^T U in registers with readlane broadcasts, and substitutes through a
//                             copy of U in LDS (the backward pass reads U by rows).  A pivot that is not positive and finite
//                             raises the flag with the series' index (the smallest wins).
//   adapt_part_kernel<NT>     the init pass over long columns: one wavefront per item (a fixed chunk of one column's entries),
//                             the same walk from zero into a slab.
//   adapt_full_*              the full-observation forms (dense storage, sparse storage with missing == 0): ONE shared S over
//                             the new rows of W, r_j per series, one factorisation (assim_factor_kernel) and n pairs of
//                             substitutions.  Not hot: plain code.
//
// Everything is written to scratch or to the inactive generation; the host commits once the flag has been read.
#pragma once

#include "common.hpp"

namespace trmf {

constexpr int kAdaptNoBadSeries = 0x7f7f7f7f;   // the flag's idle value (a byte fill)
constexpr uint32_t kAdaptChunk = 1024;          // init pass: a column longer than this is cut into items of this many entries ...
constexpr uint32_t kAdaptMaxItems = 8192;       // ... or more, so that the slab holds at most about this many partial tables

__host__ __device__ inline size_t adapt_packed(int k) { return (size_t)k * (k + 1) / 2; }
__host__ __device__ inline size_t adapt_part_reals(int k) { return adapt_packed(k) + (size_t)k; }      // a partial S, then a partial r

struct AdaptArgs {
    const uint32_t *ptr, *idx;         // CSC of the training matrix: column j at [ptr[j], ptr[j + 1]), idx = the timestamp
    const real *val;
    const uint32_t *start;             // per series: the first entry to absorb (items == nullptr or the series has none)
    const real *W;                     // rows x KP, column-interleaved
    const real *omega;                 // weight of timestamp t at omega[t - row0]; nullptr: 1 (gamma == 1)
    const real *Sin, *rin;             // the active generation (n x packed, n x k); nullptr: start from zero
    real *Sout, *rout;                 // the inactive generation
    const uint32_t *item_first;        // n + 1: items of series j are [item_first[j], item_first[j + 1]); nullptr: no items
    const uint32_t *items;             // (begin, end) entry positions per item
    real *slab;                        // adapt_part_reals(k) per item
    const real *Hold;                  // the session's H (n x KP, column-interleaved)
    real *Hnew;                        // scratch of the same shape (the pads are the caller's: zero)
    real *change;                      // per series: max_c |h_new - h_old|
    int *flag;
    real decay, lam;                   // gamma^m; lambdaI
    int row0, n, k, KP;
};

struct AdaptFullArgs {
    const uint32_t *ptr, *idx;         // CSC (sparse storage with missing == 0), or nullptr
    const real *val;
    const uint32_t *start;
    const real *Ynt;                   // dense n x rows (row-major), or nullptr
    const real *W;
    const real *omega;                 // as above
    const real *Sin, *rin;             // the shared packed S; n x k
    real *Sout, *rout;
    const real *U;                     // k x k upper factor of Sout + lambdaI I (assim_factor_kernel's output)
    const real *Hold;
    real *Hnew, *change;
    real decay;
    int row0, rows, n, k, KP, NT;
};

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
template <int NT>
__global__ void adapt_series_kernel(AdaptArgs a);
template <int NT>
__global__ void adapt_part_kernel(AdaptArgs a);
__global__ void adapt_full_gram_kernel(AdaptFullArgs a);
__global__ void adapt_full_rhs_kernel(AdaptFullArgs a);
__global__ void adapt_full_subst_kernel(AdaptFullArgs a);
__global__ void adapt_max_kernel(const real *change, int n, real *out);
#else
__device__ __forceinline__ int adapt_bcast(int v, int src_lane) { return __builtin_amdgcn_readlane(v, src_lane); }
__device__ __forceinline__ float adapt_bcast(float v, int src_lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}
__device__ __forceinline__ double adapt_bcast(double v, int src_lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), src_lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src_lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ real adapt_wave_max(real v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, kWave));
    return v;
}

// one entry: col[s] += (om w_s) w_c for lane c's column, rr += (om w_c) y
template <int KMAX>
__device__ __forceinline__ void adapt_rank1(real (&col)[KMAX], real &rr, real w, real om, real y) {
    const real aw = om * w;
#pragma unroll
    for (int s = 0; s < KMAX; s++) {
        col[s] = fma(adapt_bcast(aw, s), w, col[s]);
        if ((s & 15) == 15) __builtin_amdgcn_sched_barrier(0);           // bound the scalar operands in flight
    }
    rr = fma(aw, y, rr);
}

// entries [e0, e1) of one column in stored order.  Lane l fetches entry base + l of a batch of 64; the batch's rows of W are
// gathered four at a time (the loads of a group are in flight together), every lane reading its own column of the row.
template <int KMAX>
__device__ __forceinline__ void adapt_walk(const AdaptArgs &a, uint32_t e0, uint32_t e1, int c, int cp, bool on, real (&col)[KMAX], real &rr) {
    for (uint32_t base = e0; base < e1; base += 64u) {
        const uint32_t e = base + (uint32_t)c;
        const bool valid = e < e1;
        const int t = valid ? (int)a.idx[e] : a.row0;
        const real y = valid ? a.val[e] : real(0);
        const real om = valid ? (a.omega ? a.omega[max(t - a.row0, 0)] : real(1)) : real(0);
        const int cnt = (int)min(64u, e1 - base);
        for (int g = 0; g < cnt; g += 4) {
            real w[4], oy[4], oo[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int l = min(g + q, cnt - 1);                       // (a short last group repeats its last entry with weight 0)
                const int tq = adapt_bcast(t, l);
                const real wq = a.W[(size_t)tq * a.KP + cp];
                w[q] = on ? wq : real(0);
                oy[q] = adapt_bcast(y, l);
                oo[q] = g + q < cnt ? adapt_bcast(om, l) : real(0);
            }
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (g + q < cnt) adapt_rank1<KMAX>(col, rr, w[q], oo[q], oy[q]);
        }
    }
}

// col (lane c: column c of S, rows s <= c valid) and rr -> lane c's component of (S + lam I)^-1 r: the ridge, the factorisation
// S + lam I = U^T U in registers with readlane broadcasts, both substitutions through a copy of U in LDS (Us: KMAX x (KMAX + 1),
// the caller's; the backward pass reads U by rows).  col is destroyed.  bad is raised by a pivot that is not positive and finite.
// t = min(c, k - 1).  Shared by adapt_series_kernel and adapt_robust_series_kernel (adapt_robust_kernels.hpp).
template <int KMAX>
__device__ __forceinline__ real adapt_factor_solve(real (&col)[KMAX], real rr, real lam, bool on, int c, int t, int k, real *Us, bool &bad) {
    constexpr int SP = KMAX + 1;
    // the ridge; rows and columns >= k are padded with the identity, so no step needs a guard
#pragma unroll
    for (int s = 0; s < KMAX; s++)
        if (s == c) col[s] = on ? col[s] + lam : real(1);
#pragma unroll
    for (int q = 0; q < KMAX; q++) {
        const real piv = adapt_bcast(col[q], q);
        bad = bad || !(piv > real(0) && piv < real(INFINITY));
        const real d = sqrt(piv);
        const real u = (c == q) ? d : col[q] / d;
        col[q] = u;
#pragma unroll
        for (int s = q + 1; s < KMAX; s++) {
            col[s] = fma(-adapt_bcast(u, s), u, col[s]);
            if ((s & 15) == 15) __builtin_amdgcn_sched_barrier(0);       // bound the scalar operands in flight
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (on) {
#pragma unroll
        for (int s = 0; s < KMAX; s++)
            if (s < k) Us[s * SP + c] = s <= c ? col[s] : real(0);
    }
    __syncthreads();
    // column-oriented substitutions, one unknown per lane (assim_chain_kernel)
    real x = on ? rr : real(0);
    for (int q = 0; q < k; q++) {                           // U^T z = r
        const real zq = adapt_bcast(x, q) / Us[q * SP + q];
        if (c == q) x = zq;
        else if (c > q) x -= Us[q * SP + t] * zq;
    }
    for (int q = k - 1; q >= 0; q--) {                      // U h = z
        const real xq = adapt_bcast(x, q) / Us[q * SP + q];
        if (c == q) x = xq;
        else if (c < q) x -= Us[t * SP + q] * xq;
    }
    return x;
}

template <int NT>
__global__ __launch_bounds__(64) void adapt_part_kernel(AdaptArgs a) {
    constexpr int KMAX = kTile * NT;
    const int c = threadIdx.x, k = a.k;
    const uint32_t item = blockIdx.x;
    const bool on = c < k;
    const int cp = colpos(on ? c : k - 1, NT);
    real col[KMAX], rr = 0;
#pragma unroll
    for (int s = 0; s < KMAX; s++) col[s] = 0;
    adapt_walk<KMAX>(a, a.items[2 * item], a.items[2 * item + 1], c, cp, on, col, rr);
    real *slot = a.slab + (size_t)item * adapt_part_reals(k);
    if (on) {
#pragma unroll
        for (int s = 0; s < KMAX; s++)
            if (s <= c) slot[s * k - s * (s - 1) / 2 + c - s] = col[s];
        slot[adapt_packed(k) + c] = rr;
    }
}

template <int NT>
__global__ __launch_bounds__(64) void adapt_series_kernel(AdaptArgs a) {
    constexpr int KMAX = kTile * NT, SP = KMAX + 1;         // odd pitch: column reads spread over the banks
    __shared__ real Us[KMAX * SP];
    const int c = threadIdx.x, k = a.k;
    const int j = blockIdx.x;
    if (j >= a.n) return;
    const bool on = c < k;
    const int t = on ? c : k - 1;                           // idle lanes shadow the last unknown and store nothing
    const int cp = colpos(t, NT);
    const size_t PK = adapt_packed(k);
    // lane c keeps column c of S_j; only rows s <= c are ever read by another lane, the rest mirrors them
    real col[KMAX], rr = 0;
#pragma unroll
    for (int s = 0; s < KMAX; s++) col[s] = 0;
    if (a.Sin) {
        const real *Sj = a.Sin + (size_t)j * PK;
#pragma unroll
        for (int s = 0; s < KMAX; s++)
            if (on && s <= c) col[s] = a.decay * Sj[s * k - s * (s - 1) / 2 + c - s];
        if (on) rr = a.decay * a.rin[(size_t)j * k + c];
    }
    const uint32_t i0 = a.item_first ? a.item_first[j] : 0u, i1 = a.item_first ? a.item_first[j + 1] : 0u;
    if (i1 > i0) {                                          // the partial tables of a long column, in item order
        for (uint32_t i = i0; i < i1; i++) {
            const real *slot = a.slab + (size_t)i * adapt_part_reals(k);
#pragma unroll
            for (int s = 0; s < KMAX; s++)
                if (on && s <= c) col[s] += slot[s * k - s * (s - 1) / 2 + c - s];
            if (on) rr += slot[PK + c];
        }
    } else adapt_walk<KMAX>(a, a.start[j], a.ptr[j + 1], c, cp, on, col, rr);
    if (on) {
        real *So = a.Sout + (size_t)j * PK;
#pragma unroll
        for (int s = 0; s < KMAX; s++)
            if (s <= c) So[s * k - s * (s - 1) / 2 + c - s] = col[s];
        a.rout[(size_t)j * k + c] = rr;
    }
    bool bad = false;
    const real x = adapt_factor_solve<KMAX>(col, rr, a.lam, on, c, t, k, Us, bad);
    if (bad && c == 0) atomicMin(a.flag, j);
    real d = 0;
    if (on) {
        d = fabs(x - a.Hold[(size_t)j * a.KP + cp]);
        a.Hnew[(size_t)j * a.KP + cp] = x;
    }
    d = adapt_wave_max(d);
    if (c == 0) a.change[j] = d;
}

#if !defined(TRMF_UNIT) || TRMF_UNIT == 10    // (adapt_robust_kernels.hpp's unit includes this file for the shared code above)
// ---- the full-observation forms ------------------------------------------------------------------------------------------------
// the shared S: one thread per packed element, the new rows in ascending order
__global__ __launch_bounds__(256) void adapt_full_gram_kernel(AdaptFullArgs a) {
    const int k = a.k;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= (int)adapt_packed(k)) return;
    int s = 0, rem = e;
    while (rem >= k - s) { rem -= k - s; s++; }             // e = s k - s (s - 1) / 2 + (c - s)
    const int c = s + rem;
    const int sp = colpos(s, a.NT), cpos = colpos(c, a.NT);
    real acc = a.Sin ? a.decay * a.Sin[e] : real(0);
    for (int t = a.row0; t < a.rows; t++) {
        const real om = a.omega ? a.omega[t - a.row0] : real(1);
        const real *w = a.W + (size_t)t * a.KP;
        acc = fma(om * w[sp], w[cpos], acc);
    }
    a.Sout[e] = acc;
}

// r_j: one wavefront per series, lane c its own component; dense storage reads every new row, sparse storage the column's tail
__global__ __launch_bounds__(256) void adapt_full_rhs_kernel(AdaptFullArgs a) {
    const int wave = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + wave;
    if (j >= a.n || c >= a.k) return;
    const int cp = colpos(c, a.NT);
    real rr = a.rin ? a.decay * a.rin[(size_t)j * a.k + c] : real(0);
    if (a.Ynt) {
        const real *yj = a.Ynt + (size_t)j * a.rows;
        for (int t = a.row0; t < a.rows; t++) {
            const real om = a.omega ? a.omega[t - a.row0] : real(1);
            rr = fma(om * a.W[(size_t)t * a.KP + cp], yj[t], rr);
        }
    } else {
        for (uint32_t e = a.start[j]; e < a.ptr[j + 1]; e++) {
            const int t = (int)a.idx[e];
            const real om = a.omega ? a.omega[t - a.row0] : real(1);
            rr = fma(om * a.W[(size_t)t * a.KP + cp], a.val[e], rr);
        }
    }
    a.rout[(size_t)j * a.k + c] = rr;
}

// n pairs of substitutions with the one factor in LDS: a wavefront per series, four series per workgroup
__global__ __launch_bounds__(256) void adapt_full_subst_kernel(AdaptFullArgs a) {
    __shared__ real Us[kMaxRank * (kMaxRank + 1)];
    const int tid = threadIdx.x, wave = tid >> 6, c = tid & 63;
    const int k = a.k, SP = k + 1;
    for (int e = tid; e < k * k; e += 256) Us[(e / k) * SP + e % k] = a.U[e];
    __syncthreads();
    const int j = blockIdx.x * 4 + wave;
    if (j >= a.n) return;                                   // wave-uniform; no block barrier below
    const bool on = c < k;
    const int t = on ? c : k - 1;
    const int cp = colpos(t, a.NT);
    real x = a.rout[(size_t)j * k + t];
    for (int q = 0; q < k; q++) {                           // U^T z = r
        const real zq = adapt_bcast(x, q) / Us[q * SP + q];
        if (c == q) x = zq;
        else if (c > q) x -= Us[q * SP + t] * zq;
    }
    for (int q = k - 1; q >= 0; q--) {                      // U h = z
        const real xq = adapt_bcast(x, q) / Us[q * SP + q];
        if (c == q) x = xq;
        else if (c < q) x -= Us[t * SP + q] * xq;
    }
    real d = 0;
    if (on) {
        d = fabs(x - a.Hold[(size_t)j * a.KP + cp]);
        a.Hnew[(size_t)j * a.KP + cp] = x;
    }
    d = adapt_wave_max(d);
    if (c == 0) a.change[j] = d;
}

// max over the series (order does not matter for a maximum); one workgroup
__global__ __launch_bounds__(256) void adapt_max_kernel(const real *__restrict__ change, int n, real *__restrict__ out) {
    __shared__ real sm[256];
    real m = 0;
    for (int j = threadIdx.x; j < n; j += 256) m = fmax(m, change[j]);
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sm[0];
}
#endif
#endif

}  // namespace trmf
