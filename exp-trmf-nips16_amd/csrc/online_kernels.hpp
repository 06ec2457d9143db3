// online_kernels.hpp -- online updates (trmf_session_assimilate): new timestamps are absorbed by a forward filter instead of ALS
// iterations over the whole history.  H and Theta stay fixed; row i of W, in ascending order, becomes the minimiser of its own
// observations plus the AR prior from the rows before it:
//
//     A_i = G_i + (lambdaI + lambdaAR) I,   p_i[t] = sum_l Theta(l, t) W[i - lag_l][t],   W[i] = A_i^-1 (b_i + lambdaAR p_i)
//
// G_i / b_i come from the X-side Gram builders (gram_kernels.hpp; the shared H^T H and the rows of Y H on the full-observation
// path).  Two stages, because only the right-hand side depends on the rows before:
//
//   assim_factor_kernel<NT>   one wavefront per row, all rows in parallel: reads G_i from whichever cache layout is active (k x k,
//                             the packed upper triangle, or ONE shared Gram), adds the ridge and factors A_i = U^T U in the element
//                             type with lane c holding column c in registers (chol_wave_kernel's scheme).  A pivot that is not
//                             positive and finite raises the flag with the row's index (the smallest such row wins).
//   assim_chain_kernel        ONE workgroup walks the rows in order.  Wavefront 0 forms p_i with one lane per latent dimension from a
//                             ring of the last `reach` rows in LDS (forecast_rollout_kernel's ring; from global memory where that
//                             does not fit), then runs both substitutions with one unknown per lane; the other three wavefronts
//                             stage U_{i+1} into the second LDS buffer meanwhile.  The chain is bound by latency, not bandwidth:
//                             2k dependent steps per row, every operand in LDS.
//   assim_err_kernel          sum over Omega_i of (y - w_i . h_j)^2 per row for two versions of the rows (before / after), in fp64 and
//                             in a fixed order.
//
// Everything is written to scratch; the host commits the rows with one device copy once the flag has been read.
#pragma once

#include "common.hpp"

namespace trmf {

constexpr int kAssimChunk = 256;                // rows per pass: bounds the table of factors (8 MB at k = 64 in fp64)
constexpr int kAssimNoBadRow = 0x7f7f7f7f;      // the flag's idle value (a byte fill)

struct AssimFactorArgs {
    const real *G;                     // the Gram cache (or the one shared Gram)
    size_t gstride;                    // elements between the Grams of consecutive rows; 0: one shared Gram
    int packed;                        // upper triangles (cg_kernels.hpp: packed_gram_elems)
    real *U;                           // nrows x (k x k): upper factors, row-major, zeros below the diagonal
    int *flag;
    real lam;                          // lambdaI + lambdaAR
    int row0, nrows, k;
};

struct AssimChainArgs {
    const real *W;                     // the session's W: rows < first_row are read from here
    real *Wnew;                        // rows first_row .. : (rows - first_row) x KP, column-interleaved (the pads are the caller's: zero)
    real *flat;                        // nullptr, or (rows - first_row) x k row-major
    const real *Bv;                    // b_i: rows x KP, logical columns
    const real *U;                     // the factors of rows row0 .. row0 + nrows - 1
    const uint32_t *lag_set;
    const real *theta;                 // Theta(l, t) at t * nlag + l
    real lamAR;
    int first_row, row0, nrows, k, KP, NT, nlag;
    int reach;                         // ring rows in LDS (the largest lag), 0: the form that reads global memory
};

struct AssimErrArgs {
    const uint32_t *ptr, *idx;         // CSR of the training matrix (sparse storage), or nullptr
    const real *val;
    const real *Yd;                    // dense T x n row-major training matrix, or nullptr
    const real *H;
    const real *Wa, *Wb;               // row i of either at (i - rowa) * KP / (i - rowb) * KP
    int rowa, rowb;
    double *out;                       // per row: [2 r] with Wa, [2 r + 1] with Wb
    int row0, nrows, n, KP;
    int all;                           // every series counts, an absent entry reading as 0 (missing == 0)
};

__host__ __device__ inline size_t assim_lag_bytes(int nlag) { return ((size_t)nlag * sizeof(int) + 15) / 16 * 16; }
__host__ __device__ inline int assim_pitch(int k) { return k + 1; }     // odd for the even ranks: column reads of U spread over the banks
inline size_t assim_chain_lds_bytes(int k, int nlag, int reach) {
    const size_t ubuf = (size_t)2 * k * assim_pitch(k) * sizeof(real);
    return reach > 0 ? ubuf + assim_lag_bytes(nlag) + ((size_t)nlag + reach) * 64 * sizeof(real) : ubuf;
}

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declarations only (kernel_units.hpp)
template <int NT>
__global__ void assim_factor_kernel(AssimFactorArgs a);
__global__ void assim_chain_kernel(AssimChainArgs a);
__global__ void assim_err_kernel(AssimErrArgs a);
#else
__device__ __forceinline__ float assim_bcast(float v, int src_lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}
__device__ __forceinline__ double assim_bcast(double v, int src_lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), src_lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src_lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

template <int NT>
__global__ __launch_bounds__(256) void assim_factor_kernel(AssimFactorArgs a) {
    constexpr int KMAX = kTile * NT;
    const int wave = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.nrows) return;                           // wave-uniform; no block barrier below
    const int k = a.k;
    const real *Gi = a.G + (size_t)(a.row0 + r) * a.gstride;
    // lane c keeps column c; rows and columns >= k are padded with the identity, so no step needs a guard
    real col[KMAX];
#pragma unroll
    for (int s = 0; s < KMAX; s++) {
        real v = (s == c) ? real(1) : real(0);
        if (s < k && c < k) {
            if (a.packed) {
                const int lo = s < c ? s : c, hi = s < c ? c : s;
                v = Gi[lo * k - lo * (lo - 1) / 2 + hi - lo];
            } else v = Gi[s * k + c];
            if (s == c) v += a.lam;
        }
        col[s] = v;
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < KMAX; j++) {
        const real piv = assim_bcast(col[j], j);
        bad = bad || !(piv > real(0) && piv < real(INFINITY));
        const real d = sqrt(piv);
        const real u = (c == j) ? d : col[j] / d;
        col[j] = u;
#pragma unroll
        for (int s = j + 1; s < KMAX; s++) {
            col[s] = fma(-assim_bcast(u, s), u, col[s]);
            if ((s & 15) == 15) __builtin_amdgcn_sched_barrier(0);       // bound the scalar operands in flight
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (bad && c == 0) atomicMin(a.flag, a.row0 + r);
    real *Ur = a.U + (size_t)r * k * k;
    if (c < k) {
#pragma unroll
        for (int s = 0; s < KMAX; s++)
            if (s < k) Ur[(size_t)s * k + c] = s <= c ? col[s] : real(0);
    }
}

// b_i + lambdaAR p_i for lane c's latent dimension: products rounded to the element type and summed in ascending lag order, like
// Model.latent_forecast (no contraction)
__device__ __forceinline__ real assim_rhs_ring(const int *lag, const real *th, const real *ring, int nlag, int R, int base, int c, real b, real lamAR) {
#pragma clang fp contract(off)
    real acc = 0;
    for (int l = 0; l < nlag; l++) {
        int slot = base - lag[l];                           // 1 <= lag <= R
        slot += slot < 0 ? R : 0;
        const real prod = ring[slot * 64 + c] * th[l * 64 + c];
        acc = acc + prod;
    }
    const real pen = lamAR * acc;
    return b + pen;
}
__device__ __forceinline__ real assim_rhs_global(const AssimChainArgs &a, int i, int t, int tp, real b) {
#pragma clang fp contract(off)
    real acc = 0;
    for (int l = 0; l < a.nlag; l++) {
        const int src = i - (int)a.lag_set[l];              // >= 0: first_row >= the largest lag
        const real w = src >= a.first_row ? a.Wnew[(size_t)(src - a.first_row) * a.KP + tp] : a.W[(size_t)src * a.KP + tp];
        const real prod = w * a.theta[(size_t)t * a.nlag + l];
        acc = acc + prod;
    }
    const real pen = a.lamAR * acc;
    return b + pen;
}

__global__ __launch_bounds__(256) void assim_chain_kernel(AssimChainArgs a) {
    extern __shared__ __align__(16) unsigned char as_lds_raw[];
    const int tid = threadIdx.x, wave = tid >> 6, c = tid & 63;
    const int k = a.k, R = a.reach, UP = assim_pitch(k), usz = k * UP;
    real *Ub = reinterpret_cast<real *>(as_lds_raw);                       // two factors, pitch k + 1
    int *lag = reinterpret_cast<int *>(as_lds_raw + (size_t)2 * usz * sizeof(real));
    real *th = reinterpret_cast<real *>(as_lds_raw + (size_t)2 * usz * sizeof(real) + assim_lag_bytes(a.nlag));
    real *ring = th + (size_t)a.nlag * 64;
    const bool on = c < k;
    const int t = on ? c : k - 1;                           // idle lanes of wavefront 0 shadow the last unknown and store nothing
    const int tp = colpos(t, a.NT);
    int base = 0;
    if (R > 0 && wave == 0) {
        for (int l = c; l < a.nlag; l += 64) lag[l] = (int)a.lag_set[l];
        for (int l = 0; l < a.nlag; l++) th[l * 64 + c] = on ? a.theta[(size_t)t * a.nlag + l] : real(0);
        base = a.row0 % R;                                  // slot of row row0 (and of row row0 - R, which it replaces)
        for (int r = 0, slot = base; r < R; r++) {
            const int src = a.row0 - R + r;
            real w = 0;
            if (on) w = src >= a.first_row ? a.Wnew[(size_t)(src - a.first_row) * a.KP + tp] : a.W[(size_t)src * a.KP + tp];
            ring[slot * 64 + c] = w;
            slot = slot + 1 == R ? 0 : slot + 1;
        }
    }
    for (int e = tid; e < k * k; e += 256) Ub[(e / k) * UP + e % k] = a.U[e];
    __syncthreads();
    for (int r = 0; r < a.nrows; r++) {
        const int i = a.row0 + r;
        real *Uc = Ub + (r & 1) * usz;
        if (wave > 0) {
            if (r + 1 < a.nrows) {                          // the next row's factor, while this row is substituted
                const real *src = a.U + (size_t)(r + 1) * k * k;
                real *dst = Ub + ((r + 1) & 1) * usz;
                for (int e = tid - 64; e < k * k; e += 192) dst[(e / k) * UP + e % k] = src[e];
            }
        } else {
            const real b = a.Bv[(size_t)i * a.KP + t];
            real x = R > 0 ? assim_rhs_ring(lag, th, ring, a.nlag, R, base, c, b, a.lamAR) : assim_rhs_global(a, i, t, tp, b);
            // column-oriented substitutions, one unknown per lane (solve_rows_kernel): after step q every remaining lane has had
            // its U(.,.) z_q term removed
            for (int q = 0; q < k; q++) {                   // U^T z = b
                const real zq = assim_bcast(x, q) / Uc[q * UP + q];
                if (c == q) x = zq;
                else if (c > q) x -= Uc[q * UP + t] * zq;
            }
            for (int q = k - 1; q >= 0; q--) {              // U x = z
                const real xq = assim_bcast(x, q) / Uc[q * UP + q];
                if (c == q) x = xq;
                else if (c < q) x -= Uc[t * UP + q] * xq;
            }
            if (on) {
                a.Wnew[(size_t)(i - a.first_row) * a.KP + tp] = x;
                if (a.flat) a.flat[(size_t)(i - a.first_row) * k + t] = x;
            }
            if (R > 0) {
                ring[base * 64 + c] = on ? x : real(0);
                base = base + 1 == R ? 0 : base + 1;
            }
        }
        __syncthreads();
    }
}

// one workgroup per row; every sum in fp64, a thread's entries in index order, the threads' sums folded by a fixed tree
__global__ __launch_bounds__(256) void assim_err_kernel(AssimErrArgs a) {
    __shared__ double wa[kMaxRank], wb[kMaxRank], sa[256], sb[256];
    const int tid = threadIdx.x, r = blockIdx.x;
    if (r >= a.nrows) return;
    const int i = a.row0 + r, KP = a.KP;
    if (tid < KP) {
        wa[tid] = (double)a.Wa[(size_t)(i - a.rowa) * KP + tid];
        wb[tid] = (double)a.Wb[(size_t)(i - a.rowb) * KP + tid];
    }
    __syncthreads();
    // w . h_j: both factors are column-interleaved the same way and their pads are zero
    auto dots = [&](int j, double &pa, double &pb) {
        const real *h = a.H + (size_t)j * KP;
        pa = 0; pb = 0;
        for (int p = 0; p < KP; p++) {
            const double hv = (double)h[p];
            pa = fma(wa[p], hv, pa);
            pb = fma(wb[p], hv, pb);
        }
    };
    double ea = 0, eb = 0;
    if (a.all) {
        for (int j = tid; j < a.n; j += 256) {
            double pa, pb;
            dots(j, pa, pb);
            const double y = a.Yd ? (double)a.Yd[(size_t)i * a.n + j] : 0.0;
            ea += (y - pa) * (y - pa);
            eb += (y - pb) * (y - pb);
        }
    }
    if (a.ptr) {
        const uint32_t p0 = a.ptr[i], p1 = a.ptr[i + 1];
        for (uint32_t p = p0 + (uint32_t)tid; p < p1; p += 256u) {
            double pa, pb;
            dots((int)a.idx[p], pa, pb);
            const double y = (double)a.val[p];
            if (a.all) {                                    // the series was counted above with y = 0: (y - p)^2 - p^2 = y (y - 2 p)
                ea += y * (y - 2.0 * pa);
                eb += y * (y - 2.0 * pb);
            } else {
                ea += (y - pa) * (y - pa);
                eb += (y - pb) * (y - pb);
            }
        }
    }
    sa[tid] = ea; sb[tid] = eb;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { sa[tid] += sa[tid + w]; sb[tid] += sb[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) { a.out[2 * r] = sa[0]; a.out[2 * r + 1] = sb[0]; }
}
#endif

}  // namespace trmf
