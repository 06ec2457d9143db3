// heldout_kernels.hpp -- the model W.H^T evaluated at a resident set of held-out positions (trmf_session_eval_heldout): the
// imputation protocol of the paper scores predictions at the cells that were NOT trained on.
//
//   heldout_eval_kernel<NT>   per-workgroup fp64 partials of the six sums of TrmfHeldoutSums (+ the predictions, if asked for)
//   heldout_reduce_kernel     the partials in a fixed order -> six doubles
//
// Positions are COO in CSR order (sorted by timestamp): row u32[m], col u32[m], truth val[m].  Workgroup b owns the contiguous
// chunk [b*chunk, (b+1)*chunk) of entries whatever the rows look like (a held-out set of a skewed pattern -- zipf, imp -- costs
// the same per entry as a uniform one); inside it the 16 DPP rows of the workgroup take 16 consecutive entries per step, so the
// four entries of a wavefront mostly share their W row.  One 16-lane row per entry: lane c loads the NT adjacent reals of the
// W row and of the H row that sit at NT*c in the column-interleaved layout (common.hpp), the dot product is invariant under the
// common permutation and the pad columns are zero on both sides -- the idiom of loss_kernel.
//
// Determinism: every partial is a fixed sequence of fp64 additions (lane 0 of a DPP row, then a butterfly over the wavefront,
// then the four wavefronts in order), the slab of partials is reduced by one workgroup in a fixed order.  No atomics.
#pragma once

#include "common.hpp"

namespace trmf {

constexpr int kHoSums = 6;            // count, count_nonzero, sq_err, abs_err, abs_truth, rel_err (TrmfHeldoutSums order)
constexpr int kHoMaxBlocks = 2048;    // workgroups of one evaluation (8 wavefronts per CU of an MI355X at full size)
constexpr int kHoStep = 16;           // entries per workgroup step: 4 wavefronts x 4 DPP rows

struct HeldoutArgs {
    const uint32_t *row, *col;        // position (timestamp, series) of every held-out entry
    const real *val;                  // its truth
    const real *W, *H;                // the session's factors, KP reals per row
    real *pred;                       // nullptr, or m predictions in entry order
    double *part;                     // kHoSums x gridDim.x partials (sum-major)
    uint64_t m, chunk;                // entries; entries per workgroup (a multiple of kHoStep)
    int KP, NT;                       // read by the generic instantiation (NT template argument 0) only
};

#if !defined(TRMF_UNIT_BODIES)     // the main translation unit sees the declaration only (kernel_units.hpp)
template <int NT>
__global__ void heldout_eval_kernel(HeldoutArgs a);
#else
// NT = 1..4: k <= 64 (KP = 16 NT); NT = 0: 64 < k <= 1024, the lane's slice length a.NT read at run time
template <int NT>
__global__ __launch_bounds__(256) void heldout_eval_kernel(HeldoutArgs a) {
    __shared__ double sm[kHoSums][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15;
    const int slot = wave * 4 + (lane >> 4);                  // DPP row of the workgroup: entry e0 + slot of a step
    const int nt = NT > 0 ? NT : a.NT;
    const size_t KP = NT > 0 ? (size_t)kTile * NT : (size_t)a.KP;
    const uint64_t b0 = (uint64_t)blockIdx.x * a.chunk;
    const uint64_t b1 = b0 + a.chunk < a.m ? b0 + a.chunk : a.m;
    double s[kHoSums] = {0, 0, 0, 0, 0, 0};
    for (uint64_t e0 = b0; e0 < b1; e0 += kHoStep) {
        const uint64_t e = e0 + slot;
        const bool on = e < b1;                               // uniform over the 16 lanes of a DPP row
        const uint32_t i = on ? a.row[e] : 0u, j = on ? a.col[e] : 0u;
        const real *w = a.W + (size_t)i * KP + (size_t)nt * c;
        const real *h = a.H + (size_t)j * KP + (size_t)nt * c;
        real dot = 0;
        if constexpr (NT > 0) {
#pragma unroll
            for (int q = 0; q < NT; q++) dot = fma(w[q], h[q], dot);
        } else {
            for (int q = 0; q < nt; q++) dot = fma(w[q], h[q], dot);
        }
        dot += __shfl_xor(dot, 1, kWave);                     // the 16 lanes of the row
        dot += __shfl_xor(dot, 2, kWave);
        dot += __shfl_xor(dot, 4, kWave);
        dot += __shfl_xor(dot, 8, kWave);
        if (on && c == 0) {
            if (a.pred) a.pred[e] = dot;
            const double y = (double)a.val[e], d = (double)dot - y, ad = fabs(d), ay = fabs(y);
            s[0] += 1.0; s[2] += d * d; s[3] += ad; s[4] += ay;
            if (y != 0) { s[1] += 1.0; s[5] += ad / ay; }
        }
    }
#pragma unroll
    for (int q = 0; q < kHoSums; q++) {
        double v = s[q];
        for (int mk = 1; mk < kWave; mk <<= 1) v += __shfl_xor(v, mk, kWave);
        if (lane == 0) sm[q][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < kHoSums) {
        const int q = threadIdx.x;
        a.part[(size_t)q * gridDim.x + blockIdx.x] = (sm[q][0] + sm[q][1]) + (sm[q][2] + sm[q][3]);
    }
}
#endif

#if !defined(TRMF_UNIT)      // compiled by the main translation unit only (kernel_units.hpp)
// out[q] = sum over the nb partials of sum q, in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void heldout_reduce_kernel(const double *__restrict__ part, int nb, double *__restrict__ out) {
    __shared__ double sm[kHoSums][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kHoSums; q++) {
        double v = 0;
        for (int b = threadIdx.x; b < nb; b += 256) v += part[(size_t)q * nb + b];
        for (int mk = 1; mk < kWave; mk <<= 1) v += __shfl_xor(v, mk, kWave);
        if (lane == 0) sm[q][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < kHoSums) {
        const int q = threadIdx.x;
        out[q] = (sm[q][0] + sm[q][1]) + (sm[q][2] + sm[q][3]);
    }
}
#endif

}  // namespace trmf
