// session_online.hpp -- the calls that act on a resident session between training runs: growth and the sliding window, series churn,
// and the six online solves (assimilate, assimilate_robust, smooth, smooth_robust, series_stats_init / adapt_series,
// adapt_series_robust).  The top layer of the host session (session_state.hpp lists the layers): it uses the core's sync(),
// take_snapshot(), noise(), download_padded(), autotune() and alloc_time_scratch(); nothing below calls into it.
//
// The calls share their steps -- the storage tuple, the Gram rebuild of a window, the factor launch, the squared errors of a row
// range, the weights of the rows walked, the one-copy commit -- and each step has ONE definition, in the helper section below.
#pragma once

#include "session.hpp"

namespace trmf {

struct TrmfSessionImpl : SessionCore {
    // ---- the steps the calls share ------------------------------------------------------------------------------------------
    // Where a kernel finds Y: the compressed arrays of a sparse Y, or the dense orientation (the others null).  Row side: CSR /
    // T x n; column side: CSC / n x T.
    struct YStore { const uint32_t *ptr, *idx; const real *val, *dense; };
    YStore y_rows() const { return dense ? YStore{nullptr, nullptr, nullptr, Yd_tn.p} : YStore{Yr_ptr.p, Yr_idx.p, Yr_val.p, nullptr}; }
    YStore y_cols() const { return dense ? YStore{nullptr, nullptr, nullptr, Yd_nt.p} : YStore{Yc_ptr.p, Yc_idx.p, Yc_val.p, nullptr}; }
    // The squared errors of rows [row0, row0 + rows) against Hp: out[2 r] with the rows of Wa (the whole W), out[2 r + 1] with those
    // of Wb, whose first row is row `rowb`.
    int launch_row_errors(const real *Hp, const real *Wa, const real *Wb, int rowb, double *out, int row0, int rows) {
        const YStore y = y_rows();
        AssimErrArgs ea{y.ptr, y.idx, y.val, y.dense, Hp, Wa, Wb, 0, rowb, out, row0, rows, n, KP, full ? 1 : 0};
        hipLaunchKernelGGL(assim_err_kernel, dim3(rows), dim3(256), 0, stream, ea);
        TRMF_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // "Stage A": the Gram cache rows and right-hand sides of rows [first_row, T) by the X phase's own builders -- every X phase
    // rebuilds the rows it reads before it reads them (xsolve: gram_x / xprepare_full), so nothing relies on their old contents.
    int rebuild_window_systems(int first_row) {
        if (full) {
            if (y_times_factor(false, H.p, Bv.p, dense ? 0u : (uint32_t)first_row, (uint32_t)T)) return kFail;        // rows of Y H
            if (small_gram(H.p, n, real(0), GSx.p, stream)) return kFail;                                             // H^T H
        } else if (launch_gram_x_rows((uint32_t)first_row, (uint32_t)T)) return kFail;
        TRMF_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // The upper factors of G_i + lam I for `rows` systems from row0 on (four per workgroup); a bad pivot names its row in `flag`.
    int launch_factor(const real *Gp, size_t gstride, int packed, real *U, int *flag, real lam, int row0, int rows) {
        AssimFactorArgs fa{Gp, gstride, packed, U, flag, lam, row0, rows, k};
        if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(assim_factor_kernel<decltype(N)::value>, dim3((rows + 3) / 4), dim3(256), 0, stream, fa); }))
            return unsupported_rank();
        return 0;
    }
    // the bad-pivot flag of a call: every byte 0x7f, the value no row or series has (kAssimNoBadRow, kAdaptNoBadSeries)
    int new_flag(DevBuf<int> &flag) {
        if (flag.alloc(1, false)) return kFail;
        TRMF_HIP_CHECK(hipMemsetAsync(flag.p, 0x7f, sizeof(int), stream));
        return 0;
    }
    // The commit of a call that solved rows of W / all of H into scratch: ONE device copy after the flag has been read.
    int commit_rows(int first_row, const real *src, int rows) {
        TRMF_HIP_CHECK(hipMemcpyAsync(W.p + (size_t)first_row * KP, src, (size_t)rows * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (first_row < ad_rows) adapt_stale();                     // rows the series statistics absorbed have changed
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the new W
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        return 0;
    }
    int commit_loadings(const real *Hn) {
        TRMF_HIP_CHECK(hipMemcpyAsync(H.p, Hn, (size_t)n * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the new H
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        return 0;
    }
    // c * scale_j in the element type
    std::vector<real> huber_thresholds(double c, const double *scale) const {
        std::vector<real> thr((size_t)n);
        for (int j = 0; j < n; j++) thr[j] = (real)c * (real)scale[j];
        return thr;
    }
    // The weights of the m rows walked from row0 on, gamma^(rows - 1 - t) (none when gamma == 1: the kernels read 1), and the decay
    // gamma^m of what the tables hold.
    struct Forgetting { std::vector<real> w; real decay; };
    static Forgetting forget_weights(double gam, int row0, int m, int rows) {
        Forgetting f{{}, (real)std::pow(gam, (double)m)};
        if (gam != 1.0) {
            f.w.resize((size_t)std::max(m, 1));
            for (int i = 0; i < m; i++) f.w[i] = (real)std::pow(gam, (double)(rows - 1 - (row0 + i)));
        }
        return f;
    }
    // The init pass of the per-series fit cuts long columns into items: columns [cp[j], cp[j + 1]) of more than `chunk` entries, the
    // chunk set by the entry count of the whole problem.  first: cols + 1, items: (begin, end) per item.
    static uint32_t cut_long_columns(const uint64_t *cp, int cols, uint64_t entries, std::vector<uint32_t> &first, std::vector<uint32_t> &items) {
        uint64_t chunk = std::max<uint64_t>(kAdaptChunk, (entries + kAdaptMaxItems - 1) / kAdaptMaxItems);
        if (const char *e = test_env("TRMF_ADAPT_CHUNK")) chunk = (uint64_t)std::max(1, atoi(e));      // tests: several items per series on a small shape
        first.resize((size_t)cols + 1);
        for (int j = 0; j < cols; j++) {
            first[j] = (uint32_t)(items.size() / 2);
            if (cp[j + 1] - cp[j] > chunk)
                for (uint64_t b = cp[j]; b < cp[j + 1]; b += chunk) { items.push_back((uint32_t)b); items.push_back((uint32_t)std::min<uint64_t>(b + chunk, cp[j + 1])); }
        }
        first[cols] = (uint32_t)(items.size() / 2);
        return (uint32_t)(items.size() / 2);
    }
    // The per-series fit over a.n series.  Per-series tables: the items' partial sums, then one wavefront per series.  One shared S
    // (the full-observation forms): its Gram, the right-hand sides, the one factor ("series 0" names it), the substitution.
    int launch_series_fit(const AdaptArgs &a, uint32_t nitems) {
        if (!with_nt(NT, [&](auto N) {
                if (nitems) hipLaunchKernelGGL(adapt_part_kernel<decltype(N)::value>, dim3(nitems), dim3(64), 0, stream, a);
                hipLaunchKernelGGL(adapt_series_kernel<decltype(N)::value>, dim3(a.n), dim3(64), 0, stream, a);
            })) return unsupported_rank();
        return 0;
    }
    int launch_series_fit_full(const AdaptFullArgs &a, real *U, int *flag) {
        hipLaunchKernelGGL(adapt_full_gram_kernel, dim3((unsigned)((adapt_packed(k) + 255) / 256)), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(adapt_full_rhs_kernel, dim3((a.n + 3) / 4), dim3(256), 0, stream, a);
        if (launch_factor(a.Sout, (size_t)0, 1, U, flag, (real)lambdaI, 0, 1)) return kFail;
        hipLaunchKernelGGL(adapt_full_subst_kernel, dim3((a.n + 3) / 4), dim3(256), 0, stream, a);
        return 0;
    }
    // The PCG's vectors and sums of a window of m rows: seven m x 64 vectors over `vec`, two partial arrays over `part`.  The system
    // itself (x0, Bv, G, gstride, packed, grow) and the state are the caller's to set.
    SmoothArgs smooth_args(int first_row, int m, double rtol, real *U, real *vec, real *part, int *flag) const {
        const size_t V = (size_t)m * 64;
        SmoothArgs sa{};
        sa.W = W.p; sa.U = U;
        sa.lag_set = lag_set.p; sa.theta = theta.p;
        sa.x = vec; sa.r = vec + V; sa.z = vec + 2 * V; sa.q = vec + 3 * V; sa.e = vec + 4 * V; sa.p[0] = vec + 5 * V; sa.p[1] = vec + 6 * V;
        sa.part_rz = part; sa.part_pq = part + m; sa.flag = flag;
        sa.tol2 = rtol * rtol; sa.lamI = (real)lambdaI; sa.lamAR = (real)lambdaAR;
        sa.first_row = first_row; sa.m = m; sa.k = k; sa.KP = KP; sa.NT = NT; sa.nlag = nlag;
        return sa;
    }

    // ---- append new timestamps (trmf_session_append_rows; the rolling-window caller trmf.py:303-329) ---------------
    // Ynew: Tn x n block of NEW timestamps, same storage class as the session's Y.  Only that block (plus, for a
    // sparse Y, one 4-byte pointer per item) crosses PCIe: the CSR gains rows at its end, the CSC -- whose columns
    // each gain entries at their tails -- is rebuilt on the device from the old CSC and the block's CSC, a dense Y's
    // n x T copy is re-strided on the device, and W is extended by the AR recursion with the current Theta
    // (Model.latent_forecast, trmf.py:170-181, the reference's warm start :237-246).  H and Theta are kept.
    // The iteration counter restarts (a new train() call in the reference, trmf.cpp:647).
    int append_rows(const PyMatrix *Yn) {
        const int Tn = (int)Yn->rows, T0 = T;
        if ((int)Yn->cols != n) { set_error("append_rows: column count differs from the session's"); return kFail; }
        if ((Yn->type != TRMF_SPARSE) != dense) { set_error("append_rows: storage class (sparse/dense) differs from the session's"); return kFail; }
        if ((uint64_t)(T0 + Tn + 1) >= (1ull << 24) || (uint64_t)(T0 + Tn + 1) * KP * sizeof(real) > 0xffffffffull ||
            nnz + Yn->nnz >= (1ull << 32)) { set_error("append_rows: problem would exceed 32-bit device indices"); return kFail; }
        if (Tn <= 0) return 0;
        return slide(Yn, 0, false, nullptr);       // the growing case of the sliding window: one code path, the same bits
    }

    // ---- the sliding window (trmf_session_slide; slide_kernels.hpp) ---------------------------------------------------------------
    // Appends Ynew (as append_rows does; may be absent) and retires the `retire` oldest timestamps in ONE new generation of storage:
    // the CSR side, a dense Y (and its raw copy under a transform) and W are suffix copies, the CSC side is compacted stably per
    // column with the block's entries behind the survivors, the held-out set is compacted by the same kernel, and -- downdate -- the
    // loading statistics lose the retired entries' terms (read from the storage and the W of BEFORE the slide, written to the
    // inactive generation).  Afterwards the session is the one trmf_session_create would build from the retained entries in their
    // stored order, W[retire:] + the block's AR roll-out and the current H, Theta, weights and transform.  Failure-atomic like
    // append_rows: everything is built in locals and committed at the end.  slide_refusal() is the validation, run by the entry
    // point on the calling thread before any rank's worker starts (a refused call must not break the barrier of a TRMF_DEVICES group).
    struct SlideResult { uint64_t rows_retired = 0, entries_retired = 0, rows_appended = 0, entries_appended = 0, rows = 0, entries = 0; };
    std::string slide_refusal(const PyMatrix *Yn, int retire, int downdate) const {
        if (retire < 0) return "slide: retire must not be negative";
        if (downdate != 0 && downdate != 1) return "slide: downdate_stats must be 0 or 1";
        const int64_t Tn = Yn ? (int64_t)Yn->rows : 0;
        if (Yn) {
            if ((int)Yn->cols != n) return "slide: column count differs from the session's";
            if ((Yn->type != TRMF_SPARSE) != dense) return "slide: storage class (sparse/dense) differs from the session's";
        }
        if (retire > T) return "slide: cannot retire " + std::to_string(retire) + " rows, the session holds " + std::to_string(T) + " (rows of the block itself cannot be retired)";
        const int64_t T1 = (int64_t)T + Tn - retire;
        if (T1 < (int64_t)midx + 1)
            return "slide: retiring " + std::to_string(retire) + " rows would leave " + std::to_string(T1) + ", fewer than the largest lag + 1 = " + std::to_string(midx + 1);
        const uint64_t gone = dense ? 0 : host_row_ptr[(size_t)retire] - host_row_ptr[0];
        if ((uint64_t)(T1 + 1) >= (1ull << 24) || (uint64_t)(T1 + 1) * KP * sizeof(real) > 0xffffffffull || (!dense && nnz - gone + (Yn ? Yn->nnz : 0) >= (1ull << 32)))
            return "slide: problem would exceed 32-bit device indices";
        if (downdate) {
            if (full) return "slide: downdate_stats needs per-series statistics (sparse storage with missing != 0); the full-observation forms share one S";
            if (!ad_exists || !ad_valid) return "slide: downdate_stats without valid series statistics (trmf_session_series_stats_init)";
        }
        return "";
    }
    // counts of the columns' survivors -> host (retire > 0; the caller has filled the `o*` fields of the arguments)
    int slide_count(SlideArgs &sa, DevBuf<uint32_t> &d_kept, std::vector<uint32_t> &kept) {
        kept.assign((size_t)sa.ncols, 0u);
        if (sa.ncols <= 0) return 0;
        if (d_kept.alloc((size_t)sa.ncols, false)) return kFail;
        sa.kept = d_kept.p;
        hipLaunchKernelGGL(csc_slide_count_kernel, dim3((sa.ncols + 3) / 4), dim3(256), 0, stream, sa);
        TRMF_HIP_CHECK(hipGetLastError());
        // through the library's pinned staging when it is to be had (a copy into pageable memory is staged by the runtime)
        const size_t bytes = kept.size() * sizeof(uint32_t);
        std::unique_lock<std::mutex> lease;
        unsigned char *pin = HostStager::current().staging(bytes, lease);
        TRMF_HIP_CHECK(hipMemcpyAsync(pin ? (void *)pin : (void *)kept.data(), d_kept.p, bytes, hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (pin) std::memcpy(kept.data(), pin, bytes);
        return 0;
    }
    int slide(const PyMatrix *Yn, int retire, bool downdate, SlideResult *res) {
        const int Tn = Yn ? (int)Yn->rows : 0, T0 = T, Tk = T0 - retire, T1 = Tk + Tn;
        SlideResult out{};
        out.rows = (uint64_t)T0; out.entries = nnz;
        if (Tn <= 0 && retire == 0) { if (res) *res = out; return 0; }
        FillStreamScope fill(stream);
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        const uint64_t nzn = (Yn && !dense) ? Yn->nnz : 0;
        const uint64_t cut = dense ? 0 : host_row_ptr[(size_t)retire];        // CSR rows are contiguous: the retired entries are a prefix
        {   // the new generation of buffers in ONE slab (the pool returns the previous generation's slab once it is wholly free)
            const int Tsave = T; const uint64_t nzsave = nnz;
            T = T1; nnz = dense ? (uint64_t)T1 * n : nnz - cut + nzn;
            const size_t fp = footprint_estimate();
            T = Tsave; nnz = nzsave;
            DevicePool::current().reserve(fp);
        }
        // Failure-atomic: everything new is built in locals (device buffers, host pointer arrays, sums) and swapped into
        // the session only after every allocation, copy and kernel of the step has succeeded; a failed call leaves the
        // session exactly as it was.
        std::vector<uint64_t> new_row_ptr, new_col_ptr;
        std::vector<uint32_t> kept;                   // sparse storage, retire > 0: the survivors of every column
        uint64_t new_nnz = nnz;
        double new_ysq = ysq_acc;
        DevBuf<uint32_t> ptr2, idx2, cptr2, cidx2, hrow2, hcol2; DevBuf<real> val2, cval2, tn2, nt2, raw2, W2, hval2;
        uint64_t ho_m2 = ho_m;
        const bool ho_slide = ho_set && retire > 0 && ho_m > 0;
        const bool ad_down = downdate && retire > 0 && retire <= ad_rows;      // (retiring past the absorbed rows leaves the tables stale)
        SyncStreamOnExit drain(stream);
        if (!dense) {
            const uint64_t nz0 = nnz, nzk = nz0 - cut, nz1 = nzk + nzn;
            // CSR: the retained rows move to the front with their pointers rebased, the block's rows follow
            new_row_ptr.reserve((size_t)T1 + 1);
            for (int i = retire; i <= T0; i++) new_row_ptr.push_back(host_row_ptr[(size_t)i] - cut);
            for (int i = 1; i <= Tn; i++) new_row_ptr.push_back(nzk + Yn->row_ptr[i]);
            if (upload_ptr32(ptr2, (const size_t *)new_row_ptr.data(), (size_t)T1 + 1) || idx2.alloc(nz1, false) || val2.alloc(nz1, false)) return kFail;
            if (nzk) {
                TRMF_HIP_CHECK(hipMemcpyAsync(idx2.p, Yr_idx.p + cut, nzk * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
                TRMF_HIP_CHECK(hipMemcpyAsync(val2.p, Yr_val.p + cut, nzk * sizeof(real), hipMemcpyDeviceToDevice, stream));
            }
            if (nzn) {
                TRMF_HIP_CHECK(hipMemcpyAsync(idx2.p + nzk, Yn->col_idx, nzn * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                TRMF_HIP_CHECK(hipMemcpyAsync(val2.p + nzk, Yn->val_t, nzn * sizeof(real), hipMemcpyHostToDevice, stream));
            }
            // CSC: column j = its surviving entries in their stored order (timestamps reduced by `retire`), then the block's entries
            // of that column (timestamps shifted to follow the retained rows)
            SlideArgs sa{};
            sa.optr = Yc_ptr.p; sa.oidx = Yc_idx.p; sa.oval = Yc_val.p; sa.ncols = n; sa.retire = (uint32_t)retire; sa.shift = (uint32_t)Tk;
            DevBuf<uint32_t> d_kept;
            if (retire > 0) { if (slide_count(sa, d_kept, kept)) return kFail; }
            else { kept.resize((size_t)n); for (int j = 0; j < n; j++) kept[j] = (uint32_t)(host_col_ptr[j + 1] - host_col_ptr[j]); }
            new_col_ptr.assign((size_t)n + 1, 0);
            std::vector<uint32_t> np32((size_t)n + 1);
            for (int j = 0; j < n; j++) new_col_ptr[j + 1] = new_col_ptr[j] + kept[j] + (Yn ? (uint64_t)(Yn->col_ptr[j + 1] - Yn->col_ptr[j]) : 0);
            for (int j = 0; j <= n; j++) np32[j] = (uint32_t)new_col_ptr[j];
            if (new_col_ptr[n] != nz1) { set_error("slide: the two orientations of Y do not hold the same entries"); return kFail; }
            DevBuf<uint32_t> wptr, widx; DevBuf<real> wval;
            SyncStreamOnExit drain_block(stream);
            if (cptr2.upload(np32.data(), np32.size()) || cidx2.alloc(nz1, false) || cval2.alloc(nz1, false)) return kFail;
            if (Yn && (upload_ptr32(wptr, Yn->col_ptr, (size_t)n + 1) || widx.upload(Yn->row_idx, nzn) || wval.upload((const real *)Yn->val, nzn))) return kFail;
            if (Yn) { sa.wptr = wptr.p; sa.widx = widx.p; sa.wval = wval.p; }
            sa.nptr = cptr2.p; sa.nidx = cidx2.p; sa.nval = cval2.p;
            hipLaunchKernelGGL(csc_slide_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, sa);
            TRMF_HIP_CHECK(hipGetLastError());
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));
            new_nnz = nz1;
            if (device_sum_squares(val2.p, new_nnz, &new_ysq)) return kFail;
        } else {
            std::vector<real> blk;
            if (Yn) (void)dense_rows_to_rowmajor(Yn, blk);
            const size_t nk = (size_t)Tk * n;
            if (tn2.alloc((size_t)T1 * n, false) || nt2.alloc((size_t)T1 * n, false)) return kFail;
            if (nk) TRMF_HIP_CHECK(hipMemcpyAsync(tn2.p, Yd_tn.p + (size_t)retire * n, nk * sizeof(real), hipMemcpyDeviceToDevice, stream));
            if (!blk.empty()) TRMF_HIP_CHECK(hipMemcpyAsync(tn2.p + nk, blk.data(), blk.size() * sizeof(real), hipMemcpyHostToDevice, stream));
            if (has_transform) {                        // the block is RAW data: slide the raw copy, re-derive below
                if (raw2.alloc((size_t)T1 * n, false)) return kFail;
                if (nk) TRMF_HIP_CHECK(hipMemcpyAsync(raw2.p, Yraw.p + (size_t)retire * n, nk * sizeof(real), hipMemcpyDeviceToDevice, stream));
                if (!blk.empty()) TRMF_HIP_CHECK(hipMemcpyAsync(raw2.p + nk, blk.data(), blk.size() * sizeof(real), hipMemcpyHostToDevice, stream));
            }
            launch_transpose(tn2.p, T1, n, nt2.p);
            TRMF_HIP_CHECK(hipGetLastError());
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));      // blk is a local: its copies must have left the host
            new_nnz = (uint64_t)T1 * n;
            if (device_sum_squares(tn2.p, new_nnz, &new_ysq)) return kFail;    // over the new matrix, like a fresh session's
        }
        if (ad_down) {   // the retired entries' terms leave the tables: old storage, old W, active generation -> the other one
            std::vector<real> hom = forget_weights(ad_gamma, 0, retire, ad_rows).w;      // the weights the rows were absorbed with, negated
            for (real &v : hom) v = -v;
            DevBuf<uint32_t> d_abs; DevBuf<real> om;
            if (d_abs.upload(ad_cnt.data(), ad_cnt.size()) || (!hom.empty() && om.upload(hom.data(), hom.size()))) return kFail;
            DowndateArgs da{Yc_ptr.p, Yc_idx.p, Yc_val.p, d_abs.p, W.p, hom.empty() ? nullptr : om.p, ad_S[ad_cur].p, ad_r[ad_cur].p,
                            ad_S[1 - ad_cur].p, ad_r[1 - ad_cur].p, (uint32_t)retire, n, k, KP};
            if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(series_downdate_kernel<decltype(N)::value>, dim3(n), dim3(64), 0, stream, da); }))
                return unsupported_rank();
            TRMF_HIP_CHECK(hipGetLastError());
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));      // (d_abs and om are locals)
        }
        if (ho_slide) {  // held-out positions in retired rows are dropped, the rest shifted: the COO list as pseudo-columns of kSlideChunk entries
            const int nch = (int)((ho_m + kSlideChunk - 1) / kSlideChunk);
            std::vector<uint32_t> cp((size_t)nch + 1), hk, np((size_t)nch + 1, 0u);
            for (int c = 0; c <= nch; c++) cp[c] = (uint32_t)std::min<uint64_t>((uint64_t)c * kSlideChunk, ho_m);
            DevBuf<uint32_t> d_cp, d_np, d_kept;
            SlideArgs sa{};
            if (d_cp.upload(cp.data(), cp.size())) return kFail;
            sa.optr = d_cp.p; sa.oidx = ho_row.p; sa.oval = ho_val.p; sa.oaux = ho_col.p; sa.ncols = nch; sa.retire = (uint32_t)retire;
            if (slide_count(sa, d_kept, hk)) return kFail;
            for (int c = 0; c < nch; c++) np[c + 1] = np[c] + hk[c];
            ho_m2 = np[nch];
            if (d_np.upload(np.data(), np.size()) || hrow2.alloc(ho_m2, false) || hcol2.alloc(ho_m2, false) || hval2.alloc(ho_m2, false)) return kFail;
            sa.nptr = d_np.p; sa.nidx = hrow2.p; sa.nval = hval2.p; sa.naux = hcol2.p;
            hipLaunchKernelGGL(csc_slide_kernel, dim3((nch + 3) / 4), dim3(256), 0, stream, sa);
            TRMF_HIP_CHECK(hipGetLastError());
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));      // (the pointer arrays are locals)
        }
        DevBuf<double> hpart2;
        int ho_nb2 = ho_nb; uint64_t ho_chunk2 = ho_chunk;
        if (ho_slide) { heldout_geometry(ho_m2, &ho_nb2, &ho_chunk2); if (hpart2.alloc((size_t)kHoSums * ho_nb2, false)) return kFail; }
        {   // W: the retained rows, Tn rows rolled out by the AR model, one all-zero row at the end
            if (W2.alloc((size_t)(T1 + 1) * KP)) return kFail;
            if (Tn > 0 && retire > 0 && Tk < midx && k <= kMaxRank) {
                // the roll-out reads rows that are being retired: roll out behind the old rows first, then keep the suffix
                DevBuf<real> Wf;
                SyncStreamOnExit drain_w(stream);
                if (Wf.alloc((size_t)(T0 + Tn + 1) * KP)) return kFail;
                TRMF_HIP_CHECK(hipMemcpyAsync(Wf.p, W.p, (size_t)T0 * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
                hipLaunchKernelGGL(latent_forecast_kernel, dim3(1), dim3(64), 0, stream, Wf.p, T0, T0 + Tn, KP, NT, k, lag_set.p, nlag, theta.p);
                TRMF_HIP_CHECK(hipGetLastError());
                TRMF_HIP_CHECK(hipMemcpyAsync(W2.p, Wf.p + (size_t)retire * KP, (size_t)T1 * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
                TRMF_HIP_CHECK(hipStreamSynchronize(stream));
            } else {
                if (Tk) TRMF_HIP_CHECK(hipMemcpyAsync(W2.p, W.p + (size_t)retire * KP, (size_t)Tk * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
                // rank <= 64: the one-wavefront kernel this path has always used (its digests stay); above: the forecast's roll-out,
                // which covers every rank (the one-wavefront kernel rolled only the first 64 columns forward) and reads the OLD rows
                if (Tn > 0 && k <= kMaxRank) {
                    hipLaunchKernelGGL(latent_forecast_kernel, dim3(1), dim3(64), 0, stream, W2.p, Tk, T1, KP, NT, k, lag_set.p, nlag, theta.p);
                    TRMF_HIP_CHECK(hipGetLastError());
                } else if (Tn > 0 && launch_rollout(W.p, T0, Tn, W2.p + (size_t)Tk * KP, nullptr)) return kFail;
                TRMF_HIP_CHECK(hipStreamSynchronize(stream));
            }
        }
        // ---- commit ----
        if (!dense) {
            Yr_ptr.swap(ptr2); Yr_idx.swap(idx2); Yr_val.swap(val2);
            Yc_ptr.swap(cptr2); Yc_idx.swap(cidx2); Yc_val.swap(cval2);
            if (retire > 0 && ad_exists)            // the absorbed entries stay a prefix of every column: it lost the retired ones
                for (int j = 0; j < n && (size_t)j < ad_cnt.size(); j++) {
                    const uint32_t lost = (uint32_t)(host_col_ptr[j + 1] - host_col_ptr[j]) - kept[j];
                    ad_cnt[j] -= std::min(ad_cnt[j], lost);
                }
            host_row_ptr.swap(new_row_ptr); host_col_ptr.swap(new_col_ptr);
        } else {
            Yd_tn.swap(tn2); Yd_nt.swap(nt2);
            if (has_transform) Yraw.swap(raw2);
        }
        W.swap(W2);
        if (retire > 0) {
            if (ad_exists) {
                if (retire > ad_rows) adapt_stale();    // rows the tables never absorbed are gone: they no longer describe a prefix
                else if (ad_down) ad_cur = 1 - ad_cur;
                ad_rows = std::max(0, ad_rows - retire);
            }
            if (ho_slide) {
                ho_row.swap(hrow2); ho_col.swap(hcol2); ho_val.swap(hval2); ho_part.swap(hpart2); ho_pred.release();
                ho_m = ho_m2; ho_nb = ho_nb2; ho_chunk = ho_chunk2;
            }
            markW.release(); markH.release(); markT.release(); mark_iter = -1;     // a mark names rows that have moved
            snapW.release(); snapH.release(); snapT.release(); snap_iter = -1;
        }
        out.rows_retired = (uint64_t)retire; out.entries_retired = dense ? (uint64_t)retire * n : cut;
        out.rows_appended = (uint64_t)Tn; out.entries_appended = dense ? (uint64_t)Tn * n : nzn;
        out.rows = (uint64_t)T1; out.entries = new_nnz;
        if (res) *res = out;
        nnz = new_nnz; ysq_acc = new_ysq;
        T = T1;
        if (dense && has_transform && apply_series_transform()) return kFail;   // current coefficients over the new raw matrix
        set_trYTY();
        iter = 0;
        if (gramx_mode != kGramxReplicate && comm->world > 1 && !test_env("TRMF_GRAMX")) { gramx_mode = kGramxMeasure; gramx_calls = 0; }
        if (alloc_time_scratch()) return kFail;
        TRMF_HIP_CHECK(hipDeviceSynchronize());
        return autotune();
    }
    // ---- series churn (trmf_session_change_series; churn_kernels.hpp) ---------------------------------------------------------------
    // Retires the series with keep[j] == 0 and adds the m series of Ynew (rows() x m; may be absent) in ONE new generation of
    // storage: kept series keep their relative order and are renumbered densely from 0, the new ones follow.  The CSR side is
    // compacted stably per row with the block's entries behind the survivors (csr_churn_kernel), the CSC side is whole-column
    // copies (csc_gather_kernel) with the block's columns behind them, a dense Y -- or its raw copy under a transform -- is
    // gathered by columns (dense_churn_kernel) and by rows (row_gather_kernel), H, the transform coefficients and the per-series
    // loading statistics are row gathers, the held-out set is compacted by csr_churn_kernel over pseudo-rows.  fit: the new rows of H
    // are the ridge of adapt_series' init pass run over the new columns only (the same kernels: adapt_series_kernel / adapt_part_kernel,
    // or the full-observation forms with their one shared S), forget = the tables' gamma when they are carried, 1 otherwise.
    // Afterwards the session is the one trmf_session_create would build from the churned entries in their stored order, the current
    // W and lag weights and H = [H[keep]; H_new].  Failure-atomic like slide: everything is built in locals and committed at the end.
    // churn_refusal() is the validation, run by the entry point on the calling thread before any rank's worker starts.  A pivot of
    // the fit that is not positive and finite is not a failure of this rank's task (res->bad_series, nothing is committed).
    struct ChurnResult {
        uint64_t series_before = 0, series_retired = 0, series_added = 0, series = 0, entries_retired = 0, entries_added = 0, entries = 0, heldout_dropped = 0;
        int fitted = 0, stats_carried = 0, bad_series = -1;
        double sq_err_new = 0;
    };
    bool churn_carries_stats(int m, int fit) const { return ad_exists && ad_valid && ad_rows == T && !full && (m == 0 || fit); }
    std::string churn_refusal(const uint8_t *keep, const PyMatrix *Yn, int fit, const void *Hnew, const real *tra, const real *trb) const {
        if (fit != 0 && fit != 1) return "change_series: fit must be 0 or 1";
        const int64_t m = Yn ? (int64_t)Yn->cols : 0;
        int64_t nk = n;
        uint64_t nzk = dense ? 0 : nnz;
        if (keep) {
            nk = 0; nzk = 0;
            for (int j = 0; j < n; j++)
                if (keep[j]) { nk++; if (!dense) nzk += host_col_ptr[j + 1] - host_col_ptr[j]; }
        }
        if (Yn) {
            if ((Yn->type != TRMF_SPARSE) != dense) return "change_series: storage class (sparse/dense) differs from the session's";
            if ((int64_t)Yn->rows != (int64_t)T)
                return "change_series: the block has " + std::to_string((long long)Yn->rows) + " rows, the session holds " + std::to_string(T) + " (new series cover every timestamp held)";
        }
        if (nk + m == 0) return "change_series: no series would be left (keep is all zero and there is no block)";
        if (fit && Hnew) return "change_series: fit together with Hnew (the fit computes the new loadings)";
        if (fit && m > 0 && k > kMaxRank)
            return "change_series: the cold-start fit covers the register-tiled ranks 1..64, this session has rank " + std::to_string(k) + " (fit = 0 works at every rank)";
        if (!has_transform && (tra || trb)) return "change_series: transform coefficients given, but no series transform is set";
        if (has_transform && m > 0) {
            if (!tra || !trb) return "change_series: a series transform is set: the new series need both tr_a_new and tr_b_new";
            for (int64_t j = 0; j < m; j++) {
                if (!std::isfinite((double)tra[j]) || !std::isfinite((double)trb[j])) return "change_series: a transform coefficient of new series " + std::to_string((long long)j) + " is not finite";
                if (tra[j] == real(0)) return "change_series: tr_a_new of new series " + std::to_string((long long)j) + " is zero (the transform could not be undone)";
            }
        }
        const uint64_t n1 = (uint64_t)(nk + m);
        if (n1 + 1 >= (1ull << 24) || (n1 + 1) * KP * sizeof(real) > 0xffffffffull) return "change_series: problem would exceed 32-bit device indices";
        if (!dense && Yn) {
            if ((uint64_t)Yn->row_ptr[(size_t)T] != Yn->nnz || (uint64_t)Yn->col_ptr[(size_t)m] != Yn->nnz)
                return "change_series: the two orientations of the block hold different entry counts";
            if (nzk + Yn->nnz >= (1ull << 32)) return "change_series: problem would exceed 32-bit device indices";
            for (uint64_t e = 0; e < Yn->nnz; e++)
                if ((int64_t)Yn->col_idx[e] >= m || (int64_t)Yn->row_idx[e] >= (int64_t)T) return "change_series: a block entry lies outside rows() x m";
        }
        return "";
    }
    // counts of the rows' survivors -> host (the caller has filled the `o*` fields and the remap of the arguments)
    int churn_count(ChurnArgs &ca, DevBuf<uint32_t> &d_kept, std::vector<uint32_t> &kept) {
        kept.assign((size_t)ca.nrows, 0u);
        if (ca.nrows <= 0) return 0;
        if (d_kept.alloc((size_t)ca.nrows, false)) return kFail;
        ca.kept = d_kept.p;
        hipLaunchKernelGGL(csr_churn_count_kernel, dim3((ca.nrows + 3) / 4), dim3(256), 0, stream, ca);
        TRMF_HIP_CHECK(hipGetLastError());
        const size_t bytes = kept.size() * sizeof(uint32_t);
        std::unique_lock<std::mutex> lease;
        unsigned char *pin = HostStager::current().staging(bytes, lease);
        TRMF_HIP_CHECK(hipMemcpyAsync(pin ? (void *)pin : (void *)kept.data(), d_kept.p, bytes, hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (pin) std::memcpy(kept.data(), pin, bytes);
        return 0;
    }
    int launch_row_gather(const real *src, const uint32_t *list, int nrows, size_t rowlen, real *dst) {
        if (nrows <= 0 || rowlen == 0) return 0;
        hipLaunchKernelGGL(row_gather_kernel, dim3((unsigned)std::min(4096, (nrows + 3) / 4)), dim3(256), 0, stream, src, list, nrows, rowlen, dst);
        TRMF_HIP_CHECK(hipGetLastError());
        return 0;
    }
    int change_series(const uint8_t *keep, const PyMatrix *Yn, bool fit, const real *Hnew, const real *tra, const real *trb, ChurnResult *res) {
        const int n0 = n, m = Yn ? (int)Yn->cols : 0;
        ChurnResult out{};
        out.series_before = out.series = (uint64_t)n0; out.entries = nnz;
        if (!keep && m == 0) { if (res) *res = out; return 0; }
        if (sync()) return kFail;
        FillStreamScope fill(stream);
        std::vector<uint32_t> remap((size_t)n0), list;
        list.reserve((size_t)n0);
        for (int j = 0; j < n0; j++) {
            if (!keep || keep[j]) { remap[j] = (uint32_t)list.size(); list.push_back((uint32_t)j); }
            else remap[j] = kChurnGone;
        }
        const int nk = (int)list.size(), n1 = nk + m;
        const bool all_kept = nk == n0;
        const bool do_fit = fit && m > 0, carry = churn_carries_stats(m, fit ? 1 : 0);
        const uint64_t nzn = (Yn && !dense) ? Yn->nnz : 0;
        uint64_t nzk = 0;
        if (!dense) for (int q = 0; q < nk; q++) nzk += host_col_ptr[list[q] + 1] - host_col_ptr[list[q]];
        const uint64_t new_nnz = dense ? (uint64_t)T * n1 : nzk + nzn;
        {   // the new generation of buffers in ONE slab (the pool returns the previous generation's slab once it is wholly free)
            const uint64_t nzsave = nnz;
            n = n1; nnz = new_nnz;
            const size_t fp = footprint_estimate();
            n = n0; nnz = nzsave;
            DevicePool::current().reserve(fp);
        }
        const size_t PK = adapt_packed(k);
        std::vector<uint64_t> new_row_ptr, new_col_ptr;
        double new_ysq = ysq_acc;
        DevBuf<uint32_t> d_remap, d_list, ptr2, idx2, cptr2, cidx2, hrow2, hcol2, wptr, widx;
        DevBuf<real> val2, cval2, tn2, nt2, raw2, H2, a2, b2, S2, r2, S3, r3, hval2, wval, blk_d, blk_tr, blk_nt, Hn, Hraw, Hpad, chg, om, slab, U, Sfull, rfull;
        DevBuf<uint32_t> d_first, d_items;
        DevBuf<int> flag;
        DevBuf<double> errs, hpart2, trp;
        uint64_t ho_m2 = ho_m;
        const bool ho_churn = ho_set && !all_kept && ho_m > 0;
        SyncStreamOnExit drain(stream);
        if (d_remap.upload(remap.data(), remap.size()) || d_list.upload(list.data(), list.size())) return kFail;
        const real *fit_blk = nullptr;              // dense storage: the block T x m row-major in the scale the session trains on
        if (!dense) {
            // CSC: the kept columns in order, each as stored, then the block's columns as delivered
            new_col_ptr.assign((size_t)n1 + 1, 0);
            for (int q = 0; q < nk; q++) new_col_ptr[q + 1] = new_col_ptr[q] + (host_col_ptr[list[q] + 1] - host_col_ptr[list[q]]);
            for (int j = 0; j < m; j++) new_col_ptr[nk + j + 1] = new_col_ptr[nk + j] + (uint64_t)(Yn->col_ptr[j + 1] - Yn->col_ptr[j]);
            std::vector<uint32_t> np32((size_t)n1 + 1);
            for (int j = 0; j <= n1; j++) np32[j] = (uint32_t)new_col_ptr[j];
            if (cptr2.upload(np32.data(), np32.size()) || cidx2.alloc(new_nnz, false) || cval2.alloc(new_nnz, false)) return kFail;
            if (nk > 0) {
                CscGatherArgs ga{Yc_ptr.p, Yc_idx.p, Yc_val.p, d_list.p, cptr2.p, cidx2.p, cval2.p, nk};
                hipLaunchKernelGGL(csc_gather_kernel, dim3((nk + 3) / 4), dim3(256), 0, stream, ga);
                TRMF_HIP_CHECK(hipGetLastError());
            }
            if (nzn) {
                TRMF_HIP_CHECK(hipMemcpyAsync(cidx2.p + nzk, Yn->row_idx, nzn * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                TRMF_HIP_CHECK(hipMemcpyAsync(cval2.p + nzk, Yn->val, nzn * sizeof(real), hipMemcpyHostToDevice, stream));
            }
            // CSR: every row = its entries of kept series in stored order, renumbered, then the block's entries of that row
            ChurnArgs ca{};
            ca.optr = Yr_ptr.p; ca.oidx = Yr_idx.p; ca.oval = Yr_val.p; ca.nrows = T; ca.shift = (uint32_t)nk;
            ca.remap = all_kept ? nullptr : d_remap.p;
            std::vector<uint32_t> kept;
            DevBuf<uint32_t> d_kept;
            if (!all_kept) { if (churn_count(ca, d_kept, kept)) return kFail; }
            else { kept.resize((size_t)T); for (int i = 0; i < T; i++) kept[i] = (uint32_t)(host_row_ptr[i + 1] - host_row_ptr[i]); }
            new_row_ptr.assign((size_t)T + 1, 0);
            for (int i = 0; i < T; i++) new_row_ptr[i + 1] = new_row_ptr[i] + kept[i] + (m > 0 ? (uint64_t)(Yn->row_ptr[i + 1] - Yn->row_ptr[i]) : 0);
            if (new_row_ptr[T] != new_nnz) { set_error("change_series: the two orientations of Y do not hold the same entries"); return kFail; }
            if (upload_ptr32(ptr2, (const size_t *)new_row_ptr.data(), (size_t)T + 1) || idx2.alloc(new_nnz, false) || val2.alloc(new_nnz, false)) return kFail;
            if (m > 0) {
                if (upload_ptr32(wptr, Yn->row_ptr, (size_t)T + 1) || widx.upload(Yn->col_idx, nzn) || wval.upload((const real *)Yn->val_t, nzn)) return kFail;
                ca.wptr = wptr.p; ca.widx = widx.p; ca.wval = wval.p;
            }
            ca.nptr = ptr2.p; ca.nidx = idx2.p; ca.nval = val2.p;
            hipLaunchKernelGGL(csr_churn_kernel, dim3((T + 3) / 4), dim3(256), 0, stream, ca);
            TRMF_HIP_CHECK(hipGetLastError());
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));
            if (device_sum_squares(val2.p, new_nnz, &new_ysq)) return kFail;
        } else {
            std::vector<real> blk;
            if (m > 0) { (void)dense_rows_to_rowmajor(Yn, blk); if (blk_d.upload(blk.data(), blk.size())) return kFail; }
            const size_t N1 = (size_t)T * n1;
            if (tn2.alloc(N1, false) || nt2.alloc(N1, false) || (has_transform && raw2.alloc(N1, false))) return kFail;
            // the block is RAW data: under a transform the raw copy is churned and both orientations are re-derived after the commit
            DenseChurnArgs da{has_transform ? Yraw.p : Yd_tn.p, d_list.p, m > 0 ? blk_d.p : nullptr, has_transform ? raw2.p : tn2.p, T, n0, nk, m};
            hipLaunchKernelGGL(dense_churn_kernel, dim3((n1 + 255) / 256, (T + kChurnBand - 1) / kChurnBand), dim3(256), 0, stream, da);
            TRMF_HIP_CHECK(hipGetLastError());
            fit_blk = blk_d.p;
            if (has_transform) {
                if (a2.alloc((size_t)n1, false) || b2.alloc((size_t)n1, false)) return kFail;
                if (launch_row_gather(tr_a.p, d_list.p, nk, 1, a2.p) || launch_row_gather(tr_b.p, d_list.p, nk, 1, b2.p)) return kFail;
                if (m > 0) {
                    TRMF_HIP_CHECK(hipMemcpyAsync(a2.p + nk, tra, (size_t)m * sizeof(real), hipMemcpyHostToDevice, stream));
                    TRMF_HIP_CHECK(hipMemcpyAsync(b2.p + nk, trb, (size_t)m * sizeof(real), hipMemcpyHostToDevice, stream));
                    if (do_fit || k <= kMaxRank) {        // the block in the trained scale, for the fit and the error sum (the bits apply_series_transform gives)
                        if (blk_tr.alloc(blk.size(), false) || trp.alloc(1024)) return kFail;
                        hipLaunchKernelGGL(affine_columns_kernel, dim3(1024), dim3(256), 0, stream, blk_d.p, (size_t)T, m, a2.p + nk, b2.p + nk, blk_tr.p, trp.p);
                        TRMF_HIP_CHECK(hipGetLastError());
                        fit_blk = blk_tr.p;
                    }
                }
            } else {
                // the n x T orientation: row copies of the kept series, the block transposed behind them
                if (launch_row_gather(Yd_nt.p, d_list.p, nk, (size_t)T, nt2.p)) return kFail;
                if (m > 0) launch_transpose(blk_d.p, T, m, nt2.p + (size_t)nk * T);
                TRMF_HIP_CHECK(hipGetLastError());
            }
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));      // blk is a local: its copy must have left the host
            if (!has_transform && device_sum_squares(tn2.p, new_nnz, &new_ysq)) return kFail;    // over the new matrix, like a fresh session's
        }
        // H: the kept rows gathered, the new rows zero until the fit / the caller's values arrive (the pads and the extra row stay zero)
        if (H2.alloc((size_t)(n1 + 1) * KP)) return kFail;
        if (launch_row_gather(H.p, d_list.p, nk, (size_t)KP, H2.p)) return kFail;
        real *Hnew_rows = H2.p + (size_t)nk * KP;
        if (m > 0 && !do_fit && Hnew) {
            if (Hraw.upload(Hnew, (size_t)m * k) || Hpad.alloc((size_t)(m + 1) * KP, false)) return kFail;
            const size_t N = (size_t)(m + 1) * KP;
            hipLaunchKernelGGL(factor_pad_kernel, dim3((unsigned)std::min<size_t>(4096, (N + 255) / 256)), dim3(256), 0, stream, Hraw.p, (size_t)m, k, KP, NT, Hpad.p);
            TRMF_HIP_CHECK(hipGetLastError());
            TRMF_HIP_CHECK(hipMemcpyAsync(Hnew_rows, Hpad.p, (size_t)m * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        }
        // the loading statistics that are carried: the kept series' tables gathered (the new series' tables are the fit's output)
        if (carry) {
            if (S2.alloc((size_t)n1 * PK, false) || r2.alloc((size_t)n1 * k, false) || S3.alloc((size_t)n1 * PK, false) || r3.alloc((size_t)n1 * k, false)) return kFail;
            if (launch_row_gather(ad_S[ad_cur].p, d_list.p, nk, PK, S2.p) || launch_row_gather(ad_r[ad_cur].p, d_list.p, nk, (size_t)k, r2.p)) return kFail;
        }
        if (do_fit) {    // the cold-start fit: adapt_series' init pass over the new columns, W as it is
            const std::vector<real> hom = forget_weights(carry ? ad_gamma : 1.0, 0, T, T).w;
            if (Hn.alloc((size_t)m * KP) || chg.alloc(m, false) || (!hom.empty() && om.upload(hom.data(), hom.size())) || new_flag(flag)) return kFail;
            const real *omp = hom.empty() ? nullptr : om.p;
            if (!full) {
                // long columns are cut into items by the rule of the init pass on the churned problem (the bits of a fresh init)
                std::vector<uint32_t> hfirst, hitems;
                const uint32_t nitems = cut_long_columns(new_col_ptr.data() + nk, m, new_nnz, hfirst, hitems);
                if (nitems && (d_first.upload(hfirst.data(), hfirst.size()) || d_items.upload(hitems.data(), hitems.size()) ||
                               slab.alloc((size_t)nitems * adapt_part_reals(k), false))) return kFail;
                if (!carry && (Sfull.alloc((size_t)m * PK, false) || rfull.alloc((size_t)m * k, false))) return kFail;
                AdaptArgs a{cptr2.p + nk, cidx2.p, cval2.p, cptr2.p + nk, W.p, omp, nullptr, nullptr, carry ? S2.p + (size_t)nk * PK : Sfull.p,
                            carry ? r2.p + (size_t)nk * k : rfull.p, nitems ? d_first.p : nullptr, nitems ? d_items.p : nullptr, nitems ? slab.p : nullptr,
                            Hnew_rows, Hn.p, chg.p, flag.p, real(1), (real)lambdaI, 0, m, k, KP};
                if (launch_series_fit(a, nitems)) return kFail;
            } else {
                if (Sfull.alloc(PK, false) || rfull.alloc((size_t)m * k, false) || U.alloc((size_t)k * k, false)) return kFail;
                if (dense) {      // the m x T orientation of the block in the trained scale
                    if (blk_nt.alloc((size_t)T * m, false)) return kFail;
                    launch_transpose(fit_blk, T, m, blk_nt.p);
                }
                // the block's own arrays, not the session's: its CSC columns behind the kept ones, or its m x T orientation
                const YStore y = dense ? YStore{nullptr, nullptr, nullptr, blk_nt.p} : YStore{cptr2.p + nk, cidx2.p, cval2.p, nullptr};
                AdaptFullArgs a{y.ptr, y.idx, y.val, y.ptr, y.dense, W.p, omp, nullptr, nullptr, Sfull.p, rfull.p, U.p, Hnew_rows, Hn.p, chg.p, real(1), 0, T, m, k, KP, NT};
                if (launch_series_fit_full(a, U.p, flag.p)) return kFail;
            }
            TRMF_HIP_CHECK(hipGetLastError());
            int bad = kAdaptNoBadSeries;
            TRMF_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));
            if (bad != kAdaptNoBadSeries) { out.bad_series = bad; if (res) *res = out; return 0; }
            TRMF_HIP_CHECK(hipMemcpyAsync(Hnew_rows, Hn.p, (size_t)m * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        }
        if (m > 0 && k <= kMaxRank) {   // the new series' squared error with their new loadings (assim_err_kernel's reading of an entry), row order
            if (errs.alloc((size_t)2 * T, false)) return kFail;
            AssimErrArgs ea{dense ? nullptr : wptr.p, dense ? nullptr : widx.p, dense ? nullptr : wval.p, dense ? fit_blk : nullptr, Hnew_rows,
                            W.p, W.p, 0, 0, errs.p, 0, T, m, KP, dense ? 1 : 0};
            hipLaunchKernelGGL(assim_err_kernel, dim3(T), dim3(256), 0, stream, ea);
            TRMF_HIP_CHECK(hipGetLastError());
            std::vector<double> herr((size_t)2 * T);
            TRMF_HIP_CHECK(hipMemcpyAsync(herr.data(), errs.p, herr.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));
            for (int i = 0; i < T; i++) out.sq_err_new += herr[2 * i];
        }
        if (ho_churn) {  // held-out positions in retired series are dropped, the rest renumbered: the COO list as pseudo-rows of kSlideChunk entries
            const int nch = (int)((ho_m + kSlideChunk - 1) / kSlideChunk);
            std::vector<uint32_t> cp((size_t)nch + 1), hk, np((size_t)nch + 1, 0u);
            for (int c = 0; c <= nch; c++) cp[c] = (uint32_t)std::min<uint64_t>((uint64_t)c * kSlideChunk, ho_m);
            DevBuf<uint32_t> d_cp, d_np, d_kept;
            ChurnArgs ha{};
            if (d_cp.upload(cp.data(), cp.size())) return kFail;
            ha.optr = d_cp.p; ha.oidx = ho_col.p; ha.oval = ho_val.p; ha.oaux = ho_row.p; ha.remap = d_remap.p; ha.nrows = nch;
            if (churn_count(ha, d_kept, hk)) return kFail;
            for (int c = 0; c < nch; c++) np[c + 1] = np[c] + hk[c];
            ho_m2 = np[nch];
            if (d_np.upload(np.data(), np.size()) || hrow2.alloc(ho_m2, false) || hcol2.alloc(ho_m2, false) || hval2.alloc(ho_m2, false)) return kFail;
            ha.nptr = d_np.p; ha.nidx = hcol2.p; ha.nval = hval2.p; ha.naux = hrow2.p;
            hipLaunchKernelGGL(csr_churn_kernel, dim3((nch + 3) / 4), dim3(256), 0, stream, ha);
            TRMF_HIP_CHECK(hipGetLastError());
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));      // (the pointer arrays are locals)
        }
        int ho_nb2 = ho_nb; uint64_t ho_chunk2 = ho_chunk;
        if (ho_churn) { heldout_geometry(ho_m2, &ho_nb2, &ho_chunk2); if (hpart2.alloc((size_t)kHoSums * ho_nb2, false)) return kFail; }
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        // ---- commit ----
        out.series_retired = (uint64_t)(n0 - nk); out.series_added = (uint64_t)m; out.series = (uint64_t)n1;
        out.entries_retired = dense ? (uint64_t)T * (n0 - nk) : nnz - nzk; out.entries_added = dense ? (uint64_t)T * m : nzn; out.entries = new_nnz;
        out.heldout_dropped = ho_churn ? ho_m - ho_m2 : 0;
        out.fitted = do_fit ? 1 : 0; out.stats_carried = carry ? 1 : 0;
        if (!dense) {
            Yr_ptr.swap(ptr2); Yr_idx.swap(idx2); Yr_val.swap(val2);
            Yc_ptr.swap(cptr2); Yc_idx.swap(cidx2); Yc_val.swap(cval2);
        } else {
            Yd_tn.swap(tn2); Yd_nt.swap(nt2);
            if (has_transform) { Yraw.swap(raw2); tr_a.swap(a2); tr_b.swap(b2); }
        }
        H.swap(H2);
        if (ad_exists) {
            if (carry) {
                ad_S[ad_cur].swap(S2); ad_r[ad_cur].swap(r2); ad_S[1 - ad_cur].swap(S3); ad_r[1 - ad_cur].swap(r3);
                std::vector<uint32_t> cnt((size_t)n1);
                for (int j = 0; j < n1; j++) cnt[j] = (uint32_t)(new_col_ptr[j + 1] - new_col_ptr[j]);
                ad_cnt.swap(cnt);
            } else {                                  // the tables describe another set of series: stale, and their memory goes back
                for (int q = 0; q < 2; q++) { ad_S[q].release(); ad_r[q].release(); }
                ad_cnt.clear();
                adapt_stale();
            }
        }
        if (ho_churn) {
            ho_row.swap(hrow2); ho_col.swap(hcol2); ho_val.swap(hval2); ho_part.swap(hpart2); ho_pred.release();
            ho_m = ho_m2; ho_nb = ho_nb2; ho_chunk = ho_chunk2;
        }
        for (int q = 0; q < 2; q++) { fc_table[q].release(); fc_prev[q].release(); iv_table[q].release(); }      // per-series sums of another set of series
        fc_cur = 0; fc_rows = 0; iv_cur = 0; iv_rows = 0;
        nz_sigma2.release(); nz_q.release(); nz_set = false;
        markW.release(); markH.release(); markT.release(); mark_iter = -1;         // a mark names series that have moved
        snapW.release(); snapH.release(); snapT.release(); snap_iter = -1;
        if (!dense) { host_row_ptr.swap(new_row_ptr); host_col_ptr.swap(new_col_ptr); }
        if (res) *res = out;
        n = n1; nnz = new_nnz; ysq_acc = new_ysq;
        if (dense && has_transform && apply_series_transform()) return kFail;     // current coefficients over the new raw matrix
        set_trYTY();
        iter = 0;
        if (gramx_mode != kGramxReplicate && comm->world > 1 && !test_env("TRMF_GRAMX")) { gramx_mode = kGramxMeasure; gramx_calls = 0; }
        if (fs_mode != kShardOff && comm->world > 1 && !test_env("TRMF_FSHARD")) { fs_mode = kShardMeasure; fs_calls = 0; }
        if (alloc_series_scratch() || alloc_time_scratch()) return kFail;
        TRMF_HIP_CHECK(hipDeviceSynchronize());
        return autotune();
    }
    // ---- cell revisions (trmf_session_revise; revise_kernels.hpp) -------------------------------------------------------------------
    // Sets and deletes cells INSIDE the rows and series held, in ONE new generation of storage.  Sparse storage: every stored copy
    // of an edited cell leaves both orientations by a stable compaction (revise_count_kernel / revise_kernel, one pair for both
    // orientations), each set then places one entry at the end of its row (the sets of a row in ascending series order) and of its
    // column (ascending timestamp) -- so the result depends on the set of edits, not on their order in the batch.  Dense storage: the
    // cells are overwritten in copies of both orientations (dense_revise_kernel); under a transform the raw copy is edited and the
    // current coefficients are re-applied, as slide re-applies them.  update_stats: the loading statistics lose the removed entries'
    // terms and gain the sets' (series_revise_kernel over the touched series: storage of BEFORE the edit, W as it is, active
    // generation -> the other one).  Afterwards the session is the one trmf_session_create would build from the revised entries in
    // that stored order and the current W, H, lag weights and transform.  W, H, the lag weights, the mark, the held-out set and the
    // per-series score and noise tables are not touched.  Failure-atomic like slide: everything is built in locals and committed at
    // the end.  revise_refusal() is the validation, run by the entry point on the calling thread before any rank's worker starts.
    struct ReviseResult {
        uint64_t edits = 0, inserted = 0, replaced = 0, deleted = 0, missed = 0, copies_removed = 0, entries_before = 0, entries = 0;
        int first_row = -1, last_row = -1, stats_carried = 0;
    };
    // The batch bucketed by its major index: ptr (nmajor + 1), the minor indices ascending within a major index, values and flags.
    struct ReviseBucket { std::vector<uint32_t> ptr, idx; std::vector<real> val; std::vector<uint8_t> del; };
    static ReviseBucket revise_bucket(uint64_t count, const uint32_t *major, const uint32_t *minor, const real *vals, const uint8_t *del, int nmajor) {
        ReviseBucket b;
        b.ptr.assign((size_t)nmajor + 1, 0u); b.idx.resize(count); b.val.resize(count); b.del.resize(count);
        for (uint64_t e = 0; e < count; e++) b.ptr[(size_t)major[e] + 1]++;
        for (int i = 0; i < nmajor; i++) b.ptr[(size_t)i + 1] += b.ptr[i];
        // a counting pass places every edit in its major index's range; each range is then sorted by the minor index
        std::vector<uint32_t> next(b.ptr.begin(), b.ptr.end() - 1), slot(count);
        for (uint64_t e = 0; e < count; e++) slot[next[major[e]]++] = (uint32_t)e;
        for (int i = 0; i < nmajor; i++)
            if (b.ptr[(size_t)i + 1] - b.ptr[i] > 1)
                std::sort(slot.begin() + b.ptr[i], slot.begin() + b.ptr[(size_t)i + 1],
                          [&](uint32_t x, uint32_t y) { return minor[x] != minor[y] ? minor[x] < minor[y] : x < y; });
        for (uint64_t q = 0; q < count; q++) {
            const uint32_t e = slot[q];
            b.idx[q] = minor[e]; b.del[q] = (del && del[e]) ? 1 : 0; b.val[q] = (b.del[q] || !vals) ? real(0) : vals[e];
        }
        return b;
    }
    bool revise_carries_stats() const { return ad_exists && ad_valid && ad_rows == T && !full; }
    std::string revise_refusal(uint64_t count, const uint32_t *rows, const uint32_t *cols, const void *vals, const uint8_t *del, int update_stats) const {
        if (update_stats != 0 && update_stats != 1) return "revise: update_stats must be 0 or 1";
        if (count == 0) return "";
        // (the size is judged before the arrays are read: every edit may be an insert)
        if (count >= (1ull << 32) || (!dense && nnz + count >= (1ull << 32))) return "revise: problem would exceed 32-bit device indices";
        if (!rows || !cols) return "revise: rows and cols are needed";
        if (dense && del)
            for (uint64_t e = 0; e < count; e++)
                if (del[e]) return "revise: a delete on dense storage (every cell of a dense Y is observed; set a value instead)";
        bool any_set = false;
        for (uint64_t e = 0; e < count; e++) {
            if (rows[e] >= (uint32_t)T) return "revise: edit " + std::to_string(e) + " names row " + std::to_string(rows[e]) + ", the session holds " + std::to_string(T);
            if (cols[e] >= (uint32_t)n) return "revise: edit " + std::to_string(e) + " names series " + std::to_string(cols[e]) + ", the session holds " + std::to_string(n);
            any_set = any_set || !del || !del[e];
        }
        if (any_set && !vals) return "revise: vals is needed (the batch holds sets)";
        {   // a cell named twice: neighbours in the batch bucketed by row
            const ReviseBucket b = revise_bucket(count, rows, cols, nullptr, nullptr, T);
            for (int i = 0; i < T; i++)
                for (uint32_t q = b.ptr[i] + 1; q < b.ptr[(size_t)i + 1]; q++)
                    if (b.idx[q] == b.idx[q - 1])
                        return "revise: cell (" + std::to_string(i) + ", " + std::to_string(b.idx[q]) + ") is named twice in one batch";
        }
        if (update_stats) {
            if (full) return "revise: update_stats needs per-series statistics (sparse storage with missing != 0); the full-observation forms share one S";
            if (!ad_exists || !ad_valid) return "revise: update_stats without valid series statistics (trmf_session_series_stats_init)";
        }
        return "";
    }
    // d_src (count values on the device) -> host, through the library's pinned staging when it is to be had
    int revise_fetch(const uint32_t *d_src, std::vector<uint32_t> &dst, size_t count) {
        dst.assign(count, 0u);
        if (!count) return 0;
        const size_t bytes = count * sizeof(uint32_t);
        std::unique_lock<std::mutex> lease;
        unsigned char *pin = HostStager::current().staging(bytes, lease);
        TRMF_HIP_CHECK(hipMemcpyAsync(pin ? (void *)pin : (void *)dst.data(), d_src, bytes, hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (pin) std::memcpy(dst.data(), pin, bytes);
        return 0;
    }
    // One orientation's bucket on the device.
    struct ReviseBucketDev {
        DevBuf<uint32_t> ptr, idx; DevBuf<real> val; DevBuf<uint8_t> del;
        int upload(const ReviseBucket &b) { return ptr.upload(b.ptr.data(), b.ptr.size()) || idx.upload(b.idx.data(), b.idx.size()) || val.upload(b.val.data(), b.val.size()) || del.upload(b.del.data(), b.del.size()) ? kFail : 0; }
    };
    int revise(uint64_t count, const uint32_t *rows, const uint32_t *cols, const real *vals, const uint8_t *del, bool update_stats, ReviseResult *res) {
        ReviseResult out{};
        out.entries_before = out.entries = nnz;
        if (count == 0) { if (res) *res = out; return 0; }
        if (sync()) return kFail;
        FillStreamScope fill(stream);
        out.edits = count;
        uint64_t nsets = 0;
        uint32_t rmin = rows[0], rmax = rows[0];
        for (uint64_t e = 0; e < count; e++) { nsets += (!del || !del[e]) ? 1 : 0; rmin = std::min(rmin, rows[e]); rmax = std::max(rmax, rows[e]); }
        out.first_row = (int)rmin; out.last_row = (int)rmax;
        {   // the new generation of buffers in ONE slab (the pool returns the previous generation's slab once it is wholly free)
            const uint64_t nzsave = nnz;
            if (!dense) nnz += nsets;
            const size_t fp = footprint_estimate();
            nnz = nzsave;
            DevicePool::current().reserve(fp);
        }
        const bool carry = update_stats && revise_carries_stats();
        bool changed = true;                          // a column has changed (a batch of deletes that all miss changes nothing)
        std::vector<uint64_t> new_row_ptr, new_col_ptr;
        uint64_t new_nnz = nnz;
        double new_ysq = ysq_acc;
        DevBuf<uint32_t> ptr2, idx2, cptr2, cidx2; DevBuf<real> val2, cval2, tn2, nt2, raw2;
        SyncStreamOnExit drain(stream);
        if (!dense) {
            const ReviseBucket br = revise_bucket(count, rows, cols, vals, del, T), bc = revise_bucket(count, cols, rows, vals, del, n);
            ReviseBucketDev dr, dc;
            DevBuf<uint32_t> d_kept_r, d_kept_c, d_hits;
            SyncStreamOnExit drain_batch(stream);
            if (dr.upload(br) || dc.upload(bc) || d_kept_r.alloc((size_t)T, false) || d_kept_c.alloc((size_t)n, false) || d_hits.alloc(count)) return kFail;
            ReviseArgs ra{Yr_ptr.p, Yr_idx.p, Yr_val.p, dr.ptr.p, dr.idx.p, dr.val.p, dr.del.p, nullptr, nullptr, nullptr, d_kept_r.p, d_hits.p, T};
            ReviseArgs ca{Yc_ptr.p, Yc_idx.p, Yc_val.p, dc.ptr.p, dc.idx.p, dc.val.p, dc.del.p, nullptr, nullptr, nullptr, d_kept_c.p, nullptr, n};
            hipLaunchKernelGGL(revise_count_kernel, dim3((T + 3) / 4), dim3(256), 0, stream, ra);
            hipLaunchKernelGGL(revise_count_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, ca);
            TRMF_HIP_CHECK(hipGetLastError());
            std::vector<uint32_t> kept_r, kept_c, hits;
            if (revise_fetch(d_kept_r.p, kept_r, (size_t)T) || revise_fetch(d_kept_c.p, kept_c, (size_t)n) || revise_fetch(d_hits.p, hits, count)) return kFail;
            // the hits of every edit, in the row bucket's order: what the batch did
            for (uint64_t q = 0; q < count; q++) {
                out.copies_removed += hits[q];
                if (br.del[q]) { if (hits[q]) out.deleted++; else out.missed++; }
                else if (hits[q]) out.replaced++; else out.inserted++;
            }
            changed = nsets > 0 || out.copies_removed > 0;
            new_row_ptr.assign((size_t)T + 1, 0); new_col_ptr.assign((size_t)n + 1, 0);
            {
                std::vector<uint32_t> sets_r((size_t)T, 0u), sets_c((size_t)n, 0u);
                for (uint64_t e = 0; e < count; e++) if (!del || !del[e]) { sets_r[rows[e]]++; sets_c[cols[e]]++; }
                for (int i = 0; i < T; i++) new_row_ptr[(size_t)i + 1] = new_row_ptr[i] + kept_r[i] + sets_r[i];
                for (int j = 0; j < n; j++) new_col_ptr[(size_t)j + 1] = new_col_ptr[j] + kept_c[j] + sets_c[j];
            }
            new_nnz = new_row_ptr[T];
            if (new_col_ptr[n] != new_nnz || nnz - out.copies_removed + nsets != new_nnz) { set_error("revise: the two orientations of Y do not hold the same entries"); return kFail; }
            if (new_nnz >= (1ull << 32)) { set_error("revise: problem would exceed 32-bit device indices"); return kFail; }
            std::vector<uint32_t> np32((size_t)n + 1);
            for (int j = 0; j <= n; j++) np32[j] = (uint32_t)new_col_ptr[j];
            if (upload_ptr32(ptr2, (const size_t *)new_row_ptr.data(), (size_t)T + 1) || idx2.alloc(new_nnz, false) || val2.alloc(new_nnz, false) ||
                cptr2.upload(np32.data(), np32.size()) || cidx2.alloc(new_nnz, false) || cval2.alloc(new_nnz, false)) return kFail;
            ra.nptr = ptr2.p; ra.nidx = idx2.p; ra.nval = val2.p;
            ca.nptr = cptr2.p; ca.nidx = cidx2.p; ca.nval = cval2.p;
            hipLaunchKernelGGL(revise_kernel, dim3((T + 3) / 4), dim3(256), 0, stream, ra);
            hipLaunchKernelGGL(revise_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, ca);
            TRMF_HIP_CHECK(hipGetLastError());
            if (carry && changed) {   // the tables follow: untouched series copied, touched ones walked (old storage, W as it is)
                const size_t PK = adapt_packed(k);
                std::vector<uint32_t> touched;
                for (int j = 0; j < n; j++) if (bc.ptr[(size_t)j + 1] > bc.ptr[j]) touched.push_back((uint32_t)j);
                const std::vector<real> hom = forget_weights(ad_gamma, 0, T, T).w;
                DevBuf<uint32_t> d_list; DevBuf<real> om;
                SyncStreamOnExit drain_stats(stream);
                if (d_list.upload(touched.data(), touched.size()) || (!hom.empty() && om.upload(hom.data(), hom.size()))) return kFail;
                TRMF_HIP_CHECK(hipMemcpyAsync(ad_S[1 - ad_cur].p, ad_S[ad_cur].p, (size_t)n * PK * sizeof(real), hipMemcpyDeviceToDevice, stream));
                TRMF_HIP_CHECK(hipMemcpyAsync(ad_r[1 - ad_cur].p, ad_r[ad_cur].p, (size_t)n * k * sizeof(real), hipMemcpyDeviceToDevice, stream));
                SeriesReviseArgs sa{Yc_ptr.p, Yc_idx.p, Yc_val.p, d_list.p, dc.ptr.p, dc.idx.p, dc.val.p, dc.del.p, W.p, hom.empty() ? nullptr : om.p,
                                    ad_S[ad_cur].p, ad_r[ad_cur].p, ad_S[1 - ad_cur].p, ad_r[1 - ad_cur].p, (int)touched.size(), k, KP};
                if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(series_revise_kernel<decltype(N)::value>, dim3((unsigned)touched.size()), dim3(64), 0, stream, sa); }))
                    return unsupported_rank();
                TRMF_HIP_CHECK(hipGetLastError());
            }
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));      // (the buckets are locals)
            if (device_sum_squares(val2.p, new_nnz, &new_ysq)) return kFail;
        } else {
            const size_t N = (size_t)T * n;
            DevBuf<uint32_t> d_rows, d_cols; DevBuf<real> d_vals;
            SyncStreamOnExit drain_batch(stream);
            if (d_rows.upload(rows, count) || d_cols.upload(cols, count) || d_vals.upload(vals, count)) return kFail;
            DenseReviseArgs da{d_rows.p, d_cols.p, d_vals.p, nullptr, nullptr, (uint32_t)count, T, n};
            if (has_transform) {                        // the values are RAW data: edit the raw copy, re-derive below
                if (raw2.alloc(N, false)) return kFail;
                TRMF_HIP_CHECK(hipMemcpyAsync(raw2.p, Yraw.p, N * sizeof(real), hipMemcpyDeviceToDevice, stream));
                da.tn = raw2.p;
            } else {
                if (tn2.alloc(N, false) || nt2.alloc(N, false)) return kFail;
                TRMF_HIP_CHECK(hipMemcpyAsync(tn2.p, Yd_tn.p, N * sizeof(real), hipMemcpyDeviceToDevice, stream));
                TRMF_HIP_CHECK(hipMemcpyAsync(nt2.p, Yd_nt.p, N * sizeof(real), hipMemcpyDeviceToDevice, stream));
                da.tn = tn2.p; da.nt = nt2.p;
            }
            hipLaunchKernelGGL(dense_revise_kernel, dim3((unsigned)std::min<uint64_t>(4096, (count + 255) / 256)), dim3(256), 0, stream, da);
            TRMF_HIP_CHECK(hipGetLastError());
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));      // (the batch's device copies are locals)
            if (!has_transform && device_sum_squares(tn2.p, N, &new_ysq)) return kFail;    // over the new matrix, like a fresh session's
            out.replaced = count; out.copies_removed = count;
        }
        // ---- commit ----
        if (!dense) {
            Yr_ptr.swap(ptr2); Yr_idx.swap(idx2); Yr_val.swap(val2);
            Yc_ptr.swap(cptr2); Yc_idx.swap(cidx2); Yc_val.swap(cval2);
            host_row_ptr.swap(new_row_ptr); host_col_ptr.swap(new_col_ptr);
        } else if (has_transform) Yraw.swap(raw2);
        else { Yd_tn.swap(tn2); Yd_nt.swap(nt2); }
        if (ad_exists && changed) {
            if (carry) {
                ad_cur = 1 - ad_cur;
                for (int j = 0; j < n; j++) ad_cnt[j] = (uint32_t)(host_col_ptr[(size_t)j + 1] - host_col_ptr[j]);
            } else adapt_stale();                     // a column the tables absorbed has changed
        }
        out.stats_carried = carry ? 1 : 0;
        out.entries = new_nnz;
        if (res) *res = out;
        nnz = new_nnz; ysq_acc = new_ysq;
        if (dense && has_transform && apply_series_transform()) return kFail;     // current coefficients over the new raw matrix
        set_trYTY();
        iter = 0;
        if (gramx_mode != kGramxReplicate && comm->world > 1 && !test_env("TRMF_GRAMX")) { gramx_mode = kGramxMeasure; gramx_calls = 0; }
        if (fs_mode != kShardOff && comm->world > 1 && !test_env("TRMF_FSHARD")) { fs_mode = kShardMeasure; fs_calls = 0; }
        if (alloc_time_scratch()) return kFail;
        TRMF_HIP_CHECK(hipDeviceSynchronize());
        return autotune();
    }
    // ---- online updates (trmf_session_assimilate; online_kernels.hpp) ---------------------------------------------------------
    // Rows [first_row, T) of W re-solved in ascending order with H and Theta fixed (the caller has validated first_row, the lag set
    // and the rank).  Stage A rebuilds the Gram cache rows and right-hand sides of the range with the X phase's own builders -- every
    // X phase rebuilds the rows it reads before it reads them (xsolve: gram_x / xprepare_full), so nothing relies on their old
    // contents -- stage B factors all rows in parallel, stage C is the serial chain.  Everything lands in scratch; W changes by ONE
    // device copy after the flag has been read.  No collective: every rank holds the whole Y and W and computes the same bits.
    // A pivot that is not positive and finite is not a failure of this rank's task (res->bad_row names the row, nothing is
    // committed): the entry point reports it on the calling thread, so the barrier of a TRMF_DEVICES group stays whole.
    struct AssimResult {
        uint64_t rows = 0, entries = 0;
        double sq_err_before = 0, sq_err_after = 0;
        int bad_row = -1;
    };
    int assimilate(int first_row, AssimResult *res, real *Wout) {
        *res = AssimResult{};
        if (sync()) return kFail;
        const int nr = T - first_row;
        if (nr <= 0) return 0;
        FillStreamScope fill(stream);
        int chunk = kAssimChunk;
        if (const char *e = test_env("TRMF_ASSIM_CHUNK")) chunk = std::max(1, atoi(e));      // tests: several passes on a small shape
        chunk = std::min(chunk, nr);
        DevBuf<real> Wn, flat, U;
        DevBuf<int> flag;
        DevBuf<double> errs;
        SyncStreamOnExit drain(stream);
        if (Wn.alloc((size_t)nr * KP) || (Wout && flat.alloc((size_t)nr * k, false)) || U.alloc((size_t)chunk * k * k, false) ||
            errs.alloc((size_t)2 * nr, false) || new_flag(flag)) return kFail;
        if (rebuild_window_systems(first_row)) return kFail;      // stage A
        // stages B and C, a chunk of rows at a time
        const real lamAR = (real)lambdaAR, lam = (real)lambdaI + lamAR;
        int reach = 0;
        if (midx > 0 && assim_chain_lds_bytes(k, nlag, midx) <= kLdsMax && !test_env("TRMF_FORECAST_GLOBAL")) reach = midx;
        const size_t lds = assim_chain_lds_bytes(k, nlag, reach);
        if (allow_dyn_lds(assim_chain_kernel, lds, "online update")) return kFail;
        for (int r0 = first_row; r0 < T; r0 += chunk) {
            const int rows = std::min(chunk, T - r0);
            if (launch_factor(Gmat(), full ? (size_t)0 : xp.gstride, gpacked ? 1 : 0, U.p, flag.p, lam, r0, rows)) return kFail;
            AssimChainArgs ca{W.p, Wn.p, Wout ? flat.p : nullptr, Bv.p, U.p, lag_set.p, theta.p, lamAR, first_row, r0, rows, k, KP, NT, nlag, reach};
            hipLaunchKernelGGL(assim_chain_kernel, dim3(1), dim3(256), lds, stream, ca);
            TRMF_HIP_CHECK(hipGetLastError());
        }
        // the squared errors of the range with W as it is and as it will be
        if (launch_row_errors(H.p, W.p, Wn.p, first_row, errs.p, first_row, nr)) return kFail;
        int bad = kAssimNoBadRow;
        std::vector<double> herr((size_t)2 * nr);
        std::vector<real> hflat(Wout ? (size_t)nr * k : 0);
        TRMF_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(herr.data(), errs.p, herr.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (Wout) TRMF_HIP_CHECK(hipMemcpyAsync(hflat.data(), flat.p, hflat.size() * sizeof(real), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (bad != kAssimNoBadRow) { res->bad_row = bad; return 0; }
        if (commit_rows(first_row, Wn.p, nr)) return kFail;
        res->rows = (uint64_t)nr;
        res->entries = full ? (uint64_t)nr * (uint64_t)n : host_row_ptr[T] - host_row_ptr[first_row];
        for (int r = 0; r < nr; r++) { res->sq_err_before += herr[2 * r]; res->sq_err_after += herr[2 * r + 1]; }
        if (Wout) std::memcpy(Wout, hflat.data(), hflat.size() * sizeof(real));
        return 0;
    }
    // ---- outlier-robust online updates (trmf_session_assimilate_robust; robust_kernels.hpp) -------------------------------------
    // assimilate() with Huber weights (the caller has validated first_row, the lag set, the rank, the storage, c, the sweep count and
    // the n scales, which arrive as host values on every rank).  The weights depend on the iterate, so the Gram cache is of no use:
    // per row and sweep one part launch over the row's slices and one solve launch, 2 * sweeps * rows launches on the session's
    // stream with no host synchronisation before the one flag read.  Neither G nor Bv is touched.  Failure-atomic like assimilate():
    // rows, weights and sums land in scratch / host staging and are handed over after the flag has been read.
    struct RobustResult {
        uint64_t rows = 0, entries = 0, downweighted = 0;
        double weight_sum = 0, sq_err_before = 0, sq_err_after = 0;
        int bad_row = -1;
    };
    int assimilate_robust(int first_row, double c, int sweeps, const double *scale, RobustResult *res, real *Wout, real *weights_out) {
        *res = RobustResult{};
        if (sync()) return kFail;
        const int nr = T - first_row;
        if (nr <= 0) return 0;
        FillStreamScope fill(stream);
        int slice = kAssimRobustSlice;
        if (const char *e = test_env("TRMF_ASSIM_ROBUST_SLICE")) slice = std::max(1, atoi(e));      // tests: several slices per row on a small shape
        const uint64_t nw = dense ? (uint64_t)nr * (uint64_t)n : host_row_ptr[T] - host_row_ptr[first_row];
        auto slices_of = [&](int i) { const uint64_t len = dense ? (uint64_t)n : host_row_ptr[i + 1] - host_row_ptr[i]; return (int)((len + slice - 1) / slice); };
        int max_slices = 1;
        for (int i = first_row; i < T; i++) max_slices = std::max(max_slices, slices_of(i));
        const std::vector<real> hthr = huber_thresholds(c, scale);
        DevBuf<real> Wn, flat, wcur, prior, thr, wts, slab;
        DevBuf<int> flag;
        DevBuf<double> errs, slab_d, rowsum;
        SyncStreamOnExit drain(stream);
        if (Wn.alloc((size_t)nr * KP) || (Wout && flat.alloc((size_t)nr * k, false)) || wcur.alloc(KP) || prior.alloc(KP) || thr.upload(hthr.data(), n) ||
            wts.alloc(nw, false) || slab.alloc((size_t)max_slices * assim_robust_slot_reals(KP), false) || slab_d.alloc((size_t)2 * max_slices, false) ||
            rowsum.alloc((size_t)2 * nr, false) || errs.alloc((size_t)2 * nr, false) || new_flag(flag)) return kFail;
        const YStore y = y_rows();
        AssimRobustArgs ra{y.ptr, y.idx, y.val, y.dense, H.p, W.p, Wn.p,
                           Wout ? flat.p : nullptr, wcur.p, prior.p, thr.p, wts.p, slab.p, slab_d.p, rowsum.p, lag_set.p, theta.p, flag.p,
                           (real)lambdaI + (real)lambdaAR, (real)lambdaAR, first_row, T, first_row, n, k, KP, nlag, slice, 0, 0};
        hipLaunchKernelGGL(assim_robust_prior_kernel, dim3(1), dim3(64), 0, stream, ra);
        TRMF_HIP_CHECK(hipGetLastError());
        for (int i = first_row; i < T; i++) {
            ra.i = i; ra.nslices = slices_of(i);
            for (int s = 1; s <= sweeps; s++) {
                ra.last = s == sweeps ? 1 : 0;
                if (!with_nt(NT, [&](auto N) {
                        if (ra.nslices > 0) hipLaunchKernelGGL(assim_robust_part_kernel<decltype(N)::value>, dim3(ra.nslices), dim3(256), 0, stream, ra);
                        hipLaunchKernelGGL(assim_robust_solve_kernel<decltype(N)::value>, dim3(1), dim3(256), 0, stream, ra);
                    })) return unsupported_rank();
            }
            TRMF_HIP_CHECK(hipGetLastError());
        }
        // the squared errors of the range with W as it is and as it will be (unweighted)
        if (launch_row_errors(H.p, W.p, Wn.p, first_row, errs.p, first_row, nr)) return kFail;
        int bad = kAssimNoBadRow;
        std::vector<double> herr((size_t)2 * nr), hsum((size_t)2 * nr);
        std::vector<real> hflat(Wout ? (size_t)nr * k : 0), hwts(weights_out ? (size_t)nw : 0);
        TRMF_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(herr.data(), errs.p, herr.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(hsum.data(), rowsum.p, hsum.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (Wout) TRMF_HIP_CHECK(hipMemcpyAsync(hflat.data(), flat.p, hflat.size() * sizeof(real), hipMemcpyDeviceToHost, stream));
        if (weights_out && nw) TRMF_HIP_CHECK(hipMemcpyAsync(hwts.data(), wts.p, hwts.size() * sizeof(real), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (bad != kAssimNoBadRow) { res->bad_row = bad; return 0; }
        if (commit_rows(first_row, Wn.p, nr)) return kFail;
        res->rows = (uint64_t)nr;
        res->entries = nw;
        double down = 0;
        for (int r = 0; r < nr; r++) {                              // row order: the same sums on every rank and every call
            res->sq_err_before += herr[2 * r]; res->sq_err_after += herr[2 * r + 1];
            down += hsum[2 * r]; res->weight_sum += hsum[2 * r + 1];
        }
        res->downweighted = (uint64_t)down;
        if (Wout) std::memcpy(Wout, hflat.data(), hflat.size() * sizeof(real));
        if (weights_out && nw) std::memcpy(weights_out, hwts.data(), hwts.size() * sizeof(real));
        return 0;
    }
    // ---- the fixed-interval smoother (trmf_session_smooth; smooth_kernels.hpp) ------------------------------------------------------
    // Rows [first_row, T) of W become the joint minimiser of the objective restricted to them (the caller has validated first_row,
    // the lag set, the rank, the window against the cap, rtol and max_iter).  Stage A is assimilate()'s: Grams and right-hand sides
    // of the window by the X phase's builders, the factors of ALL rows at once (they precondition every step).  Stage B is the
    // PCG, three launches per step on the session's stream; the stop is decided on the device, and the host only follows it
    // through one pinned word: it stays kSmoothLook steps ahead of the device and stops enqueuing when it sees the stop (launches
    // after the stop return at once, so the bits do not depend on how far ahead it was).  A word that does not move for 2 s is answered
    // by a stream synchronisation and a re-read, never by enqueuing the remaining steps blind.  Everything lands in scratch; W changes
    // by ONE device copy after the flag and the sums have been read.  A call that reaches max_iter commits as well: every CG
    // iterate lowers J_win.  No collective: every rank holds the whole Y and W and computes the same bits.
    struct SmoothResult {
        uint64_t rows = 0, entries = 0;
        int iterations = 0, converged = 0;
        double residual = 0, sq_err_before = 0, sq_err_after = 0, objective_before = 0, objective_after = 0;
        int bad_row = -1;
    };
    static int smooth_max_rows() {
        int cap = kSmoothMaxRows;
        if (const char *e = test_env("TRMF_SMOOTH_MAX_ROWS")) cap = std::max(1, atoi(e));      // tests: the refusal on a small shape
        return cap;
    }
    static constexpr int kSmoothLook = 4;
    unsigned int smooth_seq = 0;
    // The PCG of one system: INIT, the steps with the pinned-word pacing described above, and the closing stop test.  `sa` carries
    // the system (W, x0, Bv, G, U), the vectors and a zeroed SmoothState of this solve's own; the word and its sequence number are set here.
    int smooth_pcg(SmoothArgs &sa, int max_iter) {
        const int m = sa.m;
        unsigned int *note = cg_note + 8;                       // a word of its own in the X-solve's pinned line
        const unsigned int seq = ++smooth_seq & 0x1ffffu;
        __atomic_store_n(note, 0u, __ATOMIC_RELEASE);
        sa.note = note; sa.note_seq = seq;
        sa.lds_theta = smooth_theta_lds_bytes(nlag) <= kLdsDefault && !test_env("TRMF_FORECAST_GLOBAL") ? 1 : 0;
        const size_t lds_th = sa.lds_theta ? smooth_theta_lds_bytes(nlag) : 0, lds_up = smooth_update_lds_bytes(k);
        const dim3 rows4((m + 3) / 4);
        auto step = [&](int mode, int j) {
            hipLaunchKernelGGL(smooth_ar_kernel, mode == SMOOTH_LAST ? dim3(1) : rows4, dim3(256), lds_th, stream, sa, mode, j);
            if (mode == SMOOTH_LAST) return;
            hipLaunchKernelGGL(smooth_apply_kernel, rows4, dim3(256), lds_th, stream, sa, mode, j);
            hipLaunchKernelGGL(smooth_update_kernel, dim3(m), dim3(64), lds_up, stream, sa, mode, j);
        };
        step(SMOOTH_INIT, 0);
        TRMF_HIP_CHECK(hipGetLastError());
        bool note_live = true;
        for (int j = 0; j < max_iter; j++) {
            step(SMOOTH_STEP, j);
            TRMF_HIP_CHECK(hipGetLastError());
            if (j < kSmoothLook) continue;
            if (!note_live) {                                   // without the word: read the stop itself every kSmoothLook steps
                if (j % kSmoothLook) continue;
                int done = 0;
                TRMF_HIP_CHECK(hipMemcpyAsync(&done, &sa.st->done, sizeof(int), hipMemcpyDeviceToHost, stream));
                TRMF_HIP_CHECK(hipStreamSynchronize(stream));
                if (done) break;
                continue;
            }
            // wait until step j - kSmoothLook has been decided: the device is then still kSmoothLook steps behind the queue's end
            const unsigned int need = (unsigned int)(j - kSmoothLook);
            const double t_wait = now_s();
            bool stopped = false;
            for (unsigned int spins = 0;; spins++) {
                const unsigned int v = __atomic_load_n(note, __ATOMIC_ACQUIRE);
                if ((v >> 15) == seq) {
                    if (v & 1u) { stopped = true; break; }
                    if (((v >> 1) & 0x3fffu) >= need) break;
                }
                if ((spins & 1023u) == 1023u && now_s() - t_wait > 2.0) {
                    // the word has not moved for 2 s (a loaded device): drain the queue and read it again instead of running ahead blind
                    TRMF_HIP_CHECK(hipStreamSynchronize(stream));
                    const unsigned int w = __atomic_load_n(note, __ATOMIC_ACQUIRE);
                    if ((w >> 15) != seq) note_live = false;        // the device never wrote it: pace by synchronising from here on
                    stopped = (w >> 15) == seq && (w & 1u);
                    break;
                }
                __builtin_ia32_pause();
            }
            if (stopped) break;
        }
        step(SMOOTH_LAST, max_iter);                             // the last step's r.z and its stop test (a no-op after a stop)
        return 0;
    }
    int smooth(int first_row, double rtol, int max_iter, SmoothResult *res, real *Wout) {
        *res = SmoothResult{};
        if (sync()) return kFail;
        const int m = T - first_row;
        if (m <= 0) return 0;
        if (ensure_cg_note()) { set_error("smooth: no pinned host memory for the word the stop is followed through"); return kFail; }
        FillStreamScope fill(stream);
        DevBuf<real> Wn, flat, U, vec, part;
        DevBuf<int> flag;
        DevBuf<double> errs, objs;
        DevBuf<SmoothState> state;
        SyncStreamOnExit drain(stream);
        if (Wn.alloc((size_t)m * KP) || (Wout && flat.alloc((size_t)m * k, false)) || U.alloc((size_t)m * k * k, false) || vec.alloc((size_t)7 * m * 64) ||
            part.alloc((size_t)2 * m) || errs.alloc((size_t)2 * m, false) || objs.alloc((size_t)4 * m, false) || state.alloc(1) || new_flag(flag))
            return kFail;
        if (rebuild_window_systems(first_row)) return kFail;      // stage A
        const real lamAR = (real)lambdaAR, lamI = (real)lambdaI;
        const size_t gstride = full ? (size_t)0 : xp.gstride;
        if (launch_factor(Gmat(), gstride, gpacked ? 1 : 0, U.p, flag.p, lamI + lamAR, first_row, m)) return kFail;
        TRMF_HIP_CHECK(hipGetLastError());
        // stage B: the system is the session's own cache, read from row first_row on
        SmoothArgs sa = smooth_args(first_row, m, rtol, U.p, vec.p, part.p, flag.p);
        sa.x0 = W.p + (size_t)first_row * KP; sa.Bv = Bv.p; sa.G = Gmat(); sa.gstride = gstride; sa.packed = gpacked ? 1 : 0; sa.grow = first_row;
        sa.st = state.p;
        if (smooth_pcg(sa, max_iter)) return kFail;
        {
            SmoothFinishArgs fa{W.p, sa.x, lag_set.p, theta.p, Wn.p, Wout ? flat.p : nullptr, objs.p, first_row, m, k, KP, NT, nlag};
            hipLaunchKernelGGL(smooth_finish_kernel, dim3((m + 3) / 4), dim3(256), 0, stream, fa);
            if (launch_row_errors(H.p, W.p, Wn.p, first_row, errs.p, first_row, m)) return kFail;
        }
        int bad = kAssimNoBadRow;
        SmoothState hst{};
        std::vector<double> herr((size_t)2 * m), hobj((size_t)4 * m);
        std::vector<real> hflat(Wout ? (size_t)m * k : 0);
        TRMF_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(&hst, state.p, sizeof(SmoothState), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(herr.data(), errs.p, herr.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(hobj.data(), objs.p, hobj.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (Wout) TRMF_HIP_CHECK(hipMemcpyAsync(hflat.data(), flat.p, hflat.size() * sizeof(real), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (bad != kAssimNoBadRow) { res->bad_row = bad; return 0; }
        if (commit_rows(first_row, Wn.p, m)) return kFail;
        res->rows = (uint64_t)m;
        res->entries = full ? (uint64_t)m * (uint64_t)n : host_row_ptr[T] - host_row_ptr[first_row];
        res->converged = hst.done ? 1 : 0;
        res->iterations = hst.done ? hst.iters : max_iter;
        const double rz_end = hst.rz[res->iterations & 1];
        res->residual = hst.rz0 > 0 ? std::sqrt(std::max(rz_end, 0.0) / hst.rz0) : 0.0;
        double w2[2] = {0, 0}, e2[2] = {0, 0};
        for (int r = 0; r < m; r++) {                               // row order: the same sums on every rank and every call
            res->sq_err_before += herr[2 * r]; res->sq_err_after += herr[2 * r + 1];
            w2[0] += hobj[4 * r]; e2[0] += hobj[4 * r + 1]; w2[1] += hobj[4 * r + 2]; e2[1] += hobj[4 * r + 3];
        }
        res->objective_before = 0.5 * (res->sq_err_before + (double)lamI * w2[0] + (double)lamAR * e2[0]);
        res->objective_after = 0.5 * (res->sq_err_after + (double)lamI * w2[1] + (double)lamAR * e2[1]);
        if (Wout) std::memcpy(Wout, hflat.data(), hflat.size() * sizeof(real));
        return 0;
    }
    // ---- the robust fixed-interval smoother (trmf_session_smooth_robust; smooth_robust_kernels.hpp) -----------------------------------
    // smooth() on the Huber form of the objective by `sweeps` rounds of reweighting (the caller has validated what smooth() and
    // assimilate_robust() ask for; the n scales arrive as host values on every rank).  Per sweep: one part launch over the items of
    // the whole window and one fold launch build the weighted G_i, b_i in scratch of this call's own (the session's G / Bv cache is
    // not touched), assim_factor_kernel factors the blocks, smooth_pcg() solves from the rows of the sweep before, and
    // smooth_finish_kernel lays the rows out for the next sweep's part kernel.  Two more part launches in score-only mode give
    // J_rob's data term before and after.  The host synchronises only where smooth_pcg() follows its word; W changes by ONE device
    // copy after the flag and the sums have been read.  A sweep that reaches max_iter is kept (converged = 0): every CG iterate
    // lowers the sweep's majoriser of J_rob.
    struct RobustSmoothResult {
        uint64_t rows = 0, entries = 0, downweighted = 0;
        int sweeps = 0, iterations = 0, converged = 0;
        double residual = 0, weight_sum = 0, sq_err_before = 0, sq_err_after = 0, objective_before = 0, objective_after = 0;
        int bad_row = -1;
    };
    int smooth_robust(int first_row, double c, int sweeps, const double *scale, double rtol, int max_iter, RobustSmoothResult *res, real *Wout,
                      real *weights_out) {
        *res = RobustSmoothResult{};
        if (sync()) return kFail;
        const int m = T - first_row;
        if (m <= 0) return 0;
        if (ensure_cg_note()) { set_error("smooth_robust: no pinned host memory for the word the stop is followed through"); return kFail; }
        FillStreamScope fill(stream);
        int slice = kSmoothRobustSlice;
        if (const char *e = test_env("TRMF_SMOOTH_ROBUST_SLICE")) slice = std::max(1, atoi(e));      // tests: several items per row on a small shape
        const uint64_t nw = dense ? (uint64_t)m * (uint64_t)n : host_row_ptr[T] - host_row_ptr[first_row];
        // the items: a row's entries in spans that depend on its length only
        std::vector<uint32_t> hitems, hrow((size_t)m + 1);
        for (int r = 0; r < m; r++) {
            hrow[r] = (uint32_t)(hitems.size() / 3);
            const uint64_t e0 = dense ? 0 : host_row_ptr[first_row + r], e1 = dense ? (uint64_t)n : host_row_ptr[first_row + r + 1];
            const uint64_t span = smooth_robust_span(e1 - e0, slice);
            for (uint64_t b = e0; b < e1; b += span) {
                hitems.push_back((uint32_t)r); hitems.push_back((uint32_t)b); hitems.push_back((uint32_t)std::min(b + span, e1));
            }
        }
        const uint32_t nitems = (uint32_t)(hitems.size() / 3);
        hrow[m] = nitems;
        if (hitems.empty()) hitems.assign(3, 0u);
        const std::vector<real> hthr = huber_thresholds(c, scale);
        DevBuf<real> xc, flat, U, vec, part, thr, wts, slab, Gs, bs;
        DevBuf<uint32_t> d_items, d_row;
        DevBuf<int> flag;
        DevBuf<double> objs, slab_d, score, rowsum;
        DevBuf<SmoothState> state;
        SyncStreamOnExit drain(stream);
        const size_t ni = std::max<size_t>(nitems, 1);
        if (xc.alloc((size_t)m * KP, false) || (Wout && flat.alloc((size_t)m * k, false)) || U.alloc((size_t)m * k * k, false) || vec.alloc((size_t)7 * m * 64) ||
            part.alloc((size_t)2 * m) || thr.upload(hthr.data(), n) || wts.alloc(std::max<uint64_t>(nw, 1), false) ||
            slab.alloc(ni * smooth_robust_slot_reals(KP), false) || Gs.alloc((size_t)m * k * k, false) || bs.alloc((size_t)m * KP, false) ||
            d_items.upload(hitems.data(), hitems.size()) || d_row.upload(hrow.data(), hrow.size()) ||
            objs.alloc((size_t)4 * m, false) || slab_d.alloc(ni * kSmoothRobustSlotD, false) || score.alloc(2 * ni * kSmoothRobustSlotD, false) ||
            rowsum.alloc((size_t)2 * m, false) || state.alloc((size_t)sweeps) || new_flag(flag)) return kFail;
        TRMF_HIP_CHECK(hipMemcpyAsync(xc.p, W.p + (size_t)first_row * KP, (size_t)m * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        const real lamAR = (real)lambdaAR, lamI = (real)lambdaI;
        const YStore y = y_rows();
        SmoothRobustArgs ra{y.ptr, y.idx, y.val, y.dense, H.p, xc.p, thr.p,
                            wts.p, d_items.p, d_row.p, slab.p, slab_d.p, Gs.p, bs.p, rowsum.p, first_row, m, n, k, KP, 0};
        auto part_launch = [&](int score_only, double *sums) {
            if (!nitems) return true;
            SmoothRobustArgs a = ra;
            a.score = score_only; a.slab_d = sums;
            return with_nt(NT, [&](auto N) { hipLaunchKernelGGL(smooth_robust_part_kernel<decltype(N)::value>, dim3(nitems), dim3(256), 0, stream, a); });
        };
        if (!part_launch(1, score.p)) return unsupported_rank();
        // the system is this call's own tables of the window, read from row 0 on
        SmoothArgs sa = smooth_args(first_row, m, rtol, U.p, vec.p, part.p, flag.p);
        sa.x0 = xc.p; sa.Bv = bs.p; sa.G = Gs.p; sa.gstride = (size_t)k * k; sa.packed = 0; sa.grow = 0;
        const dim3 rows4((m + 3) / 4);
        for (int s = 0; s < sweeps; s++) {
            if (!part_launch(0, slab_d.p)) return unsupported_rank();
            if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(smooth_robust_fold_kernel<decltype(N)::value>, dim3(m), dim3(256), 0, stream, ra); }))
                return unsupported_rank();
            if (launch_factor(Gs.p, (size_t)k * k, 0, U.p, flag.p, lamI + lamAR, 0, m)) return kFail;
            TRMF_HIP_CHECK(hipGetLastError());
            sa.st = state.p + s;
            if (smooth_pcg(sa, max_iter)) return kFail;
            SmoothFinishArgs fin{W.p, sa.x, lag_set.p, theta.p, xc.p, Wout && s == sweeps - 1 ? flat.p : nullptr, objs.p, first_row, m, k, KP, NT, nlag};
            hipLaunchKernelGGL(smooth_finish_kernel, rows4, dim3(256), 0, stream, fin);
            TRMF_HIP_CHECK(hipGetLastError());
        }
        if (!part_launch(1, score.p + ni * kSmoothRobustSlotD)) return unsupported_rank();
        TRMF_HIP_CHECK(hipGetLastError());
        int bad = kAssimNoBadRow;
        std::vector<SmoothState> hst((size_t)sweeps);
        std::vector<double> hobj((size_t)4 * m), hsum((size_t)2 * m), hscore(2 * ni * kSmoothRobustSlotD, 0.0);
        std::vector<real> hflat(Wout ? (size_t)m * k : 0), hwts(weights_out ? (size_t)nw : 0);
        TRMF_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(hst.data(), state.p, hst.size() * sizeof(SmoothState), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(hobj.data(), objs.p, hobj.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(hsum.data(), rowsum.p, hsum.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (nitems) TRMF_HIP_CHECK(hipMemcpyAsync(hscore.data(), score.p, hscore.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (Wout) TRMF_HIP_CHECK(hipMemcpyAsync(hflat.data(), flat.p, hflat.size() * sizeof(real), hipMemcpyDeviceToHost, stream));
        if (weights_out && nw) TRMF_HIP_CHECK(hipMemcpyAsync(hwts.data(), wts.p, hwts.size() * sizeof(real), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (bad != kAssimNoBadRow) { res->bad_row = first_row + bad; return 0; }
        if (commit_rows(first_row, xc.p, m)) return kFail;
        res->rows = (uint64_t)m;
        res->entries = nw;
        res->sweeps = sweeps;
        res->converged = 1;
        for (int s = 0; s < sweeps; s++) {
            const int it = hst[s].done ? hst[s].iters : max_iter;
            res->iterations += it;
            if (!hst[s].done) res->converged = 0;
            if (s == sweeps - 1) res->residual = hst[s].rz0 > 0 ? std::sqrt(std::max(hst[s].rz[it & 1], 0.0) / hst[s].rz0) : 0.0;
        }
        double down = 0, w2[2] = {0, 0}, e2[2] = {0, 0}, rho[2] = {0, 0};
        for (int r = 0; r < m; r++) {                               // row order, then item order: the same sums on every rank and every call
            down += hsum[2 * r]; res->weight_sum += hsum[2 * r + 1];
            w2[0] += hobj[4 * r]; e2[0] += hobj[4 * r + 1]; w2[1] += hobj[4 * r + 2]; e2[1] += hobj[4 * r + 3];
        }
        for (uint32_t it = 0; it < nitems; it++) {
            const double *a0 = hscore.data() + (size_t)it * kSmoothRobustSlotD, *a1 = a0 + ni * kSmoothRobustSlotD;
            rho[0] += a0[2]; res->sq_err_before += a0[3]; rho[1] += a1[2]; res->sq_err_after += a1[3];
        }
        res->downweighted = (uint64_t)down;
        res->objective_before = rho[0] + 0.5 * ((double)lamI * w2[0] + (double)lamAR * e2[0]);
        res->objective_after = rho[1] + 0.5 * ((double)lamI * w2[1] + (double)lamAR * e2[1]);
        if (Wout) std::memcpy(Wout, hflat.data(), hflat.size() * sizeof(real));
        if (weights_out && nw) std::memcpy(weights_out, hwts.data(), hwts.size() * sizeof(real));
        return 0;
    }
    // ---- online loading updates (trmf_session_series_stats_init / _adapt_series; adapt_kernels.hpp) -----------------------------------
    // One pass for both calls (the caller has validated the rank, gamma and the state of the tables).  init: the tables over all
    // rows from zero, H untouched (the pass's solve is discarded with its flag).  Otherwise: the active generation scaled by gamma^m
    // plus the entries not yet absorbed, then every h_j.  Everything lands in the inactive generation and in scratch; the generation,
    // the absorbed counts and H move after the one flag read.  No collective: every rank holds the whole Y and W and computes the
    // same bits.  A bad pivot or a pool that cannot hold the tables is not a failure of this rank's task (res->bad_series /
    // res->no_memory; nothing is committed): the entry point reports it on the calling thread, so the barrier of a TRMF_DEVICES
    // group stays whole.
    struct AdaptResult {
        uint64_t series = 0, rows = 0, entries = 0;
        double sq_err_before = 0, sq_err_after = 0, max_abs_change = 0;
        int bad_series = -1, no_memory = 0;
    };
    int adapt_series(bool init, double forget, AdaptResult *res, real *Hout) {
        *res = AdaptResult{};
        if (sync()) return kFail;
        FillStreamScope fill(stream);
        const double gam = init ? forget : ad_gamma;
        const int row0 = init ? 0 : ad_rows, m = T - row0;
        const size_t PK = adapt_packed(k), nS = full ? PK : (size_t)n * PK, nR = (size_t)n * k;
        if (init && (!ad_exists || ad_S[0].n != nS || ad_r[0].n != nR)) {      // (change_series releases stale tables: the series count moved)
            if (ad_S[0].alloc(nS, false) || ad_S[1].alloc(nS, false) || ad_r[0].alloc(nR, false) || ad_r[1].alloc(nR, false)) {
                for (int q = 0; q < 2; q++) { ad_S[q].release(); ad_r[q].release(); }
                res->no_memory = 1;
                return 0;
            }
            ad_exists = true; ad_valid = false; ad_cur = 0;
        }
        const int in = ad_cur, out = 1 - ad_cur;
        const Forgetting fg = forget_weights(gam, row0, m, T);
        const std::vector<real> &hom = fg.w;
        // sparse storage: where each column's walk starts; the init pass cuts long columns into items
        std::vector<uint32_t> hstart, hfirst, hitems;
        if (!dense) {
            hstart.resize((size_t)n);
            for (int j = 0; j < n; j++) hstart[j] = (uint32_t)(host_col_ptr[j] + (init ? 0u : ad_cnt[j]));
        }
        const uint32_t nitems = init && !full ? cut_long_columns(host_col_ptr.data(), n, nnz, hfirst, hitems) : 0u;
        DevBuf<real> Hn, chg, mx, om, slab, U;
        DevBuf<uint32_t> d_start, d_first, d_items;
        DevBuf<int> flag;
        DevBuf<double> errs;
        SyncStreamOnExit drain(stream);
        if (Hn.alloc((size_t)n * KP) || chg.alloc(n, false) || mx.alloc(1) || errs.alloc((size_t)4 * std::max(m, 1), false) ||
            (!hom.empty() && om.upload(hom.data(), hom.size())) || (!dense && d_start.upload(hstart.data(), hstart.size())) ||
            (nitems && (d_first.upload(hfirst.data(), hfirst.size()) || d_items.upload(hitems.data(), hitems.size()) ||
                        slab.alloc((size_t)nitems * adapt_part_reals(k), false))) ||
            (full && U.alloc((size_t)k * k, false)) || new_flag(flag)) return kFail;
        const real *omp = hom.empty() ? nullptr : om.p;
        const real *Sin = init ? nullptr : ad_S[in].p, *rin = init ? nullptr : ad_r[in].p;
        if (!full) {
            AdaptArgs a{Yc_ptr.p, Yc_idx.p, Yc_val.p, d_start.p, W.p, omp, Sin, rin, ad_S[out].p, ad_r[out].p, nitems ? d_first.p : nullptr,
                        nitems ? d_items.p : nullptr, nitems ? slab.p : nullptr, H.p, Hn.p, chg.p, flag.p, fg.decay, (real)lambdaI, row0, n, k, KP};
            if (launch_series_fit(a, nitems)) return kFail;
        } else {
            const YStore y = y_cols();
            AdaptFullArgs a{y.ptr, y.idx, y.val, dense ? nullptr : d_start.p, y.dense, W.p, omp, Sin, rin, ad_S[out].p, ad_r[out].p, U.p, H.p, Hn.p, chg.p,
                            fg.decay, row0, T, n, k, KP, NT};
            if (launch_series_fit_full(a, U.p, flag.p)) return kFail;
        }
        TRMF_HIP_CHECK(hipGetLastError());
        if (init) {                                                 // H stays: only the tables are handed over
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));
            ad_cur = out; ad_valid = true; ad_gamma = forget; ad_rows = T;
            if (!dense) { ad_cnt.resize((size_t)n); for (int j = 0; j < n; j++) ad_cnt[j] = (uint32_t)(host_col_ptr[j + 1] - host_col_ptr[j]); }
            res->series = (uint64_t)n; res->rows = (uint64_t)T;
            res->entries = full ? (uint64_t)T * (uint64_t)n : nnz;
            return 0;
        }
        hipLaunchKernelGGL(adapt_max_kernel, dim3(1), dim3(256), 0, stream, chg.p, n, mx.p);
        // the squared errors of the absorbed rows with H as it is and as it will be (assim_err_kernel's reading of an entry)
        if (m > 0 && (launch_row_errors(H.p, W.p, W.p, 0, errs.p, row0, m) || launch_row_errors(Hn.p, W.p, W.p, 0, errs.p + (size_t)2 * m, row0, m))) return kFail;
        TRMF_HIP_CHECK(hipGetLastError());
        int bad = kAdaptNoBadSeries;
        real hmx = 0;
        std::vector<double> herr((size_t)4 * std::max(m, 1), 0.0);
        TRMF_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(&hmx, mx.p, sizeof(real), hipMemcpyDeviceToHost, stream));
        if (m > 0) TRMF_HIP_CHECK(hipMemcpyAsync(herr.data(), errs.p, (size_t)4 * m * sizeof(double), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (bad != kAdaptNoBadSeries) { res->bad_series = bad; return 0; }
        if (Hout && download_padded(Hn, Hout, (size_t)n)) return kFail;
        if (commit_loadings(Hn.p)) return kFail;
        ad_cur = out; ad_rows = T;
        if (!dense) for (int j = 0; j < n; j++) ad_cnt[j] = (uint32_t)(host_col_ptr[j + 1] - host_col_ptr[j]);
        res->series = (uint64_t)n; res->rows = (uint64_t)m;
        res->entries = full ? (uint64_t)m * (uint64_t)n : host_row_ptr[T] - host_row_ptr[row0];
        for (int r = 0; r < m; r++) { res->sq_err_before += herr[2 * r]; res->sq_err_after += herr[(size_t)2 * m + 2 * r]; }
        res->max_abs_change = (double)hmx;
        return 0;
    }
    // ---- robust online loading updates (trmf_session_adapt_series_robust; adapt_robust_kernels.hpp) -----------------------------------
    // adapt_series() with Huber weights on the entries not yet absorbed (the caller has validated the rank, the storage -- sparse
    // with missing != 0 --, the state of the tables, c, the sweep count and the n scales, which arrive as host values on every
    // rank).  One launch of the per-series kernel runs every sweep; one launch of the objective kernel gives J_j before and after.
    // Everything lands in the inactive generation and in scratch; the generation, the absorbed counts and H move after the one
    // flag read.  The weights always come back to the host: downweighted and weight_sum are folded from them in series order.
    struct RobustAdaptResult {
        uint64_t series = 0, rows = 0, entries = 0, downweighted = 0;
        double sq_err_before = 0, sq_err_after = 0, max_abs_change = 0, weight_sum = 0, objective_before = 0, objective_after = 0;
        int bad_series = -1;
    };
    int adapt_series_robust(double c, int sweeps, const double *scale, RobustAdaptResult *res, real *Hout, uint64_t *wptr_out, uint32_t *wrows_out,
                            real *weights_out) {
        *res = RobustAdaptResult{};
        if (sync()) return kFail;
        FillStreamScope fill(stream);
        const double gam = ad_gamma;
        const int row0 = ad_rows, m = T - row0;
        const int in = ad_cur, out = 1 - ad_cur;
        const Forgetting fg = forget_weights(gam, row0, m, T);
        const std::vector<real> &hom = fg.w;
        std::vector<uint32_t> hstart((size_t)n), hwptr((size_t)n + 1);
        const std::vector<real> hthr = huber_thresholds(c, scale);
        hwptr[0] = 0;
        for (int j = 0; j < n; j++) {
            hstart[j] = (uint32_t)(host_col_ptr[j] + ad_cnt[j]);
            hwptr[j + 1] = hwptr[j] + (uint32_t)(host_col_ptr[j + 1] - host_col_ptr[j] - ad_cnt[j]);
        }
        const size_t nw = hwptr[n];
        DevBuf<real> Hn, chg, mx, om, thr, wts;
        DevBuf<uint32_t> d_start, d_wptr, wrw;
        DevBuf<int> flag;
        DevBuf<double> errs, obj;
        SyncStreamOnExit drain(stream);
        if (Hn.alloc((size_t)n * KP) || chg.alloc(n, false) || mx.alloc(1) || errs.alloc((size_t)4 * std::max(m, 1), false) ||
            (!hom.empty() && om.upload(hom.data(), hom.size())) || d_start.upload(hstart.data(), hstart.size()) ||
            d_wptr.upload(hwptr.data(), hwptr.size()) || thr.upload(hthr.data(), hthr.size()) || wts.alloc(std::max<size_t>(nw, 1), false) ||
            wrw.alloc(std::max<size_t>(nw, 1), false) || obj.alloc((size_t)2 * n, false) || new_flag(flag)) return kFail;
        AdaptRobustArgs a{Yc_ptr.p, Yc_idx.p, Yc_val.p, d_start.p, W.p, hom.empty() ? nullptr : om.p, ad_S[in].p, ad_r[in].p, ad_S[out].p, ad_r[out].p,
                          H.p, Hn.p, chg.p, flag.p, thr.p, d_wptr.p, wts.p, wrw.p, obj.p, fg.decay, (real)lambdaI, row0, n, k, KP, NT, sweeps};
        if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(adapt_robust_series_kernel<decltype(N)::value>, dim3(n), dim3(64), 0, stream, a); }))
            return unsupported_rank();
        hipLaunchKernelGGL(adapt_robust_objective_kernel, dim3(n), dim3(64), 0, stream, a);
        hipLaunchKernelGGL(adapt_max_kernel, dim3(1), dim3(256), 0, stream, chg.p, n, mx.p);
        // the squared errors of the absorbed rows with H as it is and as it will be (unweighted; adapt_series' sums)
        if (m > 0 && (launch_row_errors(H.p, W.p, W.p, 0, errs.p, row0, m) || launch_row_errors(Hn.p, W.p, W.p, 0, errs.p + (size_t)2 * m, row0, m))) return kFail;
        TRMF_HIP_CHECK(hipGetLastError());
        int bad = kAdaptNoBadSeries;
        real hmx = 0;
        std::vector<double> herr((size_t)4 * std::max(m, 1), 0.0), hobj((size_t)2 * n);
        std::vector<real> hwts(nw);
        std::vector<uint32_t> hwrw(wrows_out ? nw : 0);
        TRMF_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(&hmx, mx.p, sizeof(real), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(hobj.data(), obj.p, hobj.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (m > 0) TRMF_HIP_CHECK(hipMemcpyAsync(herr.data(), errs.p, (size_t)4 * m * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (nw) TRMF_HIP_CHECK(hipMemcpyAsync(hwts.data(), wts.p, nw * sizeof(real), hipMemcpyDeviceToHost, stream));
        if (wrows_out && nw) TRMF_HIP_CHECK(hipMemcpyAsync(hwrw.data(), wrw.p, nw * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (bad != kAdaptNoBadSeries) { res->bad_series = bad; return 0; }
        if (Hout && download_padded(Hn, Hout, (size_t)n)) return kFail;
        if (commit_loadings(Hn.p)) return kFail;
        ad_cur = out; ad_rows = T;
        for (int j = 0; j < n; j++) ad_cnt[j] = (uint32_t)(host_col_ptr[j + 1] - host_col_ptr[j]);
        res->series = (uint64_t)n; res->rows = (uint64_t)m;
        res->entries = (uint64_t)nw;
        for (int r = 0; r < m; r++) { res->sq_err_before += herr[2 * r]; res->sq_err_after += herr[(size_t)2 * m + 2 * r]; }
        for (int j = 0; j < n; j++) { res->objective_before += hobj[2 * j]; res->objective_after += hobj[2 * j + 1]; }       // series order
        for (size_t e = 0; e < nw; e++) { res->downweighted += hwts[e] < real(1) ? 1u : 0u; res->weight_sum += (double)hwts[e]; }
        res->max_abs_change = (double)hmx;
        if (wptr_out) for (int j = 0; j <= n; j++) wptr_out[j] = (uint64_t)hwptr[j];
        if (wrows_out && nw) std::memcpy(wrows_out, hwrw.data(), nw * sizeof(uint32_t));
        if (weights_out && nw) std::memcpy(weights_out, hwts.data(), nw * sizeof(real));
        return 0;
    }
};

}  // namespace trmf
