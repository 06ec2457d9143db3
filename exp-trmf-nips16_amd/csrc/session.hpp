// session.hpp -- host side of the MI355X TRMF solver: set-up of the HBM-resident problem (asynchronous, one synchronisation),
// growth by appended rows, the measure-once decisions, the outer ALS loop (trmf.cpp:599-694) as asynchronous kernel launches
// on one HIP stream, recovery from a timed-out persistent kernel, statistics.  State and the phases live in the layers below
// (session_state.hpp lists them).
//
// With several ranks (one process per GPU) the nnz-heavy kernels (F-solve, X-side Gram, loss) run on this rank's contiguous row
// block; the CG runs replicated or sharded over time (DESIGN.md "Multi-GPU").
#pragma once

#include "session_xphase.hpp"

extern "C" char **environ;      // (the TRMF_* environment is part of the key of the decision cache)

namespace trmf {

struct TrmfSessionImpl : SessionXPhase {
    ~TrmfSessionImpl() {
        // nothing of this session may still be running when its buffers go back to the pool and its stream to the cache
        if (stream) (void)hipStreamSynchronize(stream);
        if (side) (void)hipStreamSynchronize(side);
        if (aux_theta) (void)hipStreamSynchronize(aux_theta);
        for (auto &e : events) {
            hipEvent_t all[] = {e.f0, e.fk0, e.fk1, e.f1, e.xg1, e.x1, e.lv1};
            for (hipEvent_t ev : all) if (ev) (void)hipEventDestroy(ev);
        }
        for (hipEvent_t ev : {gx0, gx1, gx2, fs0, fs1, fs2, ts0, ts1}) if (ev) (void)hipEventDestroy(ev);
        release_p2p();
        for (hipEvent_t ev : {ov_b, ov_c[0], ov_c[1], ov_c[2], ov_c[3], emu_ready, emu_end}) if (ev) (void)hipEventDestroy(ev);
        if (side) (void)hipStreamDestroy(side);
        for (hipEvent_t ev : {theta_fork, theta_done}) if (ev) (void)hipEventDestroy(ev);
        if (cg_note) (void)hipHostFree(cg_note);
        StreamCache::release(aux_theta);
        StreamCache::release(stream);
    }

    // ---------------------------------------------------------------------------------------------
    // Factors carry one extra all-zero row at index `rows` (operand of masked-out MFMA lanes).  The ABI's rows x k
    // arrays cross PCIe as they are; padding and column interleaving happen on the device (a host loop took 1.5 s for
    // the 512 MB item factor of config 5).
    // `raw` (the unpadded copy) must stay alive until the pad kernel has run: a member of the session, released by
    // finish_setup() after the set-up's one synchronisation.
    int upload_padded(DevBuf<real> &dst, DevBuf<real> &raw, const real *src, size_t rows) {
        if (raw.upload(src, rows * (size_t)k) || dst.alloc((rows + 1) * (size_t)KP, false)) return kFail;
        const size_t N = (rows + 1) * (size_t)KP;
        hipLaunchKernelGGL(factor_pad_kernel, dim3((unsigned)std::min<size_t>(4096, (N + 255) / 256)), dim3(256), 0, stream,
                           raw.p, rows, k, KP, NT, dst.p);
        TRMF_HIP_CHECK(hipGetLastError());
        return 0;
    }
    int download_padded(const DevBuf<real> &src, real *dst, size_t rows) {
        if (rows == 0) return 0;
        DevBuf<real> raw;
        SyncStreamOnExit drain(stream);
        const size_t N = rows * (size_t)k;
        if (raw.alloc(N, false)) return kFail;
        hipLaunchKernelGGL(factor_unpad_kernel, dim3((unsigned)std::min<size_t>(4096, (N + 255) / 256)), dim3(256), 0, stream,
                           src.p, rows, k, KP, NT, raw.p);
        TRMF_HIP_CHECK(hipGetLastError());
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        TRMF_HIP_CHECK(hipMemcpy(dst, raw.p, N * sizeof(real), hipMemcpyDeviceToHost));
        return 0;
    }
    // All three factors -> host staging in one stream-ordered batch (pinned memory of the library when they fit, ordinary
    // memory otherwise); nothing of the caller's is touched.  commit() then copies them out: c_trmf_train's outputs change
    // together or not at all (the reference's contract for a failed call, trmf.cpp:632-634).
    struct StagedFactors {
        unsigned char *base = nullptr;
        std::unique_lock<std::mutex> lease;
        std::vector<unsigned char> fallback;
        size_t bW = 0, bH = 0, bL = 0;
        void commit(void *Wout, void *Hout, void *Lout) const {
            HostStager::parallel_copy(Wout, base, bW);
            HostStager::parallel_copy(Hout, base + bW, bH);
            if (bL) std::memcpy(Lout, base + bW + bH, bL);
        }
    };
    int download_staged(StagedFactors &sf) {
        sf.bW = (size_t)T * k * sizeof(real); sf.bH = (size_t)n * k * sizeof(real); sf.bL = (size_t)nlag * k * sizeof(real);
        const size_t total = sf.bW + sf.bH + sf.bL;
        sf.base = HostStager::current().staging(total, sf.lease);
        if (!sf.base) {
            try { sf.fallback.resize(total); } catch (const std::bad_alloc &) { set_error("host staging of the factors: out of memory"); return kFail; }
            sf.base = sf.fallback.data();
        }
        DevBuf<real> rawW, rawH;
        SyncStreamOnExit drain(stream);
        if (rawW.alloc((size_t)T * k, false) || rawH.alloc((size_t)n * k, false)) return kFail;
        auto unpad = [&](const DevBuf<real> &src, size_t rows, real *dst) {
            const size_t N = rows * (size_t)k;
            if (N) hipLaunchKernelGGL(factor_unpad_kernel, dim3((unsigned)std::min<size_t>(4096, (N + 255) / 256)), dim3(256), 0, stream, src.p, rows, k, KP, NT, dst);
        };
        unpad(W, T, rawW.p); unpad(H, n, rawH.p);
        TRMF_HIP_CHECK(hipGetLastError());
        if (sf.bW) TRMF_HIP_CHECK(hipMemcpyAsync(sf.base, rawW.p, sf.bW, hipMemcpyDeviceToHost, stream));
        if (sf.bH) TRMF_HIP_CHECK(hipMemcpyAsync(sf.base + sf.bW, rawH.p, sf.bH, hipMemcpyDeviceToHost, stream));
        if (sf.bL) TRMF_HIP_CHECK(hipMemcpyAsync(sf.base + sf.bW + sf.bH, theta.p, sf.bL, hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (test_env("TRMF_FAIL_DOWNLOAD")) { set_error("download failure forced by TRMF_FAIL_DOWNLOAD"); return kFail; }   // test hook
        return 0;
    }
    // the ABI's 64-bit pointer arrays are narrowed on their way through the pinned ring (nnz < 2^32 is checked at the boundary)
    int upload_ptr32(DevBuf<uint32_t> &dst, const size_t *src, size_t count) {
        if (dst.alloc(count, false)) return kFail;
        return HostStager::current().h2d_narrow(dst.p, (const uint64_t *)src, count, stream);
    }
    int launch_sum_squares(const real *dv, size_t count) {
        if (sumsq_part.alloc(kSumsqBlocks)) return kFail;
        hipLaunchKernelGGL(sumsq_values_kernel, dim3(kSumsqBlocks), dim3(256), 0, stream, dv, count, sumsq_part.p);
        TRMF_HIP_CHECK(hipGetLastError());
        return 0;
    }
    int finish_sum_squares(double *out) {
        std::vector<double> h(kSumsqBlocks);
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        TRMF_HIP_CHECK(hipMemcpy(h.data(), sumsq_part.p, kSumsqBlocks * sizeof(double), hipMemcpyDeviceToHost));
        double acc = 0;
        for (double x : h) acc += x;
        *out = acc;
        return 0;
    }
    int device_sum_squares(const real *dv, size_t count, double *out) { return launch_sum_squares(dv, count) || finish_sum_squares(out) ? kFail : 0; }
    size_t footprint_estimate() const {
        const size_t sz = sizeof(real), NVb = (size_t)(T + 1) * KP * sz, NHb = (size_t)(n + 1) * KP * sz;
        size_t b = dense ? 2 * (size_t)T * n * sz + (full ? (size_t)kGemmChunks * std::max(T, n) * KP * sz : 0)
                         : 2 * (size_t)nnz * (4 + sz) + ((size_t)T + n + 2) * 4;
        b += NVb + NHb + (size_t)(T + n) * k * sz;              // factors and their unpadded upload copies
        b += 11 * NVb + 4 * NVb;                                 // CG vectors, rhs; tagged rows of the persistent kernel
        if (!full) b += (size_t)T * k * k * sz;                  // Gram cache (packed on the unfused path: an upper bound)
        if (full) b += NHb;
        if (generic) b += (size_t)std::min(kGenBlocks, std::max(n, 1)) * k * k * sz;
        b += (size_t)kLogCap * sizeof(DeviceIterLog) + ((size_t)32 << 20);
        return b + b / 16;
    }
    int create(const PyMatrix *Y, const uint32_t *lags, uint32_t lag_size, const PyMatrix *Wm,
               const PyMatrix *Hm, const PyMatrix *LVm) {
        T = (int)Y->rows; n = (int)Y->cols; k = (int)Wm->cols; nnz = Y->nnz;
        KP = padded_rank(k); NT = KP / kTile; KMAX = ((k + 7) / 8) * 8;
        generic = k > kMaxRank;
        nlag = (int)lag_size; midx = nlag ? (int)lags[nlag - 1] : 0;
        has_lag0 = nlag > 0 && lags[0] == 0;
        comm = active_comm();
        if (StreamCache::acquire(&stream)) return kFail;
        FillStreamScope fill(stream);
        dense = Y->type != TRMF_SPARSE;
        DevicePool::current().reserve(footprint_estimate());

        const double tu0 = now_s();
        if (!dense) {
            host_row_ptr.assign(Y->row_ptr, Y->row_ptr + (size_t)T + 1);
            host_col_ptr.assign(Y->col_ptr, Y->col_ptr + (size_t)n + 1);
            // both orientations cross PCIe as the caller holds them: the CSC's entry order IS the F-solve's summation order
            // (the reference's, trmf.cpp:369-397), and a caller's arrays need not be the canonical transpose of its CSR (the
            // reference's own coo path keeps duplicate entries apart, rf_util.py:98-118) -- deriving one orientation from the
            // other on the device would save 80 MB = 1.7 ms of the ring's time at config 3 and give up that guarantee
            if (upload_ptr32(Yc_ptr, Y->col_ptr, (size_t)n + 1)) return kFail;      // CSC first: the first F-solve needs it
            if (Yc_idx.upload(Y->row_idx, nnz)) return kFail;
            if (Yc_val.upload((const real *)Y->val, nnz)) return kFail;
            if (upload_ptr32(Yr_ptr, Y->row_ptr, (size_t)T + 1)) return kFail;
            if (Yr_idx.upload(Y->col_idx, nnz)) return kFail;
            if (Yr_val.upload((const real *)Y->val_t, nnz)) return kFail;
            if (launch_sum_squares(Yr_val.p, nnz)) return kFail;
            bytes_uploaded += 2.0 * (double)nnz * (4 + sizeof(real)) + 8.0 * ((double)T + n + 2);
        } else {
            // dense Y (only legal with missing == 0): keep both orientations, like CSR + CSC.  The caller's array goes through the
            // pinned ring as it is -- a column-major T x n array IS the row-major n x T orientation -- the other orientation and
            // sum y^2 are formed on the device (round 4 made a host copy and a host pass: 27 of config 1's 30 ms per one-shot call)
            const size_t N = (size_t)T * n;
            if (Yd_tn.alloc(N, false) || Yd_nt.alloc(N, false)) return kFail;
            if (Y->type == TRMF_DENSE_ROWMAJOR) {
                if (HostStager::current().h2d(Yd_tn.p, Y->val, N * sizeof(real), stream)) return kFail;
                launch_transpose(Yd_tn.p, T, n, Yd_nt.p);
            } else {
                if (HostStager::current().h2d(Yd_nt.p, Y->val, N * sizeof(real), stream)) return kFail;
                launch_transpose(Yd_nt.p, n, T, Yd_tn.p);
            }
            if (launch_sum_squares(Yd_tn.p, N)) return kFail;
            bytes_uploaded += (double)N * sizeof(real);
        }
        if (lag_set.upload(lags, nlag)) return kFail;
        {
            const std::vector<uint32_t> steps = ar_lag_steps(lags, nlag);
            nsteps = (int)steps.size();
            if (lag_steps.upload(steps.data(), steps.size())) return kFail;
        }
        if (upload_padded(W, raw_W, (const real *)Wm->val, T)) return kFail;
        if (upload_padded(H, raw_H, (const real *)Hm->val, n)) return kFail;
        if (theta.upload((const real *)LVm->val, (size_t)nlag * k)) return kFail;
        bytes_uploaded += ((double)T + n + nlag) * k * sizeof(real);
        t_upload_s = now_s() - tu0;

        if (xstate.alloc(1) || log.alloc(kLogCap)) return kFail;
        if (full && (GSf.alloc((size_t)k * k) || Uf.alloc((size_t)k * k) || GSx.alloc((size_t)k * k + kHvGramPad) ||
                     sgram_part.alloc((size_t)kSmallGramBlocks * k * k)))
            return kFail;
        if (alloc_series_scratch()) return kFail;
        if (comm->world > 1 && count_ranks_per_device()) return kFail;
        if (alloc_time_scratch()) return kFail;

        events.resize(kEventRing);
        for (auto &e : events) {
            hipEvent_t *all[] = {&e.f0, &e.fk0, &e.fk1, &e.f1, &e.xg1, &e.x1, &e.lv1};
            for (hipEvent_t *ev : all) { *ev = nullptr; TRMF_HIP_CHECK(hipEventCreate(ev)); }
        }
        for (hipEvent_t *ev : {&gx0, &gx1, &gx2, &fs0, &fs1, &fs2, &ts0, &ts1}) TRMF_HIP_CHECK(hipEventCreate(ev));
        if (gramx_times.alloc((size_t)8 * comm->world)) return kFail;
        if (comm->world == 1) { gramx_mode = kGramxShard; fs_mode = kShardOn; }     // nothing to decide
        if (const char *e = test_env("TRMF_GRAMX")) gramx_mode = (e[0] == 'r') ? kGramxReplicate : kGramxShard;
        if (const char *e = test_env("TRMF_FSHARD")) fs_mode = (e[0] == 'r') ? kShardOff : kShardOn;
        if (const char *e = test_env("TRMF_THETA_SOLVE")) theta_force_lds = std::string(e) == "lds";
        // the set-up's one synchronisation: uploads landed, factors padded, sum y^2 formed
        if (finish_sum_squares(&ysq_acc)) return kFail;
        set_trYTY();
        raw_W.release(); raw_H.release(); sumsq_part.release();
        if (comm->world > 1) {
            // one small gather now: the communicator's connections are set up before the ALS loop (and before the timed
            // gathers of the shard decisions).  The values are this rank's own zeros, the buffer is rewritten before use.
            std::vector<uint64_t> off(comm->world + 1);
            for (int r = 0; r <= comm->world; r++) off[r] = (uint64_t)r * 2 * sizeof(double);
            if (comm->allgatherv(gramx_times.p, off.data(), stream)) return kFail;
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        }
        // the Theta-solve's own stream, where it will be used: acquired here, not inside somebody's timed iterations (the first
        // hipStreamCreate of a process costs ~20 ms -- it showed up as 3 ms per iteration in a 6-iteration config-5 bench line)
        if (nlag > 0 && theta_overlap_pays() && !test_env("TRMF_NO_OVERLAP")) (void)ensure_aux();
        created = true;
        return autotune();
    }

    // What is sized by the number of series n alone: called by create() and again by change_series().  (gemm_part, gen_scratch, the
    // F-row partition and the split rows depend on n too: alloc_time_scratch() derives them.)
    int alloc_series_scratch() { return full && Bf.alloc((size_t)n * KP) ? kFail : 0; }

    // Everything whose size depends on the number of timestamps T (and the row partitions): called by create()
    // and again by append_rows() and change_series().
    int alloc_time_scratch() {
        const size_t NV = (size_t)T * KP;
        if (full && dense && gemm_part.alloc((size_t)kGemmChunks * (size_t)std::max(T, n) * KP)) return kFail;
        if (Bv.alloc(NV) || g.alloc(NV) || s.alloc(NV) || r.alloc(NV) ||
            d0.alloc(NV) || d1.alloc(NV) || Hd.alloc(NV) || r1.alloc(NV) || Hd1.alloc(NV) || w_new.alloc(NV) ||
            lossrow.alloc(T))
            return kFail;
        const int nchunk = std::max(1, (T - midx + kThetaChunk - 1) / kThetaChunk);
        const int npairs = nlag * (nlag + 1) / 2 + nlag;
        if (theta_part.alloc((size_t)k * nchunk * std::max(npairs, 1))) return kFail;
        if (nlag && allow_dyn_lds(theta_gram_kernel, theta_gram_lds(), "Theta Gram (max lag too large)")) return kFail;
        if (nlag && theta_solve_lds() > kLdsMax) {          // long lag sets: the |L| x |L| systems in global scratch
            if (theta_scratch.alloc((size_t)k * ((size_t)nlag * nlag + nlag), false)) return kFail;
        } else if (nlag && allow_dyn_lds(theta_solve_kernel, theta_solve_lds(), "Theta solve (too many lags)")) return kFail;
        if (generic) {
            // one k x k slot per workgroup of the generic F-solve: min(kGenBlocks, item rows) of them (kGenBlocks * k^2 at rank 1024
            // was 2 GiB in fp32 / 4 GiB in fp64 whatever the number of rows)
            if (gen_scratch.alloc((size_t)std::min(kGenBlocks, std::max(n, 1)) * k * k, false)) return kFail;
            if (allow_dyn_lds(gram_generic_kernel<true>, gram_generic_lds(k), "generic F-solve") ||
                allow_dyn_lds(gram_generic_kernel<false>, gram_generic_lds(k), "generic Gram build")) return kFail;
        }

        nbe = (int)std::min<size_t>(kMaxPartials, (NV + 255) / 256);
        rpb = std::max(1, 256 / k);
        nba = std::min(kMaxPartials, (T + rpb - 1) / rpb);
        if (full && !generic) {      // apply_shared_mfma_kernel: a 16-row tile per wavefront and pass, <= 2 workgroups per CU resident, equal passes
            const int blocks = ((T + kApplyTile - 1) / kApplyTile + 3) / 4, passes = (blocks + 511) / 512;
            nba = std::max(1, (blocks + passes - 1) / passes);
            const size_t need = apply_shared_lds_bytes(KP);
            int rc = 0;
            if (!with_nt(NT, [&](auto N) { rc = allow_dyn_lds(apply_shared_mfma_kernel<decltype(N)::value>, need, "shared-Gram product"); })) return unsupported_rank();
            if (rc) return kFail;
        }
        tile_TI = 0; nbt = 1; persist_state = 0; persist_shard_state = 0; persist_failed = false; persist_note.clear(); snap_iter = -1;
        {   // fused Hv tile: one timestamp row per 16-byte Gram column group, if the AR halo fits a modest LDS budget.
            // Tile geometry.  Narrow: 256 threads, hv_tile_rows(k) timestamps (25 at k = 40), up to two workgroups per CU.  Wide (round 5;
            // one rank only): when the narrow tiles outnumber the CUs -- config 3: 400 tiles on 256 CUs, 144 CUs carry two workgroups
            // and the persistent kernel's pass is as slow as those -- and ceil(T / CUs) timestamps fit a 512-thread workgroup, ONE
            // workgroup per CU with that many timestamps (config 3: 250 tiles of 40): the halo rows are staged once per CU instead
            // of twice and every CU carries the same load (pass 16.7 -> 14.7 us, profiles/r05_wide_tiles.txt).  Both CG forms
            // (persistent kernel, launch per step) have both geometries and are bit-identical to each other WITHIN a geometry; several
            // ranks always use the narrow one (a rank owns 1/N of the tiles), so TRMF_TEST + TRMF_TILE=narrow is what reproduces an
            // N-rank run bit for bit on one GPU.
            int TI = hv_tile_rows(k);
            tile_nth = 256;
            if (const char *e = test_env("TRMF_HV_TI")) TI = std::max(1, std::min(TI, atoi(e)));   // experiments
            // the tile kernel addresses the CG vectors with 32-bit byte offsets through buffer descriptors
            const bool fits32 = (uint64_t)(T + 1) * KP * sizeof(real) < 0x7fffffffull;
            const bool tiles_ok = !generic && fits32 && !test_env("TRMF_NO_HV_TILE");
            const char *tk = test_env("TRMF_TILE");                 // narrow | wide (wide: also where the rule would not choose it)
            if (tiles_ok && comm->world == 1 && !(tk && tk[0] == 'n') && !test_env("TRMF_HV_TI")) {
                hipDeviceProp_t prop;
                int dev = 0;
                TRMF_HIP_CHECK(hipGetDevice(&dev));
                TRMF_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
                const int cus = std::max(1, prop.multiProcessorCount), rows_wide = hv_tile_rows(k, 512), need = (T + cus - 1) / cus;
                int wide_TI = 0;
                // (the wide geometry pays through the persistent kernel; where that cannot run -- switched off, a CG cap beyond its
                // history, LDS -- the launch-per-step path is faster on narrow tiles: 975 against 959 iter/s at config 3)
                const char *pe = getenv("TRMF_PERSIST");
                const bool persist_wanted = !(pe && atoi(pe) == 0) && max_cg() <= kCgHistCap;
                if (tk && tk[0] == 'w') wide_TI = std::min(rows_wide, std::max(need, TI + 1));
                else if (persist_wanted && (T + TI - 1) / TI > cus && need <= rows_wide &&
                         persist_lds_bytes(need, midx, KP, nlag, k, (T + need - 1) / need) <= kLdsMax) wide_TI = need;
                if (wide_TI > 0 && hv_tile_lds_bytes(wide_TI, midx, KP, nlag, k) <= 64 * 1024) { TI = wide_TI; tile_nth = 512; }
            }
            if (tiles_ok && hv_tile_lds_bytes(TI, midx, KP, nlag, k) <= (tile_nth == 512 ? 64 : 48) * 1024) {
                tile_TI = TI;
                nbt = (T + TI - 1) / TI;                     // one tile per workgroup
            } else tile_nth = 256;
        }
        // The cached Grams: k x k per timestamp for the fused kernel; the unfused path's product streams them once per CG
        // step and nothing else (1.64 GB per step at config 5), so there only the upper triangle is kept (packed_gram_elems)
        gpacked = !full && !generic && tile_TI == 0 && !test_env("TRMF_GRAM_FULL");
        const size_t gelems = gpacked ? packed_gram_elems(k) : (size_t)k * k;
        if (G.alloc((full ? 1 : (size_t)T * gelems) + kHvGramPad)) return kFail;
        if (gpacked) {
            const size_t need = (size_t)apply_stages(k) * 512 * sizeof(real);
            if (allow_dyn_lds(apply_kernel<true, 5>, need, "packed cached-Gram product") ||
                allow_dyn_lds(apply_kernel<true, 10>, need, "packed cached-Gram product") ||
                allow_dyn_lds(apply_kernel<true, 17>, need, "packed cached-Gram product"))
                return kFail;
        }
        if (setup_tile_messages()) return kFail;
        {   // unfused path: timestamps per AR tile.  One workgroup per CU (LDS); a tile costs ~(TI + 2 midx) staged rows,
            // (TI + midx) residual rows and TI output rows, and the grid runs in ceil(tiles * column groups / CUs) rounds:
            // take the tile count with the cheapest schedule among those whose halo fits the 150 KB LDS budget (tiles of at
            // most 1024 - midx timestamps keep all residuals in registers and need half the LDS: ar_tile_one_pass).
            hipDeviceProp_t prop;
            int dev = 0;
            TRMF_HIP_CHECK(hipGetDevice(&dev));
            TRMF_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
            const int cus = std::max(1, prop.multiProcessorCount), groups = KP / kArCols;
            int ti_max = (T + kArU - 1) / kArU * kArU;
            while (ti_max > kArU && ar_tile_lds_bytes(ti_max, midx, nlag) > 150 * 1024) ti_max = std::max(kArU, (ti_max / 2 + kArU - 1) / kArU * kArU);
            while (ti_max + kArU <= T && ar_tile_lds_bytes(ti_max + kArU, midx, nlag) <= 150 * 1024) ti_max += kArU;
            const int nt_min = (T + ti_max - 1) / ti_max;
            double best = 0;
            for (int nt = nt_min; nt <= 4 * nt_min + 1; nt++) {
                const int ti = ((T + nt - 1) / nt + kArU - 1) / kArU * kArU;
                const int tiles = (T + ti - 1) / ti;
                // a round is dominated by the tile's serial chain (measured: 15.2 us at TI=280, 16.0 us at TI=416), rows add little
                const double cost = (double)((tiles * groups + cus - 1) / cus) * (3.0 * ti + 3.0 * midx + 2000);
                if (best == 0 || cost < best) { best = cost; ar_TI = ti; }
            }
            if (const char *e = test_env("TRMF_AR_TI")) ar_TI = std::max(kArU, atoi(e) / kArU * kArU);   // experiments
            const size_t need = ar_tile_lds_bytes(ar_TI, midx, nlag);
            if (allow_dyn_lds(ar_tile_kernel<AR_PLAIN>, need, "AR operator (max lag too large)") ||
                allow_dyn_lds(ar_tile_kernel<AR_CG_STEP>, need, "AR operator (max lag too large)"))
                return kFail;
            nbar = ((T + ar_TI - 1) / ar_TI) * (KP / kArCols);
            if (arbase.alloc(NV)) return kFail;
        }
        // with several ranks the apply kernel's partial slots are divided among them: kShardSlots in all, so that a rank's
        // share of the rows still launches enough workgroups to stream its Grams at full rate (128 of 1024 slots per rank
        // on 8 GPUs ran config 5's product at half the bandwidth)
        xp.pstride = std::max(std::max(kMaxPartials, comm->world > 1 ? kShardSlots : 0), std::max(nbt, nbar));
        if (partials.alloc((size_t)P_NSLOTS * xp.pstride)) return kFail;
        xp.T = T; xp.k = k; xp.KP = KP; xp.NT = NT; xp.nlag = nlag; xp.midx = midx;
        xp.lambdaI = lambdaI; xp.lambdaAR = lambdaAR; xp.eps_cg = eps_cg;
        xp.full = full ? 1 : 0; xp.gstride = full ? 0 : gelems; xp.trYTY = trYTY;

        fbounds.resize(comm->world + 1); xbounds.resize(comm->world + 1); fcut.clear();
        if (!dense) {
            partition_by_nnz<uint64_t>((uint64_t)n, host_col_ptr.data(), comm->world, fbounds.data());
            partition_by_nnz<uint64_t>((uint64_t)T, host_row_ptr.data(), comm->world, xbounds.data());
        } else {
            for (int r = 0; r <= comm->world; r++) {
                fbounds[r] = (uint64_t)n * r / comm->world;
                xbounds[r] = (uint64_t)T * r / comm->world;
            }
        }
        if (decide_cg_shard()) return kFail;
        init_x_forms();
        return setup_split_rows();
    }
    // Long rows of both orientations (session_state.hpp "split rows"): lists, items and the slab of partial Grams.  Observed-entries
    // path with the register-tiled kernels only: the full-observation path has one shared Gram, the generic kernels (rank > 64) already
    // give a row a whole workgroup.
    int setup_split_rows() {
        longF.clear(); longX.clear();
        part_slab.release(); part_stride = 0;
        if (dense || generic) return 0;
        hipDeviceProp_t prop;
        int dev = 0;
        TRMF_HIP_CHECK(hipGetDevice(&dev));
        TRMF_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        const int waves = std::max(1, prop.multiProcessorCount) * 12;        // three wavefronts per SIMD: what the Gram kernels are built for
        if (build_long_rows(longF, host_col_ptr, (size_t)n, (sizeof(real) == 4 && !full) ? 512u : 2048u, waves) ||
            build_long_rows(longX, host_row_ptr, (size_t)T, 2048u, waves, true)) return kFail;
        const uint32_t items = std::max(longF.nitems, longX.nitems);
        if (!items) return 0;
        if (full) {                      // sparse Y with missing == 0: the items' partial rows of Y^T W / Y H (spmm_part_kernel), KP values each
            part_stride = (uint32_t)KP;
            return part_slab.alloc((size_t)items * part_stride, false);
        }
        if (!with_nt(NT, [&](auto N) { part_stride = split_part_reals<decltype(N)::value>(true); })) return unsupported_rank();
        return part_slab.alloc((size_t)items * part_stride, false);
    }
    int set_series_transform(const real *a, const real *b) {
        if (!dense) { set_error("set_series_transform: needs a dense Y (missing == 0)"); return kFail; }
        FillStreamScope fill(stream);
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (Yraw.n != (size_t)T * n) {              // first call: the resident copy is still the raw matrix
            if (has_transform) { set_error("set_series_transform: raw matrix lost"); return kFail; }
            if (Yraw.alloc((size_t)T * n, false)) return kFail;
            TRMF_HIP_CHECK(hipMemcpyAsync(Yraw.p, Yd_tn.p, (size_t)T * n * sizeof(real), hipMemcpyDeviceToDevice, stream));
        }
        std::vector<real> one((size_t)n, real(1)), zero((size_t)n, real(0));
        if (tr_a.upload(a ? a : one.data(), n) || tr_b.upload(b ? b : zero.data(), n)) return kFail;
        has_transform = true;
        adapt_stale();                                              // the series statistics absorbed values in the old scale
        return apply_series_transform();
    }
    int apply_series_transform() {
        const int nb = 1024;
        if (tr_part.alloc(nb)) return kFail;
        hipLaunchKernelGGL(affine_columns_kernel, dim3(nb), dim3(256), 0, stream, Yraw.p, (size_t)T, n, tr_a.p, tr_b.p, Yd_tn.p, tr_part.p);
        launch_transpose(Yd_tn.p, T, n, Yd_nt.p);
        TRMF_HIP_CHECK(hipGetLastError());
        std::vector<double> part(nb);
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        TRMF_HIP_CHECK(hipMemcpy(part.data(), tr_part.p, nb * sizeof(double), hipMemcpyDeviceToHost));
        ysq_acc = 0;
        for (double v : part) ysq_acc += v;
        set_trYTY();
        return 0;
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
    void heldout_geometry(uint64_t m, int *nb, uint64_t *chunk) const {
        // equal contiguous chunks, a multiple of one workgroup step each: the work of a workgroup does not depend on row lengths
        *nb = (int)std::max<uint64_t>(1, std::min<uint64_t>(kHoMaxBlocks, (m + 255) / 256));
        *chunk = ((m + *nb - 1) / *nb + kHoStep - 1) / kHoStep * kHoStep;
        if (*chunk == 0) *chunk = kHoStep;
        *nb = (int)std::max<uint64_t>(1, (m + *chunk - 1) / *chunk);
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
            std::vector<real> hom;
            if (ad_gamma != 1.0) {
                hom.resize((size_t)retire);
                for (int t = 0; t < retire; t++) hom[t] = -(real)std::pow(ad_gamma, (double)(ad_rows - 1 - t));
            }
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
            const double gam = carry ? ad_gamma : 1.0;
            std::vector<real> hom;
            if (gam != 1.0) {
                hom.resize((size_t)T);
                for (int t = 0; t < T; t++) hom[t] = (real)std::pow(gam, (double)(T - 1 - t));
            }
            if (Hn.alloc((size_t)m * KP) || chg.alloc(m, false) || flag.alloc(1, false) || (!hom.empty() && om.upload(hom.data(), hom.size()))) return kFail;
            TRMF_HIP_CHECK(hipMemsetAsync(flag.p, 0x7f, sizeof(int), stream));
            const real *omp = hom.empty() ? nullptr : om.p;
            if (!full) {
                // long columns are cut into items by the rule of the init pass on the churned problem (the bits of a fresh init)
                std::vector<uint32_t> hfirst((size_t)m + 1), hitems;
                uint64_t chunk = std::max<uint64_t>(kAdaptChunk, (new_nnz + kAdaptMaxItems - 1) / kAdaptMaxItems);
                if (const char *e = test_env("TRMF_ADAPT_CHUNK")) chunk = (uint64_t)std::max(1, atoi(e));
                for (int j = 0; j < m; j++) {
                    hfirst[j] = (uint32_t)(hitems.size() / 2);
                    const uint64_t c0 = new_col_ptr[nk + j], c1 = new_col_ptr[nk + j + 1];
                    if (c1 - c0 > chunk)
                        for (uint64_t b = c0; b < c1; b += chunk) { hitems.push_back((uint32_t)b); hitems.push_back((uint32_t)std::min<uint64_t>(b + chunk, c1)); }
                }
                hfirst[m] = (uint32_t)(hitems.size() / 2);
                const uint32_t nitems = (uint32_t)(hitems.size() / 2);
                if (nitems && (d_first.upload(hfirst.data(), hfirst.size()) || d_items.upload(hitems.data(), hitems.size()) ||
                               slab.alloc((size_t)nitems * adapt_part_reals(k), false))) return kFail;
                if (!carry && (Sfull.alloc((size_t)m * PK, false) || rfull.alloc((size_t)m * k, false))) return kFail;
                AdaptArgs a{cptr2.p + nk, cidx2.p, cval2.p, cptr2.p + nk, W.p, omp, nullptr, nullptr, carry ? S2.p + (size_t)nk * PK : Sfull.p,
                            carry ? r2.p + (size_t)nk * k : rfull.p, nitems ? d_first.p : nullptr, nitems ? d_items.p : nullptr, nitems ? slab.p : nullptr,
                            Hnew_rows, Hn.p, chg.p, flag.p, real(1), (real)lambdaI, 0, m, k, KP};
                if (!with_nt(NT, [&](auto N) {
                        if (nitems) hipLaunchKernelGGL(adapt_part_kernel<decltype(N)::value>, dim3(nitems), dim3(64), 0, stream, a);
                        hipLaunchKernelGGL(adapt_series_kernel<decltype(N)::value>, dim3(m), dim3(64), 0, stream, a);
                    })) return unsupported_rank();
            } else {
                if (Sfull.alloc(PK, false) || rfull.alloc((size_t)m * k, false) || U.alloc((size_t)k * k, false)) return kFail;
                if (dense) {      // the m x T orientation of the block in the trained scale
                    if (blk_nt.alloc((size_t)T * m, false)) return kFail;
                    launch_transpose(fit_blk, T, m, blk_nt.p);
                }
                AdaptFullArgs a{dense ? nullptr : cptr2.p + nk, dense ? nullptr : cidx2.p, dense ? nullptr : cval2.p, dense ? nullptr : cptr2.p + nk,
                                dense ? blk_nt.p : nullptr, W.p, omp, nullptr, nullptr, Sfull.p, rfull.p, U.p, Hnew_rows, Hn.p, chg.p, real(1), 0, T, m, k, KP, NT};
                hipLaunchKernelGGL(adapt_full_gram_kernel, dim3((unsigned)((PK + 255) / 256)), dim3(256), 0, stream, a);
                hipLaunchKernelGGL(adapt_full_rhs_kernel, dim3((m + 3) / 4), dim3(256), 0, stream, a);
                AssimFactorArgs fa{Sfull.p, (size_t)0, 1, U.p, flag.p, (real)lambdaI, 0, 1, k};       // the one shared system: "series 0" names it
                if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(assim_factor_kernel<decltype(N)::value>, dim3(1), dim3(256), 0, stream, fa); }))
                    return unsupported_rank();
                hipLaunchKernelGGL(adapt_full_subst_kernel, dim3((m + 3) / 4), dim3(256), 0, stream, a);
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
    bool decisions_pending() const {
        if (comm->world <= 1 || full) return false;
        if (fs_mode == kShardMeasure && period_H > 0) return true;
        if (period_W <= 0) return false;
        if (x_form < 0) return true;
        const bool rep_gram = tile_TI > 0 ? x_form == kXRep : (!uts && !cg_shard);
        return rep_gram && !cg_shard && gramx_mode == kGramxMeasure;
    }
    // Process-level cache of the decisions, keyed by everything they depend on (shape, element type, communicator, the TRMF_*
    // environment): the second session of a grid_search over the same problem -- c_trmf_train creates one per call -- takes the
    // first one's decisions instead of measuring again (<= 14 iterations).  Every rank makes the same sequence of calls, so the
    // caches agree; a cached form that this session cannot run (the peer-to-peer arena's trial failed this time) is ignored.
    struct TunedDecisions {
        int fs_mode, gramx_mode, x_form, tuned_iters;
        float x_ms[kXForms]; double x_ms_all[kXForms];
        std::vector<int> x_cands;
        std::string persist_note;
    };
    static std::map<std::string, TunedDecisions> &decision_cache() { static std::map<std::string, TunedDecisions> c; return c; }
    static std::mutex &decision_mu() { static std::mutex m; return m; }
    std::string decision_key() const {
        std::string key = std::to_string(T) + "," + std::to_string(n) + "," + std::to_string(k) + "," + std::to_string(nnz) + "," + std::to_string(nlag) + "," +
                          std::to_string(midx) + "," + std::to_string(sizeof(real)) + "," + std::to_string(full) + std::to_string(dense) + "," + std::to_string(comm->id) + "," +
                          std::to_string(comm->world) + "," + std::to_string(period_W > 0) + std::to_string(period_H > 0);
        for (char **e = ::environ; e && *e; e++) if (!strncmp(*e, "TRMF_", 5)) { key += ";"; key += *e; }
        return key;
    }
    int autotune() {
        tuned_iters = 0; decisions_from_cache = false;
        if (const char *e = getenv("TRMF_AUTOTUNE")) if (atoi(e) == 0) return 0;
        if (!decisions_pending()) return 0;
        const std::string key = decision_key();
        {
            std::lock_guard<std::mutex> lk(decision_mu());
            auto it = decision_cache().find(key);
            if (it != decision_cache().end() && it->second.x_cands == x_cands) {
                const TunedDecisions &d = it->second;
                fs_mode = d.fs_mode; gramx_mode = d.gramx_mode; x_form = d.x_form; persist_note = d.persist_note;
                for (int f = 0; f < kXForms; f++) { x_ms[f] = d.x_ms[f]; x_ms_all[f] = d.x_ms_all[f]; }
                x_calls = 2 * (int)x_cands.size();
                decisions_from_cache = true;
                if (!decisions_pending()) {
                    if (verbose && comm->rank == 0) fprintf(stderr, ">> %s\n", describe().c_str());
                    return 0;
                }
                decisions_from_cache = false;          // (incomplete entry: measure)
            }
        }
        DevBuf<real> W0, H0, T0;
        SyncStreamOnExit drain(stream);
        const size_t nw = (size_t)(T + 1) * KP, nh = (size_t)(n + 1) * KP, nt = (size_t)nlag * k;
        if (W0.alloc(nw, false) || H0.alloc(nh, false) || T0.alloc(nt, false)) return kFail;
        TRMF_HIP_CHECK(hipMemcpyAsync(W0.p, W.p, nw * sizeof(real), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(H0.p, H.p, nh * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (nt) TRMF_HIP_CHECK(hipMemcpyAsync(T0.p, theta.p, nt * sizeof(real), hipMemcpyDeviceToDevice, stream));
        const int v = verbose, it0 = iter;
        const bool ln = log_norms;
        verbose = 0; log_norms = false;
        int rc = 0;
        for (; tuned_iters < kAutotuneMax && decisions_pending() && rc == 0; tuned_iters++) rc = run(1);
        verbose = v; log_norms = ln; iter = it0;
        if (rc) return kFail;
        TRMF_HIP_CHECK(hipMemcpyAsync(W.p, W0.p, nw * sizeof(real), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(H.p, H0.p, nh * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (nt) TRMF_HIP_CHECK(hipMemcpyAsync(theta.p, T0.p, nt * sizeof(real), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (sync()) return kFail;
        if (!decisions_pending()) {
            TunedDecisions d{fs_mode, gramx_mode, x_form, tuned_iters, {}, {}, x_cands, persist_note};
            for (int f = 0; f < kXForms; f++) { d.x_ms[f] = x_ms[f]; d.x_ms_all[f] = x_ms_all[f]; }
            std::lock_guard<std::mutex> lk(decision_mu());
            decision_cache()[key] = d;
        }
        if (verbose && comm->rank == 0) fprintf(stderr, ">> %s\n", describe().c_str());
        return 0;
    }
    // what this session runs, in one line (trmf_session_describe; bench.py's config.parallelism)
    // which rows are cut into items (session_state.hpp "split rows"); empty when none are
    std::string describe_split() const {
        if (!longF.any() && !longX.any()) return "";
        char t[224];
        snprintf(t, sizeof t, "; split rows: F %zu rows in %u items (>= %u entries), X %zu rows in %u items (>= %u entries)", longF.rows.size(), longF.nitems,
                 longF.thresh, longX.rows.size(), longX.nitems, longX.thresh);
        return t;
    }
    std::string describe_lag() const {
        char t[96];
        if (!lag_lasso()) {
            if (nlag == 0) return "; lag penalty: ridge";
            if (const int cls = theta_reg_class()) snprintf(t, sizeof t, "; lag penalty: ridge (solve in registers, class %d)", cls);
            else snprintf(t, sizeof t, "; lag penalty: ridge (solve in %s)", theta_scratch.p ? "global scratch" : "LDS");
            return t;
        }
        snprintf(t, sizeof t, "; lag penalty: lasso l1=%g refit=%d", lambdaLagL1, lag_refit);
        return t;
    }
    std::string describe() const { return describe_forms() + describe_split() + describe_lag(); }
    std::string describe_forms() const {
        char buf[640];
        if (comm->world <= 1) {
            snprintf(buf, sizeof buf, "1 rank; X-solve %s", generic ? "unfused; generic kernels for rank > 64 (Gram build, F-solve)"
                     : tile_TI <= 0 ? "unfused (AR tile + cached-Gram product per CG step)"
                     : persist_state == 1 ? "fused, one persistent kernel per solve" : persist_state == 0 ? "fused (not run yet)" : "fused, one launch per CG step");
            std::string d(buf);
            if (!generic && tile_TI > 0) { snprintf(buf, sizeof buf, "; %d tiles of %d timestamps, %d threads", nbt, tile_TI, tile_nth); d += buf; }
            return persist_note.empty() ? d : d + " (" + persist_note + ")";
        }
        const bool fused = tile_TI > 0;
        std::string x;
        if (full) x = "full-observation path (shared Gram)";
        else if (fused && ts_possible) x = std::string("fused CG ") + x_form_name(x_form) + (x_form == kXRep && persist_state == 1 ? " (one persistent kernel per solve on every rank)" : "");
        else if (fused) x = "fused CG replicated (too few tiles to shard over time)";
        else if (uts) x = std::string("unfused CG ") + x_form_name(x_form);
        else x = cg_shard ? "unfused CG, cached-Gram product sharded (H d rows gathered per step)" : "unfused CG replicated";
        std::string meas;
        for (int f : x_cands) {
            char t[96];
            snprintf(t, sizeof t, "%s%s %.3f ms", meas.empty() ? "" : ", ", x_form_name(f), x_ms_all[f]);
            meas += t;
        }
        const bool rep_gram = !full && (fused ? x_form == kXRep : (!uts && !cg_shard));
        snprintf(buf, sizeof buf, "%d ranks; F rows %s%s; X-side Gram rows %s; %s%s%s%s; peer-to-peer transport %s%s%s; decided %s%d set-up iterations",
                 comm->world, fs_mode == kShardOff ? "replicated" : fs_mode == kShardOn ? "sharded + all-gather of H" : "sharded (undecided)",
                 (fs_mode == kShardOn && fchunks >= 2) ? " in overlapped chunks" : "",
                 !rep_gram ? "own timestamps only (never gathered)" : gramx_mode == kGramxReplicate ? "replicated" : gramx_mode == kGramxShard ? "sharded + all-gather of G" : "sharded (undecided)",
                 x.c_str(), meas.empty() ? "" : " [slowest rank's X phase: ", meas.c_str(), meas.empty() ? "" : "]",
                 p2p.on ? "available" : "unavailable", p2p.note.empty() ? "" : ": ", p2p.note.c_str(),
                 decisions_from_cache ? "by an earlier session of this process (cached), " : "in ", tuned_iters);
        return persist_note.empty() ? std::string(buf) : std::string(buf) + " (" + persist_note + ")";
    }

    // ---- the ALS loop (trmf.cpp:647-693) --------------------------------------------------------------------
    int run(int iters) {
        if (comm->world == 1 && snap_iter < 0 && period_W > 0 && iters > 0 && tile_TI > 0 && !persist_failed) {
            // the persistent kernel is about to be used: the state to come back to if it times out (persist_recover)
            FillStreamScope fill(stream);                 // (persist_usable() allocates the exchange tables on first use)
            if (max_cg() <= kCgHistCap && persist_usable(max_cg()) && take_snapshot()) return kFail;
        }
        for (int it = 0; it < iters; it++) {
            const int iter1 = ++iter;                       // 1-based like the reference
            DeviceIterLog *L = log.p + ((iter1 - 1) % kLogCap);
            PhaseEvents &ev = events[(iter1 - 1) % kEventRing];
            ev_on = ev_period > 0 && (iter1 % ev_period) == 0;
            if (ev_valid.size() != (size_t)kEventRing) ev_valid.assign(kEventRing, 0);
            ev_valid[(iter1 - 1) % kEventRing] = ev_on ? 1 : 0;
            static const DeviceIterLog blank = [] { DeviceIterLog b; std::memset(&b, 0, sizeof b); b.normF = b.normX = b.normLV = -1; return b; }();
            const bool doF = period_H > 0 && (iter1 % period_H) == 0;
            const bool doX = period_W > 0 && (iter1 % period_W) == 0;
            const bool doL = period_Lag > 0 && (iter1 % period_Lag) == 0;
            // quiet runs: accept_kernel writes the whole record; otherwise a blank record is uploaded and the
            // phases fill it in (two small copies per iteration on the stream)
            const bool device_log = doX && !log_norms && !verbose;
            if (!device_log) TRMF_HIP_CHECK(hipMemcpyAsync(L, &blank, sizeof blank, hipMemcpyHostToDevice, stream));
            TRMF_EVREC(ev.f0, stream);
            if (doF) {
                if (full ? fsolve_full(ev) : fsolve(ev)) return kFail;
                if (log_norms || verbose) log_norm(H.p, (size_t)n * KP, &L->normF);
                if (verbose) fprintf(stderr, ">> iter %d F %g\n", iter1, host_double(&L->normF));
            } else {
                TRMF_EVREC(ev.fk0, stream);
                TRMF_EVREC(ev.fk1, stream);
            }
            TRMF_EVREC(ev.f1, stream);
            if (!doX) TRMF_EVREC(ev.xg1, stream);
            if (doX) {
                if (join_theta()) return kFail;              // the X-solve reads Theta (and writes W, which the Theta-solve reads)
                xg1_event = ev_on ? ev.xg1 : nullptr;
                const int xrc = xsolve(device_log ? &L->x : nullptr, device_log ? &L->normF : nullptr);
                xg1_event = nullptr;
                if (xrc) return kFail;
                if (log_norms || verbose) log_norm(W.p, (size_t)T * KP, &L->normX);
                if (!device_log)
                    TRMF_HIP_CHECK(hipMemcpyAsync(&L->x, xstate.p, sizeof(XState), hipMemcpyDeviceToDevice, stream));
                if (verbose) {
                    fprintf(stderr, ">> iter %d X %g\n", iter1, host_double(&L->normX));
                    if (verbose >= 2) {
                        XState hx;
                        (void)hipMemcpy(&hx, xstate.p, sizeof hx, hipMemcpyDeviceToHost);
                        fprintf(stdout, "iter  1 act %5.3e pre %5.3e delta %5.3e f %5.3e |g| %5.3e CG %3d |g| %5.3e\n",
                                hx.actred, hx.prered, hx.delta, hx.f, hx.gnorm, hx.cg_iter, hx.cg_rnorm);
                        fflush(stdout);
                    }
                }
            }
            TRMF_EVREC(ev.x1, stream);
            if (doL) {
                if (verbose) {
                    log_norm(theta.p, (size_t)nlag * k, &L->normLV);
                    fprintf(stderr, ">> iter %d LV(%d %d) %g\n", iter1, nlag, k, host_double(&L->normLV));
                }
                // not the last iteration of this call, nothing reads Theta in stream order, long enough to pay: under the next F-solve
                const bool under_f = nlag > 0 && it + 1 < iters && overlap_ok();
                if (under_f) {
                    if (join_theta()) return kFail;
                    TRMF_HIP_CHECK(hipEventRecord(theta_fork, stream));
                    TRMF_HIP_CHECK(hipStreamWaitEvent(aux_theta, theta_fork, 0));
                    if (theta_solve(aux_theta)) return kFail;
                    TRMF_EVREC(ev.lv1, aux_theta);
                    TRMF_HIP_CHECK(hipEventRecord(theta_done, aux_theta));
                    theta_pending = true;
                    continue;
                }
                if (join_theta() || theta_solve(stream)) return kFail;
                if (log_norms || verbose) log_norm(theta.p, (size_t)nlag * k, &L->normLV);
                if (verbose) fprintf(stderr, ">> iter %d LV %g\n", iter1, host_double(&L->normLV));
            }
            TRMF_EVREC(ev.lv1, stream);
        }
        return join_theta();
    }
    int take_snapshot() {
        const size_t nw = (size_t)(T + 1) * KP, nh = (size_t)(n + 1) * KP, nt = (size_t)nlag * k;
        FillStreamScope fill(stream);
        if (snapW.alloc(nw, false) || snapH.alloc(nh, false) || snapT.alloc(nt, false)) return kFail;
        TRMF_HIP_CHECK(hipMemcpyAsync(snapW.p, W.p, nw * sizeof(real), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(snapH.p, H.p, nh * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (nt) TRMF_HIP_CHECK(hipMemcpyAsync(snapT.p, theta.p, nt * sizeof(real), hipMemcpyDeviceToDevice, stream));
        snap_iter = iter;
        return 0;
    }
    int mark() {
        if (sync()) return kFail;
        const size_t nw = (size_t)(T + 1) * KP, nh = (size_t)(n + 1) * KP, nt = (size_t)nlag * k;
        FillStreamScope fill(stream);
        if (markW.alloc(nw, false) || markH.alloc(nh, false) || markT.alloc(nt, false)) return kFail;
        TRMF_HIP_CHECK(hipMemcpyAsync(markW.p, W.p, nw * sizeof(real), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(markH.p, H.p, nh * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (nt) TRMF_HIP_CHECK(hipMemcpyAsync(markT.p, theta.p, nt * sizeof(real), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        mark_iter = iter;
        return 0;
    }
    int rewind() {
        if (mark_iter < 0) { set_error("rewind: no mark has been set"); return kFail; }
        const size_t nw = (size_t)(T + 1) * KP, nh = (size_t)(n + 1) * KP, nt = (size_t)nlag * k;
        if (markW.n != nw || markH.n != nh) { set_error("rewind: the session has grown since the mark (append_rows)"); return kFail; }
        if (sync()) return kFail;
        adapt_stale();                                              // the series statistics absorbed the W that is replaced here
        TRMF_HIP_CHECK(hipMemcpyAsync(W.p, markW.p, nw * sizeof(real), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(H.p, markH.p, nh * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (nt) TRMF_HIP_CHECK(hipMemcpyAsync(theta.p, markT.p, nt * sizeof(real), hipMemcpyDeviceToDevice, stream));
        iter = mark_iter;
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the rewound state
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        return 0;
    }
    int persist_recover(const XState &hx) {
        if (snap_iter < 0) { set_error("persistent CG kernel timed out and no snapshot exists"); return kFail; }
        const int redo = iter - snap_iter;
        if (verbose || getenv("TRMF_P2P_VERBOSE"))
            fprintf(stderr, ">> persistent CG kernel: a poll ran into its bound (exchange %lld, tile %lld, %s missing; is another process using the GPU?): "
                    "repeating %d iteration(s) with one launch per CG step\n", hx.p2p_diag[0], hx.p2p_diag[1], hx.p2p_diag[2] == 1 ? "records" : "halo rows", redo);
        persist_state = -1; persist_failed = true;
        persist_note = "the persistent kernel ran into a poll bound after iteration " + std::to_string(snap_iter) + ": one launch per CG step since";
        const size_t nw = (size_t)(T + 1) * KP, nh = (size_t)(n + 1) * KP, nt = (size_t)nlag * k;
        TRMF_HIP_CHECK(hipMemsetAsync(&xstate.p->p2p_error, 0, sizeof(int), stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(W.p, snapW.p, nw * sizeof(real), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(H.p, snapH.p, nh * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (nt) TRMF_HIP_CHECK(hipMemcpyAsync(theta.p, snapT.p, nt * sizeof(real), hipMemcpyDeviceToDevice, stream));
        iter = snap_iter;
        if (run(redo)) return kFail;
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        snapW.release(); snapH.release(); snapT.release(); snap_iter = -1;
        return 0;
    }

    // recover = false: report a timed-out persistent kernel instead of repeating its iterations (session teardown)
    int sync(bool recover = true) {
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
#if defined(TRMF_PERSIST_PROF)
        if (persist_prof.p) {
            std::vector<long long> hp((size_t)2 * kProfIters * kProfSlots + 2 * (size_t)kPersistMaxTiles);
            TRMF_HIP_CHECK(hipMemcpy(hp.data(), persist_prof.p, hp.size() * sizeof(long long), hipMemcpyDeviceToHost));
            for (int sel = 0; sel < 2; sel++) {
                const long long t0 = hp[(size_t)sel * kProfIters * kProfSlots];
                for (int i = 0; i < kProfIters; i++) {
                    const long long *r = hp.data() + ((size_t)sel * kProfIters + i) * kProfSlots;
                    if (!r[0] && !r[3]) continue;
                    fprintf(stderr, "PERSIST_PROF tile %s row %2d:", sel ? "mid" : "0  ", i);
                    for (int q = 0; q < kProfSlots; q++) fprintf(stderr, " %8.2f", r[q] ? (r[q] - t0) * 0.01 : 0.0);
                    fprintf(stderr, "  us\n");
                }
            }
            {   // CG iteration 5 of every tile, relative to the earliest collect: when its collect finished, when it published
                const long long *q = hp.data() + (size_t)2 * kProfIters * kProfSlots;
                long long base = 0;
                for (int t = 0; t < nbt; t++) if (q[2 * t] && (!base || q[2 * t] < base)) base = q[2 * t];
                fprintf(stderr, "PERSIST_TILES");
                for (int t = 0; t < nbt; t++) fprintf(stderr, " %.2f/%.2f", (q[2 * t] - base) * 0.01, (q[2 * t + 1] - base) * 0.01);
                fprintf(stderr, "\n");
            }
        }
#endif
        if (persist_state == 1 && comm->world == 1) {          // one rank: a timed-out solve is repeated on the launch-per-step path
            XState hx;
            TRMF_HIP_CHECK(hipMemcpy(&hx, xstate.p, sizeof hx, hipMemcpyDeviceToHost));
            if (hx.p2p_error && recover) return persist_recover(hx);
            if (hx.p2p_error) { set_error("persistent CG kernel: an exchange between workgroups timed out"); return kFail; }
            if (recover && snap_iter >= 0 && snap_iter != iter && take_snapshot()) return kFail;
        } else if (persist_state == 1 || (persist_shard_state == 1 && x_form == kXTsPersist)) {   // several ranks: a bounded poll of the persistent CG kernel ran out (the GPU must not hang)
            XState hx;
            TRMF_HIP_CHECK(hipMemcpy(&hx, xstate.p, sizeof hx, hipMemcpyDeviceToHost));
            if (hx.p2p_error) { set_error("persistent CG kernel: an exchange between workgroups timed out (is another process using the GPU? TRMF_PERSIST=0 selects the launch-per-step path)"); return kFail; }
        }
        if (p2p.on) {               // a bounded wait of the peer-to-peer exchange ran out: the factors are not to be trusted
            XState hx;
            TRMF_HIP_CHECK(hipMemcpy(&hx, xstate.p, sizeof hx, hipMemcpyDeviceToHost));
            if (hx.p2p_error) {
                char msg[256];
                snprintf(msg, sizeof msg, "time-sharded CG: a peer-to-peer exchange timed out (TRMF_CG=p2p): rank %d, message %lld, launch %lld, "
                         "peer %lld: expected epoch %lld, flag %lld", comm->rank, hx.p2p_diag[0] / 1000000, hx.p2p_diag[0] / 1000 % 1000 - 1,
                         hx.p2p_diag[0] % 1000, hx.p2p_diag[1], hx.p2p_diag[2]);
                set_error(msg);
                if (test_env("TRMF_P2P_DEBUG")) {       // what this rank derived its stop decisions from
                    std::vector<double> hp((size_t)P_NSLOTS * xp.pstride);
                    TRMF_HIP_CHECK(hipMemcpy(hp.data(), pbase(), hp.size() * sizeof(double), hipMemcpyDeviceToHost));
                    fprintf(stderr, "[p2p debug] rank %d: %s\n  stop_it %d cg_iter %d rho %.17g %.17g %.17g gnorm %.17g cgtol %.9g\n", comm->rank, msg,
                            hx.stop_it, hx.cg_iter, hx.rho_hist[0], hx.rho_hist[1], hx.rho_hist[2], hx.gnorm, (double)hx.cgtol);
                    for (int a = 0; a < P_NSLOTS; a++) {
                        double t = 0; int nz = 0;
                        for (int q = 0; q < xp.pstride; q++) { t += hp[(size_t)a * xp.pstride + q]; nz += hp[(size_t)a * xp.pstride + q] != 0; }
                        fprintf(stderr, "  partial array %2d: sum %.17g (%d nonzero)\n", a, t, nz);
                    }
                }
                return kFail;
            }
        }
        return 0;
    }

    int stats(TrmfIterStats *out, int cap) {
        if (sync()) return kFail;
        const int avail = std::min(iter, std::min(kLogCap, kEventRing));
        const int cnt = std::min(cap, avail);
        for (int q = 0; q < cnt; q++) {
            const int it0 = iter - cnt + q;                 // 0-based iteration index
            DeviceIterLog hl;
            TRMF_HIP_CHECK(hipMemcpy(&hl, log.p + (it0 % kLogCap), sizeof hl, hipMemcpyDeviceToHost));
            PhaseEvents &ev = events[it0 % kEventRing];
            TrmfIterStats &o = out[q];
            o.normF = hl.normF; o.normX = hl.normX; o.normLV = hl.normLV;
            o.f = hl.x.f; o.fnew = hl.x.fnew; o.actred = hl.x.actred; o.prered = hl.x.prered;
            o.gnorm = hl.x.gnorm; o.cg_rnorm = hl.x.cg_rnorm; o.cg_iter = hl.x.cg_iter; o.accepted = hl.x.accepted; o.delta = hl.x.delta;
            o.cg_rnorm_direct = hl.x.rho_direct >= 0 ? std::sqrt(hl.x.rho_direct) : -1.0;
            o.ms_F = o.ms_X = o.ms_LV = o.ms_F_kernel = o.ms_X_gram = -1;
            if (ev_valid.size() != (size_t)kEventRing || !ev_valid[it0 % kEventRing]) continue;      // no phase events in that iteration (ev_period)
            (void)hipEventElapsedTime(&o.ms_X_gram, ev.f1, ev.xg1);
            (void)hipEventElapsedTime(&o.ms_F, ev.f0, ev.f1);
            (void)hipEventElapsedTime(&o.ms_F_kernel, ev.fk0, ev.fk1);
            (void)hipEventElapsedTime(&o.ms_X, ev.f1, ev.x1);
            (void)hipEventElapsedTime(&o.ms_LV, ev.x1, ev.lv1);
        }
        return cnt;
    }

    // J = 0.5*sum_Omega (Y - w.h)^2 + 0.5*lambdaI(|W|^2+|H|^2) + 0.5*lambdaAR*AR(W;Theta)  
    double objective() {
        if (full) return NAN;       // defined for the observed-entries objective only
        XState *st = xstate.p;
        if (loss(W.p, true)) return NAN;
        hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(256), 0, stream, lossrow.p, T, &st->loss1);
        const double l = host_double(&st->loss1);
        {   // AR and ridge sums of W: the AR tile kernel's partials (its operator output goes to scratch)
            ArVecs av{};
            av.v = W.p;
            hipLaunchKernelGGL((ar_tile_kernel<AR_PLAIN>), dim3((T + ar_TI - 1) / ar_TI, KP / kArCols), dim3(kArThreads),
                               ar_tile_lds_bytes(ar_TI, midx, nlag), stream, xp, st, av, 0, 0, 0, lag_set.p, lag_steps.p, nsteps,
                               theta.p, arbase.p, pbase(), ar_TI, 0);
        }
        hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(256), 0, stream, P(P_AR), nbar, &st->gs);
        const double ar = host_double(&st->gs);
        hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(256), 0, stream, P(P_VV), nbar, &st->gs);
        const double w2 = host_double(&st->gs);
        log_norm(H.p, (size_t)n * KP, &st->gs);
        const double h2 = host_double(&st->gs);
        return 0.5 * l + 0.5 * lambdaI * (w2 + h2) + 0.5 * lambdaAR * ar;
    }

    // ---- held-out evaluation (trmf_session_set_heldout / _eval_heldout; heldout_kernels.hpp) ---------------------------
    // Yt has been validated by the caller (sparse, n columns, rows <= T, indices in range); `rows` is its row index per entry.
    int set_heldout(const PyMatrix *Yt, const std::vector<uint32_t> &rows) {
        ho_set = false; ho_m = 0;
        ho_row.release(); ho_col.release(); ho_val.release(); ho_pred.release(); ho_part.release(); ho_sums.release();
        if (!Yt) return 0;
        FillStreamScope fill(stream);
        const uint64_t m = Yt->nnz;
        if (ho_row.upload(rows.data(), m) || ho_col.upload(Yt->col_idx, m) || ho_val.upload((const real *)Yt->val_t, m)) return kFail;
        heldout_geometry(m, &ho_nb, &ho_chunk);
        if (ho_part.alloc((size_t)kHoSums * ho_nb, false) || ho_sums.alloc(kHoSums, false)) return kFail;
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        ho_m = m; ho_set = true;
        return 0;
    }
    // Reads W and H only, in stream order after everything enqueued before (the caller has synchronised the session).
    int eval_heldout(TrmfHeldoutSums *out, real *pred) {
        if (!ho_set) { set_error("eval_heldout: no held-out set (trmf_session_set_heldout)"); return kFail; }
        double h[kHoSums] = {0, 0, 0, 0, 0, 0};
        if (ho_m > 0) {
            FillStreamScope fill(stream);
            if (pred && ho_pred.alloc(ho_m, false)) return kFail;
            HeldoutArgs a{ho_row.p, ho_col.p, ho_val.p, W.p, H.p, pred ? ho_pred.p : nullptr, ho_part.p, ho_m, ho_chunk, KP, NT};
            if (!with_nt0(generic ? 0 : NT, [&](auto N) { hipLaunchKernelGGL(heldout_eval_kernel<decltype(N)::value>, dim3(ho_nb), dim3(256), 0, stream, a); }))
                return unsupported_rank();
            hipLaunchKernelGGL(heldout_reduce_kernel, dim3(1), dim3(256), 0, stream, ho_part.p, ho_nb, ho_sums.p);
            TRMF_HIP_CHECK(hipGetLastError());
            TRMF_HIP_CHECK(hipMemcpyAsync(h, ho_sums.p, sizeof h, hipMemcpyDeviceToHost, stream));
            if (pred) TRMF_HIP_CHECK(hipMemcpyAsync(pred, ho_pred.p, ho_m * sizeof(real), hipMemcpyDeviceToHost, stream));
            TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        }
        out->count = (uint64_t)h[0]; out->count_nonzero = (uint64_t)h[1];
        out->sq_err = h[2]; out->abs_err = h[3]; out->abs_truth = h[4]; out->rel_err = h[5];
        return 0;
    }
    // ---- forecasting (trmf_session_forecast / _forecast_scores / _forecast_reset; forecast_kernels.hpp) -------------------------
    // Rows [T0, T0 + steps) of the AR roll-out of Wsrc (T0 rows) into `roll` (steps x KP, column-interleaved; the caller has zeroed
    // the pads) and, if asked for, into `flat` (steps x k row-major).  Any rank 1..1024: one thread per latent dimension.
    int launch_rollout(const real *Wsrc, int T0, int steps, real *roll, real *flat) {
        RolloutArgs a{Wsrc, roll, flat, lag_set.p, theta.p, T0, steps, KP, NT, k, nlag, 0};
        const size_t lds = rollout_lds_bytes(nlag, midx);           // lags, Theta and the last `midx` rows of a workgroup's 64 columns
        if (midx > 0 && midx <= T0 && lds <= kLdsMax && !test_env("TRMF_FORECAST_GLOBAL")) {      // (the knob: the global-memory form where the LDS form would fit)
            if (allow_dyn_lds(forecast_rollout_kernel, lds, "forecast roll-out")) return kFail;
            a.reach = midx;
        }
        hipLaunchKernelGGL(forecast_rollout_kernel, dim3((k + 63) / 64), dim3(64), a.reach ? lds : 0, stream, a);
        TRMF_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // Reads W, H, Theta and the transform coefficients, in stream order after everything enqueued before (the caller has validated
    // the arguments and synchronised the session); the rolled rows live in scratch.  The outputs and the score table change only
    // when every step has succeeded.
    int forecast(int steps, bool clip, double threshold, const PyMatrix *truth, real *Ynew, real *Wnew) {
        FillStreamScope fill(stream);
        const size_t NY = (size_t)steps * n, NW = (size_t)steps * k, NT6 = (size_t)n * kFcSums;
        const bool score = truth != nullptr;
        DevBuf<real> roll, flat, tru, yd;
        std::vector<real> blk;
        SyncStreamOnExit drain(stream);
        if (roll.alloc((size_t)steps * KP) || (Wnew && flat.alloc(NW, false)) || (Ynew && yd.alloc(NY, false))) return kFail;
        if (score) {
            const real *src = (const real *)truth->val;
            if (truth->type != TRMF_DENSE_ROWMAJOR) { (void)dense_rows_to_rowmajor(truth, blk); src = blk.data(); }
            if (tru.upload(src, NY)) return kFail;
            if (fc_table[0].n != NT6 || fc_table[1].n != NT6 || fc_prev[0].n != (size_t)n || fc_prev[1].n != (size_t)n) {     // first scored call since a reset
                if (fc_table[0].alloc(NT6) || fc_table[1].alloc(NT6) || fc_prev[0].alloc(n) || fc_prev[1].alloc(n)) return kFail;
                fc_cur = 0; fc_rows = 0;
            }
        }
        if (launch_rollout(W.p, T, steps, roll.p, Wnew ? flat.p : nullptr)) return kFail;
        if (score || Ynew) {
            const int in = fc_cur, out = 1 - fc_cur;
            ScoreArgs a{H.p, roll.p, score ? tru.p : nullptr, Ynew ? yd.p : nullptr, has_transform ? tr_a.p : nullptr, has_transform ? tr_b.p : nullptr,
                        score ? fc_table[in].p : nullptr, score ? fc_table[out].p : nullptr, score ? fc_prev[in].p : nullptr, score ? fc_prev[out].p : nullptr,
                        (real)threshold, clip ? 1 : 0, fc_rows > 0 ? 1 : 0, n, steps, KP, NT, forecast_rows_per_pass(KP, generic)};
            const dim3 grid((n + 255) / 256);
            if (!with_nt0(generic ? 0 : NT, [&](auto N) { hipLaunchKernelGGL(forecast_score_kernel<decltype(N)::value>, grid, dim3(256), 0, stream, a); }))
                return unsupported_rank();
            TRMF_HIP_CHECK(hipGetLastError());
        }
        // the outputs come back through host staging (pinned memory of the library when they fit) and are copied out together
        const size_t bY = Ynew ? NY * sizeof(real) : 0, bW = Wnew ? NW * sizeof(real) : 0;
        std::unique_lock<std::mutex> lease;
        std::vector<unsigned char> fallback;
        unsigned char *base = nullptr;
        if (bY + bW) {
            base = HostStager::current().staging(bY + bW, lease);
            if (!base) {
                try { fallback.resize(bY + bW); } catch (const std::bad_alloc &) { set_error("host staging of the forecast: out of memory"); return kFail; }
                base = fallback.data();
            }
            if (bY) TRMF_HIP_CHECK(hipMemcpyAsync(base, yd.p, bY, hipMemcpyDeviceToHost, stream));
            if (bW) TRMF_HIP_CHECK(hipMemcpyAsync(base + bY, flat.p, bW, hipMemcpyDeviceToHost, stream));
        }
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        // ---- commit ----
        if (bY) HostStager::parallel_copy(Ynew, base, bY);
        if (bW) std::memcpy(Wnew, base + bY, bW);
        if (score) { fc_cur = 1 - fc_cur; fc_rows += (uint64_t)steps; }
        return 0;
    }
    int forecast_scores(uint64_t *rows_scored, double *per_series) {
        const size_t NT6 = (size_t)n * kFcSums;
        if (per_series) {
            std::vector<double> h(NT6, 0.0);
            if (fc_table[fc_cur].n == NT6) {
                TRMF_HIP_CHECK(hipStreamSynchronize(stream));
                TRMF_HIP_CHECK(hipMemcpy(h.data(), fc_table[fc_cur].p, NT6 * sizeof(double), hipMemcpyDeviceToHost));
            }
            std::memcpy(per_series, h.data(), NT6 * sizeof(double));
        }
        if (rows_scored) *rows_scored = fc_rows;
        return 0;
    }
    int forecast_reset() {
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        for (int q = 0; q < 2; q++) { fc_table[q].release(); fc_prev[q].release(); }      // the next scored call starts from zeroed ones
        fc_cur = 0; fc_rows = 0;
        return 0;
    }
    // ---- forecast uncertainty (trmf_session_fit_noise / _noise / _set_noise / _forecast_dist / _interval_scores) -----------------
    // Stages 1-2 of uncertainty_kernels.hpp on the current factors (the caller has checked rows > the largest lag).  The work items
    // of the residual pass are rebuilt from the host copy of the item pointers on every call (append_rows moves them): a few thousand
    // records.  Everything lands in scratch; the resident variances change by two device copies once the sums have been read.  No
    // collective: every rank holds the whole Y and the factors and computes the same bits.  A training matrix without a stored entry
    // is not a failure of this rank's task (res->no_entries; nothing is committed): the entry point reports it on the calling
    // thread, so the barrier of a TRMF_DEVICES group stays whole.
    struct NoiseResult {
        double pooled = 0, s2_min = 0, s2_max = 0, q_min = 0, q_max = 0;
        uint64_t series_pooled = 0;
        int no_entries = 0;
    };
    int fit_noise(NoiseResult *res) {
        *res = NoiseResult{};
        if (sync()) return kFail;
        FillStreamScope fill(stream);
        uint32_t chunk = kNzChunk;
        if (const char *e = test_env("TRMF_NOISE_CHUNK")) chunk = (uint32_t)std::max(1, atoi(e));      // tests: several items per series on a small shape
        std::vector<NoiseItem> items;
        std::vector<uint32_t> first((size_t)n + 1);
        for (int j = 0; j < n; j++) {
            first[j] = (uint32_t)items.size();
            if (full)       // every timestamp: the dense orientation's values, or zeros that the stored entries then correct
                for (uint32_t b = 0; b < (uint32_t)T; b += chunk)
                    items.push_back(NoiseItem{(uint32_t)j, b, std::min<uint32_t>(b + chunk, (uint32_t)T), (uint32_t)(dense ? kNzDense : kNzZero)});
            if (!dense)
                for (uint64_t b = host_col_ptr[j]; b < host_col_ptr[j + 1]; b += chunk)
                    items.push_back(NoiseItem{(uint32_t)j, (uint32_t)b, (uint32_t)std::min<uint64_t>(b + chunk, host_col_ptr[j + 1]), (uint32_t)(full ? kNzCorrect : kNzStored)});
            if (items.size() >= (1ull << 31)) { set_error("fit_noise: too many work items"); return kFail; }
        }
        first[n] = (uint32_t)items.size();
        const uint32_t nitems = (uint32_t)items.size();
        const int nchunks = (T - midx + kNzInnovChunk - 1) / kNzInnovChunk;
        DevBuf<NoiseItem> d_items;
        DevBuf<uint32_t> d_first;
        DevBuf<double> part, sq, cnt, s2, pooled, ipart, qn;
        SyncStreamOnExit drain(stream);
        if (d_items.upload(items.data(), nitems) || d_first.upload(first.data(), first.size()) || part.alloc((size_t)2 * nitems, false) ||
            sq.alloc(n, false) || cnt.alloc(n, false) || s2.alloc(n, false) || pooled.alloc(2, false) ||
            ipart.alloc((size_t)nchunks * k, false) || qn.alloc(k, false)) return kFail;
        if (nitems) {
            NoiseResidArgs ra{d_items.p, nitems, dense ? nullptr : Yc_idx.p, dense ? nullptr : Yc_val.p, dense ? Yd_nt.p : nullptr, W.p, H.p, part.p, T, KP, NT};
            const dim3 grid((nitems + 3) / 4);
            if (!with_nt0(generic ? 0 : NT, [&](auto N) { hipLaunchKernelGGL(noise_resid_kernel<decltype(N)::value>, grid, dim3(256), 0, stream, ra); }))
                return unsupported_rank();
            TRMF_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(noise_series_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, part.p, d_first.p, n, sq.p, cnt.p);
        hipLaunchKernelGGL(noise_pool_kernel, dim3(1), dim3(256), 0, stream, sq.p, cnt.p, n, s2.p, pooled.p);
        TRMF_HIP_CHECK(hipGetLastError());
        {
            size_t lds = innov_lds_bytes(nlag);
            NoiseInnovArgs ia{W.p, lag_set.p, theta.p, ipart.p, T, midx, k, KP, NT, nlag, 1};
            if (lds > kLdsMax) { ia.lds = 0; lds = 0; }                 // a lag set too long for LDS: Theta and the lags from global memory
            else if (allow_dyn_lds(noise_innov_kernel, lds, "noise fit")) return kFail;
            hipLaunchKernelGGL(noise_innov_kernel, dim3(nchunks, (k + 63) / 64), dim3(64), lds, stream, ia);
            hipLaunchKernelGGL(noise_q_kernel, dim3((k + 63) / 64), dim3(64), 0, stream, ipart.p, nchunks, k, (double)(T - midx), qn.p);
            TRMF_HIP_CHECK(hipGetLastError());
        }
        std::vector<double> hs2(n), hcnt(n), hq(k);
        double hp[2] = {0, 0};
        TRMF_HIP_CHECK(hipMemcpyAsync(hs2.data(), s2.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(hcnt.data(), cnt.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(hq.data(), qn.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(hp, pooled.p, sizeof hp, hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (!(hp[1] > 0)) { res->no_entries = 1; return 0; }
        // ---- commit ----
        if (nz_sigma2.alloc(n, false) || nz_q.alloc(k, false)) return kFail;
        TRMF_HIP_CHECK(hipMemcpyAsync(nz_sigma2.p, s2.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(nz_q.p, qn.p, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        nz_set = true;
        res->pooled = hp[0] / hp[1];
        res->s2_min = res->s2_max = hs2[0];
        for (int j = 0; j < n; j++) {
            res->s2_min = std::min(res->s2_min, hs2[j]); res->s2_max = std::max(res->s2_max, hs2[j]);
            res->series_pooled += hcnt[j] > 0 ? 0 : 1;
        }
        res->q_min = res->q_max = hq[0];
        for (int t = 0; t < k; t++) { res->q_min = std::min(res->q_min, hq[t]); res->q_max = std::max(res->q_max, hq[t]); }
        return 0;
    }
    // the caller's variances (validated: finite, not negative) in place of fitted ones; every rank keeps its own copy
    int set_noise(const double *sigma2, const double *q) {
        if (sync()) return kFail;
        FillStreamScope fill(stream);
        DevBuf<double> a, b;
        SyncStreamOnExit drain(stream);
        if (a.upload(sigma2, n) || b.upload(q, k)) return kFail;
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        nz_sigma2.swap(a); nz_q.swap(b);
        nz_set = true;
        return 0;
    }
    int noise(double *sigma2, double *q) {
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (sigma2) TRMF_HIP_CHECK(hipMemcpy(sigma2, nz_sigma2.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        if (q) TRMF_HIP_CHECK(hipMemcpy(q, nz_q.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }
    // forecast() plus the predictive standard deviation and the interval sums (the caller has validated the arguments, checked that
    // a noise is resident and synchronised the session).  The roll-out is forecast()'s; the outputs and the interval table change
    // only when every step has succeeded -- an impulse response that overflows included.
    int forecast_dist(int steps, bool clip, double threshold, double zq, const PyMatrix *truth, real *Ynew, real *Ysd, real *Wnew) {
        FillStreamScope fill(stream);
        const size_t NY = (size_t)steps * n, NW = (size_t)steps * k, NT7 = (size_t)n * kIvSums;
        const bool score = truth != nullptr;
        DevBuf<real> roll, flat, tru, yd, ysd;
        DevBuf<double> v, psig;
        DevBuf<int> flag;
        std::vector<real> blk;
        SyncStreamOnExit drain(stream);
        if (roll.alloc((size_t)steps * KP) || v.alloc((size_t)steps * KP) || flag.alloc(1) || (Wnew && flat.alloc(NW, false)) ||
            (Ynew && yd.alloc(NY, false)) || (Ysd && ysd.alloc(NY, false))) return kFail;
        if (score) {
            const real *src = (const real *)truth->val;
            if (truth->type != TRMF_DENSE_ROWMAJOR) { (void)dense_rows_to_rowmajor(truth, blk); src = blk.data(); }
            if (tru.upload(src, NY)) return kFail;
            if (iv_table[0].n != NT7 || iv_table[1].n != NT7) {      // first scored call since a reset
                if (iv_table[0].alloc(NT7) || iv_table[1].alloc(NT7)) return kFail;
                iv_cur = 0; iv_rows = 0;
            }
        }
        if (launch_rollout(W.p, T, steps, roll.p, Wnew ? flat.p : nullptr)) return kFail;
        {
            PsiArgs pa{lag_set.p, theta.p, nz_q.p, v.p, nullptr, flag.p, steps, k, KP, NT, nlag, 0};
            const size_t lds = psi_lds_bytes(nlag, midx);
            if (midx > 0 && lds <= kLdsMax && !test_env("TRMF_FORECAST_GLOBAL")) {
                if (allow_dyn_lds(forecast_psi_kernel, lds, "impulse response")) return kFail;
                pa.reach = midx;
            } else {
                if (psig.alloc(NW, false)) return kFail;
                pa.psi_glob = psig.p;
            }
            hipLaunchKernelGGL(forecast_psi_kernel, dim3((k + 63) / 64), dim3(64), pa.reach ? lds : 0, stream, pa);
            TRMF_HIP_CHECK(hipGetLastError());
        }
        if (score || Ynew || Ysd) {
            const int in = iv_cur, out = 1 - iv_cur;
            DistArgs a{H.p, roll.p, v.p, nz_sigma2.p, score ? tru.p : nullptr, Ynew ? yd.p : nullptr, Ysd ? ysd.p : nullptr,
                       has_transform ? tr_a.p : nullptr, has_transform ? tr_b.p : nullptr, score ? iv_table[in].p : nullptr, score ? iv_table[out].p : nullptr,
                       (real)threshold, zq, clip ? 1 : 0, n, steps, KP, NT, dist_rows_per_pass(KP, generic)};
            const dim3 grid((n + 255) / 256);
            if (!with_nt0(generic ? 0 : NT, [&](auto N) { hipLaunchKernelGGL(forecast_dist_kernel<decltype(N)::value>, grid, dim3(256), 0, stream, a); }))
                return unsupported_rank();
            TRMF_HIP_CHECK(hipGetLastError());
        }
        // the outputs come back through host staging (pinned memory of the library when they fit) and are copied out together
        const size_t bY = Ynew ? NY * sizeof(real) : 0, bS = Ysd ? NY * sizeof(real) : 0, bW = Wnew ? NW * sizeof(real) : 0;
        std::unique_lock<std::mutex> lease;
        std::vector<unsigned char> fallback;
        unsigned char *base = nullptr;
        if (bY + bS + bW) {
            base = HostStager::current().staging(bY + bS + bW, lease);
            if (!base) {
                try { fallback.resize(bY + bS + bW); } catch (const std::bad_alloc &) { set_error("host staging of the forecast: out of memory"); return kFail; }
                base = fallback.data();
            }
            if (bY) TRMF_HIP_CHECK(hipMemcpyAsync(base, yd.p, bY, hipMemcpyDeviceToHost, stream));
            if (bS) TRMF_HIP_CHECK(hipMemcpyAsync(base + bY, ysd.p, bS, hipMemcpyDeviceToHost, stream));
            if (bW) TRMF_HIP_CHECK(hipMemcpyAsync(base + bY + bS, flat.p, bW, hipMemcpyDeviceToHost, stream));
        }
        int bad = 0;
        TRMF_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (bad) { set_error("forecast_dist: lag weights explosive over this horizon (a latent forecast variance is not finite); nothing was changed"); return kFail; }
        // ---- commit ----
        if (bY) HostStager::parallel_copy(Ynew, base, bY);
        if (bS) HostStager::parallel_copy(Ysd, base + bY, bS);
        if (bW) std::memcpy(Wnew, base + bY + bS, bW);
        if (score) { iv_cur = 1 - iv_cur; iv_rows += (uint64_t)steps; }
        return 0;
    }
    int interval_scores(uint64_t *rows_scored, double *per_series) {
        const size_t NT7 = (size_t)n * kIvSums;
        if (per_series) {
            std::vector<double> h(NT7, 0.0);
            if (iv_table[iv_cur].n == NT7) {
                TRMF_HIP_CHECK(hipStreamSynchronize(stream));
                TRMF_HIP_CHECK(hipMemcpy(h.data(), iv_table[iv_cur].p, NT7 * sizeof(double), hipMemcpyDeviceToHost));
            }
            std::memcpy(per_series, h.data(), NT7 * sizeof(double));
        }
        if (rows_scored) *rows_scored = iv_rows;
        return 0;
    }
    int interval_reset() {
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        for (int q = 0; q < 2; q++) iv_table[q].release();      // the next scored call starts from zeroed ones
        iv_cur = 0; iv_rows = 0;
        return 0;
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
            flag.alloc(1, false) || errs.alloc((size_t)2 * nr, false)) return kFail;
        TRMF_HIP_CHECK(hipMemsetAsync(flag.p, 0x7f, sizeof(int), stream));
        // stage A
        if (full) {
            if (y_times_factor(false, H.p, Bv.p, dense ? 0u : (uint32_t)first_row, (uint32_t)T)) return kFail;        // rows of Y H
            if (small_gram(H.p, n, real(0), GSx.p, stream)) return kFail;                                             // H^T H
        } else if (launch_gram_x_rows((uint32_t)first_row, (uint32_t)T)) return kFail;
        TRMF_HIP_CHECK(hipGetLastError());
        // stages B and C, a chunk of rows at a time
        const real lamAR = (real)lambdaAR, lam = (real)lambdaI + lamAR;
        int reach = 0;
        if (midx > 0 && assim_chain_lds_bytes(k, nlag, midx) <= kLdsMax && !test_env("TRMF_FORECAST_GLOBAL")) reach = midx;
        const size_t lds = assim_chain_lds_bytes(k, nlag, reach);
        if (allow_dyn_lds(assim_chain_kernel, lds, "online update")) return kFail;
        for (int r0 = first_row; r0 < T; r0 += chunk) {
            const int rows = std::min(chunk, T - r0);
            AssimFactorArgs fa{Gmat(), full ? (size_t)0 : xp.gstride, gpacked ? 1 : 0, U.p, flag.p, lam, r0, rows, k};
            if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(assim_factor_kernel<decltype(N)::value>, dim3((rows + 3) / 4), dim3(256), 0, stream, fa); }))
                return unsupported_rank();
            AssimChainArgs ca{W.p, Wn.p, Wout ? flat.p : nullptr, Bv.p, U.p, lag_set.p, theta.p, lamAR, first_row, r0, rows, k, KP, NT, nlag, reach};
            hipLaunchKernelGGL(assim_chain_kernel, dim3(1), dim3(256), lds, stream, ca);
            TRMF_HIP_CHECK(hipGetLastError());
        }
        {   // the squared errors of the range with W as it is and as it will be
            AssimErrArgs ea{dense ? nullptr : Yr_ptr.p, dense ? nullptr : Yr_idx.p, dense ? nullptr : Yr_val.p, dense ? Yd_tn.p : nullptr, H.p,
                            W.p, Wn.p, 0, first_row, errs.p, first_row, nr, n, KP, full ? 1 : 0};
            hipLaunchKernelGGL(assim_err_kernel, dim3(nr), dim3(256), 0, stream, ea);
            TRMF_HIP_CHECK(hipGetLastError());
        }
        int bad = kAssimNoBadRow;
        std::vector<double> herr((size_t)2 * nr);
        std::vector<real> hflat(Wout ? (size_t)nr * k : 0);
        TRMF_HIP_CHECK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(herr.data(), errs.p, herr.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (Wout) TRMF_HIP_CHECK(hipMemcpyAsync(hflat.data(), flat.p, hflat.size() * sizeof(real), hipMemcpyDeviceToHost, stream));
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (bad != kAssimNoBadRow) { res->bad_row = bad; return 0; }
        // ---- commit ----
        TRMF_HIP_CHECK(hipMemcpyAsync(W.p + (size_t)first_row * KP, Wn.p, (size_t)nr * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (first_row < ad_rows) adapt_stale();                     // rows the series statistics absorbed have changed
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the new W
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
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
        std::vector<real> hthr((size_t)n);
        for (int j = 0; j < n; j++) hthr[j] = (real)c * (real)scale[j];
        DevBuf<real> Wn, flat, wcur, prior, thr, wts, slab;
        DevBuf<int> flag;
        DevBuf<double> errs, slab_d, rowsum;
        SyncStreamOnExit drain(stream);
        if (Wn.alloc((size_t)nr * KP) || (Wout && flat.alloc((size_t)nr * k, false)) || wcur.alloc(KP) || prior.alloc(KP) || thr.upload(hthr.data(), n) ||
            wts.alloc(nw, false) || slab.alloc((size_t)max_slices * assim_robust_slot_reals(KP), false) || slab_d.alloc((size_t)2 * max_slices, false) ||
            rowsum.alloc((size_t)2 * nr, false) || flag.alloc(1, false) || errs.alloc((size_t)2 * nr, false)) return kFail;
        TRMF_HIP_CHECK(hipMemsetAsync(flag.p, 0x7f, sizeof(int), stream));
        AssimRobustArgs ra{dense ? nullptr : Yr_ptr.p, dense ? nullptr : Yr_idx.p, dense ? nullptr : Yr_val.p, dense ? Yd_tn.p : nullptr, H.p, W.p, Wn.p,
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
        {   // the squared errors of the range with W as it is and as it will be (unweighted)
            AssimErrArgs ea{dense ? nullptr : Yr_ptr.p, dense ? nullptr : Yr_idx.p, dense ? nullptr : Yr_val.p, dense ? Yd_tn.p : nullptr, H.p,
                            W.p, Wn.p, 0, first_row, errs.p, first_row, nr, n, KP, full ? 1 : 0};
            hipLaunchKernelGGL(assim_err_kernel, dim3(nr), dim3(256), 0, stream, ea);
            TRMF_HIP_CHECK(hipGetLastError());
        }
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
        // ---- commit ----
        TRMF_HIP_CHECK(hipMemcpyAsync(W.p + (size_t)first_row * KP, Wn.p, (size_t)nr * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (first_row < ad_rows) adapt_stale();                     // rows the series statistics absorbed have changed
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the new W
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
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
        const size_t V = (size_t)m * 64;
        if (Wn.alloc((size_t)m * KP) || (Wout && flat.alloc((size_t)m * k, false)) || U.alloc((size_t)m * k * k, false) || vec.alloc(7 * V) ||
            part.alloc((size_t)2 * m) || flag.alloc(1, false) || errs.alloc((size_t)2 * m, false) || objs.alloc((size_t)4 * m, false) || state.alloc(1))
            return kFail;
        TRMF_HIP_CHECK(hipMemsetAsync(flag.p, 0x7f, sizeof(int), stream));
        // stage A
        if (full) {
            if (y_times_factor(false, H.p, Bv.p, dense ? 0u : (uint32_t)first_row, (uint32_t)T)) return kFail;        // rows of Y H
            if (small_gram(H.p, n, real(0), GSx.p, stream)) return kFail;                                             // H^T H
        } else if (launch_gram_x_rows((uint32_t)first_row, (uint32_t)T)) return kFail;
        TRMF_HIP_CHECK(hipGetLastError());
        const real lamAR = (real)lambdaAR, lamI = (real)lambdaI;
        {
            AssimFactorArgs fa{Gmat(), full ? (size_t)0 : xp.gstride, gpacked ? 1 : 0, U.p, flag.p, lamI + lamAR, first_row, m, k};
            if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(assim_factor_kernel<decltype(N)::value>, dim3((m + 3) / 4), dim3(256), 0, stream, fa); }))
                return unsupported_rank();
            TRMF_HIP_CHECK(hipGetLastError());
        }
        // stage B
        SmoothArgs sa{};
        sa.W = W.p; sa.x0 = W.p + (size_t)first_row * KP; sa.Bv = Bv.p; sa.G = Gmat(); sa.gstride = full ? (size_t)0 : xp.gstride; sa.packed = gpacked ? 1 : 0;
        sa.grow = first_row; sa.U = U.p;
        sa.lag_set = lag_set.p; sa.theta = theta.p;
        sa.x = vec.p; sa.r = vec.p + V; sa.z = vec.p + 2 * V; sa.q = vec.p + 3 * V; sa.e = vec.p + 4 * V; sa.p[0] = vec.p + 5 * V; sa.p[1] = vec.p + 6 * V;
        sa.part_rz = part.p; sa.part_pq = part.p + m; sa.st = state.p; sa.flag = flag.p;
        sa.tol2 = rtol * rtol; sa.lamI = lamI; sa.lamAR = lamAR;
        sa.first_row = first_row; sa.m = m; sa.k = k; sa.KP = KP; sa.NT = NT; sa.nlag = nlag;
        if (smooth_pcg(sa, max_iter)) return kFail;
        const dim3 rows4((m + 3) / 4);
        {
            SmoothFinishArgs fa{W.p, sa.x, lag_set.p, theta.p, Wn.p, Wout ? flat.p : nullptr, objs.p, first_row, m, k, KP, NT, nlag};
            hipLaunchKernelGGL(smooth_finish_kernel, rows4, dim3(256), 0, stream, fa);
            AssimErrArgs ea{dense ? nullptr : Yr_ptr.p, dense ? nullptr : Yr_idx.p, dense ? nullptr : Yr_val.p, dense ? Yd_tn.p : nullptr, H.p,
                            W.p, Wn.p, 0, first_row, errs.p, first_row, m, n, KP, full ? 1 : 0};
            hipLaunchKernelGGL(assim_err_kernel, dim3(m), dim3(256), 0, stream, ea);
            TRMF_HIP_CHECK(hipGetLastError());
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
        // ---- commit ----
        TRMF_HIP_CHECK(hipMemcpyAsync(W.p + (size_t)first_row * KP, Wn.p, (size_t)m * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (first_row < ad_rows) adapt_stale();                     // rows the series statistics absorbed have changed
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the new W
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
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
        std::vector<real> hthr((size_t)n);
        for (int j = 0; j < n; j++) hthr[j] = (real)c * (real)scale[j];
        DevBuf<real> xc, flat, U, vec, part, thr, wts, slab, Gs, bs;
        DevBuf<uint32_t> d_items, d_row;
        DevBuf<int> flag;
        DevBuf<double> objs, slab_d, score, rowsum;
        DevBuf<SmoothState> state;
        SyncStreamOnExit drain(stream);
        const size_t V = (size_t)m * 64, ni = std::max<size_t>(nitems, 1);
        if (xc.alloc((size_t)m * KP, false) || (Wout && flat.alloc((size_t)m * k, false)) || U.alloc((size_t)m * k * k, false) || vec.alloc(7 * V) ||
            part.alloc((size_t)2 * m) || thr.upload(hthr.data(), n) || wts.alloc(std::max<uint64_t>(nw, 1), false) ||
            slab.alloc(ni * smooth_robust_slot_reals(KP), false) || Gs.alloc((size_t)m * k * k, false) || bs.alloc((size_t)m * KP, false) ||
            d_items.upload(hitems.data(), hitems.size()) || d_row.upload(hrow.data(), hrow.size()) || flag.alloc(1, false) ||
            objs.alloc((size_t)4 * m, false) || slab_d.alloc(ni * kSmoothRobustSlotD, false) || score.alloc(2 * ni * kSmoothRobustSlotD, false) ||
            rowsum.alloc((size_t)2 * m, false) || state.alloc((size_t)sweeps)) return kFail;
        TRMF_HIP_CHECK(hipMemsetAsync(flag.p, 0x7f, sizeof(int), stream));
        TRMF_HIP_CHECK(hipMemcpyAsync(xc.p, W.p + (size_t)first_row * KP, (size_t)m * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        const real lamAR = (real)lambdaAR, lamI = (real)lambdaI;
        SmoothRobustArgs ra{dense ? nullptr : Yr_ptr.p, dense ? nullptr : Yr_idx.p, dense ? nullptr : Yr_val.p, dense ? Yd_tn.p : nullptr, H.p, xc.p, thr.p,
                            wts.p, d_items.p, d_row.p, slab.p, slab_d.p, Gs.p, bs.p, rowsum.p, first_row, m, n, k, KP, 0};
        auto part_launch = [&](int score_only, double *sums) {
            if (!nitems) return true;
            SmoothRobustArgs a = ra;
            a.score = score_only; a.slab_d = sums;
            return with_nt(NT, [&](auto N) { hipLaunchKernelGGL(smooth_robust_part_kernel<decltype(N)::value>, dim3(nitems), dim3(256), 0, stream, a); });
        };
        if (!part_launch(1, score.p)) return unsupported_rank();
        SmoothArgs sa{};
        sa.W = W.p; sa.x0 = xc.p; sa.Bv = bs.p; sa.G = Gs.p; sa.gstride = (size_t)k * k; sa.packed = 0; sa.grow = 0; sa.U = U.p;
        sa.lag_set = lag_set.p; sa.theta = theta.p;
        sa.x = vec.p; sa.r = vec.p + V; sa.z = vec.p + 2 * V; sa.q = vec.p + 3 * V; sa.e = vec.p + 4 * V; sa.p[0] = vec.p + 5 * V; sa.p[1] = vec.p + 6 * V;
        sa.part_rz = part.p; sa.part_pq = part.p + m; sa.flag = flag.p;
        sa.tol2 = rtol * rtol; sa.lamI = lamI; sa.lamAR = lamAR;
        sa.first_row = first_row; sa.m = m; sa.k = k; sa.KP = KP; sa.NT = NT; sa.nlag = nlag;
        const dim3 rows4((m + 3) / 4);
        for (int s = 0; s < sweeps; s++) {
            if (!part_launch(0, slab_d.p)) return unsupported_rank();
            AssimFactorArgs fa{Gs.p, (size_t)k * k, 0, U.p, flag.p, lamI + lamAR, 0, m, k};
            if (!with_nt(NT, [&](auto N) {
                    hipLaunchKernelGGL(smooth_robust_fold_kernel<decltype(N)::value>, dim3(m), dim3(256), 0, stream, ra);
                    hipLaunchKernelGGL(assim_factor_kernel<decltype(N)::value>, dim3((m + 3) / 4), dim3(256), 0, stream, fa);
                })) return unsupported_rank();
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
        // ---- commit ----
        TRMF_HIP_CHECK(hipMemcpyAsync(W.p + (size_t)first_row * KP, xc.p, (size_t)m * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (first_row < ad_rows) adapt_stale();                     // rows the series statistics absorbed have changed
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the new W
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
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
        // the weights of the rows walked, gamma^(T - 1 - t), and the decay of what the tables hold
        std::vector<real> hom;
        if (gam != 1.0) {
            hom.resize((size_t)std::max(m, 1));
            for (int i = 0; i < m; i++) hom[i] = (real)std::pow(gam, (double)(T - 1 - (row0 + i)));
        }
        const real decay = (real)std::pow(gam, (double)m);
        // sparse storage: where each column's walk starts; the init pass cuts long columns into items
        std::vector<uint32_t> hstart, hfirst, hitems;
        if (!dense) {
            hstart.resize((size_t)n);
            for (int j = 0; j < n; j++) hstart[j] = (uint32_t)(host_col_ptr[j] + (init ? 0u : ad_cnt[j]));
        }
        if (init && !full) {
            uint64_t chunk = std::max<uint64_t>(kAdaptChunk, (nnz + kAdaptMaxItems - 1) / kAdaptMaxItems);
            if (const char *e = test_env("TRMF_ADAPT_CHUNK")) chunk = (uint64_t)std::max(1, atoi(e));      // tests: several items per series on a small shape
            hfirst.resize((size_t)n + 1);
            for (int j = 0; j < n; j++) {
                hfirst[j] = (uint32_t)(hitems.size() / 2);
                if (host_col_ptr[j + 1] - host_col_ptr[j] > chunk)
                    for (uint64_t b = host_col_ptr[j]; b < host_col_ptr[j + 1]; b += chunk) {
                        hitems.push_back((uint32_t)b); hitems.push_back((uint32_t)std::min<uint64_t>(b + chunk, host_col_ptr[j + 1]));
                    }
            }
            hfirst[n] = (uint32_t)(hitems.size() / 2);
        }
        const uint32_t nitems = (uint32_t)(hitems.size() / 2);
        DevBuf<real> Hn, chg, mx, om, slab, U;
        DevBuf<uint32_t> d_start, d_first, d_items;
        DevBuf<int> flag;
        DevBuf<double> errs;
        SyncStreamOnExit drain(stream);
        if (Hn.alloc((size_t)n * KP) || chg.alloc(n, false) || mx.alloc(1) || flag.alloc(1, false) || errs.alloc((size_t)4 * std::max(m, 1), false) ||
            (!hom.empty() && om.upload(hom.data(), hom.size())) || (!dense && d_start.upload(hstart.data(), hstart.size())) ||
            (nitems && (d_first.upload(hfirst.data(), hfirst.size()) || d_items.upload(hitems.data(), hitems.size()) ||
                        slab.alloc((size_t)nitems * adapt_part_reals(k), false))) ||
            (full && U.alloc((size_t)k * k, false))) return kFail;
        TRMF_HIP_CHECK(hipMemsetAsync(flag.p, 0x7f, sizeof(int), stream));
        const real *omp = hom.empty() ? nullptr : om.p;
        const real *Sin = init ? nullptr : ad_S[in].p, *rin = init ? nullptr : ad_r[in].p;
        if (!full) {
            AdaptArgs a{Yc_ptr.p, Yc_idx.p, Yc_val.p, d_start.p, W.p, omp, Sin, rin, ad_S[out].p, ad_r[out].p, nitems ? d_first.p : nullptr,
                        nitems ? d_items.p : nullptr, nitems ? slab.p : nullptr, H.p, Hn.p, chg.p, flag.p, decay, (real)lambdaI, row0, n, k, KP};
            if (!with_nt(NT, [&](auto N) {
                    if (nitems) hipLaunchKernelGGL(adapt_part_kernel<decltype(N)::value>, dim3(nitems), dim3(64), 0, stream, a);
                    hipLaunchKernelGGL(adapt_series_kernel<decltype(N)::value>, dim3(n), dim3(64), 0, stream, a);
                })) return unsupported_rank();
        } else {
            AdaptFullArgs a{dense ? nullptr : Yc_ptr.p, dense ? nullptr : Yc_idx.p, dense ? nullptr : Yc_val.p, dense ? nullptr : d_start.p,
                            dense ? Yd_nt.p : nullptr, W.p, omp, Sin, rin, ad_S[out].p, ad_r[out].p, U.p, H.p, Hn.p, chg.p, decay, row0, T, n, k, KP, NT};
            hipLaunchKernelGGL(adapt_full_gram_kernel, dim3((unsigned)((PK + 255) / 256)), dim3(256), 0, stream, a);
            hipLaunchKernelGGL(adapt_full_rhs_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, a);
            AssimFactorArgs fa{ad_S[out].p, (size_t)0, 1, U.p, flag.p, (real)lambdaI, 0, 1, k};       // the one shared system: "series 0" names it
            if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(assim_factor_kernel<decltype(N)::value>, dim3(1), dim3(256), 0, stream, fa); }))
                return unsupported_rank();
            hipLaunchKernelGGL(adapt_full_subst_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, a);
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
        if (m > 0) {   // the squared errors of the absorbed rows with H as it is and as it will be (assim_err_kernel's reading of an entry)
            for (int pass = 0; pass < 2; pass++) {
                AssimErrArgs ea{dense ? nullptr : Yr_ptr.p, dense ? nullptr : Yr_idx.p, dense ? nullptr : Yr_val.p, dense ? Yd_tn.p : nullptr,
                                pass ? Hn.p : H.p, W.p, W.p, 0, 0, errs.p + (size_t)2 * m * pass, row0, m, n, KP, full ? 1 : 0};
                hipLaunchKernelGGL(assim_err_kernel, dim3(m), dim3(256), 0, stream, ea);
            }
        }
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
        // ---- commit ----
        TRMF_HIP_CHECK(hipMemcpyAsync(H.p, Hn.p, (size_t)n * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the new H
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
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
        std::vector<real> hom;
        if (gam != 1.0) {
            hom.resize((size_t)std::max(m, 1));
            for (int i = 0; i < m; i++) hom[i] = (real)std::pow(gam, (double)(T - 1 - (row0 + i)));
        }
        const real decay = (real)std::pow(gam, (double)m);
        std::vector<uint32_t> hstart((size_t)n), hwptr((size_t)n + 1);
        std::vector<real> hthr((size_t)n);
        hwptr[0] = 0;
        for (int j = 0; j < n; j++) {
            hstart[j] = (uint32_t)(host_col_ptr[j] + ad_cnt[j]);
            hwptr[j + 1] = hwptr[j] + (uint32_t)(host_col_ptr[j + 1] - host_col_ptr[j] - ad_cnt[j]);
            hthr[j] = (real)c * (real)scale[j];
        }
        const size_t nw = hwptr[n];
        DevBuf<real> Hn, chg, mx, om, thr, wts;
        DevBuf<uint32_t> d_start, d_wptr, wrw;
        DevBuf<int> flag;
        DevBuf<double> errs, obj;
        SyncStreamOnExit drain(stream);
        if (Hn.alloc((size_t)n * KP) || chg.alloc(n, false) || mx.alloc(1) || flag.alloc(1, false) || errs.alloc((size_t)4 * std::max(m, 1), false) ||
            (!hom.empty() && om.upload(hom.data(), hom.size())) || d_start.upload(hstart.data(), hstart.size()) ||
            d_wptr.upload(hwptr.data(), hwptr.size()) || thr.upload(hthr.data(), hthr.size()) || wts.alloc(std::max<size_t>(nw, 1), false) ||
            wrw.alloc(std::max<size_t>(nw, 1), false) || obj.alloc((size_t)2 * n, false)) return kFail;
        TRMF_HIP_CHECK(hipMemsetAsync(flag.p, 0x7f, sizeof(int), stream));
        AdaptRobustArgs a{Yc_ptr.p, Yc_idx.p, Yc_val.p, d_start.p, W.p, hom.empty() ? nullptr : om.p, ad_S[in].p, ad_r[in].p, ad_S[out].p, ad_r[out].p,
                          H.p, Hn.p, chg.p, flag.p, thr.p, d_wptr.p, wts.p, wrw.p, obj.p, decay, (real)lambdaI, row0, n, k, KP, NT, sweeps};
        if (!with_nt(NT, [&](auto N) { hipLaunchKernelGGL(adapt_robust_series_kernel<decltype(N)::value>, dim3(n), dim3(64), 0, stream, a); }))
            return unsupported_rank();
        hipLaunchKernelGGL(adapt_robust_objective_kernel, dim3(n), dim3(64), 0, stream, a);
        hipLaunchKernelGGL(adapt_max_kernel, dim3(1), dim3(256), 0, stream, chg.p, n, mx.p);
        if (m > 0) {   // the squared errors of the absorbed rows with H as it is and as it will be (unweighted; adapt_series' sums)
            for (int pass = 0; pass < 2; pass++) {
                AssimErrArgs ea{Yr_ptr.p, Yr_idx.p, Yr_val.p, nullptr, pass ? Hn.p : H.p, W.p, W.p, 0, 0, errs.p + (size_t)2 * m * pass, row0, m, n, KP, 0};
                hipLaunchKernelGGL(assim_err_kernel, dim3(m), dim3(256), 0, stream, ea);
            }
        }
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
        // ---- commit ----
        TRMF_HIP_CHECK(hipMemcpyAsync(H.p, Hn.p, (size_t)n * KP * sizeof(real), hipMemcpyDeviceToDevice, stream));
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the new H
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
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
    // New regularisation weights for the iterations enqueued from now on: the session's own copies (F-solve, Theta-solve, the
    // full-observation path's shared Gram) and the X-side parameter block every X-solve kernel receives by value.
    int set_lambdas(double lI, double lAR, double lLag) {
        if (sync()) return kFail;                 // (a recovery of a timed-out persistent kernel repeats iterations with the OLD weights)
        lambdaI = lI; lambdaAR = lAR; lambdaLag = lLag;
        xp.lambdaI = lI; xp.lambdaAR = lAR;
        return 0;
    }
    // L1 weight of the lag weights and the refit on the selected support, for the Theta-solves enqueued from now on (the caller has
    // validated l1).  (0, 0): the ridge path, exactly.
    int set_lag_penalty(double l1, int refit) {
        if (sync()) return kFail;
        if ((l1 > 0 || refit) && ensure_lasso_buffers()) return kFail;
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));        // (the record table's zero fill)
        lambdaLagL1 = l1; lag_refit = refit ? 1 : 0;
        return 0;
    }
    // The Theta phase on its own, from the current W with the current penalties; blocking.  The iteration counter and the log stay.
    int solve_lags() {
        if (sync()) return kFail;
        if (theta_solve(stream)) return kFail;
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        if (snap_iter >= 0 && take_snapshot()) return kFail;       // the recovery snapshot follows the new Theta
        TRMF_HIP_CHECK(hipStreamSynchronize(stream));
        return 0;
    }
    // Record of the last Theta-solve (the caller has synchronised the session): k x kLagRec, zeros after a ridge solve.
    int lag_stats(int32_t *per_dim, int32_t *capped, int32_t *refit_skipped) {
        std::vector<int> h((size_t)k * kLagRec, 0);
        if (lag_rec_valid && lag_rec.p && nlag > 0)
            TRMF_HIP_CHECK(hipMemcpy(h.data(), lag_rec.p, h.size() * sizeof(int), hipMemcpyDeviceToHost));
        int nc = 0, ns = 0;
        for (int t = 0; t < k; t++) { nc += h[(size_t)t * kLagRec + 2] != 0; ns += h[(size_t)t * kLagRec + 3] != 0; }
        if (per_dim) std::memcpy(per_dim, h.data(), h.size() * sizeof(int));
        if (capped) *capped = nc;
        if (refit_skipped) *refit_skipped = ns;
        return 0;
    }
};

}  // namespace trmf
