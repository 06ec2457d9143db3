// session_state.hpp -- the HBM-resident state of a TRMF session: every data member, in one place (round 5: session.hpp was a
// 2000-line monolith).  The layers above add behaviour only:
//   SessionState  ->  SessionTransport (session_transport.hpp: communicator gathers, peer-to-peer arenas, exchanges)
//                 ->  SessionFPhase    (session_fphase.hpp: the F-solve and its sharding / overlap)
//                 ->  SessionXPhase    (session_xphase.hpp: X-side Gram build, the forms of the CG, Theta)
//                 ->  SessionCore      (session.hpp: set-up, measure-once decisions, the ALS loop, recovery, statistics, forecasts)
//                 ->  TrmfSessionImpl  (session_online.hpp: growth and the sliding window, series churn, the online solves)
//
// HBM layout (all resident for the lifetime of a session):
//   Yc_*   CSC of Y viewed as CSR over items   (F-solve rows):  ptr u32[n+1], idx u32[nnz], val[nnz]
//   Yr_*   CSR of Y over timestamps            (X-side rows):   ptr u32[T+1], idx u32[nnz], val[nnz]
//   W      T x KP, H  n x KP   (KP = k rounded up to 16, zero padded, row-major, columns interleaved)
//   theta  |L| x k column-major (as the ABI delivers it)
//   G      T x k x k   cached per-timestamp Gram,  Bv  T x KP rhs,  lossrow  T doubles
//   CG     g, s, r/r1, d0/d1, Hd/Hd1, w_new, arbase: T x KP each; partial-sum arrays
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/trmf_abi.h"
#include "comm.hpp"
#include "dev_buf.hpp"
#include "full_kernels.hpp"
#include "generic_kernels.hpp"
#include "resident_kernels.hpp"
#include "theta_kernels.hpp"

namespace trmf {

std::shared_ptr<Comm> active_comm();   // trmf_abi.hip

// ---- host-side dispatch on a rank bucket: run-time value -> template argument ------------------------------------------------
// f(std::integral_constant<int, V>{}) for the V of the list that equals v.  Exact match only: returns false when none does, and
// the caller reports that (SessionState::unsupported_rank) instead of running some other instantiation.
template <int... Vs, class F> bool dispatch_int(int v, F &&f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
template <class F> bool with_nt(int nt, F &&f) { return dispatch_int<1, 2, 3, 4>(nt, f); }                        // column tiles of a rank <= 64
template <class F> bool with_nt0(int nt, F &&f) { return dispatch_int<0, 1, 2, 3, 4>(nt, f); }                    // ... or 0: the generic ranks' bucket
template <class F> bool with_kq(int kq, F &&f) { return dispatch_int<8, 16, 24, 32, 40, 48, 56, 64>(kq, f); }     // rank rounded up to 8 (KMAX, hv_kq)

struct SessionState {
    // problem
    int T = 0, n = 0, k = 0, KP = 0, NT = 0, KMAX = 0, nlag = 0, midx = 0;
    uint64_t nnz = 0;
    double lambdaI = 0, lambdaAR = 0, lambdaLag = 0;
    int period_W = 1, period_H = 1, period_Lag = 2, verbose = 0;
    bool log_norms = true;       // ||.||^2 records of the iteration log (the reference: only under verbose)
    int max_cg_iter = 20;        // 10 * 2, trmf.h:90-93 folded by trmf.cpp:603-606
    int max_cg() const { return (int)std::min<long long>(max_cg_iter, (long long)T * k); }   // the CG cap of an X-solve, trmf.cpp:523-526
    // The acceptance test takes f(w) - f(w + s) from the CG's own recurrence (tron_accept(), cg_kernels.hpp).  TRMF_TEST +
    // TRMF_CG_DIRECT=1 adds one operator pass per solve as a diagnostic (s^T H s directly: TrmfIterStats.cg_rnorm_direct, the direct
    // actred); the iterates are the same either way unless a step is rejected, which has not been seen.
    bool cg_direct = test_env("TRMF_CG_DIRECT") != nullptr && atoi(test_env("TRMF_CG_DIRECT")) != 0;
    double eps_cg = 0.1;
    int iter = 0;                // ALS iterations done so far
    // distribution
    std::shared_ptr<Comm> comm;      // shared with the library: outlives trmf_dist_finalize() while the session lives
    std::vector<uint64_t> fbounds, xbounds;   // row partitions of items / timestamps
    // device
    hipStream_t stream = nullptr;
    DevBuf<uint32_t> Yc_ptr, Yc_idx, Yr_ptr, Yr_idx, lag_set, lag_steps;   // lag_steps: ar_lag_steps() of the lag set
    int nsteps = 0;
    bool has_lag0 = false;       // the lag set contains lag 0 (trmf_session_assimilate refuses it: a row would be its own prior)
    DevBuf<real> Yc_val, Yr_val, W, H, theta, G, Bv, g, s, r, r1, d0, d1, Hd, Hd1, w_new;
    DevBuf<double> lossrow, partials, theta_part;
    // full-observation path (missing == 0)
    bool full = false, dense = false;
    DevBuf<real> Yd_tn, Yd_nt;                // dense Y as T x n and as n x T (both row-major)
    DevBuf<real> Bf, GSf, GSx, Uf;            // F-side right-hand sides (n x KP), shared Grams (k x k), Cholesky factor of GSf
    DevBuf<double> gemm_part, sgram_part;
    double trYTY = 0;
    static constexpr int kGemmChunks = 32, kSmallGramBlocks = 256;
    DevBuf<XState> xstate;
    DevBuf<DeviceIterLog> log;
    static constexpr int kLogCap = 4096;
    std::vector<PhaseEvents> events;
    static constexpr int kEventRing = 64;
    int nbe = 1, nba = 1, rpb = 1;            // grids of the elementwise / apply kernels
    bool generic = false;                     // 64 < k <= 1024: generic_kernels.hpp for the Grams / the F-solve, unfused CG
    DevBuf<real> gen_scratch, theta_scratch;  // k x k systems of the generic F-solve; |L| x |L| systems of long lag sets
    bool gpacked = false;                     // unfused path: G holds upper triangles (packed_gram_elems(k) per timestamp), apply_kernel<true>
    int tile_TI = 0, nbt = 1;                 // fused Hv kernel: timestamps per tile (0 = unfused path), tiles of the problem
    int tile_nth = 256;                       // threads of a tile's workgroup: 256, or 512 (wide tiles, one rank: one workgroup per CU)
    // fused path: per-tile records of each launch (cg_kernels.hpp "per-tile partial records") in three message buffers:
    // CG launches of even / odd iteration, gradient + plain launch.  tsh: the one-rank view (one slot, every tile);
    // tsh_rank: this rank's block of tiles when the CG is sharded over time (ts_possible).
    DevBuf<double> xmsg_own[3];               // backing store of the messages unless they live in the peer-to-peer arena
    double *xm[3] = {nullptr, nullptr, nullptr};
    TileShard tsh{}, tsh_rank{};
    // peer-to-peer exchange (TRMF_CG=p2p; cg_kernels.hpp "peer-to-peer form of the exchange"): messages + flag words of
    // this rank in one IPC-exported arena, the peers' arenas opened, the pointer table in device memory
    struct P2p {
        bool on = false;                      // arena allocated, exported, mapped by every peer, and the trial exchange passed on EVERY rank
        bool loopback = false;                // solo communicator: the peers' pointers are this rank's own arena (never IPC-opened)
        void *arena = nullptr;
        size_t bytes = 0;
        std::vector<void *> peer;             // opened arenas of the other ranks (own slot: nullptr)
        unsigned long long epoch[3] = {0, 0, 0};
        double *msg[3] = {nullptr, nullptr, nullptr};   // this rank's three messages inside the arena
        size_t ext_off = 0, ext_bytes = 0;    // tail of the arena: the persistent kernel's record table + tagged vector rows (cg_persist.hpp, SHARD)
        size_t ext_ll_bytes = 0;
        std::string note;                     // why the peer-to-peer transport is unavailable (empty: available or not tried)
    } p2p;
    bool p2p_use = false;                     // transport of the CURRENT X-solve (select_transport)
    DevBuf<PeerTable> peer_table;
    std::vector<uint64_t> tbounds;            // tile-aligned timestamp partition of the time-sharded CG
    bool ts_possible = false;
    // Form of the multi-GPU X-solve: the CG replicated on every rank, or sharded over time with the
    // per-launch exchange through the communicator or peer to peer.  Forced by TRMF_CG, else measured once: every candidate
    // runs two X phases (the second timed on every rank), the slowest rank's time decides.  The peer-to-peer transport is
    // a candidate whenever its set-up (IPC arenas + a trial exchange with a short bound) succeeded on every rank.
    enum { kXRep = 0, kXTsComm = 1, kXTsP2p = 2, kXTsPersist = 3, kXForms = 4 };
    int x_form = kXRep;                       // the decided form; -1 while the candidates are being measured
    std::vector<int> x_cands;
    int x_calls = 0, cg_pred = 4;
    float x_ms[kXForms] = {0, 0, 0, 0};       // X phase of the measured call of each candidate (this rank)
    double x_ms_all[kXForms] = {0, 0, 0, 0};     // ... the slowest rank's (after the decision)
    hipEvent_t ts0 = nullptr, ts1 = nullptr;
    int ar_TI = 64, nbar = 1;                 // unfused path: timestamps per ar_tile_kernel workgroup, its partial-sum slots
    DevBuf<real> arbase;                      // lambdaI*v + lambdaAR*AR'(v) between ar_tile_kernel and apply_kernel
    XParams xp{};
    // Knobs that exist for the tests and the measurement scripts (forced failures, forced forms) are read only when
    // TRMF_TEST is set; INTEGRATION.md lists the production knobs.
    static bool test_knobs() { static const bool on = getenv("TRMF_TEST") != nullptr; return on; }
    static int unsupported_rank() { set_error("unsupported rank"); return kFail; }      // a dispatch_int() miss
    static const char *test_env(const char *name) {
        if (test_knobs()) return getenv(name);
        // a gated knob that is set but ignored says so, once per variable (a measurement script kept setting TRMF_FSHARD
        // after the gate went in and silently measured the default path)
        if (getenv(name)) {
            static std::mutex mu; static std::map<std::string, bool> told;
            std::lock_guard<std::mutex> lk(mu);
            if (!told[name]) { told[name] = true; fprintf(stderr, "[trmf] %s is a test knob: ignored unless TRMF_TEST is set\n", name); }
        }
        return nullptr;
    }

    // base of the partial-sum arrays: the session's own buffer, or -- peer-to-peer time-sharded unfused CG -- message 1 of the arena
    double *pbase_override = nullptr;
    // sum of squares of a device value array, fp64 (fixed order): the kernel is enqueued here, the partial sums are read by
    // finish_sum_squares() after the caller's next synchronisation of the stream
    static constexpr int kSumsqBlocks = 1024;
    DevBuf<double> sumsq_part;

    // Host copies of the two pointer arrays (8 bytes per row/column): row partitions, the byte model of
    // fsolve_bytes(), and the merged pointers of append_rows() are derived from them.
    std::vector<uint64_t> host_row_ptr, host_col_ptr;
    double ysq_acc = 0;          // sum of y^2 over every entry uploaded so far (fp64)

    // ---- set-up (trmf_session_create; the first part of every c_trmf_train call) ----------------------------------------
    // Everything is enqueued on the session's stream and the host waits ONCE, at the end: the caller's arrays travel through the
    // library's pinned ring (device_pool.hpp), the 64-bit pointers are narrowed on the way, the factors are padded / interleaved
    // and sum y^2 is formed on the device; device memory comes from the process-level pool, the stream from the stream cache.
    // Round 4 took 0.12 s for config 3 here (a hipMalloc + a synchronous pageable hipMemcpy per array, ~10 stream
    // synchronisations, ~30 hipFree at the end); profiles/r05_oneshot.txt has the split now.
    double t_upload_s = 0;       // seconds of create() spent reading the caller's arrays (TrmfTrainProfile.upload_s)
    double bytes_uploaded = 0;
    DevBuf<real> raw_W, raw_H;   // unpadded factor uploads: alive until the set-up's synchronisation
    static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    bool created = false;        // create() has finished: append_rows() re-tunes, alloc_time_scratch() inside create() does not

    static double sum_squares(const real *v, uint64_t count) {
        double acc = 0;
        for (uint64_t e = 0; e < count; e++) acc += (double)v[e] * (double)v[e];
        return acc;
    }
    // rows of a dense PyMatrix (either memory order) as one row-major block (append_rows: one window of new timestamps)
    static double dense_rows_to_rowmajor(const PyMatrix *Y, std::vector<real> &tn) {
        const size_t R = Y->rows, C = Y->cols;
        const real *v = (const real *)Y->val;
        tn.resize(R * C);
        if (Y->type == TRMF_DENSE_ROWMAJOR) std::memcpy(tn.data(), v, R * C * sizeof(real));
        else
            for (size_t j = 0; j < R; j++)
                for (size_t i = 0; i < C; i++) tn[j * C + i] = v[i * R + j];
        return 0;
    }
    void launch_transpose(const real *src, int rows, int cols, real *dst) {
        if (rows > 0 && cols > 0)
            hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0, stream, src, rows, cols, dst);
    }
    // full: do_dot_product(Y, Y) in val_type (trmf.cpp:184); observed-entries path: kept in double, it is the
    // constant of  loss(w) = sum y^2 + sum_i (w_i^T G_i w_i - 2 b_i.w_i)
    void set_trYTY() { trYTY = (full || dense) ? (double)(real)ysq_acc : ysq_acc; xp.trYTY = trYTY; }

    // ---- per-series affine transform of a resident dense Y (trmf_session_set_series_transform) -------------------------
    // rolling_validate(transform=True) -- the paper scripts' setting -- refits a NormalizedTransform on every growing
    // prefix (trmf.py:82-96, 237-249), which rescales EVERY entry of Y.  The session therefore keeps the raw matrix and
    // re-derives both training orientations from it on the device; only the 2n coefficients cross PCIe per window.
    DevBuf<real> Yraw;
    DevBuf<real> tr_a, tr_b;
    DevBuf<double> tr_part;
    bool has_transform = false;

    // ---- held-out positions (trmf_session_set_heldout / _eval_heldout; heldout_kernels.hpp) -------------------------------------
    // COO in the caller's CSR order, resident until replaced; append_rows leaves it alone, slide drops the positions in retired
    // rows and shifts the rest (csc_slide_kernel), change_series drops those in retired series and renumbers the rest (csr_churn_kernel).
    bool ho_set = false;
    uint64_t ho_m = 0, ho_chunk = kHoStep;
    int ho_nb = 1;                            // workgroups of one evaluation: kHoSums partials each in ho_part
    DevBuf<uint32_t> ho_row, ho_col;
    DevBuf<real> ho_val, ho_pred;
    DevBuf<double> ho_part, ho_sums;

    // ---- forecast scores (trmf_session_forecast / _forecast_scores / _forecast_reset; forecast_kernels.hpp) -------------------
    // Six fp64 sums per series, accumulated over every scored forecast since the last reset, and the last truth row of the
    // previous scored call (the naive-forecast term of MASE runs across calls).  Two generations of each: a call reads one and
    // writes the other, and fc_cur moves only once the whole call has succeeded.  append_rows, rewind, set_lambdas and
    // set_series_transform leave them alone -- a rolling evaluation does all of them between windows.
    DevBuf<double> fc_table[2];
    DevBuf<real> fc_prev[2];
    int fc_cur = 0;
    uint64_t fc_rows = 0;                     // forecast rows scored since the last reset
    // ---- forecast uncertainty (trmf_session_fit_noise / _set_noise / _forecast_dist / _interval_scores; uncertainty_kernels.hpp) --
    // The fitted (or set) observation noise per series and innovation variance per latent dimension, resident on every rank;
    // run, assimilate, append_rows and rewind neither refit nor invalidate them (the caller decides when to refit).  The interval
    // table: seven fp64 sums per series in two generations, switched after a call's last synchronisation like the point table.
    DevBuf<double> nz_sigma2, nz_q;
    bool nz_set = false;
    DevBuf<double> iv_table[2];
    int iv_cur = 0;
    uint64_t iv_rows = 0;
    // ---- online loading updates (trmf_session_series_stats_init / _adapt_series; adapt_kernels.hpp) ---------------------------------
    // Per series the packed S_j and r_j (one shared S on the full-observation forms), absent until asked for, resident on every
    // rank.  Two generations: a call reads ad_cur and writes the other, and ad_cur moves only once the flag has been read.  ad_cnt:
    // sparse storage, the stored entries of each column already absorbed (append_rows puts new entries behind them).  Stale once
    // a row they absorbed may have changed (adapt_stale(): run, rewind, assimilate below ad_rows, a new series transform) or rows
    // they never absorbed have been retired (slide past ad_rows).  change_series carries them -- kept series gathered, new series from
    // its fit -- when they are valid, per series and have absorbed every row; otherwise it releases them and leaves them stale.
    DevBuf<real> ad_S[2], ad_r[2];
    std::vector<uint32_t> ad_cnt;
    int ad_cur = 0, ad_rows = 0;
    bool ad_exists = false, ad_valid = false;
    double ad_gamma = 1;
    void adapt_stale() { ad_valid = false; }
    // fp32: four systems per wavefront (fsolve_quad_kernel); fp64: one system per wavefront, factorised in the MFMA
    // accumulator layout (fsolve_mfma_kernel)
    // X-side Gram build across ranks: sharded rows + all-gather of G (64 MB at config 3) pays only when a
    // rank's share of the gather is cheaper than the rows it no longer computes -- true on 8 GPUs, not on 2.
    // First call measures (kernel and gather time of every rank, exchanged through the communicator so that
    // all ranks take the same decision); TRMF_GRAMX=shard|replicate overrides.
    enum { kGramxMeasure = 0, kGramxShard = 1, kGramxReplicate = 2 };
    int gramx_mode = kGramxMeasure, gramx_calls = 0;
    hipEvent_t gx0 = nullptr, gx1 = nullptr, gx2 = nullptr;
    DevBuf<double> gramx_times;
    // Sharding a phase over the ranks pays only when the all-gather of its result costs less than the rows a rank no
    // longer computes (true for the F-solve at config 3 on 4 and 8 GPUs, not on 2).  Measure-once rule, shared by the
    // F-solve and the X-side Gram build: the first two calls run sharded, the second is timed on every rank (kernel, gather); the
    // times are exchanged through the communicator and every rank takes the same decision.
    enum { kShardMeasure = 0, kShardOn = 1, kShardOff = 2 };
    int fs_mode = kShardMeasure, fs_calls = 0;
    hipEvent_t fs0 = nullptr, fs1 = nullptr, fs2 = nullptr;
    // Overlapped all-gather of H (large item factors: config 5's is 512 MB): the rank's rows are solved in C launches of
    // equal nnz; chunk c of every rank's block is gathered on a side stream while launch c + 1 runs, the last chunk follows on
    // the solver stream, which then waits for the side stream -- only the last chunk's gather is exposed.  C = 2..4 by size
    // (one chunk per 16 MB of the rank's block); below kOverlapBytes per rank the extra launches' tails cost more than the
    // gather they hide (config 4).  TRMF_FOVERLAP=0 switches it off, =2..4 forces that many chunks at any size.
    static constexpr uint64_t kOverlapBytes = 16ull << 20;
    static constexpr int kMaxChunks = 4;
    hipStream_t side = nullptr;
    hipEvent_t emu_ready = nullptr, emu_end = nullptr;     // loop-back measurement under the solo communicator (xsolve_persist)
    hipEvent_t ov_b = nullptr, ov_c[kMaxChunks] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<uint64_t> fcut;               // (world x (chunks + 1)) rows: chunk c of rank r = [fcut[r*(C+1)+c], fcut[r*(C+1)+c+1])
    int fchunks = 0;
    // ---- the Theta-solve on a second stream (round 5) -------------------------------------------------------------------
    // The reference's loop is F-solve, X-solve, Theta-solve in sequence (trmf.cpp:647-693), but the data flow is looser: the
    // Theta-solve of iteration t reads W only and its result is first read by the X-solve of iteration t + 1, so it can run on a
    // stream of its own underneath the F-solve of iteration t + 1 (which reads W and writes H).  Same kernels, same operands: the
    // iterates do not change.  The solver stream waits for it before the next X-solve, and run() never returns with work
    // outstanding there.  A fork + join through events costs ~15-20 us on this platform (profiles/r05_streams.txt), so only a
    // LONG Theta-solve is moved: the paper scripts' shape (48 lags, 0.25 ms of 1 ms per iteration, +10 %), not config 3 (28 us,
    // measured: no gain) -- theta_overlap_pays().  Off under verbose / log_norms (their records are written in stream order) and
    // with TRMF_TEST + TRMF_NO_OVERLAP (A/B measurements, the bit-identity test).
    hipStream_t aux_theta = nullptr;
    hipEvent_t theta_fork = nullptr, theta_done = nullptr;
    bool theta_pending = false;
    bool theta_force_lds = false;             // TRMF_THETA_SOLVE=lds (a test knob, read at create): the LDS form of the ridge solve for every |L|
    // ---- sparse lag weights (trmf_session_set_lag_penalty; theta_kernels.hpp: theta_lasso_kernel) ------------------------------
    // lambdaLagL1 > 0 or lag_refit: the Theta-solve is theta_gram_kernel + theta_lasso_kernel (warm-started from the current
    // Theta, which is part of mark / rewind); both zero: today's ridge kernels, nothing else launched.  The fp64 systems of a lag
    // set too long for LDS live in lasso_scratch; lag_rec holds the k x kLagRec record of the last lasso solve.
    double lambdaLagL1 = 0;
    int lag_refit = 0;
    DevBuf<double> lasso_scratch;
    DevBuf<int> lag_rec;
    bool lag_rec_valid = false;               // the last Theta-solve enqueued was a lasso solve (the ridge path keeps no record)
    bool lag_lasso() const { return lambdaLagL1 > 0 || lag_refit != 0; }
    // lagged inner products: k T |L|^2 / 2 multiply-adds in a latency-bound kernel; 1e8 (config 3) = 28 us, 3.6e9 (paper shape) = 250 us
    bool theta_overlap_pays() const { return (double)k * (double)T * (double)nlag * (double)nlag >= (test_env("TRMF_OVERLAP_ALWAYS") ? 0.0 : 1e9); }
    bool overlap_ok() { return !verbose && !log_norms && !test_env("TRMF_NO_OVERLAP") && theta_overlap_pays() && ensure_aux() == 0; }
    int ensure_aux() {
        if (aux_theta) return 0;
        if (StreamCache::acquire(&aux_theta)) return kFail;
        for (hipEvent_t *e : {&theta_fork, &theta_done})
            if (!*e) TRMF_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        return 0;
    }
    int join_theta() {
        if (!theta_pending) return 0;
        theta_pending = false;
        TRMF_HIP_CHECK(hipStreamWaitEvent(stream, theta_done, 0));
        return 0;
    }
    // ---- the unfused CG follows its own stop (round 5) ------------------------------------------------------------------
    // The launch-per-step CG enqueues every step up to the cap because the host cannot know where the CG stops; the steps after
    // the stop return at once but still cost a dispatch each (2 x ~4.6 us x 13..15 unused steps = 0.12 ms of a 0.7 ms X phase at
    // the paper scripts' shape).  The deciding launch now also writes (solve sequence, step, stopped) into one word of pinned host
    // memory; the host stays kCgLook steps ahead of the device and stops enqueuing when it sees the stop: at most kCgLook no-op
    // steps, the device's queue never runs dry, no stream synchronisation.
    static constexpr int kCgLook = 2;
    unsigned int *cg_note = nullptr;          // pinned, mapped: (seq << 8) | (step << 1) | stopped
    unsigned int cg_seq = 0;
    bool cg_note_failed = false;
    int ensure_cg_note() {
        if (cg_note || cg_note_failed) return cg_note ? 0 : kFail;
        void *p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); cg_note_failed = true; return kFail; }
        cg_note = (unsigned int *)p;
        *cg_note = 0;
        return 0;
    }
    // ---- the X-solve as ONE persistent kernel (cg_persist.hpp) ---------------------------------------------------------------
    // One rank per GPU and the GPU to itself (world == 1): every tile's workgroup stays resident for the whole solve.  Needs all
    // workgroups co-resident (checked against the occupancy the runtime reports) and the LDS of the resident
    // vectors; otherwise -- or with TRMF_PERSIST=0 -- the launch-per-step path runs.  Bit-identical results either way.
    DevBuf<unsigned long long> ll_rec, ll_vec;   // tagged records / tagged vector rows (zero = never a valid tag)
    DevBuf<long long> persist_prof;           // -DTRMF_PERSIST_PROF builds: phase stamps of the last solve (printed by sync())
    uint32_t persist_epoch = 1;
    int persist_state = 0;                    // 0: not examined yet, 1: usable, -1: not
    template <int KQ, bool SHARD = false, int NTH = 256> int persist_prepare(size_t lds) {
        const void *fn = reinterpret_cast<const void *>(&cg_persist_kernel<KQ, SHARD, NTH>);
        if (lds > kLdsMax) return 0;
        if (lds > kLdsDefault && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
        int per_cu = 0, dev = 0;
        hipDeviceProp_t prop;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, NTH, lds) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
            hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
        // (256-thread blocks are admitted per CU up to min(API answer, 8, 800 / (ceil(sgprs / 16) * 16 + 16)), same guide: 6 at this
        // kernel's ~106 SGPRs -- the register-bound answer of 2..3 is always the smaller one; capped anyway)
        return std::min(per_cu, NTH == 256 ? 4 : 1) * prop.multiProcessorCount;
    }
    template <int KQ, bool SHARD = false, int NTH = 256> int persist_launch(const PersistArgs &pa, size_t lds) {
        // a plain launch: the grid was checked against the occupancy in persist_prepare(); hipLaunchCooperativeKernel gives the same
        // residency for 15-19 us more host time per launch (MI355X guide, "coop-launch")
        hipLaunchKernelGGL((cg_persist_kernel<KQ, SHARD, NTH>), dim3(SHARD ? tsh_rank.ntiles : nbt), dim3(NTH), lds, stream, xp, xstate.p, pa);
        TRMF_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // How many ranks drive the device that hosts the most of them (1 on a real node: one process per GPU).  Persistent kernels of
    // several processes on ONE device only make progress while all of them are scheduled at once.  Measured with processes standing
    // in for GPUs (profiles/r04_persist_notes.txt): 2 processes fine; 4 fine while their other kernels are short, but time-sliced to
    // ~7 s per solve when every rank also runs the full F-solve (a 30 s poll bound lets it finish: slow progress, no lost data); 8
    // processes ~30 s per solve; even 2 processes occasionally miss the 2 s bound (it won the measurement and then timed out in a later
    // solve of the full-size test).  Where ranks SHARE a device the measure-once rule therefore leaves that form out (TRMF_CG=persist
    // still forces it); with a device per rank every poll stays bounded (2 s) and a trial that times out only loses the candidate.
    int max_ranks_per_device = 1;
    // several ranks: every rank's tiles in one persistent kernel, tables in the IPC arenas (cg_persist.hpp, SHARD)
    int persist_shard_state = 0;
    bool persist_failed = false;
    std::string persist_note;
    // Multi-GPU, unfused path: shard the cached-Gram product of every CG step.  It pays when the
    // rows a rank no longer streams (T k^2 s (1 - 1/N) bytes at ~4 TB/s) outweigh an all-gather of T KP s bytes per
    // step (latency ~40 us + bytes over the rank's xGMI links); the fused one-launch-per-step path is faster
    // replicated at the sizes it covers.  TRMF_CG=shard|replicate overrides.
    bool cg_shard = false;
    static constexpr int kShardSlots = 4096;
    int apply_slots = 1;         // partial-sum slots (= workgroups of apply_kernel) per rank when sharded
    // Time-sharded UNFUSED CG (round 3): like the fused path's, a rank owns a contiguous block of AR
    // tiles -- its timestamps -- and runs every kernel of the solve on that block only: ar_tile_kernel (vector updates, AR
    // operator), apply_kernel (cached-Gram product), the element-wise kernels.  Per step the ranks exchange the midx first /
    // last rows of d, r and H d (edge_pack_kernel -> one all-gather of equal slots -> halo_unpack_kernel) and their slots of
    // the partial-sum arrays, in one grouped round; nothing T-sized is gathered (the sharded Gram product above gathers the
    // rows of H d, T KP values, every step).  The host follows the CG's stop as in the fused path.
    bool uts = false;
    TileShard ush{};                          // rank / world / rows / edge-slot geometry (no records: the unfused kernels keep arrays)
    std::vector<uint64_t> ubounds;            // AR-tile-aligned timestamp partition
    DevBuf<double> umsg;                      // edge message: world slots of 2 sides x 3 vectors x midx rows
    double *umsg_ptr = nullptr;               // = umsg.p (communicator transport)
    unsigned u_exchanges = 0;                 // peer to peer: exchanges issued so far (selects the edge message, 0 or 2)
    int u_tile0 = 0, u_ntiles = 0, u_tpr = 0, wn_slots = 1;
    // one grouped exchange of the time-sharded unfused CG: edge rows of nvec vectors + this rank's slots of partial arrays
    // (kind 0: apply_kernel's slots, 1: ar_tile_kernel's, 2: wnew_kernel's)
    struct PartialRef { int slot, kind; };

    // ---- split rows (round 6; gram_kernels.hpp "split rows") ------------------------------------------------------------------
    // The row kernels map rows to wavefronts statically (four item rows / one timestamp per wavefront); the reference schedules rows
    // dynamically (trmf.cpp:371, :234,252,273) and has no cliff at a long row.  Per orientation, rows of at least `thresh` entries are
    // cut into items of `chunk` consecutive entries (a row of more than 256 chunks: into 256 equal items), processed one item per
    // wavefront, and their partial Grams summed in item order.  thresh: what a wavefront slot would carry if the whole orientation
    // were spread evenly over 8 rounds of the chip's resident wavefronts -- never below the length where the row kernels are still
    // balanced by the hardware's workgroup dispatch (512 entries for the fp32 F-solve's four rows per wavefront, 2048 for the
    // one-row-per-wavefront kernels), so BASELINE's uniform workloads (rows of ~100 / ~1000 entries) never take this path and keep
    // their results bit for bit.  TRMF_TEST + TRMF_LONG_ROW=<entries> (0: never) / TRMF_LONG_CHUNK=<entries> force the geometry.
    struct LongRows {
        uint32_t thresh = 0xffffffffu, chunk = 1024;
        std::vector<uint32_t> rows, first;    // host copies: ids of the long rows (ascending), first item of each (+ one past the last)
        DevBuf<uint32_t> d_rows, d_first, d_items;   // d_items: (begin, end) entry positions per item
        DevBuf<uint32_t> d_order;             // skewed: every row of the orientation, longest first (gram_x_kernel's dispatch order)
        uint32_t nitems = 0;
        uint64_t nnz_long = 0;
        bool skewed = false;                  // among the rows that stay on the row kernels the longest is >= 2x the mean (and the mean >= 64 entries)
        bool any() const { return !rows.empty(); }
        void clear() { thresh = 0xffffffffu; skewed = false; rows.clear(); first.clear(); nitems = 0; nnz_long = 0; d_rows.release(); d_first.release(); d_items.release(); d_order.release(); }
        // positions [lo, hi) of the list whose rows lie in [rb, re)
        void range(uint32_t rb, uint32_t re, uint32_t &lo, uint32_t &hi) const {
            lo = (uint32_t)(std::lower_bound(rows.begin(), rows.end(), rb) - rows.begin());
            hi = (uint32_t)(std::lower_bound(rows.begin(), rows.end(), re) - rows.begin());
        }
    } longF, longX;
    DevBuf<real> part_slab;                   // partial Grams of the items of ONE orientation at a time (F-solve, then X-side Gram)
    uint32_t part_stride = 0;                 // reals per item: upper tiles in accumulator layout + the lane groups' rhs partials
    static constexpr uint32_t kSplitMaxItemsPerRow = 256;
    int build_long_rows(LongRows &L, const std::vector<uint64_t> &ptr, size_t nrows, uint32_t lo_entries, int resident_waves, bool want_order = false) {
        L.rows.clear(); L.first.clear(); L.nitems = 0; L.nnz_long = 0;
        const uint64_t total = nrows ? ptr[nrows] - ptr[0] : 0;
        uint64_t th = (total / (8ull * (uint64_t)std::max(resident_waves, 1)) + 15) / 16 * 16;
        th = std::min<uint64_t>(std::max<uint64_t>(th, lo_entries), 8192);
        L.thresh = (uint32_t)th; L.chunk = std::max<uint32_t>(1024u, L.thresh);
        if (const char *e = test_env("TRMF_LONG_ROW")) { const long v = atol(e); L.thresh = v <= 0 ? 0xffffffffu : (uint32_t)v; L.chunk = std::max<uint32_t>(16u, std::min<uint32_t>(L.chunk, (L.thresh + 15) / 16 * 16)); }
        if (const char *e = test_env("TRMF_LONG_CHUNK")) L.chunk = std::max<uint32_t>(16u, ((uint32_t)atol(e) + 15) / 16 * 16);
        std::vector<uint32_t> items;
        uint64_t short_max = 0, short_sum = 0, short_rows = 0;
        for (size_t r = 0; r < nrows; r++) {
            const uint64_t len = ptr[r + 1] - ptr[r];
            if (len < L.thresh) { short_max = std::max(short_max, len); short_sum += len; short_rows += len > 0; continue; }
            const uint32_t per = std::max<uint32_t>(L.chunk, (uint32_t)(((len + kSplitMaxItemsPerRow - 1) / kSplitMaxItemsPerRow + 15) / 16 * 16));
            L.rows.push_back((uint32_t)r); L.first.push_back(L.nitems);
            for (uint64_t e0 = ptr[r]; e0 < ptr[r + 1]; e0 += per) {
                items.push_back((uint32_t)e0); items.push_back((uint32_t)std::min<uint64_t>(e0 + per, ptr[r + 1]));
                L.nitems++;
            }
            L.nnz_long += len;
        }
        L.first.push_back(L.nitems);
        L.skewed = short_rows > 0 && short_sum >= 64 * short_rows && short_max * short_rows >= 2 * short_sum;
        if (L.skewed && want_order) {
            std::vector<uint32_t> ord(nrows);
            for (size_t r = 0; r < nrows; r++) ord[r] = (uint32_t)r;
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
                const uint64_t la = ptr[a + 1] - ptr[a], lb = ptr[b + 1] - ptr[b];
                return (la >= L.thresh ? 0 : la) > (lb >= L.thresh ? 0 : lb);       // split rows return at once: with the empty ones, last
            });
            if (L.d_order.upload(ord.data(), ord.size())) return kFail;
        } else L.d_order.release();
        if (L.rows.empty()) { L.d_rows.release(); L.d_first.release(); L.d_items.release(); return 0; }
        return L.d_rows.upload(L.rows.data(), L.rows.size()) || L.d_first.upload(L.first.data(), L.first.size()) || L.d_items.upload(items.data(), items.size()) ? kFail : 0;
    }
    SplitRows split_view(const LongRows &L, uint32_t lo, uint32_t hi) const { return SplitRows{L.d_rows.p, L.d_first.p, part_slab.p, part_stride, lo, hi}; }

    hipEvent_t xg1_event = nullptr;           // this iteration's PhaseEvents::xg1 (set by run())
    // Phase events of an iteration (TrmfIterStats.ms_*): seven hipEventRecords.  They are not free: each is a barrier packet between
    // two kernels that would otherwise be dispatched back to back -- measured 21-26 us per iteration (config 3: +2.5 % iterations/s
    // without them, config 2: +22 %, profiles/r05b_events.txt).  ev_period (trmf_session_set_timing): 1 = every iteration (default of
    // a session: every TrmfIterStats carries times), N > 1 = the iterations whose 1-based index is a multiple of N (bench.py: 3, so
    // that the samples alternate between iterations with and without a Theta-solve), 0 = none (c_trmf_train: nobody reads them).
    // An iteration without events reports ms_* = -1.
    int ev_period = 1;
    bool ev_on = true;                        // this iteration (set by run())
    std::vector<unsigned char> ev_valid;      // per slot of the event ring: that iteration's events were recorded
#define TRMF_EVREC(EV, STREAM) do { if (ev_on) TRMF_HIP_CHECK(hipEventRecord(EV, STREAM)); } while (0)

    // Dynamic LDS above the 64 KB every launch may use needs an explicit opt-in per kernel (gfx950: up to 160 KB
    // per workgroup); anything larger is an unsupported problem, reported instead of a failed launch.
    static constexpr size_t kLdsDefault = 64 * 1024, kLdsMax = 160 * 1024;
    template <typename Fn> int allow_dyn_lds(Fn fn, size_t bytes, const char *what) {
        if (bytes <= kLdsDefault) return 0;
        if (bytes > kLdsMax) { set_error(std::string(what) + ": needs more than 160 KB of LDS per workgroup"); return kFail; }
        TRMF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        return 0;
    }

    // ---- measure-once decisions, taken BEFORE the first iteration --------------------------------------------------------
    // With several ranks three things are decided by measurement (F rows sharded or not, X-side Gram rows sharded or not, the
    // form of the X-solve); each needs a couple of ordinary iterations and host synchronisations.  autotune() runs those
    // iterations right after the session is built (and after append_rows, which changes the geometry) on the real problem,
    // then puts W, H and Theta back and resets the iteration counter: the ALS loop proper never synchronises with the host,
    // and its timed window -- wherever a caller places it -- contains no measuring iterations.  Every form
    // computes the same iterates, so the decisions change speed only.  TRMF_AUTOTUNE=0 leaves the decisions to the first
    // iterations of run() as in round 3.
    static constexpr int kAutotuneMax = 14;
    int tuned_iters = 0;
    bool decisions_from_cache = false;

    // ---- recovery when the persistent kernel's co-residency assumption breaks (one rank; VERDICT / ADVICE r4) -----------------
    // The one-GPU X-solve is ONE kernel whose workgroups wait for each other; if something else holds compute units (a second
    // process on the GPU) a poll runs into its bound, the kernel ends with XState::p2p_error set and every later persistent
    // launch returns at once.  The iterates since then are void -- and a timeout in the last exchange can leave W half-updated
    // -- so the session keeps a snapshot of (W, H, Theta, iteration counter) as of its last CHECKED synchronisation: sync()
    // restores it, switches to the launch-per-step path (bit-identical iterates, no co-residency needed) for the rest of the
    // session's life and repeats the iterations since the snapshot.  Cost: three device-to-device copies per sync()
    // (18 MB at config 3, ~10 us), only while the persistent kernel is in use.
    DevBuf<real> snapW, snapH, snapT;
    int snap_iter = -1;
    // ---- mark / rewind (trmf_session_mark, trmf_session_rewind; round 6) ------------------------------------------------------
    // A caller-visible checkpoint of (W, H, Theta, iteration counter) on the device: bench.py repeats its timed window from the
    // same post-warm-up state (a 17 ms window is invisible to an external sampler), a grid search can rerun from a
    // common warm state.  Independent of the recovery snapshot above.
    DevBuf<real> markW, markH, markT;
    int mark_iter = -1;
};

}  // namespace trmf
