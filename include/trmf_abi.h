/*
 * trmf_abi.h -- C ABI of the MI355X-native TRMF ALS solver (drop-in for rofuyu/exp-trmf-nips16).
 *
 * Two shared objects export this interface, one per element type, found by the reference's own
 * loader glob (python/trmf/trmf.py:21-22,77-80; python/trmf/rf_util.py:19-32):
 *
 *     <pkg>/trmf/corelib/trmf_float32.so      (TRMF_REAL = float)
 *     <pkg>/trmf/corelib/trmf_float64.so      (TRMF_REAL = double)
 *
 * Section 1 is the reference's boundary, byte-for-byte (every declaration cites the reference
 * file:line it replaces).  Section 2 is build-owned (no reference counterpart): device control,
 * a resident-session API so that callers can keep Y and the factors in HBM across calls
 * (SURVEY.md section 8(f) rank 4, and what bench.py times), and the multi-GPU bootstrap.
 *
 * Everything is plain C: pointers, sizes, PODs.  No torch / C++ types cross this boundary.
 * There is no CPU fallback behind it: if no HIP device is usable the entry points print a
 * diagnostic on stderr and leave the outputs untouched (c_trmf_train is `void`, like the
 * reference's) or return a negative error code (section 2).
 */
#ifndef TRMF_ABI_H
#define TRMF_ABI_H

#include <stddef.h>
#include <stdint.h>

/* Only the entry points below are exported; everything else in the libraries has hidden
 * visibility so that trmf_float32.so and trmf_float64.so can live in one process. */
#if defined(__GNUC__) || defined(__clang__)
#define TRMF_API __attribute__((visibility("default")))
#else
#define TRMF_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Section 1 -- the reference boundary
 * ---------------------------------------------------------------------------------------------- */

/* Matrix type tags: reference rf_matrix.h:3400-3405. */
enum {
    TRMF_DENSE_ROWMAJOR = 1,
    TRMF_DENSE_COLMAJOR = 2,
    TRMF_SPARSE = 3,
    TRMF_EYE = 4
};

/* PyMatrix: reference rf_matrix.h:3407-3415 (C side) and rf_util.py:35-52 (ctypes mirror).
 * Natural alignment, sizeof == 80.  Non-owning views on caller (NumPy) buffers.
 *   dense : only `val` (rows*cols elements, row- or column-major per `type`)
 *   sparse: CSR = (row_ptr[rows+1], col_idx[nnz], val_t[nnz]);
 *           CSC = (col_ptr[cols+1], row_idx[nnz], val[nnz]); both always present.        */
typedef struct {
    uint64_t rows, cols, nnz;
    size_t *row_ptr;
    size_t *col_ptr;
    uint32_t *row_idx;
    uint32_t *col_idx;
    void *val;
    void *val_t;
    int32_t type;
} PyMatrix;

/* c_trmf_train: reference trmf.h:203-210, trmf.cpp:696-725; ctypes prototype trmf.py:23-43.
 *
 *   Y        T x n observations (rows = timestamps). SPARSE required when missing != 0.
 *   lag_set  ascending uint32[lag_size]
 *   W        T x k DENSE_ROWMAJOR   (temporal factor, in/out)
 *   H        n x k DENSE_ROWMAJOR   (item factor, in/out)
 *   lag_val  lag_size x k DENSE_COLMAJOR (AR weights Theta, in/out)
 *
 * One ALS iteration = H(F)-solve, W(X)-solve, Theta-solve every period_Lag iterations
 * (trmf.cpp:647-693).  Outputs are written in place; Y and lag_set are never written.
 * Dimension/layout violations print the reference's "[ERR MSG]" lines on stderr and return
 * without touching the outputs (trmf.cpp:561-596,632-634).  So does every later failure (device
 * error, out of memory): the three factors are staged on the host and committed together or not at all.  warm_start == 0 reproduces the
 * reference's behaviour: the reference rebuilds W, H and lag_val as
 * PRIVATE random matrices of matching shapes before its dimension check (trmf.cpp:547-558:
 * std::mt19937 seeded 0, uniform / normal draws in doubles cast to the element type), trains
 * those -- the ">> iter" lines under verbose describe that run -- and discards them: the
 * caller's arrays are not updated and no "[ERR MSG]" about the caller's shapes can appear.
 * Here the same generator calls give the same private starting point, the training runs on
 * the device, and nothing is written back (tests/test_abi.py replays a capture of the
 * reference's lines).  `threads` is accepted
 * and ignored (no OpenMP on the device path).
 *
 * Checks beyond the reference's (each prints one "[ERR MSG]: ..." line and returns like a
 * dimension error; the reference aborts on an assert, reads out of bounds or has no such limit):
 *   - missing != 0 with a dense Y                  (reference: assert, rf_matrix.h:180)
 *   - lag_set not ascending, max lag >= rows of Y  (reference: out-of-bounds reads)
 *   - rank k outside 1..1024, more than 1024 lags (ranks up to 64 and lag sets whose |L| x |L| systems fit LDS run the
 *     register-tiled kernels; beyond that generic kernels compute the same thing slowly -- csrc/generic_kernels.hpp --
 *     where rounds 1-3 answered "[ERR MSG]")
 *   - a SPARSE Y with nnz >= 2^32; Y with >= 2^24 - 1 rows or columns, or a factor table
 *     (rows+1) x 16*ceil(k/16) elements above 4 GiB     (32-bit device offsets)
 *   - a lag reach / lag count whose LDS tiles exceed 160 KB per workgroup (session creation)
 *
 * Deliberate differences inside the X-solve (documented in DESIGN.md section 1): the TRON loop of
 * the reference (rf_tron.h:134-254, folded to ONE outer iteration by trmf.cpp:603-606) retries a
 * rejected step without changing anything (quirk Q3); here a rejected step leaves W unchanged
 * and the iteration goes on.  The acceptance test uses the exact quadratic identity
 * f(w+s) - f(w) = g.s + s.Hs/2 instead of a second pass over the observations, so `actred`
 * agrees with the reference's to rounding, not bit for bit.
 * verbose >= 1 prints the reference's parameter dump on stdout and the per-half-step
 * ">> iter i F|X|LV v" lines on stderr; verbose >= 2 adds the TRON line on stdout.          */
TRMF_API void c_trmf_train(const PyMatrix *pyY, uint32_t *py_lag_set, uint32_t py_lag_size,
                  PyMatrix *pyW, PyMatrix *pyH, PyMatrix *pylag_val, int warm_start,
                  double lambdaI, double lambdaAR, double lambdaLag,
                  int32_t max_iter, int32_t period_W, int32_t period_H, int32_t period_Lag,
                  int32_t threads, int32_t missing, int32_t verbose);

/* ------------------------------------------------------------------------------------------------
 * Section 2 -- build-owned additions (no reference counterpart)
 * ---------------------------------------------------------------------------------------------- */

/* Where the wall time of the LAST completed c_trmf_train call of this process went (round 5).  The reference's entry wraps
 * the caller's buffers zero-copy (trmf.cpp:696-725); this one has to put the problem into HBM and bring the factors back:
 *   setup_s     validation, device memory (a process-level pool: device_mallocs counts the hipMalloc calls of THIS call, 0
 *               once the pool holds the shape), the caller's arrays through a pinned ring (upload_s of it: the time the host
 *               spent reading them; bytes_h2d), padding / narrowing on the device, events, the set-up's one synchronisation
 *   compute_s   max_iter ALS iterations enqueued + the final synchronisation
 *   download_s  factors -> pinned staging -> the caller's arrays, committed only when ALL of them have arrived
 *   teardown_s  releasing the session (buffers back to the pool, no hipFree)
 * total_s is measured around the whole call; the four parts add up to it. */
typedef struct {
    double total_s, setup_s, upload_s, compute_s, download_s, teardown_s;
    double bytes_h2d, bytes_d2h;
    int32_t iters, device_mallocs, pool_reused, failed;
} TrmfTrainProfile;
/* 0 and *out filled when a c_trmf_train call has completed in this process (and library), -1 otherwise. */
TRMF_API int32_t trmf_last_train_profile(TrmfTrainProfile *out);
/* Give back what the library keeps between calls on the selected device: pooled device memory (when no session is alive),
 * idle streams, the pinned upload ring (24 MB) and the pinned download staging, the idle worker threads / communicators of the TRMF_DEVICES mode.  TRMF_POOL_MAX_MB (default 8192, 0 = keep
 * nothing) bounds the pool.  Returns 0, or -1 when the selected device cannot be made current (trmf_last_error() says why). */
TRMF_API int32_t trmf_release_cached(void);

/* sizeof(element type) of this library: 4 or 8. */
TRMF_API int32_t trmf_sizeof_real(void);
/* Number of visible HIP devices (0 if none / runtime unusable). */
TRMF_API int32_t trmf_device_count(void);
/* Select the HIP device used by subsequent calls from this process (default 0). 0 on success. */
TRMF_API int32_t trmf_set_device(int32_t device);
/* Free bytes of HBM on the selected device right now (-1 if no device): sizing aid, and what the leak test reads. */
TRMF_API int64_t trmf_device_free_bytes(void);
/* Bytes of the selected device's pool that live buffers of this process hold right now (-1 if no device): what a session that is
 * meant to stay the same size -- a sliding window -- is checked against. */
TRMF_API int64_t trmf_device_pool_live_bytes(void);
/* Last error text of section-2 calls (static storage, never NULL). */
TRMF_API const char *trmf_last_error(void);

/* Per-iteration record filled by a session (mirrors the reference's verbose output:
 * trmf.cpp:661,672,687 and the TRON line rf_tron.h:219). Values are -1 when a phase did not run. */
typedef struct {
    double normF, normX, normLV;           /* ||H||^2, ||W||^2, ||Theta||^2 after each phase   */
    double f, fnew, actred, prered;        /* X-subproblem objective before/after, reductions  */
    double gnorm, cg_rnorm;
    int32_t cg_iter, accepted;
    float ms_F, ms_X, ms_LV;               /* HIP-event time of each phase on the solver stream; all ms_* are -1 for an
                                              iteration that carried no events (trmf_session_set_timing)         */
    float ms_F_kernel;                     /* HIP-event time of the F-solve kernel alone       */
    double delta;                          /* trust-region bound of the TRON line (rf_tron.h:195-219) */
    double cg_rnorm_direct;                /* |-g - H s| of the step evaluated directly; cg_rnorm is the CG's recurrence
                                              (-1 where not evaluated: only the one-GPU persistent kernel does)   */
    float ms_X_gram;                       /* HIP-event time from the start of the X phase to the end of its Gram build
                                              (gram_x_kernel + gathers); ms_X - ms_X_gram is the CG solve              */
    float reserved_;
} TrmfIterStats;

typedef struct TrmfSession TrmfSession;

/* Upload Y (both orientations), lag_set and the initial factors to HBM and build all device
 * scratch.  Same argument meaning and validation as c_trmf_train.  Returns NULL on failure
 * (see trmf_last_error()).  When a communicator is active (trmf_dist_init*), every rank must
 * call this with identical inputs; rows are partitioned inside.                               */
TRMF_API TrmfSession *trmf_session_create(const PyMatrix *Y, const uint32_t *lag_set, uint32_t lag_size,
                                 const PyMatrix *W, const PyMatrix *H, const PyMatrix *lag_val,
                                 double lambdaI, double lambdaAR, double lambdaLag,
                                 int32_t period_W, int32_t period_H, int32_t period_Lag,
                                 int32_t missing, int32_t verbose);
/* Enqueue `iters` further ALS iterations (iteration numbering continues across calls, so the
 * period_* gating matches one long c_trmf_train run).  Asynchronous unless verbose > 0.        */
TRMF_API int32_t trmf_session_run(TrmfSession *s, int32_t iters);
/* Switch the ||H||^2, ||W||^2, ||Theta||^2 records of TrmfIterStats on (default) or off.  The
 * reference evaluates these norms only under `verbose` (trmf.cpp:659-688); with the switch off the
 * fields read -1 and an iteration is about 30 us shorter.  c_trmf_train follows `verbose`.        */
TRMF_API int32_t trmf_session_log_norms(TrmfSession *s, int32_t on);
/* Which iterations carry the HIP events behind TrmfIterStats.ms_*: 1 = every iteration (default), N > 1 = the iterations whose
 * 1-based index is a multiple of N, 0 = none.  The seven event records of an iteration are barrier packets between kernels that
 * would otherwise be dispatched back to back: 21-26 us per iteration on an MI355X (2.5 % of a config-3 iteration, 22 % of a
 * config-2 one).  An iteration without events reports ms_* = -1; everything else of its record is unaffected.  c_trmf_train
 * records none.  No reference counterpart.                                                                                      */
TRMF_API int32_t trmf_session_set_timing(TrmfSession *s, int32_t period);
/* Append Ynew (Tn x n, NEW timestamps, same storage class -- sparse or dense -- as the session's Y) to the resident
 * problem: the rolling-window caller of the reference (python/trmf/trmf.py:303-329) retrains on a prefix that
 * grows by one window and warm-starts from the previous model (trmf.py:237-246).  Only the block (and, for a
 * sparse Y, one 4-byte pointer per item) is uploaded: CSR rows are appended, the CSC is rebuilt on the device,
 * a dense Y's second orientation is re-strided on the device, W gains Tn rows by the AR recursion with the
 * current lag weights (Model.latent_forecast, trmf.py:170-181); H and lag_val are kept.  The iteration counter
 * restarts at 1 like a fresh c_trmf_train call (period_* gating, trmf.cpp:647).  Blocking.  With a communicator
 * active every rank must call it with the same block. */
TRMF_API int32_t trmf_session_append_rows(TrmfSession *s, const PyMatrix *Ynew);
/* The sliding window: append Ynew (as trmf_session_append_rows does, with the same validation; NULL = nothing to append) AND
 * retire the `retire` oldest timestamps, in one new generation of storage (the data is passed over once, on the device; only the
 * block crosses PCIe).  retire == 0 with a block IS trmf_session_append_rows (one code path, the same bits).
 *
 * Contract: afterwards the session is the one trmf_session_create would build from
 *   - the retained entries in their STORED order, timestamps reduced by `retire`, followed (per row / per column) by the block's
 *     (the input need not be a canonical CSR/CSC pair: the column compaction on the device is stable),
 *   - W[retire:] followed by the AR roll-out of the block,
 *   - the current H, lag weights, lambdas, lag penalty and series transform (the raw matrix slides, the current coefficients
 *     are re-applied, sum y^2 is recomputed as a fresh session computes it),
 * and every later call -- run, assimilate*, smooth*, forecast*, objective, download -- returns the bits it returns on that fresh
 * session.  The iteration counter restarts, as after append_rows.  Blocking; with a communicator active every rank makes the
 * same call.  Failure-atomic: a refused or failed call leaves the session exactly as it was.
 *
 * Refused (trmf_last_error(); the session stays usable): retire < 0; retire larger than the rows held before the call (rows of
 * the block itself cannot be retired); fewer than (largest lag + 1) rows left after the append; everything append_rows refuses,
 * the 32-bit index limits applied to the sizes AFTER the slide; downdate_stats not 0 or 1; downdate_stats == 1 without valid
 * series statistics or on a full-observation form (dense storage, sparse storage with missing == 0: one shared S).
 *
 * Other resident state.  The mark is invalidated when rows are retired.  Noise tables, forecast scores and interval scores are
 * per series / per latent dimension and stay.  Held-out positions in retired rows are dropped, the others move up by `retire`
 * (trmf_session_eval_heldout then returns the sums of a fresh trmf_session_set_heldout of the shifted set).  Series statistics
 * (trmf_session_series_stats_init): absorbed_rows and the per-series absorbed counts drop by what was retired, so the entries
 * not yet absorbed remain the tail of every column.  downdate_stats == 1 (sparse storage, missing != 0) also subtracts every
 * retired entry's om_t w_t w_t^T and om_t y w_t, om_t = forget^(absorbed_rows - 1 - t), from S_j and r_j in stored order -- the
 * tables then describe the retained rows only (a rectangular window); H is not refitted, the next adapt_series does that.
 * downdate_stats == 0 leaves the tables as they are: the retired rows stay in them as exponentially forgotten history, which is
 * recursive least squares as usually run and the natural choice for forget < 1.  Retiring rows the tables have not absorbed
 * yet makes them stale; stale tables stay stale. */
typedef struct { uint64_t rows_retired, entries_retired, rows_appended, entries_appended, rows, entries; } TrmfSlideSums;
TRMF_API int32_t trmf_session_slide(TrmfSession *s, const PyMatrix *Ynew /* or NULL */, int32_t retire, int32_t downdate_stats,
                                    TrmfSlideSums *out /* or NULL */);
/* Series churn: retire series (columns of Y, rows of H) of a resident session and add a block of new ones, in one new generation of
 * storage; only the block crosses PCIe.  keep: n flags (non-zero: the series stays), NULL keeps all.  Ynew: rows() x m, the m new
 * series over ALL timestamps the session holds, same storage class as the session's Y (raw data under a series transform), NULL:
 * nothing to add.  Kept series keep their relative order and are renumbered densely from 0; the m new series follow them.
 *
 * Contract: afterwards the session is the one trmf_session_create would build from
 *   - the churned entries in their STORED order in both orientations: every CSR row = its entries of kept series with the series
 *     renumbered, then the block's entries of that row at series + n_kept; the CSC = the kept columns in order, each as stored,
 *     then the block's columns as delivered (the input need not be a canonical CSR/CSC pair: the compactions are stable).  Dense
 *     storage: both orientations (and the raw copy under a transform) hold the kept columns followed by the block,
 *   - the current W and lag weights, lambdas, lag penalty,
 *   - H = [H[keep]; H_new], the transform coefficients [a[keep]; tr_a_new], [b[keep]; tr_b_new],
 * and every later call returns the bits it returns on that fresh session.  The iteration counter restarts, as after append_rows
 * and slide.  Everything sized by the number of series is re-derived the way trmf_session_create derives it (F-row partition, split
 * rows, scratch, the measure-once decisions).  Blocking; with a communicator active every rank makes the same call.  Failure-atomic:
 * a refused or failed call leaves the session exactly as it was.
 *
 * H_new.  fit == 1 (ranks 1..64): every new series' loadings are fitted on the device from the resident W over all rows() rows,
 *   h_j = (S_j + lambdaI I)^-1 r_j,   S_j = sum_t om_t w_t w_t^T,   r_j = sum_t om_t y_tj w_t,   om_t = forget^(rows - 1 - t)
 * by the kernels of trmf_session_series_stats_init / _adapt_series run over the new columns (sums in stored order in the element
 * type, the same Cholesky and substitutions): sparse storage with missing != 0 sums over the stored entries of column j, the
 * full-observation forms (sparse with missing == 0, dense) over every timestamp with one shared S.  forget is the series
 * statistics' when they are carried (below), 1 otherwise.  A new series without entries gets h = 0 exactly when lambdaI > 0; with
 * lambdaI == 0 a system that is not positive definite is refused, the message names the new series.  fit == 0: Hnew (m x k,
 * row-major) or, NULL, zeros.
 *
 * Other resident state.  Series statistics: when they are valid, have absorbed every row (absorbed_rows == rows()), are per series
 * (sparse storage with missing != 0) and the call fits (or adds nothing), the kept series' tables are gathered and the new series'
 * tables are the ones the fit built, so a later adapt_series goes on from them; in every other case existing statistics become
 * stale.  Held-out positions in retired series are dropped, the others renumbered.  The forecast and interval score tables are
 * reset (rows_scored 0).  A fitted or set noise is invalidated: trmf_session_fit_noise / _set_noise must be called again.  The mark
 * is released.  W, the lag weights and the iteration log stay.
 *
 * out: series_before / series_retired / series_added / series and entries_retired / entries_added / entries count series and
 * stored entries (dense: cells); heldout_dropped the held-out positions lost; fitted / stats_carried say what the call did;
 * sq_err_new = sum over the new series' stored entries of (y - w_t . h_j)^2 with the new loadings, in fp64 (ranks 1..64, else 0).
 *
 * Refused (trmf_last_error(); the session stays usable): keep all zero with no block; a block whose row count differs from rows();
 * a storage class that differs from the session's; fit together with Hnew; fit with a block at rank above 64 (fit == 0 works at
 * every rank); a series transform set without both tr_a_new and tr_b_new, coefficients given without a transform, a coefficient that
 * is not finite, a zero in tr_a_new (y -> a y + b is undone by dividing by a; b may be zero: a centred series); a block entry
 * outside rows() x m; sizes beyond the 32-bit device indices; a block whose two orientations hold different entry counts.
 * keep == NULL with Ynew == NULL is a no-op that returns 0. */
typedef struct {
    uint64_t series_before, series_retired, series_added, series;
    uint64_t entries_retired, entries_added, entries;
    uint64_t heldout_dropped;
    int32_t  fitted;        /* the new series' loadings were fitted by the call */
    int32_t  stats_carried; /* the loading statistics are still valid */
    double   sq_err_new;    /* fp64: sum over the new series' stored entries of (y - w_t.h_j)^2, with the new loadings */
} TrmfChurnSums;
TRMF_API int32_t trmf_session_change_series(TrmfSession *s, const uint8_t *keep /* n flags, or NULL: keep all */,
                                            const PyMatrix *Ynew /* rows() x m, same storage class, or NULL */,
                                            int32_t fit /* 1: fit the new loadings on the device */,
                                            const void *Hnew /* m x k row-major, or NULL (fit == 0: NULL means zeros) */,
                                            const void *tr_a_new, const void *tr_b_new /* m each: needed iff a series transform is set */,
                                            TrmfChurnSums *out /* or NULL */);
/* Cell revisions: set or delete cells INSIDE the rows and series a resident session holds -- a reading that arrives after later
 * rows have been appended, a provisional value that is corrected, a reading that is retracted -- in one new generation of storage;
 * only the batch crosses PCIe.  rows / cols: the `count` cells, distinct; vals: their values in the library's element type (raw
 * data under a series transform; ignored where del[i]); del: non-zero flags the cells to delete, NULL: every edit is a set.
 *
 * Semantics -- the result depends on the SET of edits, not on their order in the batch.  Sparse storage: every stored copy of an
 * edited cell is removed from both orientations by a stable compaction (the other entries keep their stored order; the input need
 * not be a canonical CSR/CSC pair and a cell may be stored twice); each set then places ONE entry at the end of its CSR row and at
 * the end of its CSC column, the sets of one row in ascending series order, the sets of one column in ascending timestamp order.
 * A set on a stored cell is a replace, a set on an unstored cell an insert, a delete of an unstored cell a no-op counted in
 * `missed`.  Dense storage: sets overwrite the cell in both orientations -- under a series transform the RAW copy is edited and the
 * current coefficients are re-applied, as slide re-applies them -- and deletes are refused.
 *
 * Contract: afterwards the session is, bit for bit, the one trmf_session_create would build from the revised entries in that stored
 * order and the current W, H, lag weights, lambdas, lag penalty and series transform (sum y^2 is recomputed as a fresh session
 * computes it; split rows, the F-row partition, scratch and the measure-once decisions are re-derived as create derives them), and
 * every later call returns the bits it returns on that fresh session.  The iteration counter restarts, as after slide.  Blocking;
 * with a communicator active every rank makes the same call.  Failure-atomic: a refused or failed call leaves the session exactly
 * as it was.  No floating-point atomics.  count == 0 returns 0 and changes nothing.
 *
 * Refused (trmf_last_error(); the session stays usable): a row >= rows() or a series >= n; the same cell twice in one batch; a
 * delete on dense storage; update_stats not 0 or 1; update_stats == 1 without valid series statistics or on a full-observation
 * form (dense storage, sparse storage with missing == 0: one shared S); sizes beyond the 32-bit device indices (judged with every
 * edit counted as an insert).
 *
 * Other resident state.  W, H and the lag weights are not touched: re-solving (assimilate*, smooth*, adapt_series*, run) is the
 * caller's next call.  The mark stays valid.  Noise, forecast and interval tables are per series and stay.  The held-out set is
 * untouched: a revised cell that is also held out stays held out.  Series statistics: update_stats == 1 with tables that have
 * absorbed every row (absorbed_rows == rows()) subtracts every removed entry's om_t w_t w_t^T and om_t y w_t from S_j and r_j in
 * stored order and then adds the sets' terms in ascending timestamp, om_t = forget^(rows() - 1 - t), W as it is now; the per-series
 * absorbed counts become the new column lengths and stats_carried = 1.  H is not refitted, the next adapt_series does that.  With
 * update_stats == 0, or with tables that have not absorbed every row, existing tables become stale if a column has changed.
 *
 * out: edits = count; inserted / replaced / deleted / missed classify the edits; copies_removed counts stored entries removed (a
 * cell stored twice counts twice; dense: the cells overwritten); entries_before / entries the stored entries (dense: cells);
 * first_row / last_row the smallest / largest timestamp named by the batch (-1 for an empty batch). */
typedef struct {
    uint64_t edits, inserted, replaced, deleted, missed;   /* missed: a delete of a cell that is not stored (a no-op) */
    uint64_t copies_removed;                               /* stored entries removed (a cell stored twice counts twice) */
    uint64_t entries_before, entries;
    int32_t  first_row, last_row;                          /* smallest / largest timestamp touched, -1 if none */
    int32_t  stats_carried;
} TrmfReviseSums;
TRMF_API int32_t trmf_session_revise(TrmfSession *s, uint64_t count, const uint32_t *rows, const uint32_t *cols,
                                     const void *vals /* count values of the element type; ignored where del[i] */,
                                     const uint8_t *del /* count flags or NULL: all are sets */,
                                     int32_t update_stats, TrmfReviseSums *out /* or NULL */);
/* Stored entries per timestamp of a sparse session's Y right now (rows() values; what sizes the per-entry weights of the robust
 * calls after series have been retired).  -1 for dense storage. */
TRMF_API int32_t trmf_session_row_entries(TrmfSession *s, uint64_t *per_row /* rows() */);
/* Train on a[i] * y + b[i] of series (column) i instead of the raw dense Y the session holds (missing == 0 only):
 * the per-window NormalizedTransform of the reference's rolling_validate(transform=True) (python/trmf/trmf.py:82-96,
 * 237-249, 253-257), which rescales every entry of the growing prefix.  The session keeps the raw matrix (rows passed
 * to create / append_rows are always RAW) and re-derives both training orientations on the device.  The
 * coefficients are arrays of n values of THIS library's element type (they are fitted from Y and have its dtype);
 * y * a + b is evaluated in that type with the product and the sum rounded separately, as NumPy evaluates it; only
 * the 2n coefficients are uploaded.  a == NULL / b == NULL mean 1 / 0.  May be called again at any time (e.g. after
 * append_rows, with the coefficients refitted on the grown prefix). */
TRMF_API int32_t trmf_session_set_series_transform(TrmfSession *s, const void *a /* n */, const void *b /* n */);
/* Checkpoint of the session's (W, H, lag_val, iteration counter) ON THE DEVICE, and the way back to it: after rewind the
 * session continues exactly as it did after mark (the solver is deterministic).  One mark per session (a new one replaces the
 * old); append_rows and slide invalidate it.  Both block.  No reference counterpart (bench.py repeats its timed window with these). */
TRMF_API int32_t trmf_session_mark(TrmfSession *s);
TRMF_API int32_t trmf_session_rewind(TrmfSession *s);
/* Number of timestamps currently held by the session (rows of W). */
TRMF_API int32_t trmf_session_rows(TrmfSession *s);
/* Block until all enqueued work of the session has finished. */
TRMF_API int32_t trmf_session_sync(TrmfSession *s);
/* Copy the current factors back into caller PyMatrix views (same shapes as at create). */
TRMF_API int32_t trmf_session_download(TrmfSession *s, PyMatrix *W, PyMatrix *H, PyMatrix *lag_val);
/* Copy the stats of the last min(cap, iterations-run) iterations, oldest first. Returns count. */
TRMF_API int32_t trmf_session_stats(TrmfSession *s, TrmfIterStats *out, int32_t cap);
/* Global objective J of the current factors, evaluated on device in fp64. */
TRMF_API double trmf_session_objective(TrmfSession *s);
/* Algorithmic bytes of ONE F-solve launch on this rank: nnz*(4+s+k*s) + (rows+1)*8 + rows*k*s
 * over the item rows this rank owns. */
TRMF_API double trmf_session_fsolve_bytes(TrmfSession *s);
/* One line of text: what the session runs -- with several ranks, which phases are sharded, the form of the X-solve chosen
 * by the measure-once rule (replicated / time-sharded through the communicator / time-sharded peer to peer) with the
 * slowest rank's measured X-phase time of every candidate, and whether the peer-to-peer transport is available (and why
 * not).  Writes at most cap bytes including the terminating NUL; returns the length of the full text. */
TRMF_API int32_t trmf_session_describe(TrmfSession *s, char *buf, int32_t cap);
TRMF_API void trmf_session_destroy(TrmfSession *s);

/* --- held-out evaluation (the paper's imputation protocol; no reference counterpart) -------------------------------------
 * The model W.H^T at a resident set of positions that were NOT trained on, scored on the device: predictions y^ = W[i].H[j]
 * in the element type (the products of one dot product are summed in an order of this library's choosing), and six fp64
 * sums over the set, each formed in a fixed order (repeated calls are bit-identical):
 *   count          entries                          count_nonzero  entries whose truth y != 0
 *   sq_err         sum (y^ - y)^2                   abs_err        sum |y^ - y|
 *   abs_truth      sum |y|                          rel_err        sum over y != 0 of |y^ - y| / |y|
 * The truths must be in the scale the model trains on: a session with an active series transform
 * (trmf_session_set_series_transform) refuses the evaluation.  With TRMF_DEVICES every rank holds the same factors and
 * rank 0 evaluates; with a communicator (trmf_dist_init*) every process evaluates its own copy. */
typedef struct {
    uint64_t count, count_nonzero;
    double sq_err, abs_err, abs_truth, rel_err;
} TrmfHeldoutSums;
/* Ytest: TRMF_SPARSE PyMatrix of THIS library's element type, the same number of columns as the session's Y and at most
 * trmf_session_rows() rows; its stored CSR entries (row_ptr, col_idx, val_t -- explicit zeros included) are the held-out
 * positions and truths.  Uploaded once and resident until replaced; it stays valid across append_rows (rows only grow).
 * NULL drops it.  0, or -1 with trmf_last_error() (wrong shape or type, an index out of range; the session is unchanged). */
TRMF_API int32_t trmf_session_set_heldout(TrmfSession *s, const PyMatrix *Ytest);
/* Blocking, ordered after every run() enqueued before; reads the factors only (the trajectory, the iteration statistics,
 * the mark and the measured decisions are untouched).  out: the sums above; pred: NULL or Ytest.nnz reals of the element
 * type, in Ytest's CSR order (row-major by timestamp).  0, or -1 (no held-out set, an active series transform, a device
 * failure) with the outputs untouched. */
TRMF_API int32_t trmf_session_eval_heldout(TrmfSession *s, TrmfHeldoutSums *out, void *pred);
/* Replace lambdaI / lambdaAR / lambdaLag of a live session (every rank) for the iterations enqueued from now on; blocks
 * until the work already enqueued has finished.  mark(); run(n); rewind(); set_lambdas(l'); run(n) gives the same bits as
 * a session created with l' from the marked model.  0, or -1 for a value that is not finite. */
TRMF_API int32_t trmf_session_set_lambdas(TrmfSession *s, double lambdaI, double lambdaAR, double lambdaLag);

/* --- sparse lag weights: which lags does the data use? -------------------------------------------------------------------
 * With lambdaLagL1 > 0 the lag weights of latent dimension t solve
 *     argmin  1/2 th^T G_t th - b_t^T th + 1/2 lambdaLag |th|^2 + lambdaLagL1 |th|_1
 * (G_t, b_t: the lagged inner products of W[:, t] that the ridge solve uses, without lambdaLag on the diagonal) by cyclic
 * coordinate descent in fp64, warm-started from the session's current lag weights; refit != 0 then replaces the weights on
 * the selected support S by the solution of (G_SS + lambdaLag I) th_S = b_S.  Weights off the support are exact +0.
 * Every rank; blocks until the work already enqueued has finished.  (0, 0) restores the ridge solve exactly.  0, or -1 with
 * trmf_last_error() for a lambdaLagL1 that is negative or not finite (the session is unchanged and stays usable). */
TRMF_API int32_t trmf_session_set_lag_penalty(TrmfSession *s, double lambdaLagL1, int32_t refit);
/* The lag-weight phase on its own: recompute the lag weights from the session's current W with the current penalties (ridge or
 * lasso), after every run() enqueued before; blocking.  The iteration counter, the statistics and the mark are untouched. */
TRMF_API int32_t trmf_session_solve_lags(TrmfSession *s);
/* Record of the last lag-weight solve.  per_dim: NULL, or k x 4 int32, row t = (sweeps used, non-zero weights, 1 if the sweep
 * cap was hit -- the iterate is kept --, 1 if the refit met a pivot that is not positive and finite -- the lasso's solution is
 * kept); capped / refit_skipped: NULL, or the number of dimensions with that flag.  All zero when the last solve was a ridge
 * solve (it keeps no record) or none has run. */
TRMF_API int32_t trmf_session_lag_stats(TrmfSession *s, int32_t *per_dim /* k x 4 */, int32_t *capped, int32_t *refit_skipped);

/* --- forecasting: the next timestamps of a resident model, forecast and scored on the device ----------------------------
 * The rolling evaluation of the paper (and of rolling_validate) forecasts a window from the current factors, scores it against
 * the truth, appends the window and trains on.  These calls do the forecast and the scoring where the factors live.
 *
 * Six fp64 sums per series, accumulated over every scored forecast since the last reset (e = forecast - truth y, formed in
 * fp64 from the two element-type values):
 *   abs_err sum|e|   sq_err sum e^2   abs_truth sum|y|   abs_dtruth sum|y_i - y_{i-1}| over consecutive scored rows (across
 *   calls too: the session keeps the last truth row; the very first scored row contributes nothing)
 *   rel_err sum over y != 0 of |e|/|y|   count_nonzero the number of y != 0                                               */
typedef struct {
    double abs_err, sq_err, abs_truth, abs_dtruth, rel_err, count_nonzero;
} TrmfSeriesSums;
/* Blocking, ordered after every run() enqueued before; reads W, H, the lag weights and the series-transform coefficients and
 * changes nothing a later run() can see (W is not extended; the iteration counter, the statistics, the mark and the measured
 * decisions are untouched).
 *   roll-out   Wnew[i][t] = sum_l W[i - lag_l][t] * lag_val(l, t) for i = rows .. rows + steps - 1: each product rounded to the
 *              element type, summed over the lags in ascending order -- the bits of the front end's Model.latent_forecast,
 *              for every rank 1..1024
 *   forecast   y = Wnew[i] . H[j] in the element type; clip != 0: y = max(y, threshold); with an active series transform
 *              y -> (y - b_j) / a_j (otherwise the forecast is in the training scale)
 *   truth      NULL, or a dense steps x n PyMatrix of THIS library's element type (a PyMatrix does not carry its element type:
 *              the caller answers for it), finite, in the scale of the value just produced: every series' sums grow by the
 *              steps rows in timestamp order, one thread per series, no atomics -- the same bits every time
 *   Ynew       NULL, or steps x n reals, row-major;  Wnew: NULL, or steps x k reals, row-major
 * 0, or -1 with trmf_last_error() (steps < 1, a truth that is not dense or not steps x n, a window beyond 32-bit device indices, a
 * device failure) with Ynew, Wnew, the sums and the session as they were.  With TRMF_DEVICES every rank holds the same factors
 * and rank 0 forecasts; with a communicator every process forecasts from its own copy. */
TRMF_API int32_t trmf_session_forecast(TrmfSession *s, int32_t steps, int32_t clip, double threshold, const PyMatrix *truth,
                                       void *Ynew, void *Wnew);
/* rows_scored: NULL, or the number of forecast rows scored since the last reset; per_series: NULL, or n records. */
TRMF_API int32_t trmf_session_forecast_scores(TrmfSession *s, uint64_t *rows_scored, TrmfSeriesSums *per_series);
/* Zero the sums, the row count and the kept truth row.  append_rows, rewind, set_lambdas and set_series_transform leave them. */
TRMF_API int32_t trmf_session_forecast_reset(TrmfSession *s);

/* --- online updates: assimilate new timestamps without retraining -------------------------------------------------------
 * What a deployed forecaster does most often: new observations arrive, the model absorbs them and forecasts again.  A forward
 * filter over the rows i = first_row .. rows - 1 of W, in ascending order, with H, the lag weights and every earlier row fixed
 * (later rows are ignored: they are re-solved in turn):
 *   Omega_i  the stored entries of row i of the training matrix (missing != 0); every series, an absent entry reading as 0
 *            (missing == 0, dense or sparse storage)
 *   A_i  = sum_{j in Omega_i} h_j h_j^T + (lambdaI + lambdaAR) I
 *   p_i[t] = sum_l lag_val(l, t) W[i - lag_l][t]      rows < i as already updated; each product rounded to the element type,
 *                                                     summed in ascending lag order (Model.latent_forecast)
 *   W[i] = A_i^-1 (sum_{j in Omega_i} y_ij h_j + lambdaAR p_i)      Cholesky in the element type, both substitutions
 * y is the value the session trains on (the transformed one under trmf_session_set_series_transform); the lambdas are the
 * session's current ones (trmf_session_set_lambdas), each cast to the element type before they are added.  A filter, not a
 * smoother: rows before first_row never see the new data.  Typical use: append_rows(Ynew); assimilate(rows - Tn); forecast(..).
 *
 * Blocking, ordered after every run() enqueued before; every rank computes the same rows on its own copy (no exchange) and ends
 * up with the same bits; repeated calls from the same state give the same bits.  The iteration counter, the statistics, the mark,
 * the forecast scores and the measured multi-rank decisions are untouched.
 *   out    NULL, or: rows re-solved; entries = sum |Omega_i|; sq_err_before / sq_err_after = sum over Omega of (y - w_i . h_j)^2
 *          over the range with W as it was / as it is now, in fp64 and a fixed order.  Right after append_rows, sq_err_before is
 *          the one-step-ahead forecast error of the block in the training scale.
 *   Wnew   NULL, or (rows - first_row) x k reals, row-major: the new rows
 * 0 (first_row == rows: nothing to do), or -1 with trmf_last_error() and W, the outputs and the session as they were:
 * first_row below the largest lag or above rows; a lag set that contains lag 0; rank k > 64 (online updates cover the
 * register-tiled ranks 1..64); an A_i with a pivot that is not positive and finite (possible only with lambdaI + lambdaAR == 0
 * and a rank-deficient row; the message names the first such row); a device failure. */
typedef struct {
    uint64_t rows, entries;
    double sq_err_before, sq_err_after;
} TrmfAssimilateSums;
TRMF_API int32_t trmf_session_assimilate(TrmfSession *s, int32_t first_row, TrmfAssimilateSums *out /* or NULL */,
                                         void *Wnew /* or NULL: (rows - first_row) x k, row-major */);

/* --- outlier-robust online updates: the forward filter with Huber weights -----------------------------------------------
 * trmf_session_assimilate trusts every incoming value: one spiked reading bends its row of W and travels through the AR prior
 * into every later row and forecast.  Here a cell whose residual lies beyond c scale_j of its series enters its row's system
 * with the weight c scale_j / |r| instead of 1 (iteratively reweighted least squares on Huber's loss), and the weights come back:
 * they are the anomaly signal.  Over the rows i = first_row .. rows - 1 in ascending order, with Omega_i, p_i, y and the lambdas as
 * for trmf_session_assimilate, lam = lambdaI + lambdaAR and t_j = c scale_j (c and scale_j cast to the element type first):
 *   w^0 = p_i;  for s = 1 .. sweeps:
 *       r_j = y_ij - w^{s-1} . h_j,   omega_j = t_j / |r_j| if |r_j| > t_j else 1                      (j in Omega_i)
 *       w^s = (sum_j omega_j h_j h_j^T + lam I)^-1 (sum_j omega_j y_ij h_j + lambdaAR p_i)            Cholesky in the element type
 *   W[i] = w^sweeps;   the weights reported are those of the last sweep (formed from w^{sweeps-1})
 * c = infinity is the plain filter (omega = 1 throughout).  A fixed number of sweeps, not a convergence test.  The values weighted
 * are the ones the session trains on (the transformed ones under trmf_session_set_series_transform); the resident sigma2 is in
 * that scale already.
 *
 * Blocking, ordered after every run() enqueued before; every rank computes the same rows on its own copy (no exchange) and ends
 * up with the same bits; repeated calls from the same state give the same bits.  The iteration counter, the statistics, the mark,
 * the forecast and interval scores, the noise tables and the measured multi-rank decisions are untouched.
 *   scale    n finite positive values, or NULL: the square roots of the resident sigma2 table (trmf_session_fit_noise / _set_noise)
 *   out      NULL, or: rows, entries, sq_err_before / sq_err_after as in TrmfAssimilateSums (unweighted); downweighted = the number
 *            of omega < 1; weight_sum = sum of omega in fp64 in a fixed order
 *   Wnew     NULL, or (rows - first_row) x k reals, row-major: the new rows
 *   weights  NULL, or one real per stored entry of the rows in the session's CSR order (missing != 0; a cell stored twice is two
 *            observations with a weight each), or (rows - first_row) x n reals, row-major (dense storage, missing == 0)
 * 0 (first_row == rows: nothing to do, zero sums), or -1 with trmf_last_error() and W, every output and the session as they were:
 * everything trmf_session_assimilate refuses (the message names the first row with a bad pivot); scale == NULL with no noise fitted
 * or set; a scale that is not finite and positive; c not positive or NaN; sweeps outside 1..64; sparse storage with missing == 0
 * (an absent entry there is an observation without a slot to report a weight in); a device failure. */
typedef struct {
    uint64_t rows, entries, downweighted;
    double weight_sum, sq_err_before, sq_err_after;
} TrmfRobustSums;
TRMF_API int32_t trmf_session_assimilate_robust(TrmfSession *s, int32_t first_row, double c, int32_t sweeps,
                                                const double *scale /* n, or NULL: sqrt of the resident sigma2 table */,
                                                TrmfRobustSums *out /* or NULL */, void *Wnew /* or NULL */, void *weights /* or NULL */);

/* --- online loading updates: refit H from new rows without retraining ----------------------------------------------------
 * The other half of the online updates above: those absorb new timestamps into rows of W with H fixed; these refit the series
 * loadings H from new rows in O(new data) with W fixed.  The F-solve of series j depends on the history only through
 *   S_j = sum_t om_t w_t w_t^T,   r_j = sum_t om_t y_tj w_t     t over Omega_j, the stored entries of column j (missing != 0;
 *                                                               a cell stored twice is two observations)
 *   h_j = (S_j + lambdaI I)^-1 r_j                              the system the training F-solve builds
 * With om_t = gamma^(rows - 1 - t), gamma in (0, 1], the sums decay and old data fades: recursive least squares with forgetting.
 * gamma == 1 gives what a full F-solve over the grown history gives for the current W.  On the full-observation forms (dense
 * storage; sparse storage with missing == 0, where an absent entry reads 0) S is shared: the sum over every row, and r_j sums
 * the stored entries.
 *
 * Resident state, absent until trmf_session_series_stats_init: per series the packed upper triangle of S_j (k (k + 1) / 2 reals in
 * the element type) and r_j (k reals) -- one shared S plus the r_j on the full-observation forms -- in two generations (a call
 * reads one and writes the other: n k (k + 1) / 2 reals twice), gamma, the number of rows absorbed, and for sparse storage the
 * number of stored entries of each column already absorbed (append_rows puts a block's entries behind the column's old ones,
 * whether or not the input is canonical, so the entries not yet absorbed are always the column's tail).
 *
 * trmf_session_series_stats_init(s, forget): builds the tables over all rows with W as it is and om_t = forget^(rows - 1 - t); one
 *   pass as heavy as an F-solve.  H is not changed.  gamma is fixed until the next init.
 * trmf_session_adapt_series(s, out, Hnew): with m = rows - absorbed rows,  S <- gamma^m S + sum_new gamma^(rows - 1 - t) w_t w_t^T
 *   and r likewise, the sums over the entries not yet absorbed in stored order with W as it is now; then every series'
 *   h_j = (S_j + lambdaI I)^-1 r_j by Cholesky in the element type and both substitutions.  lambdaI is the session's current one
 *   cast to the element type; the ridge is not decayed.  y is the value the session trains on (the transformed one under an
 *   active series transform).  H is replaced: forecast*, assimilate*, download, objective and the next run see the new one.  A
 *   series without a stored entry gets h_j = 0 when lambdaI > 0.  m == 0 is allowed (H refitted from the tables as they are,
 *   for example after trmf_session_set_lambdas).  Under trmf_session_assimilate_robust the cells still enter these sums
 *   UNWEIGHTED: the Huber weights are not part of the statistics (trmf_session_adapt_series_robust below is the weighted update).
 * trmf_session_series_stats_info: valid = 1 (usable), 0 (absent), -1 (stale); the rows absorbed; gamma.
 *
 * The tables go stale when a row they absorbed may have changed: trmf_session_run, trmf_session_rewind, trmf_session_assimilate /
 * _assimilate_robust with first_row below the absorbed rows, trmf_session_set_series_transform.  Stale tables are refused with a
 * message that says to initialise again.  append_rows, set_lambdas, fit_noise / set_noise and forecast* leave them valid.
 *
 * Blocking, ordered after every run() enqueued before; every rank computes every series on its own copy (no exchange) and ends
 * up with the same bits; repeated identical call sequences give the same bits (no floating-point atomics, fixed summation
 * orders).  adapt_series does not touch the iteration counter, the statistics, the mark, the forecast and interval scores, the
 * noise tables or the measured multi-rank decisions.
 *   out    NULL, or: series refitted; rows and entries absorbed by this call; sq_err_before / sq_err_after = sum over the absorbed
 *          entries of (y - w_t . h_j)^2 with H as it was / as it is now, in fp64 and a fixed order (trmf_session_assimilate's
 *          reading of an entry); max_abs_change = max |H_new - H_old|
 *   Hnew   NULL, or n x k reals, row-major: the new loadings
 * 0, or -1 with trmf_last_error() and H, the tables, the outputs and the session as they were: rank k > 64 (like the other online
 * features); forget outside (0, 1]; no tables, or stale ones; an S_j + lambdaI I with a pivot that is not positive and finite
 * (possible only with lambdaI == 0 and a series with fewer independent rows than k; the message names the smallest such series);
 * a device pool that cannot hold the tables; a device failure. */
typedef struct {
    uint64_t series, rows, entries;
    double sq_err_before, sq_err_after, max_abs_change;
} TrmfAdaptSums;
TRMF_API int32_t trmf_session_series_stats_init(TrmfSession *s, double forget);
TRMF_API int32_t trmf_session_adapt_series(TrmfSession *s, TrmfAdaptSums *out /* or NULL */, void *Hnew /* or NULL: n x k, row-major */);
TRMF_API int32_t trmf_session_series_stats_info(TrmfSession *s, int32_t *valid, int32_t *absorbed_rows, double *forget);

/* --- robust online loading updates: Huber-weighted refit of H ---------------------------------------------------------------
 * trmf_session_adapt_series with Huber weights on the entries it absorbs: the robust form of the loading update, as
 * trmf_session_assimilate_robust is of the filter.  Sparse storage with missing != 0 only (the form with per-series tables).  For
 * series j let (S_j, r_j) be the tables, m = rows - absorbed rows, d = gamma^m, om_t = gamma^(rows - 1 - t), E_j the stored entries
 * of column j not yet absorbed in stored order (a cell stored twice is two observations), tau_j = c scale_j, h^0 = H[j]:
 *   for s = 1 .. sweeps:   res_e = y_e - w_t . h^{s-1},   u_e = 1 if |res_e| <= tau_j else tau_j / |res_e|          (e in E_j)
 *                          S^s = d S_j + sum_e (u_e om_t) w_t w_t^T,   r^s = d r_j + sum_e (u_e om_t) y_e w_t
 *                          h^s = (S^s + lambdaI I)^-1 r^s                                  (Cholesky, as adapt_series)
 *   commit S^sweeps, r^sweeps, H[j] = h^sweeps; report the u_e of the last sweep
 * Every sweep restarts from the decayed OLD tables; only the new entries are reweighted: iteratively reweighted least squares on
 *   J_j(h) = h^T (d S_j + lambdaI I) h - 2 h . (d r_j) + sum_e om_t rho_tau(y_e - w_t . h),   rho_tau(x) = x^2 (|x| <= tau), 2 tau |x| - tau^2
 * so sum_j J_j never rises from one sweep to the next.  The committed tables and H keep h_j = (S_j + lambdaI I)^-1 r_j: a later
 * adapt_series or another robust call continues from them unchanged.  The weights are this call's own: residuals against the
 * loadings with W as it is now, not the filter's weights (per row, against the prior row).  A series with no new entry runs one
 * sweep (nothing to reweight).  c = +inf is adapt_series: the same operations in the same order, the same bits.
 *   c, sweeps, scale   as for trmf_session_assimilate_robust (c > 0, +inf allowed; sweeps in 1..64; n positive finite values, or
 *                      NULL for the square roots of the resident sigma2 table)
 *   out      NULL, or: the fields of TrmfAdaptSums (the squared errors unweighted); downweighted = entries with u_e < 1 and
 *            weight_sum = sum u_e, of the last sweep; objective_before / objective_after = sum_j J_j at h^0 / at h^sweeps, in fp64,
 *            summed in series order
 *   Hnew     NULL, or n x k reals, row-major
 *   wptr, wrows, weights   each NULL, or the weights series-major: n + 1 offsets; per new entry its timestamp (row number); the last
 *            sweep's u_e in the element type.  sum_j |E_j| = out->entries values.
 * Generations, staleness, blocking, sameness across ranks and calls, and what stays untouched are adapt_series'.  0, or -1 with
 * trmf_last_error() and H, the tables, the outputs and the session as they were: whatever adapt_series refuses; c not positive,
 * sweeps outside 1..64, a scale that is not finite and positive, no scale and no resident noise; the full-observation forms (dense
 * storage, sparse storage with missing == 0), which keep one shared S -- the message says so. */
typedef struct {
    uint64_t series, rows, entries, downweighted;
    double sq_err_before, sq_err_after, max_abs_change, weight_sum, objective_before, objective_after;
} TrmfRobustAdaptSums;
TRMF_API int32_t trmf_session_adapt_series_robust(TrmfSession *s, double c, int32_t sweeps, const double *scale /* n, or NULL */,
                                                  TrmfRobustAdaptSums *out /* or NULL */, void *Hnew /* or NULL */, uint64_t *wptr /* or NULL: n + 1 */,
                                                  uint32_t *wrows /* or NULL */, void *weights /* or NULL */);

/* --- fixed-interval smoother of the online rows: windowed preconditioned conjugate gradients -----------------------------
 * The filters above fit row i to its own observations and the AR prior of the rows BEFORE it; the AR penalties of the later rows
 * i + lag_l, in which w_i appears as well, are ignored, so the tail rows every forecast starts from are not the minimiser of the
 * model's own objective.  The smoother is: with f = first_row, m = rows - f, and W[0..f), H, the lag weights Theta, the lag set
 * and the session's current lambdaI, lambdaAR fixed, the rows f .. rows - 1 become the minimiser of the training objective
 * restricted to them,
 *   J_win = 1/2 sum_{i>=f} sum_{j in Omega_i} (y_ij - w_i . h_j)^2 + 1/2 lambdaI sum_{i>=f} |w_i|^2 + 1/2 lambdaAR sum_{i>=f} |e_i|^2
 *   e_i   = w_i - sum_l Theta(l, .) o w_{i - lag_l}                                   (rows < f enter e_i as constants)
 * with Omega_i and y exactly as for trmf_session_assimilate (missing or not, sparse or dense, the transformed value under an active
 * series transform).  It is what the X-solve would give for those rows if nothing else moved, at a cost of O(window).  The gradient
 *   g_i = (G_i + lambdaI I) w_i - b_i + lambdaAR (e_i - sum_{l : i + lag_l < rows} Theta(l, .) o e_{i + lag_l})
 * is linear in the rows: one SPD system of order m k.  m == 1 is the filter's row; with every lag >= m it is the filter on every
 * row; always J_win(smoothed) <= J_win(filtered).
 *
 * Order of operations: G_i, b_i by the X phase's builders; the Cholesky factors U_i of A_i = G_i + (lambdaI + lambdaAR) I for the
 * whole window (the filter's blocks: the block-Jacobi preconditioner); preconditioned conjugate gradients in the element type on
 * the correction to the rows as they stand: r = -g(W), z_i = U_i^-1 U_i^-T r_i, p = z, then per step q = A p (zero head rows),
 * alpha = (r.z) / (p.q), x += alpha p, r -= alpha q, z, beta = (r.z)_new / (r.z)_old, p = z + beta p.  The dot products are summed
 * per row in the element type and across rows in fp64, every sum in a fixed order.  The step stops when r.z <= rtol^2 (r.z)_0 or
 * after max_iter steps.  The first time the stop test holds, one step is spent on replacing the recursively updated residual by
 * the true one, r = b - A x from the rows as they then are (it counts in `iterations`), and the iteration goes on from p = z for
 * at least one more step before the test is taken again.  This removes the error a start far from the minimiser leaves in the
 * first residual; it is done once per call.  A call that reaches max_iter still commits (converged = 0): every CG iterate lowers J_win.
 *   rtol      <= 0: the default, 1e-5 in the float library (~ 84 eps), 2e-14 in the double library (~ 90 eps)
 *   max_iter  <= 0: the default, 500 (at most 16383)
 * The window may hold at most 1024 rows (the factors of all its rows stay resident for the solve: m k^2 reals).
 *
 * Blocking, ordered after every run() enqueued before; every rank computes the same rows on its own copy (no exchange) and ends
 * up with the same bits; repeated calls from the same state give the same bits (no floating-point atomics, fixed summation
 * orders).  The iteration counter, the statistics, the mark, the forecast and interval scores, the noise tables and the measured
 * multi-rank decisions are untouched.  The series statistics of trmf_session_adapt_series go stale when first_row lies below the
 * rows they absorbed (the rule of trmf_session_assimilate).
 *   out    NULL, or: rows, entries, sq_err_before / sq_err_after as in TrmfAssimilateSums; iterations = CG steps taken;
 *          converged = 1 when the stop test held, 0 when max_iter was reached; residual = sqrt((r.z) / (r.z)_0) at the end;
 *          objective_before / objective_after = J_win with the rows as they were / as they are, in fp64 and a fixed order
 *   Wnew   NULL, or (rows - first_row) x k reals, row-major: the new rows
 * 0 (first_row == rows: nothing to do, zero sums), or -1 with trmf_last_error() and W, the outputs and the session as they were:
 * everything trmf_session_assimilate refuses (the message names the first row whose A_i has a bad pivot); a window of more than
 * 1024 rows; an rtol that is not finite; max_iter above 16383; a device failure. */
typedef struct {
    uint64_t rows, entries;
    int32_t  iterations, converged;        /* converged = 0: max_iter reached */
    double   residual;                     /* sqrt((r.z) / (r.z)_0) at the end */
    double   sq_err_before, sq_err_after;  /* as TrmfAssimilateSums */
    double   objective_before, objective_after;   /* J_win, fp64, fixed order */
} TrmfSmoothSums;
TRMF_API int32_t trmf_session_smooth(TrmfSession *s, int32_t first_row, double rtol, int32_t max_iter,
                                     TrmfSmoothSums *out /* or NULL */, void *Wnew /* or NULL: (rows - first_row) x k */);

/* --- robust fixed-interval smoother: Huber-weighted windowed PCG ------------------------------------------------------------
 * trmf_session_smooth weights every cell fully, so one gross outlier among the new cells bends the tail rows; the robust filter
 * trmf_session_assimilate_robust is not the minimiser of the window's objective.  This call is both: with f = first_row,
 * thresholds t_j = c scale_j, and H, Theta, the lag set, the rows before f and the session's current lambdaI, lambdaAR fixed, and
 * Omega_i and y exactly as for trmf_session_assimilate,
 *   J_rob = sum_{i>=f} sum_{j in Omega_i} rho_{t_j}(y_ij - w_i . h_j) + 1/2 lambdaI sum_{i>=f} |w_i|^2 + 1/2 lambdaAR sum_{i>=f} |e_i|^2
 *   rho_t(r) = 1/2 r^2 if |r| <= t,  t |r| - 1/2 t^2 otherwise;       e_i as for trmf_session_smooth
 * is lowered by `sweeps` rounds of iteratively reweighted least squares:
 *   x^0 = the rows f .. as they stand;   for s = 1 .. sweeps:
 *       omega_ij = t_j / |r_ij| if |r_ij| > t_j else 1,   r_ij = y_ij - x^{s-1}_i . h_j        (in the element type)
 *       x^s = the system of trmf_session_smooth with G_i = sum_j omega_ij h_j h_j^T, b_i = sum_j omega_ij y_ij h_j, solved by its
 *             PCG started from x^{s-1}: the same preconditioner with blocks G_i + (lambdaI + lambdaAR) I from the weighted G_i, the
 *             same stop rule, rtol and max_iter (and their defaults), one residual replacement per sweep
 *   W[f ..] = x^sweeps;   the weights reported are those of the last sweep (formed from x^{sweeps-1})
 * The number of sweeps is fixed.  Each sweep is a majorise-minimise step and every CG iterate lowers the sweep's majoriser, so
 * J_rob(after) <= J_rob(before) also when a sweep stops at max_iter; such a call still commits, with converged = 0.  c = infinity
 * minimises J_win of trmf_session_smooth, to rounding and not to the bit (the weighted Grams are summed in another order than the
 * X phase's).  On dense storage every row gets its own weighted Gram.
 *
 * The entries of a row are summed in items of 256 entries (at most 8 items per row: longer rows get longer items), the items of a
 * row in ascending order.  Blocking, ordered after every run() enqueued before; every rank computes the same rows on its own copy
 * and ends up with the same bits; repeated calls from the same state give the same bits (no floating-point atomics, fixed
 * summation orders).  Neither the Gram cache of the X phase nor anything trmf_session_smooth leaves untouched is touched; the
 * series statistics go stale by the rule of trmf_session_smooth; the recovery snapshot follows the new W.
 *   scale    NULL (the square root of the resident sigma2 table), or n positive finite values
 *   out      NULL, or: rows, entries; downweighted = cells with omega < 1 and weight_sum = sum of omega in the last sweep;
 *            sweeps; iterations = CG steps over all sweeps; converged = 1 only if every sweep's stop test held; residual = that of
 *            the last sweep; sq_err_before / sq_err_after unweighted, as in TrmfSmoothSums; objective_before / objective_after =
 *            J_rob with the rows as they were / as they are, in fp64 and a fixed order
 *   Wnew     NULL, or (rows - first_row) x k reals, row-major: the new rows
 *   weights  NULL, or the layout of trmf_session_assimilate_robust: one per stored entry of rows first_row .. in CSR order (sparse
 *            storage, missing != 0), or (rows - first_row) x n row-major (dense storage)
 * 0 (first_row == rows: nothing to do, zero sums), or -1 with trmf_last_error() and W, the outputs and the session as they were:
 * everything trmf_session_smooth refuses (the window cap of 1024 rows included) and everything trmf_session_assimilate_robust
 * refuses (c not positive, sweeps outside 1..64, a scale that is not positive and finite, no scale and no noise table, sparse
 * storage with missing == 0). */
typedef struct {
    uint64_t rows, entries, downweighted;
    int32_t  sweeps, iterations, converged, reserved;
    double   residual, weight_sum;
    double   sq_err_before, sq_err_after;          /* unweighted */
    double   objective_before, objective_after;    /* J_rob, fp64, fixed order */
} TrmfRobustSmoothSums;
TRMF_API int32_t trmf_session_smooth_robust(TrmfSession *s, int32_t first_row, double c, int32_t sweeps,
                                            const double *scale /* n, or NULL */, double rtol, int32_t max_iter,
                                            TrmfRobustSmoothSums *out /* or NULL */, void *Wnew /* or NULL */, void *weights /* or NULL */);

/* --- forecast uncertainty: noise fit, predictive standard deviation and interval scores ---------------------------------
 * TRMF read as a linear-Gaussian state-space model (the paper's own reading): y_ij = w_i . h_j + eps_ij with eps_ij ~ N(0, sigma_j^2),
 * every latent dimension t an AR process with innovation variance q_t.  With m the largest lag and T = trmf_session_rows():
 *   sigma_j^2 = (1/|Omega_j|) sum_{i in Omega_j} (y_ij - w_i . h_j)^2   over the stored entries of series j (missing != 0), or over
 *               every timestamp with an absent entry reading as 0 (missing == 0, |Omega_j| = T); y is the value the session trains
 *               on; products, dot product, difference, square and sum in fp64 from the stored element-type values.  A series
 *               without a stored entry takes the pooled value sum_j sq_j / sum_j cnt_j (both summed in series order)
 *   q_t       = (1/(T - m)) sum_{i >= m} (w_i[t] - p_i[t])^2,  p_i the one-step latent forecast formed as the roll-out forms it
 *               (products rounded to the element type, ascending lag order); difference, square and sum in fp64
 *   psi_t[0] = 1, psi_t[s] = sum_{l: lag_l <= s} lag_val(l, t) psi_t[s - lag_l]  (fp64);   v_t[s] = q_t sum_{u <= s} psi_t[u]^2
 *   V[s][j]  = sigma_j^2 + sum_t H[j][t]^2 v_t[s]     the predictive variance of the forecast of series j, s + 1 steps ahead
 *   sd[s][j] = sqrt(V[s][j]) (/ |a_j| under an active series transform y -> a_j y + b_j), rounded once to the element type
 * A PLUG-IN interval: it ignores the estimation error of H, of the lag weights and of the last rows of W, and the residuals are
 * in-sample ones, so it is too narrow where the model overfits.  trmf_session_set_noise is the hook for a caller who has
 * out-of-sample variances (for example TrmfSeriesSums.sq_err of earlier windows).  Every sum is formed in a fixed order without
 * atomics: repeated calls, and every rank, give the same bits.
 *
 * None of these calls touches the point-score table and its kept truth row, the trajectory and the iteration counter, the
 * statistics, the mark or the measured multi-rank decisions. */
typedef struct {
    double pooled_sigma2;                  /* sum_j sq_j / sum_j cnt_j                                     */
    double sigma2_min, sigma2_max;         /* over the series, those that took the pooled value included  */
    uint64_t series_pooled;                /* series without a stored entry                                */
    double q_min, q_max;
} TrmfNoiseStats;
/* Fit sigma_j^2 (n doubles) and q_t (k doubles) on the current factors into resident tables.  Blocking, ordered after every
 * run() enqueued before; every rank computes on its own copy (no exchange).  Later run / assimilate / append_rows / rewind calls
 * neither refit nor invalidate the tables: the caller decides when to refit.  out may be NULL.  0, or -1 with
 * trmf_last_error() (rows <= the largest lag, a training matrix without a stored entry, a device failure) with the tables as
 * they were. */
TRMF_API int32_t trmf_session_fit_noise(TrmfSession *s, TrmfNoiseStats *out /* or NULL */);
/* Read (either pointer may be NULL) / replace the resident tables.  -1 when none has been fitted or set (noise), or for a
 * value that is negative or not finite (set_noise; the tables stay as they were). */
TRMF_API int32_t trmf_session_noise(TrmfSession *s, double *sigma2 /* n */, double *q /* k */);
TRMF_API int32_t trmf_session_set_noise(TrmfSession *s, const double *sigma2 /* n */, const double *q /* k */);
/* Seven fp64 sums per series over the scored cells (e = truth - mean, z = e / sd, both from the two element-type values the call
 * stores): cells; covered = the number with |e| <= zq sd; sd_sum; abs_truth = sum |truth|; z2_sum; nll_sum = sum of
 * log(2 pi sd^2)/2 + z^2/2; crps_sum = sum of sd (z (2 Phi(z) - 1) + 2 phi(z) - 1/sqrt(pi)), Phi through the fp64 erf.  A series'
 * cells are added in timestamp order by one thread. */
typedef struct {
    double cells, covered, sd_sum, abs_truth, z2_sum, nll_sum, crps_sum;
} TrmfIntervalSums;
/* trmf_session_forecast plus the predictive standard deviation: the same arguments, zq > 0 (the normal quantile of the interval
 * scored into `covered`) and Ysd (NULL, or steps x n reals, row-major, in the units of Ynew).  Ynew and Wnew are bit for bit what
 * trmf_session_forecast returns.  With a truth the interval table grows (not the point-score table).  0, or -1 with
 * trmf_last_error() -- before any device work: no noise fitted or set, zq not positive and finite, and every reason
 * trmf_session_forecast refuses; after it: lag weights explosive over this horizon (a v_t[s] that is not finite), a device
 * failure -- with Ynew, Ysd, Wnew and the table as they were.  With TRMF_DEVICES rank 0 forecasts. */
TRMF_API int32_t trmf_session_forecast_dist(TrmfSession *s, int32_t steps, int32_t clip, double threshold, double zq,
                                            const PyMatrix *truth, void *Ynew, void *Ysd, void *Wnew);
/* rows_scored: NULL, or the forecast rows scored by forecast_dist since the last reset; per_series: NULL, or n records. */
TRMF_API int32_t trmf_session_interval_scores(TrmfSession *s, uint64_t *rows_scored, TrmfIntervalSums *per_series);
TRMF_API int32_t trmf_session_interval_reset(TrmfSession *s);

/* --- multi-GPU (one process per GPU; RCCL all-gathers over xGMI) ---------------------------- */
#define TRMF_UNIQUE_ID_BYTES 128
/* Rank 0: create an RCCL unique id; the caller broadcasts the bytes to all ranks
 * (e.g. with torch.distributed) and every rank passes them to trmf_dist_init. */
TRMF_API int32_t trmf_dist_get_unique_id(void *out_id /* TRMF_UNIQUE_ID_BYTES */);
/* world <= 64 (slots of the staged all-gather); larger worlds are refused here. */
TRMF_API int32_t trmf_dist_init(int32_t rank, int32_t world, const void *id /* TRMF_UNIQUE_ID_BYTES */);
/* Host-staged communicator for tests and RCCL-less setups: `allgatherv` must gather, in place,
 * the byte ranges [offsets[r], offsets[r+1]) of `buf` owned by each rank r. Returns 0 on success. */
typedef int32_t (*trmf_allgatherv_fn)(void *buf, const uint64_t *offsets, int32_t world,
                                      void *ctx);
TRMF_API int32_t trmf_dist_init_callback(int32_t rank, int32_t world, trmf_allgatherv_fn allgatherv,
                                void *ctx);
/* Measurement aid: act as rank `rank` of `world` WITHOUT peers (every gather is skipped).  A session created under it
 * runs exactly the kernels that rank would run, alone on the GPU -- its times are that rank's compute share; the factors
 * are NOT a solution (the other ranks' blocks stay stale).  Used by scripts/shard_compute_times.py. */
TRMF_API int32_t trmf_dist_init_solo(int32_t rank, int32_t world);
TRMF_API int32_t trmf_dist_rank(void);
TRMF_API int32_t trmf_dist_world(void);
TRMF_API void trmf_dist_finalize(void);
/* Contiguous row partition balanced by nnz: bounds[0]=0 <= ... <= bounds[world]=nrows. */
TRMF_API int32_t trmf_partition_by_nnz(uint64_t nrows, const size_t *ptr, int32_t world,
                              uint64_t *bounds /* world+1 */);

#ifdef __cplusplus
}
#endif
#endif /* TRMF_ABI_H */
