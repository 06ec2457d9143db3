// trmf_abi.hip -- extern "C" entry points of trmf_float{32,64}.so (see include/trmf_abi.h).
//
// Section 1: c_trmf_train, the reference's own boundary (trmf.h:203-210, trmf.cpp:696-725).
// Section 2: build-owned session / device / multi-GPU entry points.
//
// There is deliberately no host implementation of the solver behind these symbols: if the HIP
// runtime reports no usable device the calls fail loudly.
#include "../../include/trmf_abi.h"

#include <memory>
#include <mutex>
#include <random>

#include "session_group.hpp"

namespace trmf {

static std::string g_last_error = "";
static std::mutex g_err_mu;
static thread_local std::string tl_last_error;     // the calling thread's own last error (a rank thread's cause, not a peer's echo)
void set_error(const std::string &msg) {
    tl_last_error = msg;
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_last_error = msg;
}

static int g_device = 0;
static std::mutex g_prof_mu;
static TrmfTrainProfile g_last_profile;
static bool g_have_profile = false;
static std::shared_ptr<Comm> g_self = std::make_shared<SelfComm>();
static std::shared_ptr<Comm> g_comm;
// A session shares ownership of the communicator it was created under, so trmf_dist_finalize() before
// trmf_session_destroy() leaves the session's communicator alive until the session goes away.
// (a worker thread of an in-process session group has its own communicator and device: session_group.hpp)
std::shared_ptr<Comm> active_comm() { return tl_comm() ? tl_comm() : g_comm ? g_comm : g_self; }
// (per thread: a peer woken by the broken barrier sets "another rank ... failed" at once, and would replace the failing rank's text)
std::string SessionGroup::trmf_last_error_text() { return tl_last_error; }

static bool bind_device() {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) {
        set_error("no HIP device visible (the MI355X TRMF solver has no CPU fallback)");
        return false;
    }
    if (hipSetDevice(tl_device() >= 0 ? tl_device() : g_device) != hipSuccess) {
        set_error("hipSetDevice failed");
        return false;
    }
    return true;
}
// Every entry point that touches the device selects the library's device (trmf_set_device) for its duration and
// puts the caller's current device back on return.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    DeviceGuard() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = bind_device();
    }
    ~DeviceGuard() { if (prev >= 0 && prev != g_device) (void)hipSetDevice(prev); }
};

// check_dimension, trmf.cpp:561-596 (same messages, same order)
static bool check_dimension(const PyMatrix *Y, const PyMatrix *W, const PyMatrix *H, const PyMatrix *LV,
                            uint32_t lag_size) {
    bool pass = true;
    if (Y->rows != W->rows) { fprintf(stderr, "[ERR MSG]: Y.rows (%ld) != W.rows (%ld)\n", (long)Y->rows, (long)W->rows); pass = false; }
    if (Y->cols != H->rows) { fprintf(stderr, "[ERR MSG]: Y.cols (%ld) != H.rows (%ld)\n", (long)Y->cols, (long)H->rows); pass = false; }
    if (W->cols != H->cols) { fprintf(stderr, "[ERR MSG]: W.cols (%ld) != H.cols (%ld)\n", (long)W->cols, (long)H->cols); pass = false; }
    if (lag_size != LV->rows) { fprintf(stderr, "[ERR MSG]: lag_set.size(%ld) != lag_val.rows(%ld)\n", (long)lag_size, (long)LV->rows); pass = false; }
    if (W->cols != LV->cols) { fprintf(stderr, "[ERR MSG]: W.cols(%ld) != lag_val.cols(%ld)\n", (long)W->cols, (long)LV->cols); pass = false; }
    if (W->type != TRMF_DENSE_ROWMAJOR) { fprintf(stderr, "[ERR MSG]: W should be rowmajored\n"); pass = false; }
    if (H->type != TRMF_DENSE_ROWMAJOR) { fprintf(stderr, "[ERR MSG]: H should be rowmajored\n"); pass = false; }
    if (LV->type != TRMF_DENSE_COLMAJOR) { fprintf(stderr, "[ERR MSG]: lag_val should be colmajored\n"); pass = false; }
    return pass;
}

// Limits of the device path (documented in DESIGN.md); violations are reported, never worked around.
static bool check_device_limits(const PyMatrix *Y, const PyMatrix *W, uint32_t lag_size, int missing) {
    bool pass = true;
    // the reference asserts (aborts) on a dense Y with missing != 0 (rf_matrix.h:180); here: diagnostic
    if (missing && Y->type != TRMF_SPARSE) { fprintf(stderr, "[ERR MSG]: missing!=0 requires a sparse Y\n"); pass = false; }
    if (Y->type != TRMF_SPARSE && Y->type != TRMF_DENSE_ROWMAJOR && Y->type != TRMF_DENSE_COLMAJOR) { fprintf(stderr, "[ERR MSG]: unsupported Y matrix type %d\n", (int)Y->type); pass = false; }
    // register-tiled kernels up to rank 64, generic kernels (csrc/generic_kernels.hpp) up to 1024, on both training paths
    if (W->cols < 1 || W->cols > (uint64_t)kMaxRankGeneric) { fprintf(stderr, "[ERR MSG]: rank k=%ld outside the supported range 1..%d\n", (long)W->cols, kMaxRankGeneric); pass = false; }
    if (lag_size > (uint32_t)kMaxLags) { fprintf(stderr, "[ERR MSG]: |lag_set|=%u exceeds the supported %d\n", lag_size, kMaxLags); pass = false; }
    if ((Y->type == TRMF_SPARSE && Y->nnz >= (1ull << 32)) || Y->rows >= (1ull << 31) || Y->cols >= (1ull << 31)) { fprintf(stderr, "[ERR MSG]: problem exceeds 32-bit device indices\n"); pass = false; }
    // gathered factor rows are addressed with 32-bit byte offsets (gram_ring): tables up to 4 GiB
    const uint64_t rowbytes = (uint64_t)padded_rank((int)W->cols) * sizeof(real);
    if ((Y->rows + 1) * rowbytes > 0xffffffffull || (Y->cols + 1) * rowbytes > 0xffffffffull ||
        Y->rows + 1 >= (1ull << 24) || Y->cols + 1 >= (1ull << 24)) {
        fprintf(stderr, "[ERR MSG]: factor tables exceed the 4 GiB / 2^24 rows of 32-bit gather offsets\n"); pass = false;
    }
    return pass;
}

// The reference's dimension check plus this build's own limits (include/trmf_abi.h lists them); diagnostics on stderr.
static bool validate_problem(const PyMatrix *Y, const uint32_t *lag_set, uint32_t lag_size, const PyMatrix *W,
                             const PyMatrix *H, const PyMatrix *LV, int32_t missing) {
    if (!check_dimension(Y, W, H, LV, lag_size)) { set_error("dimension check failed"); return false; }
    if (!check_device_limits(Y, W, lag_size, missing)) { set_error("unsupported problem"); return false; }
    for (uint32_t l = 1; l < lag_size; l++)
        if (lag_set[l] < lag_set[l - 1]) { fprintf(stderr, "[ERR MSG]: lag_set must be ascending\n"); set_error("lag_set not ascending"); return false; }
    if (lag_size && lag_set[lag_size - 1] >= Y->rows) { fprintf(stderr, "[ERR MSG]: max lag >= number of timestamps\n"); set_error("lag too large"); return false; }
    return true;
}

// one session on the calling thread's device under the calling thread's communicator (the problem has been validated)
static TrmfSessionImpl *build_session(const PyMatrix *Y, const uint32_t *lag_set, uint32_t lag_size,
                                      const PyMatrix *W, const PyMatrix *H, const PyMatrix *LV,
                                      double lambdaI, double lambdaAR, double lambdaLag, int32_t period_W,
                                      int32_t period_H, int32_t period_Lag, int32_t missing, int32_t verbose) {
    if (!bind_device()) return nullptr;
    std::unique_ptr<TrmfSessionImpl> s(new TrmfSessionImpl());
    s->lambdaI = lambdaI; s->lambdaAR = lambdaAR; s->lambdaLag = lambdaLag;
    s->period_W = period_W; s->period_H = period_H; s->period_Lag = period_Lag; s->verbose = verbose;
    s->full = (missing == 0);
    if (s->create(Y, lag_set, lag_size, W, H, LV)) {
        const std::string why = SessionGroup::trmf_last_error_text();
        active_comm()->abort();          // before the half-built session is torn down (its teardown passes the group's barrier)
        set_error(why);
        return nullptr;
    }
    return s.release();
}

// What a TrmfSession* points to: ONE session on the library's device -- or, under TRMF_DEVICES / TRMF_GPUS (session_group.hpp), one
// session per listed device, each on a worker thread of this process, joined by an in-process communicator.
struct SessionHandle {
    TrmfSessionImpl *single = nullptr;
    SessionGroup *group = nullptr;
    TrmfSessionImpl *first() const { return group ? group->impl[0] : single; }
    // f on every rank's session (one rank: on the calling thread)
    int all(const std::function<int(TrmfSessionImpl *)> &f) const {
        return group ? group->on_all([&](int r) { return f(group->impl[r]); }) : f(single);
    }
    int rank0(const std::function<int(TrmfSessionImpl *)> &f) const {
        return group ? group->on_rank0([&](int) { return f(group->impl[0]); }) : f(single);
    }
    // call(session, slot, &result[slot]) on every rank's session, one result per rank of a group (one otherwise); slot 0 is the
    // session whose outputs go to the caller.  Every rank computes the same bits, so a condition that every rank finds alike (a bad
    // pivot) is read from the results on the calling thread, not raised by a failing worker task.  Empty: a task failed.
    template <class R, class F>
    std::vector<R> per_rank(F &&call) const {
        std::vector<R> res(group ? (size_t)group->world() : 1);
        if (all([&](TrmfSessionImpl *t) { const int slot = group ? t->comm->rank : 0; return call(t, slot, &res[slot]); })) res.clear();
        return res;
    }
    ~SessionHandle() {
        if (group) SessionGroup::release(group);      // the sessions go; threads + communicators wait for the next call (session_group.hpp)
        else if (single) { (void)single->sync(false); delete single; }
    }
};

static SessionHandle *make_session(const PyMatrix *Y, const uint32_t *lag_set, uint32_t lag_size,
                                   const PyMatrix *W, const PyMatrix *H, const PyMatrix *LV,
                                   double lambdaI, double lambdaAR, double lambdaLag, int32_t period_W,
                                   int32_t period_H, int32_t period_Lag, int32_t missing, int32_t verbose) {
    if (!validate_problem(Y, lag_set, lag_size, W, H, LV, missing)) return nullptr;
    if (!bind_device()) { fprintf(stderr, "[ERR MSG]: %s\n", trmf_last_error()); return nullptr; }
    std::unique_ptr<SessionHandle> h(new SessionHandle());
    std::string why;
    const std::vector<int> devs = (g_comm || tl_comm()) ? std::vector<int>() : inproc_devices(&why);
    if (!why.empty()) { set_error(why); fprintf(stderr, "[ERR MSG]: %s\n", why.c_str()); return nullptr; }
    if (devs.empty()) {
        h->single = build_session(Y, lag_set, lag_size, W, H, LV, lambdaI, lambdaAR, lambdaLag, period_W, period_H, period_Lag, missing, verbose);
        if (!h->single) { fprintf(stderr, "[ERR MSG]: %s\n", trmf_last_error()); return nullptr; }
        return h.release();
    }
    h->group = SessionGroup::acquire(devs);
    if (!h->group) { fprintf(stderr, "[ERR MSG]: %s\n", trmf_last_error()); return nullptr; }
    int rc = 0;
    if (rc == 0)
        rc = h->group->on_all([&](int r) {          // every rank uploads the whole problem to its device and builds its session
            h->group->impl[r] = build_session(Y, lag_set, lag_size, W, H, LV, lambdaI, lambdaAR, lambdaLag, period_W, period_H, period_Lag, missing,
                                              r == 0 ? verbose : 0);        // the reference's log lines once
            return h->group->impl[r] ? 0 : kFail;
        });
    if (rc) { fprintf(stderr, "[ERR MSG]: %s\n", trmf_last_error()); return nullptr; }    // (~SessionHandle tears the group down)
    if (verbose) fprintf(stderr, ">> %d ranks as threads of this process on devices TRMF_DEVICES; communicator: %s\n", h->group->world(), h->group->comm_kind.c_str());
    return h.release();
}

// ---- the checks of the online entry points ------------------------------------------------------------------------------------
// Each returns true, with the error set, when the call is refused.  All of them run on the calling thread, before DeviceGuard and
// before any rank's worker (a rejected call must not break the barrier of a TRMF_DEVICES group); `what` is the call's name as its
// messages spell it, and what differs between the calls' messages is passed in.
static bool refused(const std::string &why) { set_error(why); return true; }
static bool rank_refusal(const TrmfSessionImpl *f, const std::string &what) {
    return f->k > kMaxRank && refused(what + ": online updates cover the register-tiled ranks 1..64, this session has rank " + std::to_string(f->k));
}
static bool online_refusal(const TrmfSessionImpl *f, const std::string &what) {
    return rank_refusal(f, what) || (f->has_lag0 && refused(what + ": the lag set contains lag 0 (a row would be its own prior)"));
}
// the calls that report a weight per stored entry
static bool weight_slot_refusal(const TrmfSessionImpl *f, const std::string &what) {
    return f->full && !f->dense && refused(what + ": sparse storage with missing == 0 is not covered (an absent entry there is an observation without a slot "
                                                  "to report its weight in); store the matrix dense");
}
static bool first_row_refusal(const TrmfSessionImpl *f, const std::string &what, int32_t first_row) {
    return (first_row < f->midx || first_row > f->T) &&
           refused(what + ": first_row " + std::to_string(first_row) + " outside [" + std::to_string(f->midx) + " (the largest lag), " + std::to_string(f->T) + " (rows)]");
}
// The smoothers' window: its cap, and the PCG's stop with the defaults put in (the robust smoother checks c and sweeps between the two).
static bool window_refusal(const TrmfSessionImpl *f, const std::string &what, int32_t first_row) {
    const int cap = TrmfSessionImpl::smooth_max_rows();
    return f->T - first_row > cap && refused(what + ": a window of " + std::to_string(f->T - first_row) + " rows is above the cap of " + std::to_string(cap) +
                                             " rows (the factors of every window row stay resident for the solve)");
}
static bool window_refusal(const std::string &what, double &rtol, int32_t &max_iter) {
    if (!std::isfinite(rtol)) return refused(what + ": rtol must be finite (<= 0: the default of the element type)");
    if (max_iter > kSmoothMaxIter) return refused(what + ": max_iter " + std::to_string(max_iter) + " above " + std::to_string(kSmoothMaxIter));
    if (rtol <= 0) rtol = kSmoothDefaultRtol;
    if (max_iter <= 0) max_iter = kSmoothDefaultMaxIter;
    return false;
}
// plain: what c == infinity amounts to, in the call's own words
static bool huber_refusal(const std::string &what, double c, int32_t sweeps, int max_sweeps, const char *plain) {
    if (!(c > 0)) return refused(what + ": c must be positive (infinity: " + plain + ")");
    return (sweeps < 1 || sweeps > max_sweeps) && refused(what + ": sweeps " + std::to_string(sweeps) + " outside 1.." + std::to_string(max_sweeps));
}
static bool scale_refusal(const TrmfSessionImpl *f, const std::string &what, const double *scale) {
    return !scale && !f->nz_set && refused(what + ": no scale given and no noise fitted or set (trmf_session_fit_noise / _set_noise)");
}
static bool stats_refusal(const TrmfSessionImpl *f, const std::string &what) {
    if (!f->ad_exists) return refused(what + ": no series statistics (trmf_session_series_stats_init first)");
    return !f->ad_valid && refused(what + ": the series statistics are stale: rows they absorbed may have changed (run, rewind, assimilate below the absorbed "
                                          "rows, or a new series transform); initialise them again (trmf_session_series_stats_init)");
}
// The n scales every rank receives as the same host values: the caller's, or the square roots of the resident noise (read from rank
// 0's device, hence after DeviceGuard); each must be finite and positive.
static bool resolve_scales(const SessionHandle *s, const TrmfSessionImpl *f, const std::string &what, const double *scale, std::vector<double> &sc) {
    sc.resize((size_t)f->n);
    if (scale) std::copy(scale, scale + f->n, sc.begin());
    else {
        if (s->rank0([&](TrmfSessionImpl *t) { return t->noise(sc.data(), nullptr); })) return true;
        for (double &v : sc) v = std::sqrt(v);
    }
    for (int j = 0; j < f->n; j++)
        if (!(std::isfinite(sc[j]) && sc[j] > 0))
            return refused(what + ": the scale of series " + std::to_string(j) + " is not finite and positive" + (scale ? "" : " (the square root of the resident sigma2)"));
    return false;
}
// A bad pivot of a row's system, found by every rank alike.  gram: "G", or "the weighted G" of the robust calls.
template <class R>
static bool pivot_refusal(const std::string &what, const std::vector<R> &res, const char *gram) {
    for (const R &r : res)
        if (r.bad_row >= 0)
            return refused(what + ": row " + std::to_string(r.bad_row) + ": a pivot of " + gram + " + (lambdaI + lambdaAR) I is not positive and finite "
                           "(lambdaI + lambdaAR == 0 and a rank-deficient row?); nothing was changed");
    return false;
}

}  // namespace trmf

using namespace trmf;

extern "C" {

struct TrmfSession { SessionHandle h; };        // opaque to callers; never instantiated as such

// ------------------------------------------------------------------------------------------------
// Section 1
// ------------------------------------------------------------------------------------------------
void c_trmf_train(const PyMatrix *pyY, uint32_t *py_lag_set, uint32_t py_lag_size, PyMatrix *pyW,
                  PyMatrix *pyH, PyMatrix *pylag_val, int warm_start, double lambdaI, double lambdaAR,
                  double lambdaLag, int32_t max_iter, int32_t period_W, int32_t period_H,
                  int32_t period_Lag, int32_t threads, int32_t missing, int32_t verbose) {
    if (verbose > 0) {   // parameter dump, trmf.cpp:607-629 (after the fold of :603-606)
        fprintf(stdout, ">> param.solver_type %d\n", missing ? 31 : 30);
        fprintf(stdout, ">> param.max_iter %d\n", max_iter);
        fprintf(stdout, ">> param.lambdaI %g\n", lambdaI);
        fprintf(stdout, ">> param.lambdaAR %g\n", lambdaAR);
        fprintf(stdout, ">> param.lambdaLag %g\n", lambdaLag);
        fprintf(stdout, ">> param.period_W %d\n", period_W);
        fprintf(stdout, ">> param.period_H %d\n", period_H);
        fprintf(stdout, ">> param.period_Lag %d\n", period_Lag);
        fprintf(stdout, ">> param.threads %d\n", threads);
        fprintf(stdout, ">> param.verbose %d\n", verbose);
        fprintf(stdout, ">> param.eps %g\n", 0.1);
        fprintf(stdout, ">> param.eps_cg %g\n", 0.1);
        fprintf(stdout, ">> param.max_tron_iter %d\n", 1);
        fprintf(stdout, ">> param.max_cg_iter %d\n", 20);
        fprintf(stdout, ">> prob.lag_size %ld:  ", (long)py_lag_size);
        for (uint32_t i = 0; i < py_lag_size; i++) fprintf(stdout, " %d", (int)py_lag_set[i]);
        fprintf(stdout, "\n");
        fflush(stdout);
    }
    // Quirk Q1: with warm_start == 0 the reference rebuilds W, H and lag_val as PRIVATE random matrices of
    // matching shapes before its dimension check (trmf_initialization, trmf.cpp:547-558, 719-722: rng_t = std::mt19937 seeded 0,
    // a fresh uniform_real_distribution<double>(0,1) / normal_distribution<double>(0,1) per element, cast to val_type,
    // rf_matrix.h:56-68, 740-753), trains those -- its ">> iter" lines under verbose describe that run -- and discards them:
    // the caller's arrays come back unchanged and no "[ERR MSG]" about the caller's shapes can appear.  Same here: the same
    // generator calls in the same order produce the same starting point (libstdc++ on both sides), the training runs on the
    // device on private copies, and nothing is written back.
    std::vector<real> cold_W, cold_H, cold_LV;
    PyMatrix privW, privH, privLV;
    if (!warm_start) {
        const size_t m = pyY->rows, n = pyY->cols, k = pyW->cols;
        std::mt19937 rng(0);
        cold_W.resize(m * k); cold_H.resize(n * k); cold_LV.resize((size_t)py_lag_size * k);
        for (real &x : cold_W) x = (real)std::uniform_real_distribution<double>(0.0, 1.0)(rng);
        for (real &x : cold_H) x = (real)std::uniform_real_distribution<double>(0.0, 1.0)(rng);
        for (real &x : cold_LV) x = (real)std::normal_distribution<double>(0.0, 1.0)(rng);
        auto view = [](std::vector<real> &buf, size_t rows, size_t cols, int32_t type) {
            PyMatrix v{};
            v.rows = rows; v.cols = cols; v.nnz = rows * cols; v.val = buf.data(); v.type = type;
            return v;
        };
        privW = view(cold_W, m, k, TRMF_DENSE_ROWMAJOR);
        privH = view(cold_H, n, k, TRMF_DENSE_ROWMAJOR);
        privLV = view(cold_LV, py_lag_size, k, TRMF_DENSE_COLMAJOR);
        pyW = &privW; pyH = &privH; pylag_val = &privLV;       // from here on the call works on the private model
    }
    DeviceGuard guard;                               // device of this library for the call, the caller's afterwards
    // where the call's wall time goes (trmf_last_train_profile): set-up / compute / download / teardown
    const double t0 = TrmfSessionImpl::now_s();
    TrmfTrainProfile prof{};
    const DevicePool::Stats ps0 = guard.ok ? DevicePool::current().stats() : DevicePool::Stats{};
    SessionHandle *s = make_session(pyY, py_lag_set, py_lag_size, pyW, pyH, pylag_val, lambdaI, lambdaAR,
                                    lambdaLag, period_W, period_H, period_Lag, missing, verbose);
    if (!s) {                                        // diagnostics already on stderr; outputs untouched
        prof.failed = 1; prof.total_s = prof.setup_s = TrmfSessionImpl::now_s() - t0;
        std::lock_guard<std::mutex> lk(g_prof_mu); g_last_profile = prof; g_have_profile = true;
        return;
    }
    (void)s->all([&](TrmfSessionImpl *t) {
        t->log_norms = verbose > 0;                  // the norm lines exist only under verbose (trmf.cpp:659-688)
        t->ev_period = 0;                            // nobody reads per-phase times of a one-shot call (they cost 21-26 us per iteration)
        return 0;
    });
    const double t1 = TrmfSessionImpl::now_s();
    int rc = s->all([&](TrmfSessionImpl *t) { const int r = t->run(max_iter); return r ? r : t->sync(); });
    const double t2 = TrmfSessionImpl::now_s();
    // the factors come back through host staging and are committed together: a failure anywhere -- on ANY rank -- leaves W, H and
    // lag_val as the caller passed them (the reference's contract for a failed call, trmf.cpp:632-634).  Staged and committed on rank
    // 0's thread (the staging lease is a mutex: locked and released by one thread); every rank holds the same factors.
    size_t d2h = 0;
    if (rc == 0)
        rc = s->rank0([&](TrmfSessionImpl *t) {
            TrmfSessionImpl::StagedFactors staged;
            const int r = t->download_staged(staged);
            if (r == 0) { staged.commit(pyW->val, pyH->val, pylag_val->val); d2h = staged.bW + staged.bH + staged.bL; }
            return r;
        });
    if (rc) fprintf(stderr, "[ERR MSG]: device failure, outputs untouched: %s\n", trmf_last_error());
    const double t3 = TrmfSessionImpl::now_s();
    prof.upload_s = s->first()->t_upload_s; prof.bytes_h2d = s->first()->bytes_uploaded;
    prof.bytes_d2h = (double)d2h;
    delete s;
    const double t4 = TrmfSessionImpl::now_s();
    const DevicePool::Stats ps1 = DevicePool::current().stats();
    prof.total_s = t4 - t0; prof.setup_s = t1 - t0; prof.compute_s = t2 - t1; prof.download_s = t3 - t2; prof.teardown_s = t4 - t3;
    prof.iters = max_iter; prof.device_mallocs = (int32_t)(ps1.hip_mallocs - ps0.hip_mallocs); prof.pool_reused = (int32_t)(ps1.reused - ps0.reused);
    prof.failed = rc != 0;
    std::lock_guard<std::mutex> lk(g_prof_mu); g_last_profile = prof; g_have_profile = true;
}

// ------------------------------------------------------------------------------------------------
// Section 2
// ------------------------------------------------------------------------------------------------
int32_t trmf_sizeof_real(void) { return (int32_t)sizeof(real); }

int32_t trmf_last_train_profile(TrmfTrainProfile *out) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_have_profile || !out) return kFail;
    *out = g_last_profile;
    return 0;
}
int32_t trmf_release_cached(void) {
    SessionGroup::drop_idle();           // worker threads + communicators of the TRMF_DEVICES mode kept between calls
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    DevicePool::current().trim();
    StreamCache::drop_idle();
    HostStager::current().release_staging();
    HostStager::current().release_ring();
    return 0;
}

int32_t trmf_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

int32_t trmf_set_device(int32_t device) {
    int cnt = trmf_device_count();
    if (device < 0 || device >= cnt) { set_error("device index out of range"); return kFail; }
    g_device = device;
    return hipSetDevice(device) == hipSuccess ? 0 : kFail;
}

int64_t trmf_device_free_bytes(void) {
    DeviceGuard guard;
    if (!guard.ok) return -1;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return -1;
    return (int64_t)free_b;
}

int64_t trmf_device_pool_live_bytes(void) {
    DeviceGuard guard;
    if (!guard.ok) return -1;
    return (int64_t)DevicePool::current().stats().live_bytes;
}

const char *trmf_last_error(void) {
    static thread_local std::string copy;
    std::lock_guard<std::mutex> lk(g_err_mu);
    copy = g_last_error;
    return copy.c_str();
}

TrmfSession *trmf_session_create(const PyMatrix *Y, const uint32_t *lag_set, uint32_t lag_size,
                                 const PyMatrix *W, const PyMatrix *H, const PyMatrix *lag_val,
                                 double lambdaI, double lambdaAR, double lambdaLag, int32_t period_W,
                                 int32_t period_H, int32_t period_Lag, int32_t missing, int32_t verbose) {
    DeviceGuard guard;
    return reinterpret_cast<TrmfSession *>(make_session(Y, lag_set, lag_size, W, H, lag_val, lambdaI, lambdaAR,
                                                        lambdaLag, period_W, period_H, period_Lag, missing, verbose));
}
#define HND(s) reinterpret_cast<SessionHandle *>(s)

int32_t trmf_session_run(TrmfSession *s, int32_t iters) {
    if (!s) return kFail;
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { if (iters > 0) t->adapt_stale(); return t->run(iters); }) : kFail;   // (W is about to change)
}
int32_t trmf_session_log_norms(TrmfSession *s, int32_t on) {
    if (!s) return kFail;
    return HND(s)->all([&](TrmfSessionImpl *t) { t->log_norms = on != 0; return 0; });
}
int32_t trmf_session_set_timing(TrmfSession *s, int32_t period) {
    if (!s || period < 0) return kFail;
    return HND(s)->all([&](TrmfSessionImpl *t) { t->ev_period = period; return 0; });
}
int32_t trmf_session_sync(TrmfSession *s) {
    if (!s) return kFail;
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->sync(); }) : kFail;
}
int32_t trmf_session_mark(TrmfSession *s) {
    if (!s) return kFail;
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->mark(); }) : kFail;
}
int32_t trmf_session_rewind(TrmfSession *s) {
    if (!s) return kFail;
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->rewind(); }) : kFail;
}
int32_t trmf_session_append_rows(TrmfSession *s, const PyMatrix *Ynew) {
    if (!s || !Ynew) { set_error("null session or block"); return kFail; }
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->append_rows(Ynew); }) : kFail;
}
// Every argument is checked here, on the calling thread, before any rank's worker runs (a rejected call must not break the barrier
// of a TRMF_DEVICES group).
int32_t trmf_session_slide(TrmfSession *s, const PyMatrix *Ynew, int32_t retire, int32_t downdate_stats, TrmfSlideSums *out) {
    if (!s) { set_error("null session"); return kFail; }
    const std::string why = HND(s)->first()->slide_refusal(Ynew, retire, downdate_stats);
    if (!why.empty()) { set_error(why); return kFail; }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    const auto all = HND(s)->per_rank<TrmfSessionImpl::SlideResult>(
        [&](TrmfSessionImpl *t, int, TrmfSessionImpl::SlideResult *r) { return t->slide(Ynew, retire, downdate_stats != 0, r); });
    if (all.empty()) return kFail;
    if (out) {
        const auto &res = all[0];
        out->rows_retired = res.rows_retired; out->entries_retired = res.entries_retired; out->rows_appended = res.rows_appended;
        out->entries_appended = res.entries_appended; out->rows = res.rows; out->entries = res.entries;
    }
    return 0;
}
// Series churn: validated here like slide; a pivot of the cold-start fit that is not positive is found by every rank alike and
// reported here, not by a failing worker task.
int32_t trmf_session_change_series(TrmfSession *s, const uint8_t *keep, const PyMatrix *Ynew, int32_t fit, const void *Hnew, const void *tr_a_new,
                                   const void *tr_b_new, TrmfChurnSums *out) {
    if (!s) { set_error("null session"); return kFail; }
    const std::string why = HND(s)->first()->churn_refusal(keep, Ynew, fit, Hnew, (const real *)tr_a_new, (const real *)tr_b_new);
    if (!why.empty()) { set_error(why); return kFail; }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    const auto res = HND(s)->per_rank<TrmfSessionImpl::ChurnResult>([&](TrmfSessionImpl *t, int, TrmfSessionImpl::ChurnResult *r) {
        return t->change_series(keep, Ynew, fit != 0, (const real *)Hnew, (const real *)tr_a_new, (const real *)tr_b_new, r);
    });
    if (res.empty()) return kFail;
    for (const auto &r : res)
        if (r.bad_series >= 0) {
            const TrmfSessionImpl *f = HND(s)->first();
            set_error((f->full ? std::string("change_series: the new series' shared system") : "change_series: new series " + std::to_string(r.bad_series)) +
                      ": a pivot of S + lambdaI I is not positive and finite (lambdaI == 0 and a new series with fewer independent rows than the "
                      "rank?); nothing was changed");
            return kFail;
        }
    if (out) {
        const auto &r = res[0];
        out->series_before = r.series_before; out->series_retired = r.series_retired; out->series_added = r.series_added; out->series = r.series;
        out->entries_retired = r.entries_retired; out->entries_added = r.entries_added; out->entries = r.entries;
        out->heldout_dropped = r.heldout_dropped; out->fitted = r.fitted; out->stats_carried = r.stats_carried; out->sq_err_new = r.sq_err_new;
    }
    return 0;
}
// Cell revisions: validated here like slide and change_series.
int32_t trmf_session_revise(TrmfSession *s, uint64_t count, const uint32_t *rows, const uint32_t *cols, const void *vals, const uint8_t *del,
                            int32_t update_stats, TrmfReviseSums *out) {
    if (!s) { set_error("null session"); return kFail; }
    const std::string why = HND(s)->first()->revise_refusal(count, rows, cols, vals, del, update_stats);
    if (!why.empty()) { set_error(why); return kFail; }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    const auto all = HND(s)->per_rank<TrmfSessionImpl::ReviseResult>([&](TrmfSessionImpl *t, int, TrmfSessionImpl::ReviseResult *r) {
        return t->revise(count, rows, cols, (const real *)vals, del, update_stats != 0, r);
    });
    if (all.empty()) return kFail;
    if (out) {
        const auto &r = all[0];
        out->edits = r.edits; out->inserted = r.inserted; out->replaced = r.replaced; out->deleted = r.deleted; out->missed = r.missed;
        out->copies_removed = r.copies_removed; out->entries_before = r.entries_before; out->entries = r.entries;
        out->first_row = r.first_row; out->last_row = r.last_row; out->stats_carried = r.stats_carried;
    }
    return 0;
}
int32_t trmf_session_row_entries(TrmfSession *s, uint64_t *per_row) {
    if (!s || !per_row) { set_error("null argument"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    if (f->dense) { set_error("row_entries: dense storage holds every cell"); return kFail; }
    for (int i = 0; i < f->T; i++) per_row[i] = f->host_row_ptr[(size_t)i + 1] - f->host_row_ptr[(size_t)i];
    return 0;
}
int32_t trmf_session_rows(TrmfSession *s) { return s ? HND(s)->first()->T : kFail; }
int32_t trmf_session_set_series_transform(TrmfSession *s, const void *a, const void *b) {
    if (!s) { set_error("null session"); return kFail; }
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->set_series_transform((const real *)a, (const real *)b); }) : kFail;
}

int32_t trmf_session_download(TrmfSession *s, PyMatrix *W, PyMatrix *H, PyMatrix *lag_val) {
    if (!s) return kFail;
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    if (HND(s)->all([&](TrmfSessionImpl *t) { return t->sync(); })) return kFail;       // every rank holds the same factors: rank 0 answers
    return HND(s)->rank0([&](TrmfSessionImpl *t) -> int {
        if (W && (W->rows != (uint64_t)t->T || W->cols != (uint64_t)t->k || W->type != TRMF_DENSE_ROWMAJOR)) { set_error("W shape/layout mismatch"); return kFail; }
        if (H && (H->rows != (uint64_t)t->n || H->cols != (uint64_t)t->k || H->type != TRMF_DENSE_ROWMAJOR)) { set_error("H shape/layout mismatch"); return kFail; }
        if (lag_val && (lag_val->rows != (uint64_t)t->nlag || lag_val->cols != (uint64_t)t->k || lag_val->type != TRMF_DENSE_COLMAJOR)) { set_error("lag_val shape/layout mismatch"); return kFail; }
        if (W && t->download_padded(t->W, (real *)W->val, t->T)) return kFail;
        if (H && t->download_padded(t->H, (real *)H->val, t->n)) return kFail;
        if (lag_val && t->nlag)
            TRMF_HIP_CHECK(hipMemcpy(lag_val->val, t->theta.p, sizeof(real) * (size_t)t->nlag * t->k, hipMemcpyDeviceToHost));
        return 0;
    });
}

int32_t trmf_session_stats(TrmfSession *s, TrmfIterStats *out, int32_t cap) {
    if (!(s && out && cap > 0)) return 0;
    DeviceGuard guard;
    if (!guard.ok) return 0;
    if (HND(s)->group && HND(s)->all([&](TrmfSessionImpl *t) { return t->sync(); })) return 0;
    int cnt = 0;
    (void)HND(s)->rank0([&](TrmfSessionImpl *t) { cnt = t->stats(out, cap); return cnt < 0 ? kFail : 0; });
    return cnt < 0 ? 0 : cnt;
}
double trmf_session_objective(TrmfSession *s) {
    if (!s) return NAN;
    DeviceGuard guard;
    if (!guard.ok) return NAN;
    double J = NAN;
    (void)HND(s)->all([&](TrmfSessionImpl *t) { const double v = t->objective(); if (t->comm->rank == 0) J = v; return 0; });
    return J;
}
double trmf_session_fsolve_bytes(TrmfSession *s) { return s ? HND(s)->first()->fsolve_bytes() : 0.0; }
int32_t trmf_session_describe(TrmfSession *s, char *buf, int32_t cap) {
    if (!s) return kFail;
    std::string d = HND(s)->first()->describe();
    if (HND(s)->group) d += "; ranks are threads of this process (TRMF_DEVICES), communicator: " + HND(s)->group->comm_kind;
    if (buf && cap > 0) { std::strncpy(buf, d.c_str(), (size_t)cap - 1); buf[cap - 1] = 0; }
    return (int32_t)d.size();
}
void trmf_session_destroy(TrmfSession *s) {
    if (!s) return;
    DeviceGuard guard;
    delete HND(s);
}

// Held-out set and weights: every argument is checked here, on the calling thread, before any rank's worker runs -- a rejected
// call must not break the barrier of a TRMF_DEVICES group (a failed worker task poisons it).
int32_t trmf_session_set_heldout(TrmfSession *s, const PyMatrix *Yt) {
    if (!s) { set_error("null session"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    std::vector<uint32_t> rows;
    if (Yt) {
        if (Yt->type != TRMF_SPARSE) { set_error("set_heldout: Ytest must be a sparse PyMatrix"); return kFail; }
        if (Yt->cols != (uint64_t)f->n) { set_error("set_heldout: Ytest has " + std::to_string(Yt->cols) + " columns, the session " + std::to_string(f->n)); return kFail; }
        if (Yt->rows > (uint64_t)f->T) { set_error("set_heldout: Ytest has more rows than the session's W (" + std::to_string(f->T) + ")"); return kFail; }
        if (Yt->nnz >= (1ull << 32)) { set_error("set_heldout: Ytest exceeds 32-bit entry indices"); return kFail; }
        if (!Yt->row_ptr || (Yt->nnz && (!Yt->col_idx || !Yt->val_t))) { set_error("set_heldout: Ytest lacks its CSR arrays"); return kFail; }
        if (Yt->row_ptr[0] != 0 || Yt->row_ptr[Yt->rows] != Yt->nnz) { set_error("set_heldout: Ytest row pointers do not span its entries"); return kFail; }
        rows.resize(Yt->nnz);
        for (uint64_t i = 0; i < Yt->rows; i++) {
            const size_t p0 = Yt->row_ptr[i], p1 = Yt->row_ptr[i + 1];
            if (p1 < p0 || p1 > Yt->nnz) { set_error("set_heldout: Ytest row pointers are not ascending"); return kFail; }
            for (size_t e = p0; e < p1; e++) rows[e] = (uint32_t)i;
        }
        for (uint64_t e = 0; e < Yt->nnz; e++)
            if (Yt->col_idx[e] >= (uint32_t)f->n) { set_error("set_heldout: Ytest column index " + std::to_string(Yt->col_idx[e]) + " out of range"); return kFail; }
    }
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->set_heldout(Yt, rows); }) : kFail;
}
int32_t trmf_session_eval_heldout(TrmfSession *s, TrmfHeldoutSums *out, void *pred) {
    if (!s || !out) { set_error("null session or output"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    if (!f->ho_set) { set_error("eval_heldout: no held-out set (trmf_session_set_heldout)"); return kFail; }
    if (f->has_transform) { set_error("eval_heldout: the session trains on a series transform; held-out truths would be in another scale"); return kFail; }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    if (HND(s)->all([&](TrmfSessionImpl *t) { return t->sync(); })) return kFail;       // every rank holds the same factors: rank 0 answers
    TrmfHeldoutSums sums{};
    const int rc = HND(s)->rank0([&](TrmfSessionImpl *t) { return t->eval_heldout(&sums, (real *)pred); });
    if (rc == 0) *out = sums;
    return rc;
}
// Forecast: like the held-out calls, every argument is checked on the calling thread before any rank's worker runs.
static int check_forecast_args(const TrmfSessionImpl *f, const std::string &what, int32_t steps, int32_t clip, double threshold, const PyMatrix *truth) {
    if (steps < 1) { set_error(what + ": steps must be at least 1"); return kFail; }
    if ((uint64_t)f->T + (uint64_t)steps + 1 >= (1ull << 24) || (uint64_t)steps * (uint64_t)f->n >= (1ull << 32)) {
        set_error(what + ": the window would exceed 32-bit device indices"); return kFail;
    }
    if (clip && !std::isfinite(threshold)) { set_error(what + ": the threshold must be finite"); return kFail; }
    if (truth) {
        if (truth->type != TRMF_DENSE_ROWMAJOR && truth->type != TRMF_DENSE_COLMAJOR) { set_error(what + ": the truth must be a dense PyMatrix"); return kFail; }
        if (truth->rows != (uint64_t)steps || truth->cols != (uint64_t)f->n) {
            set_error(what + ": the truth is " + std::to_string(truth->rows) + " x " + std::to_string(truth->cols) + ", the forecast " + std::to_string(steps) +
                      " x " + std::to_string(f->n));
            return kFail;
        }
        if (!truth->val) { set_error(what + ": the truth lacks its values"); return kFail; }
    }
    return 0;
}
int32_t trmf_session_forecast(TrmfSession *s, int32_t steps, int32_t clip, double threshold, const PyMatrix *truth, void *Ynew, void *Wnew) {
    if (!s) { set_error("null session"); return kFail; }
    if (check_forecast_args(HND(s)->first(), "forecast", steps, clip, threshold, truth)) return kFail;
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    if (HND(s)->all([&](TrmfSessionImpl *t) { return t->sync(); })) return kFail;       // every rank holds the same factors: rank 0 answers
    return HND(s)->rank0([&](TrmfSessionImpl *t) { return t->forecast(steps, clip != 0, threshold, truth, (real *)Ynew, (real *)Wnew); });
}
int32_t trmf_session_forecast_scores(TrmfSession *s, uint64_t *rows_scored, TrmfSeriesSums *per_series) {
    if (!s) { set_error("null session"); return kFail; }
    static_assert(sizeof(TrmfSeriesSums) == kFcSums * sizeof(double), "the resident table is an array of TrmfSeriesSums");
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    return HND(s)->rank0([&](TrmfSessionImpl *t) { return t->forecast_scores(rows_scored, reinterpret_cast<double *>(per_series)); });
}
int32_t trmf_session_forecast_reset(TrmfSession *s) {
    if (!s) { set_error("null session"); return kFail; }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    return HND(s)->rank0([&](TrmfSessionImpl *t) { return t->forecast_reset(); });
}
int32_t trmf_session_set_lambdas(TrmfSession *s, double lambdaI, double lambdaAR, double lambdaLag) {
    if (!s) { set_error("null session"); return kFail; }
    if (!std::isfinite(lambdaI) || !std::isfinite(lambdaAR) || !std::isfinite(lambdaLag)) { set_error("set_lambdas: weights must be finite"); return kFail; }
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->set_lambdas(lambdaI, lambdaAR, lambdaLag); }) : kFail;
}
int32_t trmf_session_set_lag_penalty(TrmfSession *s, double lambdaLagL1, int32_t refit) {
    if (!s) { set_error("null session"); return kFail; }
    if (!std::isfinite(lambdaLagL1) || lambdaLagL1 < 0) { set_error("set_lag_penalty: lambdaLagL1 must be finite and not negative"); return kFail; }
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->set_lag_penalty(lambdaLagL1, refit); }) : kFail;
}
int32_t trmf_session_solve_lags(TrmfSession *s) {
    if (!s) { set_error("null session"); return kFail; }
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->solve_lags(); }) : kFail;
}
int32_t trmf_session_lag_stats(TrmfSession *s, int32_t *per_dim, int32_t *capped, int32_t *refit_skipped) {
    if (!s) { set_error("null session"); return kFail; }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    if (HND(s)->all([&](TrmfSessionImpl *t) { return t->sync(); })) return kFail;       // every rank holds the same record: rank 0 answers
    return HND(s)->rank0([&](TrmfSessionImpl *t) { return t->lag_stats(per_dim, capped, refit_skipped); });
}

// The online solves.  Every argument -- the scales included, which every rank receives as the same host values -- is checked on the
// calling thread before any rank's worker runs (the helpers above; see trmf_session_set_heldout); a bad pivot or a pool without
// room is found on the device by every rank alike and reported here, not by a failing worker task.
int32_t trmf_session_assimilate(TrmfSession *s, int32_t first_row, TrmfAssimilateSums *out, void *Wnew) {
    if (!s) { set_error("null session"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    const std::string what = "assimilate";
    if (online_refusal(f, what) || first_row_refusal(f, what, first_row)) return kFail;
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    const auto res = HND(s)->per_rank<TrmfSessionImpl::AssimResult>(
        [&](TrmfSessionImpl *t, int slot, TrmfSessionImpl::AssimResult *r) { return t->assimilate(first_row, r, slot == 0 ? (real *)Wnew : nullptr); });
    if (res.empty() || pivot_refusal(what, res, "G")) return kFail;
    if (out) { out->rows = res[0].rows; out->entries = res[0].entries; out->sq_err_before = res[0].sq_err_before; out->sq_err_after = res[0].sq_err_after; }
    return 0;
}

int32_t trmf_session_assimilate_robust(TrmfSession *s, int32_t first_row, double c, int32_t sweeps, const double *scale, TrmfRobustSums *out,
                                       void *Wnew, void *weights) {
    if (!s) { set_error("null session"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    const std::string what = "assimilate_robust";
    if (online_refusal(f, what) || weight_slot_refusal(f, what) || first_row_refusal(f, what, first_row) ||
        huber_refusal(what, c, sweeps, kAssimRobustMaxSweeps, "the plain filter") || scale_refusal(f, what, scale)) return kFail;
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    std::vector<double> sc;
    if (resolve_scales(HND(s), f, what, scale, sc)) return kFail;
    const auto res = HND(s)->per_rank<TrmfSessionImpl::RobustResult>([&](TrmfSessionImpl *t, int slot, TrmfSessionImpl::RobustResult *r) {
        return t->assimilate_robust(first_row, c, sweeps, sc.data(), r, slot == 0 ? (real *)Wnew : nullptr, slot == 0 ? (real *)weights : nullptr);
    });
    if (res.empty() || pivot_refusal(what, res, "the weighted G")) return kFail;
    if (out) {
        out->rows = res[0].rows; out->entries = res[0].entries; out->downweighted = res[0].downweighted;
        out->weight_sum = res[0].weight_sum; out->sq_err_before = res[0].sq_err_before; out->sq_err_after = res[0].sq_err_after;
    }
    return 0;
}

// Fixed-interval smoother: a bad pivot is one of a preconditioner block.
int32_t trmf_session_smooth(TrmfSession *s, int32_t first_row, double rtol, int32_t max_iter, TrmfSmoothSums *out, void *Wnew) {
    if (!s) { set_error("null session"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    const std::string what = "smooth";
    if (online_refusal(f, what) || first_row_refusal(f, what, first_row) || window_refusal(f, what, first_row) || window_refusal(what, rtol, max_iter))
        return kFail;
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    const auto res = HND(s)->per_rank<TrmfSessionImpl::SmoothResult>([&](TrmfSessionImpl *t, int slot, TrmfSessionImpl::SmoothResult *r) {
        return t->smooth(first_row, rtol, max_iter, r, slot == 0 ? (real *)Wnew : nullptr);
    });
    if (res.empty() || pivot_refusal(what, res, "G")) return kFail;
    if (out) {
        const auto &r = res[0];
        out->rows = r.rows; out->entries = r.entries; out->iterations = r.iterations; out->converged = r.converged; out->residual = r.residual;
        out->sq_err_before = r.sq_err_before; out->sq_err_after = r.sq_err_after;
        out->objective_before = r.objective_before; out->objective_after = r.objective_after;
    }
    return 0;
}

// Robust smoother: the checks of trmf_session_smooth and of trmf_session_assimilate_robust.
int32_t trmf_session_smooth_robust(TrmfSession *s, int32_t first_row, double c, int32_t sweeps, const double *scale, double rtol, int32_t max_iter,
                                   TrmfRobustSmoothSums *out, void *Wnew, void *weights) {
    if (!s) { set_error("null session"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    const std::string what = "smooth_robust";
    if (online_refusal(f, what) || weight_slot_refusal(f, what) || first_row_refusal(f, what, first_row) || window_refusal(f, what, first_row) ||
        huber_refusal(what, c, sweeps, kSmoothRobustMaxSweeps, "the plain smoother's objective") || window_refusal(what, rtol, max_iter) ||
        scale_refusal(f, what, scale)) return kFail;
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    std::vector<double> sc;
    if (resolve_scales(HND(s), f, what, scale, sc)) return kFail;
    const auto res = HND(s)->per_rank<TrmfSessionImpl::RobustSmoothResult>([&](TrmfSessionImpl *t, int slot, TrmfSessionImpl::RobustSmoothResult *r) {
        return t->smooth_robust(first_row, c, sweeps, sc.data(), rtol, max_iter, r, slot == 0 ? (real *)Wnew : nullptr, slot == 0 ? (real *)weights : nullptr);
    });
    if (res.empty() || pivot_refusal(what, res, "the weighted G")) return kFail;
    if (out) {
        const auto &r = res[0];
        out->rows = r.rows; out->entries = r.entries; out->downweighted = r.downweighted;
        out->sweeps = r.sweeps; out->iterations = r.iterations; out->converged = r.converged; out->reserved = 0;
        out->residual = r.residual; out->weight_sum = r.weight_sum;
        out->sq_err_before = r.sq_err_before; out->sq_err_after = r.sq_err_after;
        out->objective_before = r.objective_before; out->objective_after = r.objective_after;
    }
    return 0;
}

// Online loading updates: the state of the tables is checked like an argument.
static int adapt_call(TrmfSession *s, bool init, double forget, TrmfAdaptSums *out, void *Hnew) {
    const std::string what = init ? "series_stats_init" : "adapt_series";
    const TrmfSessionImpl *f = HND(s)->first();
    if (rank_refusal(f, what)) return kFail;
    if (init && !(forget > 0 && forget <= 1)) { set_error("series_stats_init: forget must lie in (0, 1]"); return kFail; }
    if (!init && stats_refusal(f, what)) return kFail;
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    const auto res = HND(s)->per_rank<TrmfSessionImpl::AdaptResult>([&](TrmfSessionImpl *t, int slot, TrmfSessionImpl::AdaptResult *r) {
        return t->adapt_series(init, forget, r, slot == 0 ? (real *)Hnew : nullptr);
    });
    if (res.empty()) return kFail;
    for (const auto &r : res) {
        if (r.no_memory) {
            const size_t PK = adapt_packed(f->k);
            const double bytes = 2.0 * ((f->full ? (double)PK : (double)f->n * (double)PK) + (double)f->n * f->k) * sizeof(real);
            set_error("series_stats_init: the device pool cannot hold the series statistics (two generations of n k (k + 1) / 2 + n k reals: " +
                      std::to_string((unsigned long long)bytes) + " bytes); nothing was changed");
            return kFail;
        }
        if (r.bad_series >= 0) {
            set_error("adapt_series: series " + std::to_string(r.bad_series) + ": a pivot of S + lambdaI I is not positive and finite (lambdaI == 0 and "
                      "a series with fewer independent rows than the rank?); nothing was changed");
            return kFail;
        }
    }
    if (out) {
        out->series = res[0].series; out->rows = res[0].rows; out->entries = res[0].entries;
        out->sq_err_before = res[0].sq_err_before; out->sq_err_after = res[0].sq_err_after; out->max_abs_change = res[0].max_abs_change;
    }
    return 0;
}
int32_t trmf_session_series_stats_init(TrmfSession *s, double forget) {
    if (!s) { set_error("null session"); return kFail; }
    return adapt_call(s, true, forget, nullptr, nullptr);
}
int32_t trmf_session_adapt_series(TrmfSession *s, TrmfAdaptSums *out, void *Hnew) {
    if (!s) { set_error("null session"); return kFail; }
    return adapt_call(s, false, 1.0, out, Hnew);
}
// Robust online loading update: the checks of adapt_series and of assimilate_robust's c, sweeps and scale.
int32_t trmf_session_adapt_series_robust(TrmfSession *s, double c, int32_t sweeps, const double *scale, TrmfRobustAdaptSums *out, void *Hnew,
                                         uint64_t *wptr, uint32_t *wrows, void *weights) {
    if (!s) { set_error("null session"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    const std::string what = "adapt_series_robust";
    if (rank_refusal(f, what)) return kFail;
    if (f->full) {
        set_error(std::string("adapt_series_robust: ") + (f->dense ? "dense storage" : "sparse storage with missing == 0") +
                  " is a full-observation form: it keeps ONE shared S for all series, and a weight per cell needs a table per series "
                  "(sparse storage with missing != 0); use adapt_series");
        return kFail;
    }
    if (stats_refusal(f, what) || huber_refusal(what, c, sweeps, kAdaptRobustMaxSweeps, "the plain update") || scale_refusal(f, what, scale)) return kFail;
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    std::vector<double> sc;
    if (resolve_scales(HND(s), f, what, scale, sc)) return kFail;
    const auto res = HND(s)->per_rank<TrmfSessionImpl::RobustAdaptResult>([&](TrmfSessionImpl *t, int slot, TrmfSessionImpl::RobustAdaptResult *r) {
        const bool lead = slot == 0;
        return t->adapt_series_robust(c, sweeps, sc.data(), r, lead ? (real *)Hnew : nullptr, lead ? wptr : nullptr, lead ? wrows : nullptr,
                                      lead ? (real *)weights : nullptr);
    });
    if (res.empty()) return kFail;
    for (const auto &r : res)
        if (r.bad_series >= 0) {
            set_error("adapt_series_robust: series " + std::to_string(r.bad_series) + ": a pivot of the weighted S + lambdaI I is not positive and finite "
                      "(lambdaI == 0 and a series with fewer independent rows than the rank?); nothing was changed");
            return kFail;
        }
    if (out) {
        const auto &r = res[0];
        out->series = r.series; out->rows = r.rows; out->entries = r.entries; out->downweighted = r.downweighted;
        out->sq_err_before = r.sq_err_before; out->sq_err_after = r.sq_err_after; out->max_abs_change = r.max_abs_change;
        out->weight_sum = r.weight_sum; out->objective_before = r.objective_before; out->objective_after = r.objective_after;
    }
    return 0;
}
int32_t trmf_session_series_stats_info(TrmfSession *s, int32_t *valid, int32_t *absorbed_rows, double *forget) {
    if (!s) { set_error("null session"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    if (valid) *valid = !f->ad_exists ? 0 : f->ad_valid ? 1 : -1;
    if (absorbed_rows) *absorbed_rows = f->ad_exists ? f->ad_rows : 0;
    if (forget) *forget = f->ad_exists ? f->ad_gamma : 1.0;
    return 0;
}

// Forecast uncertainty: the arguments are checked on the calling thread before any rank's worker runs (see trmf_session_set_heldout);
// a training matrix without a stored entry is found by every rank alike and reported here, not by a failing worker task.
int32_t trmf_session_fit_noise(TrmfSession *s, TrmfNoiseStats *out) {
    if (!s) { set_error("null session"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    if (f->T <= f->midx) {
        set_error("fit_noise: " + std::to_string(f->T) + " rows do not reach past the largest lag " + std::to_string(f->midx));
        return kFail;
    }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    const auto res = HND(s)->per_rank<TrmfSessionImpl::NoiseResult>([&](TrmfSessionImpl *t, int, TrmfSessionImpl::NoiseResult *r) { return t->fit_noise(r); });
    if (res.empty()) return kFail;
    for (const auto &r : res)
        if (r.no_entries) { set_error("fit_noise: the training matrix has no stored entry; nothing was changed"); return kFail; }
    if (out) {
        out->pooled_sigma2 = res[0].pooled; out->sigma2_min = res[0].s2_min; out->sigma2_max = res[0].s2_max;
        out->series_pooled = res[0].series_pooled; out->q_min = res[0].q_min; out->q_max = res[0].q_max;
    }
    return 0;
}
int32_t trmf_session_noise(TrmfSession *s, double *sigma2, double *q) {
    if (!s) { set_error("null session"); return kFail; }
    if (!HND(s)->first()->nz_set) { set_error("noise: none has been fitted or set (trmf_session_fit_noise / _set_noise)"); return kFail; }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    return HND(s)->rank0([&](TrmfSessionImpl *t) { return t->noise(sigma2, q); });
}
int32_t trmf_session_set_noise(TrmfSession *s, const double *sigma2, const double *q) {
    if (!s || !sigma2 || !q) { set_error("set_noise: null session or table"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    for (int j = 0; j < f->n; j++)
        if (!(std::isfinite(sigma2[j]) && sigma2[j] >= 0)) { set_error("set_noise: sigma2[" + std::to_string(j) + "] is negative or not finite"); return kFail; }
    for (int t = 0; t < f->k; t++)
        if (!(std::isfinite(q[t]) && q[t] >= 0)) { set_error("set_noise: q[" + std::to_string(t) + "] is negative or not finite"); return kFail; }
    DeviceGuard guard;
    return guard.ok ? HND(s)->all([&](TrmfSessionImpl *t) { return t->set_noise(sigma2, q); }) : kFail;
}
int32_t trmf_session_forecast_dist(TrmfSession *s, int32_t steps, int32_t clip, double threshold, double zq, const PyMatrix *truth,
                                   void *Ynew, void *Ysd, void *Wnew) {
    if (!s) { set_error("null session"); return kFail; }
    const TrmfSessionImpl *f = HND(s)->first();
    if (!f->nz_set) { set_error("forecast_dist: no noise has been fitted or set (trmf_session_fit_noise / _set_noise)"); return kFail; }
    if (!(std::isfinite(zq) && zq > 0)) { set_error("forecast_dist: zq must be positive and finite"); return kFail; }
    if (check_forecast_args(f, "forecast_dist", steps, clip, threshold, truth)) return kFail;
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    if (HND(s)->all([&](TrmfSessionImpl *t) { return t->sync(); })) return kFail;       // every rank holds the same factors: rank 0 answers
    return HND(s)->rank0([&](TrmfSessionImpl *t) { return t->forecast_dist(steps, clip != 0, threshold, zq, truth, (real *)Ynew, (real *)Ysd, (real *)Wnew); });
}
int32_t trmf_session_interval_scores(TrmfSession *s, uint64_t *rows_scored, TrmfIntervalSums *per_series) {
    if (!s) { set_error("null session"); return kFail; }
    static_assert(sizeof(TrmfIntervalSums) == kIvSums * sizeof(double), "the resident table is an array of TrmfIntervalSums");
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    return HND(s)->rank0([&](TrmfSessionImpl *t) { return t->interval_scores(rows_scored, reinterpret_cast<double *>(per_series)); });
}
int32_t trmf_session_interval_reset(TrmfSession *s) {
    if (!s) { set_error("null session"); return kFail; }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    return HND(s)->rank0([&](TrmfSessionImpl *t) { return t->interval_reset(); });
}

// ---- multi-GPU ----------------------------------------------------------------------------------
int32_t trmf_dist_get_unique_id(void *out_id) {
    RcclApi &api = rccl_api();
    if (!api.load()) return kFail;
    RcclApi::UniqueId id;
    const int rc = api.GetUniqueId(&id);
    if (rc != 0) { set_error(std::string("ncclGetUniqueId: ") + api.GetErrorString(rc)); return kFail; }
    std::memcpy(out_id, &id, TRMF_UNIQUE_ID_BYTES);
    return 0;
}

int32_t trmf_dist_init(int32_t rank, int32_t world, const void *id_bytes) {
    if (world < 1 || rank < 0 || rank >= world) { set_error("bad rank/world"); return kFail; }
    if (world > kMaxWorld) { set_error("more ranks than the staged gather supports (64)"); return kFail; }
    DeviceGuard guard;
    if (!guard.ok) return kFail;
    RcclApi &api = rccl_api();
    if (!api.load()) return kFail;
    RcclApi::UniqueId id;
    std::memcpy(&id, id_bytes, TRMF_UNIQUE_ID_BYTES);
    std::shared_ptr<RcclComm> c = std::make_shared<RcclComm>();
    c->rank = rank; c->world = world; c->device = tl_device() >= 0 ? tl_device() : g_device;
    const int rc = api.CommInitRank(&c->comm, world, id, rank);
    if (rc != 0) { set_error(std::string("ncclCommInitRank: ") + api.GetErrorString(rc)); c->comm = nullptr; return kFail; }
    g_comm = std::move(c);
    return 0;
}

int32_t trmf_dist_init_callback(int32_t rank, int32_t world, trmf_allgatherv_fn fn, void *ctx) {
    if (world < 1 || rank < 0 || rank >= world || !fn) { set_error("bad rank/world/callback"); return kFail; }
    if (world > kMaxWorld) { set_error("more ranks than the staged gather supports (64)"); return kFail; }
    std::shared_ptr<CallbackComm> c = std::make_shared<CallbackComm>();
    c->rank = rank; c->world = world; c->fn = fn; c->ctx = ctx;
    g_comm = std::move(c);
    return 0;
}

int32_t trmf_dist_init_solo(int32_t rank, int32_t world) {
    if (world < 1 || rank < 0 || rank >= world || world > kMaxWorld) { set_error("bad rank/world"); return kFail; }
    std::shared_ptr<SoloComm> c = std::make_shared<SoloComm>();
    c->rank = rank; c->world = world;
    g_comm = std::move(c);
    return 0;
}

int32_t trmf_dist_rank(void) { return active_comm()->rank; }
int32_t trmf_dist_world(void) { return active_comm()->world; }
void trmf_dist_finalize(void) { g_comm.reset(); }

int32_t trmf_partition_by_nnz(uint64_t nrows, const size_t *ptr, int32_t world, uint64_t *bounds) {
    if (world < 1 || !ptr || !bounds) { set_error("bad arguments"); return kFail; }
    partition_by_nnz<size_t>(nrows, ptr, world, bounds);
    return 0;
}

}  // extern "C"
