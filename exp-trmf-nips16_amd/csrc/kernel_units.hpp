// kernel_units.hpp -- which translation unit compiles which kernel instantiations (round 5).
//
// Rounds 1-4 built each library from ONE translation unit: ~150 kernel instantiations, 5-6 minutes per library.  The four heavy
// template families are now instantiated explicitly in units of their own (csrc/unit_*.hip), compiled in parallel; the main
// unit (trmf_abi.hip: the host code and every other kernel) sees their declarations only and references their host stubs.  All units of a library are linked into one .so; each registers its own code object with the runtime, and a stub's
// address is the kernel's handle in every unit (checked on the GPU: scripts/ubench/tu_split).
//
//   unit_hv_rep.hip    hv_tile_kernel<MODE, KQ, false>   (32)  one rank / replicated CG, launch per step
//   unit_hv_wide.hip   hv_tile_kernel<MODE, KQ, false, 512> (32)  the same over wide tiles (512 threads; one rank)
//   unit_hv_shard.hip  hv_tile_kernel<MODE, KQ, true>    (32)  time-sharded CG, launch per step
//   unit_persist.hip   cg_persist_kernel<KQ, SHARD, NTH> (24)  the persistent CG kernel (256 threads: one rank / sharded; 512: one rank, wide tiles)
//   unit_gram.hip      fsolve_quad / fsolve_mfma (8), gram_x_kernel (16), loss_kernel (4)
//   unit_split.hip     the split path of long rows (round 6): gram_part_kernel (8), fsolve_*_long_kernel (8), gram_x_long_kernel (16)
//   unit_full.hip      the MFMA kernels of the full-observation path (20)
//   unit_heldout.hip   heldout_eval_kernel (5): the model at a resident set of held-out positions (trmf_session_eval_heldout)
//   unit_forecast.hip  forecast_rollout_kernel, forecast_score_kernel (5): the next timestamps forecast and scored (trmf_session_forecast)
//   unit_online.hip    assim_factor_kernel (4), assim_chain_kernel, assim_err_kernel: the forward filter of trmf_session_assimilate
//   unit_robust.hip    assim_robust_part_kernel (4), assim_robust_solve_kernel (4), assim_robust_prior_kernel: trmf_session_assimilate_robust
//   unit_uncertainty.hip  noise_resid_kernel (5), forecast_dist_kernel (5), the noise / psi kernels: trmf_session_fit_noise, _forecast_dist
//   unit_adapt.hip     adapt_series_kernel (4), adapt_part_kernel (4), the full-observation forms: trmf_session_adapt_series
//   unit_smooth.hip    smooth_ar_kernel, smooth_apply_kernel, smooth_update_kernel, smooth_finish_kernel: the windowed PCG of trmf_session_smooth
//   unit_smooth_robust.hip  smooth_robust_part_kernel (4), smooth_robust_fold_kernel (4): the weighted Grams of trmf_session_smooth_robust
//   unit_adapt_robust.hip   adapt_robust_series_kernel (4), adapt_robust_objective_kernel: trmf_session_adapt_series_robust
//   unit_slide.hip     csc_slide_count_kernel, csc_slide_kernel, series_downdate_kernel (4): the sliding window of trmf_session_slide
//   unit_churn.hip     csr_churn_count_kernel, csr_churn_kernel, csc_gather_kernel, dense_churn_kernel, row_gather_kernel: trmf_session_change_series
//   unit_revise.hip    revise_count_kernel, revise_kernel, dense_revise_kernel, series_revise_kernel (4): the cell revisions of trmf_session_revise
//
// A unit defines TRMF_UNIT before including this file; the non-template kernels of the shared headers are compiled by the main
// unit only (#if !defined(TRMF_UNIT) around them).
#pragma once

// (a unit includes only the headers of its own family: TRMF_UNIT = 1 gram, 2 hv_tile, 3 persist, 4 full, 5 held-out, 6 forecast, 7 online, 8 uncertainty, 9 robust online, 10 online loadings, 11 smoother, 12 robust smoother, 13 robust online loadings, 14 sliding window, 15 series churn, 16 cell revisions; the kernels of these families
// have their BODIES only where TRMF_UNIT_BODIES is defined -- the main unit sees declarations, so that it neither compiles them
// nor runs them through the optimiser as `extern template` would (available_externally bodies: 3 of its 3.5 minutes))
#if defined(TRMF_UNIT) || defined(TRMF_SINGLE_UNIT)
#define TRMF_UNIT_BODIES 1
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 1
#include "gram_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 2
#include "cg_kernels.hpp"
#endif
#if defined(TRMF_UNIT) && TRMF_UNIT == 4
#include "cg_kernels.hpp"
#include "gram_kernels.hpp"
#include "full_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 5
#include "heldout_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 6
#include "forecast_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 7
#include "online_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 8
#include "uncertainty_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 9
#include "robust_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 10
#include "adapt_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 11
#include "smooth_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 12
#include "smooth_robust_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 13
#include "adapt_robust_kernels.hpp"     // (includes adapt_kernels.hpp for the shared rank-1 update and factorisation)
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 14
#include "slide_kernels.hpp"            // (includes adapt_kernels.hpp for the shared rank-1 update)
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 15
#include "churn_kernels.hpp"
#endif
#if !defined(TRMF_UNIT) || TRMF_UNIT == 16
#include "revise_kernels.hpp"           // (includes adapt_kernels.hpp for the shared rank-1 update)
#endif
#if !defined(TRMF_UNIT)
#include "cg_persist_args.hpp"     // the declaration only: the body is unit_persist.hip's business
#elif TRMF_UNIT == 3
#include "cg_persist.hpp"
#endif
#if defined(TRMF_SINGLE_UNIT)
#include "cg_persist.hpp"
#endif

namespace trmf {

#define TRMF_HV_SIG (XParams, XState *, HvVecs, TileShard, int, int, const uint32_t *, const real *, const real *, const double *, double *, const PeerTable *, int, int)
#define TRMF_HV_KQS(X, MODE, SHARD, NTH)                           \
    X void hv_tile_kernel<MODE, 8, SHARD, NTH> TRMF_HV_SIG;        \
    X void hv_tile_kernel<MODE, 16, SHARD, NTH> TRMF_HV_SIG;       \
    X void hv_tile_kernel<MODE, 24, SHARD, NTH> TRMF_HV_SIG;       \
    X void hv_tile_kernel<MODE, 32, SHARD, NTH> TRMF_HV_SIG;       \
    X void hv_tile_kernel<MODE, 40, SHARD, NTH> TRMF_HV_SIG;       \
    X void hv_tile_kernel<MODE, 48, SHARD, NTH> TRMF_HV_SIG;       \
    X void hv_tile_kernel<MODE, 56, SHARD, NTH> TRMF_HV_SIG;       \
    X void hv_tile_kernel<MODE, 64, SHARD, NTH> TRMF_HV_SIG;
#define TRMF_UNIT_HV(X, SHARD, NTH)                                                                                   \
    TRMF_HV_KQS(X, HV_GRAD, SHARD, NTH) TRMF_HV_KQS(X, HV_CG_FIRST, SHARD, NTH) TRMF_HV_KQS(X, HV_CG_STEP, SHARD, NTH) TRMF_HV_KQS(X, HV_PLAIN, SHARD, NTH)

#define TRMF_PERSIST_SIG (XParams, XState *, PersistArgs)
#define TRMF_PERSIST_KQS(X, SHARD, NTH)                                  \
    X void cg_persist_kernel<8, SHARD, NTH> TRMF_PERSIST_SIG;            \
    X void cg_persist_kernel<16, SHARD, NTH> TRMF_PERSIST_SIG;           \
    X void cg_persist_kernel<24, SHARD, NTH> TRMF_PERSIST_SIG;           \
    X void cg_persist_kernel<32, SHARD, NTH> TRMF_PERSIST_SIG;           \
    X void cg_persist_kernel<40, SHARD, NTH> TRMF_PERSIST_SIG;           \
    X void cg_persist_kernel<48, SHARD, NTH> TRMF_PERSIST_SIG;           \
    X void cg_persist_kernel<56, SHARD, NTH> TRMF_PERSIST_SIG;           \
    X void cg_persist_kernel<64, SHARD, NTH> TRMF_PERSIST_SIG;
#define TRMF_UNIT_PERSIST(X) TRMF_PERSIST_KQS(X, false, 256) TRMF_PERSIST_KQS(X, true, 256) TRMF_PERSIST_KQS(X, false, 512)

#define TRMF_FSOLVE_SIG (const uint32_t *, const uint32_t *, const real *, const real *, real *, uint32_t, uint32_t, int, real, uint32_t, uint32_t)
#define TRMF_FSOLVE_LONG_SIG (SplitRows, real *, int, real)
#if defined(TRMF_F32)
#define TRMF_FSOLVE_ONE(X, NT, KMAX) X void fsolve_quad_kernel<NT, KMAX> TRMF_FSOLVE_SIG;
#define TRMF_FSOLVE_LONG_ONE(X, NT, KMAX) X void fsolve_quad_long_kernel<NT, KMAX> TRMF_FSOLVE_LONG_SIG;
#else
#define TRMF_FSOLVE_ONE(X, NT, KMAX) X void fsolve_mfma_kernel<NT, KMAX> TRMF_FSOLVE_SIG;
#define TRMF_FSOLVE_LONG_ONE(X, NT, KMAX) X void fsolve_mfma_long_kernel<NT, KMAX> TRMF_FSOLVE_LONG_SIG;
#endif
#define TRMF_GRAMX_SIG (const uint32_t *, const uint32_t *, const real *, const real *, real *, real *, uint32_t, uint32_t, int, uint32_t, size_t, uint32_t, const uint32_t *)
// the split path of long rows (gram_kernels.hpp "split rows"): partial Grams per item, then the row kernels' second halves
#define TRMF_GRAMX_LONG_SIG (SplitRows, real *, real *, int, size_t)
#define TRMF_GRAM_PART_SIG (const uint32_t *, const real *, const real *, const uint32_t *, uint32_t, uint32_t, real *, uint32_t, uint32_t)
#define TRMF_SPLIT_NT(X, NT)                                               \
    X void gram_part_kernel<NT, true> TRMF_GRAM_PART_SIG;                  \
    X void gram_part_kernel<NT, false> TRMF_GRAM_PART_SIG;                 \
    X void gram_x_long_kernel<NT, true, true> TRMF_GRAMX_LONG_SIG;         \
    X void gram_x_long_kernel<NT, true, false> TRMF_GRAMX_LONG_SIG;        \
    X void gram_x_long_kernel<NT, false, true> TRMF_GRAMX_LONG_SIG;        \
    X void gram_x_long_kernel<NT, false, false> TRMF_GRAMX_LONG_SIG;
#define TRMF_UNIT_SPLIT(X)                                                                                                   \
    TRMF_FSOLVE_LONG_ONE(X, 1, 8) TRMF_FSOLVE_LONG_ONE(X, 1, 16) TRMF_FSOLVE_LONG_ONE(X, 2, 24) TRMF_FSOLVE_LONG_ONE(X, 2, 32) \
    TRMF_FSOLVE_LONG_ONE(X, 3, 40) TRMF_FSOLVE_LONG_ONE(X, 3, 48) TRMF_FSOLVE_LONG_ONE(X, 4, 56) TRMF_FSOLVE_LONG_ONE(X, 4, 64) \
    TRMF_SPLIT_NT(X, 1) TRMF_SPLIT_NT(X, 2) TRMF_SPLIT_NT(X, 3) TRMF_SPLIT_NT(X, 4)
#define TRMF_GRAMX_NT(X, NT)                                     \
    X void gram_x_kernel<NT, true, true> TRMF_GRAMX_SIG;         \
    X void gram_x_kernel<NT, true, false> TRMF_GRAMX_SIG;        \
    X void gram_x_kernel<NT, false, true> TRMF_GRAMX_SIG;        \
    X void gram_x_kernel<NT, false, false> TRMF_GRAMX_SIG;
#define TRMF_LOSS_SIG (const uint32_t *, const uint32_t *, const real *, const real *, const real *, double *, uint32_t, uint32_t, uint32_t)
#define TRMF_UNIT_GRAM(X)                                                                                                    \
    TRMF_FSOLVE_ONE(X, 1, 8) TRMF_FSOLVE_ONE(X, 1, 16) TRMF_FSOLVE_ONE(X, 2, 24) TRMF_FSOLVE_ONE(X, 2, 32)                   \
    TRMF_FSOLVE_ONE(X, 3, 40) TRMF_FSOLVE_ONE(X, 3, 48) TRMF_FSOLVE_ONE(X, 4, 56) TRMF_FSOLVE_ONE(X, 4, 64)                  \
    TRMF_GRAMX_NT(X, 1) TRMF_GRAMX_NT(X, 2) TRMF_GRAMX_NT(X, 3) TRMF_GRAMX_NT(X, 4)                                         \
    X void loss_kernel<1> TRMF_LOSS_SIG; X void loss_kernel<2> TRMF_LOSS_SIG; X void loss_kernel<3> TRMF_LOSS_SIG; X void loss_kernel<4> TRMF_LOSS_SIG;

// the full-observation path's MFMA kernels (full_kernels.hpp).  On their own they compile in seconds; in one module with the
// non-template kernels of cg_kernels.hpp / generic_kernels.hpp LLVM's CodeGenPrepare spent 175 s of the main unit's 180 s.
#define TRMF_APPLY_SHARED_SIG (XParams, const XState *, int, const real *, const real *, const real *, const real *, const real *, int, real *, int, double *, int, int, int)
#define TRMF_FULL_NT(X, NT)                                                                                                              \
    X void spmm_rows_kernel<NT>(const uint32_t *, const uint32_t *, const real *, const real *, real *, uint32_t, uint32_t, uint32_t, uint32_t);  \
    X void spmm_part_kernel<NT>(const uint32_t *, const real *, const real *, const uint32_t *, uint32_t, uint32_t, real *, uint32_t);  \
    X void dense_tn_mfma_kernel<NT>(const real *, int, int, const real *, double *);                                                    \
    X void small_gram_mfma_kernel<NT>(const real *, int, int, double *);                                                                \
    X void chol_wave_kernel<NT>(const real *, real *, int);                                                                             \
    X void apply_shared_mfma_kernel<NT> TRMF_APPLY_SHARED_SIG;
#define TRMF_UNIT_FULL(X) TRMF_FULL_NT(X, 1) TRMF_FULL_NT(X, 2) TRMF_FULL_NT(X, 3) TRMF_FULL_NT(X, 4)

// held-out evaluation (heldout_kernels.hpp): NT = 1..4 for k <= 64, NT = 0 the generic instantiation for 64 < k <= 1024
#define TRMF_UNIT_HELDOUT(X)                                                                                                 \
    X void heldout_eval_kernel<0>(HeldoutArgs); X void heldout_eval_kernel<1>(HeldoutArgs); X void heldout_eval_kernel<2>(HeldoutArgs); \
    X void heldout_eval_kernel<3>(HeldoutArgs); X void heldout_eval_kernel<4>(HeldoutArgs);

// forecasting (forecast_kernels.hpp): the score kernel as NT = 1..4 for k <= 64 and NT = 0 for 64 < k <= 1024.  The roll-out is
// not a template: its body is compiled where TRMF_UNIT_BODIES is defined, i.e. by unit_forecast.hip alone among the units.
#define TRMF_UNIT_FORECAST(X)                                                                                                \
    X void forecast_score_kernel<0>(ScoreArgs); X void forecast_score_kernel<1>(ScoreArgs); X void forecast_score_kernel<2>(ScoreArgs); \
    X void forecast_score_kernel<3>(ScoreArgs); X void forecast_score_kernel<4>(ScoreArgs);

// online updates (online_kernels.hpp): the factor kernel as NT = 1..4 (k <= 64); the chain and the error kernel are not templates
#define TRMF_UNIT_ONLINE(X)                                                                                                  \
    X void assim_factor_kernel<1>(AssimFactorArgs); X void assim_factor_kernel<2>(AssimFactorArgs);                          \
    X void assim_factor_kernel<3>(AssimFactorArgs); X void assim_factor_kernel<4>(AssimFactorArgs);

// robust online updates (robust_kernels.hpp): the part and the solve kernel as NT = 1..4 (k <= 64); the prior kernel is not a template
#define TRMF_UNIT_ROBUST(X)                                                                                                  \
    X void assim_robust_part_kernel<1>(AssimRobustArgs); X void assim_robust_part_kernel<2>(AssimRobustArgs);                \
    X void assim_robust_part_kernel<3>(AssimRobustArgs); X void assim_robust_part_kernel<4>(AssimRobustArgs);                \
    X void assim_robust_solve_kernel<1>(AssimRobustArgs); X void assim_robust_solve_kernel<2>(AssimRobustArgs);              \
    X void assim_robust_solve_kernel<3>(AssimRobustArgs); X void assim_robust_solve_kernel<4>(AssimRobustArgs);

// forecast uncertainty (uncertainty_kernels.hpp): the residual pass and the dist kernel as NT = 1..4 (k <= 64) and NT = 0
// (64 < k <= 1024); the other kernels are not templates
#define TRMF_UNIT_UNCERTAINTY(X)                                                                                             \
    X void noise_resid_kernel<0>(NoiseResidArgs); X void noise_resid_kernel<1>(NoiseResidArgs); X void noise_resid_kernel<2>(NoiseResidArgs); \
    X void noise_resid_kernel<3>(NoiseResidArgs); X void noise_resid_kernel<4>(NoiseResidArgs);                              \
    X void forecast_dist_kernel<0>(DistArgs); X void forecast_dist_kernel<1>(DistArgs); X void forecast_dist_kernel<2>(DistArgs); \
    X void forecast_dist_kernel<3>(DistArgs); X void forecast_dist_kernel<4>(DistArgs);

// online loading updates (adapt_kernels.hpp): the per-series kernel and the init pass's part kernel as NT = 1..4 (k <= 64); the
// kernels of the full-observation forms are not templates
#define TRMF_UNIT_ADAPT(X)                                                                                                   \
    X void adapt_series_kernel<1>(AdaptArgs); X void adapt_series_kernel<2>(AdaptArgs);                                      \
    X void adapt_series_kernel<3>(AdaptArgs); X void adapt_series_kernel<4>(AdaptArgs);                                      \
    X void adapt_part_kernel<1>(AdaptArgs); X void adapt_part_kernel<2>(AdaptArgs);                                          \
    X void adapt_part_kernel<3>(AdaptArgs); X void adapt_part_kernel<4>(AdaptArgs);

// robust smoother (smooth_robust_kernels.hpp): the part and the fold kernel as NT = 1..4 (k <= 64)
#define TRMF_UNIT_SMOOTH_ROBUST(X)                                                                                           \
    X void smooth_robust_part_kernel<1>(SmoothRobustArgs); X void smooth_robust_part_kernel<2>(SmoothRobustArgs);            \
    X void smooth_robust_part_kernel<3>(SmoothRobustArgs); X void smooth_robust_part_kernel<4>(SmoothRobustArgs);            \
    X void smooth_robust_fold_kernel<1>(SmoothRobustArgs); X void smooth_robust_fold_kernel<2>(SmoothRobustArgs);            \
    X void smooth_robust_fold_kernel<3>(SmoothRobustArgs); X void smooth_robust_fold_kernel<4>(SmoothRobustArgs);

// robust online loading updates (adapt_robust_kernels.hpp): the per-series kernel as NT = 1..4 (k <= 64); the objective kernel is not a template
#define TRMF_UNIT_ADAPT_ROBUST(X)                                                                                            \
    X void adapt_robust_series_kernel<1>(AdaptRobustArgs); X void adapt_robust_series_kernel<2>(AdaptRobustArgs);            \
    X void adapt_robust_series_kernel<3>(AdaptRobustArgs); X void adapt_robust_series_kernel<4>(AdaptRobustArgs);

// sliding window (slide_kernels.hpp): the downdate of the loading statistics as NT = 1..4 (k <= 64); the compaction kernels are not templates
#define TRMF_UNIT_SLIDE(X)                                                                                                   \
    X void series_downdate_kernel<1>(DowndateArgs); X void series_downdate_kernel<2>(DowndateArgs);                          \
    X void series_downdate_kernel<3>(DowndateArgs); X void series_downdate_kernel<4>(DowndateArgs);

// cell revisions (revise_kernels.hpp): the update of the loading statistics as NT = 1..4 (k <= 64); the compaction and scatter kernels are not templates
#define TRMF_UNIT_REVISE(X)                                                                                                  \
    X void series_revise_kernel<1>(SeriesReviseArgs); X void series_revise_kernel<2>(SeriesReviseArgs);                      \
    X void series_revise_kernel<3>(SeriesReviseArgs); X void series_revise_kernel<4>(SeriesReviseArgs);

#define TRMF_DEFINE_KERNEL template __global__

}  // namespace trmf
