// Batched forward rollout of returned controls through the continuous dynamics (nlot_rollout_batch,
// include/nlot.h) for gfx950: the C entry point and its dispatch.  The kernel is k_roll<D, G, OpenLoop> of
// nlot_roll.h, which nlot_track_batch (nlot_track.hip) instantiates with its feedback law; the problem checks are
// check_problem / check_sample_count (nlot_internal.h).  DESIGN.md §11.
#include "nlot_roll.h"

extern "C" void nlot_default_rollout_options(NlotRolloutOptions* opt) {
    if (!opt) return;
    opt->substeps = 8;
    opt->edge_points = 3;
    opt->clearance_min = 0.0;
    opt->deviation_tol = INFINITY;
    opt->goal_tol = INFINITY;
}

extern "C" int32_t nlot_rollout_batch(const NlotProblem* prob, const NlotRolloutOptions* opt, const double* X,
                                      const double* U, const double* xg, double* X_roll, double* clearance,
                                      int32_t* where, double* deviation, int32_t* dev_where, double* goal_error,
                                      int32_t* flags, int64_t B, void* stream) {
    using namespace nlot;
    if (!prob || !opt) {
        set_error("nlot_rollout_batch: null problem or options");
        return NLOT_ERR_INVALID;
    }
    if (opt->substeps < 1) {
        set_error("nlot_rollout_batch: substeps must be >= 1");
        return NLOT_ERR_INVALID;
    }
    if (opt->edge_points < 0) {
        set_error("nlot_rollout_batch: edge_points must be >= 0");
        return NLOT_ERR_INVALID;
    }
    if (!check_problem(prob, B, "nlot_rollout_batch") ||
        !check_sample_count(prob, opt->substeps, opt->edge_points, "nlot_rollout_batch", "substeps"))
        return NLOT_ERR_INVALID;
    if (!X || !U || !clearance || !where || !deviation || !dev_where || !goal_error || !flags) {
        set_error("nlot_rollout_batch: null pointer");
        return NLOT_ERR_INVALID;
    }
    const OpenLoop a{opt->substeps, opt->edge_points, opt->clearance_min, opt->deviation_tol, opt->goal_tol, X, U, xg,
                     X_roll, clearance, where, deviation, dev_where, goal_error, flags, B};
    hipStream_t st = (hipStream_t)stream;
    return with_device_problem(prob, st, [&](const NlotProblem* dP) {
        dispatch_dynamics(prob->dynamics, [&](auto d) { launch_roll<decltype(d)::value>(prob, dP, a, st); });
    });
}
