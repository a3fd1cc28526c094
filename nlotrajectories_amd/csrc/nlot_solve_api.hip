// The solver's C ABI: input validation, workspace sizes, the dispatch of nlot_solve_batch to the instantiation of
// run<>() for the problem's dynamics model and integrator (compiled in the units of nlot_solver.hip), and the
// statistics of the last call.  No kernel is compiled here.
#include "nlot_solver_ws.h"

namespace nlot {

thread_local NlotSolveStats g_stats;
int g_timing = 0;  // nlot_set_timing: 0 off; k: one step in each group of k, at position (step / k) % k (rotating)

static int validate(const NlotProblem* p, const NlotSolverOptions* o, const NlotMlp* mlp, int64_t B) {
    if (!p || !o) { set_error("null problem/options"); return NLOT_ERR_INVALID; }
    static const int NXS[6] = {4, 4, 3, 5, 4, 7};
    if (p->dynamics < 0 || p->dynamics > 5 || p->nx != NXS[p->dynamics] || p->nu != 2) {
        set_error("dynamics / nx / nu mismatch");
        return NLOT_ERR_INVALID;
    }
    if (p->N < 2 || p->N > 4096 || p->dt <= 0) { set_error("N must be in [2, 4096], dt > 0"); return NLOT_ERR_INVALID; }
    if (o->general_bounds != 0 && o->general_bounds != 1) {
        set_error("general_bounds: 0 variable bounds, 1 constraint rows (CasADi Opti's form)");
        return NLOT_ERR_INVALID;
    }
    if (p->integrator != NLOT_INTEG_EULER && p->integrator != NLOT_INTEG_RK4) {
        set_error("integrator must be NLOT_INTEG_EULER or NLOT_INTEG_RK4"); return NLOT_ERR_INVALID;
    }
    if (p->shape == NLOT_SHAPE_POLYGON && (p->n_body < 1 || p->n_body > MMAX)) {
        set_error("polygon footprint: 1..4 corners"); return NLOT_ERR_INVALID;
    }
    if (p->shape == NLOT_SHAPE_POLYGON && p->nx < 3) { set_error("polygon footprint needs a heading state"); return NLOT_ERR_INVALID; }
    if (p->sdf_kind == NLOT_SDF_MLP && !mlp) { set_error("learned SDF requires an NlotMlp"); return NLOT_ERR_INVALID; }
    if (p->sdf_kind == NLOT_SDF_ANALYTIC && (p->n_obs < 1 || p->n_obs > NLOT_MAX_OBS)) {
        set_error("analytic SDF needs 1..NLOT_MAX_OBS (128) obstacles"); return NLOT_ERR_INVALID;
    }
    if (p->sdf_kind == NLOT_SDF_ANALYTIC) {
        if (p->n_verts < 0 || p->n_verts > NLOT_MAX_VERTS) { set_error("n_verts out of range"); return NLOT_ERR_INVALID; }
        for (int i = 0; i < p->n_obs; ++i) {
            const NlotObstacle& q = p->obs[i];
            if (q.type < NLOT_OBS_CIRCLE || q.type > NLOT_OBS_TRAPEZOID) { set_error("unknown obstacle type"); return NLOT_ERR_INVALID; }
            const bool poly = q.type == NLOT_OBS_POLYGON || q.type == NLOT_OBS_TRAPEZOID;
            if (poly && (q.nv < (q.type == NLOT_OBS_TRAPEZOID ? 4 : 2) || (q.type == NLOT_OBS_TRAPEZOID && q.nv != 4) ||
                         q.v0 < 0 || q.v0 + q.nv > p->n_verts)) {
                set_error("polygon / trapezoid obstacle: vertex range outside verts[0, n_verts) (a trapezoid has 4)");
                return NLOT_ERR_INVALID;
            }
        }
    }
    for (int i = 0; i < p->nu; ++i)
        if (!(p->umin[i] < p->umax[i])) { set_error("control bounds must satisfy min < max"); return NLOT_ERR_INVALID; }
    if (o->max_iter < 0 || o->max_iter > 10000000) { set_error("max_iter must be in [0, 1e7]"); return NLOT_ERR_INVALID; }
    if (o->resto && (o->resto_penalty_parameter <= 0 || o->required_infeasibility_reduction <= 0 ||
                     o->required_infeasibility_reduction >= 1 || o->resto_proximity_weight < 0)) {
        set_error("restoration options: rho > 0, 0 < kappa_resto < 1, proximity weight >= 0");
        return NLOT_ERR_INVALID;
    }
    if (o->max_soc < 0 || o->watchdog_shortened_iter_trigger < 0 || o->watchdog_trial_iter_max < 0) {
        set_error("max_soc / watchdog options must be >= 0");
        return NLOT_ERR_INVALID;
    }
    if (o->mu_strategy != 0 && o->mu_strategy != 1) { set_error("mu_strategy: 0 monotone, 1 adaptive"); return NLOT_ERR_INVALID; }
    if (B <= 0 || B > (int64_t)1 << 26) { set_error("B out of range"); return NLOT_ERR_INVALID; }
    return NLOT_OK;
}
}  // namespace nlot

extern "C" size_t nlot_solve_workspace_size(const NlotProblem* p, int64_t B) {
    if (!p) return 0;
    nlot::Dims d = nlot::make_dims(*p);
    return nlot::ws_bytes(d, B, p->sdf_kind == NLOT_SDF_MLP);
}
extern "C" size_t nlot_solve_workspace_size_slots(const NlotProblem* p, int64_t B, int32_t max_active) {
    return nlot_solve_workspace_size(p, nlot::slot_count(B, max_active));
}

extern "C" int32_t nlot_solve_batch(const NlotProblem* p, const NlotSolverOptions* o, const NlotMlp* mlp,
                                    const double* x0, const double* xg, const double* Xinit, double* X, double* U,
                                    double* S, double* cost, int32_t* status, int32_t* iters, int64_t B,
                                    void* workspace, size_t wbytes, void* stream) {
    using namespace nlot;
    int rc = validate(p, o, mlp, B);
    if (rc) return rc;
    if (!x0 || !xg || !X || !U || !cost || !status || !iters || !workspace) {
        set_error("nlot_solve_batch: null pointer");
        return NLOT_ERR_INVALID;
    }
    if (wbytes < nlot_solve_workspace_size_slots(p, B, o->max_active)) {
        set_error("nlot_solve_batch: workspace too small");
        return NLOT_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    // the dynamics model and the integrator select the instantiation (Euler: DYN; RK4: DYN + NLOT_RK4_BIAS)
    const int dyn = p->dynamics + (p->integrator == NLOT_INTEG_RK4 ? NLOT_RK4_BIAS : 0);
#define NLOT_RUN(D) return run<D>(*p, *o, mlp, x0, xg, Xinit, X, U, S, cost, status, iters, B, workspace, st)
#ifdef NLOT_ONLY_DYN  // kernel-tuning builds (make tune): the one instantiation
    if (dyn == NLOT_ONLY_DYN) NLOT_RUN(NLOT_ONLY_DYN);
    set_error("tuning build (NLOT_ONLY_DYN): this dynamics model is not compiled in");
    return NLOT_ERR_INVALID;
#else
    switch (dyn) {
    case NLOT_POINT_1ST: NLOT_RUN(NLOT_POINT_1ST);
    case NLOT_POINT_2ND: NLOT_RUN(NLOT_POINT_2ND);
    case NLOT_UNICYCLE: NLOT_RUN(NLOT_UNICYCLE);
    case NLOT_UNICYCLE_2ND: NLOT_RUN(NLOT_UNICYCLE_2ND);
    case NLOT_ACKERMANN: NLOT_RUN(NLOT_ACKERMANN);
    case NLOT_ACKERMANN_2ND: NLOT_RUN(NLOT_ACKERMANN_2ND);
    case NLOT_POINT_1ST + NLOT_RK4_BIAS: NLOT_RUN(NLOT_POINT_1ST + NLOT_RK4_BIAS);
    case NLOT_POINT_2ND + NLOT_RK4_BIAS: NLOT_RUN(NLOT_POINT_2ND + NLOT_RK4_BIAS);
    case NLOT_UNICYCLE + NLOT_RK4_BIAS: NLOT_RUN(NLOT_UNICYCLE + NLOT_RK4_BIAS);
    case NLOT_UNICYCLE_2ND + NLOT_RK4_BIAS: NLOT_RUN(NLOT_UNICYCLE_2ND + NLOT_RK4_BIAS);
    case NLOT_ACKERMANN + NLOT_RK4_BIAS: NLOT_RUN(NLOT_ACKERMANN + NLOT_RK4_BIAS);
    case NLOT_ACKERMANN_2ND + NLOT_RK4_BIAS: NLOT_RUN(NLOT_ACKERMANN_2ND + NLOT_RK4_BIAS);
    }
    set_error("unknown dynamics");
    return NLOT_ERR_INVALID;
#endif
#undef NLOT_RUN
}

extern "C" void nlot_set_timing(int32_t every) { nlot::g_timing = every > 0 ? every : 0; }
extern "C" void nlot_last_stats(NlotSolveStats* out) {
    if (out) *out = nlot::g_stats;
}
