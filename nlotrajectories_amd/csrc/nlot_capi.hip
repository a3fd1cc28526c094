// C-ABI plumbing of libnlot.so: version, thread-local errors, the problem checks the measurement entry points share
// (check_problem, check_sample_count of nlot_internal.h), defaults, and the CasADi external
// compatibility shim (gen/nn_sdf.cpp:36-104 signatures).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>

#include "nlot_internal.h"

namespace nlot {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

bool check_problem(const NlotProblem* prob, int64_t B, const char* who) {
    static const int kNx[6] = {4, 4, 3, 5, 4, 7};
    const std::string w(who);
    if (prob->dynamics < 0 || prob->dynamics > NLOT_ACKERMANN_2ND || prob->nx != kNx[prob->dynamics] || prob->nu != 2 ||
        prob->N < 1 || prob->N > 1 << 24 || prob->n_obs < 0 || prob->n_obs > NLOT_MAX_OBS || prob->n_verts < 0 ||
        prob->n_verts > NLOT_MAX_VERTS || (prob->shape != NLOT_SHAPE_DOT && prob->shape != NLOT_SHAPE_POLYGON) ||
        (prob->shape == NLOT_SHAPE_POLYGON && (prob->n_body < 1 || prob->n_body > NLOT_MAX_BODY))) {
        set_error(w + ": invalid problem (dynamics, nx / nu, 1 <= N <= 2^24, shape, n_body, n_obs, n_verts)");
        return false;
    }
    for (int i = 0; i < prob->n_obs; ++i) {
        const NlotObstacle& q = prob->obs[i];
        if (q.type < NLOT_OBS_CIRCLE || q.type > NLOT_OBS_TRAPEZOID) {
            set_error(w + ": unknown obstacle type");
            return false;
        }
        if ((q.type == NLOT_OBS_POLYGON || q.type == NLOT_OBS_TRAPEZOID) &&
            (q.v0 < 0 || q.nv < 2 || q.v0 > prob->n_verts - q.nv)) {
            set_error(w + ": polygon vertex range outside verts[0, n_verts)");
            return false;
        }
    }
    if (B < 1 || B > (int64_t)1 << 26) {
        set_error(w + ": B out of range");
        return false;
    }
    return true;
}

bool check_sample_count(const NlotProblem* prob, int substeps, int edge_points, const char* who, const char* name) {
    // the kernels count poses, footprint points and (k_verify) their product with ints
    const int64_t P = (int64_t)prob->N * substeps + 1;
    const int64_t npp = prob->shape == NLOT_SHAPE_POLYGON ? (int64_t)prob->n_body * (1 + (int64_t)edge_points) : 1;
    if (P > INT32_MAX || npp > INT32_MAX || P * npp > INT32_MAX - 64) {
        set_error(std::string(who) + ": sample count (N " + name + " + 1) * n_body (1 + edge_points) overflows int32");
        return false;
    }
    return true;
}
}  // namespace nlot

extern "C" int32_t nlot_abi_version(void) { return NLOT_ABI_VERSION; }
extern "C" const char* nlot_last_error(void) { return nlot::g_err.c_str(); }

extern "C" void nlot_default_options(NlotSolverOptions* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->tol = 1e-4;               // runner.py:118
    o->max_iter = 1000;          // runner.py:117
    o->mu_strategy = 1;          // adaptive + quality-function oracle (runner.py:118-119)
    o->mu_init = 0.1;
    o->barrier_tol_factor = 0.05;  // runner.py:120
    o->dual_inf_tol = 1.0;
    o->constr_viol_tol = 1e-4;
    o->compl_inf_tol = 1e-4;
    o->constr_mult_init_max = 1e3;
    o->bound_push = 1e-2;
    o->bound_frac = 1e-2;
    o->max_soc = 4;                          // IPOPT defaults from here on
    o->resto = 1;
    o->watchdog_shortened_iter_trigger = 10;
    o->watchdog_trial_iter_max = 3;
    o->max_soft_resto_iters = 10;
    o->kappa_soc = 0.99;
    o->tiny_step_tol = 10 * 2.220446049250313e-16;
    o->tiny_step_y_tol = 1e-2;
    o->soft_resto_pderror_reduction_factor = 0.9999;
    o->required_infeasibility_reduction = 0.9;
    o->resto_penalty_parameter = 1000.0;
    o->resto_proximity_weight = 1.0;
    o->bound_mult_reset_threshold = 1000.0;
    o->resto_failure_feasibility_threshold = 0.0;
    o->general_bounds = 1;  // opti.bounded / subject_to(slack >= 0) as constraint rows (runner.py:67-69,101-103)
}

// ------------------------------------------------------------------------------------------------
// CasADi external shim.  gen/nn_sdf.cpp:3 constructs ONE static global L4CasADi model at dlopen; the
// equivalent here is the model bound by nlot_casadi_bind.  Each call evaluates one 1x2 point (the
// sparsity of gen/nn_sdf.cpp:36-37) on the GPU synchronously; CasADi owns arg/res (host doubles).
// ------------------------------------------------------------------------------------------------
namespace {
const NlotMlp* g_bound = nullptr;  // cleared by nlot_mlp_destroy (casadi_unbind)
int g_bound_dev = 0;               // device the bound model lives on
std::mutex g_mu;
float* g_dev[64] = {};  // per device: [0..1] point, [2] lam, [3] val, [4..5] grad, [6..9] hess
const casadi_int_t s_in0[3] = {1, 2, 1};
const casadi_int_t s_out0[3] = {1, 1, 1};

int shim_eval(const double* x, const double* adj, double* val, double* grad, double* hess) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_bound) {
        nlot::set_error("nn_sdf: no model bound (nlot_casadi_bind)");
        return 1;
    }
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(g_bound_dev) != hipSuccess) return 1;
    struct Restore {
        int d;
        ~Restore() { (void)hipSetDevice(d); }
    } restore{prev};
    float*& scratch = g_dev[g_bound_dev & 63];
    if (!scratch && hipMalloc(&scratch, 16 * sizeof(float)) != hipSuccess) return 1;
    float* g_dev = scratch;
    float h[16] = {0};
    h[0] = (float)x[0];  // CasADi double -> fp32, as the TorchScript graph requires
    h[1] = (float)x[1];
    h[2] = adj ? (float)adj[0] : 1.f;
    if (hipMemcpy(g_dev, h, 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 1;
    bool full = grad || hess;
    if (nlot_sdf_mlp_eval(g_bound, g_dev, 1, g_dev + 3, full ? g_dev + 4 : nullptr, full ? g_dev + 2 : nullptr,
                          hess ? g_dev + 6 : nullptr, nullptr) != NLOT_OK)
        return 1;
    if (hipMemcpy(h + 3, g_dev + 3, 7 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (val) val[0] = h[3];
    if (grad) {
        grad[0] = h[4];
        grad[1] = h[5];
    }
    if (hess) /* column-major 2x2 (symmetric) */
        for (int i = 0; i < 4; ++i) hess[i] = h[6 + i];
    return 0;
}
}  // namespace

extern "C" int32_t nlot_casadi_bind(const NlotMlp* mlp) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_bound = mlp;
    g_bound_dev = mlp ? mlp->device : 0;
    return NLOT_OK;
}

void nlot::casadi_unbind(const NlotMlp* m) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_bound == m) g_bound = nullptr;
}

extern "C" casadi_int_t nn_sdf_n_in(void) { return 1; }
extern "C" casadi_int_t nn_sdf_n_out(void) { return 1; }
extern "C" const casadi_int_t* nn_sdf_sparsity_in(casadi_int_t i) { return i == 0 ? s_in0 : nullptr; }
extern "C" const casadi_int_t* nn_sdf_sparsity_out(casadi_int_t i) { return i == 0 ? s_out0 : nullptr; }
extern "C" int nn_sdf(const casadi_real_t** arg, casadi_real_t** res, casadi_int_t*, casadi_real_t*, int) {
    return shim_eval(arg[0], nullptr, res[0], nullptr, nullptr);
}
// jac [i0, out_o0] -> [jac_o0_i0]  (gen/nn_sdf.cpp:64-70)
extern "C" casadi_int_t jac_nn_sdf_n_in(void) { return 2; }
extern "C" casadi_int_t jac_nn_sdf_n_out(void) { return 1; }
extern "C" int jac_nn_sdf(const casadi_real_t** arg, casadi_real_t** res, casadi_int_t*, casadi_real_t*, int) {
    double v;
    return shim_eval(arg[0], nullptr, &v, res[0], nullptr);
}
// adj1 [i0, out_o0, adj_o0] -> [out_adj_i0]  (gen/nn_sdf.cpp:76-83)
extern "C" casadi_int_t adj1_nn_sdf_n_in(void) { return 3; }
extern "C" casadi_int_t adj1_nn_sdf_n_out(void) { return 1; }
extern "C" int adj1_nn_sdf(const casadi_real_t** arg, casadi_real_t** res, casadi_int_t*, casadi_real_t*, int) {
    double v;
    return shim_eval(arg[0], arg[2], &v, res[0], nullptr);
}
// jac_adj1 [i0, out_o0, adj_o0, out_adj_i0] -> [jac_adj_i0_i0, -, -]  (gen/nn_sdf.cpp:88-104):
// only res[0] is provided, exactly like the generated file (which throws; this returns 1).
extern "C" casadi_int_t jac_adj1_nn_sdf_n_in(void) { return 4; }
extern "C" casadi_int_t jac_adj1_nn_sdf_n_out(void) { return 3; }
extern "C" int jac_adj1_nn_sdf(const casadi_real_t** arg, casadi_real_t** res, casadi_int_t*, casadi_real_t*, int) {
    if (res[1] != nullptr || res[2] != nullptr || res[0] == nullptr) {
        nlot::set_error("jac_adj1_nn_sdf: only jac_adj_i0_i0 is provided (as in L4CasADi)");
        return 1;
    }
    double v, g[2];
    return shim_eval(arg[0], arg[2], &v, g, res[0]);
}
