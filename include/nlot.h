/*
 * nlot.h — C ABI of the MI355X-native batched trajectory optimiser (libnlot.so).
 *
 * This is the drop-in boundary for the reference's NLP constraint-evaluation hot path
 * (SURVEY.md §8b).  Everything is plain C: POD structs, caller-owned pointers, int return codes,
 * an explicit hipStream_t passed as void*, no exceptions and no global mutable state on the
 * compute entry points (each call uses only its arguments and the caller's workspace).
 *
 * Replaced reference interfaces (file:line under /root/reference):
 *   nlot_sdf_mlp_eval        <- gen/nn_sdf.cpp:57-60  nn_sdf        (value)
 *                               gen/nn_sdf.cpp:67-70  jac_nn_sdf    (gradient)
 *                               gen/nn_sdf.cpp:79-83  adj1_nn_sdf   (lambda * gradient)
 *                               gen/nn_sdf.cpp:91-104 jac_adj1_nn_sdf (lambda * Hessian)
 *                           batched over P points on the device instead of one 1x2 point per call.
 *   nlot_solve_batch         <- src/nlotrajectories/core/runner.py:44-153 RunBenchmark.run
 *                               (NLP of runner.py:46-108 solved by CasADi Opti + IPOPT,
 *                               runner.py:113-133) for B independent start/goal instances.
 *   nn_sdf / jac_nn_sdf / adj1_nn_sdf / jac_adj1_nn_sdf and their _n_in/_n_out/_sparsity_*
 *                            <- gen/nn_sdf.cpp:36-104, same CasADi external signatures, served by
 *                               the model bound with nlot_casadi_bind (host buffers, like CasADi).
 */
#ifndef NLOT_H
#define NLOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLOT_ABI_VERSION 19

/* ---- error codes ------------------------------------------------------------------------- */
#define NLOT_OK 0
#define NLOT_ERR_INVALID -1    /* bad argument / unsupported configuration */
#define NLOT_ERR_HIP -2        /* HIP runtime error */
#define NLOT_ERR_WORKSPACE -3  /* workspace too small */

/* ---- per-problem solve status (output array `status`) ----------------------------------- */
#define NLOT_SOLVED 0             /* IPOPT "Solve_Succeeded" analogue: E_0 <= tol + abs. tols */
#define NLOT_MAXITER 1            /* max_iter reached (IPOPT Maximum_Iterations_Exceeded)     */
#define NLOT_LS_FAILED 2          /* alpha < alpha_min with restoration switched off (opt.resto = 0) */
#define NLOT_NUMERIC 3            /* non-finite values / inertia correction failed            */
#define NLOT_RESTO_FAILED 4       /* IPOPT Restoration_Failed: restoration line search failed, or it
                                     converged to a feasible point the filter does not accept  */
#define NLOT_INFEASIBLE 5         /* IPOPT Infeasible_Problem_Detected (restoration converged to a
                                     point of local infeasibility)                              */
#define NLOT_TINY_STEP 6          /* IPOPT Search_Direction_Becomes_Too_Small                  */

/* ---- dynamics (core/dynamics.py:7-13, DYNAMICS_CLASS_MAP 151-158) ------------------------ */
enum NlotDynamics {
    NLOT_POINT_1ST = 0,   /* PointMass1stOrder  dynamics.py:33-41  nx=4 nu=2 */
    NLOT_POINT_2ND = 1,   /* PointMass2ndOrder  dynamics.py:44-56  nx=4 nu=2 */
    NLOT_UNICYCLE = 2,    /* Unicycle           dynamics.py:59-73  nx=3 nu=2 */
    NLOT_UNICYCLE_2ND = 3,/* Unicycle2ndOrder   dynamics.py:76-96  nx=5 nu=2 */
    NLOT_ACKERMANN = 4,   /* Ackermann          dynamics.py:99-118 nx=4 nu=2 */
    NLOT_ACKERMANN_2ND = 5/* Ackermann2ndOrder  dynamics.py:121-148 nx=7 nu=2 (vector order as-is) */
};

/* ---- robot geometry (core/geometry.py) --------------------------------------------------- */
enum NlotShape {
    NLOT_SHAPE_DOT = 0,     /* DotGeometry geometry.py:59-70: sdf(x,y) >= 0, slack ignored      */
    NLOT_SHAPE_POLYGON = 1  /* PolygonGeometry geometry.py:73-117 (rectangle 125-135, triangle
                               138-144): soft-min over corners + slack, or per-corner >= 0       */
};

/* ---- analytic obstacles (core/sdf/casadi.py) ---------------------------------------------- */
enum NlotObstacleType {
    NLOT_OBS_CIRCLE = 0,    /* CircleObstacle.approximated_sdf casadi.py:33-41 */
    NLOT_OBS_SQUARE = 1,    /* SquareObstacle.approximated_sdf casadi.py:69-118 */
    NLOT_OBS_POLYGON = 2,   /* PolygonObstacle.approximated_sdf casadi.py:150-186 (EllipticRingObstacle
                               casadi.py:193-248 is a polygon of its arc points); (cx, cy) = centroid */
    NLOT_OBS_TRAPEZOID = 3  /* TrapezoidObstacle.approximated_sdf casadi.py:317-374 (4 vertices) */
};

enum NlotIntegrator {
    NLOT_INTEG_EULER = 0, /* x_{k+1} = x_k + dt f(x_k, u_k), runner.py:62-63 */
    NLOT_INTEG_RK4 = 1    /* x_{k+1} = x_k + dt (k1 + 2 k2 + 2 k3 + k4) / 6 (opt-in, non-parity) */
};

enum NlotSdfKind {
    NLOT_SDF_ANALYTIC = 0, /* MultiObstacle.approximated_sdf casadi.py:385-386 (soft_min union) */
    NLOT_SDF_MLP = 1       /* NNObstacle.approximated_sdf l4casadi.py:241-257 (learned)         */
};

#define NLOT_MAX_OBS 128   /* primitive obstacles (a discr_s of 30 arc points is 58 trapezoids) */
#define NLOT_MAX_VERTS 512 /* polygon / trapezoid vertices of all obstacles */
#define NLOT_MAX_BODY 8
#define NLOT_MAX_NU 4

typedef struct NlotObstacle {
    int32_t type;      /* NlotObstacleType */
    int32_t group;     /* -1: a term of the scene's soft_min; g >= 0: consecutive obstacles of group g are first
                          soft_min'ed together (a MultiObstacle inside the scene: ConvexEllipticRing casadi.py:393-445,
                          ConvexSObstacle casadi.py:448-525), and that value is the scene's term */
    int32_t v0, nv;    /* polygon / trapezoid: vertices verts[v0 .. v0 + nv) in the reference's point order */
    double cx, cy;     /* circle / square: center; polygon: centroid (mean of the points, casadi.py:133) */
    double size;       /* circle: radius; square: side length */
    double margin;
} NlotObstacle;

/* One NLP of runner.py:44-108 (all B instances share it; start/goal differ per instance). */
typedef struct NlotProblem {
    int32_t dynamics;        /* NlotDynamics */
    int32_t shape;           /* NlotShape */
    int32_t nx, nu;          /* must match the dynamics */
    int32_t n_body;          /* polygon corner count (rectangle 4, triangle 3) */
    int32_t N;               /* knots - 1 (solver.N) */
    double body[NLOT_MAX_BODY][2]; /* corners in body frame, geometry.py:125-144 order */
    double wheelbase;        /* Ackermann L */
    double dt;
    int32_t use_slack;       /* runner.py:66-69 */
    int32_t use_smooth;      /* runner.py:91-96 */
    double slack_penalty;    /* rho */
    double smooth_weight;    /* w */
    int32_t enforce_heading; /* runner.py:51-56 */
    int32_t sdf_kind;        /* NlotSdfKind */
    double umin[NLOT_MAX_NU], umax[NLOT_MAX_NU]; /* runner.py:101-103 */
    double softmin_alpha;    /* utils.py:18 alpha = 10 */
    double path_eps;         /* runner.py:81 epsilon = 1e-8 */
    int32_t n_obs;
    int32_t n_verts;
    NlotObstacle obs[NLOT_MAX_OBS];
    double verts[NLOT_MAX_VERTS][2];
    int32_t integrator;      /* NLOT_INTEG_EULER (the reference's defects, runner.py:62-63; default) or NLOT_INTEG_RK4
                                (opt-in classical RK4 step as the defect map; not the reference's NLP) */
    int32_t pad2_;
} NlotProblem;

/* IPOPT options (runner.py:113-125 + IPOPT defaults).  See DESIGN.md §4 for the restatement. */
typedef struct NlotSolverOptions {
    double tol;                  /* 1e-4 (runner.py:118) */
    int32_t max_iter;            /* 1000 (runner.py:117) */
    int32_t mu_strategy;         /* 0 = monotone (Fiacco-McCormick), 1 = adaptive with the quality-function
                                    oracle (the reference's setting, runner.py:118-119; default) */
    double mu_init;              /* 0.1 */
    double barrier_tol_factor;   /* kappa_eps (IPOPT default 10; the reference sets 0.05, runner.py:120) */
    double dual_inf_tol;         /* 1 */
    double constr_viol_tol;      /* 1e-4 */
    double compl_inf_tol;        /* 1e-4 */
    double constr_mult_init_max; /* 1e3 */
    double bound_push;           /* 1e-2 */
    double bound_frac;           /* 1e-2 */
    int32_t max_soc;             /* second-order corrections per iteration (IPOPT default 4) */
    int32_t resto;               /* 1: feasibility restoration phase on line-search failure (IPOPT) */
    int32_t watchdog_shortened_iter_trigger; /* 10 (IPOPT default; 0 switches the watchdog off) */
    int32_t watchdog_trial_iter_max;         /* 3 */
    int32_t max_soft_resto_iters;            /* 10 */
    int32_t max_active;          /* solver scheduling, not an IPOPT option: 0 = all B instances from the start;
                                    n > 0 = continuous batching, at most n instances in flight and the next ones
                                    admitted (in index order) as others finish — per-instance results are the same */
    double kappa_soc;                        /* 0.99 */
    double tiny_step_tol;                    /* 10 eps = 2.22e-15 */
    double tiny_step_y_tol;                  /* 1e-2 */
    double soft_resto_pderror_reduction_factor; /* 0.9999 (0 switches the soft restoration off) */
    double required_infeasibility_reduction; /* kappa_resto = 0.9 */
    double resto_penalty_parameter;          /* rho = 1000 */
    double resto_proximity_weight;           /* zeta = weight * sqrt(mu), weight 1 */
    double bound_mult_reset_threshold;       /* 1000 */
    double resto_failure_feasibility_threshold; /* 0 means 1e2 * tol (IPOPT default) */
    int32_t general_bounds;      /* 1 (default since ABI v12): the control bounds and slack >= 0 as constraint rows
                                    g(x) = U, g(x) = S with bounded IPOPT slacks, U and S free — the NLP CasADi Opti
                                    hands IPOPT (runner.py:67-69,101-103); 0: the same bounds as variable bounds */
    int32_t pad_gb_;
} NlotSolverOptions;

/* Learned SDF: an l4casadi-wrappable torch model, flattened.
 *   FourierMLP (core/nn_architectures.py:30-72):  h0 = scale * cos(p @ A + b0)         (in_kind 1)
 *   l4c.naive.MultiLayerPerceptron:              h0 = act(p @ A + b0)                  (in_kind 0)
 *   SIREN (core/nn_architectures.py:8-26,75-100): in_kind 0 with act = NLOT_ACT_SINE, fourier_scale = omega_0
 *   then n_hidden x  h_{l+1} = act(W_l h_l + b_l);   f = w_out . h + b_out.
 * ReLU nets run on the MFMA kernels (n_hidden 1-4); the smooth activations on the hyper-dual kernel
 * (value, gradient and Hessian propagated forward through every layer; n_hidden 0-4), DESIGN.md §7.
 * All weights fp32 (the reference's l4casadi path evaluates the TorchScript graph in fp32,
 * gen/nn_sdf.cpp casts the CasADi doubles to float).  Host OR device pointers depending on the
 * consumer (nlot_mlp_create copies host arrays to the device). */
#define NLOT_MLP_IN_LINEAR_RELU 0
#define NLOT_MLP_IN_FOURIER 1
/* activations (core/nn_architectures.py:47-52 names; l4casadi naive: ReLU/Tanh/Sigmoid/LeakyReLU) */
#define NLOT_ACT_RELU 0
#define NLOT_ACT_TANH 1
#define NLOT_ACT_SIGMOID 2
#define NLOT_ACT_LEAKY_RELU 3 /* negative slope 0.01 (F.leaky_relu / nn.LeakyReLU default) */
#define NLOT_ACT_SINE 4       /* sin(omega_0 z), SineLayer nn_architectures.py:8-26; omega_0 in fourier_scale */

typedef struct NlotMlpDesc {
    int32_t in_kind;       /* NLOT_MLP_IN_* */
    int32_t hidden;        /* H (multiple of 32, <= 256) */
    int32_t n_hidden;      /* hidden HxH layers (>= 0) */
    int32_t act;           /* NLOT_ACT_* of the hidden layers (and of the input layer when in_kind 0) */
    float fourier_scale;   /* FourierFeatureLayer.scale (in_kind 1); omega_0 when act = NLOT_ACT_SINE */
    float b_out;
    const float* A;        /* [2][H]  (in, out) */
    const float* b0;       /* [H] */
    const float* W;        /* [n_hidden][H][H]  (out, in) = nn.Linear.weight */
    const float* b;        /* [n_hidden][H] */
    const float* w_out;    /* [H] */
} NlotMlpDesc;

typedef struct NlotMlp NlotMlp; /* opaque device-resident weights */

/* ---- version / errors --------------------------------------------------------------------- */
int32_t nlot_abi_version(void);
/* Last error message of the calling thread (thread-local; never NULL). */
const char* nlot_last_error(void);
/* Fill `opt` with the defaults documented above. */
void nlot_default_options(NlotSolverOptions* opt);

/* ---- learned-SDF weights ------------------------------------------------------------------- */
/* Copies the host arrays of `desc` to device memory; returns NULL on error (see nlot_last_error). */
NlotMlp* nlot_mlp_create(const NlotMlpDesc* desc);
/* The net's MFMA arithmetic (ABI v13).  Both are fp32 arithmetic (products exact in the fp32 accumulator); they
 * differ in the MFMA sums' order and so at the rounding level:
 *   NLOT_MLP_ARITH_SPLIT_BF16  operands split into three bf16 parts, six bf16 MFMA products per fp32 product (the
 *                              default of nlot_mlp_create: 2.65x the f32-MFMA peak)
 *   NLOT_MLP_ARITH_F32         v_mfma_f32 products (the reference's fp32 net, gen/nn_sdf.cpp, at the f32 peak)
 *   NLOT_MLP_ARITH_SEQ         (ABI v15; ReLU nets) every sum a sequential fp32 FMA chain in index order, one thread per
 *                              point: a fixed, documented summation order (the test oracle's), for bitwise-reproducible
 *                              comparisons; not a throughput path */
#define NLOT_MLP_ARITH_SPLIT_BF16 0
#define NLOT_MLP_ARITH_F32 1
#define NLOT_MLP_ARITH_SEQ 2
NlotMlp* nlot_mlp_create_ex(const NlotMlpDesc* desc, int32_t arith);
void nlot_mlp_destroy(NlotMlp* mlp);

/* Batched SDF-MLP evaluation on the device (the nn_sdf family, gen/nn_sdf.cpp:57-104).
 *   pts  [P][2] fp32 device, row-major.   val [P] (required).
 *   grad [P][2] or NULL: df/dp.             lam [P] or NULL (NULL = 1): adjoint seed.
 *   hess [P][2][2] or NULL: lam * d2f/dp2 (jac_adj1).  When lam != NULL, grad is lam * df/dp (adj1).
 * `stream` is a hipStream_t (NULL = default stream). Asynchronous. */
int32_t nlot_sdf_mlp_eval(const NlotMlp* mlp, const float* pts, int64_t P, float* val, float* grad,
                          const float* lam, float* hess, void* stream);

/* ---- batched trajectory optimisation ------------------------------------------------------ */
/* Bytes of device workspace nlot_solve_batch needs for B instances. */
size_t nlot_solve_workspace_size(const NlotProblem* prob, int64_t B);
/* Bytes for B instances streamed through max_active slots (continuous batching, ABI v10): the workspace holds the
 * slots' state only, so it depends on min(B, max_active), not on B (max_active <= 0: all B at once). */
size_t nlot_solve_workspace_size_slots(const NlotProblem* prob, int64_t B, int32_t max_active);

/* Solve B independent instances of `prob` (start x0[b], goal xg[b]) on the device.
 *   x0, xg    [B][nx] fp64 device
 *   X_init    [B][N+1][nx] fp64 device, or NULL = LinearInitializer (trajectory_initialization.py:54-55)
 *   X         [B][N+1][nx] fp64 device (out)   U [B][N][nu] fp64 (out)   S [B][N+1] fp64 or NULL
 *   cost      [B] fp64 (out: objective value, runner.py:80-98 / run_benchmark.py:166)
 *   status    [B] int32 (out: NLOT_SOLVED ...)   iters [B] int32 (out)
 *   mlp       required iff prob->sdf_kind == NLOT_SDF_MLP
 *   workspace >= nlot_solve_workspace_size_slots(prob, B, opt->max_active) bytes of device memory (per-slot state;
 *             an instance writes its outputs when it finishes, and its slot goes to the next instance).
 * Returns when all instances finished (the host drives the iteration loop on `stream`). */
int32_t nlot_solve_batch(const NlotProblem* prob, const NlotSolverOptions* opt, const NlotMlp* mlp,
                         const double* x0, const double* xg, const double* X_init, double* X,
                         double* U, double* S, double* cost, int32_t* status, int32_t* iters,
                         int64_t B, void* workspace, size_t workspace_bytes, void* stream);

/* Per-solve counters of the last nlot_solve_batch on this thread (host side, for benchmarking). */
typedef struct NlotSolveStats {
    int32_t iterations;        /* lock-step iterations run */
    int32_t ls_rounds;         /* line-search rounds launched */
    int64_t mlp_points_full;   /* points evaluated with value+grad+hess */
    int64_t mlp_points_value;  /* points evaluated value-only (trial points) */
    double mlp_full_ms;        /* summed device time of the full MLP launches (hipEvents) */
    double mlp_value_ms;       /* summed device time of the value-only MLP launches */
    int32_t mlp_full_launches;
    int32_t mlp_value_launches;
    double iterate_ms;         /* summed device time of the solver-step (k_iterate) launches */
    int32_t slots_in_lds;      /* 1: Riccati stage slots held in LDS, 0: in the HBM workspace */
    int32_t pad_;
    int64_t mlp_points_full_reused; /* full-launch points whose forward came from the accepted trial point */
    double ric_ms;             /* summed device time of the Newton-solve (k_ric) launches (hipEvents) */
    int32_t ric_launches;
    int32_t pad2_;
    int64_t ric_solves;        /* instance Newton solves (factorisations) those launches performed */
    int64_t ric_soc_solves;    /* second-order corrections: substitutions with the stored factors (side stream) */
    int64_t ric_resto_solves;  /* restoration-phase Newton solves (side stream) */
    int32_t filter_capacity;   /* entries per filter (line search, adaptive-mu progress, restoration); ABI v11 */
    int32_t filter_peak;       /* the largest size any filter reached */
    int64_t filter_forgotten;  /* entries forgotten at capacity (IPOPT's filter is unbounded: 0 = faithful) */
    /* ABI v14: the *_ms sums above cover the timed global steps only (nlot_set_timing); these count them and the
     * work their launches did (one full MLP, one value MLP in up to two parts, one k_ric launch per step) */
    int32_t timed_steps;
    int32_t timing_every;
    int64_t timed_points_full;
    int64_t timed_points_full_reused;
    int64_t timed_points_value;
    int64_t timed_ric_solves;
} NlotSolveStats;
/* hipEvent timing of the MLP, solver-step and k_ric launches inside nlot_solve_batch: 0 off, 1 every global step,
 * k > 1 one step in each group of k consecutive steps, at the position (group index mod k) (a sample over every
 * position: each timed step adds ~10 event packets to the queue, ~2 % of the step time when every step is timed). */
void nlot_set_timing(int32_t every);
void nlot_last_stats(NlotSolveStats* out);

/* ---- CasADi external compatibility shim (gen/nn_sdf.cpp:36-104) ----------------------------
 * A CasADi user can `casadi.external("nn_sdf", "libnlot.so")` after binding a model.  These are
 * host functions on double buffers owned by CasADi, one 1x2 point per call, exactly like the
 * generated file; they run the MLP on the GPU synchronously.  Bind with nlot_casadi_bind (the
 * reference's static global L4CasADi object, gen/nn_sdf.cpp:3). */
typedef double casadi_real_t;
typedef long long int casadi_int_t;
int32_t nlot_casadi_bind(const NlotMlp* mlp);

/* ---- RRT initializer (core/trajectory_initialization.py:58-239, RRTInitializer) ----------------- */
typedef struct NlotRrtOptions {
    double bounds[2][2];       /* [[xmin, ymin], [xmax, ymax]] sampling box (YAML rrt_bounds) */
    double step_size;          /* extension step (0.05) */
    double margin;             /* safety distance added to the footprint inflation (0.01) */
    double goal_sample_rate;   /* probability of sampling the goal (0.05) */
    uint64_t seed;             /* counter-based RNG seed (the reference draws from Python's global `random`) */
    int32_t max_iter;          /* tree extensions tried (1000) */
    int32_t first_instance;    /* index of instance 0 of this call in the caller's batch (the random stream is keyed by
                                  it: a batch split into calls draws as one call; 0 otherwise) */
} NlotRrtOptions;

/* Bytes of device workspace nlot_rrt_init needs for B instances (tree, path and spline buffers). */
size_t nlot_rrt_workspace_size(const NlotRrtOptions* opt, int64_t B);

/* Batched RRTInitializer.get_initial_guess: per instance, an RRT in the xy plane from x0[b][0:2] to xg[b][0:2]
 * against the scene's EXACT SDF (MultiObstacle.sdf, casadi.py:381-383; the footprint by point inflation,
 * trajectory_initialization.py:108-113), the path with intermediate points at turns > 60 degrees, greedy
 * shortcuts and a not-a-knot cubic spline resampled to N + 1 points; other states 0 (:233-236).
 *   x0, xg   [B][nx] fp64 device      X_init [B][N+1][nx] fp64 device (out)
 *   ok       [B] int32 device (out): 1, or 0 where the reference raises "RRT failed to find a path within max_iter"
 *            (X_init of that instance is then the straight line)
 * Requires prob->sdf_kind-independent obstacles: the analytic scene in prob->obs (the training target in l4casadi
 * mode). Asynchronous on `stream`. */
int32_t nlot_rrt_init(const NlotProblem* prob, const NlotRrtOptions* opt, const double* x0, const double* xg,
                      double* X_init, int32_t* ok, int64_t B, void* workspace, size_t workspace_bytes, void* stream);
/* ---- batched trajectory verification against the exact scene (ABI v16) ------------------------
 * NLOT_SOLVED says the interior-point method converged on the NLP; these say what the trajectory does in the scene:
 * the obstacle constraint is soft with use_slack (runner.py:66-77), it holds at the N + 1 knots and the footprint's
 * corners only (densify_polygon is called with num_points = 0, geometry.py:110-112), and in learned-SDF mode it is a
 * constraint on the net.  The check samples: it bounds, it does not prove. */
typedef struct NlotVerifyOptions {
    int32_t sub;           /* poses per interval, >= 1 (default 8) */
    int32_t edge_points;   /* interior points per footprint edge, >= 0 (default 3) */
    double clearance_min;  /* NLOT_VERIFY_COLLISION if clearance < this (0) */
    double defect_tol;     /* NLOT_VERIFY_DEFECT if defect > this (1e-4 = constr_viol_tol) */
    double bound_tol;      /* NLOT_VERIFY_UBOUND / _BOUNDARY if ubound / boundary > this (1e-4) */
} NlotVerifyOptions;
#define NLOT_VERIFY_COLLISION 1  /* clearance < clearance_min */
#define NLOT_VERIFY_CONTAINS 2   /* an obstacle's centre (circle, square) or vertex (polygon, trapezoid) lies strictly
                                    inside the footprint at a sampled pose (polygon bodies); clearance is unchanged */
#define NLOT_VERIFY_DEFECT 4
#define NLOT_VERIFY_UBOUND 8
#define NLOT_VERIFY_BOUNDARY 16
#define NLOT_VERIFY_NONFINITE 32 /* a non-finite entry in the instance's X, U (or x0, xg): the four double outputs are
                                    NaN, where is -1 and no other flag is set */
/* Fill `opt` with the defaults documented above. */
void nlot_default_verify_options(NlotVerifyOptions* opt);

/* Verify B trajectories of `prob` against the scene's EXACT SDF (MultiObstacle.sdf, casadi.py:381-383, margins
 * subtracted) in prob->obs, whatever prob->sdf_kind says (like nlot_rrt_init).  Per instance:
 *   clearance  min of the exact SDF over P = N sub + 1 poses x the footprint points.  Pose s < N sub is
 *              x_k + tau (x_{k+1} - x_k), k = s / sub, tau = (s mod sub) / sub; pose N sub is knot N; components 0, 1
 *              and, for a polygon body, the heading 2 (interpolated linearly, no angle wrapping).  Footprint: the one
 *              point of NLOT_SHAPE_DOT, or per edge corner i and edge_points interior points at t = j / (edge_points + 1)
 *              towards corner i + 1 (densify_polygon, geometry.py:85-105, with num_points = edge_points)
 *   where      pose index of that minimum (the lowest on exact ties); where / sub is the knot at or before it
 *   defect     max over k and components of |x_{k+1} - Phi(x_k, u_k)|, Phi the problem's defect map (prob->integrator)
 *   ubound     max over k, i of max(umin_i - u, u - umax_i, 0)
 *   boundary   max |X_0 - x0| and |X_N - xg| (component 2 of the latter only with enforce_heading, runner.py:50-56);
 *              0 when x0 and xg are NULL
 *   flags      NLOT_VERIFY_* bits; 0 = the trajectory passed every check
 *   X [B][N+1][nx], U [B][N][nu], x0, xg [B][nx] (both or neither) fp64 device; the six outputs [B] device, all required.
 * Asynchronous on `stream`; no workspace, no global state (a stream-ordered temporary holds the problem).
 * NLOT_ERR_INVALID before any device call for: n_obs == 0, null pointers, sub < 1, edge_points < 0, exactly one of
 * x0 / xg, B outside 1 .. 2^26, a per-instance sample count beyond int32. */
int32_t nlot_verify_batch(const NlotProblem* prob, const NlotVerifyOptions* opt, const double* X, const double* U,
                          const double* x0, const double* xg, double* clearance, int32_t* where, double* defect,
                          double* ubound, double* boundary, int32_t* flags, int64_t B, void* stream);

/* ---- batched forward rollout of the returned controls through the dynamics (ABI v17) ------------
 * What a user executes is U.  nlot_verify_batch measures the plan X (its `defect` is X against the problem's own
 * discrete map, so a perfect Euler plan passes); the continuous-time robot fed U under zero-order hold does not
 * follow an Euler plan: it drifts from it at first order in dt.  The rollout integrates the problem's continuous
 * dynamics from X_0 under U and measures the rolled motion.  It is RK4 at h = dt / substeps,
 * not the exact flow; it is zero-order hold and open loop (no feedback); and it samples poses and footprint points,
 * so section 10's half-spacing bound applies to its clearance too: it bounds, it does not prove. */
typedef struct NlotRolloutOptions {
    int32_t substeps;      /* classical RK4 steps per interval, >= 1 (default 8) */
    int32_t edge_points;   /* interior points per footprint edge, >= 0 (default 3) */
    double clearance_min;  /* NLOT_ROLLOUT_COLLISION if clearance < this (0) */
    double deviation_tol;  /* NLOT_ROLLOUT_DEVIATION if deviation > this (+inf: off) */
    double goal_tol;       /* NLOT_ROLLOUT_GOAL if goal_error > this (+inf: off) */
} NlotRolloutOptions;
#define NLOT_ROLLOUT_COLLISION 1
#define NLOT_ROLLOUT_CONTAINS 2
#define NLOT_ROLLOUT_DEVIATION 4
#define NLOT_ROLLOUT_GOAL 8
#define NLOT_ROLLOUT_NONFINITE 32  /* non-finite input (X, U, xg) */
#define NLOT_ROLLOUT_DIVERGED 64   /* finite input, but a rolled state became non-finite */
/* Fill `opt` with the defaults documented above. */
void nlot_default_rollout_options(NlotRolloutOptions* opt);

/* Roll the controls of B trajectories of `prob` forward through its continuous dynamics f.  Per instance:
 *   rolled motion  starts at X[b][0]; pose s, s = 0 .. N substeps, is the state after s classical RK4 steps
 *              x + h (k1 + 2 k2 + 2 k3 + k4) / 6 of size h = dt / substeps, with the control U[b][s / substeps] held
 *              constant over its interval.  This is the flow WHATEVER prob->integrator says; at substeps = 1 the
 *              rolled knots of an NLOT_INTEG_RK4 problem are exactly that problem's defect map.  Rolled knot k is
 *              pose k substeps
 *   X_roll     [B][N+1][nx] the rolled knots, or NULL
 *   clearance  min of the scene's exact SDF (as in nlot_verify_batch) over the P = N substeps + 1 rolled poses x the
 *              footprint points of nlot_verify_batch (the one point of NLOT_SHAPE_DOT, or per edge corner i and
 *              edge_points interior points at t = j / (edge_points + 1)); the heading is component 2 of the rolled
 *              state.  Unlike nlot_verify_batch, n_obs == 0 is allowed: clearance = +inf, where = -1 and neither
 *              COLLISION nor CONTAINS is set (a learned-SDF problem without a scene can still be rolled for its
 *              deviation and goal error)
 *   where      pose index of that minimum (the lowest on exact ties); where / substeps is the knot at or before it
 *   NLOT_ROLLOUT_CONTAINS  the test of NLOT_VERIFY_CONTAINS at the rolled poses
 *   deviation  max over k = 0 .. N of hypot(X_roll_k[0] - X_k[0], X_roll_k[1] - X_k[1])
 *   dev_where  the lowest k attaining it (0 with deviation 0 when nothing departs)
 *   goal_error hypot of the position difference between rolled knot N and g; g = xg[b] if xg is given, else X[b][N]
 *   flags      NLOT_ROLLOUT_* bits; 0 = passed.  A non-finite entry in the instance's X, U (or xg) gives
 *              NLOT_ROLLOUT_NONFINITE alone, the four double outputs NaN and where = dev_where = -1.  Finite input
 *              whose rolled state turns non-finite gives NLOT_ROLLOUT_DIVERGED alone with the same NaN / -1 outputs;
 *              X_roll is unspecified from that knot on
 *   X [B][N+1][nx], U [B][N][nu], xg [B][nx] or NULL: fp64 device; the six outputs [B] device, all required.
 * An instance's outputs depend on that instance's inputs only: they are bitwise the same whatever B is and wherever
 * in the batch the instance sits.
 * Asynchronous on `stream`; no workspace, no global state (a stream-ordered temporary holds the problem).
 * NLOT_ERR_INVALID before any device call for: null prob or opt, substeps < 1, edge_points < 0, an invalid problem
 * (the checks of nlot_verify_batch without its n_obs == 0 refusal), B outside 1 .. 2^26, a null required pointer
 * (everything but xg and X_roll), (N substeps + 1) * n_body (1 + edge_points) beyond int32. */
int32_t nlot_rollout_batch(const NlotProblem* prob, const NlotRolloutOptions* opt, const double* X, const double* U,
                           const double* xg, double* X_roll, double* clearance, int32_t* where, double* deviation,
                           int32_t* dev_where, double* goal_error, int32_t* flags, int64_t B, void* stream);

/* ---- the analytic scene at arbitrary points, and SDF-quality metrics (ABI v18) ------------------
 * nlot_scene_sdf_eval evaluates the scene the solver (approximated), the RRT, nlot_verify_batch and nlot_rollout_batch
 * (exact) see, at caller-given points; nlot_sdf_metrics is the reference's compute_metrics (run_benchmark.py:34-46,
 * core/metrics.py) on two sampled SDFs.  Both are asynchronous on `stream`, take no workspace
 * and keep no global state: the problem and every temporary live in stream-ordered allocations. */
#define NLOT_SCENE_EXACT 0   /* MultiObstacle.sdf casadi.py:381-383: the min of the obstacles' exact SDFs */
#define NLOT_SCENE_APPROX 1  /* MultiObstacle.approximated_sdf casadi.py:385-386 (soft_min, prob->softmin_alpha): the
                                function the analytic-mode solver constrains */
/* val[i] = the scene's SDF of kind `kind` at pts[i], the scene being prob->obs whatever prob->sdf_kind says (like
 * nlot_verify_batch); only the scene fields of `prob` (n_obs, n_verts, obs, verts, softmin_alpha) are read.
 *   pts [P][2], val [P] fp64 device; grad [P][2] (d/dx, d/dy) and hess [P][3] (xx, xy, yy) fp64 device or NULL, each on
 *   its own, for NLOT_SCENE_APPROX only (the exact SDF has no derivative code).
 * A point's outputs depend on that point and the scene only: they are bitwise the same wherever the point sits in
 * `pts` and whatever P is.
 * NLOT_ERR_INVALID before any device call for: a null prob, pts or val; kind outside {0, 1}; n_obs == 0; an invalid
 * scene (n_obs, n_verts, an obstacle type or a vertex range out of bounds); P outside 1 .. 2^30; grad or hess with
 * NLOT_SCENE_EXACT. */
int32_t nlot_scene_sdf_eval(const NlotProblem* prob, int32_t kind, const double* pts, int64_t P, double* val,
                            double* grad, double* hess, void* stream);

typedef struct NlotSdfMetricsOptions {
    double threshold; /* the occupied sets are sdf < threshold (0) */
    double eps;       /* the surface bands are |sdf| < eps (1e-2) */
} NlotSdfMetricsOptions;
typedef struct NlotSdfMetrics { /* 64 bytes, written on the device */
    double mse;          /* mean of (target - pred)^2 */
    double iou;          /* |{target < threshold} and {pred < threshold}| / |... or ...|; 1.0 when the union is empty */
    double hausdorff;    /* max(max_{q in Q} min_{t in T} |q - t|, max_{t in T} min_{q in Q} |t - q|), T = {pts[i] :
                            |target[i]| < eps}, Q = {pts[i] : |pred[i]| < eps}; NaN when T or Q is empty */
    double chamfer;      /* (mean_{q in Q} min_t |q - t| + mean_{t in T} min_q |t - q|) / 2; NaN when T or Q is empty */
    double surface_loss; /* mean of pred[i]^2 over i in T; NaN when T is empty */
    int64_t n_target_surface, n_pred_surface; /* |T|, |Q| */
    int64_t n_points;    /* P */
} NlotSdfMetrics;
/* Fill `opt` with the defaults documented above. */
void nlot_default_sdf_metrics_options(NlotSdfMetricsOptions* opt);
/* The metrics of core/metrics.py of `pred` against `target`, two SDFs sampled at the same P points.
 *   pts [P][2], target [P], pred [P] fp64 device; out: one NlotSdfMetrics in device memory.
 * Comparisons are IEEE: a NaN entry of target or pred is in no set and makes mse NaN; it is not flagged otherwise.
 * The nearest-neighbour distances are brute force over T x Q in fp64 (min of squared distances, one sqrt).
 * The same inputs give bitwise the same NlotSdfMetrics on every call (index-ordered compaction, fixed-order
 * reductions, no floating-point atomics).  The stream-ordered temporaries are 32 P bytes for the two bands (their
 * sizes are not known on the host) plus 176 bytes per 1024 points of per-block records.
 * NLOT_ERR_INVALID before any device call for: a null pointer; P outside 1 .. 2^30; eps not > 0 or not finite; a
 * non-finite threshold. */
int32_t nlot_sdf_metrics(const NlotSdfMetricsOptions* opt, const double* pts, const double* target, const double* pred,
                         int64_t P, NlotSdfMetrics* out, void* stream);
/* ---- time-varying LQR gains about a plan, and the closed-loop tracking rollout (ABI v19) ---------
 * nlot_rollout_batch is open loop.  What tracks a plan on a robot is a feedback law about it; these two calls give
 * the standard one and measure what it does in the scene.
 *
 * Phi(x, u) is ONE classical RK4 step of size prob->dt of the problem's continuous dynamics with u held constant,
 * WHATEVER prob->integrator says: nlot_rollout_batch's flow at substeps = 1.  A_k = dPhi/dx and B_k = dPhi/du, both at
 * (X_k, U_k), by forward-mode differentiation of that step (exact to rounding).  With Q = diag(q), Qf = diag(qf),
 * R = diag(r):
 *   P_N = Qf;  for k = N - 1 .. 0:
 *     S   = R + B_k^T P_{k+1} B_k                      (2 x 2)
 *     K_k = S^-1 B_k^T P_{k+1} A_k                     (closed-form 2 x 2 inverse)
 *     P_k = Q + A_k^T P_{k+1} (A_k - B_k K_k),  then P_k <- (P_k + P_k^T) / 2
 * the finite-horizon discrete LQR of the deviation e_k = x_k - X_k under du_k = -K_k e_k. */
#define NLOT_MAX_NX 8
typedef struct NlotTvlqrOptions {
    double q[NLOT_MAX_NX];   /* diag of Q  (state weight, knots 0..N-1), each >= 0, finite; default 1 */
    double qf[NLOT_MAX_NX];  /* diag of Qf (knot N), each >= 0, finite; default 1 */
    double r[NLOT_MAX_NU];   /* diag of R, each > 0, finite; default 1 */
} NlotTvlqrOptions;          /* only the first nx / nu entries are read */
/* Fill `opt` with the defaults documented above. */
void nlot_default_tvlqr_options(NlotTvlqrOptions* opt);
#define NLOT_TVLQR_NONFINITE 32  /* a non-finite entry in the instance's X or U */
#define NLOT_TVLQR_DIVERGED 64   /* finite input, but det S <= 0 or a non-finite S, K or P at some knot */
/* The gains of B plans of `prob`.
 *   X [B][N+1][nx], U [B][N][nu] fp64 device (what nlot_solve_batch returns)
 *   K      [B][N][nu][nx] fp64 device: K_k, row-major
 *   P0     [B][nx][nx] fp64 device or NULL: P_0, the cost-to-go of a start offset d being d^T P_0 d for the
 *          linearised loop
 *   status [B] int32 device: 0, or NLOT_TVLQR_NONFINITE or NLOT_TVLQR_DIVERGED alone; either gives K all zero
 *          (tracking with it is the open loop) and P0 all NaN
 * An instance's outputs depend on that instance's inputs only: they are bitwise the same whatever B is and wherever
 * in the batch the instance sits.
 * Asynchronous on `stream`; no workspace, no global state (a stream-ordered temporary holds the problem).
 * NLOT_ERR_INVALID before any device call for: a null prob, opt, X, U, K or status; an invalid problem (the checks of
 * nlot_rollout_batch; n_obs == 0 is allowed); a q or qf entry that is negative or not finite, an r entry that is not
 * positive or not finite (the first nx / nu entries); B outside 1 .. 2^26. */
int32_t nlot_tvlqr_batch(const NlotProblem* prob, const NlotTvlqrOptions* opt, const double* X, const double* U,
                         double* K, double* P0, int32_t* status, int64_t B, void* stream);

typedef struct NlotTrackOptions {
    int32_t substeps;      /* classical RK4 steps per interval, >= 1 (default 8) */
    int32_t edge_points;   /* interior points per footprint edge, >= 0 (default 3) */
    int32_t clamp;         /* 1 (default): the applied control is clamped to prob->umin / umax; 0: it is not */
    int32_t pad_;
    double clearance_min;  /* NLOT_TRACK_COLLISION if clearance < this (0) */
    double deviation_tol;  /* NLOT_TRACK_DEVIATION if deviation > this (+inf: off) */
    double goal_tol;       /* NLOT_TRACK_GOAL if goal_error > this (+inf: off) */
} NlotTrackOptions;
/* Fill `opt` with the defaults documented above. */
void nlot_default_track_options(NlotTrackOptions* opt);
#define NLOT_TRACK_COLLISION 1
#define NLOT_TRACK_CONTAINS 2
#define NLOT_TRACK_DEVIATION 4
#define NLOT_TRACK_GOAL 8
#define NLOT_TRACK_SATURATED 16  /* saturated > 0 */
#define NLOT_TRACK_NONFINITE 32  /* non-finite input (X, U, K, dx0, xg) */
#define NLOT_TRACK_DIVERGED 64   /* finite input, but an applied control or a rolled state became non-finite */
/* nlot_rollout_batch's measurement with the loop closed.  Everything is as nlot_rollout_batch documents (poses,
 * footprint points, clearance, where, containment, deviation, dev_where, goal_error, n_obs == 0) except:
 *   rolled motion  starts at X[b][0] + dx0[b] (dx0 [B][nx] fp64 device; NULL: 0).  At rolled knot k < N, with state x:
 *              e = x - X_k over all nx components (no angle is wrapped, as everywhere in this library);
 *              u = U_k - K_k e (K [B][N][nu][nx] as nlot_tvlqr_batch writes it; NULL: u = U_k);
 *              with opt->clamp, u_i <- min(max(u_i, umin_i), umax_i);
 *              u is then held over the interval through `substeps` RK4 steps.  The controller is sampled at the
 *              knots only
 *   U_applied  [B][N][nu] fp64 device or NULL: those u
 *   saturated  [B] int32 device: the number of knots at which the clamp changed at least one component (0 without
 *              opt->clamp)
 *   flags      NLOT_TRACK_* bits; 0 = passed.  A non-finite entry in the instance's X, U, K, dx0 or xg gives
 *              NLOT_TRACK_NONFINITE alone, the three double outputs NaN and where = dev_where = saturated = -1.
 *              Finite input from which an applied control (before the clamp) or a rolled state turns non-finite gives
 *              NLOT_TRACK_DIVERGED alone with the same NaN / -1 outputs; X_roll and U_applied are unspecified from
 *              that knot on
 * With K = NULL, dx0 = NULL and clamp = 0 the rolled motion is nlot_rollout_batch's.
 * An instance's outputs depend on that instance's inputs only: they are bitwise the same whatever B is and wherever
 * in the batch the instance sits.
 * Asynchronous on `stream`; no workspace, no global state (a stream-ordered temporary holds the problem).
 * NLOT_ERR_INVALID before any device call for everything nlot_rollout_batch refuses; the required pointers are all but
 * K, dx0, xg, X_roll and U_applied. */
int32_t nlot_track_batch(const NlotProblem* prob, const NlotTrackOptions* opt, const double* X, const double* U,
                         const double* K, const double* dx0, const double* xg, double* X_roll, double* U_applied,
                         double* clearance, int32_t* where, double* deviation, int32_t* dev_where, double* goal_error,
                         int32_t* saturated, int32_t* flags, int64_t B, void* stream);

casadi_int_t nn_sdf_n_in(void);
casadi_int_t nn_sdf_n_out(void);
const casadi_int_t* nn_sdf_sparsity_in(casadi_int_t i);
const casadi_int_t* nn_sdf_sparsity_out(casadi_int_t i);
int nn_sdf(const casadi_real_t** arg, casadi_real_t** res, casadi_int_t* iw, casadi_real_t* w, int mem);
casadi_int_t jac_nn_sdf_n_in(void);
casadi_int_t jac_nn_sdf_n_out(void);
int jac_nn_sdf(const casadi_real_t** arg, casadi_real_t** res, casadi_int_t* iw, casadi_real_t* w, int mem);
casadi_int_t adj1_nn_sdf_n_in(void);
casadi_int_t adj1_nn_sdf_n_out(void);
int adj1_nn_sdf(const casadi_real_t** arg, casadi_real_t** res, casadi_int_t* iw, casadi_real_t* w, int mem);
casadi_int_t jac_adj1_nn_sdf_n_in(void);
casadi_int_t jac_adj1_nn_sdf_n_out(void);
int jac_adj1_nn_sdf(const casadi_real_t** arg, casadi_real_t** res, casadi_int_t* iw, casadi_real_t* w, int mem);

#ifdef __cplusplus
}
#endif
#endif /* NLOT_H */
