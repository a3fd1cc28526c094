// The solver workspace: phases, per-instance scalars, dimensions and the carve-up of the caller's buffer (host and device).
// Included by nlot_solver.hip (the kernels and run<>()) and by the C ABI unit, nlot_solve_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "nlot_internal.h"

namespace nlot {

// PH_SOFT1 / PH_SOFT2: IPOPT's soft restoration step (BacktrackingLineSearch::TrySoftRestoStep) — the damped
// step's filter test on a value launch, then (not filter-acceptable) the primal-dual error at the tentatively
// accepted point on a full launch.  PH_RINIT: first step of a feasibility restoration phase (its point's full
// evaluation, then MinC_1NrmRestorationPhase's initialisation); while SC_RESTO = 1 the EVAL / LS phases belong to
// the restoration problem (k_resto_a / k_ric<DYN, true> / k_resto_b / k_resto_ls).
enum Phase { PH_INIT = 0, PH_EVAL = 1, PH_LS = 2, PH_DONE = 3, PH_SOC = 4, PH_SOFT1 = 5, PH_SOFT2 = 6, PH_RINIT = 7 };
// k_iter_a's passes (run() launches SOC on the side stream at the start of a step and EVAL after the full MLP launch)
enum IterPass { PASS_ALL = 0, PASS_INIT = 1, PASS_SOC = 2, PASS_EVAL = 3 };

enum Scal {
    SC_MU, SC_TAU, SC_DWLAST, SC_THMAX, SC_THMIN, SC_ALPHA, SC_AMAX, SC_AMIN, SC_AZ, SC_THETA, SC_PHI, SC_GD,
    SC_DW, SC_DC, SC_STATUS, SC_ITERS, SC_PHASE, SC_TRIALS, SC_NFILT, SC_RANK, SC_E0, SC_NCAND,
    SC_FREE, SC_MUMAX, SC_NAF,  // adaptive mu: free-mode flag, mu_max, progress-filter entries
    // hand-off k_iter_a -> k_ric -> k_iter_b: Newton-solve state (0 idle, 1 pending, 2 solved, 3 LSQ
    // failed), its barrier parameters and right-hand-side count, and the optimality scalars the
    // quality-function oracle needs
    SC_RIC, SC_RMU0, SC_RMU1, SC_RNR, SC_USEQF, SC_AVG, SC_DSQ, SC_PSQ, SC_NZC,
    SC_ACCSLOT,  // trial-list slot of the accepted line-search candidate (forward reuse), -1 if none
    // IPOPT's globalisation safeguards: second-order correction (count in progress, the
    // original trial's alpha and alpha_z, theta of the last corrected trial), k_ric's fixed delta_w (-1: the
    // inertia-correction loop), watchdog (active, shortened-step counter, trials, reference values and the
    // saved line-search scalars), tiny step (this iteration, the previous one), max primal infeasibility
    SC_SOCK, SC_SOCA, SC_SOCAZ, SC_SOCTH, SC_RICFIX,
    SC_WD, SC_WDSHORT, SC_WDTRIAL, SC_WDTH, SC_WDPH, SC_WDGD, SC_WDAT, SC_WDAZ, SC_WDAMIN, SC_WDMU, SC_WDTAU,
    SC_TINY, SC_TINYLAST, SC_PRIMAL,
    // IPOPT's filter reset heuristic: last rejection of this line search was by the filter, successive such
    // iterations, resets done
    SC_LASTREJF, SC_NFREJ, SC_NFRES,
    // soft restoration: active, iterations, primal-dual error at the current point and the mu it was taken at
    SC_INSOFT, SC_SOFTCNT, SC_PDC, SC_MUPD,
    // feasibility restoration (MinC_1Nrm): active, first iteration, the original problem's mu / tau / last
    // delta_w, theta_R and phi_R at the restoration's start, rho, zeta, the restoration's theta_max / theta_min
    // and filter entries, restoration phases started (statistics)
    SC_RESTO, SC_RFIRST, SC_RMUO, SC_RTAUO, SC_RDWO, SC_THR, SC_PHR, SC_RHO, SC_ZETA, SC_RTHMAX, SC_RTHMIN,
    SC_RNFILT, SC_NRESTO,
    // inertia correction carried over to the next global step (k_ric's attempt cap): the next delta_w to try (-1:
    // none pending) and the delta_w already added into hg
    SC_RETRY, SC_DWHG,
    SC_COUNT
};
// Filters (line search, adaptive-mu progress, restoration): IPOPT's Filter is an unbounded list from which
// dominated entries are removed.  At most one entry enters per iteration (the line-search filter can grow to
// 2 max_iter + O(1) in principle); the largest size measured over the round-4 metric bench was 613 (bench.py
// config.filters), so 1024 entries per filter are unbounded in effect there.  An overflow forgets the oldest entry;
// it is counted (NlotSolveStats.filter_forgotten, the restoration filter included) and reported by bench.py.
constexpr int FILT_MAX = 1024;
// ints per step-parity counter set (workspace counters: 2 sets): [0..8) the phase machine's counts (Ws::cnt), [8..11)
// diagnostics of the factorising Newton solves (attempts summed, their maximum, solves needing more than one), [11]
// the largest filter size reached and [12] filter entries forgotten at capacity (diagnostics), [15] the most
// factorisations one restoration Newton solve took (diagnostics), [13]
// where k_admit's slots start in the active list.  After the two sets: the free-slot count and k_admit's error flag.
constexpr int CSET = 16;
constexpr int NSPEC = 8;  // step lengths evaluated per line-search round after a first rejection
constexpr int MMAX = 4;  // inequalities per knot (rectangle without slack)

struct Dims {
    int N, nx, nu, ns, M, nc, nb, nv, sd;  // nv = nu + ns (stage k < N)
    int tidx[8];
    int ppk;  // SDF points per knot (corners, or 1 for a dot)
    // general bounds (NlotSolverOptions.general_bounds): the control bounds and slack >= 0 as constraint rows, the way
    // CasADi's Opti hands them to IPOPT (runner.py:67-69,101-103).  ngb = bound rows N nu + ns (N + 1) (the workspace
    // always holds their arrays: the workspace size does not depend on the options); gcb = 1 selects the form
    int ngb, gcb;
};

static Dims make_dims(const NlotProblem& p) {
    Dims d{};
    d.N = p.N;
    d.nx = p.nx;
    d.nu = p.nu;
    d.ns = p.use_slack ? 1 : 0;
    d.nb = p.shape == NLOT_SHAPE_DOT ? 1 : p.n_body;
    d.M = p.shape == NLOT_SHAPE_DOT ? 1 : (p.use_slack ? 1 : p.n_body);
    d.sd = (p.shape == NLOT_SHAPE_POLYGON && p.use_slack) ? 1 : 0;
    d.nv = p.nu + d.ns;
    d.nc = 0;
    for (int i = 0; i < p.nx; ++i)
        if (p.enforce_heading || i != 2) d.tidx[d.nc++] = i;
    d.ppk = d.nb;
    d.ngb = p.N * p.nu + d.ns * (p.N + 1);
    d.gcb = 0;  // run() sets it from the options
    return d;
}

// Riccati storage per knot (one Newton solve with up to two right-hand sides):
//   slot (LDS when it fits, else HBM): [A B 0] (nx x nz) | c | M (2x2) | K (nv x nx) | k (2 x nv) | Kn (nv x nc)
//     — everything the sequential forward sweep reads;
//   hg (HBM): H (nz x nz) | g (2 x nz) — built in parallel over knots, read once by the backward sweep
//     (prefetched one stage ahead);
//   vf (HBM): P (nx x nx) | p (2 x nx) | Gamma (nx x nc) — written by the backward sweep, read by the
//     parallel multiplier pass.  (nz = nx + nu + 1, nv = nu + 1, nc = nx.)
//   Layouts (row-major, ncol = nx + 2 + nc gain columns K | k_0 | k_1 | Kn):
//     slot = [A B 0 | c | pad] (nx x ab_row) | M | GN (ncol x nv);  hg = [H | g_0 g_1] (nz x (nz+2)) (the
//     Riccati lane of column j reads row j, H being symmetric, or a g column top to bottom);
//     vf = [P | p_0 p_1 | Gamma] (nx x ncol).
__host__ __device__ constexpr int ab_row(int nx, int nu) { return (nx + nu + 2 + 1) & ~1; }  // [A B 0 | c], even
__host__ __device__ constexpr int slot_len(int nx, int nu) {
    return nx * ab_row(nx, nu) + 4 + (nx + 2 + nx) * (nu + 1);
}
__host__ __device__ constexpr int hg_len(int nx, int nu) { return (nx + nu + 1) * (nx + nu + 3); }
__host__ __device__ constexpr int vf_len(int nx, int nu) { return nx * (nx + 2 + nx); }
// quality-function oracle step buffers (affine / centering): dX dU dS yi yk yt | dT dzl dzu dzs dvt | dsb (the
// bound rows' slack step, general bounds)
__host__ __device__ constexpr int qf_len(int N, int nx, int nu, int M, int ngb) {
    return (N + 1) * nx + N * nu + (N + 1) + nx + N * nx + 8 + (N + 1) * M + 2 * N * nu + (N + 1) + (N + 1) * M + ngb;
}

// an iterate (X U S T yi yk yt yd zl zu zs vt sb yb) or a step (dX dU dS dT yi_n yk_n yt_n yd_n dzl dzu dzs dvt dsb
// yb_n): the save areas of the second-order correction and the watchdog
__host__ __device__ constexpr int it_len(int N, int nx, int nu, int M, int ngb) {
    return (N + 1) * nx + 3 * N * nu + 2 * (N + 1) + 3 * (N + 1) * M + nx + N * nx + 8 + 2 * ngb;
}

// restoration rows (oracle Sol::rp ...): [initial state nx][dynamics N nx][terminal nc][inequalities (N+1) M]
// [bound rows ngb (general bounds)], allocated with the terminal block padded to 8
__host__ __device__ constexpr int ne_len(int N, int nx, int M, int ngb) { return nx + N * nx + 8 + (N + 1) * M + ngb; }

// a stored pivoted LDL^T factor of an n x n block (ldl_factor's in-place form, then the permutation): the Q_vv
// factor of every stage and the terminal block's, kept by each Newton solve for the second-order corrections
__host__ __device__ constexpr int ldl_len(int n) { return n * n + n; }

// instance-major arrays: (name, per-instance length)
#define NLOT_WS_ARRAYS(X_)                                                                             \
    X_(X, (N + 1) * nx) X_(U, N * nu) X_(S, N + 1) X_(T, (N + 1) * M) X_(yi, nx) X_(yk, N * nx) X_(yt, 8) \
    X_(yd, (N + 1) * M) X_(zl, N * nu) X_(zu, N * nu) X_(zs, N + 1) X_(vt, (N + 1) * M)                \
    X_(dv, (N + 1) * M) X_(Jd, (N + 1) * M * 3) X_(Hd, (N + 1) * 6) X_(rci, nx) X_(rcd, N * nx)         \
    X_(rct, 8) X_(rcq, (N + 1) * M) X_(dX, (N + 1) * nx) X_(dU, N * nu) X_(dS, N + 1)                  \
    X_(dT, (N + 1) * M) X_(yi_n, nx) X_(yk_n, N * nx) X_(yt_n, 8) X_(yd_n, (N + 1) * M)                \
    X_(dzl, N * nu) X_(dzu, N * nu) X_(dzs, N + 1) X_(dvt, (N + 1) * M) X_(sc, SC_COUNT)               \
    X_(filt, 2 * FILT_MAX) X_(afilt, 2 * FILT_MAX) X_(qa, qf_len(N, nx, nu, M, ngb)) X_(qc, qf_len(N, nx, nu, M, ngb)) \
    X_(stg, (N + 1) * slot_len(nx, nu)) X_(hg, (N + 1) * hg_len(nx, nu)) X_(vf, (N + 1) * vf_len(nx, nu))   \
    X_(dX2, (N + 1) * nx) X_(dU2, N * nu) X_(dS2, N + 1) X_(yi2, nx) X_(yk2, N * nx) X_(yt2, 8)         \
    X_(sts, it_len(N, nx, nu, M, ngb)) X_(rcs, nx + N * nx + 8 + (N + 1) * M + ngb)                     \
    X_(wdi, it_len(N, nx, nu, M, ngb)) X_(wdd, it_len(N, nx, nu, M, ngb))                               \
    X_(rp, ne_len(N, nx, M, ngb)) X_(rn, ne_len(N, nx, M, ngb)) X_(rzp, ne_len(N, nx, M, ngb))           \
    X_(rzn, ne_len(N, nx, M, ngb)) X_(rdp, ne_len(N, nx, M, ngb)) X_(rdn, ne_len(N, nx, M, ngb))         \
    X_(rdzp, ne_len(N, nx, M, ngb)) X_(rdzn, ne_len(N, nx, M, ngb)) X_(dsoft, ne_len(N, nx, M, ngb))     \
    X_(esoft, ne_len(N, nx, M, ngb)) X_(rfilt, 2 * FILT_MAX)                                            \
    X_(qfac, (N + 1) * ldl_len(nu + 1)) X_(tfac, ldl_len(nx)) X_(x0s, nx) X_(xgs, nx) X_(phi, N * nx * (nx + 2)) \
    X_(sb, ngb) X_(yb, ngb) X_(rcb, ngb) X_(dsb, ngb) X_(yb_n, ngb)

struct Ws {
#define NLOT_DECL(name, cnt) \
    double* name;            \
    int L_##name;
    NLOT_WS_ARRAYS(NLOT_DECL)
#undef NLOT_DECL
    float* pts;  // compacted corner list, rank-major [rank][P][2]
    float* mo;   // MLP outputs [6][cap * P] (rank-major within a plane)
    // trial lists by global-step parity q: the full launch of step s + 1 reuses step s's accepted
    // candidate while k_accept of step s already emits the candidates of step s + 1
    float* tpts[2];      // trial corner list [slot][P][2] (slot = rank + candidate), cap * NSPEC slots
    float* tval[2];      // its values [slot][P]
    uint32_t* tmask[2];  // its hidden-layer ReLU patterns [4][slot][P]
    int* tsrc;           // per evaluation rank: trial slot whose forward the full launch may reuse, or -1
    int* cnt;  // counters of step parity q at cnt + CSET q: [0] evaluation ranks, [1] trial slots, [2] next active
               // count, [3] full-launch points whose forward was reused, [4] Newton solves, [5] restoration list count,
               // [6] second-order corrections, [7] restoration Newton solves
    int* act[2]; // active instance lists (ping-pong)
    int* actr[2]; // the instances of act in a restoration phase (count: counter [5] of the step's set)
    int* ricl;    // this step's factorising Newton solves (count: counter [4]), compacted by k_iter_a for k_ric
    int* socl;    // this step's second-order corrections (count: counter [6])
    // Slots: every array above is indexed by slot (cap slots); sinst[slot] is the instance a slot holds.  An instance
    // leaving the active list (k_accept) writes its outputs (o*, instance-indexed, caller-owned) and frees its slot
    // (freel, count at cnt[2 CSET]); k_admit gives free slots to the next instances, k_init_state starts them.
    int* sinst;
    int* freel;
    double *oX, *oU, *oS, *ocost;
    int32_t *ostat, *oiters;
    int64_t cap;
    int ppk;
    int prio;  // NLOT_SETPRIO: the side-stream chains (restoration solves, corrections) raise their waves' issue priority
};

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// doubles of all instance-major arrays for B instances, each array rounded up to 256 bytes
static size_t ws_doubles(const Dims& d, int64_t B) {
    const int N = d.N, nx = d.nx, nu = d.nu, M = d.M, ngb = d.ngb;
    size_t n = 0;
#define NLOT_CNT(name, cnt) n += ((size_t)(cnt) * (size_t)B + 31) & ~(size_t)31;
    NLOT_WS_ARRAYS(NLOT_CNT)
#undef NLOT_CNT
    return n;
}

constexpr size_t kHdr = 32768;  // device copies of NlotProblem, Dims, Ws (kernels read them through pointers:
                                // a by-value struct argument indexed at run time is copied to scratch)
constexpr size_t kHdrProblem = 0, kHdrDims = 24576, kHdrWs = 28672;  // NlotProblem ~14.5 KB (vertex pool)

static size_t ws_bytes(const Dims& d, int64_t B, bool mlp) {
    size_t b = kHdr + align256(ws_doubles(d, B) * sizeof(double));
    if (mlp) {  // corner list and outputs sized for NSPEC line-search candidates per instance
        const size_t P = (size_t)d.ppk * (d.N + 1);
        b += align256(P * (size_t)B * NSPEC * 2 * sizeof(float));
        b += align256(6 * P * (size_t)B * NSPEC * sizeof(float));
        b += 2 * align256(P * (size_t)B * NSPEC * 2 * sizeof(float));     // tpts, per step parity
        b += 2 * align256(P * (size_t)B * NSPEC * sizeof(float));         // tval
        b += 2 * align256(4 * P * (size_t)B * NSPEC * sizeof(uint32_t));  // tmask
        b += align256((size_t)B * sizeof(int));                    // tsrc
    }
    b += align256(2 * (size_t)B * sizeof(int));
    b += align256(2 * (size_t)B * sizeof(int));  // restoration lists
    b += 2 * align256((size_t)B * sizeof(int));  // Newton-solve and correction lists
    b += 2 * align256((size_t)B * sizeof(int));  // slot -> instance, free slots
    b += 256;  // counters (2 sets of CSET ints)
    return b;
}

static Ws carve(const Dims& d, int64_t B, bool mlp, void* base) {
    Ws w{};
    w.cap = B;
    w.ppk = d.ppk;
    const int N = d.N, nx = d.nx, nu = d.nu, M = d.M, ngb = d.ngb;
    base = (char*)base + kHdr;
    double* q = (double*)base;
#define NLOT_TAKE(name, cnt)          \
    w.name = q;                       \
    w.L_##name = (int)(cnt);          \
    q += ((size_t)(cnt) * (size_t)B + 31) & ~(size_t)31;
    NLOT_WS_ARRAYS(NLOT_TAKE)
#undef NLOT_TAKE
    char* c = (char*)base + align256(ws_doubles(d, B) * sizeof(double));
    if (mlp) {
        const size_t P = (size_t)d.ppk * (N + 1);
        w.pts = (float*)c;
        c += align256(P * (size_t)B * NSPEC * 2 * sizeof(float));
        w.mo = (float*)c;
        c += align256(6 * P * (size_t)B * NSPEC * sizeof(float));
        for (int q = 0; q < 2; ++q) {
            w.tpts[q] = (float*)c;
            c += align256(P * (size_t)B * NSPEC * 2 * sizeof(float));
            w.tval[q] = (float*)c;
            c += align256(P * (size_t)B * NSPEC * sizeof(float));
            w.tmask[q] = (uint32_t*)c;
            c += align256(4 * P * (size_t)B * NSPEC * sizeof(uint32_t));
        }
        w.tsrc = (int*)c;
        c += align256((size_t)B * sizeof(int));
    }
    w.act[0] = (int*)c;
    w.act[1] = (int*)c + B;
    c += align256(2 * (size_t)B * sizeof(int));
    w.actr[0] = (int*)c;
    w.actr[1] = (int*)c + B;
    c += align256(2 * (size_t)B * sizeof(int));
    w.ricl = (int*)c;
    c += align256((size_t)B * sizeof(int));
    w.socl = (int*)c;
    c += align256((size_t)B * sizeof(int));
    w.sinst = (int*)c;
    c += align256((size_t)B * sizeof(int));
    w.freel = (int*)c;
    c += align256((size_t)B * sizeof(int));
    w.cnt = (int*)c;
    return w;
}

// slots of a call: min(B, max_active) (continuous batching) or B; the workspace holds the slots' state only
static int64_t slot_count(int64_t B, int32_t max_active) { return max_active > 0 && max_active < B ? max_active : B; }

// the solve itself, one instantiation per dynamics model and integrator (nlot_solver_run.h; the units of
// nlot_solver.hip instantiate it, nlot_solve_batch dispatches to it)
template <int DYN>
int run(const NlotProblem& p, const NlotSolverOptions& o, const NlotMlp* mlp, const double* x0, const double* xg,
        const double* Xinit, double* X, double* U, double* S, double* cost, int32_t* status, int32_t* iters,
        int64_t B, void* workspace, hipStream_t st);

}  // namespace nlot
