// Batched forward rollout of returned controls through the continuous dynamics (nlot_rollout_batch,
// include/nlot.h) for gfx950.
//
// The integration is sequential in time, so an instance cannot use a wavefront the way k_verify does.  A lane
// group of G lanes (a power of two, a template parameter chosen on the host from the footprint's point count)
// serves one instance, 64 / G instances per wave, fp64 throughout:
//   * integration: every lane of a group integrates its instance redundantly, sub-stepped classical RK4 with the
//     solver's own f_eff (Dyn<D + NLOT_RK4_BIAS>::f of nlot_device.h).  Same inputs, same instruction stream: the
//     state is bitwise equal across the group, so nothing is broadcast and there is no LDS;
//   * clearance: at every pose lane j evaluates footprint points j, j + G, ... against the scene's exact SDF and
//     keeps its own running (min, pose); the obstacle loop inside exact_sdf is wave-uniform, so obs[i] / verts[e]
//     stay on the scalar-load path as in k_verify and k_rrt;
//   * containment (polygon bodies): lane j tests obstacles j, j + G, ... at every pose;
//   * the group is reduced once, at the end, with __shfl_xor over offsets < G (the lowest pose on exact ties), and
//     lane 0 of the group stores.
// Groups past B leave at once and nothing synchronises across groups, so an instance's outputs depend on that
// instance's inputs only.
#include <climits>
#include <cmath>

#include "nlot_device.h"
#include "nlot_internal.h"

namespace nlot {
namespace {

constexpr int kBlock = 256;

struct RolloutArgs {
    NlotRolloutOptions opt;
    const double* X;
    const double* U;
    const double* xg;
    double* X_roll;
    double* clearance;
    int32_t* where;
    double* deviation;
    int32_t* dev_where;
    double* goal_error;
    int32_t* flags;
    int64_t B;
};

template <int G>
__device__ inline int group_or(int v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

template <int D, int G>
__global__ __launch_bounds__(kBlock) void k_rollout(const NlotProblem* __restrict__ pp, RolloutArgs a) {
    using DY = Dyn<D + NLOT_RK4_BIAS>;
    constexpr int NX = DY::NX, NU = DY::NU;
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    if (b >= a.B) return;  // whole groups leave: the shuffles below stay inside a group
    const int j = threadIdx.x & (G - 1);
    const NlotProblem& p = *pp;
    const int N = p.N, sub = a.opt.substeps;
    const double* X = a.X + (size_t)b * (N + 1) * NX;
    const double* U = a.U + (size_t)b * N * NU;
    const double* g = a.xg ? a.xg + (size_t)b * NX : X + (size_t)N * NX;

    // non-finite input: fmin and the comparisons below drop NaNs, so it is tested on its own
    int bad = 0;
    for (int i = j; i < (N + 1) * NX; i += G) bad |= !isfinite(X[i]);
    for (int i = j; i < N * NU; i += G) bad |= !isfinite(U[i]);
    if (a.xg) {
        for (int i = j; i < NX; i += G) bad |= !isfinite(g[i]);
    }
    if (group_or<G>(bad)) {
        if (j == 0) {
            a.clearance[b] = a.deviation[b] = a.goal_error[b] = NAN;
            a.where[b] = a.dev_where[b] = -1;
            a.flags[b] = NLOT_ROLLOUT_NONFINITE;
        }
        return;
    }

    const bool poly = p.shape == NLOT_SHAPE_POLYGON;
    const int per_edge = 1 + a.opt.edge_points;
    const int npp = p.n_obs == 0 ? 0 : poly ? p.n_body * per_edge : 1;  // no scene: no footprint work
    const bool inner = poly && p.n_body >= 3 && p.n_obs > 0;
    const double h = p.dt / (double)sub;
    double* Xr = a.X_roll ? a.X_roll + (size_t)b * (N + 1) * NX : nullptr;

    double x[NX], u[NU] = {}, fe[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = X[i];
    double best = INFINITY, dev = 0.0;
    int bs = INT_MAX, dk = 0, contains = 0, diverged = 0;

    // footprint points j, j + G, ... and obstacles j, j + G, ... of pose s (the state x)
    auto visit = [&](int s) {
        double sn = 0.0, cs = 1.0;
        if (poly) sincos(x[2], &sn, &cs);
        for (int q = j; q < npp; q += G) {
            double wx = x[0], wy = x[1];
            if (poly) {  // PolygonGeometry.transform of corners i, i + 1, then densify_polygon's (1 - t) p0 + t p1
                const int i = q / per_edge, m = q - i * per_edge, i1 = i + 1 < p.n_body ? i + 1 : 0;
                const double ax = x[0] + cs * p.body[i][0] - sn * p.body[i][1];
                const double ay = x[1] + sn * p.body[i][0] + cs * p.body[i][1];
                wx = ax;
                wy = ay;
                if (m > 0) {
                    const double bx = x[0] + cs * p.body[i1][0] - sn * p.body[i1][1];
                    const double by = x[1] + sn * p.body[i1][0] + cs * p.body[i1][1];
                    const double t = (double)m / (double)per_edge;
                    wx = (1.0 - t) * ax + t * bx;
                    wy = (1.0 - t) * ay + t * by;
                }
            }
            const double v = exact_sdf(p, wx, wy);
            if (v < best) {  // s ascends: the first pose of the lane's minimum
                best = v;
                bs = s;
            }
        }
        if (inner) {  // an obstacle smaller than the footprint can sit inside it with every perimeter point outside
            for (int i = j; i < p.n_obs; i += G) {
                const NlotObstacle& q = p.obs[i];
                if (q.type == NLOT_OBS_CIRCLE || q.type == NLOT_OBS_SQUARE) {
                    const double dx = q.cx - x[0], dy = q.cy - x[1];
                    contains |= inside_body(p, cs * dx + sn * dy, -sn * dx + cs * dy);
                } else {
                    for (int e = 0; e < q.nv; ++e) {
                        const double dx = p.verts[q.v0 + e][0] - x[0], dy = p.verts[q.v0 + e][1] - x[1];
                        contains |= inside_body(p, cs * dx + sn * dy, -sn * dx + cs * dy);
                    }
                }
            }
        }
    };

    for (int k = 0, s = 0; k <= N; ++k) {  // x is rolled knot k = pose s = k sub
        const double* xk = X + (size_t)k * NX;
        const double d = hypot(x[0] - xk[0], x[1] - xk[1]);
        if (d > dev) {  // k ascends: the lowest knot of the maximum
            dev = d;
            dk = k;
        }
        if (Xr && j == 0) {
#pragma unroll
            for (int i = 0; i < NX; ++i) Xr[(size_t)k * NX + i] = x[i];
        }
        if (k < N) {  // zero-order hold over the interval
#pragma unroll
            for (int i = 0; i < NU; ++i) u[i] = U[(size_t)k * NU + i];
        }
        for (int r = 0; r < sub; ++r, ++s) {
            visit(s);
            if (k == N) break;  // the last pose is knot N
            DY::f(x, u, p.wheelbase, fe, h);
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                x[i] += h * fe[i];
                diverged |= !isfinite(x[i]);
            }
        }
    }

#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off);
        const int os = __shfl_xor(bs, off);
        if (ov < best || (ov == best && os < bs)) {
            best = ov;
            bs = os;
        }
    }
    contains = group_or<G>(contains);

    if (j == 0) {
        if (diverged) {
            a.clearance[b] = a.deviation[b] = a.goal_error[b] = NAN;
            a.where[b] = a.dev_where[b] = -1;
            a.flags[b] = NLOT_ROLLOUT_DIVERGED;
            return;
        }
        const double ge = hypot(x[0] - g[0], x[1] - g[1]);
        int fl = 0;
        if (best < a.opt.clearance_min) fl |= NLOT_ROLLOUT_COLLISION;
        if (contains) fl |= NLOT_ROLLOUT_CONTAINS;
        if (dev > a.opt.deviation_tol) fl |= NLOT_ROLLOUT_DEVIATION;
        if (ge > a.opt.goal_tol) fl |= NLOT_ROLLOUT_GOAL;
        a.clearance[b] = best;
        a.where[b] = bs == INT_MAX ? -1 : bs;
        a.deviation[b] = dev;
        a.dev_where[b] = dk;
        a.goal_error[b] = ge;
        a.flags[b] = fl;
    }
}

template <int D, int G>
void launch_dg(const NlotProblem* dP, const RolloutArgs& a, hipStream_t st) {
    const unsigned grid = (unsigned)((a.B * G + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((k_rollout<D, G>), dim3(grid), dim3(kBlock), 0, st, dP, a);
}
template <int D>
void launch_d(int G, const NlotProblem* dP, const RolloutArgs& a, hipStream_t st) {
    switch (G) {
        case 1: return launch_dg<D, 1>(dP, a, st);
        case 4: return launch_dg<D, 4>(dP, a, st);
        case 16: return launch_dg<D, 16>(dP, a, st);
        default: return launch_dg<D, 64>(dP, a, st);
    }
}

}  // namespace
}  // namespace nlot

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
    static const int kNx[6] = {4, 4, 3, 5, 4, 7};
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
    if (prob->dynamics < 0 || prob->dynamics > NLOT_ACKERMANN_2ND || prob->nx != kNx[prob->dynamics] || prob->nu != 2 ||
        prob->N < 1 || prob->N > 1 << 24 || prob->n_obs < 0 || prob->n_obs > NLOT_MAX_OBS || prob->n_verts < 0 ||
        prob->n_verts > NLOT_MAX_VERTS || (prob->shape != NLOT_SHAPE_DOT && prob->shape != NLOT_SHAPE_POLYGON) ||
        (prob->shape == NLOT_SHAPE_POLYGON && (prob->n_body < 1 || prob->n_body > NLOT_MAX_BODY))) {
        set_error("nlot_rollout_batch: invalid problem (dynamics, nx / nu, 1 <= N <= 2^24, shape, n_body, n_obs, n_verts)");
        return NLOT_ERR_INVALID;
    }
    for (int i = 0; i < prob->n_obs; ++i) {
        const NlotObstacle& q = prob->obs[i];
        if (q.type < NLOT_OBS_CIRCLE || q.type > NLOT_OBS_TRAPEZOID) {
            set_error("nlot_rollout_batch: unknown obstacle type");
            return NLOT_ERR_INVALID;
        }
        if ((q.type == NLOT_OBS_POLYGON || q.type == NLOT_OBS_TRAPEZOID) &&
            (q.v0 < 0 || q.nv < 2 || q.v0 > prob->n_verts - q.nv)) {
            set_error("nlot_rollout_batch: polygon vertex range outside verts[0, n_verts)");
            return NLOT_ERR_INVALID;
        }
    }
    if (B < 1 || B > (int64_t)1 << 26) {
        set_error("nlot_rollout_batch: B out of range");
        return NLOT_ERR_INVALID;
    }
    // the kernel counts poses and footprint points with ints
    const int64_t P = (int64_t)prob->N * opt->substeps + 1;
    const int64_t npp = prob->shape == NLOT_SHAPE_POLYGON ? (int64_t)prob->n_body * (1 + (int64_t)opt->edge_points) : 1;
    if (P > INT32_MAX || npp > INT32_MAX || P * npp > INT32_MAX - 64) {
        set_error("nlot_rollout_batch: sample count (N substeps + 1) * n_body (1 + edge_points) overflows int32");
        return NLOT_ERR_INVALID;
    }
    if (!X || !U || !clearance || !where || !deviation || !dev_where || !goal_error || !flags) {
        set_error("nlot_rollout_batch: null pointer");
        return NLOT_ERR_INVALID;
    }
    const int G = npp <= 1 ? 1 : npp <= 4 ? 4 : npp <= 16 ? 16 : 64;  // lanes per instance: one footprint point each
    // the kernel reads the problem through a pointer (it is larger than the kernel-argument area): a stream-ordered
    // device copy that lives for this call only — no workspace argument, no global state
    hipStream_t st = (hipStream_t)stream;
    NlotProblem* dP = nullptr;
    NLOT_HIP_CHECK(hipMallocAsync((void**)&dP, sizeof(NlotProblem), st));
    hipError_t e = hipMemcpyAsync(dP, prob, sizeof(NlotProblem), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const RolloutArgs a{*opt, X, U, xg, X_roll, clearance, where, deviation, dev_where, goal_error, flags, B};
        switch (prob->dynamics) {
            case NLOT_POINT_1ST: launch_d<NLOT_POINT_1ST>(G, dP, a, st); break;
            case NLOT_POINT_2ND: launch_d<NLOT_POINT_2ND>(G, dP, a, st); break;
            case NLOT_UNICYCLE: launch_d<NLOT_UNICYCLE>(G, dP, a, st); break;
            case NLOT_UNICYCLE_2ND: launch_d<NLOT_UNICYCLE_2ND>(G, dP, a, st); break;
            case NLOT_ACKERMANN: launch_d<NLOT_ACKERMANN>(G, dP, a, st); break;
            default: launch_d<NLOT_ACKERMANN_2ND>(G, dP, a, st); break;
        }
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(dP, st);
    NLOT_HIP_CHECK(e);
    NLOT_HIP_CHECK(ef);
    return NLOT_OK;
}
