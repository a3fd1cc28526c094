// What the three measurement kernels share (internal, not part of the ABI): k_verify (nlot_verify.hip) uses the group
// reductions, footprint_point and obstacles_inside_body; nlot_rollout_batch and nlot_track_batch are the one rollout
// kernel k_roll<D, G, Law> below, instantiated with the OpenLoop law in nlot_rollout.hip and with the ClosedLoop law
// in nlot_track.hip, which keep only the dispatch and the C entry points (and, nlot_track.hip, k_tvlqr).
//
// k_roll: the integration is sequential in time, so an instance cannot use a wavefront the way k_verify does.  A lane
// group of G lanes (a power of two, a template parameter chosen on the host from the footprint's point count)
// serves one instance, 64 / G instances per wave, fp64 throughout:
//   * integration: every lane of a group integrates its instance redundantly, sub-stepped classical RK4 with the
//     solver's own f_eff (Dyn<D + NLOT_RK4_BIAS>::f of nlot_device.h).  Same inputs, same instruction stream: the
//     state is bitwise equal across the group, so nothing is broadcast and there is no LDS;
//   * control: the law gives u of interval k at its knot (OpenLoop: U_k; ClosedLoop: the clamped feedback, computed
//     redundantly by every lane from the bitwise-equal state), held over the interval;
//   * clearance: at every pose lane j evaluates footprint points j, j + G, ... against the scene's exact SDF and
//     keeps its own running (min, pose); the obstacle loop inside exact_sdf is wave-uniform, so obs[i] / verts[e]
//     stay on the scalar-load path as in k_verify and k_rrt;
//   * containment (polygon bodies): lane j tests obstacles j, j + G, ... at every pose;
//   * the group is reduced once, at the end, with __shfl_xor over offsets < G (the lowest pose on exact ties), and
//     lane 0 of the group stores.
// Groups past B leave at once and nothing synchronises across groups, so an instance's outputs depend on that
// instance's inputs only.  The body is written in the kernel and the law is a kernel argument: the
// same body in a __device__ function called from two kernels costs 3-10 VGPRs and, at two instantiations, a wave
// of occupancy.
#pragma once
#include <climits>
#include <cmath>

#include "nlot_device.h"
#include "nlot_internal.h"

namespace nlot {

template <int G>
__device__ inline int group_or(int v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
// (min, its index) over a group of G lanes, the lowest index on exact ties
template <int G>
__device__ inline void group_argmin(double& best, int& bs) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off);
        const int os = __shfl_xor(bs, off);
        if (ov < best || (ov == best && os < bs)) {
            best = ov;
            bs = os;
        }
    }
}

// Point q of a polygon body's sampled perimeter at the pose (px, py, heading with sine sn, cosine cs):
// PolygonGeometry.transform of corners i, i + 1, then densify_polygon's (1 - t) p0 + t p1
__device__ inline void footprint_point(const NlotProblem& p, double px, double py, double sn, double cs, int q,
                                       int per_edge, double* wx, double* wy) {
    const int i = q / per_edge, m = q - i * per_edge, i1 = i + 1 < p.n_body ? i + 1 : 0;
    const double ax = px + cs * p.body[i][0] - sn * p.body[i][1];
    const double ay = py + sn * p.body[i][0] + cs * p.body[i][1];
    *wx = ax;
    *wy = ay;
    if (m > 0) {
        const double bx = px + cs * p.body[i1][0] - sn * p.body[i1][1];
        const double by = py + sn * p.body[i1][0] + cs * p.body[i1][1];
        const double t = (double)m / (double)per_edge;
        *wx = (1.0 - t) * ax + t * bx;
        *wy = (1.0 - t) * ay + t * by;
    }
}

// Sets `contains` if one of the obstacles first, first + stride, ... has its centre / a vertex strictly inside the
// polygon body at that pose: an obstacle smaller than the footprint can sit inside it with every perimeter point
// outside.  It ORs into the caller's variable: accumulating in a local and returning it reschedules k_roll's pose loop
// (+0.4-2 % on the MI355X at equal registers).
__device__ inline void obstacles_inside_body(const NlotProblem& p, double px, double py, double sn, double cs,
                                             int first, int stride, int& contains) {
    for (int i = first; i < p.n_obs; i += stride) {
        const NlotObstacle& q = p.obs[i];
        if (q.type == NLOT_OBS_CIRCLE || q.type == NLOT_OBS_SQUARE) {
            const double dx = q.cx - px, dy = q.cy - py;
            contains |= inside_body(p, cs * dx + sn * dy, -sn * dx + cs * dy);
        } else {
            for (int e = 0; e < q.nv; ++e) {
                const double dx = p.verts[q.v0 + e][0] - px, dy = p.verts[q.v0 + e][1] - py;
                contains |= inside_body(p, cs * dx + sn * dy, -sn * dx + cs * dy);
            }
        }
    }
}

constexpr int kRollBlock = 256;

// nlot_rollout_batch's law: the control of interval k is U_k, the roll starts at X_0.  Its members are what both
// laws read and write.
struct OpenLoop {
    int substeps, edge_points;
    double clearance_min, deviation_tol, goal_tol;
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

    static constexpr int kNonfinite = NLOT_ROLLOUT_NONFINITE, kDiverged = NLOT_ROLLOUT_DIVERGED;

    template <int NX, int NU, int G>
    __device__ int inputs_nonfinite(int64_t, int, int) const {
        return 0;
    }
    template <int NX>
    __device__ double start(int64_t, int, double x0) const {
        return x0;
    }
    template <int NX, int NU>
    __device__ void control(const NlotProblem&, int64_t, int k, int, const double* U, const double*, const double*,
                            double* u, int&, int&) const {
#pragma unroll
        for (int i = 0; i < NU; ++i) u[i] = U[(size_t)k * NU + i];
    }
    __device__ void fail(int64_t b, int why) const {
        clearance[b] = deviation[b] = goal_error[b] = NAN;
        where[b] = dev_where[b] = -1;
        flags[b] = why;
    }
    __device__ void store(int64_t b, double best, int bs, int contains, double dev, int dk, double ge, int fl) const {
        if (best < clearance_min) fl |= NLOT_ROLLOUT_COLLISION;
        if (contains) fl |= NLOT_ROLLOUT_CONTAINS;
        if (dev > deviation_tol) fl |= NLOT_ROLLOUT_DEVIATION;
        if (ge > goal_tol) fl |= NLOT_ROLLOUT_GOAL;
        clearance[b] = best;
        where[b] = bs == INT_MAX ? -1 : bs;
        deviation[b] = dev;
        dev_where[b] = dk;
        goal_error[b] = ge;
        flags[b] = fl;
    }
    __device__ void done(int64_t b, double best, int bs, int contains, double dev, int dk, double ge, int) const {
        store(b, best, bs, contains, dev, dk, ge, 0);
    }
};

// nlot_track_batch's law: u_k = clamp(U_k - K_k (x(t_k) - X_k)) from the rolled state at knot k, the roll starts at
// X_0 + dx0; it counts the knots at which the clamp acted and stores the applied controls
struct ClosedLoop : OpenLoop {
    const double* K;
    const double* dx0;
    double* U_applied;
    int32_t* saturated;
    int clamp;

    static_assert(NLOT_TRACK_COLLISION == NLOT_ROLLOUT_COLLISION && NLOT_TRACK_CONTAINS == NLOT_ROLLOUT_CONTAINS &&
                      NLOT_TRACK_DEVIATION == NLOT_ROLLOUT_DEVIATION && NLOT_TRACK_GOAL == NLOT_ROLLOUT_GOAL,
                  "ClosedLoop::done takes these four bits from OpenLoop::store");
    static constexpr int kNonfinite = NLOT_TRACK_NONFINITE, kDiverged = NLOT_TRACK_DIVERGED;

    template <int NX, int NU, int G>
    __device__ int inputs_nonfinite(int64_t b, int N, int j) const {
        int bad = 0;
        if (K) {
            for (int i = j; i < N * NU * NX; i += G) bad |= !isfinite(K[(size_t)b * N * NU * NX + i]);
        }
        if (dx0) {
            for (int i = j; i < NX; i += G) bad |= !isfinite(dx0[(size_t)b * NX + i]);
        }
        return bad;
    }
    template <int NX>
    __device__ double start(int64_t b, int i, double x0) const {
        return dx0 ? x0 + dx0[(size_t)b * NX + i] : x0;
    }
    template <int NX, int NU>
    __device__ void control(const NlotProblem& p, int64_t b, int k, int j, const double* U, const double* x,
                            const double* xk, double* u, int& sat, int& diverged) const {
        int changed = 0;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            double ui = U[(size_t)k * NU + i];
            if (K) {
                const double* Kk = K + (((size_t)b * p.N + k) * NU + i) * NX;
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < NX; ++l) s += Kk[l] * (x[l] - xk[l]);
                ui -= s;
            }
            diverged |= !isfinite(ui);  // fmin / fmax would hide a NaN
            if (clamp) {
                const double uc = fmin(fmax(ui, p.umin[i]), p.umax[i]);
                changed |= uc != ui;
                ui = uc;
            }
            u[i] = ui;
        }
        sat += changed;
        if (U_applied && j == 0) {
#pragma unroll
            for (int i = 0; i < NU; ++i) U_applied[((size_t)b * p.N + k) * NU + i] = u[i];
        }
    }
    __device__ void fail(int64_t b, int why) const {
        saturated[b] = -1;
        OpenLoop::fail(b, why);
    }
    __device__ void done(int64_t b, double best, int bs, int contains, double dev, int dk, double ge, int sat) const {
        saturated[b] = sat;
        store(b, best, bs, contains, dev, dk, ge, sat > 0 ? NLOT_TRACK_SATURATED : 0);
    }
};

template <int D, int G, class Law>
static __global__ __launch_bounds__(kRollBlock) void k_roll(const NlotProblem* __restrict__ pp, Law a) {
    using DY = Dyn<D + NLOT_RK4_BIAS>;
    constexpr int NX = DY::NX, NU = DY::NU;
    const int64_t b = ((int64_t)blockIdx.x * kRollBlock + threadIdx.x) / G;
    if (b >= a.B) return;  // whole groups leave: the shuffles below stay inside a group
    const int j = threadIdx.x & (G - 1);
    const NlotProblem& p = *pp;
    const int N = p.N, sub = a.substeps;
    const double* X = a.X + (size_t)b * (N + 1) * NX;
    const double* U = a.U + (size_t)b * N * NU;
    const double* g = a.xg ? a.xg + (size_t)b * NX : X + (size_t)N * NX;

    // non-finite input: fmin and the comparisons below drop NaNs, so it is tested on its own
    int bad = 0;
    for (int i = j; i < (N + 1) * NX; i += G) bad |= !isfinite(X[i]);
    for (int i = j; i < N * NU; i += G) bad |= !isfinite(U[i]);
    bad |= a.template inputs_nonfinite<NX, NU, G>(b, N, j);
    if (a.xg) {
        for (int i = j; i < NX; i += G) bad |= !isfinite(g[i]);
    }
    if (group_or<G>(bad)) {
        if (j == 0) a.fail(b, Law::kNonfinite);
        return;
    }

    const bool poly = p.shape == NLOT_SHAPE_POLYGON;
    const int per_edge = 1 + a.edge_points;
    const int npp = p.n_obs == 0 ? 0 : poly ? p.n_body * per_edge : 1;  // no scene: no footprint work
    const bool inner = poly && p.n_body >= 3 && p.n_obs > 0;
    const double h = p.dt / (double)sub;
    double* Xr = a.X_roll ? a.X_roll + (size_t)b * (N + 1) * NX : nullptr;

    double x[NX], u[NU] = {}, fe[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = a.template start<NX>(b, i, X[i]);
    double best = INFINITY, dev = 0.0;
    int bs = INT_MAX, dk = 0, contains = 0, diverged = 0, sat = 0;

    // footprint points j, j + G, ... and obstacles j, j + G, ... of pose s (the state x)
    auto visit = [&](int s) {
        double sn = 0.0, cs = 1.0;
        if (poly) sincos(x[2], &sn, &cs);
        for (int q = j; q < npp; q += G) {
            double wx = x[0], wy = x[1];
            if (poly) footprint_point(p, x[0], x[1], sn, cs, q, per_edge, &wx, &wy);
            const double v = exact_sdf(p, wx, wy);
            if (v < best) {  // s ascends: the first pose of the lane's minimum
                best = v;
                bs = s;
            }
        }
        if (inner) obstacles_inside_body(p, x[0], x[1], sn, cs, j, G, contains);
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
        if (k < N) a.template control<NX, NU>(p, b, k, j, U, x, xk, u, sat, diverged);  // held over the interval
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

    group_argmin<G>(best, bs);
    contains = group_or<G>(contains);

    if (j == 0) {
        if (diverged) {
            a.fail(b, Law::kDiverged);
            return;
        }
        a.done(b, best, bs, contains, dev, dk, hypot(x[0] - g[0], x[1] - g[1]), sat);
    }
}

// Launch k_roll on the device copy dP of *prob (check_sample_count's int32 bound holds): G is the lanes per
// instance, one footprint point each
template <int D, class Law>
static void launch_roll(const NlotProblem* prob, const NlotProblem* dP, const Law& a, hipStream_t st) {
    const int npp = prob->shape == NLOT_SHAPE_POLYGON ? prob->n_body * (1 + a.edge_points) : 1;
    const int G = npp <= 1 ? 1 : npp <= 4 ? 4 : npp <= 16 ? 16 : 64;
    const dim3 grid((unsigned)((a.B * G + kRollBlock - 1) / kRollBlock)), block(kRollBlock);
    switch (G) {
        case 1: hipLaunchKernelGGL((k_roll<D, 1, Law>), grid, block, 0, st, dP, a); break;
        case 4: hipLaunchKernelGGL((k_roll<D, 4, Law>), grid, block, 0, st, dP, a); break;
        case 16: hipLaunchKernelGGL((k_roll<D, 16, Law>), grid, block, 0, st, dP, a); break;
        default: hipLaunchKernelGGL((k_roll<D, 64, Law>), grid, block, 0, st, dP, a); break;
    }
}

}  // namespace nlot
