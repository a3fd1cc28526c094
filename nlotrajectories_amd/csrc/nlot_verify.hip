// Batched trajectory verification against the exact scene (nlot_verify_batch, include/nlot.h) for gfx950.
//
// One wavefront per instance, fp64 throughout, four instances per 256-thread block (the waves of a block do not
// talk to each other: no LDS, no barrier, so the waves past B in the last block simply leave).  Per instance:
//   * clearance: the lanes stride over the flat (pose, footprint point) index, evaluate the scene's exact SDF
//     (exact_sdf of nlot_device.h, the function the RRT plans against) and min-reduce (value, pose index), the lowest
//     pose index on exact ties;
//   * containment (polygon bodies): the lanes stride over the poses and test every obstacle's centre / vertices
//     for being strictly inside the footprint;
//   * residuals: the lanes stride over the intervals and max-reduce the defect of the problem's own defect map
//     (Dyn<D>::f of nlot_device.h, Euler or RK4) and the control-bound violation; the boundary residual is nx
//     values.
// The obstacle data is read through the kernel's NlotProblem pointer with wave-uniform indices, i.e. on the
// scalar-load path, as k_rrt does.
#include "nlot_roll.h"

namespace nlot {
namespace {

constexpr int kWavesPerBlock = 4;

__device__ inline double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// max_i |x_{k+1,i} - (x_k + dt f(x_k, u_k))_i| of interval k for the instantiation DYN (Euler: the dynamics id;
// RK4: id + NLOT_RK4_BIAS, whose f is the effective rate), the solver's defect (nlot_solver.hip)
template <int DYN>
__device__ double interval_defect(const NlotProblem& p, const double* xk, const double* xk1, const double* uk) {
    constexpr int NX = Dyn<DYN>::NX, NU = Dyn<DYN>::NU;
    double x[NX], u[NU], f[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = xk[i];
#pragma unroll
    for (int i = 0; i < NU; ++i) u[i] = uk[i];
    Dyn<DYN>::f(x, u, p.wheelbase, f, p.dt);
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) d = fmax(d, fabs(xk1[i] - (x[i] + p.dt * f[i])));
    return d;
}

__device__ double interval_defect_any(const NlotProblem& p, const double* xk, const double* xk1, const double* uk) {
    if (p.integrator == NLOT_INTEG_RK4)
        return dispatch_dynamics(p.dynamics, [&](auto d) {
            return interval_defect<decltype(d)::value + NLOT_RK4_BIAS>(p, xk, xk1, uk);
        });
    return dispatch_dynamics(p.dynamics, [&](auto d) { return interval_defect<decltype(d)::value>(p, xk, xk1, uk); });
}

// pose s of the P = N sub + 1 sampled ones: x_k + tau (x_{k+1} - x_k), k = s / sub, tau = (s mod sub) / sub; the
// last one is knot N.  Components 0, 1 and (polygon body) 2, the heading interpolated without wrapping.
__device__ inline void sample_pose(const double* X, int nx, int N, int sub, int s, bool heading, double* px,
                                   double* py, double* th) {
    const int k = s / sub, r = s - k * sub;
    const double* a = X + (size_t)k * nx;
    if (k >= N || r == 0) {
        *px = a[0];
        *py = a[1];
        *th = heading ? a[2] : 0.0;
        return;
    }
    const double tau = (double)r / (double)sub;
    const double* b = a + nx;
    *px = a[0] + tau * (b[0] - a[0]);
    *py = a[1] + tau * (b[1] - a[1]);
    *th = heading ? a[2] + tau * (b[2] - a[2]) : 0.0;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_verify(
    const NlotProblem* __restrict__ pp, NlotVerifyOptions o, const double* __restrict__ Xall,
    const double* __restrict__ Uall, const double* __restrict__ x0, const double* __restrict__ xg,
    double* __restrict__ clearance, int32_t* __restrict__ where, double* __restrict__ defect,
    double* __restrict__ ubound, double* __restrict__ boundary, int32_t* __restrict__ flags, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (b >= B) return;  // whole waves leave: nothing below synchronises across waves
    const int lane = threadIdx.x & 63;
    const NlotProblem& p = *pp;
    const int nx = p.nx, nu = p.nu, N = p.N, sub = o.sub;
    const double* X = Xall + (size_t)b * (N + 1) * nx;
    const double* U = Uall + (size_t)b * N * nu;

    // non-finite input: fmin / fmax drop NaNs, so it is tested on its own
    int bad = 0;
    for (int i = lane; i < (N + 1) * nx; i += 64) bad |= !isfinite(X[i]);
    for (int i = lane; i < N * nu; i += 64) bad |= !isfinite(U[i]);
    if (x0) {
        for (int i = lane; i < nx; i += 64) bad |= !isfinite(x0[b * nx + i]) || !isfinite(xg[b * nx + i]);
    }
    if (group_or<64>(bad)) {
        if (lane == 0) {
            clearance[b] = defect[b] = ubound[b] = boundary[b] = NAN;
            where[b] = -1;
            flags[b] = NLOT_VERIFY_NONFINITE;
        }
        return;
    }

    // clearance over the flat (pose, footprint point) index
    const bool poly = p.shape == NLOT_SHAPE_POLYGON;
    const int per_edge = 1 + o.edge_points;
    const int npp = poly ? p.n_body * per_edge : 1;
    const int P = N * sub + 1;
    const int total = P * npp;  // the host refuses a count beyond int32
    double best = INFINITY;
    int bs = INT_MAX;
    for (int idx = lane; idx < total; idx += 64) {
        const int s = idx / npp, j = idx - s * npp;
        double px, py, th;
        sample_pose(X, nx, N, sub, s, poly, &px, &py, &th);
        double wx = px, wy = py;
        if (poly) {
            double sn, cs;
            sincos(th, &sn, &cs);
            footprint_point(p, px, py, sn, cs, j, per_edge, &wx, &wy);
        }
        const double v = exact_sdf(p, wx, wy);
        if (v < best) {  // s ascends within a lane: the first pose of the lane's minimum
            best = v;
            bs = s;
        }
    }
    group_argmin<64>(best, bs);

    // containment: an obstacle smaller than the footprint can sit inside it with every perimeter point outside
    int contains = 0;
    if (poly && p.n_body >= 3) {
        for (int s = lane; s < P; s += 64) {
            double px, py, th, sn, cs;
            sample_pose(X, nx, N, sub, s, true, &px, &py, &th);
            sincos(th, &sn, &cs);
            obstacles_inside_body(p, px, py, sn, cs, 0, 1, contains);
        }
        contains = group_or<64>(contains);
    }

    // residuals
    double dmax = 0.0, umax = 0.0;
    for (int k = lane; k < N; k += 64) {
        const double* xk = X + (size_t)k * nx;
        const double* uk = U + (size_t)k * nu;
        dmax = fmax(dmax, interval_defect_any(p, xk, xk + nx, uk));
        for (int i = 0; i < nu; ++i) umax = fmax(umax, fmax(fmax(p.umin[i] - uk[i], uk[i] - p.umax[i]), 0.0));
    }
    dmax = wave_max(dmax);
    umax = wave_max(umax);
    double bnd = 0.0;
    if (x0) {  // runner.py:50-56: the start state in full, the goal without component 2 unless enforce_heading
        for (int i = lane; i < nx; i += 64) {
            bnd = fmax(bnd, fabs(X[i] - x0[b * nx + i]));
            if (i != 2 || p.enforce_heading) bnd = fmax(bnd, fabs(X[(size_t)N * nx + i] - xg[b * nx + i]));
        }
        bnd = wave_max(bnd);
    }

    if (lane == 0) {
        int fl = 0;
        if (best < o.clearance_min) fl |= NLOT_VERIFY_COLLISION;
        if (contains) fl |= NLOT_VERIFY_CONTAINS;
        if (dmax > o.defect_tol) fl |= NLOT_VERIFY_DEFECT;
        if (umax > o.bound_tol) fl |= NLOT_VERIFY_UBOUND;
        if (bnd > o.bound_tol) fl |= NLOT_VERIFY_BOUNDARY;
        clearance[b] = best;
        where[b] = bs == INT_MAX ? -1 : bs;
        defect[b] = dmax;
        ubound[b] = umax;
        boundary[b] = bnd;
        flags[b] = fl;
    }
}

}  // namespace
}  // namespace nlot

extern "C" void nlot_default_verify_options(NlotVerifyOptions* opt) {
    if (!opt) return;
    opt->sub = 8;
    opt->edge_points = 3;
    opt->clearance_min = 0.0;
    opt->defect_tol = 1e-4;
    opt->bound_tol = 1e-4;
}

extern "C" int32_t nlot_verify_batch(const NlotProblem* prob, const NlotVerifyOptions* opt, const double* X,
                                     const double* U, const double* x0, const double* xg, double* clearance,
                                     int32_t* where, double* defect, double* ubound, double* boundary, int32_t* flags,
                                     int64_t B, void* stream) {
    using namespace nlot;
    if (!prob || !opt) {
        set_error("nlot_verify_batch: null problem or options");
        return NLOT_ERR_INVALID;
    }
    if (opt->sub < 1) {
        set_error("nlot_verify_batch: sub must be >= 1");
        return NLOT_ERR_INVALID;
    }
    if (opt->edge_points < 0) {
        set_error("nlot_verify_batch: edge_points must be >= 0");
        return NLOT_ERR_INVALID;
    }
    if (prob->n_obs == 0) {
        set_error("nlot_verify_batch: the problem carries no scene (n_obs == 0)");
        return NLOT_ERR_INVALID;
    }
    if (!check_problem(prob, B, "nlot_verify_batch") ||
        !check_sample_count(prob, opt->sub, opt->edge_points, "nlot_verify_batch", "sub"))
        return NLOT_ERR_INVALID;
    if ((x0 == nullptr) != (xg == nullptr)) {
        set_error("nlot_verify_batch: x0 and xg must both be given or both be NULL");
        return NLOT_ERR_INVALID;
    }
    if (!X || !U || !clearance || !where || !defect || !ubound || !boundary || !flags) {
        set_error("nlot_verify_batch: null pointer");
        return NLOT_ERR_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    return with_device_problem(prob, st, [&](const NlotProblem* dP) {
        const unsigned grid = (unsigned)((B + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL(k_verify, dim3(grid), dim3(64 * kWavesPerBlock), 0, st, dP, *opt, X, U, x0, xg, clearance,
                           where, defect, ubound, boundary, flags, B);
    });
}
