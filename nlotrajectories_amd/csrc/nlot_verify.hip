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
#include <climits>
#include <cmath>

#include "nlot_device.h"
#include "nlot_internal.h"

namespace nlot {
namespace {

constexpr int kWavesPerBlock = 4;

__device__ inline int wave_or(int v) {
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
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
    switch (p.dynamics + (p.integrator == NLOT_INTEG_RK4 ? NLOT_RK4_BIAS : 0)) {
        case NLOT_POINT_1ST: return interval_defect<NLOT_POINT_1ST>(p, xk, xk1, uk);
        case NLOT_POINT_2ND: return interval_defect<NLOT_POINT_2ND>(p, xk, xk1, uk);
        case NLOT_UNICYCLE: return interval_defect<NLOT_UNICYCLE>(p, xk, xk1, uk);
        case NLOT_UNICYCLE_2ND: return interval_defect<NLOT_UNICYCLE_2ND>(p, xk, xk1, uk);
        case NLOT_ACKERMANN: return interval_defect<NLOT_ACKERMANN>(p, xk, xk1, uk);
        case NLOT_ACKERMANN_2ND: return interval_defect<NLOT_ACKERMANN_2ND>(p, xk, xk1, uk);
        case NLOT_POINT_1ST + NLOT_RK4_BIAS: return interval_defect<NLOT_POINT_1ST + NLOT_RK4_BIAS>(p, xk, xk1, uk);
        case NLOT_POINT_2ND + NLOT_RK4_BIAS: return interval_defect<NLOT_POINT_2ND + NLOT_RK4_BIAS>(p, xk, xk1, uk);
        case NLOT_UNICYCLE + NLOT_RK4_BIAS: return interval_defect<NLOT_UNICYCLE + NLOT_RK4_BIAS>(p, xk, xk1, uk);
        case NLOT_UNICYCLE_2ND + NLOT_RK4_BIAS: return interval_defect<NLOT_UNICYCLE_2ND + NLOT_RK4_BIAS>(p, xk, xk1, uk);
        case NLOT_ACKERMANN + NLOT_RK4_BIAS: return interval_defect<NLOT_ACKERMANN + NLOT_RK4_BIAS>(p, xk, xk1, uk);
        default: return interval_defect<NLOT_ACKERMANN_2ND + NLOT_RK4_BIAS>(p, xk, xk1, uk);
    }
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
    if (wave_or(bad)) {
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
        if (poly) {  // PolygonGeometry.transform of corners i, i + 1, then densify_polygon's (1 - t) p0 + t p1
            const int i = j / per_edge, m = j - i * per_edge, i1 = i + 1 < p.n_body ? i + 1 : 0;
            double sn, cs;
            sincos(th, &sn, &cs);
            const double ax = px + cs * p.body[i][0] - sn * p.body[i][1], ay = py + sn * p.body[i][0] + cs * p.body[i][1];
            wx = ax;
            wy = ay;
            if (m > 0) {
                const double bx = px + cs * p.body[i1][0] - sn * p.body[i1][1];
                const double by = py + sn * p.body[i1][0] + cs * p.body[i1][1];
                const double t = (double)m / (double)per_edge;
                wx = (1.0 - t) * ax + t * bx;
                wy = (1.0 - t) * ay + t * by;
            }
        }
        const double v = exact_sdf(p, wx, wy);
        if (v < best) {  // s ascends within a lane: the first pose of the lane's minimum
            best = v;
            bs = s;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off);
        const int os = __shfl_xor(bs, off);
        if (ov < best || (ov == best && os < bs)) {
            best = ov;
            bs = os;
        }
    }

    // containment: an obstacle smaller than the footprint can sit inside it with every perimeter point outside
    int contains = 0;
    if (poly && p.n_body >= 3) {
        for (int s = lane; s < P; s += 64) {
            double px, py, th, sn, cs;
            sample_pose(X, nx, N, sub, s, true, &px, &py, &th);
            sincos(th, &sn, &cs);
            for (int i = 0; i < p.n_obs; ++i) {
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
        contains = wave_or(contains);
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
    static const int kNx[6] = {4, 4, 3, 5, 4, 7};
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
    if (prob->dynamics < 0 || prob->dynamics > NLOT_ACKERMANN_2ND || prob->nx != kNx[prob->dynamics] || prob->nu != 2 ||
        prob->N < 1 || prob->N > 1 << 24 || prob->n_obs < 0 || prob->n_obs > NLOT_MAX_OBS || prob->n_verts < 0 ||
        prob->n_verts > NLOT_MAX_VERTS || (prob->shape != NLOT_SHAPE_DOT && prob->shape != NLOT_SHAPE_POLYGON) ||
        (prob->shape == NLOT_SHAPE_POLYGON && (prob->n_body < 1 || prob->n_body > NLOT_MAX_BODY))) {
        set_error("nlot_verify_batch: invalid problem (dynamics, nx / nu, 1 <= N <= 2^24, shape, n_body, n_obs, n_verts)");
        return NLOT_ERR_INVALID;
    }
    for (int i = 0; i < prob->n_obs; ++i) {
        const NlotObstacle& q = prob->obs[i];
        if (q.type < NLOT_OBS_CIRCLE || q.type > NLOT_OBS_TRAPEZOID) {
            set_error("nlot_verify_batch: unknown obstacle type");
            return NLOT_ERR_INVALID;
        }
        if ((q.type == NLOT_OBS_POLYGON || q.type == NLOT_OBS_TRAPEZOID) &&
            (q.v0 < 0 || q.nv < 2 || q.v0 > prob->n_verts - q.nv)) {
            set_error("nlot_verify_batch: polygon vertex range outside verts[0, n_verts)");
            return NLOT_ERR_INVALID;
        }
    }
    if (B < 1 || B > (int64_t)1 << 26) {
        set_error("nlot_verify_batch: B out of range");
        return NLOT_ERR_INVALID;
    }
    {  // the kernel indexes the (pose, footprint point) samples of an instance with an int
        const int64_t P = (int64_t)prob->N * opt->sub + 1;
        const int64_t npp = prob->shape == NLOT_SHAPE_POLYGON ? (int64_t)prob->n_body * (1 + (int64_t)opt->edge_points) : 1;
        if (P > INT32_MAX || npp > INT32_MAX || P * npp > INT32_MAX - 64) {
            set_error("nlot_verify_batch: sample count (N sub + 1) * n_body (1 + edge_points) overflows int32");
            return NLOT_ERR_INVALID;
        }
    }
    if ((x0 == nullptr) != (xg == nullptr)) {
        set_error("nlot_verify_batch: x0 and xg must both be given or both be NULL");
        return NLOT_ERR_INVALID;
    }
    if (!X || !U || !clearance || !where || !defect || !ubound || !boundary || !flags) {
        set_error("nlot_verify_batch: null pointer");
        return NLOT_ERR_INVALID;
    }
    // the kernel reads the problem through a pointer (it is larger than the kernel-argument area): a stream-ordered
    // device copy that lives for this call only — no workspace argument, no global state
    hipStream_t st = (hipStream_t)stream;
    NlotProblem* dP = nullptr;
    NLOT_HIP_CHECK(hipMallocAsync((void**)&dP, sizeof(NlotProblem), st));
    hipError_t e = hipMemcpyAsync(dP, prob, sizeof(NlotProblem), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)((B + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL(k_verify, dim3(grid), dim3(64 * kWavesPerBlock), 0, st, dP, *opt, X, U, x0, xg, clearance,
                           where, defect, ubound, boundary, flags, B);
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(dP, st);
    NLOT_HIP_CHECK(e);
    NLOT_HIP_CHECK(ef);
    return NLOT_OK;
}
