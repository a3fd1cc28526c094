// Time-varying LQR gains about a plan (nlot_tvlqr_batch) and the closed-loop tracking rollout that uses them
// (nlot_track_batch, include/nlot.h) for gfx950.  DESIGN.md §13.
//
// k_tvlqr: the Riccati sweep is sequential in k and its matrices are at most 7 x 7, so a wave per instance would idle
// and a thread per instance could not hold them.  A group of 16 lanes serves one instance, 4 instances per wave:
//   * lane j < nx + nu pushes the tangent e_j through one RK4 step with first-order dual numbers (Du below, through
//     the solver's own fgen / rk4_feff), so it owns column j of [A B]; lanes past nx + nu carry a zero tangent and
//     run the same instructions;
//   * P is held column per lane (lane j < nx: P[.][j]).  M = P [A B], S = R + B^T P B, K, W = P (A - B K) and the new
//     P = Q + A^T W are sums over __shfl reads inside the group; the new P is symmetrised by computing P[i][j] and
//     P[j][i] in the same lane (the second from shuffled W), so no register array is indexed by the lane id;
//   * every lane stores its own column of K (and of P_0), so the zeros a diverged instance gets are written by the
//     thread that wrote the gains.
// nlot_track_batch has no kernel of its own here: it is the rollout kernel k_roll<D, G, ClosedLoop> of nlot_roll.h
// (nlot_rollout_batch's, with the control of every interval computed from the rolled state at its knot); this unit
// holds its C entry point and dispatch.
// Neither kernel uses LDS, scratch or atomics, and nothing is decided from B: an instance's outputs depend on that
// instance's inputs only.
#include "nlot_roll.h"

namespace nlot {

// first-order dual number (value, one tangent) with the scalar helpers fgen / rk4_feff are written in
struct Du {
    double v, d;
};
__device__ inline Du operator+(const Du& a, const Du& b) { return {a.v + b.v, a.d + b.d}; }
__device__ inline Du operator*(const Du& a, double c) { return {a.v * c, a.d * c}; }
__device__ inline Du operator*(const Du& a, const Du& b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ inline Du tsin(const Du& a) {
    double s, c;
    sincos(a.v, &s, &c);
    return {s, c * a.d};
}
__device__ inline Du tcos(const Du& a) {
    double s, c;
    sincos(a.v, &s, &c);
    return {c, -s * a.d};
}
__device__ inline Du ttan(const Du& a) {
    const double t = tan(a.v);
    return {t, (1.0 + t * t) * a.d};
}
__device__ inline Du trecip(const Du& a) {
    const double r = 1.0 / a.v;
    return {r, -(r * r) * a.d};
}
__device__ inline Du taddc(const Du& a, double c) { return {a.v + c, a.d}; }
__device__ inline Du tconst(double c, const Du&) { return {c, 0.0}; }

namespace {

constexpr int kBlock = 256;
constexpr int kLqrGroup = 16;  // lanes per instance of k_tvlqr: nx + nu <= 9 columns of [A B]

struct TvlqrArgs {
    NlotTvlqrOptions opt;
    const double* X;
    const double* U;
    double* K;
    double* P0;
    int32_t* status;
    int64_t B;
};

template <int D>
__global__ __launch_bounds__(kBlock) void k_tvlqr(const NlotProblem* __restrict__ pp, TvlqrArgs a) {
    using DY = Dyn<D>;
    constexpr int NX = DY::NX, NU = DY::NU, G = kLqrGroup;
    static_assert(NU == 2 && NX + NU <= G && NX <= NLOT_MAX_NX, "k_tvlqr: 2 controls, one lane per column of [A B]");
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    if (b >= a.B) return;  // whole groups leave: the shuffles below stay inside a group
    const int j = threadIdx.x & (G - 1);
    const NlotProblem& p = *pp;
    const int N = p.N;
    const double dt = p.dt, L = p.wheelbase;
    const double* X = a.X + (size_t)b * (N + 1) * NX;
    const double* U = a.U + (size_t)b * N * NU;
    double* K = a.K + (size_t)b * N * NU * NX;
    double* P0 = a.P0 ? a.P0 + (size_t)b * NX * NX : nullptr;

    int bad = 0;
    for (int i = j; i < (N + 1) * NX; i += G) bad |= !isfinite(X[i]);
    for (int i = j; i < N * NU; i += G) bad |= !isfinite(U[i]);
    const bool nonfinite = group_or<G>(bad) != 0;

    // this lane's diagonal entries of Q, Qf (columns j < NX) and the 2 x 2 R, by compile-time indices only
    double qj = 0.0, qfj = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        if (i == j) {
            qj = a.opt.q[i];
            qfj = a.opt.qf[i];
        }
    }
    const double r0 = a.opt.r[0], r1 = a.opt.r[1];

    double pc[NX];  // column j of P (zero in the lanes past NX)
#pragma unroll
    for (int i = 0; i < NX; ++i) pc[i] = i == j ? qfj : 0.0;

    bad = 0;
    for (int k = nonfinite ? -1 : N - 1; k >= 0; --k) {
        // column j of [A B] at (X_k, U_k): the tangent of one RK4 step in direction e_j
        Du xd[NX], ud[NU], fe[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) xd[i] = {X[(size_t)k * NX + i], i == j ? 1.0 : 0.0};
#pragma unroll
        for (int i = 0; i < NU; ++i) ud[i] = {U[(size_t)k * NU + i], NX + i == j ? 1.0 : 0.0};
        rk4_feff<D, NX>(xd, ud, dt, L, fe);
        double c[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) c[i] = (i == j ? 1.0 : 0.0) + dt * fe[i].d;

        // M = P [A B], column j:  m[i] = sum_l P[i][l] c[l], P[i][l] = P[l][i] = entry l of lane i's column
        double m[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            double s = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) s += __shfl(pc[l], i, G) * c[l];
            m[i] = s;
        }
        // g = B^T M, column j: B^T P A in the lanes j < NX, B^T P B in the lanes NX, NX + 1
        double g0 = 0.0, g1 = 0.0;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            g0 += __shfl(c[i], NX, G) * m[i];
            g1 += __shfl(c[i], NX + 1, G) * m[i];
        }
        const double s00 = r0 + __shfl(g0, NX, G), s01 = __shfl(g0, NX + 1, G);
        const double s10 = __shfl(g1, NX, G), s11 = r1 + __shfl(g1, NX + 1, G);
        const double det = s00 * s11 - s01 * s10;
        // K = S^-1 B^T P A, column j (meaningful in the lanes j < NX)
        const double k0 = (s11 * g0 - s01 * g1) / det, k1 = (s00 * g1 - s10 * g0) / det;
        // W = P (A - B K) = M_A - M_B K, column j
        double w[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) w[i] = m[i] - __shfl(m[i], NX, G) * k0 - __shfl(m[i], NX + 1, G) * k1;
        // P = Q + A^T W, symmetrised: P[i][j] = sum_l A[l][i] W[l][j] from this lane's w and lane i's c, P[j][i] from
        // this lane's c and lane i's w
        int nf = !(det > 0.0) || !isfinite(det);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            double pij = 0.0, pji = 0.0;
#pragma unroll
            for (int l = 0; l < NX; ++l) {
                pij += __shfl(c[l], i, G) * w[l];
                pji += c[l] * __shfl(w[l], i, G);
            }
            pc[i] = (i == j ? qj : 0.0) + 0.5 * (pij + pji);
            nf |= !isfinite(pc[i]);
        }
        nf |= !isfinite(k0) || !isfinite(k1);
        if (j < NX) {
            bad |= nf;
            K[((size_t)k * NU + 0) * NX + j] = k0;
            K[((size_t)k * NU + 1) * NX + j] = k1;
        } else {
#pragma unroll
            for (int i = 0; i < NX; ++i) pc[i] = 0.0;
        }
    }

    const bool diverged = group_or<G>(bad) != 0;
    if (j < NX) {
        if (nonfinite || diverged) {  // open loop: every lane zeroes the gains it wrote
            for (int k = 0; k < N; ++k) K[((size_t)k * NU + 0) * NX + j] = K[((size_t)k * NU + 1) * NX + j] = 0.0;
        }
        if (P0) {
#pragma unroll
            for (int i = 0; i < NX; ++i) P0[(size_t)i * NX + j] = nonfinite || diverged ? NAN : pc[i];
        }
    }
    if (j == 0) a.status[b] = nonfinite ? NLOT_TVLQR_NONFINITE : diverged ? NLOT_TVLQR_DIVERGED : 0;
}

}  // namespace
}  // namespace nlot

extern "C" void nlot_default_tvlqr_options(NlotTvlqrOptions* opt) {
    if (!opt) return;
    for (int i = 0; i < NLOT_MAX_NX; ++i) opt->q[i] = opt->qf[i] = 1.0;
    for (int i = 0; i < NLOT_MAX_NU; ++i) opt->r[i] = 1.0;
}

extern "C" void nlot_default_track_options(NlotTrackOptions* opt) {
    if (!opt) return;
    opt->substeps = 8;
    opt->edge_points = 3;
    opt->clamp = 1;
    opt->pad_ = 0;
    opt->clearance_min = 0.0;
    opt->deviation_tol = INFINITY;
    opt->goal_tol = INFINITY;
}

extern "C" int32_t nlot_tvlqr_batch(const NlotProblem* prob, const NlotTvlqrOptions* opt, const double* X, const double* U,
                                    double* K, double* P0, int32_t* status, int64_t B, void* stream) {
    using namespace nlot;
    if (!prob || !opt) {
        set_error("nlot_tvlqr_batch: null problem or options");
        return NLOT_ERR_INVALID;
    }
    if (!check_problem(prob, B, "nlot_tvlqr_batch")) return NLOT_ERR_INVALID;
    for (int i = 0; i < prob->nx; ++i) {
        if (!(opt->q[i] >= 0.0) || !std::isfinite(opt->q[i]) || !(opt->qf[i] >= 0.0) || !std::isfinite(opt->qf[i])) {
            set_error("nlot_tvlqr_batch: q and qf must be finite and >= 0");
            return NLOT_ERR_INVALID;
        }
    }
    for (int i = 0; i < prob->nu; ++i) {
        if (!(opt->r[i] > 0.0) || !std::isfinite(opt->r[i])) {
            set_error("nlot_tvlqr_batch: r must be finite and > 0");
            return NLOT_ERR_INVALID;
        }
    }
    if (!X || !U || !K || !status) {
        set_error("nlot_tvlqr_batch: null pointer");
        return NLOT_ERR_INVALID;
    }
    const TvlqrArgs a{*opt, X, U, K, P0, status, B};
    hipStream_t st = (hipStream_t)stream;
    return with_device_problem(prob, st, [&](const NlotProblem* dP) {
        const dim3 grid((unsigned)((B * kLqrGroup + kBlock - 1) / kBlock)), block(kBlock);
        dispatch_dynamics(prob->dynamics, [&](auto d) {
            hipLaunchKernelGGL((k_tvlqr<decltype(d)::value>), grid, block, 0, st, dP, a);
        });
    });
}

extern "C" int32_t nlot_track_batch(const NlotProblem* prob, const NlotTrackOptions* opt, const double* X, const double* U,
                                    const double* K, const double* dx0, const double* xg, double* X_roll,
                                    double* U_applied, double* clearance, int32_t* where, double* deviation,
                                    int32_t* dev_where, double* goal_error, int32_t* saturated, int32_t* flags, int64_t B,
                                    void* stream) {
    using namespace nlot;
    if (!prob || !opt) {
        set_error("nlot_track_batch: null problem or options");
        return NLOT_ERR_INVALID;
    }
    if (opt->substeps < 1) {
        set_error("nlot_track_batch: substeps must be >= 1");
        return NLOT_ERR_INVALID;
    }
    if (opt->edge_points < 0) {
        set_error("nlot_track_batch: edge_points must be >= 0");
        return NLOT_ERR_INVALID;
    }
    if (!check_problem(prob, B, "nlot_track_batch") ||
        !check_sample_count(prob, opt->substeps, opt->edge_points, "nlot_track_batch", "substeps"))
        return NLOT_ERR_INVALID;
    if (!X || !U || !clearance || !where || !deviation || !dev_where || !goal_error || !saturated || !flags) {
        set_error("nlot_track_batch: null pointer");
        return NLOT_ERR_INVALID;
    }
    const ClosedLoop a{{opt->substeps, opt->edge_points, opt->clearance_min, opt->deviation_tol, opt->goal_tol, X, U, xg,
                        X_roll, clearance, where, deviation, dev_where, goal_error, flags, B},
                       K, dx0, U_applied, saturated, opt->clamp};
    hipStream_t st = (hipStream_t)stream;
    return with_device_problem(prob, st, [&](const NlotProblem* dP) {
        dispatch_dynamics(prob->dynamics, [&](auto d) { launch_roll<decltype(d)::value>(prob, dP, a, st); });
    });
}
