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
// k_track: k_rollout's shape (lane groups of G from the footprint's point count, redundant integration, footprint
// points and obstacles strided over the group, one __shfl_xor reduction at the end, lane 0 stores) with the control
// of every interval computed from the rolled state at its knot.
// Neither kernel uses LDS, scratch or atomics, and nothing is decided from B: an instance's outputs depend on that
// instance's inputs only.
#include <climits>
#include <cmath>

#include "nlot_device.h"
#include "nlot_internal.h"

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

template <int G>
__device__ inline int group_or(int v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

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

struct TrackArgs {
    NlotTrackOptions opt;
    const double* X;
    const double* U;
    const double* K;
    const double* dx0;
    const double* xg;
    double* X_roll;
    double* U_applied;
    double* clearance;
    int32_t* where;
    double* deviation;
    int32_t* dev_where;
    double* goal_error;
    int32_t* saturated;
    int32_t* flags;
    int64_t B;
};

template <int D, int G>
__global__ __launch_bounds__(kBlock) void k_track(const NlotProblem* __restrict__ pp, TrackArgs a) {
    using DY = Dyn<D + NLOT_RK4_BIAS>;
    constexpr int NX = DY::NX, NU = DY::NU;
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    if (b >= a.B) return;  // whole groups leave: the shuffles below stay inside a group
    const int j = threadIdx.x & (G - 1);
    const NlotProblem& p = *pp;
    const int N = p.N, sub = a.opt.substeps;
    const double* X = a.X + (size_t)b * (N + 1) * NX;
    const double* U = a.U + (size_t)b * N * NU;
    const double* K = a.K ? a.K + (size_t)b * N * NU * NX : nullptr;
    const double* d0 = a.dx0 ? a.dx0 + (size_t)b * NX : nullptr;
    const double* g = a.xg ? a.xg + (size_t)b * NX : X + (size_t)N * NX;

    // non-finite input: fmin and the comparisons below drop NaNs, so it is tested on its own
    int bad = 0;
    for (int i = j; i < (N + 1) * NX; i += G) bad |= !isfinite(X[i]);
    for (int i = j; i < N * NU; i += G) bad |= !isfinite(U[i]);
    if (K) {
        for (int i = j; i < N * NU * NX; i += G) bad |= !isfinite(K[i]);
    }
    if (d0) {
        for (int i = j; i < NX; i += G) bad |= !isfinite(d0[i]);
    }
    if (a.xg) {
        for (int i = j; i < NX; i += G) bad |= !isfinite(g[i]);
    }
    if (group_or<G>(bad)) {
        if (j == 0) {
            a.clearance[b] = a.deviation[b] = a.goal_error[b] = NAN;
            a.where[b] = a.dev_where[b] = a.saturated[b] = -1;
            a.flags[b] = NLOT_TRACK_NONFINITE;
        }
        return;
    }

    const bool poly = p.shape == NLOT_SHAPE_POLYGON;
    const int per_edge = 1 + a.opt.edge_points;
    const int npp = p.n_obs == 0 ? 0 : poly ? p.n_body * per_edge : 1;  // no scene: no footprint work
    const bool inner = poly && p.n_body >= 3 && p.n_obs > 0;
    const bool clamp = a.opt.clamp != 0;
    const double h = p.dt / (double)sub;
    double* Xr = a.X_roll ? a.X_roll + (size_t)b * (N + 1) * NX : nullptr;
    double* Ua = a.U_applied ? a.U_applied + (size_t)b * N * NU : nullptr;

    double x[NX], u[NU] = {}, fe[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = d0 ? X[i] + d0[i] : X[i];
    double best = INFINITY, dev = 0.0;
    int bs = INT_MAX, dk = 0, contains = 0, diverged = 0, sat = 0;

    // footprint points j, j + G, ... and obstacles j, j + G, ... of pose s (the state x), as in k_rollout
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
        if (k < N) {  // the feedback law, sampled at the knot and held over the interval
            int changed = 0;
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                double ui = U[(size_t)k * NU + i];
                if (K) {
                    double s = 0.0;
#pragma unroll
                    for (int l = 0; l < NX; ++l) s += K[((size_t)k * NU + i) * NX + l] * (x[l] - xk[l]);
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
            if (Ua && j == 0) {
#pragma unroll
                for (int i = 0; i < NU; ++i) Ua[(size_t)k * NU + i] = u[i];
            }
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
            a.where[b] = a.dev_where[b] = a.saturated[b] = -1;
            a.flags[b] = NLOT_TRACK_DIVERGED;
            return;
        }
        const double ge = hypot(x[0] - g[0], x[1] - g[1]);
        int fl = 0;
        if (best < a.opt.clearance_min) fl |= NLOT_TRACK_COLLISION;
        if (contains) fl |= NLOT_TRACK_CONTAINS;
        if (dev > a.opt.deviation_tol) fl |= NLOT_TRACK_DEVIATION;
        if (ge > a.opt.goal_tol) fl |= NLOT_TRACK_GOAL;
        if (sat > 0) fl |= NLOT_TRACK_SATURATED;
        a.clearance[b] = best;
        a.where[b] = bs == INT_MAX ? -1 : bs;
        a.deviation[b] = dev;
        a.dev_where[b] = dk;
        a.goal_error[b] = ge;
        a.saturated[b] = sat;
        a.flags[b] = fl;
    }
}

template <int D, int G>
void launch_track_dg(const NlotProblem* dP, const TrackArgs& a, hipStream_t st) {
    const unsigned grid = (unsigned)((a.B * G + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((k_track<D, G>), dim3(grid), dim3(kBlock), 0, st, dP, a);
}
template <int D>
void launch_track_d(int G, const NlotProblem* dP, const TrackArgs& a, hipStream_t st) {
    switch (G) {
        case 1: return launch_track_dg<D, 1>(dP, a, st);
        case 4: return launch_track_dg<D, 4>(dP, a, st);
        case 16: return launch_track_dg<D, 16>(dP, a, st);
        default: return launch_track_dg<D, 64>(dP, a, st);
    }
}
template <int D>
void launch_tvlqr_d(const NlotProblem* dP, const TvlqrArgs& a, hipStream_t st) {
    const unsigned grid = (unsigned)((a.B * kLqrGroup + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((k_tvlqr<D>), dim3(grid), dim3(kBlock), 0, st, dP, a);
}

// nlot_rollout_batch's checks of the problem and of B; `who` prefixes the message
bool problem_ok(const NlotProblem* prob, int64_t B, const char* who) {
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
    if (!problem_ok(prob, B, "nlot_tvlqr_batch")) return NLOT_ERR_INVALID;
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
    // the kernel reads the problem through a pointer: a stream-ordered device copy that lives for this call only
    hipStream_t st = (hipStream_t)stream;
    NlotProblem* dP = nullptr;
    NLOT_HIP_CHECK(hipMallocAsync((void**)&dP, sizeof(NlotProblem), st));
    hipError_t e = hipMemcpyAsync(dP, prob, sizeof(NlotProblem), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const TvlqrArgs a{*opt, X, U, K, P0, status, B};
        switch (prob->dynamics) {
            case NLOT_POINT_1ST: launch_tvlqr_d<NLOT_POINT_1ST>(dP, a, st); break;
            case NLOT_POINT_2ND: launch_tvlqr_d<NLOT_POINT_2ND>(dP, a, st); break;
            case NLOT_UNICYCLE: launch_tvlqr_d<NLOT_UNICYCLE>(dP, a, st); break;
            case NLOT_UNICYCLE_2ND: launch_tvlqr_d<NLOT_UNICYCLE_2ND>(dP, a, st); break;
            case NLOT_ACKERMANN: launch_tvlqr_d<NLOT_ACKERMANN>(dP, a, st); break;
            default: launch_tvlqr_d<NLOT_ACKERMANN_2ND>(dP, a, st); break;
        }
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(dP, st);
    NLOT_HIP_CHECK(e);
    NLOT_HIP_CHECK(ef);
    return NLOT_OK;
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
    if (!problem_ok(prob, B, "nlot_track_batch")) return NLOT_ERR_INVALID;
    // the kernel counts poses and footprint points with ints
    const int64_t P = (int64_t)prob->N * opt->substeps + 1;
    const int64_t npp = prob->shape == NLOT_SHAPE_POLYGON ? (int64_t)prob->n_body * (1 + (int64_t)opt->edge_points) : 1;
    if (P > INT32_MAX || npp > INT32_MAX || P * npp > INT32_MAX - 64) {
        set_error("nlot_track_batch: sample count (N substeps + 1) * n_body (1 + edge_points) overflows int32");
        return NLOT_ERR_INVALID;
    }
    if (!X || !U || !clearance || !where || !deviation || !dev_where || !goal_error || !saturated || !flags) {
        set_error("nlot_track_batch: null pointer");
        return NLOT_ERR_INVALID;
    }
    const int G = npp <= 1 ? 1 : npp <= 4 ? 4 : npp <= 16 ? 16 : 64;  // lanes per instance: one footprint point each
    hipStream_t st = (hipStream_t)stream;
    NlotProblem* dP = nullptr;
    NLOT_HIP_CHECK(hipMallocAsync((void**)&dP, sizeof(NlotProblem), st));
    hipError_t e = hipMemcpyAsync(dP, prob, sizeof(NlotProblem), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const TrackArgs a{*opt, X,     U,         K,         dx0,        xg,        X_roll, U_applied,
                          clearance, where, deviation, dev_where, goal_error, saturated, flags,  B};
        switch (prob->dynamics) {
            case NLOT_POINT_1ST: launch_track_d<NLOT_POINT_1ST>(G, dP, a, st); break;
            case NLOT_POINT_2ND: launch_track_d<NLOT_POINT_2ND>(G, dP, a, st); break;
            case NLOT_UNICYCLE: launch_track_d<NLOT_UNICYCLE>(G, dP, a, st); break;
            case NLOT_UNICYCLE_2ND: launch_track_d<NLOT_UNICYCLE_2ND>(G, dP, a, st); break;
            case NLOT_ACKERMANN: launch_track_d<NLOT_ACKERMANN>(G, dP, a, st); break;
            default: launch_track_d<NLOT_ACKERMANN_2ND>(G, dP, a, st); break;
        }
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(dP, st);
    NLOT_HIP_CHECK(e);
    NLOT_HIP_CHECK(ef);
    return NLOT_OK;
}
