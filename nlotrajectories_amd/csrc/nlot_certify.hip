// Certified clearance of B plans by Lipschitz branch-and-bound (nlot_certify_batch, include/nlot.h) for gfx950.
//
// The domain of one instance is every instant of the interpolated motion (interval k, tau in [0, 1]) times the
// footprint's boundary (edge i, t in [0, 1]; a dot has one "edge" of length 0).  f = the scene's exact SDF at
// pos(tau) + R(theta(tau)) c(t) is 1-Lipschitz in the point, and every point of a box with centre (tau_c, t_c) and
// half-widths (h_tau, h_t) lies within
//     r = h_tau (|dxy_k| + rho_i |dtheta_k|) + h_t L_i
// of the centre point, so f >= f(centre) - r on the box.
//
// One wavefront per instance, fp64 throughout, two instances per 128-thread block: a wave's only memory besides its
// registers is its own box stack in LDS, kCertCap boxes of 16 bytes = 16 KB, so a block takes 32 KB and five blocks
// (ten waves) are resident per CU; the waves of a block never synchronise (whole waves past B leave).  Per instance:
//   * seed: the lanes stride over the knot x corner samples (nlot_verify_batch's sub = 1, edge_points = 0 set) and
//     min-reduce the upper bound U with its witness (k, tau), the lowest on exact ties;
//   * rounds: the stack is LIFO.  When fewer than 64 boxes are stacked it is topped up with the next unseeded
//     (interval, edge) boxes at full width, so memory does not grow with N.  A round pops up to 64 boxes, one per
//     lane; each lane evaluates f at its centre; U is min-reduced; a box retires with L = min(L, v - r) when
//     v - r >= U - tol (with `decide` also when v - r >= clearance_min), else it is bisected along the dimension with
//     the larger share of r and both children are pushed at 2 x (the lane's rank in the ballot of splitting lanes):
//     the order depends on nothing but the instance;
//   * the refining loop ends when stack and seeds are exhausted, when max_evals evaluations are spent, when the next
//     push could overflow the stack, or (decide) when U < clearance_min.  In the last three cases the drain evaluates
//     every box still stacked and every unseeded box once and retires it with its own v - r, no splitting.  Every
//     round spends at least one evaluation, so the rounds are bounded by max_evals and the whole instance by
//     max_evals + kCertCap + N n_edges + (N + 1) n_corners evaluations.
// Results depend on kCertCap and kCertMaxDepth only through NLOT_CERTIFY_BUDGET: a box whose dimensions are all at
// kCertMaxDepth bisections (positions are 31-bit integers) retires with its own bound and sets that flag too.
// The obstacle loop inside exact_sdf is wave-uniform (inactive lanes recompute the round's last box rather than
// branch around it), so obs[i] / verts[e] stay on the scalar-load path as in k_verify.  No matrix product, no MFMA.
#include "nlot_roll.h"

namespace nlot {
namespace {

constexpr int kCertWaves = 2;       // waves per block
constexpr int kCertCap = 1024;      // boxes per wave's stack
constexpr int kCertMaxDepth = 30;   // bisections per dimension
static_assert(kCertCap >= 128, "a round pushes up to 128 boxes");

// LDS written by some lanes of the wave is read by others: order the accesses within the wavefront
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a box: x = interval k, y = edge | tau depth << 8 | t depth << 16, z / w = integer positions in tau / t: the box is
// [z, z + 1] 2^-dtau x [w, w + 1] 2^-dt
__device__ inline uint4 make_box(int k, int e, int dq, int dt, unsigned iq, unsigned it) {
    return make_uint4((unsigned)k, (unsigned)e | (unsigned)dq << 8 | (unsigned)dt << 16, iq, it);
}

// (v, k, tau) of the wave's least v, the lowest (k, tau) on exact ties; lanes without a sample pass v = +inf
__device__ inline void wave_witness(double& v, int& k, double& tau) {
    const double v0 = v;
    const int k0 = k;
    group_argmin<64>(v, k);
    double t = (v0 == v && k0 == k) ? tau : INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t = fmin(t, __shfl_xor(t, o));
    tau = t;
}

struct Witness {
    double v;
    int k;
    double tau;
    __device__ void take(double ov, int ok, double otau) {
        if (ov < v || (ov == v && (ok < k || (ok == k && otau < tau)))) {
            v = ov;
            k = ok;
            tau = otau;
        }
    }
};

__global__ __launch_bounds__(64 * kCertWaves) void k_certify(
    const NlotProblem* __restrict__ pp, NlotCertifyOptions o, const double* __restrict__ Xall,
    double* __restrict__ lower, double* __restrict__ upper, int32_t* __restrict__ where, double* __restrict__ tau_out,
    int32_t* __restrict__ evals_out, int32_t* __restrict__ flags, int64_t B) {
    __shared__ uint4 stacks[kCertWaves][kCertCap];
    const int64_t b = (int64_t)blockIdx.x * kCertWaves + (threadIdx.x >> 6);
    if (b >= B) return;  // whole waves leave: nothing below synchronises across waves
    const int lane = threadIdx.x & 63;
    uint4* stack = stacks[threadIdx.x >> 6];
    const NlotProblem& p = *pp;
    const int nx = p.nx, N = p.N;
    const double* X = Xall + (size_t)b * (N + 1) * nx;

    int bad = 0;
    for (int i = lane; i < (N + 1) * nx; i += 64) bad |= !isfinite(X[i]);
    if (group_or<64>(bad)) {
        if (lane == 0) {
            lower[b] = upper[b] = tau_out[b] = NAN;
            where[b] = -1;
            evals_out[b] = 0;
            flags[b] = NLOT_CERTIFY_NONFINITE;
        }
        return;
    }

    const bool poly = p.shape == NLOT_SHAPE_POLYGON;
    const int E = poly ? p.n_body : 1;  // edges = corners
    const int total = N * E;            // seed boxes, (k, edge) = (s / E, s mod E); at most 2^27

    // f at the centre of a box, the two shares of its radius and the centre's tau
    auto eval = [&](uint4 q, double* v, double* rq, double* rt, double* tau) {
        const int k = (int)q.x, e = (int)(q.y & 255u), dq = (int)(q.y >> 8 & 255u), dt = (int)(q.y >> 16 & 255u);
        const double tq = ldexp((double)(2u * q.z + 1u), -(dq + 1)), tt = ldexp((double)(2u * q.w + 1u), -(dt + 1));
        const double* a = X + (size_t)k * nx;
        const double* c = a + nx;
        const double dx = c[0] - a[0], dy = c[1] - a[1];
        const double px = a[0] + tq * dx, py = a[1] + tq * dy;
        double wx = px, wy = py, move = hypot(dx, dy), len = 0.0;
        if (poly) {
            const int e1 = e + 1 < p.n_body ? e + 1 : 0;
            const double c0x = p.body[e][0], c0y = p.body[e][1], c1x = p.body[e1][0], c1y = p.body[e1][1];
            const double dth = c[2] - a[2];
            double sn, cs;
            sincos(a[2] + tq * dth, &sn, &cs);
            const double ax = px + cs * c0x - sn * c0y, ay = py + sn * c0x + cs * c0y;
            const double bx = px + cs * c1x - sn * c1y, by = py + sn * c1x + cs * c1y;
            wx = (1.0 - tt) * ax + tt * bx;
            wy = (1.0 - tt) * ay + tt * by;
            move += fmax(hypot(c0x, c0y), hypot(c1x, c1y)) * fabs(dth);
            len = hypot(c1x - c0x, c1y - c0y);
        }
        *v = exact_sdf(p, wx, wy);
        *rq = ldexp(move, -(dq + 1));
        *rt = ldexp(len, -(dt + 1));
        *tau = tq;
    };
    // v - r of a box; a radius that is not finite (overflowing differences) bounds nothing
    auto bound = [](double v, double rq, double rt) {
        const double r = rq + rt;
        return r < INFINITY ? v - r : -INFINITY;
    };

    // seed U: knots x corners.  Knot s < N is (k, tau) = (s, 0), knot N is (N - 1, 1)
    Witness U = {INFINITY, INT_MAX, INFINITY};
    const int nseed = (N + 1) * E;
    for (int idx = lane; idx < nseed; idx += 64) {
        const int s = idx / E, j = idx - s * E;
        const double* a = X + (size_t)s * nx;
        double wx = a[0], wy = a[1];
        if (poly) {
            double sn, cs;
            sincos(a[2], &sn, &cs);
            footprint_point(p, a[0], a[1], sn, cs, j, 1, &wx, &wy);
        }
        U.take(exact_sdf(p, wx, wy), s < N ? s : N - 1, s < N ? 0.0 : 1.0);  // s ascends within a lane
    }
    wave_witness(U.v, U.k, U.tau);
    int evals = nseed;

    // containment at knot 0: the lanes stride over the obstacles
    int contains = 0;
    if (poly && p.n_body >= 3) {
        double sn, cs;
        sincos(X[2], &sn, &cs);
        obstacles_inside_body(p, X[0], X[1], sn, cs, lane, 64, contains);
        contains = group_or<64>(contains);
    }

    double L = INFINITY;  // per lane; reduced at the end
    int sp = 0, seed = 0, spent = 0, budget = 0, drain = 0;
    while (true) {
        if (sp < 64 && seed < total) {  // top up to 64 boxes
            const int n = min(64 - sp, total - seed);
            if (lane < n) stack[sp + lane] = make_box((seed + lane) / E, (seed + lane) % E, 0, 0, 0u, 0u);
            sp += n;
            seed += n;
            wave_lds_sync();
        }
        if (sp == 0) break;
        if (o.decide && U.v < o.clearance_min) {
            drain = 1;
            break;
        }
        const int n = min(min(sp, 64), o.max_evals - spent);
        if (n <= 0 || sp + n > kCertCap) {  // the budget is spent, or the pushes of this round could overflow
            budget = drain = 1;
            break;
        }
        sp -= n;
        const bool act = lane < n;
        const uint4 q = stack[sp + min(lane, n - 1)];
        wave_lds_sync();  // the pushes below overwrite what other lanes have just read
        double v, rq, rt, tq;
        eval(q, &v, &rq, &rt, &tq);
        spent += n;
        Witness w = {act ? v : INFINITY, act ? (int)q.x : INT_MAX, tq};
        wave_witness(w.v, w.k, w.tau);
        U.take(w.v, w.k, w.tau);
        const double lb = bound(v, rq, rt);
        const int dq = (int)(q.y >> 8 & 255u), dt = (int)(q.y >> 16 & 255u);
        // the dimension to bisect: the larger share of r among those with depth left; none: the box retires as it is
        const bool can_q = dq < kCertMaxDepth && rq > 0.0, can_t = dt < kCertMaxDepth && rt > 0.0;
        const bool split_q = can_q && (rq >= rt || !can_t);
        bool retire = lb >= U.v - o.tol || (o.decide && lb >= o.clearance_min);
        if (act && !retire && !can_q && !can_t) {
            retire = true;
            budget = 1;
        }
        if (act && retire) L = fmin(L, lb);
        const bool split = act && !retire;
        const uint64_t m = __ballot(split);
        if (split) {
            const int at = sp + 2 * __popcll(m & ((1ull << lane) - 1ull));
            const int e = (int)(q.y & 255u);
            if (split_q) {
                stack[at] = make_box((int)q.x, e, dq + 1, dt, 2u * q.z, q.w);
                stack[at + 1] = make_box((int)q.x, e, dq + 1, dt, 2u * q.z + 1u, q.w);
            } else {
                stack[at] = make_box((int)q.x, e, dq, dt + 1, q.z, 2u * q.w);
                stack[at + 1] = make_box((int)q.x, e, dq, dt + 1, q.z, 2u * q.w + 1u);
            }
        }
        sp += 2 * __popcll(m);
        wave_lds_sync();
    }

    if (drain) {  // every remaining box once, retired with its own bound
        const int rest = sp + (total - seed);
        Witness w = {INFINITY, INT_MAX, INFINITY};
        for (int i = lane; i < rest; i += 64) {
            const int s = seed + (i - sp);
            const uint4 q = i < sp ? stack[i] : make_box(s / E, s % E, 0, 0, 0u, 0u);
            double v, rq, rt, tq;
            eval(q, &v, &rq, &rt, &tq);
            w.take(v, (int)q.x, tq);
            L = fmin(L, bound(v, rq, rt));
        }
        wave_witness(w.v, w.k, w.tau);
        U.take(w.v, w.k, w.tau);
        evals += rest;
    }
    evals += spent;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) L = fmin(L, __shfl_xor(L, off));
    budget = group_or<64>(budget);

    if (lane == 0) {
        L = fmin(L, U.v);  // the box that holds U's point bounds it from below, up to rounding
        int fl = 0;
        if (U.v < o.clearance_min) fl |= NLOT_CERTIFY_COLLISION;
        if (contains) fl |= NLOT_CERTIFY_CONTAINS;
        if (L < o.clearance_min && !(U.v < o.clearance_min)) fl |= NLOT_CERTIFY_UNDECIDED;
        if (budget) fl |= NLOT_CERTIFY_BUDGET;
        lower[b] = L;
        upper[b] = U.v;
        where[b] = U.k;
        tau_out[b] = U.tau;
        evals_out[b] = evals;
        flags[b] = fl;
    }
}

}  // namespace
}  // namespace nlot

extern "C" void nlot_default_certify_options(NlotCertifyOptions* opt) {
    if (!opt) return;
    opt->tol = 1e-3;
    opt->clearance_min = 0.0;
    opt->decide = 0;
    opt->max_evals = 0;
}

extern "C" int32_t nlot_certify_batch(const NlotProblem* prob, const NlotCertifyOptions* opt, const double* X,
                                      double* lower, double* upper, int32_t* where, double* tau, int32_t* evals,
                                      int32_t* flags, int64_t B, void* stream) {
    using namespace nlot;
    if (!prob || !opt) {
        set_error("nlot_certify_batch: null problem or options");
        return NLOT_ERR_INVALID;
    }
    if (!(opt->tol > 0.0) || !std::isfinite(opt->tol)) {
        set_error("nlot_certify_batch: tol must be > 0 and finite");
        return NLOT_ERR_INVALID;
    }
    if (!std::isfinite(opt->clearance_min)) {
        set_error("nlot_certify_batch: clearance_min must be finite");
        return NLOT_ERR_INVALID;
    }
    if (opt->decide != 0 && opt->decide != 1) {
        set_error("nlot_certify_batch: decide must be 0 or 1");
        return NLOT_ERR_INVALID;
    }
    if (opt->max_evals < 0 || opt->max_evals > 1 << 24) {
        set_error("nlot_certify_batch: max_evals must be 0 (default) or 1 .. 2^24");
        return NLOT_ERR_INVALID;
    }
    if (prob->n_obs == 0) {
        set_error("nlot_certify_batch: the problem carries no scene (n_obs == 0)");
        return NLOT_ERR_INVALID;
    }
    if (!check_problem(prob, B, "nlot_certify_batch")) return NLOT_ERR_INVALID;
    if (!X || !lower || !upper || !where || !tau || !evals || !flags) {
        set_error("nlot_certify_batch: null pointer");
        return NLOT_ERR_INVALID;
    }
    NlotCertifyOptions o = *opt;
    if (o.max_evals == 0) {
        const int64_t edges = prob->shape == NLOT_SHAPE_POLYGON ? prob->n_body : 1;
        const int64_t d = 4096 + 256 * (int64_t)prob->N * edges;
        o.max_evals = (int32_t)(d < (int64_t)1 << 24 ? d : (int64_t)1 << 24);
    }
    hipStream_t st = (hipStream_t)stream;
    return with_device_problem(prob, st, [&](const NlotProblem* dP) {
        const unsigned grid = (unsigned)((B + kCertWaves - 1) / kCertWaves);
        hipLaunchKernelGGL(k_certify, dim3(grid), dim3(64 * kCertWaves), 0, st, dP, o, X, lower, upper, where, tau,
                           evals, flags, B);
    });
}
