// The analytic scene at arbitrary points (nlot_scene_sdf_eval) and the SDF-quality metrics of two sampled SDFs
// (nlot_sdf_metrics, include/nlot.h) for gfx950.  fp64 throughout; DESIGN.md §12.
//
// k_scene_eval<KIND, DERIVS>: one thread per point in a grid-stride loop, calling exact_sdf / sdf_scene of
//   nlot_device.h unchanged.  The obstacle and vertex loops are wave-uniform and the problem arrives through a
//   const __restrict__ pointer, so obs[i] and verts[e] are scalar loads: no LDS stage.
// nlot_sdf_metrics, six launches:
//   k_band_count    each block owns kBandElems consecutive points: the sizes of its pieces of the two surface bands
//                   T = {|target| < eps}, Q = {|pred| < eps}, its occupancy counts and its partial sums of
//                   (target - pred)^2 and of pred^2 over T, reduced in a fixed order
//   k_band_offsets  one block: the exclusive scan of the band sizes over the blocks, the totals, and mse, iou,
//                   surface_loss and the counts of the result
//   k_band_scatter  the same blocks write their band points behind their offsets, in index order (block scan)
//   k_nearest x 2   one query point per thread; the block streams the other band through an LDS tile and keeps the
//                   minimum squared distance, one sqrt at the end; per-block (max, sum) partials
//   k_metrics_finish one block: the partials in block order -> hausdorff, chamfer
// The band sizes are known on the device only, so the band lists are sized for P points and k_nearest is launched
// for P queries; the blocks past the band's size leave at once.
#include <cmath>

#include "nlot_device.h"
#include "nlot_internal.h"

namespace nlot {
namespace {

constexpr int kEvalThreads = 256;

template <int KIND, bool DERIVS>
__global__ __launch_bounds__(kEvalThreads) void k_scene_eval(const NlotProblem* __restrict__ pp,
                                                             const double* __restrict__ pts, int64_t P,
                                                             double* __restrict__ val, double* __restrict__ grad,
                                                             double* __restrict__ hess) {
    const NlotProblem& p = *pp;
    const int64_t stride = (int64_t)gridDim.x * kEvalThreads;
    for (int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x; i < P; i += stride) {
        const double x = pts[2 * i], y = pts[2 * i + 1];
        if (KIND == NLOT_SCENE_EXACT) {
            val[i] = exact_sdf(p, x, y);
        } else {
            const HD h = sdf_scene(p, x, y, DERIVS);
            val[i] = h.v;
            if (DERIVS) {
                if (grad) {
                    grad[2 * i] = h.gx;
                    grad[2 * i + 1] = h.gy;
                }
                if (hess) {
                    hess[3 * i] = h.hxx;
                    hess[3 * i + 1] = h.hxy;
                    hess[3 * i + 2] = h.hyy;
                }
            }
        }
    }
}

// ---- metrics ---------------------------------------------------------------------------------------------------
constexpr int kBandThreads = 256;
constexpr int kBandItems = 4;  // consecutive points per thread: a thread's points precede the next thread's
constexpr int kBandElems = kBandThreads * kBandItems;
constexpr int kRedThreads = 256;  // the single-block kernels

struct BandPart {  // one block of k_band_count
    int32_t nT, nQ, nI, nU;
    double sq, surf;
};
struct BandOff {  // exclusive band offsets of a block
    int64_t t, q;
};
struct NearPart {
    double mx, sum;
};

// sum over the block in a fixed tree order (thread t + s into t); every thread gets the result.  `s` holds NT doubles.
template <int NT>
__device__ inline double block_sum(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}
template <int NT>
__device__ inline double block_max(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + o]);
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}
// exclusive scan of v over the block's threads; *total = the block's sum.  `sw` holds NT / 64 values.
template <int NT, class T>
__device__ inline T block_excl_scan(T v, T* total, T* sw) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T n = __shfl_up(inc, o);
        if (lane >= o) inc += n;
    }
    if (lane == 63) sw[w] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int i = 0; i < NT / 64; ++i) {
        const T c = sw[i];
        if (i < w) base += c;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__global__ __launch_bounds__(kBandThreads) void k_band_count(NlotSdfMetricsOptions o, const double* __restrict__ target,
                                                             const double* __restrict__ pred, int64_t P,
                                                             BandPart* __restrict__ part) {
    __shared__ double s[kBandThreads];
    __shared__ int sw[kBandThreads / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kBandElems + (int64_t)threadIdx.x * kBandItems;
    int nT = 0, nQ = 0, nI = 0, nU = 0;
    double sq = 0.0, surf = 0.0;
    for (int k = 0; k < kBandItems; ++k) {
        const int64_t i = i0 + k;
        if (i >= P) break;
        const double t = target[i], q = pred[i], d = t - q;
        sq += d * d;
        const bool inT = fabs(t) < o.eps, a = t < o.threshold, b = q < o.threshold;
        nT += inT;
        nQ += fabs(q) < o.eps;
        nI += a && b;
        nU += a || b;
        if (inT) surf += q * q;
    }
    // the four counts are at most kBandElems = 2^10 each: two per int
    int c0, c1;
    block_excl_scan<kBandThreads>(nT | (nQ << 16), &c0, sw);
    block_excl_scan<kBandThreads>(nI | (nU << 16), &c1, sw);
    sq = block_sum<kBandThreads>(sq, s);
    surf = block_sum<kBandThreads>(surf, s);
    if (threadIdx.x == 0) part[blockIdx.x] = {c0 & 0xffff, c0 >> 16, c1 & 0xffff, c1 >> 16, sq, surf};
}

__global__ __launch_bounds__(kRedThreads) void k_band_offsets(const BandPart* __restrict__ part, int64_t nb, int64_t P,
                                                              BandOff* __restrict__ off, NlotSdfMetrics* __restrict__ out) {
    __shared__ double s[kRedThreads];
    __shared__ int64_t sw[kRedThreads / 64];
    // thread t owns the blocks [t per, (t + 1) per): band sizes for the scan, counts; the sums go strided (below)
    const int64_t per = (nb + kRedThreads - 1) / kRedThreads;
    const int64_t b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    int64_t nT = 0, nQ = 0, nI = 0, nU = 0;
    for (int64_t b = b0; b < b1; ++b) {
        nT += part[b].nT;
        nQ += part[b].nQ;
        nI += part[b].nI;
        nU += part[b].nU;
    }
    int64_t totT, totQ, totI, totU;
    int64_t t = block_excl_scan<kRedThreads>(nT, &totT, sw);
    int64_t q = block_excl_scan<kRedThreads>(nQ, &totQ, sw);
    block_excl_scan<kRedThreads>(nI, &totI, sw);
    block_excl_scan<kRedThreads>(nU, &totU, sw);
    for (int64_t b = b0; b < b1; ++b) {
        off[b] = {t, q};
        t += part[b].nT;
        q += part[b].nQ;
    }
    // fixed order: thread t adds the blocks t, t + 256, ... in ascending order, then the tree
    double sq = 0.0, surf = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += kRedThreads) {
        sq += part[b].sq;
        surf += part[b].surf;
    }
    sq = block_sum<kRedThreads>(sq, s);
    surf = block_sum<kRedThreads>(surf, s);
    if (threadIdx.x == 0) {
        out->mse = sq / (double)P;
        out->iou = totU == 0 ? 1.0 : (double)totI / (double)totU;
        out->hausdorff = NAN;  // k_metrics_finish
        out->chamfer = NAN;
        out->surface_loss = totT == 0 ? NAN : surf / (double)totT;
        out->n_target_surface = totT;
        out->n_pred_surface = totQ;
        out->n_points = P;
    }
}

__global__ __launch_bounds__(kBandThreads) void k_band_scatter(NlotSdfMetricsOptions o, const double* __restrict__ pts,
                                                               const double* __restrict__ target,
                                                               const double* __restrict__ pred, int64_t P,
                                                               const BandOff* __restrict__ off, double2* __restrict__ T,
                                                               double2* __restrict__ Q) {
    __shared__ int sw[kBandThreads / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kBandElems + (int64_t)threadIdx.x * kBandItems;
    bool inT[kBandItems], inQ[kBandItems];
    int nT = 0, nQ = 0;
#pragma unroll
    for (int k = 0; k < kBandItems; ++k) {
        const int64_t i = i0 + k;
        inT[k] = i < P && fabs(target[i]) < o.eps;
        inQ[k] = i < P && fabs(pred[i]) < o.eps;
        nT += inT[k];
        nQ += inQ[k];
    }
    int tot;
    const int ex = block_excl_scan<kBandThreads>(nT | (nQ << 16), &tot, sw);
    // the block's pieces lie inside the lists: off + the block's counts <= the band's size <= P
    int64_t t = off[blockIdx.x].t + (ex & 0xffff), q = off[blockIdx.x].q + (ex >> 16);
#pragma unroll
    for (int k = 0; k < kBandItems; ++k) {
        if (inT[k] || inQ[k]) {
            const double2 xy = make_double2(pts[2 * (i0 + k)], pts[2 * (i0 + k) + 1]);
            if (inT[k]) T[t++] = xy;
            if (inQ[k]) Q[q++] = xy;
        }
    }
}

// min over the nb points of B of |a - b| for each of the na points of A: one query per thread, B streamed through an
// LDS tile of TILE points (16 bytes each).  Every lane of a wave reads the same tile entry: an LDS broadcast.  The
// tail tile's loop bound and the tail queries are masked; nothing is padded.  part[block] = (max, sum) over the
// block's queries.
template <int TILE, int NT>
__global__ __launch_bounds__(NT) void k_nearest(const double2* __restrict__ A, const int64_t* __restrict__ na_p,
                                                const double2* __restrict__ B, const int64_t* __restrict__ nb_p,
                                                NearPart* __restrict__ part) {
    __shared__ double2 tile[TILE];
    __shared__ double s[NT];
    const int64_t na = *na_p, nb = *nb_p;
    const int64_t a0 = (int64_t)blockIdx.x * NT;
    if (a0 >= na || nb == 0) return;  // block-uniform: before any barrier
    const int64_t a = a0 + threadIdx.x;
    const bool live = a < na;
    const double2 qa = live ? A[a] : make_double2(0.0, 0.0);
    double best = INFINITY;
    for (int64_t j0 = 0; j0 < nb; j0 += TILE) {
        const int cnt = nb - j0 < TILE ? (int)(nb - j0) : TILE;
        __syncthreads();  // the previous tile has been read
        for (int j = threadIdx.x; j < cnt; j += NT) tile[j] = B[j0 + j];
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < cnt; ++j) {
            const double dx = qa.x - tile[j].x, dy = qa.y - tile[j].y;
            best = fmin(best, dx * dx + dy * dy);
        }
    }
    const double d = live ? sqrt(best) : 0.0;  // distances are >= 0: a dead lane's 0 changes neither max nor sum
    __syncthreads();
    const double mx = block_max<NT>(d, s);
    const double sum = block_sum<NT>(d, s);
    if (threadIdx.x == 0) part[blockIdx.x] = {mx, sum};
}

template <int NT>
__global__ __launch_bounds__(kRedThreads) void k_metrics_finish(const NearPart* __restrict__ partQ,
                                                                const NearPart* __restrict__ partT,
                                                                NlotSdfMetrics* __restrict__ out) {
    __shared__ double s[kRedThreads];
    const int64_t nT = out->n_target_surface, nQ = out->n_pred_surface;
    if (nT == 0 || nQ == 0) return;  // hausdorff and chamfer stay NaN (k_band_offsets)
    const int64_t bQ = (nQ + NT - 1) / NT, bT = (nT + NT - 1) / NT;
    double mx = 0.0, sq = 0.0, st = 0.0;
    for (int64_t b = threadIdx.x; b < bQ; b += kRedThreads) {
        mx = fmax(mx, partQ[b].mx);
        sq += partQ[b].sum;
    }
    for (int64_t b = threadIdx.x; b < bT; b += kRedThreads) {
        mx = fmax(mx, partT[b].mx);
        st += partT[b].sum;
    }
    mx = block_max<kRedThreads>(mx, s);
    sq = block_sum<kRedThreads>(sq, s);
    st = block_sum<kRedThreads>(st, s);
    if (threadIdx.x == 0) {
        out->hausdorff = mx;
        out->chamfer = (sq / (double)nQ + st / (double)nT) / 2;
    }
}

}  // namespace
}  // namespace nlot

// k_nearest's tile (points) and block size; NLOT_NEAREST_TILE is restated as scene_gpu.NEAREST_TILE for the tests
#define NLOT_NEAREST_TILE 1024
#define NLOT_NEAREST_THREADS 256

extern "C" int32_t nlot_scene_sdf_eval(const NlotProblem* prob, int32_t kind, const double* pts, int64_t P, double* val,
                                       double* grad, double* hess, void* stream) {
    using namespace nlot;
    if (!prob || !pts || !val) {
        set_error("nlot_scene_sdf_eval: null problem, pts or val");
        return NLOT_ERR_INVALID;
    }
    if (kind != NLOT_SCENE_EXACT && kind != NLOT_SCENE_APPROX) {
        set_error("nlot_scene_sdf_eval: kind must be NLOT_SCENE_EXACT or NLOT_SCENE_APPROX");
        return NLOT_ERR_INVALID;
    }
    if (prob->n_obs == 0) {
        set_error("nlot_scene_sdf_eval: the problem carries no scene (n_obs == 0)");
        return NLOT_ERR_INVALID;
    }
    if (prob->n_obs < 0 || prob->n_obs > NLOT_MAX_OBS || prob->n_verts < 0 || prob->n_verts > NLOT_MAX_VERTS) {
        set_error("nlot_scene_sdf_eval: invalid scene (n_obs, n_verts)");
        return NLOT_ERR_INVALID;
    }
    for (int i = 0; i < prob->n_obs; ++i) {
        const NlotObstacle& q = prob->obs[i];
        if (q.type < NLOT_OBS_CIRCLE || q.type > NLOT_OBS_TRAPEZOID) {
            set_error("nlot_scene_sdf_eval: invalid scene (unknown obstacle type)");
            return NLOT_ERR_INVALID;
        }
        if ((q.type == NLOT_OBS_POLYGON || q.type == NLOT_OBS_TRAPEZOID) &&
            (q.v0 < 0 || q.nv < 2 || q.v0 > prob->n_verts - q.nv)) {
            set_error("nlot_scene_sdf_eval: invalid scene (polygon vertex range outside verts[0, n_verts))");
            return NLOT_ERR_INVALID;
        }
    }
    if (P < 1 || P > (int64_t)1 << 30) {
        set_error("nlot_scene_sdf_eval: P out of range");
        return NLOT_ERR_INVALID;
    }
    if (kind == NLOT_SCENE_EXACT && (grad || hess)) {
        set_error("nlot_scene_sdf_eval: grad and hess need NLOT_SCENE_APPROX (the exact SDF has no derivatives)");
        return NLOT_ERR_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    return with_device_problem(prob, st, [&](const NlotProblem* dP) {
        const int64_t want = (P + kEvalThreads - 1) / kEvalThreads, cap = (int64_t)device_cus() * 16;
        const dim3 grid((unsigned)(want < cap ? want : cap)), block(kEvalThreads);
        if (kind == NLOT_SCENE_EXACT)
            hipLaunchKernelGGL((k_scene_eval<NLOT_SCENE_EXACT, false>), grid, block, 0, st, dP, pts, P, val, grad, hess);
        else if (grad || hess)
            hipLaunchKernelGGL((k_scene_eval<NLOT_SCENE_APPROX, true>), grid, block, 0, st, dP, pts, P, val, grad, hess);
        else
            hipLaunchKernelGGL((k_scene_eval<NLOT_SCENE_APPROX, false>), grid, block, 0, st, dP, pts, P, val, grad, hess);
    });
}

extern "C" void nlot_default_sdf_metrics_options(NlotSdfMetricsOptions* opt) {
    if (!opt) return;
    opt->threshold = 0.0;
    opt->eps = 1e-2;
}

extern "C" int32_t nlot_sdf_metrics(const NlotSdfMetricsOptions* opt, const double* pts, const double* target,
                                    const double* pred, int64_t P, NlotSdfMetrics* out, void* stream) {
    using namespace nlot;
    static_assert(sizeof(NlotSdfMetrics) == 64 && sizeof(NlotSdfMetricsOptions) == 16, "include/nlot.h");
    if (!opt || !pts || !target || !pred || !out) {
        set_error("nlot_sdf_metrics: null pointer");
        return NLOT_ERR_INVALID;
    }
    if (P < 1 || P > (int64_t)1 << 30) {
        set_error("nlot_sdf_metrics: P out of range");
        return NLOT_ERR_INVALID;
    }
    if (!(opt->eps > 0.0) || !std::isfinite(opt->eps)) {
        set_error("nlot_sdf_metrics: eps must be finite and > 0");
        return NLOT_ERR_INVALID;
    }
    if (!std::isfinite(opt->threshold)) {
        set_error("nlot_sdf_metrics: threshold must be finite");
        return NLOT_ERR_INVALID;
    }
    constexpr int TILE = NLOT_NEAREST_TILE, NT = NLOT_NEAREST_THREADS;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = (P + kBandElems - 1) / kBandElems;  // blocks of the band kernels
    const int64_t nq = (P + NT - 1) / NT;                  // blocks of k_nearest, per direction
    // one stream-ordered block: T [P], Q [P] double2, then the per-block records (all 8-byte aligned)
    const size_t bytes = (size_t)P * 2 * sizeof(double2) + (size_t)nb * (sizeof(BandPart) + sizeof(BandOff)) +
                         (size_t)nq * 2 * sizeof(NearPart);
    char* blk = nullptr;
    NLOT_HIP_CHECK(hipMallocAsync((void**)&blk, bytes, st));
    double2* T = (double2*)blk;
    double2* Q = T + P;
    BandPart* part = (BandPart*)(Q + P);
    BandOff* off = (BandOff*)(part + nb);
    NearPart* partQ = (NearPart*)(off + nb);
    NearPart* partT = partQ + nq;
    hipLaunchKernelGGL(k_band_count, dim3((unsigned)nb), dim3(kBandThreads), 0, st, *opt, target, pred, P, part);
    hipLaunchKernelGGL(k_band_offsets, dim3(1), dim3(kRedThreads), 0, st, part, nb, P, off, out);
    hipLaunchKernelGGL(k_band_scatter, dim3((unsigned)nb), dim3(kBandThreads), 0, st, *opt, pts, target, pred, P, off, T, Q);
    hipLaunchKernelGGL((k_nearest<TILE, NT>), dim3((unsigned)nq), dim3(NT), 0, st, Q, &out->n_pred_surface, T,
                       &out->n_target_surface, partQ);
    hipLaunchKernelGGL((k_nearest<TILE, NT>), dim3((unsigned)nq), dim3(NT), 0, st, T, &out->n_target_surface, Q,
                       &out->n_pred_surface, partT);
    hipLaunchKernelGGL((k_metrics_finish<NT>), dim3(1), dim3(kRedThreads), 0, st, partQ, partT, out);
    const hipError_t e = hipGetLastError();
    const hipError_t ef = hipFreeAsync(blk, st);
    NLOT_HIP_CHECK(e);
    NLOT_HIP_CHECK(ef);
    return NLOT_OK;
}
