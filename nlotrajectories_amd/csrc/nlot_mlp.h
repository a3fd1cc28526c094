// What the learned-SDF MLP kernel families share (internal): nlot_mlp_f32.hip, nlot_mlp_bf16.hip, nlot_mlp_stream.hip
// and nlot_mlp_ref.hip hold one family each behind the launcher declared here; nlot_mlp.hip chooses among them.
#pragma once
#include "nlot_internal.h"

namespace nlot {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxResidentLayers = 2;  // HxH layers the LDS-resident kernels hold (H <= 128)
constexpr int kMaxStreamLayers = 4;

// sin and cos of a Fourier-layer argument (|x| up to ~1e3 here: weights ~N(0, 9.4^2), inputs in the
// workspace box): 3-part Cody-Waite reduction by pi/2 with FMA, Cephes sinf/cosf minimax polynomials on
// [-pi/4, pi/4] (~1 ulp), quadrant by select.  No slow path: ~20 instructions for both.
__device__ __forceinline__ void sincos_fourier(float x, float* sn, float* cs) {
    const float j = rintf(x * 0.636619772367581343f);
    float r = fmaf(j, -1.57079637050628662109375f, x);
    r = fmaf(j, 4.37113900018624283e-8f, r);
    r = fmaf(j, 1.71512451e-15f, r);
    const float r2 = r * r;
    const float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f), r2 * r, r);
    const float pc = fmaf(fmaf(fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2,
                                    4.166664568298827e-2f), r2, -0.5f), r2, 1.0f);
    const int q = (int)j & 3;
    const float s0 = (q & 1) ? pc : ps, c0 = (q & 1) ? ps : pc;
    *sn = (q & 2) ? -s0 : s0;
    *cs = ((q + 1) & 2) ? -c0 : c0;
}

// Fourier-layer argument in turns for the transcendental unit (v_sin_f32 / v_cos_f32 give sin and cos of
// 2 pi t): r = x - 2 pi j in [-pi, pi] by a two-part Cody-Waite reduction with FMA (the first product is
// exact; the dropped third part, |j| * 3.4e-15, stays below 1e-12 for |x| <= 1e3), then r / (2 pi).  The
// split-bf16 kernels use it: 4 instructions and one 8-cycle transcendental per sin or cos, against ~14 for
// the polynomials and quadrant selects of sincos_fourier.
__device__ __forceinline__ float turns_fourier(float x) {
    const float j = rintf(x * 0.159154943091895336f);
    float r = fmaf(j, -6.28318548202514648f, x);
    r = fmaf(j, 1.74845560e-7f, r);
    return r * 0.159154943091895336f;
}

// row index (hidden unit) held by register r of a 32x32 accumulator on lane-half hl
__device__ __forceinline__ int acc_row(int r, int hl) { return (r & 3) + 8 * (r >> 2) + 4 * hl; }

// A launch covers cnt * P_per points, cnt = *cnt_dev when given (the solver's compacted instances).  Point g of it
// lives at address g (ld == 0, contiguous rank-major list) or (g % cnt) + (g / cnt) * ld of pts / lam / out.
__device__ __forceinline__ int64_t point_count(const int* cnt_dev, int64_t cnt_host) {
    return cnt_dev ? (int64_t)(*cnt_dev) : cnt_host;
}
__device__ __forceinline__ int64_t point_addr(int64_t gi, int64_t cnt, int64_t ld) {
    return ld == 0 ? gi : (gi % cnt) + (gi / cnt) * ld;
}

// value, lam * gradient and lam * Hessian of point pi; a null gradient or Hessian plane is skipped, and hyx may
// alias hxy
__device__ __forceinline__ void store_point(const MlpOut& out, int64_t pi, float f, float gx, float gy, float hxx,
                                            float hxy, float hyy) {
    out.val[pi * out.sv] = f;
    if (out.gx) {
        out.gx[pi * out.sg] = gx;
        out.gy[pi * out.sg] = gy;
    }
    if (out.hxx) {
        out.hxx[pi * out.sh] = hxx;
        out.hxy[pi * out.sh] = hxy;
        if (out.hyx != out.hxy) out.hyx[pi * out.sh] = hxy;
        out.hyy[pi * out.sh] = hyy;
    }
}

// One hidden unit of the input layer, h0 = scale cos(z) (Fourier) or relu(z) with z = ax px + ay py + b0, in the
// contraction of d = lam df/dh0 into gradient and Hessian: lam d2f/dp2 = A diag(d .* (-scale cos z)) A^T for a
// Fourier layer, 0 for a ReLU one (piecewise linear).
__device__ __forceinline__ void input_contract(float ax, float ay, float z, float d, bool fourier, float scale,
                                               float& gx, float& gy, float& hxx, float& hxy, float& hyy) {
    float dz, c2;
    if (fourier) {
        float sn, cs;
        sincos_fourier(z, &sn, &cs);
        dz = d * (-scale * sn);
        c2 = d * (-scale * cs);
    } else {
        dz = z > 0.f ? d : 0.f;
        c2 = 0.f;
    }
    gx = fmaf(ax, dz, gx);
    gy = fmaf(ay, dz, gy);
    hxx = fmaf(ax * ax, c2, hxx);
    hxy = fmaf(ax * ay, c2, hxy);
    hyy = fmaf(ay * ay, c2, hyy);
}

// blocks of a persistent launch: one per tile of points_per_tile points, at least 1 and at most cap
inline int persistent_grid(int64_t points, int points_per_tile, int64_t cap) {
    const int64_t tiles = (points + points_per_tile - 1) / points_per_tile;
    return (int)(tiles < cap ? (tiles > 0 ? tiles : 1) : cap);
}

// f(std::integral_constant<int, H>{}) for the hidden width H in {64, 128, 256} up to MAXH
template <int MAXH = 256, class F>
inline int dispatch_width(int H, F&& f) {
    if (H == 64) return f(std::integral_constant<int, 64>{});
    if (H == 128) return f(std::integral_constant<int, 128>{});
    if constexpr (MAXH >= 256)
        if (H == 256) return f(std::integral_constant<int, 256>{});
    set_error("MLP kernel: hidden width must be 64, 128 or 256 (DESIGN.md §7)");
    return NLOT_ERR_INVALID;
}

// One launcher per family, arguments as launch_mlp_strided's, which has checked w.n_hidden for the family: f32 takes
// H <= 128 with 1 or 2 HxH layers, bf16 H = 128 with one HxH layer and w.Wp, the others every width
int launch_mlp_f32(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                   const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_bf16(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                    const float* lam, const MlpOut& out, bool full, hipStream_t stream, const MlpReuse* reuse);
int launch_mlp_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                      const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_smooth(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                      const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_seq(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                   const float* lam, const MlpOut& out, bool full, hipStream_t stream);

}  // namespace nlot
