// What the learned-SDF MLP kernel families share (internal): nlot_mlp_f32.hip, nlot_mlp_bf16.hip, nlot_mlp_stream.hip,
// nlot_mlp_hdual.hip, nlot_mlp_hdual_stream.hip, nlot_mlp_hdual_bf16.hip, nlot_mlp_hdual_bf16_stream.hip,
// nlot_mlp_relu_bf16_stream.hip and nlot_mlp_ref.hip hold one family each behind the launcher declared here; nlot_mlp.hip chooses among them.
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

// x = h + m + l in three bf16 parts (8 + 8 + 8 significant bits, exact up to 2^-24 relative): the operands of the
// split-bf16 kernels (mlp_bf16, mlp_hdual_bf16, mlp_hdual_bf16_stream, mlp_relu_bf16_stream)
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
#pragma clang fp contract(off)  // x is the rounded fp32 input: never fuse its producer into the subtractions
    h = (__bf16)x;
    const float r = x - (float)h;  // exact
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);    // exact difference
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

// s(z), s'(z), s''(z) of the activation: mlp_smooth, mlp_hdual and mlp_hdual_stream evaluate them by these
// expressions
__device__ __forceinline__ void act3(int act, float omega, float z, float& s, float& d1, float& d2) {
    if (act == NLOT_ACT_TANH) {
        s = tanhf(z);
        d1 = 1.f - s * s;
        d2 = -2.f * s * d1;
    } else if (act == NLOT_ACT_SIGMOID) {
        s = 1.f / (1.f + expf(-z));
        d1 = s * (1.f - s);
        d2 = d1 * (1.f - 2.f * s);
    } else if (act == NLOT_ACT_LEAKY_RELU) {
        s = z > 0.f ? z : 0.01f * z;
        d1 = z > 0.f ? 1.f : 0.01f;
        d2 = 0.f;
    } else if (act == NLOT_ACT_SINE) {
        const float u = omega * z;  // torch: sin(omega_0 * linear(x)), the product rounded first
        s = sinf(u);
        const float c = cosf(u);
        d1 = omega * c;
        d2 = -omega * omega * s;
    } else {  // ReLU
        s = z > 0.f ? z : 0.f;
        d1 = z > 0.f ? 1.f : 0.f;
        d2 = 0.f;
    }
}

// f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>), in order.  The tile loops of mlp_hdual and
// mlp_hdual_stream whose bodies hold the activation are unrolled this way, not by #pragma unroll: sinf / cosf with
// their large-argument paths make the unrolled body larger than the pragma's size threshold, the loop then stays a
// loop, and the register arrays it indexes go to scratch.
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
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

// NLOT_MLP_ARITH_HDUAL_MFMA keeps every HxH layer in LDS (nlot_mlp_hdual.hip): the layers that fit beside 160 KB
inline int hdual_max_layers(int H) { return H == 128 ? 2 : H == 64 ? 4 : 0; }
// null when mlp_hdual serves the net, else why not (nlot_mlp_create_ex refuses with it before any device call)
inline const char* hdual_refusal(int act, int H, int n_hidden) {
    if (act == NLOT_ACT_RELU || n_hidden < 1 || n_hidden > hdual_max_layers(H))
        return "NLOT_MLP_ARITH_HDUAL_MFMA serves smooth activations (tanh, sigmoid, leaky ReLU, sine) with hidden width "
               "128 and 1-2 HxH layers or hidden width 64 and 1-4; ReLU nets take the reverse-sweep arithmetics, other "
               "smooth shapes NLOT_MLP_ARITH_F32 (mlp_smooth)";
    return nullptr;
}

// NLOT_MLP_ARITH_HDUAL_STREAM keeps the activations in LDS and streams the weights (nlot_mlp_hdual_stream.hip): null
// when mlp_hdual_stream serves the net, else why not (nlot_mlp_create_ex refuses with it before any device call)
inline const char* hdual_stream_refusal(int act, int H, int n_hidden) {
    if (act == NLOT_ACT_RELU || (H != 64 && H != 128 && H != 256) || n_hidden < 1 || n_hidden > kMaxStreamLayers)
        return "NLOT_MLP_ARITH_HDUAL_STREAM serves smooth activations (tanh, sigmoid, leaky ReLU, sine) with hidden width "
               "64, 128 or 256 and 1-4 HxH layers; ReLU nets take the reverse-sweep arithmetics, a smooth net without "
               "HxH layers NLOT_MLP_ARITH_F32 (mlp_smooth)";
    return nullptr;
}

// NLOT_MLP_ARITH_HDUAL_BF16 keeps every HxH layer in LDS as three bf16 parts in fragment order (nlot_mlp_hdual_bf16.hip):
// 96 KB hold one layer at H = 128 or four at H = 64
__host__ __device__ constexpr int hdual_bf16_max_layers(int H) { return H == 128 ? 1 : H == 64 ? 4 : 0; }
// null when mlp_hdual_bf16 serves the net, else why not (nlot_mlp_create_ex refuses with it before any device call)
inline const char* hdual_bf16_refusal(int act, int H, int n_hidden) {
    if (act == NLOT_ACT_RELU || n_hidden < 1 || n_hidden > hdual_bf16_max_layers(H))
        return "NLOT_MLP_ARITH_HDUAL_BF16 serves smooth activations (tanh, sigmoid, leaky ReLU, sine) with hidden width "
               "128 and 1 HxH layer or hidden width 64 and 1-4; other smooth shapes take NLOT_MLP_ARITH_HDUAL_MFMA or "
               "NLOT_MLP_ARITH_HDUAL_STREAM, ReLU nets the reverse-sweep arithmetics";
    return nullptr;
}

// NLOT_MLP_ARITH_HDUAL_BF16_STREAM keeps the split activations in LDS and streams the split weights
// (nlot_mlp_hdual_bf16_stream.hip): null when mlp_hdual_bf16_stream serves the net, else why not (nlot_mlp_create_ex
// refuses with it before any device call)
inline const char* hdual_bf16_stream_refusal(int act, int H, int n_hidden) {
    if (act == NLOT_ACT_RELU || (H != 128 && H != 256) || n_hidden < 1 || n_hidden > kMaxStreamLayers)
        return "NLOT_MLP_ARITH_HDUAL_BF16_STREAM serves smooth activations (tanh, sigmoid, leaky ReLU, sine) with hidden "
               "width 128 or 256 and 1-4 HxH layers; hidden width 64 takes NLOT_MLP_ARITH_HDUAL_BF16, ReLU nets "
               "NLOT_MLP_ARITH_SPLIT_BF16, a smooth net without HxH layers NLOT_MLP_ARITH_F32 (mlp_smooth)";
    return nullptr;
}

// NLOT_MLP_ARITH_SPLIT_BF16_STREAM keeps the split activations and the reverse sweep's e in LDS and streams the split
// weights and their transposes (nlot_mlp_relu_bf16_stream.hip): null when mlp_relu_bf16_stream serves the net, else why
// not (nlot_mlp_create_ex refuses with it before any device call)
inline const char* relu_bf16_stream_refusal(int act, int H, int n_hidden) {
    if (act != NLOT_ACT_RELU || (H != 128 && H != 256) || n_hidden < 1 || n_hidden > kMaxStreamLayers)
        return "NLOT_MLP_ARITH_SPLIT_BF16_STREAM serves ReLU nets with hidden width 128 or 256 and 1-4 HxH layers; hidden "
               "width 64 takes NLOT_MLP_ARITH_SPLIT_BF16 or NLOT_MLP_ARITH_F32 (the f32-MFMA kernels), smooth activations "
               "NLOT_MLP_ARITH_HDUAL_BF16_STREAM, and a ReLU net needs an HxH layer in every arithmetic";
    return nullptr;
}

// One launcher per family, arguments as launch_mlp_strided's, which has checked w.n_hidden for the family: f32 takes
// H <= 128 with 1 or 2 HxH layers, bf16 H = 128 with one HxH layer and w.Wp, hdual what hdual_refusal passes,
// hdual_stream what hdual_stream_refusal passes and w.Wf, hdual_bf16 what hdual_bf16_refusal passes and w.Wb,
// hdual_bf16_stream what hdual_bf16_stream_refusal passes and w.Ws, relu_bf16_stream what relu_bf16_stream_refusal
// passes with w.Ws and w.Wr, the others every width
int launch_mlp_f32(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                   const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_bf16(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                    const float* lam, const MlpOut& out, bool full, hipStream_t stream, const MlpReuse* reuse);
int launch_mlp_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                      const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_smooth(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                      const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_hdual(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                     const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_hdual_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                            const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_hdual_bf16(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                          const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_hdual_bf16_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                                 const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_relu_bf16_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                                const float* lam, const MlpOut& out, bool full, hipStream_t stream);
int launch_mlp_seq(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                   const float* lam, const MlpOut& out, bool full, hipStream_t stream);

}  // namespace nlot
