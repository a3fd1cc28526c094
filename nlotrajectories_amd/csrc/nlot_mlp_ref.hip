// The two learned-SDF MLP families that are not throughput paths: mlp_smooth (smooth activations) and mlp_seq (the
// oracle's order of every sum).
#include "nlot_mlp.h"

namespace nlot {

// ---------------------------------------------------------------------------------------------
// Smooth activations (tanh, sigmoid, leaky ReLU, SIREN's sine; core/nn_architectures.py:8-100 and
// l4casadi's naive MLP): the Hessian has a term from every layer, so value, gradient and Hessian are
// carried FORWARD through the net as hyper-duals in fp32 — per hidden unit the 6 components
// (a, a_x, a_y, a_xx, a_xy, a_yy) of a point, with z = W a + b linear in all of them and, per unit,
//   a = s(z), a_x = s'(z) z_x, a_xx = s''(z) z_x^2 + s'(z) z_xx, a_xy = s''(z) z_x z_y + s'(z) z_xy, ...
// A block of 256 threads owns a tile of kSmoothPB points: thread t computes hidden unit t % H for the
// points of group t / H; the layer's activations of the tile sit in LDS as [k][point][component] (one
// broadcast float4 stream per k), the weights come transposed ([in][out]: a coalesced row per k) from L2.
// These nets are not on the metric path (the reference's YAMLs use ReLU); the bound is the fp32 VALU at
// 6 H^2 FMA per point and layer.
// ---------------------------------------------------------------------------------------------
constexpr int kSmoothPB = 8;

// s(z), s'(z), s''(z) of the activation
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

template <int H, bool FULL>
__global__ __launch_bounds__(256) void mlp_smooth(MlpDev w, const float* __restrict__ pts, int64_t cnt_host,
                                                  const int* __restrict__ cnt_dev, int P_per, int64_t ld,
                                                  const float* __restrict__ lam, MlpOut out) {
    constexpr int NC = FULL ? 6 : 1;            // hyper-dual components carried
    constexpr int NG = 256 / H;                 // point groups of a block
    constexpr int PPT = kSmoothPB / NG;         // points per thread
    constexpr int ROW = kSmoothPB * NC;         // floats per k in LDS
    static_assert(NG >= 1 && PPT >= 1 && (PPT * NC) % 2 == 0, "mlp_smooth shape");
    __shared__ __attribute__((aligned(16))) float act_s[H * ROW];
    __shared__ float pxy[kSmoothPB][2];
    __shared__ float lam_s[kSmoothPB];
    __shared__ int64_t pidx[kSmoothPB];
    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    const int t = threadIdx.x, i = t % H, grp = t / H, p0 = grp * PPT;
    const int act = w.act, L = w.n_hidden;
    const float omega = w.scale;
    const bool fourier = w.in_kind == NLOT_MLP_IN_FOURIER;
    for (int64_t tile = blockIdx.x; tile * kSmoothPB < npts; tile += gridDim.x) {
        if (t < kSmoothPB) {
            const int64_t gi = tile * kSmoothPB + t;
            const bool valid = gi < npts;
            const int64_t pi = valid ? point_addr(gi, cnt, ld) : -1;
            pidx[t] = pi;
            pxy[t][0] = valid ? pts[2 * pi] : 0.f;
            pxy[t][1] = valid ? pts[2 * pi + 1] : 0.f;
            lam_s[t] = (valid && lam) ? lam[pi] : 1.f;
        }
        __syncthreads();
        // input layer: z = p A + b0 (as torch: p @ A then + b0), dz/dp = (A0, A1), d2z = 0
        const float a0 = w.A[i], a1 = w.A[H + i], bb = w.b0[i];
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int p = p0 + q;
            const float z = fmaf(pxy[p][1], a1, pxy[p][0] * a0) + bb;
            float s, d1, d2;
            if (fourier) {  // scale * cos(z) (nn_architectures.py:38)
                const float sn = sinf(z), cs = cosf(z);
                s = cs * w.scale;
                d1 = -w.scale * sn;
                d2 = -w.scale * cs;
            } else {
                act3(act, omega, z, s, d1, d2);
            }
            float* dst = act_s + i * ROW + p * NC;
            dst[0] = s;
            if constexpr (FULL) {
                dst[1] = d1 * a0;
                dst[2] = d1 * a1;
                dst[3] = d2 * a0 * a0;
                dst[4] = d2 * a0 * a1;
                dst[5] = d2 * a1 * a1;
            }
        }
        __syncthreads();
        // hidden layers
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            const float* Wt = w.Wt + (size_t)l * H * H + i;
            float acc[PPT * NC];
#pragma unroll
            for (int e = 0; e < PPT * NC; ++e) acc[e] = 0.f;
            const float* src = act_s + p0 * NC;
#pragma unroll 4
            for (int k = 0; k < H; ++k) {
                const float wk = Wt[(size_t)k * H];
                const float2* ak = reinterpret_cast<const float2*>(src + k * ROW);
#pragma unroll
                for (int e2 = 0; e2 < PPT * NC / 2; ++e2) {
                    const float2 v = ak[e2];
                    acc[2 * e2] = fmaf(wk, v.x, acc[2 * e2]);
                    acc[2 * e2 + 1] = fmaf(wk, v.y, acc[2 * e2 + 1]);
                }
            }
            const float bl = w.b[(size_t)l * H + i];
            __syncthreads();  // every thread has read the layer's input
#pragma unroll
            for (int q = 0; q < PPT; ++q) {
                const float* z = acc + q * NC;
                float s, d1, d2;
                act3(act, omega, z[0] + bl, s, d1, d2);
                float* dst = act_s + i * ROW + (p0 + q) * NC;
                dst[0] = s;
                if constexpr (FULL) {
                    dst[1] = d1 * z[1];
                    dst[2] = d1 * z[2];
                    dst[3] = fmaf(d2 * z[1], z[1], d1 * z[3]);
                    dst[4] = fmaf(d2 * z[1], z[2], d1 * z[4]);
                    dst[5] = fmaf(d2 * z[2], z[2], d1 * z[5]);
                }
            }
            __syncthreads();
        }
        // output layer: thread (point, component) contracts w_out over the hidden units
        if (t < ROW) {
            const int p = t / NC, c = t % NC;
            float s = 0.f;
            for (int k = 0; k < H; ++k) s = fmaf(w.w_out[k], act_s[k * ROW + t], s);
            const int64_t pi = pidx[p];
            if (pi >= 0) {
                const float lm = lam_s[p];
                if (c == 0) out.val[pi * out.sv] = s + w.b_out;
                if constexpr (FULL) {
                    if (c == 1 && out.gx) out.gx[pi * out.sg] = lm * s;
                    if (c == 2 && out.gy) out.gy[pi * out.sg] = lm * s;
                    if (out.hxx) {
                        if (c == 3) out.hxx[pi * out.sh] = lm * s;
                        if (c == 4) {
                            out.hxy[pi * out.sh] = lm * s;
                            if (out.hyx != out.hxy) out.hyx[pi * out.sh] = lm * s;
                        }
                        if (c == 5) out.hyy[pi * out.sh] = lm * s;
                    }
                }
            }
        }
        __syncthreads();  // the tile's LDS is reused by the next one
    }
}

template <int H, bool FULL>
static int launch_smooth(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                         const float* lam, const MlpOut& out, hipStream_t stream) {
    const int grid = persistent_grid(n * P_per, kSmoothPB, (int64_t)device_cus() * 8);
    hipLaunchKernelGGL((mlp_smooth<H, FULL>), dim3(grid), dim3(256), 0, stream, w, pts, n, n_dev, P_per, ld, lam, out);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

int launch_mlp_smooth(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                      const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return dispatch_width(w.H, [&](auto width) {
        constexpr int H = decltype(width)::value;
        return full ? launch_smooth<H, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                    : launch_smooth<H, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
    });
}

// ---------------------------------------------------------------------------------------------
// NLOT_MLP_ARITH_SEQ (ABI v15): the ReLU net in the reference order of every sum.  One thread per point; each dot
// product is a sequential fmaf chain over its index in increasing order with the bias added after it, FMA
// contraction off: the expression sequence of the oracle's default order (oracle/nlot_oracle.c oracle_mlp_point,
// NLOT_ORACLE_MLP_REV unset).  For a Linear + ReLU input layer (benchmark 6's trained net, l4casadi's naive MLP) the
// outputs are bitwise the oracle's; a Fourier input layer's cos / sin are the fp64 functions rounded to fp32 on both
// sides (the correctly rounded fp32 values except where the two libms' fp64 results straddle an fp32 rounding
// boundary, about once in 2^28 evaluations).  Test arithmetic: it takes the net's rounding out of a GPU-vs-oracle comparison, so that what is left
// is the solver's fp64 (tests/test_pinned_iterates_gpu.py).  Not a throughput path: VALU chains, per-thread arrays
// in scratch.  The value launches write no ReLU patterns and the full launches reuse no forward (both optional).
// ---------------------------------------------------------------------------------------------
template <int H, bool FULL>
__global__ __launch_bounds__(64) void mlp_seq(MlpDev w, const float* __restrict__ pts, int64_t cnt_host,
                                              const int* __restrict__ cnt_dev, int P_per, int64_t ld,
                                              const float* __restrict__ lam, MlpOut out) {
#pragma clang fp contract(off)
    constexpr int MW = H / 32;
    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    const int L = w.n_hidden;
    const bool fourier = w.in_kind == NLOT_MLP_IN_FOURIER;
    for (int64_t gi = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gi < npts; gi += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pi = point_addr(gi, cnt, ld);
        const float px = pts[2 * pi], py = pts[2 * pi + 1];
        float z0[H], h[H], hn[H];
        uint32_t mask[kMaxStreamLayers + 1][MW];
        for (int k = 0; k < H; ++k) {  // p @ A + b0 (graph ___torch_mangle_0.py)
            const float z = fmaf(py, w.A[H + k], px * w.A[k]) + w.b0[k];
            z0[k] = z;
            h[k] = fourier ? (float)cos((double)z) * w.scale : (z > 0.f ? z : 0.f);
        }
        for (int q = 0; q < MW; ++q) {
            uint32_t m = 0;
            for (int t = 0; t < 32; ++t) m |= (fourier || z0[32 * q + t] > 0.f) ? (1u << t) : 0u;
            mask[0][q] = m;
        }
        for (int l = 0; l < L; ++l) {
            const float* W = w.W + (size_t)l * H * H;
            for (int j = 0; j < H; ++j) {
                float a = 0.f;
                for (int k = 0; k < H; ++k) a = fmaf(W[(size_t)j * H + k], h[k], a);
                a += w.b[(size_t)l * H + j];
                hn[j] = a > 0.f ? a : 0.f;
            }
            for (int q = 0; q < MW; ++q) {
                uint32_t m = 0;
                for (int t = 0; t < 32; ++t) m |= hn[32 * q + t] > 0.f ? (1u << t) : 0u;
                mask[l + 1][q] = m;
            }
            for (int j = 0; j < H; ++j) h[j] = hn[j];
        }
        float f = 0.f;
        for (int j = 0; j < H; ++j) f = fmaf(w.w_out[j], h[j], f);
        out.val[pi * out.sv] = f + w.b_out;
        if constexpr (FULL) {
            // reverse sweep: d = df/dh_l, each column sum dn[k] = sum_j W[j][k] d[j] over j in increasing order
            const float lm = lam ? lam[pi] : 1.f;
            float* d = h;
            float* dn = hn;
            for (int j = 0; j < H; ++j) d[j] = lm * w.w_out[j];
            for (int l = L - 1; l >= 0; --l) {
                const float* W = w.W + (size_t)l * H * H;
                for (int j = 0; j < H; ++j) d[j] = (mask[l + 1][j >> 5] >> (j & 31)) & 1u ? d[j] : 0.f;
                for (int k = 0; k < H; ++k) {
                    float t = 0.f;
                    for (int j = 0; j < H; ++j) t = fmaf(W[(size_t)j * H + k], d[j], t);
                    dn[k] = t;
                }
                float* s = d;
                d = dn;
                dn = s;
            }
            float gx = 0.f, gy = 0.f, hxx = 0.f, hxy = 0.f, hyy = 0.f;
            // Written out, not input_contract and store_point: the oracle's sin / cos (fp64, rounded) and the stored
            // ReLU pattern; and f held until a store_point here costs mlp_seq<64, true> its second wave per SIMD
            for (int k = 0; k < H; ++k) {
                const float ax = w.A[k], ay = w.A[H + k];
                float dz, c2;
                if (fourier) {
                    dz = d[k] * (-w.scale * (float)sin((double)z0[k]));
                    c2 = d[k] * (-w.scale * (float)cos((double)z0[k]));
                } else {
                    dz = (mask[0][k >> 5] >> (k & 31)) & 1u ? d[k] : 0.f;
                    c2 = 0.f;  // ReLU input layer: piecewise linear, Hessian 0 a.e.
                }
                gx = fmaf(ax, dz, gx);
                gy = fmaf(ay, dz, gy);
                hxx = fmaf(ax * ax, c2, hxx);
                hxy = fmaf(ax * ay, c2, hxy);
                hyy = fmaf(ay * ay, c2, hyy);
            }
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
    }
}

template <int H, bool FULL>
static int launch_seq(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                      const float* lam, const MlpOut& out, hipStream_t stream) {
    const int grid = persistent_grid(n * P_per, 64, (int64_t)device_cus() * 16);
    hipLaunchKernelGGL((mlp_seq<H, FULL>), dim3(grid), dim3(64), 0, stream, w, pts, n, n_dev, P_per, ld, lam, out);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

int launch_mlp_seq(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                   const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return dispatch_width(w.H, [&](auto width) {
        constexpr int H = decltype(width)::value;
        return full ? launch_seq<H, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                    : launch_seq<H, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
    });
}

}  // namespace nlot
