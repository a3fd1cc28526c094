// NLOT_MLP_ARITH_HDUAL_MFMA (ABI v21): the smooth-activation nets (tanh, sigmoid, leaky ReLU, SIREN's sine) on the
// matrix cores.  As in mlp_smooth (nlot_mlp_ref.hip) value, gradient and Hessian go FORWARD through the net as
// hyper-duals, six components (a, a_x, a_y, a_xx, a_xy, a_yy) per hidden unit and point; z = W a + b is linear in all
// six, so an HxH layer over P points is one GEMM W [HxH] . A [H x 6P] with the same A operand (the weights) for the
// six products, and everything nonlinear is element-wise on a (unit, point) pair.
//
// Mapping (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 sums).  256 threads = 4 waves, one per SIMD with the
// whole 512-register file; a wave owns 16 points (MFMA column = point = lane & 15), a block tile is 64 points and
// the grid is persistent.  Per 16-unit output tile a wave carries NC = 6 (FULL) or 1 (value) accumulators of 4
// registers per lane, register i = row 16 T + 4 (lane >> 4) + i.  The six accumulators of a tile share lane and
// register index, so the activation step (a_xx = s'' z_x^2 + s' z_xx, ...) is lane-local, and the activated tile is
// at once four B operands of the next layer: k-step (T, i) multiplies register i of input tile T, its k index on
// lane group lg being unit 16 T + 4 lg + i, and the A operand takes W[row][16 T + 4 lg + i] to match.  Activations
// never leave registers between the input layer and the output contraction.
//
// Weights.  Every HxH layer of the net is resident in LDS for the whole launch (loaded once per block), fp32,
// row-major [l][out][RS] with RS = H + 4; so are biases, the input layer (A, b0) and w_out.  The A operands of the
// four k-steps (T, 0..3) of output tile t are the four consecutive floats W[16 t + pn][16 T + 4 lg ..+3]: one
// ds_read_b128 feeds 4 x NC MFMAs (24 in FULL).  Bank conflicts: a b128 read is served 16 lanes (256 B = all 64
// banks) at a time; the 16 lanes of a lane group differ in pn only, so their addresses are RS floats apart, and
// RS = 4 (mod 64) puts lane pn on banks 4 pn .. 4 pn + 3 (+ const): the 16 quads tile the 64 banks exactly.  (RS = H
// would put all 16 on the same four.)  RS is a multiple of 4, so every read is 16-byte aligned.
//
// What fits in 160 KB: H = 128 with 1 or 2 HxH layers (2 x 128 x 132 x 4 B = 132 KB), H = 64 with 1 to 4 (68 KB).
//
// The value-only instantiation runs the component-0 chain through the same MFMAs in the same k order (it interleaves
// several output tiles for independent accumulators; an accumulator's own chain is unchanged), the same act3 and the
// same output contraction: a value launch is bitwise the full launch's value.
#include "nlot_mlp.h"

namespace nlot {

__host__ __device__ constexpr int hdual_stride(int H) { return H + 4; }
__host__ __device__ constexpr size_t hdual_lds_floats(int H, int L) {
    return (size_t)L * H * hdual_stride(H) + (size_t)4 * H + (size_t)L * H;
}

template <int H, int ACT, bool FULL>
__global__ __launch_bounds__(256, 1) void mlp_hdual(MlpDev w, const float* __restrict__ pts, int64_t cnt_host,
                                                    const int* __restrict__ cnt_dev, int P_per, int64_t ld,
                                                    const float* __restrict__ lam, MlpOut out) {
    constexpr int NC = FULL ? 6 : 1;         // hyper-dual components carried
    constexpr int NT = H / 16;               // 16-unit tiles of a layer
    constexpr int RS = hdual_stride(H);
    constexpr int TB = FULL ? 1 : 4;         // output tiles in flight (value: independent chains for the MFMA pipe)
    constexpr int TP = 64;                   // points per block tile
    static_assert(NT % TB == 0 && RS % 64 == 4, "mlp_hdual shape");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L = w.n_hidden;
    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    if ((int64_t)blockIdx.x * TP >= npts) return;  // a compacted launch: fewer tiles than blocks
    float* sW = smem;                         // [L][H][RS]
    float* sA0 = sW + (size_t)L * H * RS;     // [H]
    float* sA1 = sA0 + H;                     // [H]
    float* sb0 = sA1 + H;                     // [H]
    float* sw = sb0 + H;                      // [H]
    float* sbl = sw + H;                      // [L][H]
    for (int idx = threadIdx.x; idx < L * H * (H / 4); idx += 256) {
        const int row = idx / (H / 4), c4 = idx % (H / 4);
        *reinterpret_cast<float4*>(sW + (size_t)row * RS + 4 * c4) = reinterpret_cast<const float4*>(w.W)[idx];
    }
    for (int idx = threadIdx.x; idx < H; idx += 256) {
        sA0[idx] = w.A[idx];
        sA1[idx] = w.A[H + idx];
        sb0[idx] = w.b0[idx];
        sw[idx] = w.w_out[idx];
    }
    for (int idx = threadIdx.x; idx < L * H; idx += 256) sbl[idx] = w.b[idx];
    __syncthreads();  // the only barrier: LDS is read-only from here on
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pn = lane & 15, lg = lane >> 4;  // point of the lane; lane group (k / row offset 4 lg)
    const bool fourier = w.in_kind == NLOT_MLP_IN_FOURIER;
    const float scale = w.scale;  // Fourier scale, or SIREN's omega_0
    for (int64_t tile = blockIdx.x; tile * TP < npts; tile += gridDim.x) {
        const int64_t gi = tile * TP + wave * 16 + pn;
        const bool valid = gi < npts;
        const int64_t pi = valid ? point_addr(gi, cnt, ld) : 0;
        float px = 0.f, py = 0.f;
        if (valid) {
            px = pts[2 * pi];
            py = pts[2 * pi + 1];
        }
        f32x4 h[NC][NT];  // the layer's activations: component c of unit 16 T + 4 lg + i of the lane's point
        // input layer: z = p A + b0 (as torch: p @ A then + b0), dz/dp = (A0, A1), d2z = 0
        static_for<NT>([&](auto Tc) {
            constexpr int T = decltype(Tc)::value;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 16 * T + 4 * lg + i;
                const float a0 = sA0[k], a1 = sA1[k];
                const float z = fmaf(py, a1, px * a0) + sb0[k];
                float s, d1, d2;
                if (fourier) {  // scale * cos(z)
                    const float sn = sinf(z), cs = cosf(z);
                    s = cs * scale;
                    d1 = -scale * sn;
                    d2 = -scale * cs;
                } else {
                    act3(ACT, scale, z, s, d1, d2);
                }
                h[0][T][i] = s;
                if constexpr (FULL) {
                    h[1][T][i] = d1 * a0;
                    h[2][T][i] = d1 * a1;
                    h[3][T][i] = d2 * a0 * a0;
                    h[4][T][i] = d2 * a0 * a1;
                    h[5][T][i] = d2 * a1 * a1;
                }
            }
        });
        // HxH layers: z_c = W h_c for the NC components, then the activation per (unit, point)
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            const float* Wl = sW + (size_t)l * H * RS + pn * RS + 4 * lg;  // row pn of a tile, the lane group's k quad
            const float* bl = sbl + l * H + 4 * lg;
            f32x4 hn[NC][NT];
            static_for<NT / TB>([&](auto tc) {
                constexpr int t0 = decltype(tc)::value * TB;
                f32x4 acc[TB][NC];
#pragma unroll
                for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[tb][c] = f32x4{};
                // the A quads of input tile T + 1 are read ahead of the MFMAs of tile T (one wave per SIMD: nothing
                // else hides the LDS latency)
                f32x4 a_cur[TB];
#pragma unroll
                for (int tb = 0; tb < TB; ++tb) a_cur[tb] = *reinterpret_cast<const f32x4*>(Wl + 16 * (t0 + tb) * RS);
#pragma unroll
                for (int T = 0; T < NT; ++T) {
                    f32x4 a_nxt[TB];
                    if (T + 1 < NT) {
#pragma unroll
                        for (int tb = 0; tb < TB; ++tb)
                            a_nxt[tb] = *reinterpret_cast<const f32x4*>(Wl + 16 * (t0 + tb) * RS + 16 * (T + 1));
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                            for (int c = 0; c < NC; ++c)
                                acc[tb][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[tb][i], h[c][T][i], acc[tb][c], 0, 0, 0);
#pragma unroll
                    for (int tb = 0; tb < TB; ++tb) a_cur[tb] = a_nxt[tb];
                    asm volatile("" ::: "memory");  // bound the LDS loads the scheduler hoists (register file)
                }
#pragma unroll
                for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int t = t0 + tb;
                        float s, d1, d2;
                        act3(ACT, scale, acc[tb][0][i] + bl[16 * t + i], s, d1, d2);
                        hn[0][t][i] = s;
                        if constexpr (FULL) {
                            const float zx = acc[tb][1][i], zy = acc[tb][2][i];
                            hn[1][t][i] = d1 * zx;
                            hn[2][t][i] = d1 * zy;
                            hn[3][t][i] = fmaf(d2 * zx, zx, d1 * acc[tb][3][i]);
                            hn[4][t][i] = fmaf(d2 * zx, zy, d1 * acc[tb][4][i]);
                            hn[5][t][i] = fmaf(d2 * zy, zy, d1 * acc[tb][5][i]);
                        }
                    }
            });
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int t = 0; t < NT; ++t) h[c][t] = hn[c][t];
        }
        // output layer: each lane contracts w_out with its H / 4 units per component; two shuffles sum the 4 lane groups
        float o[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) o[c] = 0.f;
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float wk = sw[16 * T + 4 * lg + i];
#pragma unroll
                for (int c = 0; c < NC; ++c) o[c] = fmaf(wk, h[c][T][i], o[c]);
            }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            o[c] += __shfl_xor(o[c], 16);
            o[c] += __shfl_xor(o[c], 32);
        }
        if (valid && lg == 0) {
            const float f = o[0] + w.b_out;
            if constexpr (FULL) {
                const float lm = lam ? lam[pi] : 1.f;
                store_point(out, pi, f, lm * o[1], lm * o[2], lm * o[3], lm * o[4], lm * o[5]);
            } else {
                out.val[pi * out.sv] = f;
            }
        }
    }
}

template <int H, int ACT, bool FULL>
static int launch_hdual(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                        const float* lam, const MlpOut& out, hipStream_t stream) {
    const size_t lds = sizeof(float) * hdual_lds_floats(H, w.n_hidden);
    static std::atomic<uint64_t> attr{0};
    NLOT_HIP_CHECK(set_lds_attr_once(attr, (const void*)mlp_hdual<H, ACT, FULL>, (int)(sizeof(float) * hdual_lds_floats(H, hdual_max_layers(H)))));
    const int grid = persistent_grid(n * P_per, 64, device_cus());
    hipLaunchKernelGGL((mlp_hdual<H, ACT, FULL>), dim3(grid), dim3(256), lds, stream, w, pts, n, n_dev, P_per, ld, lam, out);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

template <int H, int ACT>
static int launch_hdual_act(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                            const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return full ? launch_hdual<H, ACT, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                : launch_hdual<H, ACT, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
}

int launch_mlp_hdual(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                     const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    if (const char* why = hdual_refusal(w.act, w.H, w.n_hidden)) {  // nlot_mlp_create_ex has checked; a guard for LDS
        set_error(why);
        return NLOT_ERR_INVALID;
    }
    return dispatch_width<128>(w.H, [&](auto width) {
        constexpr int H = decltype(width)::value;
        switch (w.act) {
            case NLOT_ACT_TANH: return launch_hdual_act<H, NLOT_ACT_TANH>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
            case NLOT_ACT_SIGMOID: return launch_hdual_act<H, NLOT_ACT_SIGMOID>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
            case NLOT_ACT_LEAKY_RELU: return launch_hdual_act<H, NLOT_ACT_LEAKY_RELU>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
            default: return launch_hdual_act<H, NLOT_ACT_SINE>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
        }
    });
}

}  // namespace nlot
