// NLOT_MLP_ARITH_HDUAL_STREAM (ABI v22): the MFMA hyper-dual arithmetic of mlp_hdual (nlot_mlp_hdual.hip) for the
// smooth nets that kernel cannot hold: H = 256, and H = 128 with 3 or 4 HxH layers.  There every layer sits in LDS and
// every activation in registers; at H = 256 the six components of 16 points are 384 registers for a layer's input
// alone, and three 128 x 132 layers are 203 KB.  Here it is the other way round: the four waves of a block split the
// UNITS of a layer, the activations live in LDS, and the weights stream from L2 straight into registers.
//
// Mapping (v_mfma_f32_16x16x4_f32).  256 threads = 4 waves, one per SIMD; a block tile is G groups of 16 points (MFMA
// column = point = lane & 15) and all four waves work on the same points.  Wave w owns output units
// [w H/4, (w + 1) H/4) of every layer, NQ = H/64 sixteen-unit tiles; per tile and point group it carries NC = 6
// (FULL) or 1 (value) accumulators of 4 registers, register i = row 16 t + 4 (lane >> 4) + i as in mlp_hdual, so the
// activation step is lane-local across the six components.  G is chosen so that a wave holds 96 accumulator registers
// in FULL (H = 256: G = 1, 128: 2, 64: 4) and 64 or fewer in value (G = 4).
//
// Activations.  One LDS buffer act[c][point][unit], point stride PS = H + 4 floats.  The B operands of the four k-steps
// (T, 0..3) are the four consecutive units 16 T + 4 lg ..+3 of the lane's point: one ds_read_b128 per component and
// group.  The 16 lanes of a lane group differ in the point only, PS floats apart, and PS = 4 (mod 64) puts them on 16
// disjoint bank quads (mlp_hdual's argument for its weight rows).  After its accumulation a wave applies act3 and
// writes each activated tile back as one ds_write_b128 per (component, tile, group) into the same layout, in place:
// two barriers per layer (every wave has read the input; every wave has written the output).  The input layer is
// computed per lane straight into the buffer, each wave its quarter of the units.  The last HxH layer's activations
// are not written: the wave contracts them with w_out from registers, two __shfl_xor sum the four lane groups, and
// the four waves' partials are summed through LDS in wave order 0..3.
//
// Weights never pass through LDS: a wave reads only its own rows, so staging would buy no sharing.
// nlot_mlp_create_ex repacks the HxH layers into fragment order [layer][wave][T][tile t][lane][4 floats], lane
// (pn, lg) holding W[16 (w NQ + t) + pn][16 T + 4 lg ..+3] (MlpDev::Wf), so that the A quad of a wave is one coalesced
// 1 KB global_load_dwordx4.  It feeds 4 NC G MFMAs (24 to 96); the quads and the B operands of input tile T + 1 are
// fetched ahead of the MFMAs of tile T.
//
// The value-only instantiation runs the component-0 chain with the same k order, the same act3 and the same output
// reduction order: a value launch is bitwise the full launch's value.
#include "nlot_mlp.h"

namespace nlot {

__host__ __device__ constexpr int hstream_groups(int H, bool full) { return full ? 256 / H : 4; }
__host__ __device__ constexpr size_t hstream_lds_floats(int H, bool full) {
    const int nc = full ? 6 : 1, tp = 16 * hstream_groups(H, full);
    // act, then A (2 rows), b0, w_out and the layers' biases, then the waves' output partials
    return (size_t)nc * tp * (H + 4) + (size_t)(4 + kMaxStreamLayers) * H + (size_t)4 * nc * tp;
}

template <int H, int ACT, bool FULL>
__global__ __launch_bounds__(256, 1) void mlp_hdual_stream(MlpDev w, const float* __restrict__ pts, int64_t cnt_host,
                                                           const int* __restrict__ cnt_dev, int P_per, int64_t ld,
                                                           const float* __restrict__ lam, MlpOut out) {
    constexpr int NC = FULL ? 6 : 1;  // hyper-dual components carried
    constexpr int NT = H / 16;        // 16-unit input tiles of a layer
    constexpr int NQ = H / 64;        // 16-unit output tiles of a wave
    constexpr int G = hstream_groups(H, FULL);
    constexpr int TP = 16 * G;        // points per block tile
    constexpr int PS = H + 4;         // point stride of act
    static_assert(PS % 64 == 4 && NQ * NC * G * 4 <= 96, "mlp_hdual_stream shape");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L = w.n_hidden;
    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    if ((int64_t)blockIdx.x * TP >= npts) return;  // a compacted launch: fewer tiles than blocks
    float* sAct = smem;                        // [NC][TP][PS]
    float* sA0 = sAct + NC * TP * PS;          // [H]
    float* sA1 = sA0 + H;                      // [H]
    float* sb0 = sA1 + H;                      // [H]
    float* sw = sb0 + H;                       // [H]
    float* sbl = sw + H;                       // [L][H]
    float* sPart = sbl + kMaxStreamLayers * H; // [4 waves][NC][TP]
    for (int idx = threadIdx.x; idx < H; idx += 256) {
        sA0[idx] = w.A[idx];
        sA1[idx] = w.A[H + idx];
        sb0[idx] = w.b0[idx];
        sw[idx] = w.w_out[idx];
    }
    for (int idx = threadIdx.x; idx < L * H; idx += 256) sbl[idx] = w.b[idx];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pn = lane & 15, lg = lane >> 4;  // point of the lane; lane group (k / row offset 4 lg)
    const bool fourier = w.in_kind == NLOT_MLP_IN_FOURIER;
    const float scale = w.scale;  // Fourier scale, or SIREN's omega_0
    float* actl = sAct + pn * PS + 4 * lg;  // the lane's quad of tile 0, component 0, group 0
    for (int64_t tile = blockIdx.x; tile * TP < npts; tile += gridDim.x) {
        // input layer: z = p A + b0 (as torch: p @ A then + b0), dz/dp = (A0, A1), d2z = 0; the wave's units only
        static_for<NQ * G>([&](auto ic) {
            constexpr int t = decltype(ic)::value / G, g = decltype(ic)::value % G;
            const int64_t gi = tile * TP + g * 16 + pn;
            float px = 0.f, py = 0.f;
            if (gi < npts) {
                const int64_t pi = point_addr(gi, cnt, ld);
                px = pts[2 * pi];
                py = pts[2 * pi + 1];
            }
            const int u0 = 16 * (wave * NQ + t);
            f32x4 hn[NC];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = u0 + 4 * lg + i;
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
                hn[0][i] = s;
                if constexpr (FULL) {
                    hn[1][i] = d1 * a0;
                    hn[2][i] = d1 * a1;
                    hn[3][i] = d2 * a0 * a0;
                    hn[4][i] = d2 * a0 * a1;
                    hn[5][i] = d2 * a1 * a1;
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) *reinterpret_cast<f32x4*>(actl + (c * TP + g * 16) * PS + u0) = hn[c];
        });
        __syncthreads();
        float o[G][NC];  // the wave's part of the output contraction
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int c = 0; c < NC; ++c) o[g][c] = 0.f;
        // HxH layers: z_c = W h_c for the NC components and the wave's rows, then the activation per (unit, point)
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            // the wave's fragments of layer l: quad (T, t) at 256 (T NQ + t) floats
            const float* Wl = w.Wf + ((size_t)(l * 4 + wave) * NT * NQ * 64 + lane) * 4;
            f32x4 acc[NQ][G][NC];
#pragma unroll
            for (int t = 0; t < NQ; ++t)
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[t][g][c] = f32x4{};
            // operands of input tile T + 1 are fetched ahead of the MFMAs of tile T (one wave per SIMD: nothing else
            // hides the L2 and LDS latency); the last iteration fetches its own again rather than branch
            f32x4 a_cur[NQ], b_cur[G][NC];
#pragma unroll
            for (int t = 0; t < NQ; ++t) a_cur[t] = *reinterpret_cast<const f32x4*>(Wl + 256 * t);
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int c = 0; c < NC; ++c) b_cur[g][c] = *reinterpret_cast<const f32x4*>(actl + (c * TP + g * 16) * PS);
#pragma unroll 2
            for (int T = 0; T < NT; ++T) {
                const int Tn = T + 1 < NT ? T + 1 : T;
                f32x4 a_nxt[NQ], b_nxt[G][NC];
#pragma unroll
                for (int t = 0; t < NQ; ++t) a_nxt[t] = *reinterpret_cast<const f32x4*>(Wl + 256 * (Tn * NQ + t));
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        b_nxt[g][c] = *reinterpret_cast<const f32x4*>(actl + (c * TP + g * 16) * PS + 16 * Tn);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < NQ; ++t)
#pragma unroll
                        for (int g = 0; g < G; ++g)
#pragma unroll
                            for (int c = 0; c < NC; ++c)
                                acc[t][g][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[t][i], b_cur[g][c][i], acc[t][g][c], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < NQ; ++t) a_cur[t] = a_nxt[t];
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int c = 0; c < NC; ++c) b_cur[g][c] = b_nxt[g][c];
            }
            __syncthreads();  // every wave has read the layer's input: act may be overwritten
            const bool last = l == L - 1;
            const float* bl = sbl + l * H + 4 * lg;
            static_for<NQ * G>([&](auto ic) {
                constexpr int t = decltype(ic)::value / G, g = decltype(ic)::value % G;
                const int u0 = 16 * (wave * NQ + t);
                f32x4 hn[NC];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float s, d1, d2;
                    act3(ACT, scale, acc[t][g][0][i] + bl[u0 + i], s, d1, d2);
                    hn[0][i] = s;
                    if constexpr (FULL) {
                        const float zx = acc[t][g][1][i], zy = acc[t][g][2][i];
                        hn[1][i] = d1 * zx;
                        hn[2][i] = d1 * zy;
                        hn[3][i] = fmaf(d2 * zx, zx, d1 * acc[t][g][3][i]);
                        hn[4][i] = fmaf(d2 * zx, zy, d1 * acc[t][g][4][i]);
                        hn[5][i] = fmaf(d2 * zy, zy, d1 * acc[t][g][5][i]);
                    }
                }
                if (!last) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) *reinterpret_cast<f32x4*>(actl + (c * TP + g * 16) * PS + u0) = hn[c];
                } else {  // output layer: the lane contracts w_out with its units, tile by tile in index order
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float wk = sw[u0 + 4 * lg + i];
#pragma unroll
                        for (int c = 0; c < NC; ++c) o[g][c] = fmaf(wk, hn[c][i], o[g][c]);
                    }
                }
            });
            __syncthreads();  // every wave has written the layer's output
        }
        // two shuffles sum the 4 lane groups; the 4 waves' partials go through LDS and are summed in wave order
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                float v = o[g][c];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (lg == 0) sPart[(wave * NC + c) * TP + g * 16 + pn] = v;
            }
        __syncthreads();  // the next tile writes sPart only after its own layer barriers
        const int64_t gi = tile * TP + threadIdx.x;
        if (threadIdx.x < TP && gi < npts) {
            const int64_t pi = point_addr(gi, cnt, ld);
            float r[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float* p = sPart + c * TP + threadIdx.x;
                r[c] = ((p[0] + p[NC * TP]) + p[2 * NC * TP]) + p[3 * NC * TP];
            }
            const float f = r[0] + w.b_out;
            if constexpr (FULL) {
                const float lm = lam ? lam[pi] : 1.f;
                store_point(out, pi, f, lm * r[1], lm * r[2], lm * r[3], lm * r[4], lm * r[5]);
            } else {
                out.val[pi * out.sv] = f;
            }
        }
    }
}

template <int H, int ACT, bool FULL>
static int launch_hstream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                          const float* lam, const MlpOut& out, hipStream_t stream) {
    constexpr size_t lds = sizeof(float) * hstream_lds_floats(H, FULL);
    static_assert(lds <= 160 * 1024, "mlp_hdual_stream LDS");
    static std::atomic<uint64_t> attr{0};
    NLOT_HIP_CHECK(set_lds_attr_once(attr, (const void*)mlp_hdual_stream<H, ACT, FULL>, (int)lds));
    const int grid = persistent_grid(n * P_per, 16 * hstream_groups(H, FULL), device_cus());
    hipLaunchKernelGGL((mlp_hdual_stream<H, ACT, FULL>), dim3(grid), dim3(256), lds, stream, w, pts, n, n_dev, P_per, ld, lam, out);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

template <int H, int ACT>
static int launch_hstream_act(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                              const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return full ? launch_hstream<H, ACT, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                : launch_hstream<H, ACT, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
}

int launch_mlp_hdual_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                            const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    if (const char* why = hdual_stream_refusal(w.act, w.H, w.n_hidden)) {  // nlot_mlp_create_ex has checked; a guard
        set_error(why);                                                     // for the biases' LDS and for Wf
        return NLOT_ERR_INVALID;
    }
    if (!w.Wf) {
        set_error("mlp_hdual_stream: the net was not created with NLOT_MLP_ARITH_HDUAL_STREAM");
        return NLOT_ERR_INVALID;
    }
    return dispatch_width(w.H, [&](auto width) {
        constexpr int H = decltype(width)::value;
        switch (w.act) {
            case NLOT_ACT_TANH: return launch_hstream_act<H, NLOT_ACT_TANH>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
            case NLOT_ACT_SIGMOID: return launch_hstream_act<H, NLOT_ACT_SIGMOID>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
            case NLOT_ACT_LEAKY_RELU: return launch_hstream_act<H, NLOT_ACT_LEAKY_RELU>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
            default: return launch_hstream_act<H, NLOT_ACT_SINE>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
        }
    });
}

}  // namespace nlot
