// NLOT_MLP_ARITH_HDUAL_BF16 (ABI v24): mlp_hdual's forward hyper-dual algorithm (nlot_mlp_hdual.hip) with every HxH
// product made from split-bf16 operands on v_mfma_f32_16x16x32_bf16, as mlp_bf16 makes the ReLU nets' (nlot_mlp_bf16.hip).
// Both operands are split into three bf16 parts, x = h + m + l (split3), and an fp32 product is the six bf16 MFMA
// products mm, lh, hl, mh, hm, hh with fp32 accumulation, small terms first (mfma6's order, one accumulator).
//
// Mapping.  256 threads = 4 waves, one per SIMD with the whole 512-register file; a wave owns 16 points (MFMA column =
// point = lane & 15), a block tile is 64 points and the grid is persistent.  Per 16-unit output tile a wave carries
// NC = 6 (FULL) or 1 (value) accumulators of 4 registers per lane, register i = unit 16 t + 4 (lane >> 4) + i; the six
// of a tile share lane and register index, so the activation step is lane-local.  One 16x16x32 k block consumes 32
// input units, 8 per lane: slot j of lane group lg in block kb is unit 32 kb + 16 (j >> 2) + 4 lg + (j & 3), which are
// the eight values the lane holds after activating output tiles 2 kb and 2 kb + 1 of the previous layer (registers
// j & 3).  An activated tile pair is split in registers and is at once the three B operands of one k block of the next
// layer, per component; the A operand carries the same k permutation, fixed at creation.  (The MFMA pairs slot j of
// lane group lg of A with the same slot of B, so any unit order is right as long as both sides use it.)  Activations
// never leave registers between the input layer and the output contraction.
//
// The last HxH layer's activated tiles are not split or kept: each group of tiles is contracted with w_out in fp32 as
// it is produced (six running sums per lane), which is what makes H = 128 fit: 288 registers of split input, and no
// split output.
//
// Weights.  Every HxH layer is resident in LDS for the whole launch (copied once per block by 16-byte copies), as the
// image made at creation, [layer][part h, m, l][output tile t][k block kb][lane][8 bf16]: a lane's 16 bytes are row
// 16 t + (lane & 15) in the k-slot order above.  An A operand is one ds_read_b128 per part, lane-contiguous and so
// conflict-free without padding.  96 KB hold one layer at H = 128 or four at H = 64; biases, A, b0 and w_out sit
// beside the image in fp32.  One barrier per launch.
//
// In flight.  TB output tiles at a time: 1 in FULL at H = 128 (6 accumulators; no layer follows, so no tile pair has to
// be complete), 2 in FULL at H = 64 (12 accumulators, one tile pair = one k block of the next layer), 4 in value
// launches (4 accumulators).  For each of the six split products the MFMAs loop over the TB x NC accumulators, so
// consecutive MFMAs never share one, and an accumulator's own chain (k blocks in order, six products each) is the same
// in both instantiations: a value launch is bitwise the full launch's value.  The A operands of k block kb + 1 are read
// ahead of the MFMAs of block kb (one wave per SIMD: nothing else hides the LDS latency).
#include "nlot_mlp.h"

namespace nlot {

__host__ __device__ constexpr size_t hdual_bf16_lds_bytes(int H, int L) {
    return (size_t)L * 3 * H * H * 2 + ((size_t)4 * H + (size_t)L * H) * 4;
}

template <int H, int ACT, bool FULL>
__global__ __launch_bounds__(256, 1) void mlp_hdual_bf16(MlpDev w, const float* __restrict__ pts, int64_t cnt_host,
                                                         const int* __restrict__ cnt_dev, int P_per, int64_t ld,
                                                         const float* __restrict__ lam, MlpOut out) {
    constexpr int NC = FULL ? 6 : 1;  // hyper-dual components carried
    constexpr int NT = H / 16;        // 16-unit output tiles of a layer
    constexpr int NKB = H / 32;       // 32-unit k blocks of a layer (one per output tile pair of the layer before)
    constexpr int TB = FULL ? (H == 128 ? 1 : 2) : 4;  // output tiles in flight
    constexpr int TP = 64;            // points per block tile
    static_assert((TB % 2 == 0 || hdual_bf16_max_layers(H) == 1) && NT % TB == 0, "mlp_hdual_bf16 shape");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L = w.n_hidden;
    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    if ((int64_t)blockIdx.x * TP >= npts) return;  // a compacted launch: fewer tiles than blocks
    const int nfrag = L * 3 * NT * NKB * 64;        // 16-byte fragments of the image
    uint4* sWb = reinterpret_cast<uint4*>(smem);    // [L][3][NT][NKB][64]
    float* sA0 = smem + (size_t)4 * nfrag;          // [H]
    float* sA1 = sA0 + H;                           // [H]
    float* sb0 = sA1 + H;                           // [H]
    float* sw = sb0 + H;                            // [H]
    float* sbl = sw + H;                            // [L][H]
    for (int idx = threadIdx.x; idx < nfrag; idx += 256) sWb[idx] = reinterpret_cast<const uint4*>(w.Wb)[idx];
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
        // the layer's activations as B operands: part p of component c, slot j = unit 32 kb + 16 (j >> 2) + 4 lg + (j & 3)
        bf16x8 B[NKB][NC][3];
        // v (component c of the unit in register i of output tile t) into its slot of the next layer's operands
        auto put = [&](bf16x8 (&dst)[NKB][NC][3], int t, int c, int i, float v) {
            __bf16 hh, mm, ll;
            split3(v, hh, mm, ll);
            const int kb = t >> 1, j = 4 * (t & 1) + i;
            dst[kb][c][0][j] = hh;
            dst[kb][c][1][j] = mm;
            dst[kb][c][2][j] = ll;
        };
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
                put(B, T, 0, i, s);
                if constexpr (FULL) {
                    put(B, T, 1, i, d1 * a0);
                    put(B, T, 2, i, d1 * a1);
                    put(B, T, 3, i, d2 * a0 * a0);
                    put(B, T, 4, i, d2 * a0 * a1);
                    put(B, T, 5, i, d2 * a1 * a1);
                }
            }
        });
        float o[NC];  // the output layer's running sums over the lane's H / 4 units
#pragma unroll
        for (int c = 0; c < NC; ++c) o[c] = 0.f;
        // One HxH layer: z_c = W h_c for the NC components by split products, then the activation per (unit, point).
        // The last layer's activations go straight into o, the others' into Bn, the next layer's operands.
        auto layer = [&](int l, bf16x8 (&Bn)[NKB][NC][3], auto last_c) {
            constexpr bool LAST = decltype(last_c)::value;
            const bf16x8* Wl = reinterpret_cast<const bf16x8*>(sWb) + (size_t)l * 3 * NT * NKB * 64 + lane;
            const float* bl = sbl + l * H + 4 * lg;
            auto a_frag = [&](int part, int t, int kb) { return Wl[((part * NT + t) * NKB + kb) * 64]; };
            static_for<NT / TB>([&](auto gc) {
                constexpr int t0 = decltype(gc)::value * TB;
                f32x4 acc[TB][NC];
#pragma unroll
                for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[tb][c] = f32x4{};
                bf16x8 a_cur[TB][3];
#pragma unroll
                for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                    for (int p = 0; p < 3; ++p) a_cur[tb][p] = a_frag(p, t0 + tb, 0);
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) {
                    bf16x8 a_nxt[TB][3];
                    if (kb + 1 < NKB) {
#pragma unroll
                        for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                            for (int p = 0; p < 3; ++p) a_nxt[tb][p] = a_frag(p, t0 + tb, kb + 1);
                    }
                    auto prod = [&](int pa, int pb) {  // part pa of the weights times part pb of the activations
#pragma unroll
                        for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                            for (int c = 0; c < NC; ++c)
                                acc[tb][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_cur[tb][pa], B[kb][c][pb],
                                                                                     acc[tb][c], 0, 0, 0);
                    };
                    prod(1, 1);  // mm, lh, hl, mh, hm, hh: small terms first
                    prod(2, 0);
                    prod(0, 2);
                    prod(1, 0);
                    prod(0, 1);
                    prod(0, 0);
#pragma unroll
                    for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                        for (int p = 0; p < 3; ++p) a_cur[tb][p] = a_nxt[tb][p];
                    asm volatile("" ::: "memory");  // bound the LDS loads the scheduler hoists (register file)
                }
#pragma unroll
                for (int tb = 0; tb < TB; ++tb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int t = t0 + tb;
                        float v[NC], s, d1, d2;
                        act3(ACT, scale, acc[tb][0][i] + bl[16 * t + i], s, d1, d2);
                        v[0] = s;
                        if constexpr (FULL) {
                            const float zx = acc[tb][1][i], zy = acc[tb][2][i];
                            v[1] = d1 * zx;
                            v[2] = d1 * zy;
                            v[3] = fmaf(d2 * zx, zx, d1 * acc[tb][3][i]);
                            v[4] = fmaf(d2 * zx, zy, d1 * acc[tb][4][i]);
                            v[5] = fmaf(d2 * zy, zy, d1 * acc[tb][5][i]);
                        }
                        if constexpr (LAST) {
                            const float wk = sw[16 * t + 4 * lg + i];
#pragma unroll
                            for (int c = 0; c < NC; ++c) o[c] = fmaf(wk, v[c], o[c]);
                        } else {
#pragma unroll
                            for (int c = 0; c < NC; ++c) put(Bn, t, c, i, v[c]);
                        }
                    }
            });
        };
        if constexpr (hdual_bf16_max_layers(H) > 1) {
#pragma unroll 1
            for (int l = 0; l + 1 < L; ++l) {
                bf16x8 Bn[NKB][NC][3];
                layer(l, Bn, std::false_type{});
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
                    for (int c = 0; c < NC; ++c)
#pragma unroll
                        for (int p = 0; p < 3; ++p) B[kb][c][p] = Bn[kb][c][p];
            }
        }
        layer(L - 1, B, std::true_type{});  // (the last layer writes no operands)
        // output layer: two shuffles sum the 4 lane groups
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
static int launch_hdual_bf16(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                             const float* lam, const MlpOut& out, hipStream_t stream) {
    constexpr size_t lds_max = hdual_bf16_lds_bytes(H, hdual_bf16_max_layers(H));
    static_assert(lds_max <= 160 * 1024, "mlp_hdual_bf16 LDS");
    static std::atomic<uint64_t> attr{0};
    NLOT_HIP_CHECK(set_lds_attr_once(attr, (const void*)mlp_hdual_bf16<H, ACT, FULL>, (int)lds_max));
    const int grid = persistent_grid(n * P_per, 64, device_cus());
    hipLaunchKernelGGL((mlp_hdual_bf16<H, ACT, FULL>), dim3(grid), dim3(256), hdual_bf16_lds_bytes(H, w.n_hidden), stream, w,
                       pts, n, n_dev, P_per, ld, lam, out);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

template <int H, int ACT>
static int launch_hdual_bf16_act(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                                 const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return full ? launch_hdual_bf16<H, ACT, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                : launch_hdual_bf16<H, ACT, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
}

int launch_mlp_hdual_bf16(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                          const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    if (const char* why = hdual_bf16_refusal(w.act, w.H, w.n_hidden)) {  // nlot_mlp_create_ex has checked; a guard for LDS
        set_error(why);
        return NLOT_ERR_INVALID;
    }
    if (!w.Wb) {
        set_error("mlp_hdual_bf16: the net was not created with NLOT_MLP_ARITH_HDUAL_BF16");
        return NLOT_ERR_INVALID;
    }
    return dispatch_width<128>(w.H, [&](auto width) {
        constexpr int H = decltype(width)::value;
        switch (w.act) {
            case NLOT_ACT_TANH: return launch_hdual_bf16_act<H, NLOT_ACT_TANH>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
            case NLOT_ACT_SIGMOID: return launch_hdual_bf16_act<H, NLOT_ACT_SIGMOID>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
            case NLOT_ACT_LEAKY_RELU: return launch_hdual_bf16_act<H, NLOT_ACT_LEAKY_RELU>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
            default: return launch_hdual_bf16_act<H, NLOT_ACT_SINE>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
        }
    });
}

}  // namespace nlot
