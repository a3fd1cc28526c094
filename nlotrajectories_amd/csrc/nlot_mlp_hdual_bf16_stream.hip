// NLOT_MLP_ARITH_HDUAL_BF16_STREAM (ABI v25): mlp_hdual_stream's split of the work (nlot_mlp_hdual_stream.hip) with
// mlp_hdual_bf16's products (nlot_mlp_hdual_bf16.hip), for the smooth nets whose split layers fit neither the LDS nor the
// registers of mlp_hdual_bf16: H = 128 with 2-4 HxH layers and H = 256.  Every HxH product is six bf16 MFMA products of
// operands split into three bf16 parts, x = h + m + l (split3), in mfma6's order mm, lh, hl, mh, hm, hh with fp32
// accumulation in one accumulator.
//
// Mapping (v_mfma_f32_16x16x32_bf16).  256 threads = 4 waves, one per SIMD; a block tile is G groups of 16 points (MFMA
// column = point = lane & 15), all four waves work on the same points and the grid is persistent.  Wave w owns output
// units [w H/4, (w + 1) H/4) of every layer, NQ = H/64 sixteen-unit tiles; per tile and group it carries NC = 6 (FULL)
// or 1 (value) accumulators of 4 registers, register i = row 16 t + 4 (lane >> 4) + i, so the activation step is
// lane-local across the six components.  G = 256 / H in FULL (96 accumulator registers), 4 in value launches.
//
// Activations live in LDS already split: one bf16 buffer act[component][part h, m, l][point][unit], point stride
// PS = H + 8.  One k block is 32 input units, slot j of lane group lg in block kb being unit 32 kb + 8 lg + j: a lane's B
// operand for one (component, part, group) is one ds_read_b128 of its own point's row, and the weight image carries the
// same map (the MFMA pairs slot j of A with slot j of B, whatever the hardware's own k order).  The 16 lanes of a lane
// group differ in the point only, PS / 2 = 4 (mod 64) dwords apart: 16 disjoint bank quads.  After its accumulation a
// wave applies act3 in fp32, splits each activated value ONCE (the four consumer waves read parts, they do not split)
// and writes its 4 consecutive units as one ds_write_b64 per (component, part, tile, group), in place: two barriers
// per layer (every wave has read the input; every wave has written the output).  The input layer is computed per lane
// in fp32, split and written straight into the buffer, each wave its quarter of the units.  The last HxH layer's
// activations are neither split nor stored: the wave contracts them with w_out in fp32 from registers, two __shfl_xor
// sum the four lane groups, and the four waves' partials are summed through LDS in wave order 0..3.
//
// LDS.  The buffer is 6 x 3 x 16 G x (H + 8) x 2 bytes: 152,064 at H = 256 (G = 1), 156,672 at H = 128 (G = 2).  Only
// A, b0, w_out (4 H floats) and the waves' partials sit beside it; the layers' biases stay in global memory and are
// read where the activation needs them, four per lane and tile.
//
// Weights never pass through LDS.  nlot_mlp_create_ex splits the HxH layers on the host and repacks them into fragment
// order [layer][wave][kb][tile t][part][lane][8 bf16], lane (row = lane & 15, lg) holding
// W[16 (w NQ + t) + row][32 kb + 8 lg ..+7] (MlpDev::Ws): a wave's A operand for one (kb, tile, part) is one coalesced
// 1 KB global_load_dwordx4.  The 3 NQ operands of block kb + 1 are fetched ahead of the MFMAs of block kb; the last
// iteration fetches its own again rather than branch.
//
// In flight.  Components in the outer loop: the B operands of one component (3 parts x G) are live while the next
// component's (or the next block's component 0) are being read.  For each of the six split products the MFMAs loop
// over the component's NQ x G accumulators, so consecutive MFMAs never share one.  An accumulator's own chain (k blocks
// in order, six products each) does not depend on NC or G, and act3 and the output reduction are shared: a value
// launch is bitwise the full launch's value.
#include "nlot_mlp.h"

namespace nlot {

__host__ __device__ constexpr int hbs_groups(int H, bool full) { return full ? 256 / H : 4; }
__host__ __device__ constexpr size_t hbs_act_bytes(int H, bool full) {
    return (size_t)(full ? 6 : 1) * 3 * 16 * hbs_groups(H, full) * (H + 8) * 2;
}
__host__ __device__ constexpr size_t hbs_lds_bytes(int H, bool full) {
    // act, then A (2 rows), b0 and w_out, then the waves' output partials
    return hbs_act_bytes(H, full) + ((size_t)4 * H + (size_t)4 * (full ? 6 : 1) * 16 * hbs_groups(H, full)) * 4;
}

template <int H, int ACT, bool FULL>
__global__ __launch_bounds__(256, 1) void mlp_hdual_bf16_stream(MlpDev w, const float* __restrict__ pts,
                                                                int64_t cnt_host, const int* __restrict__ cnt_dev,
                                                                int P_per, int64_t ld, const float* __restrict__ lam,
                                                                MlpOut out) {
    constexpr int NC = FULL ? 6 : 1;  // hyper-dual components carried
    constexpr int NKB = H / 32;       // 32-unit k blocks of a layer
    constexpr int NQ = H / 64;        // 16-unit output tiles of a wave
    constexpr int G = hbs_groups(H, FULL);
    constexpr int TP = 16 * G;        // points per block tile
    constexpr int PS = H + 8;         // point stride of act, in bf16
    static_assert((PS / 2) % 64 == 4 && PS % 8 == 0 && NQ * NC * G * 4 <= 96, "mlp_hdual_bf16_stream shape");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L = w.n_hidden;
    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    if ((int64_t)blockIdx.x * TP >= npts) return;  // a compacted launch: fewer tiles than blocks
    __bf16* sAct = reinterpret_cast<__bf16*>(smem);  // [NC][3][TP][PS]
    float* sA0 = smem + NC * 3 * TP * PS / 2;        // [H]
    float* sA1 = sA0 + H;                            // [H]
    float* sb0 = sA1 + H;                            // [H]
    float* sw = sb0 + H;                             // [H]
    float* sPart = sw + H;                           // [4 waves][NC][TP]
    for (int idx = threadIdx.x; idx < H; idx += 256) {
        sA0[idx] = w.A[idx];
        sA1[idx] = w.A[H + idx];
        sb0[idx] = w.b0[idx];
        sw[idx] = w.w_out[idx];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pn = lane & 15, lg = lane >> 4;  // point of the lane; lane group (k offset 8 lg, row offset 4 lg)
    const bool fourier = w.in_kind == NLOT_MLP_IN_FOURIER;
    const float scale = w.scale;  // Fourier scale, or SIREN's omega_0
    __bf16* actl = sAct + pn * PS;  // the lane's point in part 0 of component 0, group 0
    // the lane's four units u0 + 4 lg ..+3 of component c, group g: split once, one 8-byte store per part
    auto put = [&](int c, int g, int u0, const f32x4& v) {
        bf16x4 part[3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __bf16 hh, mm, ll;
            split3(v[i], hh, mm, ll);
            part[0][i] = hh;
            part[1][i] = mm;
            part[2][i] = ll;
        }
#pragma unroll
        for (int p = 0; p < 3; ++p)
            *reinterpret_cast<bf16x4*>(actl + ((c * 3 + p) * TP + g * 16) * PS + u0 + 4 * lg) = part[p];
    };
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
            for (int c = 0; c < NC; ++c) put(c, g, u0, hn[c]);
        });
        __syncthreads();
        float o[G][NC];  // the wave's part of the output contraction
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int c = 0; c < NC; ++c) o[g][c] = 0.f;
        // HxH layers: z_c = W h_c for the NC components and the wave's rows by split products, then the activation
        // per (unit, point)
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            // the wave's fragments of layer l: operand (kb, t, part) at 64 ((kb NQ + t) 3 + part) fragments of 16 bytes
            const bf16x8* Wl = reinterpret_cast<const bf16x8*>(w.Ws) + (size_t)(l * 4 + wave) * NKB * NQ * 3 * 64 + lane;
            const __bf16* bl = actl + 8 * lg;  // the lane's slots of k block 0
            f32x4 acc[NQ][G][NC];
#pragma unroll
            for (int t = 0; t < NQ; ++t)
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[t][g][c] = f32x4{};
            bf16x8 a_cur[NQ][3], b_cur[G][3];
#pragma unroll
            for (int t = 0; t < NQ; ++t)
#pragma unroll
                for (int p = 0; p < 3; ++p) a_cur[t][p] = Wl[(t * 3 + p) * 64];
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int p = 0; p < 3; ++p) b_cur[g][p] = *reinterpret_cast<const bf16x8*>(bl + (p * TP + g * 16) * PS);
#pragma unroll 2
            for (int kb = 0; kb < NKB; ++kb) {
                const int kbn = kb + 1 < NKB ? kb + 1 : kb;
                bf16x8 a_nxt[NQ][3];
#pragma unroll
                for (int t = 0; t < NQ; ++t)
#pragma unroll
                    for (int p = 0; p < 3; ++p) a_nxt[t][p] = Wl[((kbn * NQ + t) * 3 + p) * 64];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    // the next component's operands of this block, or component 0's of the next block
                    const int cn = c + 1 < NC ? c + 1 : 0, kn = c + 1 < NC ? kb : kbn;
                    bf16x8 b_nxt[G][3];
#pragma unroll
                    for (int g = 0; g < G; ++g)
#pragma unroll
                        for (int p = 0; p < 3; ++p)
                            b_nxt[g][p] = *reinterpret_cast<const bf16x8*>(bl + ((cn * 3 + p) * TP + g * 16) * PS + 32 * kn);
                    auto prod = [&](int pa, int pb) {  // part pa of the weights times part pb of the activations
#pragma unroll
                        for (int t = 0; t < NQ; ++t)
#pragma unroll
                            for (int g = 0; g < G; ++g)
                                acc[t][g][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_cur[t][pa], b_cur[g][pb],
                                                                                       acc[t][g][c], 0, 0, 0);
                    };
                    prod(1, 1);  // mm, lh, hl, mh, hm, hh: small terms first
                    prod(2, 0);
                    prod(0, 2);
                    prod(1, 0);
                    prod(0, 1);
                    prod(0, 0);
#pragma unroll
                    for (int g = 0; g < G; ++g)
#pragma unroll
                        for (int p = 0; p < 3; ++p) b_cur[g][p] = b_nxt[g][p];
                }
#pragma unroll
                for (int t = 0; t < NQ; ++t)
#pragma unroll
                    for (int p = 0; p < 3; ++p) a_cur[t][p] = a_nxt[t][p];
            }
            __syncthreads();  // every wave has read the layer's input: act may be overwritten
            const bool last = l == L - 1;
            const float* bias = w.b + l * H + 4 * lg;
            static_for<NQ * G>([&](auto ic) {
                constexpr int t = decltype(ic)::value / G, g = decltype(ic)::value % G;
                const int u0 = 16 * (wave * NQ + t);
                const f32x4 bq = *reinterpret_cast<const f32x4*>(bias + u0);
                f32x4 hn[NC];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float s, d1, d2;
                    act3(ACT, scale, acc[t][g][0][i] + bq[i], s, d1, d2);
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
                    for (int c = 0; c < NC; ++c) put(c, g, u0, hn[c]);
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
static int launch_hbs(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                      const float* lam, const MlpOut& out, hipStream_t stream) {
    constexpr size_t lds = hbs_lds_bytes(H, FULL);
    static_assert(lds <= 160 * 1024, "mlp_hdual_bf16_stream LDS");
    static std::atomic<uint64_t> attr{0};
    NLOT_HIP_CHECK(set_lds_attr_once(attr, (const void*)mlp_hdual_bf16_stream<H, ACT, FULL>, (int)lds));
    const int grid = persistent_grid(n * P_per, 16 * hbs_groups(H, FULL), device_cus());
    hipLaunchKernelGGL((mlp_hdual_bf16_stream<H, ACT, FULL>), dim3(grid), dim3(256), lds, stream, w, pts, n, n_dev, P_per, ld,
                       lam, out);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

template <int H, int ACT>
static int launch_hbs_act(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                          const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return full ? launch_hbs<H, ACT, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                : launch_hbs<H, ACT, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
}

template <int H>
static int launch_hbs_width(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                            const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    switch (w.act) {
        case NLOT_ACT_TANH: return launch_hbs_act<H, NLOT_ACT_TANH>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
        case NLOT_ACT_SIGMOID: return launch_hbs_act<H, NLOT_ACT_SIGMOID>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
        case NLOT_ACT_LEAKY_RELU: return launch_hbs_act<H, NLOT_ACT_LEAKY_RELU>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
        default: return launch_hbs_act<H, NLOT_ACT_SINE>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
    }
}

int launch_mlp_hdual_bf16_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                                 const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    if (const char* why = hdual_bf16_stream_refusal(w.act, w.H, w.n_hidden)) {  // nlot_mlp_create_ex has checked; a
        set_error(why);                                                          // guard for Ws and the widths compiled
        return NLOT_ERR_INVALID;
    }
    if (!w.Ws) {
        set_error("mlp_hdual_bf16_stream: the net was not created with NLOT_MLP_ARITH_HDUAL_BF16_STREAM");
        return NLOT_ERR_INVALID;
    }
    return w.H == 128 ? launch_hbs_width<128>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream)
                      : launch_hbs_width<256>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
}

}  // namespace nlot
