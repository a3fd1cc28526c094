// NLOT_MLP_ARITH_SPLIT_BF16_STREAM (ABI v26): the ReLU nets' forward pass and reverse sweep (as mlp_stream computes them,
// nlot_mlp_stream.hip) on mlp_hdual_bf16_stream's split of the work and its products (nlot_mlp_hdual_bf16_stream.hip),
// for the ReLU nets whose layers do not fit in LDS: H = 128 or 256 with 1-4 HxH layers.  Every HxH product, W h in the
// forward pass and W^T e in the reverse sweep, is six bf16 MFMA products of operands split into three bf16 parts,
// x = h + m + l (split3), with fp32 accumulation.
//
// Mapping (v_mfma_f32_16x16x32_bf16).  256 threads = 4 waves, one per SIMD; a block tile is G groups of 16 points (MFMA
// column = point = lane & 15), all four waves work on the same points and the grid is persistent.  Wave w owns units
// [w H/4, (w + 1) H/4) of every layer, NQ = H/64 sixteen-unit tiles: the outputs of a forward product, the inputs of the
// layer in a reverse one.  Per tile and group it carries one accumulator of 4 registers, register i = row 16 t +
// 4 (lane >> 4) + i.  One component is carried where the hyper-dual kernel carries six, so the tile is six times as wide
// for the same registers and LDS: G = 1536 / H, 96 points at H = 256 and 192 at H = 128 (96 accumulator registers), in
// value and full launches alike.  A weight fragment fetched from L2 feeds 96 or 192 MFMA columns.
//
// Activations live in LDS already split: one bf16 buffer act[part h, m, l][point][unit], point stride PS = H + 8, with
// the slot map, bank spread and 8-byte in-place writes of mlp_hdual_bf16_stream; two barriers per layer (every wave has
// read the input; every wave has written the output).  The reverse sweep's e lives in the same buffer, split the same
// way: after the forward pass only the ReLU patterns are needed, and those are bits in registers of the wave that owns
// the units, 4 per (tile, group, layer) and lane (96 per layer), never in LDS or memory.  The layer loops are rolled, so
// a layer's words are written and read through selects on the layer index, not indexed.
//
// Weights never pass through LDS.  nlot_mlp_create_ex splits the HxH layers on the host into two images in fragment
// order [layer][wave][kb][tile t][part][lane][8 bf16]: MlpDev::Ws, lane (row, lg) holding W[16 (w NQ + t) + row]
// [32 kb + 8 lg ..+7], for the forward products, and MlpDev::Wr, the same lane holding W[32 kb + 8 lg ..+7]
// [16 (w NQ + t) + row], for the reverse ones: both sweeps run one product loop, on the other image.  A wave's A operand
// for one (kb, tile, part) is one coalesced 1 KB global_load_dwordx4; the 3 NQ operands of block kb + 1 are fetched
// ahead of the MFMAs of block kb, and the last iteration fetches its own again rather than branch.
//
// In flight.  Within a k block the groups go in pairs: the B operands of one pair (3 parts x 2 groups, one ds_read_b128
// each) are live while the next pair's (or the next block's first pair's) are being read, and for each of the six split
// products the MFMAs loop over the pair's 2 NQ accumulators, so consecutive MFMAs never share one.  The forward products
// go into one accumulator in mfma6's order mm, lh, hl, mh, hm, hh.  In the reverse sweep the five smaller products go
// into a running accumulator of their own and hh into the main one, added once per output tile (mfma5s,
// nlot_mlp_bf16.hip: one MFMA accumulator drops the low bits of small products added to a large running sum).  An
// accumulator's chain (k blocks in order, six products each) does not depend on the group, the pairing or the launch.
//
// Output.  A wave contracts its quarter in fp32 from registers, in unit order: f with w_out after the last forward
// layer, and after the reverse sweep d = lam df/dh0 with the input layer by input_contract (gradient for both input
// layers; Hessian A diag(d .* (-scale cos z)) A^T for Fourier, 0 for Linear+ReLU).  Two __shfl_xor sum the lane groups
// and the four waves' partials are summed through LDS in wave order 0..3 (the gradient's and Hessian's in the head of
// the activation buffer, free by then).  Every sum has a fixed order: a point's results are bitwise independent of P, of
// its place in the launch and of the addressing, and the value launch, the forward part alone, is bitwise the full
// launch's value.
#include "nlot_mlp.h"

namespace nlot {

__host__ __device__ constexpr int rbs_groups(int H) { return 1536 / H; }
__host__ __device__ constexpr size_t rbs_act_bytes(int H) { return (size_t)3 * 16 * rbs_groups(H) * (H + 8) * 2; }
__host__ __device__ constexpr size_t rbs_lds_bytes(int H) {
    // act, then A (2 rows), b0 and w_out, then the waves' partials of f
    return rbs_act_bytes(H) + ((size_t)4 * H + (size_t)4 * 16 * rbs_groups(H)) * 4;
}

template <int H, bool FOURIER, bool FULL>
__global__ __launch_bounds__(256, 1) void mlp_relu_bf16_stream(MlpDev w, const float* __restrict__ pts, int64_t cnt_host,
                                                               const int* __restrict__ cnt_dev, int P_per, int64_t ld,
                                                               const float* __restrict__ lam, MlpOut out) {
    constexpr int NKB = H / 32;  // 32-unit k blocks of a layer
    constexpr int NQ = H / 64;   // 16-unit tiles of a wave
    constexpr int G = rbs_groups(H);
    constexpr int TP = 16 * G;   // points per block tile
    constexpr int PS = H + 8;    // point stride of act, in bf16
    constexpr int MW = NQ * G * 4 / 32;  // words of a layer's ReLU pattern per lane
    static_assert((PS / 2) % 64 == 4 && PS % 8 == 0 && G % 2 == 0 && NQ * G * 4 == 96 && TP <= 256 &&
                      (size_t)20 * TP * 4 <= rbs_act_bytes(H),
                  "mlp_relu_bf16_stream shape");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L = w.n_hidden;
    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    if ((int64_t)blockIdx.x * TP >= npts) return;  // a compacted launch: fewer tiles than blocks
    __bf16* sAct = reinterpret_cast<__bf16*>(smem);  // [3][TP][PS]
    float* sPart = smem;                             // [4 waves][5][TP] after the reverse sweep, in act's place
    float* sA0 = smem + 3 * TP * PS / 2;             // [H]
    float* sA1 = sA0 + H;                            // [H]
    float* sb0 = sA1 + H;                            // [H]
    float* sw = sb0 + H;                             // [H]
    float* sF = sw + H;                              // [4 waves][TP]
    for (int idx = threadIdx.x; idx < H; idx += 256) {
        sA0[idx] = w.A[idx];
        sA1[idx] = w.A[H + idx];
        sb0[idx] = w.b0[idx];
        sw[idx] = w.w_out[idx];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pn = lane & 15, lg = lane >> 4;  // point of the lane; lane group (k offset 8 lg, row offset 4 lg)
    const float scale = w.scale;
    __bf16* actl = sAct + pn * PS;     // the lane's point in part 0, group 0
    const __bf16* bl = actl + 8 * lg;  // the lane's slots of k block 0
    // the lane's four units u0 + 4 lg ..+3 of group g: split once, one 8-byte store per part
    auto put = [&](int g, int u0, const f32x4& v) {
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
        for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x4*>(actl + (p * TP + g * 16) * PS + u0 + 4 * lg) = part[p];
    };
    f32x4 acc[NQ][G], acs[FULL ? NQ : 1][FULL ? G : 1];
    // acc (+ acs) = the wave's rows of (image Wl) x (act): Wl the wave's fragments of one layer, operand (kb, t, part)
    // at 64 ((kb NQ + t) 3 + part) fragments of 16 bytes.  rev: the five smaller products into acs.
    auto product = [&](auto rev, const bf16x8* Wl) {
        constexpr bool REV = decltype(rev)::value;
#pragma unroll
        for (int t = 0; t < NQ; ++t)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                acc[t][g] = f32x4{};
                if constexpr (REV) acs[t][g] = f32x4{};
            }
        bf16x8 a_cur[NQ][3], b_cur[2][3];
#pragma unroll
        for (int t = 0; t < NQ; ++t)
#pragma unroll
            for (int p = 0; p < 3; ++p) a_cur[t][p] = Wl[(t * 3 + p) * 64];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int p = 0; p < 3; ++p) b_cur[h][p] = *reinterpret_cast<const bf16x8*>(bl + (p * TP + h * 16) * PS);
#pragma unroll 1
        for (int kb = 0; kb < NKB; ++kb) {
            const int kbn = kb + 1 < NKB ? kb + 1 : kb;
            bf16x8 a_nxt[NQ][3];
#pragma unroll
            for (int t = 0; t < NQ; ++t)
#pragma unroll
                for (int p = 0; p < 3; ++p) a_nxt[t][p] = Wl[((kbn * NQ + t) * 3 + p) * 64];
#pragma unroll
            for (int gp = 0; gp < G / 2; ++gp) {
                // the next pair's operands of this block, or the first pair's of the next block
                const int gn = gp + 1 < G / 2 ? gp + 1 : 0, kn = gp + 1 < G / 2 ? kb : kbn;
                bf16x8 b_nxt[2][3];
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        b_nxt[h][p] = *reinterpret_cast<const bf16x8*>(bl + (p * TP + (2 * gn + h) * 16) * PS + 32 * kn);
                auto prod = [&](int pa, int pb, auto& dst) {  // part pa of the weights times part pb of the activations
#pragma unroll
                    for (int t = 0; t < NQ; ++t)
#pragma unroll
                        for (int h = 0; h < 2; ++h)
                            dst[t][2 * gp + h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_cur[t][pa], b_cur[h][pb],
                                                                                         dst[t][2 * gp + h], 0, 0, 0);
                };
                auto& small = [&]() -> auto& {
                    if constexpr (REV) return acs;
                    else return acc;
                }();
                prod(1, 1, small);  // mm, lh, hl, mh, hm: small terms first
                prod(2, 0, small);
                prod(0, 2, small);
                prod(1, 0, small);
                prod(0, 1, small);
                prod(0, 0, acc);  // hh
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int p = 0; p < 3; ++p) b_cur[h][p] = b_nxt[h][p];
            }
#pragma unroll
            for (int t = 0; t < NQ; ++t)
#pragma unroll
                for (int p = 0; p < 3; ++p) a_cur[t][p] = a_nxt[t][p];
        }
    };
    for (int64_t tile = blockIdx.x; tile * TP < npts; tile += gridDim.x) {
        // input layer: z = p A + b0 (as torch: p @ A then + b0); the wave's units only
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
            f32x4 hn;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = u0 + 4 * lg + i;
                const float z = fmaf(py, sA1[k], px * sA0[k]) + sb0[k];
                if constexpr (FOURIER) {
                    float sn, cs;
                    sincos_fourier(z, &sn, &cs);
                    hn[i] = cs * scale;
                } else {
                    hn[i] = z > 0.f ? z : 0.f;
                }
            }
            put(g, u0, hn);
        });
        __syncthreads();
        float o[G];  // the wave's part of the output contraction
#pragma unroll
        for (int g = 0; g < G; ++g) o[g] = 0.f;
        uint32_t mk[kMaxStreamLayers][MW] = {};  // bit 4 (t G + g) + i: unit 16 (wave NQ + t) + 4 lg + i of HxH layer l's output is on
        // ---------------- forward: h = relu(W h + b) ----------------
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            product(std::false_type{}, reinterpret_cast<const bf16x8*>(w.Ws) + (size_t)(l * 4 + wave) * NKB * NQ * 3 * 64 + lane);
            __syncthreads();  // every wave has read the layer's input: act may be overwritten
            const bool last = l == L - 1;
            const float* bias = w.b + l * H + 4 * lg;
            static_for<NQ * G>([&](auto ic) {
                constexpr int t = decltype(ic)::value / G, g = decltype(ic)::value % G;
                constexpr int word = decltype(ic)::value / 8, sh = 4 * (decltype(ic)::value % 8);
                const int u0 = 16 * (wave * NQ + t);
                const f32x4 bq = *reinterpret_cast<const f32x4*>(bias + u0);
                f32x4 hn;
                uint32_t m = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = acc[t][g][i] + bq[i];
                    const bool on = v > 0.f;
                    hn[i] = on ? v : 0.f;
                    m |= (uint32_t)on << (sh + i);
                }
                if constexpr (FULL) {  // the layer index is runtime: predicated writes keep the patterns in registers
#pragma unroll
                    for (int ll = 0; ll < kMaxStreamLayers; ++ll)
                        if (ll == l) mk[ll][word] = sh == 0 ? m : (mk[ll][word] | m);
                }
                if (!last) {
                    put(g, u0, hn);
                } else {  // output layer: the lane contracts w_out with its units, tile by tile in index order
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[g] = fmaf(sw[u0 + 4 * lg + i], hn[i], o[g]);
                    if constexpr (FULL) {  // e_L = lam w_out .* mask_L starts the reverse sweep
                        const int64_t gi = tile * TP + g * 16 + pn;
                        const float lm = lam ? (gi < npts ? lam[point_addr(gi, cnt, ld)] : 0.f) : 1.f;
                        f32x4 e;
#pragma unroll
                        for (int i = 0; i < 4; ++i) e[i] = ((m >> (sh + i)) & 1) ? lm * sw[u0 + 4 * lg + i] : 0.f;
                        put(g, u0, e);
                    }
                }
            });
            __syncthreads();  // every wave has written the layer's output
        }
        // two shuffles sum the 4 lane groups; the 4 waves' partials go through LDS and are summed in wave order
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float v = o[g];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lg == 0) sF[wave * TP + g * 16 + pn] = v;
        }
        if constexpr (FULL) {
            // ---------------- reverse sweep: e_l = mask_l .* (W_l^T e_{l+1}), down to d = lam df/dh0 ----------------
#pragma unroll 1
            for (int l = L - 1; l >= 0; --l) {
                product(std::true_type{}, reinterpret_cast<const bf16x8*>(w.Wr) + (size_t)(l * 4 + wave) * NKB * NQ * 3 * 64 + lane);
                __syncthreads();  // every wave has read e_{l+1}
                static_for<NQ * G>([&](auto ic) {
                    constexpr int t = decltype(ic)::value / G, g = decltype(ic)::value % G;
                    constexpr int word = decltype(ic)::value / 8, sh = 4 * (decltype(ic)::value % 8);
                    acc[t][g] += acs[t][g];
                    if (l > 0) {  // the units are HxH layer l - 1's outputs: its pattern, by selects
                        uint32_t m = mk[0][word];
#pragma unroll
                        for (int ll = 1; ll < kMaxStreamLayers; ++ll) m = ll == l - 1 ? mk[ll][word] : m;
                        f32x4 e;
#pragma unroll
                        for (int i = 0; i < 4; ++i) e[i] = ((m >> (sh + i)) & 1) ? acc[t][g][i] : 0.f;
                        put(g, 16 * (wave * NQ + t), e);
                    }
                });
                __syncthreads();  // every wave has written e_l (l = 0: act is free for the partials)
            }
            // acc = d: contract with the input layer's derivatives, group by group, the wave's units in index order
            float px = 0.f, py = 0.f, gx = 0.f, gy = 0.f, hxx = 0.f, hxy = 0.f, hyy = 0.f;
            static_for<G * NQ>([&](auto ic) {
                constexpr int g = decltype(ic)::value / NQ, t = decltype(ic)::value % NQ;
                if constexpr (t == 0) {
                    const int64_t gi = tile * TP + g * 16 + pn;
                    px = py = gx = gy = hxx = hxy = hyy = 0.f;
                    if (gi < npts) {
                        const int64_t pi = point_addr(gi, cnt, ld);
                        px = pts[2 * pi];
                        py = pts[2 * pi + 1];
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = 16 * (wave * NQ + t) + 4 * lg + i;
                    const float ax = sA0[k], ay = sA1[k];
                    const float z = fmaf(py, ay, px * ax) + sb0[k];
                    input_contract(ax, ay, z, acc[t][g][i], FOURIER, scale, gx, gy, hxx, hxy, hyy);
                }
                if constexpr (t == NQ - 1) {
                    const float r[5] = {gx, gy, hxx, hxy, hyy};
#pragma unroll
                    for (int c = 0; c < 5; ++c) {
                        float v = r[c];
                        v += __shfl_xor(v, 16);
                        v += __shfl_xor(v, 32);
                        if (lg == 0) sPart[(wave * 5 + c) * TP + g * 16 + pn] = v;
                    }
                }
            });
        }
        __syncthreads();  // the partials are written (the next tile writes sF only after its own layer barriers)
        const int64_t gi = tile * TP + threadIdx.x;
        if (threadIdx.x < TP && gi < npts) {
            const int64_t pi = point_addr(gi, cnt, ld);
            const float* p = sF + threadIdx.x;
            const float f = (((p[0] + p[TP]) + p[2 * TP]) + p[3 * TP]) + w.b_out;
            if constexpr (FULL) {
                float r[5];
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const float* q = sPart + c * TP + threadIdx.x;
                    r[c] = ((q[0] + q[5 * TP]) + q[10 * TP]) + q[15 * TP];
                }
                store_point(out, pi, f, r[0], r[1], r[2], r[3], r[4]);
            } else {
                out.val[pi * out.sv] = f;
            }
        }
        if constexpr (FULL) __syncthreads();  // the partials are read: the next tile's input layer overwrites them
    }
}

template <int H, bool FOURIER, bool FULL>
static int launch_rbs(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                      const float* lam, const MlpOut& out, hipStream_t stream) {
    constexpr size_t lds = rbs_lds_bytes(H);
    static_assert(lds <= 160 * 1024, "mlp_relu_bf16_stream LDS");
    static std::atomic<uint64_t> attr{0};
    NLOT_HIP_CHECK(set_lds_attr_once(attr, (const void*)mlp_relu_bf16_stream<H, FOURIER, FULL>, (int)lds));
    const int grid = persistent_grid(n * P_per, 16 * rbs_groups(H), device_cus());
    hipLaunchKernelGGL((mlp_relu_bf16_stream<H, FOURIER, FULL>), dim3(grid), dim3(256), lds, stream, w, pts, n, n_dev, P_per,
                       ld, lam, out);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

template <int H, bool FOURIER>
static int launch_rbs_in(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                         const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return full ? launch_rbs<H, FOURIER, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                : launch_rbs<H, FOURIER, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
}

template <int H>
static int launch_rbs_width(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                            const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return w.in_kind == NLOT_MLP_IN_FOURIER ? launch_rbs_in<H, true>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream)
                                            : launch_rbs_in<H, false>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
}

int launch_mlp_relu_bf16_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                                const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    if (const char* why = relu_bf16_stream_refusal(w.act, w.H, w.n_hidden)) {  // nlot_mlp_create_ex has checked; a guard
        set_error(why);                                                         // for the images and the widths compiled
        return NLOT_ERR_INVALID;
    }
    if (!w.Ws || !w.Wr) {
        set_error("mlp_relu_bf16_stream: the net was not created with NLOT_MLP_ARITH_SPLIT_BF16_STREAM");
        return NLOT_ERR_INVALID;
    }
    return w.H == 128 ? launch_rbs_width<128>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream)
                      : launch_rbs_width<256>(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
}

}  // namespace nlot
