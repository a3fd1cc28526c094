// Layer-streaming kernel for nets whose weights do not fit in LDS (the stress config 2-256x4-1: three
// 256x256 HxH layers = 768 KB of fp32; any H in {64, 128, 256} with up to kMaxStreamLayers HxH layers).
// f32-input MFMA v_mfma_f32_16x16x4_f32 (exact fp32 products): a wave owns 16 points (column = point),
// 16-unit tiles in 4 registers per lane (row 4 (lane >> 4) + i), and that accumulator is the B operand of
// the next layer's product with k = 16 T + 4 (lane >> 4) + i (k order permuted consistently on A).
// Weights pass through LDS a quarter layer (a "unit") at a time, software-pipelined: the global loads of
// unit u + 1 are issued into registers before the MFMAs of unit u, so their L2 latency hides under the
// 8192 MFMA cycles per wave of a quarter (H = 256).  A unit is stored with a row stride of H/4 + 4 floats,
// so every ds_read_b32 of an A operand (16 consecutive outputs x 4 k of the lane groups) hits 64 banks:
//   forward  y = W h:     rows j0 .. j0 + H/4 of W, k-major: sW[k][j - j0]
//   reverse  g = W^T e:   columns i0 .. i0 + H/4, as sW[j][i - i0]
// 4 waves (one per SIMD with the whole 512-register file; 64 points per block tile) share each unit: the
// weights cross L2 -> LDS 4 L x 4 B H^2 per 64 points for value + reverse sweep (3 MB at H = 256, L = 3).
#include "nlot_mlp.h"

namespace nlot {

__host__ __device__ constexpr int stream_stride(int H) { return H / 4 + 4; }
__host__ __device__ constexpr size_t stream_lds_floats(int H) {
    return (size_t)H * stream_stride(H) + (size_t)4 * H + (size_t)kMaxStreamLayers * H;
}

template <int H, bool FULL>
__global__ __launch_bounds__(256, 1) void mlp_stream(MlpDev w, const float* __restrict__ pts, int64_t cnt_host,
                                                     const int* __restrict__ cnt_dev, int P_per, int64_t ld,
                                                     const float* __restrict__ lam, MlpOut out) {
    constexpr int Q = H / 4, NQ = Q / 16, NT = H / 16, RS = stream_stride(H);
    constexpr int PF = H * H / 4096;  // float4 of a unit per thread (Q x H floats over 256 threads)
    static_assert(PF >= 1 && NQ >= 1, "H >= 64");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sW = smem;                  // the staged unit [H][RS]
    float* sA0 = sW + (size_t)H * RS;  // [H]
    float* sA1 = sA0 + H;              // [H]
    float* sb0 = sA1 + H;              // [H]
    float* sw = sb0 + H;               // [H]
    float* sbl = sw + H;               // [kMaxStreamLayers][H]: HxH layer biases
    const int L = w.n_hidden;
    for (int idx = threadIdx.x; idx < H; idx += 256) {
        sA0[idx] = w.A[idx];
        sA1[idx] = w.A[H + idx];
        sb0[idx] = w.b0[idx];
        sw[idx] = w.w_out[idx];
    }
    for (int idx = threadIdx.x; idx < L * H; idx += 256) sbl[idx] = w.b[idx];
    __syncthreads();  // the input layer is read by every wave before the first staging barrier
    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pn = lane & 15, lg = lane >> 4;  // point of the lane, lane group (k / row offset 4 lg)
    const bool fourier = w.in_kind == NLOT_MLP_IN_FOURIER;
    const float scale = w.scale;
    // units of one block tile: forward (layer l, quarter q) = 4 l + q; FULL adds the reverse sweep,
    // 4 L + 4 (L - 1 - l) + q
    const int U = FULL ? 8 * L : 4 * L;
    float4 pf[PF];
    // Forward units: a wave covers 16 rows x 16 k per float4 pass (lane = jj + 16 kk: row 16 jb + jj, k = 16 kq +
    // 4 kk .. + 3), so each transposed ds_write_b32 hits bank 16 kk + jj + const: 64 distinct banks.
    // Reverse units: 16-byte row pieces, stored as they are.
    // Per-thread parts of the unit addresses; the rest are compile-time offsets per r (a runtime-indexed
    // address set would be hoisted out of the tile loop into registers)
    constexpr int KQ = H / 16, QC = Q / 4;
    const int jj = threadIdx.x & 15, kk = (threadIdx.x >> 4) & 3, w4 = threadIdx.x >> 6;
    const int fwd_g = jj * H + 16 * w4 + 4 * kk, fwd_s = (16 * w4 + 4 * kk) * RS + jj;
    const int rev_g = (threadIdx.x / QC) * H + 4 * (threadIdx.x % QC), rev_s = (threadIdx.x / QC) * RS + 4 * (threadIdx.x % QC);
    auto fetch = [&](int u) {
        const bool fwd = u < 4 * L;
        const int l = fwd ? (u >> 2) : L - 1 - ((u - 4 * L) >> 2), q = u & 3;
        const float* src = w.W + (size_t)l * H * H + (fwd ? q * Q * H + fwd_g : q * Q + rev_g);
        if (fwd) {
#pragma unroll
            for (int r = 0; r < PF; ++r)
                pf[r] = *reinterpret_cast<const float4*>(src + 16 * ((4 * r) / KQ) * H + 16 * ((4 * r) % KQ));
        } else {
#pragma unroll
            for (int r = 0; r < PF; ++r) pf[r] = *reinterpret_cast<const float4*>(src + (256 * r / QC) * H);
        }
    };
    auto commit = [&](int u) {
        if (u < 4 * L) {
#pragma unroll
            for (int r = 0; r < PF; ++r) {
                float* d = sW + fwd_s + 16 * ((4 * r) % KQ) * RS + 16 * ((4 * r) / KQ);
                d[0] = pf[r].x;
                d[RS] = pf[r].y;
                d[2 * RS] = pf[r].z;
                d[3 * RS] = pf[r].w;
            }
        } else {
#pragma unroll
            for (int r = 0; r < PF; ++r) *reinterpret_cast<float4*>(sW + rev_s + (256 * r / QC) * RS) = pf[r];
        }
    };
    // acc_q[t] += W_unit(16 t + pn, k) B(k), k over all H (both sweeps read the unit as sW[k][16 t + pn]); the A
    // operands of group (T, i) are loaded one group ahead of its MFMAs (one wave per SIMD: nothing else hides the
    // LDS latency)
    auto unit_mfma = [&](f32x4* accq, const f32x4* bsrc) {
        float a_cur[NQ];
#pragma unroll
        for (int t = 0; t < NQ; ++t) a_cur[t] = sW[(4 * lg) * RS + 16 * t + pn];
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float a_nxt[NQ];
                if (4 * T + i + 1 < 4 * NT) {
                    const int kn = 16 * ((4 * T + i + 1) >> 2) + 4 * lg + ((i + 1) & 3);
#pragma unroll
                    for (int t = 0; t < NQ; ++t) a_nxt[t] = sW[kn * RS + 16 * t + pn];
                }
                const float bv = bsrc[T][i];
#pragma unroll
                for (int t = 0; t < NQ; ++t) accq[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[t], bv, accq[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < NQ; ++t) a_cur[t] = a_nxt[t];
                asm volatile("" ::: "memory");  // bound the LDS loads the scheduler hoists (register file)
            }
    };
    fetch(0);
    constexpr int TP = 64;  // points per block tile (4 waves x 16, one per SIMD with the whole register file)
    for (int64_t tile = blockIdx.x; tile * TP < npts; tile += gridDim.x) {
        const int64_t gi = tile * TP + wave * 16 + pn;
        const bool valid = gi < npts;
        const int64_t pi = valid ? point_addr(gi, cnt, ld) : 0;
        float px = 0.f, py = 0.f;
        if (valid) {
            px = pts[2 * pi];
            py = pts[2 * pi + 1];
        }
        f32x4 acc[NT];
        uint32_t mask[kMaxStreamLayers][NT / 8 > 0 ? NT / 8 : 1];  // ReLU bit 4 (t & 7) + i of word t >> 3
        // input layer h0 (unit k = 16 T + 4 lg + i of the lane's point), computed once into the B registers
#pragma unroll
        for (int T = 0; T < NT; ++T)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 16 * T + 4 * lg + i;
                const float z = fmaf(py, sA1[k], px * sA0[k]) + sb0[k];
                if (fourier) {
                    float sn, cs;
                    sincos_fourier(z, &sn, &cs);
                    acc[T][i] = cs * scale;
                } else {
                    acc[T][i] = z > 0.f ? z : 0.f;
                }
            }
        // ---------------- forward through the HxH layers ----------------
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            f32x4 nacc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) nacc[t] = f32x4{};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int u = 4 * l + q;
                __syncthreads();
                commit(u);
                __syncthreads();
                fetch(u + 1 < U ? u + 1 : 0);
                unit_mfma(nacc + q * NQ, acc);
            }
            const float* bl = sbl + l * H;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                uint32_t m = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = nacc[t][i] + bl[16 * t + 4 * lg + i];
                    const bool on = v > 0.f;
                    acc[t][i] = on ? v : 0.f;
                    m |= (uint32_t)on << (4 * (t & 7) + i);
                }
                if constexpr (FULL) {  // layer index is runtime: predicated writes keep the masks in registers
#pragma unroll
                    for (int ll = 0; ll < kMaxStreamLayers; ++ll)
                        if (ll == l) mask[ll][t >> 3] = (t & 7) == 0 ? m : (mask[ll][t >> 3] | m);
                }
            }
        }
        auto lsum = [](float v) {  // sum over the 4 lane groups (the 4 k / row offsets of a point)
            v += __shfl_xor(v, 16);
            return v + __shfl_xor(v, 32);
        };
        float fpart = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) fpart = fmaf(sw[16 * t + 4 * lg + i], acc[t][i], fpart);
        const float f = lsum(fpart) + w.b_out;
        if constexpr (!FULL) {
            if (valid && lg == 0) out.val[pi * out.sv] = f;
            continue;
        } else {
            // ---------------- reverse sweep: e = lam w_out .* mask_top; g = W_l^T e; e = g .* mask_{l-1} ----
            const float lm = lam ? (valid ? lam[pi] : 0.f) : 1.f;
            auto mask_of = [&](int l, int word) {  // mask[l][word] for a runtime l, by selects
                uint32_t m = mask[0][word];
#pragma unroll
                for (int ll = 1; ll < kMaxStreamLayers; ++ll) m = ll == l ? mask[ll][word] : m;
                return m;
            };
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[t][i] = ((mask_of(L - 1, t >> 3) >> (4 * (t & 7) + i)) & 1) ? lm * sw[16 * t + 4 * lg + i] : 0.f;
#pragma unroll 1
            for (int l = L - 1; l >= 0; --l) {
                f32x4 g[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) g[t] = f32x4{};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int u = 4 * L + 4 * (L - 1 - l) + q;
                    __syncthreads();
                    commit(u);
                    __syncthreads();
                    fetch(u + 1 < U ? u + 1 : 0);
                    unit_mfma(g + q * NQ, acc);
                }
                if (l > 0) {
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[t][i] = ((mask_of(l - 1, t >> 3) >> (4 * (t & 7) + i)) & 1) ? g[t][i] : 0.f;
                } else {
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = g[t];
                }
            }
            // acc = lam df/dh0: contract with the input layer's derivatives (lane = (k, point))
            float gx = 0.f, gy = 0.f, hxx = 0.f, hxy = 0.f, hyy = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = 16 * t + 4 * lg + i;
                    const float ax = sA0[k], ay = sA1[k];
                    const float z = fmaf(py, ay, px * ax) + sb0[k];
                    input_contract(ax, ay, z, acc[t][i], fourier, scale, gx, gy, hxx, hxy, hyy);
                }
            gx = lsum(gx);
            gy = lsum(gy);
            hxx = lsum(hxx);
            hxy = lsum(hxy);
            hyy = lsum(hyy);
            if (valid && lg == 0) store_point(out, pi, f, gx, gy, hxx, hxy, hyy);
        }
    }
}

template <int H, bool FULL>
static int launch_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                    const float* lam, const MlpOut& out, hipStream_t stream) {
    const size_t lds = sizeof(float) * stream_lds_floats(H);
    static std::atomic<uint64_t> attr{0};
    NLOT_HIP_CHECK(set_lds_attr_once(attr, (const void*)mlp_stream<H, FULL>, (int)lds));
    const int grid = persistent_grid(n * P_per, 64, device_cus());
    hipLaunchKernelGGL((mlp_stream<H, FULL>), dim3(grid), dim3(256), lds, stream, w, pts, n, n_dev, P_per, ld, lam, out);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

int launch_mlp_stream(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                      const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return dispatch_width(w.H, [&](auto width) {
        constexpr int H = decltype(width)::value;
        return full ? launch_stream<H, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                    : launch_stream<H, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
    });
}

}  // namespace nlot
