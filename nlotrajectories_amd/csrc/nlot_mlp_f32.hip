// Learned-SDF MLP, f32 MFMA with the weights resident in LDS: mlp_kernel<H,L,FULL>, H <= 128, 1 or 2 HxH layers.
//
// Mapping (MI355X, wave64, f32-input MFMA v_mfma_f32_32x32x2_f32 = exact k-ordered fp32 FMA chain):
//   * a wave owns 32 points; a 256-thread block owns 128 points per tile and loops over tiles
//     (persistent grid: the weights are staged into LDS once per block);
//   * forward GEMM:  Z^T[hidden j][point i] = W[j][:] . h[:][i]  — A operand = W from LDS
//     (row stride H+1 floats: the 32 rows a ds_read_b32 touches land in 32 distinct banks),
//     B operand = the hidden activations of the point held by the lane;  the input layer h0 is
//     computed on the fly per k-step (1 cos per lane per MFMA k-step, hidden under the MFMA);
//   * the accumulator layout (hidden unit in registers, point in lanes) is exactly the B-operand
//     layout of the next product, so every further hidden layer and the whole reverse sweep
//     (G^T = W^T (lam*w_out .* mask)) chain register-to-register with no LDS transpose;
//   * the gradient / Hessian w.r.t. the 2-D input are contractions over the hidden units of the
//     input layer: per-lane partial sums + one cross-half shuffle.  For a Fourier input layer
//     lam*d2f/dp2 = A diag(g .* (-scale cos z)) A^T (g = df/dh0), for a ReLU input layer it is 0.
#include "nlot_mlp.h"

namespace nlot {

// FULL kernels with one hidden layer run 512-thread blocks (8 waves = 2 per SIMD) sharing one LDS copy of
// the weights, with a per-wave [64][33] staging tile for the reverse sweep (two k-halves at a time).
__host__ __device__ constexpr size_t mlp_lds_floats(int H, int L, bool staged) {
    return (size_t)L * H * (H + 1) + 4 * H + (size_t)L * H + (staged ? (size_t)8 * 64 * 33 : 0);
}
__host__ __device__ constexpr bool mlp_staged(int H, int L) {
    return L == 1 && H % 64 == 0 && mlp_lds_floats(H, L, true) * 4 <= 160 * 1024;
}
__host__ __device__ constexpr int mlp_threads(int H, int L, bool full) { return full && mlp_staged(H, L) ? 512 : 256; }

template <int H, int L, bool FULL>
__global__ __launch_bounds__(mlp_threads(H, L, FULL), (FULL || L > 1) ? 1 : 2) void mlp_kernel(MlpDev w, const float* __restrict__ pts, int64_t cnt_host,
                                                      const int* __restrict__ cnt_dev, int P_per, int64_t ld,
                                                      const float* __restrict__ lam, MlpOut out) {
    constexpr int HP = H + 1;   // padded LDS row
    constexpr int NT = H / 32;  // 32x32 tiles along the hidden dimension
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sW = smem;                                   // [L][H][HP]
    float* sA0 = sW + (size_t)L * H * HP;               // [H]
    float* sA1 = sA0 + H;                               // [H]
    float* sb0 = sA1 + H;                               // [H]
    float* sb = sb0 + H;                                // [L][H]
    float* sw = sb + L * H;                             // [H]
    // FULL kernels whose LDS budget allows: a per-wave [H][33] staging tile for the reverse sweep's
    // operand and for df/dh0 (runtime k-loops instead of fully unrolled register chains: no spills)
    constexpr bool STAGED = FULL && mlp_staged(H, L);
    float* sStage = sw + H;                             // [8 waves][64][33] when STAGED
    constexpr int TP = mlp_threads(H, L, FULL) / 2;     // points per block tile (32 per wave)

    for (int idx = threadIdx.x; idx < L * H * H; idx += blockDim.x) {
        int l = idx / (H * H), rem = idx - l * H * H, j = rem / H, k = rem - j * H;
        sW[(size_t)l * H * HP + j * HP + k] = w.W[idx];
    }
    for (int idx = threadIdx.x; idx < H; idx += blockDim.x) {
        sA0[idx] = w.A[idx];
        sA1[idx] = w.A[H + idx];
        sb0[idx] = w.b0[idx];
        sw[idx] = w.w_out[idx];
    }
    for (int idx = threadIdx.x; idx < L * H; idx += blockDim.x) sb[idx] = w.b[idx];
    __syncthreads();

    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int il = lane & 31, hl = lane >> 5;
    const bool fourier = w.in_kind == NLOT_MLP_IN_FOURIER;
    const float scale = w.scale;

    for (int64_t tile = blockIdx.x; tile * TP < npts; tile += gridDim.x) {
        const int64_t gi = tile * TP + wave * 32 + il;
        const bool valid = gi < npts;
        const int64_t pi = valid ? point_addr(gi, cnt, ld) : 0;
        float px = 0.f, py = 0.f;
        if (valid) {
            px = pts[2 * pi];
            py = pts[2 * pi + 1];
        }
        // ---------------- input layer + first hidden GEMM ----------------
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
#pragma unroll 4
        for (int s = 0; s < H / 2; ++s) {
            const int k = 2 * s + hl;
            const float z = fmaf(py, sA1[k], px * sA0[k]) + sb0[k];
            float h0;
            if (fourier) {
                float sn, cs;
                sincos_fourier(z, &sn, &cs);
                h0 = cs * scale;
            } else {
                h0 = z > 0.f ? z : 0.f;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float a = sW[(t * 32 + il) * HP + k];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, h0, acc[t], 0, 0, 0);
            }
        }
        uint64_t mask[L];
        // bias + ReLU of layer 0
        {
            uint64_t m = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[t][r] + sb[t * 32 + acc_row(r, hl)];
                    const bool on = v > 0.f;
                    acc[t][r] = on ? v : 0.f;
                    m |= (uint64_t)on << (t * 16 + r);
                }
            mask[0] = m;
        }
        // ---------------- further hidden layers (register-chained) ----------------
#pragma unroll
        for (int l = 1; l < L; ++l) {
            const float* Wl = sW + (size_t)l * H * HP;
            f32x16 nacc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) nacc[t] = f32x16{};
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kk = ti * 32 + acc_row(r, hl);
                    const float bv = acc[ti][r];
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const float a = Wl[(t * 32 + il) * HP + kk];
                        nacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, nacc[t], 0, 0, 0);
                    }
                }
            uint64_t m = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = nacc[t][r] + sb[l * H + t * 32 + acc_row(r, hl)];
                    const bool on = v > 0.f;
                    acc[t][r] = on ? v : 0.f;
                    m |= (uint64_t)on << (t * 16 + r);
                }
            mask[l] = m;
        }
        // ---------------- output layer ----------------
        float fpart = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) fpart = fmaf(sw[t * 32 + acc_row(r, hl)], acc[t][r], fpart);
        const float f = fpart + __shfl_xor(fpart, 32) + w.b_out;

        if constexpr (!FULL) {
            if (valid && hl == 0) out.val[pi * out.sv] = f;
            continue;
        } else {
            // ---------------- reverse sweep ----------------
            const float lm = lam ? (valid ? lam[pi] : 0.f) : 1.f;
            float gx = 0.f, gy = 0.f, hxx = 0.f, hxy = 0.f, hyy = 0.f;
            if constexpr (STAGED) {
                float* sE = sStage + wave * (64 * 33);  // [k within the half][point], padded
                const uint64_t m = mask[0];
                f32x16 g[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) g[t] = f32x16{};
                // g = W^T e with e = lam * w_out .* mask, staged 64 rows of k at a time
#pragma unroll
                for (int hh = 0; hh < H / 64; ++hh) {
                    __syncthreads();
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int t = 2 * hh + tt, kl = tt * 32 + acc_row(r, hl);
                            sE[kl * 33 + il] = ((m >> (t * 16 + r)) & 1) ? lm * sw[t * 32 + acc_row(r, hl)] : 0.f;
                        }
                    __syncthreads();
#pragma unroll 4
                    for (int s = 0; s < 32; ++s) {
                        const int kl = 2 * s + hl, k = hh * 64 + kl;
                        const float bv = sE[kl * 33 + il];
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            const float a = sW[k * HP + t * 32 + il];
                            g[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, g[t], 0, 0, 0);
                        }
                    }
                }
                // g = df/dh0 (x lam): contract with the input layer's derivatives, lane = (k, point)
#pragma unroll
                for (int hh = 0; hh < H / 64; ++hh) {
                    __syncthreads();
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) sE[(tt * 32 + acc_row(r, hl)) * 33 + il] = g[2 * hh + tt][r];
                    __syncthreads();
#pragma unroll 2
                    for (int s = 0; s < 32; ++s) {
                        const int kl = 2 * s + hl, k = hh * 64 + kl;
                        const float ax = sA0[k], ay = sA1[k];
                        const float z = fmaf(py, ay, px * ax) + sb0[k];
                        input_contract(ax, ay, z, sE[kl * 33 + il], fourier, scale, gx, gy, hxx, hxy, hyy);
                    }
                }
            } else {
            // e = lam * w_out .* mask_top  (in place, accumulator layout)
            {
                const uint64_t m = mask[L - 1];
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[t][r] = ((m >> (t * 16 + r)) & 1) ? lm * sw[t * 32 + acc_row(r, hl)] : 0.f;
            }
#pragma unroll
            for (int l = L - 1; l >= 0; --l) {
                const float* Wl = sW + (size_t)l * H * HP;
                f32x16 g[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) g[t] = f32x16{};
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int jj = tj * 32 + acc_row(r, hl);
                        const float bv = acc[tj][r];
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            const float a = Wl[jj * HP + t * 32 + il];
                            g[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, g[t], 0, 0, 0);
                        }
                    }
                if (l > 0) {
                    const uint64_t m = mask[l - 1];
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[t][r] = ((m >> (t * 16 + r)) & 1) ? g[t][r] : 0.f;
                } else {
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = g[t];
                }
            }
            // acc = df/dh0 (x lam); contract with the input layer's derivatives
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = t * 32 + acc_row(r, hl);
                    const float ax = sA0[k], ay = sA1[k];
                    const float z = fmaf(py, ay, px * ax) + sb0[k];
                    input_contract(ax, ay, z, acc[t][r], fourier, scale, gx, gy, hxx, hxy, hyy);
                }
            }
            gx += __shfl_xor(gx, 32);
            gy += __shfl_xor(gy, 32);
            hxx += __shfl_xor(hxx, 32);
            hxy += __shfl_xor(hxy, 32);
            hyy += __shfl_xor(hyy, 32);
            if (valid && hl == 0) store_point(out, pi, f, gx, gy, hxx, hxy, hyy);
        }
    }
}

template <int H, int L, bool FULL>
static int launch_t(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                    const float* lam, const MlpOut& out, hipStream_t stream) {
    const size_t lds = sizeof(float) * mlp_lds_floats(H, L, FULL && mlp_staged(H, L));
    static std::atomic<uint64_t> attr_set{0};
    NLOT_HIP_CHECK(set_lds_attr_once(attr_set, (const void*)mlp_kernel<H, L, FULL>, 160 * 1024));
    constexpr int NTH = mlp_threads(H, L, FULL);
    // resident blocks per CU: VGPR-limited (FULL: 1 wave/SIMD) and LDS-limited
    const int64_t cap = (int64_t)device_cus() * ((!FULL && L == 1 && lds <= 80 * 1024) ? 2 : 1);
    const int grid = persistent_grid(n * P_per, NTH / 2, cap);
    hipLaunchKernelGGL((mlp_kernel<H, L, FULL>), dim3(grid), dim3(NTH), lds, stream, w, pts, n, n_dev, P_per, ld, lam, out);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

int launch_mlp_f32(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                   const float* lam, const MlpOut& out, bool full, hipStream_t stream) {
    return dispatch_width<128>(w.H, [&](auto width) {  // H = 256 does not fit in LDS: launch_mlp_strided streams it
        constexpr int H = decltype(width)::value;
        if (w.n_hidden == 1)
            return full ? launch_t<H, 1, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                        : launch_t<H, 1, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
        return full ? launch_t<H, kMaxResidentLayers, true>(w, pts, n, n_dev, P_per, ld, lam, out, stream)
                    : launch_t<H, kMaxResidentLayers, false>(w, pts, n, n_dev, P_per, ld, lam, out, stream);
    });
}

}  // namespace nlot
