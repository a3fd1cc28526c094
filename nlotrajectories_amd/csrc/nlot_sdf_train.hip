// Training of the learned SDF (the ReLU MLP 2-128-128-1 of every shipped config) in one persistent kernel:
// k_sdf_train runs consecutive Adam steps of the trainer's loss (MSE + surface + eikonal) with the net resident in
// one CU, k_sdf_batch_loss is the forward-only validation loss.  include/nlot.h (ABI v20), DESIGN.md §14.
//
// k_sdf_train<EIK>: one 512-thread workgroup (8 waves, 2 per SIMD) per network, no synchronisation between
// workgroups.  Per step, 256 rows, four barriers:
//   rows     wave w loads rows 32 w .. 32 w + 31 of the batch (lane = row, both lane halves), counts its band rows
//   A        per wave, register-chained as in nlot_mlp_f32.hip (accumulator layout = hidden unit in registers, row in
//            lanes = B-operand layout of the next product, W2 the A operand read from LDS straight or transposed):
//              z2 = W2 a1 + b2 (a1 recomputed per k-step from x, y), a2, D2, f, df
//              u = W2^T (D2 o w3), r1 = D1 o u, g = W1^T r1, q                     [g, q: EIK]
//              s2 = W2 t1, t1 = D1 o (W1 q) recomputed per k-step                   [EIK]
//            the sums over the wave's 32 rows that the gradients of W1, b1, w3 need are reduce-scatters over the
//            lanes (62 shuffles for 64 values), written as per-wave partials; df, q and the D2 bit mask go to LDS
//   B1       grad W2 = [df r2 ; r2]^T [a1 ; t1], depth 512 (256 without EIK): wave w owns the 32x32 tiles
//            (w / 2, 2 (w % 2)) and (w / 2, 2 (w % 2) + 1) of W2.  Operands are rebuilt per k-step from the row
//            scalars, the bit mask, w3, W1, b1.  The wave then applies Adam to its tiles from its accumulators and
//            writes them back into LDS; the tiles' moments are read from and written to the state block (L2) each
//            step: held in registers they cost 64 VGPRs for the whole launch and the compiler spilled them
//            (DESIGN.md §14).  Waves with w % 2 == 0 also sum b2's gradient.
//   B2       the 641 small parameters: per-wave partials summed in wave order, Adam, new values into LDS
// Every sum has a fixed order that depends on the batch alone, so a network's result is bitwise the same however its
// steps are spread over launches and whichever other networks share the call.
#include <cmath>

#include "nlot_mlp.h"

namespace nlot {
namespace {

constexpr int H = 128, HP = H + 1, NT = H / 32, BATCH = 256, NTHREADS = 512, NWAVES = NTHREADS / 64;
constexpr int N_PARAMS = 2 * H + H + H * H + H + H + 1;  // 17025, torch parameters() order
constexpr int OFF_W2 = 3 * H;                            // W1 [H][2], b1 [H] come first
// the 641 parameters other than W2, packed: W1 at 0, b1 at 2H, b2 at 3H, w3 at 4H, b3 at 5H
constexpr int N_SMALL = 5 * H + 1, S_B1 = 2 * H, S_B2 = 3 * H, S_W3 = 4 * H, S_B3 = 5 * H, SMALL_PAD = 5 * H + 4;
__host__ __device__ constexpr int small_to_param(int c) { return c < OFF_W2 ? c : c + H * H; }

// LDS (floats).  The small parameters come first: every read of them has a constant offset from a lane-dependent
// base, which fits the 16-bit offset field of ds_read only below 64 KB (past it, each offset costs an address register)
constexpr int L_P = 0;                              // small parameters, then their m, v and b2's gradient
constexpr int L_M = L_P + SMALL_PAD, L_V = L_M + SMALL_PAD, L_G = L_V + SMALL_PAD;
constexpr int L_W = L_G + SMALL_PAD;                // W2 [H][HP]
constexpr int L_LOSS = L_W + H * HP;                // k_sdf_batch_loss ends here: [NWAVES][2] sums, [NWAVES] band rows
constexpr int L_PART = L_LOSS;                      // [NWAVES][4][H]: per-wave sums for W1[:,0], W1[:,1], b1, w3
constexpr int L_ROW = L_PART + NWAVES * 4 * H;      // [BATCH][8]: x, y, df, qx, qy
constexpr int L_MASK = L_ROW + BATCH * 8;           // [BATCH][NT] words: bit i of word t = D2 of hidden unit 32 t + i
constexpr int L_RED = L_MASK + BATCH * NT;          // [NWAVES][4]: sum e^2, sum_band f^2, sum (|g|-1)^2, sum df
constexpr int L_CNT = L_RED + NWAVES * 4;           // [NWAVES] band rows
constexpr int L_TRAIN = L_CNT + NWAVES;
constexpr size_t kTrainLds = sizeof(float) * L_TRAIN, kLossLds = sizeof(float) * (L_LOSS + 3 * NWAVES);
static_assert(kTrainLds <= 160 * 1024, "LDS");

struct TrainK {  // NlotSdfTrainOptions as the kernels take it
    double lr, beta1, beta2;
    float adam_eps, ws, eps_s, we;
};

// pre-activation of input-layer unit k: one expression everywhere, so that D1 is the same bit in every product
__device__ __forceinline__ float z_in(const float* sP, int k, float x, float y) {
    return fmaf(y, sP[2 * k + 1], fmaf(x, sP[2 * k], sP[S_B1 + k]));
}

__device__ __forceinline__ void stage_params(float* smem, const float* __restrict__ par) {
    for (int i = threadIdx.x; i < H * H; i += NTHREADS) smem[L_W + (i >> 7) * HP + (i & (H - 1))] = par[OFF_W2 + i];
    for (int c = threadIdx.x; c < N_SMALL; c += NTHREADS) smem[L_P + c] = par[small_to_param(c)];
}

// z2 = W2 a1 + b2 for the lane's row (x, y): acc = a2 = relu(z2), m = D2 (bit 16 t + r = register r of tile t),
// returns f = w3 . a2 + b3
__device__ __forceinline__ float forward(const float* smem, float x, float y, int il, int hl, f32x16 (&acc)[NT],
                                         uint64_t& m) {
    const float* sW = smem + L_W;
    const float* sP = smem + L_P;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
#pragma unroll 4
    for (int s = 0; s < H / 2; ++s) {
        const int k = 2 * s + hl;
        const float z = z_in(sP, k, x, y);
        const float a1 = z > 0.f ? z : 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(sW[(t * 32 + il) * HP + k], a1, acc[t], 0, 0, 0);
    }
    m = 0;
    float fp = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = t * 32 + acc_row(r, hl);
            const float v = acc[t][r] + sP[S_B2 + j];
            const bool on = v > 0.f;
            acc[t][r] = on ? v : 0.f;
            m |= (uint64_t)on << (t * 16 + r);
            fp = fmaf(sP[S_W3 + j], acc[t][r], fp);
        }
        __builtin_amdgcn_sched_barrier(0);  // one tile's LDS reads at a time
    }
    // keep D2 as these two registers: seen through, the 64 comparisons above stay live as 64 lane masks instead
    uint32_t mlo = (uint32_t)m, mhi = (uint32_t)(m >> 32);
    asm volatile("" : "+v"(mlo), "+v"(mhi));
    m = ((uint64_t)mhi << 32) | mlo;
    return fp + __shfl_xor(fp, 32) + sP[S_B3];
}

// one reduce-scatter step over lane bit HALF / 2: values i and i + HALF fold into i (static register indices)
template <int HALF>
__device__ __forceinline__ void fold(float (&a)[32], int il) {
    const bool up = il & (HALF / 2);
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const float keep = up ? a[i + HALF] : a[i], send = up ? a[i] : a[i + HALF];
        a[i] = keep + __shfl_xor(send, HALF / 2);
    }
    if constexpr (HALF > 2) fold<HALF / 2>(a, il);
}

// sum over the 32 lanes of a half of the 64 values val(16 t + r) (unit 32 t + acc_row(r, hl)): a reduce-scatter, after
// which lane il holds the sums of values 2 il and 2 il + 1; they go to dst[unit] (+= when ADD)
template <bool ADD, class F>
__device__ __forceinline__ void row_sums(F&& val, int il, int hl, float* dst) {
    float a[32];
    {
        const bool up = il & 16;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const float lo = val(i), hi = val(i + 32);
            a[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, 16);
        }
    }
    fold<16>(a, il);
    // lane bit 4 chose between values i and i + 32, bit 3 between i and i + 16, ..., bit 0 between i and i + 2
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = 2 * il + i;
        const int unit = (e >> 4) * 32 + acc_row(e & 15, hl);
        if (ADD)
            dst[unit] += a[i];
        else
            dst[unit] = a[i];
    }
}

__device__ __forceinline__ float wave_row_sum(float v) {  // over the 32 lanes of a half, the same in every lane
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ inline double ipow(double b, uint32_t t) {  // b^t by squaring: a function of t alone
    double r = 1.0;
    for (; t; t >>= 1, b *= b)
        if (t & 1) r *= b;
    return r;
}

struct AdamStep {  // torch.optim.Adam's scalars of step t, computed in fp64 as there
    float w1, b2, w2, step, bc2s, eps;
};
__device__ __forceinline__ AdamStep adam_step(const TrainK& k, uint32_t t) {
    AdamStep a;
    a.w1 = (float)(1.0 - k.beta1);
    a.b2 = (float)k.beta2;
    a.w2 = (float)(1.0 - k.beta2);
    a.step = (float)(k.lr / (1.0 - ipow(k.beta1, t)));
    a.bc2s = (float)sqrt(1.0 - ipow(k.beta2, t));
    a.eps = k.adam_eps;
    return a;
}
// m <- lerp(m, g, 1 - beta1), v <- beta2 v + (1 - beta2) g g, returns p - step m / (sqrt(v) / bc2s + eps)
__device__ __forceinline__ float adam(float p, float g, float& m, float& v, const AdamStep& a) {
    m = fmaf(g - m, a.w1, m);
    v = fmaf(a.w2 * g, g, v * a.b2);
    return p - a.step * (m / (sqrtf(v) / a.bc2s + a.eps));
}

template <bool EIK>
__global__ __launch_bounds__(NTHREADS, 1) void k_sdf_train(TrainK K, float* __restrict__ state,
                                                          const float* __restrict__ pts,
                                                          const float* __restrict__ target,
                                                          const int32_t* __restrict__ order, int64_t n,
                                                          int64_t first_row, int64_t n_rows, int n_steps,
                                                          float* __restrict__ step_loss, float* __restrict__ grad_last) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sW = smem + L_W;
    float* sP = smem + L_P;
    float* sG = smem + L_G;
    float* sRow = smem + L_ROW;
    uint32_t* sMask = (uint32_t*)(smem + L_MASK);
    float* sRed = smem + L_RED;
    int* sCnt = (int*)(smem + L_CNT);

    const int net = blockIdx.x;
    float* par = state + (size_t)net * (3 * N_PARAMS + 1);
    float* gm = par + N_PARAMS;
    float* gv = gm + N_PARAMS;
    uint32_t* gt = (uint32_t*)(gv + N_PARAMS);
    pts += (size_t)net * n * 2;
    target += (size_t)net * n;
    order += (size_t)net * n_rows;
    step_loss += (size_t)net * n_steps;
    if (grad_last) grad_last += (size_t)net * N_PARAMS;

    const int wave = threadIdx.x >> 6;
    // this wave's W2 tiles: rows 32 jt + acc_row(r, hl), columns 32 (kt0 + c) + il
    const int jt = wave >> 1, kt0 = 2 * (wave & 1);

    stage_params(smem, par);
    for (int c = threadIdx.x; c < N_SMALL; c += NTHREADS) {
        smem[L_M + c] = gm[small_to_param(c)];
        smem[L_V + c] = gv[small_to_param(c)];
    }
    const uint32_t t0 = *gt;
    __syncthreads();

    const float eps_s = K.eps_s, ws = K.ws, we = K.we;
    for (int step = 0; step < n_steps; ++step) {
        // the lane index is made opaque once per step: otherwise the hundred-odd LDS and global addresses derived
        // from it are hoisted out of the step loop, where they do not fit the register file (scratch)
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));
        const int il = lane & 31, hl = lane >> 5;
        // ---------------- rows ----------------
        const int64_t base = first_row + (int64_t)step * BATCH;
        const int nb = (int)(n_rows - base < BATCH ? n_rows - base : BATCH);
        const int row = wave * 32 + il;
        const bool valid = row < nb;
        float x = 0.f, y = 0.f, tgt = 0.f;
        if (valid) {
            int64_t idx = order[base + row];
            idx = idx < 0 ? 0 : (idx >= n ? n - 1 : idx);
            x = pts[2 * idx];
            y = pts[2 * idx + 1];
            tgt = target[idx];
        }
        const bool band = valid && ws > 0.f && fabsf(tgt) < eps_s;
        const uint64_t bb = __ballot(band && hl == 0);
        if (lane == 0) sCnt[wave] = __popcll(bb);
        __syncthreads();
        int ns = 0;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) ns += sCnt[w];

        // ---------------- A: forward, input gradient, per-wave sums ----------------
        float* part = smem + L_PART + wave * 4 * H;
        float df, qx = 0.f, qy = 0.f;
        uint64_t m2;
        {
            f32x16 acc[NT];
            const float f = forward(smem, x, y, il, hl, acc, m2);
            const float e = f - tgt;
            df = valid ? e * (2.f / (float)nb) + (band ? ws * 2.f * f / (float)ns : 0.f) : 0.f;
            row_sums<false>([&](int e) { return df * acc[e >> 4][e & 15]; }, il, hl, part + 3 * H);  // sum df a2
            const float s1 = wave_row_sum(valid ? e * e : 0.f), s2 = wave_row_sum(band ? f * f : 0.f),
                        s4 = wave_row_sum(df);
            if (lane == 0) {
                sRed[wave * 4 + 0] = s1;
                sRed[wave * 4 + 1] = s2;
                sRed[wave * 4 + 3] = s4;
            }
        }
        {
            // u = W2^T r2, r2 = D2 o w3, then r1 = D1 o u
            f32x16 u[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) u[t] = f32x16{};
#pragma unroll 4
            for (int e = 0; e < NT * 16; ++e) {  // a runtime loop: the operands come from LDS and the bit mask
                const int j = (e >> 4) * 32 + acc_row(e & 15, hl);
                const float r2 = ((m2 >> e) & 1) ? sP[S_W3 + j] : 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    u[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(sW[j * HP + t * 32 + il], r2, u[t], 0, 0, 0);
            }
            float gx = 0.f, gy = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = t * 32 + acc_row(r, hl);
                    const float r1 = z_in(sP, k, x, y) > 0.f ? u[t][r] : 0.f;
                    u[t][r] = r1;
                    gx = fmaf(sP[2 * k], r1, gx);
                    gy = fmaf(sP[2 * k + 1], r1, gy);
                }
                __builtin_amdgcn_sched_barrier(0);  // one tile's LDS reads and conditions at a time
            }
            float s3 = 0.f;
            {  // without EIK g only feeds we * s3 = 0; the chain stays: the variant compiled without it spills
                gx += __shfl_xor(gx, 32);
                gy += __shfl_xor(gy, 32);
                const float gn = sqrtf(gx * gx + gy * gy);
                if (EIK && valid && gn > 0.f) {
                    const float c = we * 2.f * (gn - 1.f) / (gn * (float)nb);
                    qx = c * gx;
                    qy = c * gy;
                }
                s3 = wave_row_sum(valid ? (gn - 1.f) * (gn - 1.f) : 0.f);
            }
            if (lane == 0) sRed[wave * 4 + 2] = s3;
            // grad W1[k][:] = sum_n r1 (df x + q), grad b1[k] = sum_n r1 df
            const float cx = fmaf(df, x, qx), cy = fmaf(df, y, qy);
            row_sums<false>([&](int e) { return cx * u[e >> 4][e & 15]; }, il, hl, part);
            __builtin_amdgcn_sched_barrier(0);
            row_sums<false>([&](int e) { return cy * u[e >> 4][e & 15]; }, il, hl, part + H);
            __builtin_amdgcn_sched_barrier(0);
            row_sums<false>([&](int e) { return df * u[e >> 4][e & 15]; }, il, hl, part + 2 * H);
        }
        if (EIK) {
            // s2 = W2 t1, then grad w3 += sum_n D2 o s2
            f32x16 s2[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) s2[t] = f32x16{};
#pragma unroll 4
            for (int s = 0; s < H / 2; ++s) {
                const int k = 2 * s + hl;
                const float t1 = z_in(sP, k, x, y) > 0.f ? fmaf(sP[2 * k + 1], qy, sP[2 * k] * qx) : 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    s2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(sW[(t * 32 + il) * HP + k], t1, s2[t], 0, 0, 0);
            }
            row_sums<true>([&](int e) { return ((m2 >> e) & 1) ? s2[e >> 4][e & 15] : 0.f; }, il, hl, part + 3 * H);
        }
        // the row's scalars and its D2 bits for B1
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            uint32_t wd = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) wd |= (uint32_t)((m2 >> (t * 16 + r)) & 1) << acc_row(r, hl);
            wd |= __shfl_xor(wd, 32);
            if (hl == 0) sMask[row * NT + t] = wd;
        }
        if (hl == 0) {
            float* rr = sRow + row * 8;
            rr[0] = x;
            rr[1] = y;
            rr[2] = df;
            rr[3] = qx;
            rr[4] = qy;
        }
        __syncthreads();

        // ---------------- B1: grad W2 over the whole batch, Adam on this wave's tiles ----------------
        const AdamStep as = adam_step(K, t0 + (uint32_t)step + 1u);
        const bool last = grad_last && step == n_steps - 1;
        {
            f32x16 gW[2] = {f32x16{}, f32x16{}};
            const float w3j = sP[S_W3 + jt * 32 + il];
            float w0[2], w1[2], bk[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int k = (kt0 + c) * 32 + il;
                w0[c] = sP[2 * k];
                w1[c] = sP[2 * k + 1];
                bk[c] = sP[S_B1 + k];
            }
            float gb2 = 0.f;
#pragma unroll 2
            for (int s = 0; s < BATCH / 2; ++s) {
                const int nn = 2 * s + hl;
                const f32x4 ra = *(const f32x4*)(sRow + nn * 8);
                const float rqy = sRow[nn * 8 + 4];
                const float r2 = ((sMask[nn * NT + jt] >> il) & 1) ? w3j : 0.f;
                const float adf = ra[2] * r2;
                gb2 += adf;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float z = fmaf(ra[1], w1[c], fmaf(ra[0], w0[c], bk[c]));  // z_in
                    const float a1 = z > 0.f ? z : 0.f;
                    gW[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(adf, a1, gW[c], 0, 0, 0);
                    if (EIK) {
                        const float t1 = z > 0.f ? fmaf(w1[c], rqy, w0[c] * ra[3]) : 0.f;
                        gW[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(r2, t1, gW[c], 0, 0, 0);
                    }
                }
            }
            gb2 += __shfl_xor(gb2, 32);
            if (kt0 == 0 && hl == 0) sG[S_B2 + jt * 32 + il] = gb2;
            // element (c, r) of the tiles sits at a constant offset from the lane's first one
            const int i0 = OFF_W2 + (jt * 32 + 4 * hl) * H + kt0 * 32 + il;
            float* wl = sW + (jt * 32 + 4 * hl) * HP + kt0 * 32 + il;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ro = (r & 3) + 8 * (r >> 2);  // acc_row(r, hl) - 4 hl
                    const int i = i0 + ro * H + c * 32;
                    float mm = gm[i], vv = gv[i];
                    wl[ro * HP + c * 32] = adam(wl[ro * HP + c * 32], gW[c][r], mm, vv, as);
                    gm[i] = mm;
                    gv[i] = vv;
                    if (last) grad_last[i] = gW[c][r];
                }
        }
        __syncthreads();

        // ---------------- B2: the small parameters, the loss ----------------
        for (int c = threadIdx.x; c < N_SMALL; c += NTHREADS) {
            float g;
            if (c >= S_B2 && c < S_W3) {
                g = sG[c];
            } else {
                // W1[k][d] -> partial d, b1 -> 2, w3 -> 3, b3 -> the waves' sums of df
                const float* src = c < S_B1   ? smem + L_PART + (c & 1) * H + (c >> 1)
                                   : c < S_B2 ? smem + L_PART + 2 * H + (c - S_B1)
                                   : c < S_B3 ? smem + L_PART + 3 * H + (c - S_W3)
                                              : sRed + 3;
                const int stride = c < S_B3 ? 4 * H : 4;
                g = 0.f;
#pragma unroll
                for (int w = 0; w < NWAVES; ++w) g += src[w * stride];
            }
            if (last) grad_last[small_to_param(c)] = g;
            smem[L_P + c] = adam(smem[L_P + c], g, smem[L_M + c], smem[L_V + c], as);
        }
        if (threadIdx.x == NTHREADS - 1) {
            float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
            for (int w = 0; w < NWAVES; ++w) {
                s1 += sRed[w * 4];
                s2 += sRed[w * 4 + 1];
                s3 += sRed[w * 4 + 2];
            }
            float loss = s1 / (float)nb;
            if (ns > 0) loss += ws * (s2 / (float)ns);
            loss += we * (s3 / (float)nb);
            step_loss[step] = loss;
        }
        __syncthreads();
    }

    // ---------------- state back to global memory ----------------
    for (int i = threadIdx.x; i < H * H; i += NTHREADS) par[OFF_W2 + i] = sW[(i >> 7) * HP + (i & (H - 1))];
    for (int c = threadIdx.x; c < N_SMALL; c += NTHREADS) {
        par[small_to_param(c)] = smem[L_P + c];
        gm[small_to_param(c)] = smem[L_M + c];
        gv[small_to_param(c)] = smem[L_V + c];
    }
    if (threadIdx.x == 0) *gt = t0 + (uint32_t)n_steps;
}

// mse + ws * surface of rows 256 b .. of network blockIdx.y, forward only (the trainer's validation loss per batch)
__global__ __launch_bounds__(NTHREADS, 1) void k_sdf_batch_loss(TrainK K, const float* __restrict__ state,
                                                               const float* __restrict__ pts,
                                                               const float* __restrict__ target, int64_t n,
                                                               float* __restrict__ batch_loss) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sRed = smem + L_LOSS;
    int* sCnt = (int*)(sRed + 2 * NWAVES);
    const int net = blockIdx.y;
    stage_params(smem, state + (size_t)net * (3 * N_PARAMS + 1));
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, il = lane & 31, hl = lane >> 5;
    const int64_t base = (int64_t)blockIdx.x * BATCH;
    const int nb = (int)(n - base < BATCH ? n - base : BATCH);
    const int row = wave * 32 + il;
    const bool valid = row < nb;
    float x = 0.f, y = 0.f, tgt = 0.f;
    if (valid) {
        const int64_t idx = (int64_t)net * n + base + row;
        x = pts[2 * idx];
        y = pts[2 * idx + 1];
        tgt = target[idx];
    }
    const bool band = valid && K.ws > 0.f && fabsf(tgt) < K.eps_s;
    f32x16 acc[NT];
    uint64_t m2;
    const float f = forward(smem, x, y, il, hl, acc, m2), e = f - tgt;
    const float s1 = wave_row_sum(valid ? e * e : 0.f), s2 = wave_row_sum(band ? f * f : 0.f);
    const uint64_t bb = __ballot(band && hl == 0);
    if (lane == 0) {
        sRed[wave * 2] = s1;
        sRed[wave * 2 + 1] = s2;
        sCnt[wave] = __popcll(bb);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t1 = 0.f, t2 = 0.f;
        int ns = 0;
        for (int w = 0; w < NWAVES; ++w) {
            t1 += sRed[w * 2];
            t2 += sRed[w * 2 + 1];
            ns += sCnt[w];
        }
        float loss = t1 / (float)nb;
        if (ns > 0) loss += K.ws * (t2 / (float)ns);
        batch_loss[(size_t)net * gridDim.x + blockIdx.x] = loss;
    }
}

// the checks the two entry points share; false after set_error
bool check_options(const NlotSdfTrainOptions* opt, const char* who) {
    const std::string w(who);
    if (opt->hidden != H || opt->n_hidden != 1 || opt->batch != BATCH) {
        set_error(w + ": unsupported shape (hidden must be 128, n_hidden 1, batch 256: the ReLU net 2-128-128-1)");
        return false;
    }
    if (!(opt->lr > 0.0) || !std::isfinite(opt->lr) || !(opt->beta1 >= 0.0 && opt->beta1 < 1.0) ||
        !(opt->beta2 >= 0.0 && opt->beta2 < 1.0) || !(opt->adam_eps >= 0.0) || !std::isfinite(opt->adam_eps)) {
        set_error(w + ": lr must be finite and > 0, beta1 and beta2 in [0, 1), adam_eps finite and >= 0");
        return false;
    }
    if (!(opt->surface_weight >= 0.0) || !std::isfinite(opt->surface_weight) || !(opt->eikonal_weight >= 0.0) ||
        !std::isfinite(opt->eikonal_weight) || !(opt->surface_eps > 0.0) || !std::isfinite(opt->surface_eps)) {
        set_error(w + ": surface_weight and eikonal_weight must be finite and >= 0, surface_eps finite and > 0");
        return false;
    }
    return true;
}

TrainK kernel_options(const NlotSdfTrainOptions* o) {
    return TrainK{o->lr, o->beta1, o->beta2, (float)o->adam_eps, (float)o->surface_weight, (float)o->surface_eps,
                  (float)o->eikonal_weight};
}

}  // namespace
}  // namespace nlot

extern "C" void nlot_sdf_train_default_options(NlotSdfTrainOptions* opt) {
    if (!opt) return;
    *opt = NlotSdfTrainOptions{128, 1, 256, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1e-2, 0.0};
}

extern "C" int64_t nlot_sdf_train_state_floats(const NlotSdfTrainOptions* opt) {
    using namespace nlot;
    if (!opt || opt->hidden != H || opt->n_hidden != 1) return 0;
    return 3 * (int64_t)N_PARAMS + 1;
}

extern "C" int32_t nlot_sdf_train_steps(const NlotSdfTrainOptions* opt, float* state, const float* pts,
                                        const float* target, const int32_t* order, int64_t n, int64_t first_row,
                                        int64_t n_rows, float* step_loss, float* grad_last, int64_t M, void* stream) {
    using namespace nlot;
    static_assert(sizeof(NlotSdfTrainOptions) == 72, "include/nlot.h");
    if (!opt || !state || !pts || !target || !order || !step_loss) {
        set_error("nlot_sdf_train_steps: null pointer");
        return NLOT_ERR_INVALID;
    }
    if (!check_options(opt, "nlot_sdf_train_steps")) return NLOT_ERR_INVALID;
    if (M < 1 || M > 65535) {
        set_error("nlot_sdf_train_steps: M out of range");
        return NLOT_ERR_INVALID;
    }
    if (n < 1 || n > (int64_t)1 << 30 || n_rows < 1 || n_rows > (int64_t)1 << 30) {
        set_error("nlot_sdf_train_steps: n and n_rows must be in 1 .. 2^30");
        return NLOT_ERR_INVALID;
    }
    if (first_row < 0 || first_row >= n_rows || first_row % BATCH != 0) {
        set_error("nlot_sdf_train_steps: first_row must be a multiple of 256 in [0, n_rows)");
        return NLOT_ERR_INVALID;
    }
    const int n_steps = (int)((n_rows - first_row + BATCH - 1) / BATCH);
    const TrainK K = kernel_options(opt);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)M), block(NTHREADS);
    static std::atomic<uint64_t> set_e{0}, set_p{0};
    if (K.we > 0.f) {
        NLOT_HIP_CHECK(set_lds_attr_once(set_e, (const void*)k_sdf_train<true>, (int)kTrainLds));
        hipLaunchKernelGGL(k_sdf_train<true>, grid, block, kTrainLds, st, K, state, pts, target, order, n, first_row,
                           n_rows, n_steps, step_loss, grad_last);
    } else {
        NLOT_HIP_CHECK(set_lds_attr_once(set_p, (const void*)k_sdf_train<false>, (int)kTrainLds));
        hipLaunchKernelGGL(k_sdf_train<false>, grid, block, kTrainLds, st, K, state, pts, target, order, n, first_row,
                           n_rows, n_steps, step_loss, grad_last);
    }
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

extern "C" int32_t nlot_sdf_batch_loss(const NlotSdfTrainOptions* opt, const float* state, const float* pts,
                                       const float* target, int64_t n, float* batch_loss, int64_t M, void* stream) {
    using namespace nlot;
    if (!opt || !state || !pts || !target || !batch_loss) {
        set_error("nlot_sdf_batch_loss: null pointer");
        return NLOT_ERR_INVALID;
    }
    if (!check_options(opt, "nlot_sdf_batch_loss")) return NLOT_ERR_INVALID;
    if (M < 1 || M > 65535) {
        set_error("nlot_sdf_batch_loss: M out of range");
        return NLOT_ERR_INVALID;
    }
    if (n < 1 || n > (int64_t)1 << 30) {
        set_error("nlot_sdf_batch_loss: n must be in 1 .. 2^30");
        return NLOT_ERR_INVALID;
    }
    static std::atomic<uint64_t> set_l{0};
    NLOT_HIP_CHECK(set_lds_attr_once(set_l, (const void*)k_sdf_batch_loss, (int)kLossLds));
    const dim3 grid((unsigned)((n + BATCH - 1) / BATCH), (unsigned)M), block(NTHREADS);
    hipLaunchKernelGGL(k_sdf_batch_loss, grid, block, kLossLds, (hipStream_t)stream, kernel_options(opt), state, pts,
                       target, n, batch_loss);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}
