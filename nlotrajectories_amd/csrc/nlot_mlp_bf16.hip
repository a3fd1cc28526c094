// Split-bf16 MFMA kernels with fp32-equivalent products (Fourier / ReLU input layer, one HxH layer).
// Both operands are split into three bf16 parts, x = x_hi + x_mid + x_lo (8 + 8 + 8 significant bits,
// exact up to 2^-24 relative), and each 32x32x16 block takes the six products down to 2^-24:
// hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid — every product exact in the fp32 accumulator, the dropped
// ones below fp32 rounding.  6 v_mfma_f32_32x32x16_bf16 (6 x 32 cycles) replace 8 v_mfma_f32_32x32x2_f32
// (8 x 64 cycles) per 16 k.  The weight planes are split once at nlot_mlp_create (MlpDev::Wp) and staged
// once per block as one row-major image; the forward GEMM reads it by rows (ds_read_b128), the reverse
// sweep G = W^T (lam w_out .* mask) by transposed reads (ds_read_b64_tr_b16) — one image for both.  The
// input-layer activations are split as they are computed, directly in the B-operand layout (lane l:
// point l & 31, k = 16 s + 8 (l >> 5) + j); the reverse sweep's B operand is the forward accumulator
// (mask and w_out) split in place (accumulator-as-operand k order).
#include "nlot_mlp.h"

namespace nlot {

__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
#pragma clang fp contract(off)  // x is the rounded fp32 input: never fuse its producer into the subtractions
    h = (__bf16)x;
    const float r = x - (float)h;  // exact
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);    // exact difference
}

// The five smaller split products of a k block into a running accumulator of their own; the hi x hi products go into
// the main one and the two are added once per output tile by a VALU add (round to nearest).  One
// v_mfma_f32_32x32x16_bf16 aligns its addends (the accumulator and its 16 products) to the largest of them and keeps
// about two bits below that one's fp32 ulp (scripts/mfma_round_probe.hip), so small products added straight to a large
// running sum lose their low bits; their own sum stays ~2^-8 of the main one and keeps them.
// The reverse sweep (G = W^T e, the gradient and Hessian) uses it: with mfma6's direct accumulation there the product
// net left benchmark 6's pinned path on instances where no fp32 summation order of the oracle's net does
// (profiles/r06/ab_split_two_acc/).  A second accumulator restarted from zero and added per k block
// gave the same fix for 3.6 % more time on the full launch (1.569 against 1.513 ms, profiles/r06/ab_rev_acc/).  The
// forward GEMMs keep mfma6: a second accumulator there halves the value's -5e-9 offset, but the value kernel spills
// at 3 waves per SIMD (-20 % there, -5 % traj/s).
__device__ __forceinline__ f32x16 mfma5s(const bf16x8& ah, const bf16x8& am, const bf16x8& al, const bf16x8& bh,
                                         const bf16x8& bm, const bf16x8& bl, f32x16 acs) {
    acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acs, 0, 0, 0);
    acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acs, 0, 0, 0);
    acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acs, 0, 0, 0);
    acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acs, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acs, 0, 0, 0);
}

// six split-bf16 products, smallest terms first
__device__ __forceinline__ f32x16 mfma6(const bf16x8& ah, const bf16x8& am, const bf16x8& al, const bf16x8& bh,
                                        const bf16x8& bm, const bf16x8& bl, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
    return acc;
}

// A fragment (32x32x16) of W^T from the row-major plane image by two transposed reads: lane group
// g = lane / 16 covers columns c0 = col0 + 16 (g & 1) .. +15 of W; lane 4q + p of the group supplies row
// r0 + q, columns c0 + 4p .. +3, and receives its own column's 4 rows.  Rows follow the
// accumulator-as-operand k order: element jj of lane half h is row jbase + 8 (jj >> 2) + 4 h + (jj & 3).
template <int RS>
__device__ __forceinline__ bf16x8 wt_frag(const __bf16* plane, int jbase, int col0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3, h = g >> 1;
    const int c0 = col0 + 16 * (g & 1);
    const __bf16* a0 = plane + (size_t)(jbase + 4 * h + q) * RS + c0 + 4 * p;
    const __bf16* a1 = a0 + (size_t)8 * RS;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(a0));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(a1));
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// one weight image per CU, shared by block size / 256 waves per SIMD: value-only launches 3 (512 and 1024 threads
// gained nothing over 768, profiles/r06/ab_value_threads/); FULL (value + reverse sweep) 2.  Round 4: the input layer
// is a template parameter (no per-element branch on the kind), its weights are read as float4 runs (a lane's 8
// consecutive k of a 16-wide k block), and the reverse sweep's contraction re-reads its LDS operands every tile (an
// opaque zero offset keeps the compiler from hoisting 192 loop-invariant floats into registers across the tile loop,
// which had pinned FULL at one wave per SIMD: 256 VGPRs + 184 AGPRs, or 504 B/lane of scratch at two).
constexpr int kBf16ValueThreads = 768, kBf16FullThreads = 512;
__host__ __device__ constexpr int bf16_threads(bool full) { return full ? kBf16FullThreads : kBf16ValueThreads; }

template <int H>
__host__ __device__ constexpr size_t mlp_bf16_lds_bytes() {
    return (size_t)3 * H * (H + 8) * 2 + (size_t)8 * H * 4;
}

// a zero the compiler cannot see through (a VGPR written by an opaque move): added to an LDS offset inside a loop,
// it keeps loop-invariant LDS reads in the loop
__device__ __forceinline__ int opaque_zero() {
    int z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return z;
}

__device__ __forceinline__ void lds8(const float* p, float (&o)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w, o[4] = b.x, o[5] = b.y, o[6] = b.z, o[7] = b.w;
}

// input-layer activation of z = p @ A + b0 (nn_architectures.py:38 for the Fourier layer)
template <bool FOUR>
__device__ __forceinline__ float in_act(float z, float scale) {
    if constexpr (FOUR) {
        // rounded product (no contraction into split3's subtraction): h0 is the fp32 value the oracle forms
#pragma clang fp contract(off)
        return __builtin_amdgcn_cosf(turns_fourier(z)) * scale;
    } else {
        return z > 0.f ? z : 0.f;
    }
}

template <int H, bool FULL, bool FOUR>
__global__ __launch_bounds__(bf16_threads(FULL), 1) void mlp_bf16(MlpDev w, const float* __restrict__ pts, int64_t cnt_host,
                                                            const int* __restrict__ cnt_dev, int P_per, int64_t ld,
                                                            const float* __restrict__ lam, MlpOut out, MlpReuse ru) {
    constexpr int RS = H + 8;    // padded plane row (bf16): 16-byte rows offset by 4 banks
    constexpr int NT = H / 32;   // 32-row tiles
    constexpr int NKB = H / 16;  // 16-wide k blocks
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* sWp = reinterpret_cast<__bf16*>(smem);                  // [3][H][RS]
    float* sA0 = reinterpret_cast<float*>(sWp + (size_t)3 * H * RS);  // [H]
    float* sA1 = sA0 + H;
    float* sb0 = sA1 + H;
    float* sb = sb0 + H;
    float* sw = sb + H;
    float* sq = sw + H;  // [3][H]: A0^2, A0 A1, A1^2 (the Fourier Hessian's per-k factors, as the oracle rounds them)
    __shared__ int s_reused;
    for (int idx = threadIdx.x; idx < 3 * H * H / 8; idx += blockDim.x) {  // 16-byte chunks of the planes
        const int pr = idx / (H / 8), c8 = idx % (H / 8);                   // pr = plane * H + row
        *reinterpret_cast<uint4*>(sWp + (size_t)pr * RS + c8 * 8) = reinterpret_cast<const uint4*>(w.Wp)[idx];
    }
    for (int idx = threadIdx.x; idx < H; idx += blockDim.x) {
        const float a0 = w.A[idx], a1 = w.A[H + idx];
        sA0[idx] = a0;
        sA1[idx] = a1;
        sb0[idx] = w.b0[idx];
        sb[idx] = w.b[idx];
        sw[idx] = w.w_out[idx];
        sq[idx] = a0 * a0;
        sq[H + idx] = a0 * a1;
        sq[2 * H + idx] = a1 * a1;
    }
    if (threadIdx.x == 0) s_reused = 0;
    __syncthreads();

    const int64_t cnt = point_count(cnt_dev, cnt_host);
    const int64_t npts = cnt * P_per;
    const int64_t g0 = (ru.base && ld == 0) ? (int64_t)(*ru.base) * P_per : 0;  // first point of the launch
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int il = lane & 31, hl = lane >> 5;
    const float scale = w.scale;
    constexpr int TP = bf16_threads(FULL) / 2;  // points per block tile (32 per wave)
    if constexpr (!FULL) {
        // Value-only launches, software-pipelined inside the wave: the B fragment (input-layer activations, split)
        // of k block s + 1 — or, in the last block, block 0 of the wave's NEXT tile — is computed between the MFMAs
        // of block s (2 elements per 32x32 output tile), so a wave's VALU work issues into its own MFMA gaps
        // instead of alternating with them.  Same arithmetic per point as the FULL forward below.
        static_assert(8 % NT == 0, "two input-layer elements per output tile and k block");
        constexpr int EPT = 8 / NT;
        const int64_t G = gridDim.x;
        auto point = [&](int64_t tile, float& x, float& y) {
            const int64_t gi = g0 + tile * TP + wave * 32 + il;
            x = y = 0.f;
            if (gi < npts) {
                const int64_t pi = point_addr(gi, cnt, ld);
                x = pts[2 * pi];
                y = pts[2 * pi + 1];
            }
        };
        float cx, cy, nx, ny;
        point(blockIdx.x, cx, cy);
        point(blockIdx.x + G, nx, ny);
        bf16x8 bh, bm, bl;
        {
            float a0[8], a1[8], c0[8];
            lds8(sA0 + 8 * hl, a0);
            lds8(sA1 + 8 * hl, a1);
            lds8(sb0 + 8 * hl, c0);
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                __bf16 a, b, c;
                split3(in_act<FOUR>(fmaf(cy, a1[jj], cx * a0[jj]) + c0[jj], scale), a, b, c);
                bh[jj] = a;
                bm[jj] = b;
                bl[jj] = c;
            }
        }
        for (int64_t tile = blockIdx.x; g0 + tile * TP < npts; tile += G) {
            float fx, fy;
            point(tile + 2 * G, fx, fy);
            f32x16 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
#pragma unroll 1
            for (int s = 0; s < NKB; ++s) {
                const bool last = s == NKB - 1;
                const int sn = last ? 0 : s + 1;
                const float qx = last ? nx : cx, qy = last ? ny : cy;
                float a0[8], a1[8], c0[8];
                const int kn = 16 * sn + 8 * hl;
                lds8(sA0 + kn, a0);
                lds8(sA1 + kn, a1);
                lds8(sb0 + kn, c0);
                bf16x8 nh, nm, nl;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const __bf16* rowp = sWp + (size_t)(t * 32 + il) * RS + 16 * s + 8 * hl;
                    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(rowp);
                    const bf16x8 am = *reinterpret_cast<const bf16x8*>(rowp + (size_t)H * RS);
                    const bf16x8 al = *reinterpret_cast<const bf16x8*>(rowp + (size_t)2 * H * RS);
                    acc[t] = mfma6(ah, am, al, bh, bm, bl, acc[t]);
#pragma unroll
                    for (int u = 0; u < EPT; ++u) {
                        const int jj = t * EPT + u;
                        __bf16 a, b, c;
                        split3(in_act<FOUR>(fmaf(qy, a1[jj], qx * a0[jj]) + c0[jj], scale), a, b, c);
                        nh[jj] = a;
                        nm[jj] = b;
                        nl[jj] = c;
                    }
                }
                bh = nh;
                bm = nm;
                bl = nl;
            }
            float fpart = 0.f;
            uint64_t mk = 0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = t * 32 + acc_row(r, hl);
                    const float v = acc[t][r] + sb[j];
                    const int on = min(max(__float_as_int(v), 0), 1);
                    fpart = fmaf(sw[j], fmaxf(v, 0.f), fpart);
                    mk |= (uint64_t)on << (t * 16 + r);
                }
            const float fw = fpart + __shfl_xor(fpart, 32) + w.b_out;
            const int64_t gi = g0 + tile * TP + wave * 32 + il;
            if (gi < npts) {
                const int64_t pi = point_addr(gi, cnt, ld);
                if (hl == 0) out.val[pi * out.sv] = fw;
                if (out.mask) {
                    out.mask[(2 * hl) * out.mask_plane + pi] = (uint32_t)mk;
                    out.mask[(2 * hl + 1) * out.mask_plane + pi] = (uint32_t)(mk >> 32);
                }
            }
            cx = nx;
            cy = ny;
            nx = fx;
            ny = fy;
        }
        return;
    }

    // A block's tiles are tile0, tile0 + G, ...: each tile's inputs (point, the reuse source and, one tile later,
    // the source's trial point / value / ReLU pattern) are loaded ahead, so the dependent global round trips of a
    // tile overlap the previous tile's MFMA work
    struct TileIn {
        float px, py;
        int src;
    };
    struct ReuseIn {
        float tx, ty, tv;
        uint32_t m0, m1;
    };
    const bool reuse_on = FULL && ru.src && ld == 0;
    auto load_in = [&](int64_t tile, TileIn& a) {
        const int64_t gi = g0 + tile * TP + wave * 32 + il;
        a.px = a.py = 0.f;
        a.src = -1;
        if (gi < npts) {
            const int64_t pi = point_addr(gi, cnt, ld);
            a.px = pts[2 * pi];
            a.py = pts[2 * pi + 1];
            if (reuse_on) a.src = ru.src[gi / P_per];
        }
    };
    auto load_reuse = [&](int64_t tile, const TileIn& a, ReuseIn& r) {
        r.tx = r.ty = r.tv = 0.f;
        r.m0 = r.m1 = 0u;
        if (reuse_on && a.src >= 0) {
            const int64_t gi = g0 + tile * TP + wave * 32 + il;
            const int64_t q = (int64_t)a.src * P_per + (gi - (gi / P_per) * P_per);
            r.tx = ru.tpts[2 * q];
            r.ty = ru.tpts[2 * q + 1];
            r.tv = ru.tval[q];
            r.m0 = ru.tmask[(2 * hl) * ru.plane + q];
            r.m1 = ru.tmask[(2 * hl + 1) * ru.plane + q];
        }
    };
    const int64_t G = gridDim.x;
    TileIn in0, in1;
    ReuseIn re0;
    load_in(blockIdx.x, in0);
    load_reuse(blockIdx.x, in0, re0);
    load_in(blockIdx.x + G, in1);
    for (int64_t tile = blockIdx.x; g0 + tile * TP < npts; tile += G) {
        TileIn in2;
        ReuseIn re1;
        load_in(tile + 2 * G, in2);
        load_reuse(tile + G, in1, re1);
        const int64_t gi = g0 + tile * TP + wave * 32 + il;
        const bool valid = gi < npts;
        const int64_t pi = valid ? point_addr(gi, cnt, ld) : 0;
        const float px = in0.px, py = in0.py;
        // ---------------- forward reuse (full launches after an accepted trial point) ----------------
        float f = 0.f;
        uint64_t mask = 0;
        bool have = false;
        if (reuse_on && valid && in0.src >= 0 && re0.tx == px && re0.ty == py) {
            f = re0.tv;
            mask = (uint64_t)re0.m0 | ((uint64_t)re0.m1 << 32);
            have = true;
        }
        const bool skip = __all(have || !valid);  // wave-uniform
        if (FULL && skip && ru.nreused) {
            const uint64_t vb = __ballot(valid && hl == 0);
            if (lane == 0) atomicAdd(&s_reused, (int)__popcll(vb));
        }
        if (!skip) {  // the forward for all 32 points of the wave
        // ---------------- input layer + hidden GEMM ----------------
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
#pragma unroll 1
        for (int s = 0; s < NKB; ++s) {
            // the lane's 8 consecutive k of this block: k = 16 s + 8 hl + jj
            float a0[8], a1[8], c0[8];
            const int k0 = 16 * s + 8 * hl;
            lds8(sA0 + k0, a0);
            lds8(sA1 + k0, a1);
            lds8(sb0 + k0, c0);
            bf16x8 bh, bm, bl;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float z = fmaf(py, a1[jj], px * a0[jj]) + c0[jj];
                __bf16 a, b, c;
                split3(in_act<FOUR>(z, scale), a, b, c);
                bh[jj] = a;
                bm[jj] = b;
                bl[jj] = c;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const __bf16* rowp = sWp + (size_t)(t * 32 + il) * RS + 16 * s + 8 * hl;
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(rowp);
                const bf16x8 am = *reinterpret_cast<const bf16x8*>(rowp + (size_t)H * RS);
                const bf16x8 al = *reinterpret_cast<const bf16x8*>(rowp + (size_t)2 * H * RS);
                acc[t] = mfma6(ah, am, al, bh, bm, bl, acc[t]);
            }
        }
        // ---------------- bias + ReLU + output layer (accumulator layout of the f32 MFMA: acc_row) ----------------
        float fpart = 0.f;
        uint64_t mk = 0;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = t * 32 + acc_row(r, hl);
                const float v = acc[t][r] + sb[j];
                // on = v > 0 without a compare: the int image of a float is > 0 exactly for v > 0 (-0 and the
                // negatives have the sign bit); clamp(., 0, 1) is one v_med3_i32, max(v, 0) one v_max_f32
                const int on = min(max(__float_as_int(v), 0), 1);
                fpart = fmaf(sw[j], fmaxf(v, 0.f), fpart);
                mk |= (uint64_t)on << (t * 16 + r);
            }
        const float fw = fpart + __shfl_xor(fpart, 32) + w.b_out;
        if (!have) {
            f = fw;
            mask = mk;
        }
        }  // forward
        if constexpr (FULL) {  // (the value-only launches have returned above)
            // ---------------- reverse sweep: G = W^T e, e = lam * w_out .* mask ----------------
            // e is split once into the B fragments of all 2 NT k-steps (blk = 2 tj + sl: accumulator registers
            // 8 sl .. 8 sl + 7 of output tile tj, permuted k order; 3 NT x 2 x 4 VGPRs); then output tile tk of
            // G = W^T e accumulates over the k-steps while the contraction of tile tk - 1 (whose accumulator is
            // complete) runs between its MFMAs: 2 of its 16 rows per k-step
            const float lm = lam ? (valid ? lam[pi] : 0.f) : 1.f;
            constexpr int NB = 2 * NT;
            bf16x8 Bh[NB], Bm[NB], Bl[NB];
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) {
                const int tj = blk >> 1, sl = blk & 1;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const int r = 8 * sl + jj;
                    const float e = ((mask >> (tj * 16 + r)) & 1) ? lm * sw[tj * 32 + acc_row(r, hl)] : 0.f;
                    __bf16 a, b, c;
                    split3(e, a, b, c);
                    Bh[blk][jj] = a;
                    Bm[blk][jj] = b;
                    Bl[blk][jj] = c;
                }
            }
            // g = df/dh0 (x lam): contract with the input layer's derivatives (lane: k rows, point); the four rows
            // of a register quad are consecutive k: one 16-byte read per input-layer vector
            float gx = 0.f, gy = 0.f, hxx = 0.f, hxy = 0.f, hyy = 0.f;
            const int zo = opaque_zero();
            auto contract2 = [&](const f32x16& gp, int tp, int r0) {  // rows r0, r0 + 1 of output tile tp
                const int r4 = r0 >> 2, rr0 = r0 & 3;
                const int k0 = tp * 32 + 8 * r4 + 4 * hl + zo;
                const float4 A0 = *reinterpret_cast<const float4*>(sA0 + k0);
                const float4 A1 = *reinterpret_cast<const float4*>(sA1 + k0);
                const float4 B0 = *reinterpret_cast<const float4*>(sb0 + k0);
                float4 Q0, Q1, Q2;  // A0^2, A0 A1, A1^2 (staged once per block)
                if constexpr (FOUR) {
                    Q0 = *reinterpret_cast<const float4*>(sq + k0);
                    Q1 = *reinterpret_cast<const float4*>(sq + H + k0);
                    Q2 = *reinterpret_cast<const float4*>(sq + 2 * H + k0);
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int rr = rr0 + u;
                    const float ax = rr == 0 ? A0.x : rr == 1 ? A0.y : rr == 2 ? A0.z : A0.w;
                    const float ay = rr == 0 ? A1.x : rr == 1 ? A1.y : rr == 2 ? A1.z : A1.w;
                    const float bz = rr == 0 ? B0.x : rr == 1 ? B0.y : rr == 2 ? B0.z : B0.w;
                    const float z = fmaf(py, ay, px * ax) + bz;
                    const float d = gp[r0 + u];
                    if constexpr (FOUR) {  // the factor -scale is applied to the sums
                        const float qxx = rr == 0 ? Q0.x : rr == 1 ? Q0.y : rr == 2 ? Q0.z : Q0.w;
                        const float qxy = rr == 0 ? Q1.x : rr == 1 ? Q1.y : rr == 2 ? Q1.z : Q1.w;
                        const float qyy = rr == 0 ? Q2.x : rr == 1 ? Q2.y : rr == 2 ? Q2.z : Q2.w;
                        const float tz = turns_fourier(z);
                        const float dz = d * __builtin_amdgcn_sinf(tz);
                        const float c2 = d * __builtin_amdgcn_cosf(tz);
                        gx = fmaf(ax, dz, gx);
                        gy = fmaf(ay, dz, gy);
                        hxx = fmaf(qxx, c2, hxx);
                        hxy = fmaf(qxy, c2, hxy);
                        hyy = fmaf(qyy, c2, hyy);
                    } else {  // ReLU input layer: piecewise linear, Hessian 0 a.e.
                        const float dz = z > 0.f ? d : 0.f;
                        gx = fmaf(ax, dz, gx);
                        gy = fmaf(ay, dz, gy);
                    }
                }
            };
            static_assert(NB == 8, "2 contraction rows per k-step cover a 16-row output tile");
            f32x16 gprev = f32x16{};
#pragma unroll
            for (int tk = 0; tk < NT; ++tk) {
                f32x16 g = f32x16{}, gs = f32x16{};
#pragma unroll
                for (int blk = 0; blk < NB; ++blk) {
                    const int jbase = 16 * blk;  // 32 tj + 16 sl
                    const bf16x8 ah = wt_frag<RS>(sWp, jbase, 32 * tk, lane);
                    const bf16x8 am = wt_frag<RS>(sWp + (size_t)H * RS, jbase, 32 * tk, lane);
                    const bf16x8 al = wt_frag<RS>(sWp + (size_t)2 * H * RS, jbase, 32 * tk, lane);
                    gs = mfma5s(ah, am, al, Bh[blk], Bm[blk], Bl[blk], gs);
                    g = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, Bh[blk], g, 0, 0, 0);
                    if (tk > 0) contract2(gprev, tk - 1, 2 * blk);
                }
                gprev = g + gs;
            }
#pragma unroll
            for (int r0 = 0; r0 < 16; r0 += 2) contract2(gprev, NT - 1, r0);
            const float sg = FOUR ? -scale : 1.f;
            gx = sg * (gx + __shfl_xor(gx, 32));
            gy = sg * (gy + __shfl_xor(gy, 32));
            hxx = sg * (hxx + __shfl_xor(hxx, 32));
            hxy = sg * (hxy + __shfl_xor(hxy, 32));
            hyy = sg * (hyy + __shfl_xor(hyy, 32));
            if (valid && hl == 0) store_point(out, pi, f, gx, gy, hxx, hxy, hyy);
        }
        in0 = in1;  // the next tile's inputs (loaded during this tile)
        in1 = in2;
        re0 = re1;
    }
    if (FULL && ru.nreused) {  // statistics: full-launch points whose forward was reused
        __syncthreads();
        if (threadIdx.x == 0 && s_reused) atomicAdd(ru.nreused, s_reused);
    }
}

template <bool FULL>
static int launch_t(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                    const float* lam, const MlpOut& out, hipStream_t stream, const MlpReuse* reuse) {
    constexpr int H = 128;
    constexpr size_t lv = mlp_bf16_lds_bytes<H>();
    static std::atomic<uint64_t> attr_v{0}, attr_f{0};
    NLOT_HIP_CHECK(set_lds_attr_once(attr_v, (const void*)mlp_bf16<H, FULL, false>, (int)lv));
    NLOT_HIP_CHECK(set_lds_attr_once(attr_f, (const void*)mlp_bf16<H, FULL, true>, (int)lv));
    constexpr int NTB = bf16_threads(FULL);
    const int grid = persistent_grid(n * P_per, NTB / 2, device_cus());
    const MlpReuse ru = reuse ? *reuse : MlpReuse{};
    if (w.in_kind == NLOT_MLP_IN_FOURIER)
        hipLaunchKernelGGL((mlp_bf16<H, FULL, true>), dim3(grid), dim3(NTB), lv, stream, w, pts, n, n_dev, P_per, ld,
                           lam, out, ru);
    else
        hipLaunchKernelGGL((mlp_bf16<H, FULL, false>), dim3(grid), dim3(NTB), lv, stream, w, pts, n, n_dev, P_per, ld,
                           lam, out, ru);
    NLOT_HIP_CHECK(hipGetLastError());
    return NLOT_OK;
}

int launch_mlp_bf16(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                    const float* lam, const MlpOut& out, bool full, hipStream_t stream, const MlpReuse* reuse) {
    return full ? launch_t<true>(w, pts, n, n_dev, P_per, ld, lam, out, stream, reuse)
                : launch_t<false>(w, pts, n, n_dev, P_per, ld, lam, out, stream, reuse);
}

}  // namespace nlot
