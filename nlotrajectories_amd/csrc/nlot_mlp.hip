// Batched learned-SDF MLP: value, lambda*gradient and lambda*Hessian at P points (gfx950).
//
// Replaces the per-point CasADi externals nn_sdf / jac_nn_sdf / adj1_nn_sdf / jac_adj1_nn_sdf
// (/root/reference/_l4c_generated/nn_sdf.cpp:57-104), whose TorchScript graphs evaluate
//   f(p) = w_out . relu(W_l ... relu(W_0 h0 + b_0) ...) + b_out,   h0 = scale*cos(p A + b0)  (FourierMLP,
//   core/nn_architectures.py:30-72)  or  h0 = relu(p A + b0)  (l4casadi naive MLP)
// in fp32, one 1x2 point per call.  Here one launch evaluates every corner of every knot of every
// active problem.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nlot_mlp.h"

namespace nlot {

int device_cus() {
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::atomic<int>& c = cus[dev & 63];
    int v = c.load(std::memory_order_relaxed);
    if (v == 0) {
        hipDeviceProp_t prop;
        v = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount
                                                                                               : 256;
        c.store(v, std::memory_order_relaxed);
    }
    return v;
}

int launch_mlp_strided(const MlpDev& w, const float* pts, int64_t n, const int* n_dev, int P_per, int64_t ld,
                       const float* lam, const MlpOut& out, bool full, hipStream_t stream, const MlpReuse* reuse) {
    if (n <= 0) return NLOT_OK;
    if (w.arith == NLOT_MLP_ARITH_SEQ)  // ReLU nets only (nlot_mlp_create_ex checks)
        return launch_mlp_seq(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
    if (w.act != NLOT_ACT_RELU) {  // smooth activations: forward hyper-duals (the ReLU masks / reuse do not apply)
        if (w.n_hidden < 0 || w.n_hidden > kMaxStreamLayers) {
            set_error("MLP kernel: 0 to 4 hidden HxH layers are supported for smooth activations");
            return NLOT_ERR_INVALID;
        }
        return launch_mlp_smooth(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
    }
    if (w.n_hidden < 1 || w.n_hidden > kMaxStreamLayers) {
        set_error("MLP kernel: 1 to 4 hidden HxH layers are supported (DESIGN.md §7)");
        return NLOT_ERR_INVALID;
    }
    // weights beyond LDS (H = 256, or more than 2 HxH layers): the layer-streaming kernel
    if (w.H == 256 || w.n_hidden > kMaxResidentLayers)
        return launch_mlp_stream(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
    // 2-128-128-1: the split-bf16 MFMA kernels (fp32-equivalent products); a net created with NLOT_MLP_ARITH_F32 (no
    // planes) or NLOT_MLP=f32 in the environment takes the f32-MFMA kernels
    static const bool use_bf16 = !(getenv("NLOT_MLP") && strcmp(getenv("NLOT_MLP"), "f32") == 0);
    if (w.H == 128 && w.n_hidden == 1 && use_bf16 && w.Wp)
        return launch_mlp_bf16(w, pts, n, n_dev, P_per, ld, lam, out, full, stream, reuse);
    return launch_mlp_f32(w, pts, n, n_dev, P_per, ld, lam, out, full, stream);
}

}  // namespace nlot

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" NlotMlp* nlot_mlp_create(const NlotMlpDesc* d) { return nlot_mlp_create_ex(d, NLOT_MLP_ARITH_SPLIT_BF16); }

extern "C" NlotMlp* nlot_mlp_create_ex(const NlotMlpDesc* d, int32_t arith) {
    using namespace nlot;
    if (arith != NLOT_MLP_ARITH_SPLIT_BF16 && arith != NLOT_MLP_ARITH_F32 && arith != NLOT_MLP_ARITH_SEQ) {
        set_error("nlot_mlp_create_ex: arith must be NLOT_MLP_ARITH_SPLIT_BF16, NLOT_MLP_ARITH_F32 or NLOT_MLP_ARITH_SEQ");
        return nullptr;
    }
    if (arith == NLOT_MLP_ARITH_SEQ && d && d->act != NLOT_ACT_RELU) {
        set_error("nlot_mlp_create_ex: NLOT_MLP_ARITH_SEQ is defined for ReLU nets only");
        return nullptr;
    }
    if (!d || !d->A || !d->b0 || !d->w_out || (d->n_hidden > 0 && (!d->W || !d->b))) {
        set_error("nlot_mlp_create: null descriptor or weight pointer");
        return nullptr;
    }
    if (d->act < NLOT_ACT_RELU || d->act > NLOT_ACT_SINE ||
        (d->in_kind != NLOT_MLP_IN_FOURIER && d->in_kind != NLOT_MLP_IN_LINEAR_RELU)) {
        set_error("nlot_mlp_create: activation must be NLOT_ACT_* and the input layer Fourier or Linear+act");
        return nullptr;
    }
    const bool smooth = d->act != NLOT_ACT_RELU;
    if ((d->hidden != 64 && d->hidden != 128 && d->hidden != 256) || d->n_hidden < (smooth ? 0 : 1) ||
        d->n_hidden > kMaxStreamLayers) {
        set_error("nlot_mlp_create: hidden width 64/128/256 with 1-4 hidden HxH layers supported (0-4 for smooth "
                  "activations; DESIGN.md §7)");
        return nullptr;
    }
    const int H = d->hidden, L = d->n_hidden;
    const size_t nA = 2 * H, nb0 = H, nW = (size_t)L * H * H, nb = (size_t)L * H, nw = H;
    const bool split = arith == NLOT_MLP_ARITH_SPLIT_BF16;
    const size_t nWp = split ? (size_t)3 * H * H / 2 : 0;  // bf16 planes of layer 0, in float units
    const size_t nWt = smooth ? nW : 0;        // transposed HxH layers (mlp_smooth)
    const size_t total = nA + nb0 + nW + nb + nw + nWp + nWt + 4;
    float* blk = nullptr;
    if (hipMalloc(&blk, total * sizeof(float)) != hipSuccess) {
        set_error("nlot_mlp_create: hipMalloc failed");
        return nullptr;
    }
    float* p = blk;
    auto put = [&](const float* src, size_t cnt) -> float* {
        float* dst = p;
        if (cnt) hipMemcpy(dst, src, cnt * sizeof(float), hipMemcpyHostToDevice);
        p += cnt;
        return dst;
    };
    NlotMlp* m = new NlotMlp;
    m->block = blk;
    m->device = 0;
    (void)hipGetDevice(&m->device);
    m->dev.arith = arith;
    m->dev.in_kind = d->in_kind;
    m->dev.H = H;
    m->dev.n_hidden = L;
    m->dev.act = d->act;
    m->dev.scale = d->fourier_scale;
    m->dev.b_out = d->b_out;
    m->dev.A = put(d->A, nA);
    m->dev.b0 = put(d->b0, nb0);
    m->dev.W = put(d->W, nW);
    m->dev.b = put(d->b, nb);
    m->dev.w_out = put(d->w_out, nw);
    m->dev.Wp = nullptr;
    if (L > 0 && split) {  // layer-0 weights split into three bf16 planes, round-to-nearest-even at each step (host, exact)
        std::vector<uint16_t> planes((size_t)3 * H * H);
        auto bf16_rne = [](float x) -> uint16_t {
            uint32_t u;
            memcpy(&u, &x, 4);
            return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
        };
        auto bf16_f = [](uint16_t h) -> float {
            const uint32_t u = (uint32_t)h << 16;
            float f;
            memcpy(&f, &u, 4);
            return f;
        };
        for (size_t i = 0; i < (size_t)H * H; ++i) {
            const float x = d->W[i];
            const uint16_t hi = bf16_rne(x);
            const float r = x - bf16_f(hi);
            const uint16_t mid = bf16_rne(r);
            const uint16_t lo = bf16_rne(r - bf16_f(mid));
            planes[i] = hi;
            planes[(size_t)H * H + i] = mid;
            planes[(size_t)2 * H * H + i] = lo;
        }
        m->dev.Wp = put(reinterpret_cast<const float*>(planes.data()), nWp);
    }
    m->dev.Wt = nullptr;
    if (smooth && L > 0) {  // [l][in][out] for mlp_smooth's coalesced rows
        std::vector<float> wt(nW);
        for (int l = 0; l < L; ++l)
            for (int o = 0; o < H; ++o)
                for (int k = 0; k < H; ++k) wt[(size_t)l * H * H + (size_t)k * H + o] = d->W[(size_t)l * H * H + (size_t)o * H + k];
        m->dev.Wt = put(wt.data(), nWt);
    }
    if (hipDeviceSynchronize() != hipSuccess) {
        set_error("nlot_mlp_create: copy failed");
        hipFree(blk);
        delete m;
        return nullptr;
    }
    return m;
}

extern "C" void nlot_mlp_destroy(NlotMlp* m) {
    if (!m) return;
    nlot::casadi_unbind(m);
    hipFree(m->block);
    delete m;
}

extern "C" int32_t nlot_sdf_mlp_eval(const NlotMlp* mlp, const float* pts, int64_t P, float* val, float* grad,
                                     const float* lam, float* hess, void* stream) {
    using namespace nlot;
    if (!mlp || !pts || !val || P < 0) {
        set_error("nlot_sdf_mlp_eval: null argument");
        return NLOT_ERR_INVALID;
    }
    MlpOut o{};
    o.val = val;
    o.sv = 1;
    if (grad) {
        o.gx = grad;
        o.gy = grad + 1;
        o.sg = 2;
    }
    if (hess) {
        o.hxx = hess;
        o.hxy = hess + 1;
        o.hyx = hess + 2;
        o.hyy = hess + 3;
        o.sh = 4;
    }
    const bool full = grad || hess;  // every kernel skips a null grad or hess plane (jac_adj1 alone is allowed)
    return launch_mlp_strided(mlp->dev, pts, P, nullptr, 1, 0, lam, o, full, (hipStream_t)stream);
}
