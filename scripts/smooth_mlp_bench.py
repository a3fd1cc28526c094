"""Launch time of a smooth-activation learned SDF: mlp_smooth (scalar FMA) against mlp_hdual (MFMA hyper-duals,
DeviceMlp(w, "hdual_mfma")).

Two nets of the artefact's shape: the artefact's FourierMLP 2-128-128-1 with tanh hidden layers, and a seeded SIREN
2-128-128-1.  Per net, full (value, gradient, Hessian) and value launches at --points points, timed with device events
around --reps launches after --warmup of them.  The kernels alternate mlp_smooth, mlp_hdual, mlp_smooth in one
process, so that the spread of the two mlp_smooth runs bounds what the machine itself contributes.  Achieved FLOP/s
counts the HxH layers' products only, 2 NC L H^2 per point (NC = 6 components full, 1 value), against the f32 MFMA
peak of 157.3 TFLOP/s.  Writes one JSON to profiles/smooth_mlp_bench.json and prints it.

--arith hdual_stream times mlp_hdual_stream (DeviceMlp(w, "hdual_stream"): activations in LDS, weights streamed from
L2) in the same mlp_smooth / kernel / mlp_smooth alternation on the shapes mlp_hdual cannot hold, a tanh 2-256x4-1 (the
stress shape) and a tanh net of H = 128 with 4 HxH layers, and on the artefact-shaped Fourier-tanh 2-128-128-1, where
mlp_hdual is timed as a third contestant.  That mode writes profiles/smooth_mlp_stream_bench.json.

--arith hdual_bf16 times mlp_hdual_bf16 (DeviceMlp(w, "hdual_bf16"): the split-bf16 MFMA products) against mlp_hdual
in the order mlp_hdual / mlp_hdual_bf16 / mlp_hdual, so that the spread of the two mlp_hdual runs bounds the machine's
share, with mlp_smooth's time as a third column, on the Fourier-tanh and SIREN 2-128-128-1 and a tanh 2-64x(4 HxH)-1.
FLOP/s are fp32-equivalent (one split product counted as one), against the f32 MFMA peak and against the split-bf16
roofline of 416.7 TFLOP/s (the bf16 MFMA peak over six).  That mode writes profiles/smooth_mlp_bf16_bench.json.

--arith hdual_bf16_stream times mlp_hdual_bf16_stream (DeviceMlp(w, "hdual_bf16_stream"): the split-bf16 products with
the split activations in LDS and the split weights streamed) against mlp_hdual_stream in the order mlp_hdual_stream /
mlp_hdual_bf16_stream / mlp_hdual_stream on the three nets of --arith hdual_stream, with the same fp32-equivalent
FLOP/s and both peaks.  That mode writes profiles/smooth_mlp_bf16_stream_bench.json.

    python scripts/smooth_mlp_bench.py [--arith hdual_mfma|hdual_stream|hdual_bf16|hdual_bf16_stream]
                                       [--points 1000000] [--reps 20] [--warmup 3]
"""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3  # v_mfma_f32_16x16x4_f32: 256 FLOP / cycle / CU x 256 CUs x 2.4 GHz
PEAK_SPLIT_TFLOPS = 416.7  # fp32-equivalent: the bf16 MFMA peak of 2500 TFLOP/s over six products per fp32 product


def time_ms(mlp, pts, full, reps, warmup):
    import torch

    from nlotrajectories_amd.ops import sdf_mlp_eval

    for _ in range(warmup):
        sdf_mlp_eval(mlp, pts, derivatives=full)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        sdf_mlp_eval(mlp, pts, derivatives=full)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def stream_bench(a, pts):
    """The --arith hdual_stream mode: {net: {launch: times}}."""
    import torch

    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.nn import MlpWeights, MultiLayerPerceptron
    from nlotrajectories_amd.ops import DeviceMlp

    torch.manual_seed(0)
    nets = {"mlp_tanh_2-256x4-1": MlpWeights.from_module(MultiLayerPerceptron(2, 256, 1, 4, "Tanh")),
            "mlp_tanh_2-128x5-1": MlpWeights.from_module(MultiLayerPerceptron(2, 128, 1, 5, "Tanh")),
            "fourier_tanh_2-128-128-1": dataclasses.replace(MlpWeights.artefact(), act=_abi.ACT_TANH)}
    out = {}
    for name, w in nets.items():
        smooth, stream = DeviceMlp(w, "f32"), DeviceMlp(w, "hdual_stream")
        hdual = DeviceMlp(w, "hdual_mfma") if w.n_hidden == 1 else None  # the one shape here the resident kernel holds
        res = {}
        for launch, full in (("full", True), ("value", False)):
            sa, st, sb = (time_ms(m, pts, full, a.reps, a.warmup) for m in (smooth, stream, smooth))
            flop = 2.0 * (6 if full else 1) * w.n_hidden * w.hidden ** 2 * a.points
            res[launch] = dict(mlp_smooth_ms=[sa, sb], mlp_smooth_spread_ms=abs(sa - sb), mlp_hdual_stream_ms=st,
                               speedup=min(sa, sb) / st, flop_per_point=flop / a.points,
                               mlp_hdual_stream_tflops=flop / st * 1e-9,
                               mlp_hdual_stream_share_of_peak=flop / st * 1e-9 / PEAK_TFLOPS,
                               mlp_smooth_tflops=flop / min(sa, sb) * 1e-9)
            if hdual:
                hd = time_ms(hdual, pts, full, a.reps, a.warmup)
                res[launch].update(mlp_hdual_ms=hd, stream_over_hdual=st / hd)
        out[name] = res
    return out


def bf16_bench(a, pts):
    """The --arith hdual_bf16 mode: {net: {launch: times}}."""
    import torch

    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.nn import SIREN, MlpWeights, MultiLayerPerceptron
    from nlotrajectories_amd.ops import DeviceMlp

    torch.manual_seed(0)
    nets = {"fourier_tanh_2-128-128-1": dataclasses.replace(MlpWeights.artefact(), act=_abi.ACT_TANH),
            "siren_2-128-128-1": MlpWeights.from_module(SIREN(2, 128, 1, num_layers=3, omega_0=30)),
            "mlp_tanh_2-64x5-1": MlpWeights.from_module(MultiLayerPerceptron(2, 64, 1, 5, "Tanh"))}
    out = {}
    for name, w in nets.items():
        hdual, split, smooth = DeviceMlp(w, "hdual_mfma"), DeviceMlp(w, "hdual_bf16"), DeviceMlp(w, "f32")
        res = {}
        for launch, full in (("full", True), ("value", False)):
            ha, sp, hb = (time_ms(m, pts, full, a.reps, a.warmup) for m in (hdual, split, hdual))
            sm = time_ms(smooth, pts, full, a.reps, a.warmup)
            flop = 2.0 * (6 if full else 1) * w.n_hidden * w.hidden ** 2 * a.points
            res[launch] = dict(mlp_hdual_ms=[ha, hb], mlp_hdual_spread_ms=abs(ha - hb), mlp_hdual_bf16_ms=sp,
                               mlp_smooth_ms=sm, speedup_over_hdual=min(ha, hb) / sp,
                               gain_ms=min(ha, hb) - sp, flop_per_point=flop / a.points,
                               mlp_hdual_bf16_tflops=flop / sp * 1e-9, mlp_hdual_tflops=flop / min(ha, hb) * 1e-9,
                               mlp_hdual_bf16_share_of_f32_peak=flop / sp * 1e-9 / PEAK_TFLOPS,
                               mlp_hdual_bf16_share_of_split_peak=flop / sp * 1e-9 / PEAK_SPLIT_TFLOPS)
        out[name] = res
    return out


def bf16_stream_bench(a, pts):
    """The --arith hdual_bf16_stream mode: {net: {launch: times}}."""
    import torch

    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.nn import MlpWeights, MultiLayerPerceptron
    from nlotrajectories_amd.ops import DeviceMlp

    torch.manual_seed(0)  # stream_bench's nets
    nets = {"mlp_tanh_2-256x4-1": MlpWeights.from_module(MultiLayerPerceptron(2, 256, 1, 4, "Tanh")),
            "mlp_tanh_2-128x5-1": MlpWeights.from_module(MultiLayerPerceptron(2, 128, 1, 5, "Tanh")),
            "fourier_tanh_2-128-128-1": dataclasses.replace(MlpWeights.artefact(), act=_abi.ACT_TANH)}
    out = {}
    for name, w in nets.items():
        stream, split = DeviceMlp(w, "hdual_stream"), DeviceMlp(w, "hdual_bf16_stream")
        res = {}
        for launch, full in (("full", True), ("value", False)):
            sa, sp, sb = (time_ms(m, pts, full, a.reps, a.warmup) for m in (stream, split, stream))
            flop = 2.0 * (6 if full else 1) * w.n_hidden * w.hidden ** 2 * a.points
            res[launch] = dict(mlp_hdual_stream_ms=[sa, sb], mlp_hdual_stream_spread_ms=abs(sa - sb),
                               mlp_hdual_bf16_stream_ms=sp, speedup_over_hdual_stream=min(sa, sb) / sp,
                               gain_ms=min(sa, sb) - sp, flop_per_point=flop / a.points,
                               mlp_hdual_bf16_stream_tflops=flop / sp * 1e-9,
                               mlp_hdual_stream_tflops=flop / min(sa, sb) * 1e-9,
                               mlp_hdual_bf16_stream_share_of_f32_peak=flop / sp * 1e-9 / PEAK_TFLOPS,
                               mlp_hdual_bf16_stream_share_of_split_peak=flop / sp * 1e-9 / PEAK_SPLIT_TFLOPS)
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", choices=["hdual_mfma", "hdual_stream", "hdual_bf16", "hdual_bf16_stream"],
                    default="hdual_mfma")
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch

    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.nn import SIREN, MlpWeights
    from nlotrajectories_amd.ops import DeviceMlp

    assert torch.cuda.is_available(), "smooth_mlp_bench.py measures on the GPU"
    torch.manual_seed(0)
    nets = {"fourier_tanh_2-128-128-1": dataclasses.replace(MlpWeights.artefact(), act=_abi.ACT_TANH),
            "siren_2-128-128-1": MlpWeights.from_module(SIREN(2, 128, 1, num_layers=3, omega_0=30))}
    pts = torch.tensor(np.random.default_rng(0).uniform(-0.5, 1.5, (a.points, 2)).astype(np.float32), device="cuda")
    out = dict(points=a.points, reps=a.reps, warmup=a.warmup, peak_tflops=PEAK_TFLOPS, nets={})
    if a.arith == "hdual_stream":
        nets = {}
        out.update(arith=a.arith, nets=stream_bench(a, pts))
    if a.arith == "hdual_bf16":
        nets = {}
        out.update(arith=a.arith, peak_split_tflops=PEAK_SPLIT_TFLOPS, nets=bf16_bench(a, pts))
    if a.arith == "hdual_bf16_stream":
        nets = {}
        out.update(arith=a.arith, peak_split_tflops=PEAK_SPLIT_TFLOPS, nets=bf16_stream_bench(a, pts))
    for name, w in nets.items():
        smooth, hdual = DeviceMlp(w, "f32"), DeviceMlp(w, "hdual_mfma")
        res = {}
        for launch, full in (("full", True), ("value", False)):
            sa, hd, sb = (time_ms(m, pts, full, a.reps, a.warmup) for m in (smooth, hdual, smooth))
            flop = 2.0 * (6 if full else 1) * w.n_hidden * w.hidden ** 2 * a.points
            res[launch] = dict(mlp_smooth_ms=[sa, sb], mlp_smooth_spread_ms=abs(sa - sb), mlp_hdual_ms=hd,
                               speedup=min(sa, sb) / hd, flop_per_point=flop / a.points,
                               mlp_hdual_tflops=flop / hd * 1e-9, mlp_hdual_share_of_peak=flop / hd * 1e-9 / PEAK_TFLOPS,
                               mlp_smooth_tflops=flop / min(sa, sb) * 1e-9)
        out["nets"][name] = res
    text = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = {"hdual_stream": "smooth_mlp_stream_bench.json", "hdual_bf16": "smooth_mlp_bf16_bench.json",
            "hdual_bf16_stream": "smooth_mlp_bf16_stream_bench.json"}.get(a.arith, "smooth_mlp_bench.json")
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
