"""MLP kernel microbenchmark: full (value + grad + Hessian) and value-only launches on the metric-size
point set (16384 instances x 204 corners), hipEvent-timed, with achieved TFLOP/s (fp32-equivalent flops) and the
fraction of the split-bf16 peak (2.5 PF/s dense bf16 / 6 products = 416.7 TF/s).  NLOT_LIB selects the build.

    python scripts/mlp_bench.py [P [artefact|stress|relu128x5 [arith]]]

With an arith (a DeviceMlp.ARITH name, e.g. split_bf16_stream) each launch kind is timed default / arith / default in
this process, and the times, the bracketing spread and the rates go to profiles/relu_bf16_stream_bench.json under the
net's name as well."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nlotrajectories_amd.nn import MlpWeights, MultiLayerPerceptron  # noqa: E402
from nlotrajectories_amd.ops import DeviceMlp, sdf_mlp_eval  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 16384 * 204
net = sys.argv[2] if len(sys.argv) > 2 else "artefact"
arith = sys.argv[3] if len(sys.argv) > 3 else None
if net == "stress":
    w = MlpWeights.stress_sdf_mlp(0)
elif net == "relu128x5":
    torch.manual_seed(0)
    w = MlpWeights.from_module(MultiLayerPerceptron(2, 128, 1, 5, "ReLU"))
else:
    w = MlpWeights.artefact()
pts = (torch.rand(P, 2, device="cuda") * 1.6 - 0.3).contiguous()


def time_ms(mlp, full, n=10):
    for _ in range(2):
        sdf_mlp_eval(mlp, pts, derivatives=full)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        sdf_mlp_eval(mlp, pts, derivatives=full)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def report(what, full, ms):
    flop = P * (w.flops_per_point_fwd_grad if full else w.flops_per_point_fwd)
    print(f"{what + ' ' if what else ''}{'full ' if full else 'value'} P={P} {ms:.3f} ms  {flop / ms / 1e9:.1f} TFLOP/s  "
          f"(frac {flop / ms / 1e9 / 416.7:.3f} of the split-bf16 peak)", flush=True)
    return flop / ms / 1e9


mlp = DeviceMlp(w)
if arith is None:
    for full in (True, False):
        report("", full, time_ms(mlp, full))
else:
    new, res = DeviceMlp(w, arith), {}
    for launch, full in (("full", True), ("value", False)):
        a, t, b = (time_ms(m, full) for m in (mlp, new, mlp))
        report("default", full, a)
        tf = report(arith, full, t)
        report("default", full, b)
        res[launch] = dict(default_ms=[a, b], default_spread_ms=abs(a - b), arith_ms=t, speedup=min(a, b) / t,
                           default_tflops=tf * t / min(a, b), arith_tflops=tf,
                           arith_share_of_split_peak=tf / 416.7)
    path = os.path.join(ROOT, "profiles", "relu_bf16_stream_bench.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    out[net] = dict(points=P, arith=arith, hidden=w.hidden, n_hidden=w.n_hidden, **res)
    with open(path, "w") as f:
        f.write(json.dumps(out) + "\n")
