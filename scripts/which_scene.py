"""Which scene was the shipped artefact net trained on?  (the caveat of §10 and §11.)

Evaluates the artefact FourierMLP (nlotrajectories_amd/data/nn_sdf_artefact.npz) against the exact SDF of each of the
six benchmark scenes with scene_gpu.scene_metrics (the reference's compute_metrics, on the device, 1000 x 1000 grid
of [-1, 2]^2) and prints one JSON line per scene.  The scene the net was trained on is the one with a small MSE and
an IoU near 1; the analytic approximated SDF of the same scene is printed next to it as the yardstick.

    python scripts/which_scene.py [--n 1000]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nlotrajectories_amd.nn import MlpWeights  # noqa: E402
from nlotrajectories_amd.ops import DeviceMlp  # noqa: E402
from nlotrajectories_amd.problem import BENCHMARKS  # noqa: E402
from nlotrajectories_amd.scene_gpu import scene_metrics  # noqa: E402

KEYS = ("mse", "iou", "hausdorff", "chamfer", "surface_loss")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000, help="grid points per axis")
    a = ap.parse_args(argv)
    mlp = DeviceMlp(MlpWeights.artefact())
    for name in sorted(BENCHMARKS):
        obs = BENCHMARKS[name]["problem"].obstacles
        row = {"scene": name, "n": a.n, "net": dict(zip(KEYS, scene_metrics(obs, mlp, n=a.n))),
               "analytic": dict(zip(KEYS, scene_metrics(obs, None, n=a.n)))}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
