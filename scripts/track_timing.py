"""Timings of DESIGN.md §13: tvlqr_batch and track_batch next to rollout_batch (the yardstick) on the metric body in
b3's scene, hipEvents around each call after warm-up calls.  One JSON line per batch size, every call listed.

    python scripts/track_timing.py [--B 32768 2048] [--N 50] [--warmup 3] [--reps 10]

The plans are seeded Euler plans (controls uniform in half the bounds from starts in the unit square); the times do not
depend on what the plans are, only on their shapes.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nlotrajectories_amd.cli import _f  # noqa: E402
from nlotrajectories_amd.problem import BENCHMARKS, METRIC_PROBLEM  # noqa: E402
from nlotrajectories_amd.rollout import rollout_batch  # noqa: E402
from nlotrajectories_amd.tracking import track_batch, tvlqr_batch  # noqa: E402


def euler_plans(p, B, seed=0):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-0.5, 0.5, (B, p.N, p.nu))
    X = np.zeros((B, p.N + 1, p.nx))
    X[:, 0, :2] = rng.uniform(0.0, 1.0, (B, 2))
    X[:, 0, 2] = rng.uniform(-np.pi, np.pi, B)
    for k in range(p.N):
        X[:, k + 1] = X[:, k] + p.dt * _f(p, X[:, k].T, U[:, k].T).T
    return X, U


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(round(a.elapsed_time(b), 4))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[32768, 2048])
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args(argv)
    p = METRIC_PROBLEM.with_(N=a.N)
    scene = BENCHMARKS["b3"]["problem"].obstacles
    for B in a.B:
        X, U = (torch.as_tensor(t, device="cuda") for t in euler_plans(p, B))
        K, _, st = tvlqr_batch(p, X, U)
        dx0 = torch.zeros(B, p.nx, dtype=torch.float64, device="cuda")
        dx0[:, 0], dx0[:, 1] = 0.02, -0.02
        t = lambda fn: timed(fn, a.warmup, a.reps)  # noqa: E731
        row = {"B": B, "N": a.N, "gains_status_nonzero": int((st != 0).sum()),
               "tvlqr_ms": t(lambda: tvlqr_batch(p, X, U)),
               "track_ms": t(lambda: track_batch(p, X, U, K=K, dx0=dx0, obstacles=scene)),
               "track_open_loop_ms": t(lambda: track_batch(p, X, U, obstacles=scene, clamp=False)),
               "track_no_scene_ms": t(lambda: track_batch(p, X, U, K=K, dx0=dx0)),
               "rollout_ms": t(lambda: rollout_batch(p, X, U, obstacles=scene)),
               "rollout_no_scene_ms": t(lambda: rollout_batch(p, X, U))}
        for k in [k for k in row if k.endswith("_ms")]:
            row[k.replace("_ms", "_median_ms")] = float(np.median(row[k]))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
