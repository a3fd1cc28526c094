"""Time certify_batch (default options and decide=True) next to verify_batch at its defaults, same process, same plans.

    python scripts/certify_bench.py [--B 32768] [--N 50] [--scene b3] [--out profiles/certify_bench.json]

The plans are seeded and smooth: start and goal uniform in [-0.2, 1.3]^2, the straight line between them plus a
half-sine bump of amplitude uniform in [-0.3, 0.3] across it, the heading along the path; the metric workload's body in
the scene's obstacles.  hipEvents around each call, 3 warm-up calls, 10 timed: median and range in ms.  Also the mean
and largest evaluation count, the share of instances cut short by the budget, the verdicts, and how the instances
verify_batch passes split into proven clear / collision / undecided.  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def plans(problem, B, seed=0):
    rng = np.random.default_rng(seed)
    a, g = rng.uniform(-0.2, 1.3, (B, 1, 2)), rng.uniform(-0.2, 1.3, (B, 1, 2))
    s = np.linspace(0, 1, problem.N + 1)[None, :, None]
    d = g - a
    xy = a + s * d + rng.uniform(-0.3, 0.3, (B, 1, 1)) * np.sin(np.pi * s) * np.stack([-d[..., 1], d[..., 0]], -1)
    v = np.gradient(xy, axis=1)
    X = np.zeros((B, problem.N + 1, problem.nx))
    X[..., :2] = xy
    X[..., 2] = np.unwrap(np.arctan2(v[..., 1], v[..., 0]), axis=1)
    return X, np.zeros((B, problem.N, problem.nu))


def timed(fn, warmup=3, calls=10):
    import torch

    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32768)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--scene", default="b3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    import torch

    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.certify import certify_batch
    from nlotrajectories_amd.problem import BENCHMARKS, METRIC_PROBLEM
    from nlotrajectories_amd.verify import verify_batch

    prob, obs = METRIC_PROBLEM.with_(N=a.N), BENCHMARKS[a.scene]["problem"].obstacles
    X, U = (torch.tensor(t, device="cuda") for t in plans(prob, a.B))
    out = dict(B=a.B, N=a.N, scene=a.scene)
    v, out["verify"] = timed(lambda: verify_batch(prob, X, U, obstacles=obs))
    vok = (v["flags"] & (_abi.VERIFY_COLLISION | _abi.VERIFY_CONTAINS)).cpu().numpy() == 0
    for name, kw in (("certify", {}), ("certify_decide", dict(decide=True))):
        c, r = timed(lambda: certify_batch(prob, X, obstacles=obs, **kw))
        fl, ev = c["flags"].cpu().numpy(), c["evals"].cpu().numpy()
        hit = (fl & (_abi.CERTIFY_COLLISION | _abi.CERTIFY_CONTAINS)) != 0
        split = lambda m: dict(clear=int((fl[m] == 0).sum()), collision=int(hit[m].sum()),  # noqa: E731
                               undecided=int((~hit[m] & (fl[m] != 0)).sum()))
        r.update(evals_mean=float(ev.mean()), evals_max=int(ev.max()), verify_samples=(a.N * 8 + 1) * 16,
                 budget_share=float(((fl & _abi.CERTIFY_BUDGET) != 0).mean()), verdicts=split(np.ones(a.B, bool)),
                 verify_collision_free=split(vok),
                 width_max_no_budget=float((c["upper"] - c["lower"]).cpu().numpy()[(fl & _abi.CERTIFY_BUDGET) == 0].max()))
        out[name] = r
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
