"""Verify dumped solver outputs against an exact scene (nlot_verify_batch).

    python scripts/verify_outputs.py DIR --scene b2|b3|b4|b5|b6|<config.yaml> [--workload metric|stress]

DIR holds the X.npy, U.npy and status.npy that `bench.py --dump-outputs DIR` writes.  The problem (body, dynamics,
bounds, N) is the workload's; the scene is a restated benchmark's (problem.BENCHMARKS) or a YAML config's obstacles:
the metric and stress workloads solve against a learned SDF and carry no scene of their own, so the scene is the
caller's statement of where the trajectories are meant to drive.  Prints one JSON line: the share of the solved
instances with flags == 0, the shares per flag, and the clearance quantiles of the solved instances.

--rollout [--rollout-substeps 8] also rolls the dumped controls through the continuous dynamics (nlot_rollout_batch)
and adds one key `rollout`: the shares per rollout flag, the quantiles of the deviation from the plan, of the goal
error (against the plan's last knot: the dump carries no goals) and of the rolled clearance over the solved instances,
and how many of the instances verify_batch passes the rollout flags.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scene_obstacles(name):
    from nlotrajectories_amd.problem import BENCHMARKS

    if name in BENCHMARKS:
        return BENCHMARKS[name]["problem"].obstacles
    from nlotrajectories_amd.config import Config

    return Config.load(name).obstacle_dicts()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--scene", required=True, help="b2|b3|b4|b5|b6 (problem.BENCHMARKS) or a benchmark YAML")
    ap.add_argument("--workload", choices=["metric", "stress"], default="metric", help="the bench.py workload of the dump")
    ap.add_argument("--sub", type=int, default=8)
    ap.add_argument("--edge-points", type=int, default=3)
    ap.add_argument("--rollout", action="store_true", help="also roll the controls through the dynamics (rollout_batch)")
    ap.add_argument("--rollout-substeps", type=int, default=8)
    a = ap.parse_args(argv)

    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.problem import METRIC_PROBLEM, STRESS_PROBLEM
    from nlotrajectories_amd.verify import verify_batch

    prob = METRIC_PROBLEM if a.workload == "metric" else STRESS_PROBLEM
    X, U, status = (np.load(os.path.join(a.dir, k + ".npy")) for k in ("X", "U", "status"))
    if X.shape[1:] != (prob.N + 1, prob.nx):
        raise SystemExit(f"X.npy is {X.shape}: not a dump of the {a.workload} workload (N = {prob.N}, nx = {prob.nx})")
    v = verify_batch(prob, X, U, obstacles=scene_obstacles(a.scene), sub=a.sub, edge_points=a.edge_points)
    solved = status.astype(np.int64) == _abi.NLOT_SOLVED
    flags = v["flags"].cpu().numpy()[solved]
    clearance = v["clearance"].cpu().numpy()[solved]
    n = int(solved.sum())
    out = dict(scene=a.scene, workload=a.workload, sub=a.sub, edge_points=a.edge_points, instances=int(len(status)),
               solved=n, ok_share=float((flags == 0).mean()) if n else None,
               flag_shares={name: float(((flags & bit) != 0).mean()) if n else None
                            for bit, name in _abi.VERIFY_FLAG_NAMES.items()},
               clearance_quantiles={str(q): float(np.quantile(clearance, q)) if n else None
                                    for q in (0.0, 0.01, 0.1, 0.5, 0.9, 1.0)},
               max_defect=float(v["defect"].cpu().numpy()[solved].max()) if n else None)
    if a.rollout:
        from nlotrajectories_amd.rollout import rollout_batch

        r = rollout_batch(prob, X, U, obstacles=scene_obstacles(a.scene), substeps=a.rollout_substeps,
                          edge_points=a.edge_points)
        rflags = r["flags"].cpu().numpy()[solved]
        qs = (0.0, 0.01, 0.1, 0.5, 0.9, 1.0)
        quant = lambda k: {str(q): float(np.nanquantile(r[k].cpu().numpy()[solved], q)) if n else None for q in qs}  # noqa: E731
        out["rollout"] = dict(substeps=a.rollout_substeps,
                              flag_shares={name: float(((rflags & bit) != 0).mean()) if n else None
                                           for bit, name in _abi.ROLLOUT_FLAG_NAMES.items()},
                              deviation_quantiles=quant("deviation"), goal_error_quantiles=quant("goal_error"),
                              clearance_quantiles=quant("clearance"), verify_ok=int((flags == 0).sum()),
                              verify_ok_rollout_flagged=int(((flags == 0) & (rflags != 0)).sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
