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

--track [--track-substeps 8 --track-q 1 --track-r 1 --track-qf 1] (each weight one value, or one per component) also computes the TVLQR gains about every dumped plan
(nlot_tvlqr_batch) and rolls it with the loop closed (nlot_track_batch); it adds one key `track` with the same fields
as `rollout` for the closed loop, the share of the solved instances that saturate, the quantiles of the saturated-knot
count, and the gains' status counts.
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
    ap.add_argument("--track", action="store_true", help="also track the plans with their TVLQR gains (track_batch)")
    ap.add_argument("--track-substeps", type=int, default=8)
    ap.add_argument("--track-q", type=float, nargs="+", default=[1.0], help="one value, or one per state component")
    ap.add_argument("--track-r", type=float, nargs="+", default=[1.0], help="one value, or one per control")
    ap.add_argument("--track-qf", type=float, nargs="+", default=[1.0], help="one value, or one per state component")
    a = ap.parse_args(argv)
    for k in ("track_q", "track_r", "track_qf"):  # one value: a scalar for every component
        v = getattr(a, k)
        setattr(a, k, v[0] if len(v) == 1 else v)

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
    if a.track:
        from nlotrajectories_amd.tracking import track_batch, tvlqr_batch

        K, _, kst = tvlqr_batch(prob, X, U, q=a.track_q, r=a.track_r, qf=a.track_qf)
        t = track_batch(prob, X, U, K=K, obstacles=scene_obstacles(a.scene), substeps=a.track_substeps,
                        edge_points=a.edge_points)
        tflags, kst = t["flags"].cpu().numpy()[solved], kst.cpu().numpy()[solved]
        sat = t["saturated"].cpu().numpy()[solved]
        qs = (0.0, 0.01, 0.1, 0.5, 0.9, 1.0)
        quant = lambda k: {str(q): float(np.nanquantile(t[k].cpu().numpy()[solved], q)) if n else None for q in qs}  # noqa: E731
        hits = _abi.TRACK_COLLISION | _abi.TRACK_CONTAINS
        out["track"] = dict(substeps=a.track_substeps, q=a.track_q, r=a.track_r, qf=a.track_qf,
                            gains_nonfinite=int((kst == _abi.TVLQR_NONFINITE).sum()),
                            gains_diverged=int((kst == _abi.TVLQR_DIVERGED).sum()),
                            flag_shares={name: float(((tflags & bit) != 0).mean()) if n else None
                                         for bit, name in _abi.TRACK_FLAG_NAMES.items()},
                            deviation_quantiles=quant("deviation"), goal_error_quantiles=quant("goal_error"),
                            clearance_quantiles=quant("clearance"),
                            saturated_share=float((sat > 0).mean()) if n else None,
                            saturated_knots_quantiles={str(q): float(np.quantile(sat, q)) if n else None for q in qs},
                            verify_ok=int((flags == 0).sum()),
                            verify_ok_track_collides=int(((flags == 0) & ((tflags & hits) != 0)).sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
