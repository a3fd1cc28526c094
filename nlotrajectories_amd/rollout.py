"""Batched forward rollout of returned controls through the dynamics (nlot_rollout_batch, csrc/nlot_rollout.hip).

What a user executes is `U`.  `verify_batch` measures the plan `X`; the continuous-time robot fed `U` under zero-order
hold does not follow an Euler plan.  `rollout_batch` integrates the problem's continuous dynamics from `X[:, 0]` with
sub-stepped classical RK4 and measures the rolled motion: how far it departs from the plan, how far from the goal it
ends, and the clearance its footprint keeps in the exact scene (the definitions and what the rollout
does not prove: it is RK4 at h = dt / substeps, zero-order hold, open loop, and it samples poses).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _abi
from ._lib import check, lib, plan_tensors, ptr, require_gpu, scene_problem, stream_ptr
from .problem import Problem


def rollout_batch(problem: Problem, X, U, xg=None, obstacles=None, substeps=8, edge_points=3, clearance_min=0.0,
                  deviation_tol=math.inf, goal_tol=math.inf, device="cuda"):
    """Roll the controls of B trajectories (X [B, N+1, nx], U [B, N, nu], what solve_batch returns) of `problem`.

    `obstacles` overrides problem.obstacles (a learned-SDF problem such as METRIC_PROBLEM carries no scene: pass the
    one its net was trained on); without any scene the clearance is +inf and where is -1.  xg [B, nx]: the goal, else
    the plan's last knot.  Returns a dict of device tensors: X_roll [B, N+1, nx] (the rolled knots) and, [B] each,
    clearance, where (pose index of the minimum; where // substeps is the knot), deviation, dev_where (knot),
    goal_error (fp64), flags (int32, _abi.ROLLOUT_* bits) and ok = (flags == 0)."""
    require_gpu()
    pc = scene_problem(problem, obstacles)  # without a scene: rolled for deviation and goal error only
    opt = _abi.rollout_options(substeps, edge_points, clearance_min, deviation_tol, goal_tol)
    f64 = dict(dtype=torch.float64, device=device)
    X, U, B, xg = plan_tensors(problem, X, U, device, ("xg", xg, (problem.nx,)))
    out = {k: torch.empty(B, **f64) for k in ("clearance", "deviation", "goal_error")}
    out["X_roll"] = torch.empty_like(X)
    for k in ("where", "dev_where", "flags"):
        out[k] = torch.empty(B, dtype=torch.int32, device=device)
    check(lib().nlot_rollout_batch(C.byref(pc), C.byref(opt), ptr(X), ptr(U), ptr(xg), ptr(out["X_roll"]),
                                   ptr(out["clearance"]), ptr(out["where"]), ptr(out["deviation"]),
                                   ptr(out["dev_where"]), ptr(out["goal_error"]), ptr(out["flags"]), B, stream_ptr()),
          "nlot_rollout_batch")
    out["ok"] = out["flags"] == 0
    return {k: out[k] for k in ("X_roll", "clearance", "where", "deviation", "dev_where", "goal_error", "flags", "ok")}
