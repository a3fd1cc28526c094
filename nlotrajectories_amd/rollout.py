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
from ._lib import check, lib, require_gpu, stream_ptr
from .problem import Problem


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def rollout_batch(problem: Problem, X, U, xg=None, obstacles=None, substeps=8, edge_points=3, clearance_min=0.0,
                  deviation_tol=math.inf, goal_tol=math.inf, device="cuda"):
    """Roll the controls of B trajectories (X [B, N+1, nx], U [B, N, nu], what solve_batch returns) of `problem`.

    `obstacles` overrides problem.obstacles (a learned-SDF problem such as METRIC_PROBLEM carries no scene: pass the
    one its net was trained on); without any scene the clearance is +inf and where is -1.  xg [B, nx]: the goal, else
    the plan's last knot.  Returns a dict of device tensors: X_roll [B, N+1, nx] (the rolled knots) and, [B] each,
    clearance, where (pose index of the minimum; where // substeps is the knot), deviation, dev_where (knot),
    goal_error (fp64), flags (int32, _abi.ROLLOUT_* bits) and ok = (flags == 0)."""
    scene = problem.obstacles if obstacles is None else obstacles
    require_gpu()
    if scene:
        pc = problem.with_(sdf="analytic", obstacles=list(scene)).to_c()  # to_c() drops the scene of an mlp problem
    else:
        pc = problem.with_(sdf="mlp", obstacles=[]).to_c()  # n_obs == 0: rolled for deviation and goal error only
    opt = _abi.rollout_options(substeps, edge_points, clearance_min, deviation_tol, goal_tol)
    f64 = dict(dtype=torch.float64, device=device)
    X = torch.as_tensor(X, **f64).contiguous()
    U = torch.as_tensor(U, **f64).contiguous()
    if X.dim() != 3 or X.shape[1:] != (problem.N + 1, problem.nx):
        raise ValueError(f"X must be [B, {problem.N + 1}, {problem.nx}]")
    B = X.shape[0]
    if U.shape != (B, problem.N, problem.nu):
        raise ValueError(f"U must be [{B}, {problem.N}, {problem.nu}]")
    if xg is not None:
        xg = torch.as_tensor(xg, **f64).contiguous()
        if xg.shape != (B, problem.nx):
            raise ValueError(f"xg must be [{B}, {problem.nx}]")
    out = {k: torch.empty(B, **f64) for k in ("clearance", "deviation", "goal_error")}
    out["X_roll"] = torch.empty_like(X)
    for k in ("where", "dev_where", "flags"):
        out[k] = torch.empty(B, dtype=torch.int32, device=device)
    check(lib().nlot_rollout_batch(C.byref(pc), C.byref(opt), _ptr(X), _ptr(U), _ptr(xg), _ptr(out["X_roll"]),
                                   _ptr(out["clearance"]), _ptr(out["where"]), _ptr(out["deviation"]),
                                   _ptr(out["dev_where"]), _ptr(out["goal_error"]), _ptr(out["flags"]), B, stream_ptr()),
          "nlot_rollout_batch")
    out["ok"] = out["flags"] == 0
    return {k: out[k] for k in ("X_roll", "clearance", "where", "deviation", "dev_where", "goal_error", "flags", "ok")}
