"""Batched trajectory verification against the exact scene (nlot_verify_batch, csrc/nlot_verify.hip).

`NLOT_SOLVED` says the interior-point method converged on the NLP.  `verify_batch` measures what the returned
trajectory does in the scene the user drives in: its clearance from the scene's exact SDF over poses sampled
between the knots and footprint points sampled along the edges, whether an obstacle sits inside the footprint,
the dynamics defect, the control-bound violation and the boundary residual (the definitions and
what the check does not prove).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _abi
from ._lib import check, lib, plan_tensors, ptr, require_gpu, scene_problem, stream_ptr
from .problem import Problem


def verify_batch(problem: Problem, X, U, x0=None, xg=None, obstacles=None, sub=8, edge_points=3, clearance_min=0.0,
                 defect_tol=1e-4, bound_tol=1e-4, device="cuda"):
    """Verify B trajectories (X [B, N+1, nx], U [B, N, nu], what solve_batch returns) of `problem`.

    `obstacles` overrides problem.obstacles (a learned-SDF problem such as METRIC_PROBLEM carries no scene: pass the
    one its net was trained on).  x0, xg [B, nx]: both or neither; without them `boundary` is 0.  Returns a dict of
    device tensors [B]: clearance, where (pose index of the minimum; where // sub is the knot), defect, ubound,
    boundary (fp64), flags (int32, _abi.VERIFY_* bits) and ok = (flags == 0)."""
    scene = problem.obstacles if obstacles is None else obstacles
    if not scene:
        raise ValueError("verify_batch measures against the scene's exact SDF: the problem has no obstacles, pass obstacles=")
    if (x0 is None) != (xg is None):
        raise ValueError("x0 and xg must both be given or both be None")
    require_gpu()
    pc = scene_problem(problem, scene)
    opt = _abi.verify_options(sub, edge_points, clearance_min, defect_tol, bound_tol)
    f64 = dict(dtype=torch.float64, device=device)
    X, U, B, x0, xg = plan_tensors(problem, X, U, device, ("x0/xg", x0, (problem.nx,)), ("x0/xg", xg, (problem.nx,)))
    out = {k: torch.empty(B, **f64) for k in ("clearance", "defect", "ubound", "boundary")}
    out["where"] = torch.empty(B, dtype=torch.int32, device=device)
    out["flags"] = torch.empty(B, dtype=torch.int32, device=device)
    check(lib().nlot_verify_batch(C.byref(pc), C.byref(opt), ptr(X), ptr(U), ptr(x0), ptr(xg),
                                  ptr(out["clearance"]), ptr(out["where"]), ptr(out["defect"]), ptr(out["ubound"]),
                                  ptr(out["boundary"]), ptr(out["flags"]), B, stream_ptr()), "nlot_verify_batch")
    out["ok"] = out["flags"] == 0
    return {k: out[k] for k in ("clearance", "where", "defect", "ubound", "boundary", "flags", "ok")}
