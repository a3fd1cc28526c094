"""Time-varying LQR gains about a plan and the closed-loop tracking rollout (nlot_tvlqr_batch, nlot_track_batch,
csrc/nlot_track.hip).

`rollout_batch` feeds the returned controls to the continuous dynamics open loop.  Nobody executes a plan that way:
`tvlqr_batch` gives the finite-horizon discrete LQR gains `K_k` about each plan (a backward Riccati sweep on the
linearisation of one RK4 step at the knots), and `track_batch` is `rollout_batch`'s measurement with the loop closed,
`u_k = clamp(U_k - K_k (x(t_k) - X_k))`, from an optional start offset: deviation, goal error, clearance in the exact
scene and how often the feedback runs into the control bounds (the definitions and what the closed
loop does not prove: the controller is sampled at the knots only, it is LQR about an Euler plan linearised with the
RK4 map, no angle is wrapped, and the clearance is sampled).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _abi
from ._lib import check, lib, plan_tensors, ptr, require_gpu, scene_problem, stream_ptr
from .problem import Problem


def tvlqr_batch(problem: Problem, X, U, q=1.0, r=1.0, qf=1.0, device="cuda"):
    """The TVLQR gains about B plans (X [B, N+1, nx], U [B, N, nu], what solve_batch returns) of `problem`.

    q, qf (state weights at knots 0..N-1 and at knot N) and r (control weight) are the diagonals of Q, Qf, R: scalars
    or nx / nu values.  Returns (K [B, N, nu, nx], P0 [B, nx, nx], status [B] int32): status is 0 or
    _abi.TVLQR_NONFINITE / TVLQR_DIVERGED, both of which give K = 0 (the open loop) and P0 = NaN."""
    require_gpu()
    pc = scene_problem(problem, obstacles=[])  # the gains do not see the scene
    opt = _abi.tvlqr_options(q, r, qf, nx=problem.nx, nu=problem.nu)
    f64 = dict(dtype=torch.float64, device=device)
    X, U, B = plan_tensors(problem, X, U, device)
    K = torch.empty(B, problem.N, problem.nu, problem.nx, **f64)
    P0 = torch.empty(B, problem.nx, problem.nx, **f64)
    status = torch.empty(B, dtype=torch.int32, device=device)
    check(lib().nlot_tvlqr_batch(C.byref(pc), C.byref(opt), ptr(X), ptr(U), ptr(K), ptr(P0), ptr(status), B,
                                 stream_ptr()), "nlot_tvlqr_batch")
    return K, P0, status


def track_batch(problem: Problem, X, U, K=None, dx0=None, xg=None, obstacles=None, substeps=8, edge_points=3,
                clamp=True, clearance_min=0.0, deviation_tol=math.inf, goal_tol=math.inf, device="cuda"):
    """Roll B plans of `problem` with the loop closed: u_k = U_k - K_k (x(t_k) - X_k), clamped to the problem's
    control bounds unless clamp=False, held over interval k.

    K [B, N, nu, nx] (tvlqr_batch's; None: the open loop), dx0 [B, nx] (the start offset from X[:, 0]; None: 0).
    `obstacles`, xg, substeps, edge_points and the thresholds are rollout_batch's.  Returns rollout_batch's dict plus
    U_applied [B, N, nu] (fp64) and saturated [B] (int32: the knots at which the clamp acted); flags carry
    _abi.TRACK_* bits and ok = (flags == 0)."""
    require_gpu()
    pc = scene_problem(problem, obstacles)  # without a scene: no clearance
    opt = _abi.track_options(substeps, edge_points, clamp, clearance_min, deviation_tol, goal_tol)
    f64 = dict(dtype=torch.float64, device=device)
    X, U, B, K, dx0, xg = plan_tensors(problem, X, U, device, ("K", K, (problem.N, problem.nu, problem.nx)),
                                       ("dx0", dx0, (problem.nx,)), ("xg", xg, (problem.nx,)))
    out = {k: torch.empty(B, **f64) for k in ("clearance", "deviation", "goal_error")}
    out["X_roll"] = torch.empty_like(X)
    out["U_applied"] = torch.empty_like(U)
    for k in ("where", "dev_where", "saturated", "flags"):
        out[k] = torch.empty(B, dtype=torch.int32, device=device)
    check(lib().nlot_track_batch(C.byref(pc), C.byref(opt), ptr(X), ptr(U), ptr(K), ptr(dx0), ptr(xg),
                                 ptr(out["X_roll"]), ptr(out["U_applied"]), ptr(out["clearance"]), ptr(out["where"]),
                                 ptr(out["deviation"]), ptr(out["dev_where"]), ptr(out["goal_error"]),
                                 ptr(out["saturated"]), ptr(out["flags"]), B, stream_ptr()), "nlot_track_batch")
    out["ok"] = out["flags"] == 0
    return {k: out[k] for k in ("X_roll", "U_applied", "clearance", "where", "deviation", "dev_where", "goal_error",
                                "saturated", "flags", "ok")}
