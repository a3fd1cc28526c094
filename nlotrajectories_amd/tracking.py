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
from ._lib import check, lib, require_gpu, stream_ptr
from .problem import Problem


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _plan(problem, X, U, f64):
    X = torch.as_tensor(X, **f64).contiguous()
    U = torch.as_tensor(U, **f64).contiguous()
    if X.dim() != 3 or X.shape[1:] != (problem.N + 1, problem.nx):
        raise ValueError(f"X must be [B, {problem.N + 1}, {problem.nx}]")
    B = X.shape[0]
    if U.shape != (B, problem.N, problem.nu):
        raise ValueError(f"U must be [{B}, {problem.N}, {problem.nu}]")
    return X, U, B


def tvlqr_batch(problem: Problem, X, U, q=1.0, r=1.0, qf=1.0, device="cuda"):
    """The TVLQR gains about B plans (X [B, N+1, nx], U [B, N, nu], what solve_batch returns) of `problem`.

    q, qf (state weights at knots 0..N-1 and at knot N) and r (control weight) are the diagonals of Q, Qf, R: scalars
    or nx / nu values.  Returns (K [B, N, nu, nx], P0 [B, nx, nx], status [B] int32): status is 0 or
    _abi.TVLQR_NONFINITE / TVLQR_DIVERGED, both of which give K = 0 (the open loop) and P0 = NaN."""
    require_gpu()
    pc = problem.with_(sdf="mlp", obstacles=[]).to_c()  # the gains do not see the scene
    opt = _abi.tvlqr_options(q, r, qf, nx=problem.nx, nu=problem.nu)
    f64 = dict(dtype=torch.float64, device=device)
    X, U, B = _plan(problem, X, U, f64)
    K = torch.empty(B, problem.N, problem.nu, problem.nx, **f64)
    P0 = torch.empty(B, problem.nx, problem.nx, **f64)
    status = torch.empty(B, dtype=torch.int32, device=device)
    check(lib().nlot_tvlqr_batch(C.byref(pc), C.byref(opt), _ptr(X), _ptr(U), _ptr(K), _ptr(P0), _ptr(status), B,
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
    scene = problem.obstacles if obstacles is None else obstacles
    require_gpu()
    if scene:
        pc = problem.with_(sdf="analytic", obstacles=list(scene)).to_c()  # to_c() drops the scene of an mlp problem
    else:
        pc = problem.with_(sdf="mlp", obstacles=[]).to_c()  # n_obs == 0: no clearance
    opt = _abi.track_options(substeps, edge_points, clamp, clearance_min, deviation_tol, goal_tol)
    f64 = dict(dtype=torch.float64, device=device)
    X, U, B = _plan(problem, X, U, f64)
    if K is not None:
        K = torch.as_tensor(K, **f64).contiguous()
        if K.shape != (B, problem.N, problem.nu, problem.nx):
            raise ValueError(f"K must be [{B}, {problem.N}, {problem.nu}, {problem.nx}]")
    if dx0 is not None:
        dx0 = torch.as_tensor(dx0, **f64).contiguous()
        if dx0.shape != (B, problem.nx):
            raise ValueError(f"dx0 must be [{B}, {problem.nx}]")
    if xg is not None:
        xg = torch.as_tensor(xg, **f64).contiguous()
        if xg.shape != (B, problem.nx):
            raise ValueError(f"xg must be [{B}, {problem.nx}]")
    out = {k: torch.empty(B, **f64) for k in ("clearance", "deviation", "goal_error")}
    out["X_roll"] = torch.empty_like(X)
    out["U_applied"] = torch.empty_like(U)
    for k in ("where", "dev_where", "saturated", "flags"):
        out[k] = torch.empty(B, dtype=torch.int32, device=device)
    check(lib().nlot_track_batch(C.byref(pc), C.byref(opt), _ptr(X), _ptr(U), _ptr(K), _ptr(dx0), _ptr(xg),
                                 _ptr(out["X_roll"]), _ptr(out["U_applied"]), _ptr(out["clearance"]), _ptr(out["where"]),
                                 _ptr(out["deviation"]), _ptr(out["dev_where"]), _ptr(out["goal_error"]),
                                 _ptr(out["saturated"]), _ptr(out["flags"]), B, stream_ptr()), "nlot_track_batch")
    out["ok"] = out["flags"] == 0
    return {k: out[k] for k in ("X_roll", "U_applied", "clearance", "where", "deviation", "dev_where", "goal_error",
                                "saturated", "flags", "ok")}
