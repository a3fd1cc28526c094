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
from ._lib import check, lib, require_gpu, stream_ptr
from .problem import Problem


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


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
    pc = problem.with_(sdf="analytic", obstacles=list(scene)).to_c()  # to_c() drops the scene of an mlp problem
    opt = _abi.verify_options(sub, edge_points, clearance_min, defect_tol, bound_tol)
    f64 = dict(dtype=torch.float64, device=device)
    X = torch.as_tensor(X, **f64).contiguous()
    U = torch.as_tensor(U, **f64).contiguous()
    if X.dim() != 3 or X.shape[1:] != (problem.N + 1, problem.nx):
        raise ValueError(f"X must be [B, {problem.N + 1}, {problem.nx}]")
    B = X.shape[0]
    if U.shape != (B, problem.N, problem.nu):
        raise ValueError(f"U must be [{B}, {problem.N}, {problem.nu}]")
    if x0 is not None:
        x0 = torch.as_tensor(x0, **f64).contiguous()
        xg = torch.as_tensor(xg, **f64).contiguous()
        if x0.shape != (B, problem.nx) or xg.shape != x0.shape:
            raise ValueError(f"x0/xg must be [{B}, {problem.nx}]")
    out = {k: torch.empty(B, **f64) for k in ("clearance", "defect", "ubound", "boundary")}
    out["where"] = torch.empty(B, dtype=torch.int32, device=device)
    out["flags"] = torch.empty(B, dtype=torch.int32, device=device)
    check(lib().nlot_verify_batch(C.byref(pc), C.byref(opt), _ptr(X), _ptr(U), _ptr(x0), _ptr(xg),
                                  _ptr(out["clearance"]), _ptr(out["where"]), _ptr(out["defect"]), _ptr(out["ubound"]),
                                  _ptr(out["boundary"]), _ptr(out["flags"]), B, stream_ptr()), "nlot_verify_batch")
    out["ok"] = out["flags"] == 0
    return {k: out[k] for k in ("clearance", "where", "defect", "ubound", "boundary", "flags", "ok")}
