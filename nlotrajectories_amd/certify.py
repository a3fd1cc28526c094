"""Certified clearance of plans by Lipschitz branch-and-bound (nlot_certify_batch, csrc/nlot_certify.hip).

`verify_batch` samples the interpolated motion, so its clearance is an upper bound of the true one and a positive
value proves nothing.  `certify_batch` brackets the true minimum of the scene's exact SDF over every instant of the
interpolated motion and every point of the footprint's boundary: `lower <= min <= upper`, refined where the clearance
is small until the bracket is `tol` wide (the bound, the search, and what it does not cover).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _abi
from ._lib import check, lib, ptr, require_gpu, scene_problem, stream_ptr
from .problem import Problem


def certify_batch(problem: Problem, X, obstacles=None, tol=1e-3, clearance_min=0.0, decide=False, max_evals=0,
                  device="cuda"):
    """Bracket the clearance of B plans X [B, N+1, nx] of `problem` (what solve_batch returns).

    `obstacles` overrides problem.obstacles, as in verify_batch.  decide=True only decides the verdict against
    clearance_min instead of tightening the bracket to tol; max_evals caps the refinement's SDF evaluations per plan
    (0: the library's default).  Returns a dict of device tensors [B]: lower, upper, tau (fp64), where, evals, flags
    (int32, _abi.CERTIFY_* bits) and clear = (flags == 0): proven collision-free."""
    scene = problem.obstacles if obstacles is None else obstacles
    if not scene:
        raise ValueError("certify_batch measures against the scene's exact SDF: the problem has no obstacles, pass obstacles=")
    require_gpu()
    pc = scene_problem(problem, scene)
    opt = _abi.certify_options(tol, clearance_min, decide, max_evals)
    X = torch.as_tensor(X, dtype=torch.float64, device=device).contiguous()
    if X.dim() != 3 or X.shape[1:] != (problem.N + 1, problem.nx):
        raise ValueError(f"X must be [B, {problem.N + 1}, {problem.nx}]")
    B = X.shape[0]
    out = {k: torch.empty(B, dtype=torch.float64, device=device) for k in ("lower", "upper", "tau")}
    out.update({k: torch.empty(B, dtype=torch.int32, device=device) for k in ("where", "evals", "flags")})
    check(lib().nlot_certify_batch(C.byref(pc), C.byref(opt), ptr(X), ptr(out["lower"]), ptr(out["upper"]),
                                   ptr(out["where"]), ptr(out["tau"]), ptr(out["evals"]), ptr(out["flags"]), B,
                                   stream_ptr()), "nlot_certify_batch")
    out["clear"] = out["flags"] == 0
    return {k: out[k] for k in ("lower", "upper", "where", "tau", "evals", "flags", "clear")}
