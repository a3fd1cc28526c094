"""The analytic scene and the SDF-quality metrics on the device (nlot_scene_sdf_eval, nlot_sdf_metrics,
csrc/nlot_scene.hip).

`scene.py` restates the scene's formulas in numpy for the host; these evaluate the functions the solver
(approximated SDF) and the RRT / verifier / rollout (exact SDF) themselves use, on the GPU, and compute the
reference's `compute_metrics` (run_benchmark.py:34-46, core/metrics.py) there.  Everything is opt-in: the CLI and
the trainer keep the host path by default (`--metrics-device gpu`, `NNObstacleTrainer(sdf_device="gpu")`).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _abi
from ._lib import check, lib, ptr, require_gpu, scene_problem, stream_ptr
from .problem import Problem

KINDS = {"exact": _abi.SCENE_EXACT, "approx": _abi.SCENE_APPROX}
# k_nearest's LDS tile in points (NLOT_NEAREST_TILE of csrc/nlot_scene.hip): the band size at which it takes a second tile
NEAREST_TILE = 1024


def _scene_problem(obstacles_or_problem):
    """An NlotProblem that carries the scene: the given Problem's (verify_batch's), or a dot body around bare
    obstacle dicts (only the scene fields are read)."""
    if isinstance(obstacles_or_problem, Problem):
        if not obstacles_or_problem.obstacles:
            raise ValueError("scene_sdf_eval: the problem has no obstacles")
        return scene_problem(obstacles_or_problem)
    scene = list(obstacles_or_problem)
    if not scene:
        raise ValueError("scene_sdf_eval: no obstacles")
    return Problem(dynamics="point_2nd", shape="dot", sdf="analytic", obstacles=scene).to_c()


def _points(pts):
    if not torch.is_tensor(pts):
        pts = np.asarray(pts, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 1:
        raise ValueError(f"pts must be [P, 2] with P >= 1, not {tuple(pts.shape)}")
    return pts


def _device(a, **kw):
    """A contiguous device tensor of `a` (a numpy array is copied: it may be read-only)."""
    return (a.to(**kw) if torch.is_tensor(a) else torch.tensor(np.asarray(a), **kw)).contiguous()


def scene_sdf_eval(obstacles_or_problem, pts, kind="exact", derivatives=False, device="cuda"):
    """The scene's SDF at pts [P, 2]: kind "exact" (MultiObstacle.sdf) or "approx" (MultiObstacle.approximated_sdf,
    the solver's).  Returns the fp64 device tensor val [P], or with derivatives=True ("approx" only) the tuple
    (val [P], grad [P, 2], hess [P, 3] = xx, xy, yy)."""
    if kind not in KINDS:
        raise ValueError(f"kind must be 'exact' or 'approx', not {kind!r}")
    if derivatives and kind == "exact":
        raise ValueError("derivatives need kind='approx': the exact SDF has no derivative code")
    pts = _points(pts)
    pc = _scene_problem(obstacles_or_problem)
    require_gpu()
    f64 = dict(dtype=torch.float64, device=device)
    pts = _device(pts, **f64)
    P = pts.shape[0]
    val = torch.empty(P, **f64)
    grad = torch.empty(P, 2, **f64) if derivatives else None
    hess = torch.empty(P, 3, **f64) if derivatives else None
    check(lib().nlot_scene_sdf_eval(C.byref(pc), KINDS[kind], ptr(pts), P, ptr(val), ptr(grad), ptr(hess),
                                    stream_ptr()), "nlot_scene_sdf_eval")
    return (val, grad, hess) if derivatives else val


def sdf_metrics(pts, target, pred, threshold=0.0, eps=1e-2, device="cuda"):
    """core/metrics.py on the device: pts [P, 2], target [P], pred [P] (any shape with P entries).  Returns a dict:
    mse, iou, hausdorff, chamfer, surface_loss (None where the reference returns None: an empty surface band) and the
    counts n_target_surface, n_pred_surface, n_points.  A NaN entry is in no set and makes mse NaN."""
    pts = _points(pts)
    P = pts.shape[0]
    for name, a in (("target", target), ("pred", pred)):
        n = a.numel() if torch.is_tensor(a) else np.size(a)
        if n != P:
            raise ValueError(f"{name} must have {P} entries (one per point), not {n}")
    if not (eps > 0 and math.isfinite(eps)) or not math.isfinite(threshold):
        raise ValueError("eps must be finite and > 0, threshold finite")
    require_gpu()
    f64 = dict(dtype=torch.float64, device=device)
    pts, target, pred = _device(pts, **f64), _device(target, **f64).reshape(-1), _device(pred, **f64).reshape(-1)
    out = torch.empty(C.sizeof(_abi.NlotSdfMetrics), dtype=torch.uint8, device=pts.device)
    opt = _abi.sdf_metrics_options(threshold, eps)
    check(lib().nlot_sdf_metrics(C.byref(opt), ptr(pts), ptr(target), ptr(pred), P, ptr(out), stream_ptr()),
          "nlot_sdf_metrics")
    m = _abi.NlotSdfMetrics.from_buffer_copy(out.cpu().numpy().tobytes())
    r = {k: getattr(m, k) for k, _ in m._fields_}
    for k in ("hausdorff", "chamfer", "surface_loss"):
        if math.isnan(r[k]):
            r[k] = None
    return r


def scene_metrics(obstacles, mlp=None, n=1000, lo=-1.0, hi=2.0, threshold=0.0, eps=1e-2):
    """run_benchmark.py:35-46 compute_metrics on the device: the approximated SDF (the net `mlp`, a DeviceMlp, or
    the scene's own approximated SDF) against the exact one on an n x n grid of [lo, hi]^2.  Returns (mse, iou,
    hausdorff, chamfer, surface_loss), what cli._metrics returns.  The grid is numpy's, as on the host path."""
    x = np.linspace(lo, hi, n)
    X, Y = np.meshgrid(x, x)
    require_gpu()
    pts = torch.as_tensor(np.stack([X.ravel(), Y.ravel()], 1), device="cuda")
    exact = scene_sdf_eval(obstacles, pts, "exact")
    if mlp is not None:
        from .ops import sdf_mlp_eval

        approx = sdf_mlp_eval(mlp, pts.to(torch.float32), derivatives=False)[0].to(torch.float64)
    else:
        approx = scene_sdf_eval(obstacles, pts, "approx")
    r = sdf_metrics(pts, exact, approx, threshold=threshold, eps=eps)
    return r["mse"], r["iou"], r["hausdorff"], r["chamfer"], r["surface_loss"]
