"""Loader for libnlot.so (the HIP kernels behind the C ABI of include/nlot.h).

There is no CPU fallback: every compute entry point of this package goes through this library, and
importing a compute function without the built library or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from . import _abi

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# NLOT_LIB selects an alternative in-tree build (e.g. the phase-timer build libnlot_prof.so)
LIB_PATH = os.path.join(PKG_DIR, os.environ.get("NLOT_LIB", "libnlot.so"))
CSRC = os.path.join(PKG_DIR, "csrc")

# symbols include/nlot.h declares (checked by tests/test_abi.py)
EXPORTED = [
    "nlot_abi_version", "nlot_last_error", "nlot_default_options", "nlot_mlp_create", "nlot_mlp_create_ex", "nlot_mlp_destroy",
    "nlot_sdf_mlp_eval", "nlot_solve_workspace_size", "nlot_solve_workspace_size_slots", "nlot_solve_batch", "nlot_set_timing",
    "nlot_last_stats", "nlot_casadi_bind", "nn_sdf_n_in", "nn_sdf_n_out", "nn_sdf_sparsity_in",
    "nn_sdf_sparsity_out", "nn_sdf", "jac_nn_sdf_n_in", "jac_nn_sdf_n_out", "jac_nn_sdf",
    "adj1_nn_sdf_n_in", "adj1_nn_sdf_n_out", "adj1_nn_sdf", "jac_adj1_nn_sdf_n_in",
    "jac_adj1_nn_sdf_n_out", "jac_adj1_nn_sdf", "nlot_rrt_workspace_size", "nlot_rrt_init",
    "nlot_default_verify_options", "nlot_verify_batch", "nlot_default_rollout_options", "nlot_rollout_batch",
    "nlot_scene_sdf_eval", "nlot_default_sdf_metrics_options", "nlot_sdf_metrics",
    "nlot_default_tvlqr_options", "nlot_tvlqr_batch", "nlot_default_track_options", "nlot_track_batch",
]


class NlotError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile libnlot.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j8"]
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=True)
    subprocess.run(args, check=True)
    return LIB_PATH


_lib = None


def lib():
    """The loaded library with argtypes set.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NlotError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(no CPU fallback exists)")
    L = C.CDLL(LIB_PATH)
    vp, dp, fp, i32p = C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p
    L.nlot_abi_version.restype = C.c_int32
    L.nlot_last_error.restype = C.c_char_p
    L.nlot_default_options.argtypes = [C.POINTER(_abi.NlotSolverOptions)]
    L.nlot_mlp_create.argtypes = [C.POINTER(_abi.NlotMlpDesc)]
    L.nlot_mlp_create.restype = vp
    L.nlot_mlp_create_ex.argtypes = [C.POINTER(_abi.NlotMlpDesc), C.c_int32]
    L.nlot_mlp_create_ex.restype = vp
    L.nlot_mlp_destroy.argtypes = [vp]
    L.nlot_sdf_mlp_eval.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    L.nlot_sdf_mlp_eval.restype = C.c_int32
    L.nlot_solve_workspace_size.argtypes = [C.POINTER(_abi.NlotProblem), C.c_int64]
    L.nlot_solve_workspace_size.restype = C.c_size_t
    L.nlot_solve_workspace_size_slots.argtypes = [C.POINTER(_abi.NlotProblem), C.c_int64, C.c_int32]
    L.nlot_solve_workspace_size_slots.restype = C.c_size_t
    L.nlot_solve_batch.argtypes = [C.POINTER(_abi.NlotProblem), C.POINTER(_abi.NlotSolverOptions), vp, vp, vp, vp,
                                   vp, vp, vp, vp, vp, vp, C.c_int64, vp, C.c_size_t, vp]
    L.nlot_solve_batch.restype = C.c_int32
    L.nlot_set_timing.argtypes = [C.c_int32]
    L.nlot_last_stats.argtypes = [C.POINTER(_abi.NlotSolveStats)]
    L.nlot_rrt_workspace_size.argtypes = [C.POINTER(_abi.NlotRrtOptions), C.c_int64]
    L.nlot_rrt_workspace_size.restype = C.c_size_t
    L.nlot_rrt_init.argtypes = [C.POINTER(_abi.NlotProblem), C.POINTER(_abi.NlotRrtOptions), vp, vp, vp, vp, C.c_int64,
                                vp, C.c_size_t, vp]
    L.nlot_rrt_init.restype = C.c_int32
    L.nlot_default_verify_options.argtypes = [C.POINTER(_abi.NlotVerifyOptions)]
    L.nlot_default_verify_options.restype = None
    L.nlot_verify_batch.argtypes = [C.POINTER(_abi.NlotProblem), C.POINTER(_abi.NlotVerifyOptions), vp, vp, vp, vp, vp,
                                    vp, vp, vp, vp, vp, C.c_int64, vp]
    L.nlot_verify_batch.restype = C.c_int32
    L.nlot_default_rollout_options.argtypes = [C.POINTER(_abi.NlotRolloutOptions)]
    L.nlot_default_rollout_options.restype = None
    L.nlot_rollout_batch.argtypes = [C.POINTER(_abi.NlotProblem), C.POINTER(_abi.NlotRolloutOptions), vp, vp, vp, vp, vp,
                                     vp, vp, vp, vp, vp, C.c_int64, vp]
    L.nlot_rollout_batch.restype = C.c_int32
    L.nlot_scene_sdf_eval.argtypes = [C.POINTER(_abi.NlotProblem), C.c_int32, vp, C.c_int64, vp, vp, vp, vp]
    L.nlot_scene_sdf_eval.restype = C.c_int32
    L.nlot_default_sdf_metrics_options.argtypes = [C.POINTER(_abi.NlotSdfMetricsOptions)]
    L.nlot_default_sdf_metrics_options.restype = None
    L.nlot_sdf_metrics.argtypes = [C.POINTER(_abi.NlotSdfMetricsOptions), vp, vp, vp, C.c_int64, vp, vp]
    L.nlot_sdf_metrics.restype = C.c_int32
    L.nlot_default_tvlqr_options.argtypes = [C.POINTER(_abi.NlotTvlqrOptions)]
    L.nlot_default_tvlqr_options.restype = None
    L.nlot_tvlqr_batch.argtypes = [C.POINTER(_abi.NlotProblem), C.POINTER(_abi.NlotTvlqrOptions), vp, vp, vp, vp, vp,
                                   C.c_int64, vp]
    L.nlot_tvlqr_batch.restype = C.c_int32
    L.nlot_default_track_options.argtypes = [C.POINTER(_abi.NlotTrackOptions)]
    L.nlot_default_track_options.restype = None
    L.nlot_track_batch.argtypes = [C.POINTER(_abi.NlotProblem), C.POINTER(_abi.NlotTrackOptions), vp, vp, vp, vp, vp,
                                   vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp]
    L.nlot_track_batch.restype = C.c_int32
    L.nlot_casadi_bind.argtypes = [vp]
    L.nlot_casadi_bind.restype = C.c_int32
    if L.nlot_abi_version() != 19:
        raise NlotError("libnlot.so ABI version mismatch")
    _lib = L
    return L


def check(rc: int, what: str):
    if rc != 0:
        raise NlotError(f"{what} failed ({rc}): {lib().nlot_last_error().decode()}")


def require_gpu():
    import torch

    if not torch.cuda.is_available():
        raise NlotError("nlotrajectories_amd needs a ROCm GPU (MI355X); no CPU fallback exists")


def stream_ptr(stream=None):
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def ptr(t):
    """The data pointer of tensor `t` as an argument of the library (None: NULL)."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def plan_tensors(problem, X, U, device, *extras):
    """B plans of `problem` as contiguous fp64 tensors on `device`: X [B, N+1, nx], U [B, N, nu] and the optional
    per-instance inputs `extras`, each (name, array or None, shape after B).  Returns (X, U, B, *extras), a None
    extra staying None; a wrong shape raises ValueError."""
    import torch

    f64 = dict(dtype=torch.float64, device=device)
    X = torch.as_tensor(X, **f64).contiguous()
    U = torch.as_tensor(U, **f64).contiguous()
    if X.dim() != 3 or X.shape[1:] != (problem.N + 1, problem.nx):
        raise ValueError(f"X must be [B, {problem.N + 1}, {problem.nx}]")
    B = X.shape[0]
    if U.shape != (B, problem.N, problem.nu):
        raise ValueError(f"U must be [{B}, {problem.N}, {problem.nu}]")
    out = []
    for name, t, shape in extras:
        if t is not None:
            t = torch.as_tensor(t, **f64).contiguous()
            if t.shape != (B, *shape):
                raise ValueError(f"{name} must be [{', '.join(map(str, (B, *shape)))}]")
        out.append(t)
    return (X, U, B, *out)


def scene_problem(problem, obstacles=None):
    """The NlotProblem a measurement against the exact scene passes: `problem` with the scene `obstacles` (None: its
    own), or with n_obs == 0 when there is none."""
    scene = problem.obstacles if obstacles is None else obstacles
    if scene:
        return problem.with_(sdf="analytic", obstacles=list(scene)).to_c()  # to_c() drops the scene of an mlp problem
    return problem.with_(sdf="mlp", obstacles=[]).to_c()
