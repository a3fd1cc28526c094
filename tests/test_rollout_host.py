"""nlot_rollout_batch / nlot_default_rollout_options on the host (no GPU): the C defaults agree with the Python ones,
the flag bits agree with the header, and every documented refusal comes back as NLOT_ERR_INVALID with its message
before any device call."""
import ctypes as C
import inspect
import math


def test_default_rollout_options_agree():
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.rollout import rollout_batch

    o = _abi.NlotRolloutOptions(substeps=-7, edge_points=-7, clearance_min=-7.0, deviation_tol=-7.0, goal_tol=-7.0)
    _lib.lib().nlot_default_rollout_options(C.byref(o))
    d = _abi.rollout_options()
    sig = inspect.signature(rollout_batch).parameters
    for k, _ in o._fields_:
        assert getattr(o, k) == getattr(d, k) == sig[k].default, k
    assert (o.substeps, o.edge_points, o.clearance_min, o.deviation_tol, o.goal_tol) == (8, 3, 0.0, math.inf, math.inf)
    _lib.lib().nlot_default_rollout_options(None)  # a null pointer is ignored


def test_rollout_flag_constants_match_the_header():
    import os
    import re

    from nlotrajectories_amd import _abi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = dict(re.findall(r"#define NLOT_ROLLOUT_([A-Z]+)\s+(\d+)", open(os.path.join(root, "include", "nlot.h")).read()))
    assert {k: int(v) for k, v in hdr.items()} == {"COLLISION": 1, "CONTAINS": 2, "DEVIATION": 4, "GOAL": 8,
                                                   "NONFINITE": 32, "DIVERGED": 64}
    for k, v in hdr.items():
        assert getattr(_abi, "ROLLOUT_" + k) == int(v)
    assert _abi.ROLLOUT_FLAG_NAMES == {int(v): k.lower() for k, v in hdr.items()}


def test_rollout_batch_refuses_bad_arguments_before_the_device():
    """Every refusal include/nlot.h lists, with null (or never dereferenced) device pointers: no GPU is touched."""
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.problem import BENCHMARKS

    L = _lib.lib()
    pc = BENCHMARKS["b2"]["problem"].to_c()
    fake = C.c_void_p(64)  # a non-null "device pointer": the call must refuse before it could be used

    def call(opt=None, B=4, prob=pc, ptrs=None, null_opt=False, **kw):
        opt = opt or _abi.rollout_options()
        a = dict(X=ptrs, U=ptrs, xg=None, X_roll=None, clearance=ptrs, where=ptrs, deviation=ptrs, dev_where=ptrs,
                 goal_error=ptrs, flags=ptrs)
        a.update(kw)
        rc = L.nlot_rollout_batch(C.byref(prob) if prob is not None else None, None if null_opt else C.byref(opt),
                                  *a.values(), B, None)
        return rc, L.nlot_last_error().decode()

    rc, msg = call()
    assert rc == -1 and msg == "nlot_rollout_batch: null pointer"
    rc, msg = call(prob=None, ptrs=fake)
    assert rc == -1 and "null problem or options" in msg
    rc, msg = call(null_opt=True, ptrs=fake)
    assert rc == -1 and "null problem or options" in msg
    rc, msg = call(_abi.rollout_options(substeps=0), ptrs=fake)
    assert rc == -1 and "substeps must be >= 1" in msg
    rc, msg = call(_abi.rollout_options(edge_points=-1), ptrs=fake)
    assert rc == -1 and "edge_points must be >= 0" in msg
    for B in (0, -1, (1 << 26) + 1):
        rc, msg = call(B=B, ptrs=fake)
        assert rc == -1 and "B out of range" in msg, B
    # every required pointer on its own; xg and X_roll are optional, so with them given the others still decide
    for name in ("X", "U", "clearance", "where", "deviation", "dev_where", "goal_error", "flags"):
        rc, msg = call(ptrs=fake, xg=fake, X_roll=fake, **{name: None})
        assert rc == -1 and msg == "nlot_rollout_batch: null pointer", name
    # (N substeps + 1) * n_body (1 + edge_points) = (50 * 2^22 + 1) * 4 * 4 > 2^31
    rc, msg = call(_abi.rollout_options(substeps=1 << 22), ptrs=fake)
    assert rc == -1 and "overflows int32" in msg
    rc, msg = call(_abi.rollout_options(edge_points=(1 << 31) - 1), ptrs=fake)
    assert rc == -1 and "overflows int32" in msg
    # an invalid problem: the checks of nlot_verify_batch
    for field, value in (("dynamics", 6), ("nx", 4), ("N", 0), ("shape", 2), ("n_body", 9), ("n_obs", 129)):
        bad = BENCHMARKS["b2"]["problem"].to_c()
        setattr(bad, field, value)
        rc, msg = call(prob=bad, ptrs=fake)
        assert rc == -1 and "invalid problem" in msg, field
    bad = BENCHMARKS["b2"]["problem"].to_c()
    bad.obs[0].type = 7
    rc, msg = call(prob=bad, ptrs=fake)
    assert rc == -1 and "unknown obstacle type" in msg
    bad = BENCHMARKS["b4"]["problem"].to_c()
    bad.obs[0].nv = bad.n_verts + 1
    rc, msg = call(prob=bad, ptrs=fake)
    assert rc == -1 and "vertex range" in msg


def test_rollout_batch_allows_an_empty_scene():
    """n_obs == 0 is not refused (nlot_verify_batch refuses it): a learned-SDF problem's to_c() carries no scene, and
    with all-null pointers the call fails on the pointers, not on the scene."""
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.problem import METRIC_PROBLEM

    L = _lib.lib()
    pc = METRIC_PROBLEM.to_c()
    assert pc.n_obs == 0
    opt = _abi.rollout_options()
    rc = L.nlot_rollout_batch(C.byref(pc), C.byref(opt), None, None, None, None, None, None, None, None, None, None, 4, None)
    assert rc == -1 and L.nlot_last_error().decode() == "nlot_rollout_batch: null pointer"

