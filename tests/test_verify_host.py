"""nlot_verify_batch / nlot_default_verify_options on the host (no GPU): the C defaults agree with the Python ones,
and every documented refusal comes back as NLOT_ERR_INVALID with its message before any device call."""
import ctypes as C
import inspect


def test_default_verify_options_agree():
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.verify import verify_batch

    o = _abi.NlotVerifyOptions(sub=-7, edge_points=-7, clearance_min=-7.0, defect_tol=-7.0, bound_tol=-7.0)
    _lib.lib().nlot_default_verify_options(C.byref(o))
    d = _abi.verify_options()
    sig = inspect.signature(verify_batch).parameters
    for k, _ in o._fields_:
        assert getattr(o, k) == getattr(d, k) == sig[k].default, k
    assert (o.sub, o.edge_points, o.clearance_min, o.defect_tol, o.bound_tol) == (8, 3, 0.0, 1e-4, 1e-4)


def test_verify_flag_constants_match_the_header():
    import os
    import re

    from nlotrajectories_amd import _abi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = dict(re.findall(r"#define NLOT_VERIFY_([A-Z]+)\s+(\d+)", open(os.path.join(root, "include", "nlot.h")).read()))
    assert {k: int(v) for k, v in hdr.items()} == {"COLLISION": 1, "CONTAINS": 2, "DEFECT": 4, "UBOUND": 8,
                                                   "BOUNDARY": 16, "NONFINITE": 32}
    for k, v in hdr.items():
        assert getattr(_abi, "VERIFY_" + k) == int(v)


def test_verify_batch_refuses_bad_arguments_before_the_device():
    """Every refusal include/nlot.h lists, with null (or never dereferenced) device pointers: no GPU is touched."""
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.problem import BENCHMARKS, METRIC_PROBLEM

    L = _lib.lib()
    pc = BENCHMARKS["b2"]["problem"].to_c()
    fake = C.c_void_p(64)  # a non-null "device pointer": the call must refuse before it could be used

    def call(opt=None, B=4, prob=pc, x0=None, xg=None, ptrs=None):
        opt = opt or _abi.verify_options()
        rc = L.nlot_verify_batch(C.byref(prob) if prob is not None else None, C.byref(opt), ptrs, ptrs, x0, xg, ptrs, ptrs,
                                 ptrs, ptrs, ptrs, ptrs, B, None)
        return rc, L.nlot_last_error().decode()

    rc, msg = call()
    assert rc == -1 and msg == "nlot_verify_batch: null pointer"
    rc, msg = call(prob=None)
    assert rc == -1 and "null problem or options" in msg
    rc, msg = call(_abi.verify_options(sub=0), ptrs=fake)
    assert rc == -1 and "sub must be >= 1" in msg
    rc, msg = call(_abi.verify_options(edge_points=-1), ptrs=fake)
    assert rc == -1 and "edge_points must be >= 0" in msg
    rc, msg = call(prob=METRIC_PROBLEM.to_c(), ptrs=fake)  # a learned-SDF problem: to_c() carries no scene
    assert rc == -1 and "n_obs == 0" in msg
    for B in (0, -1, (1 << 26) + 1):
        rc, msg = call(B=B, ptrs=fake)
        assert rc == -1 and "B out of range" in msg, B
    for kw in (dict(x0=fake), dict(xg=fake)):
        rc, msg = call(ptrs=fake, **kw)
        assert rc == -1 and "x0 and xg must both be given or both be NULL" in msg
    # (N sub + 1) * n_body (1 + edge_points) = (50 * 2^22 + 1) * 4 * 4 > 2^31
    rc, msg = call(_abi.verify_options(sub=1 << 22), ptrs=fake)
    assert rc == -1 and "overflows int32" in msg
    rc, msg = call(_abi.verify_options(edge_points=(1 << 31) - 1), ptrs=fake)
    assert rc == -1 and "overflows int32" in msg


def test_verify_batch_needs_a_scene():
    """The Python call raises ValueError, before it asks for the GPU, when neither the problem nor `obstacles` gives
    a scene, and when only one of x0 / xg is given."""
    import pytest

    from nlotrajectories_amd.problem import BENCHMARKS, METRIC_PROBLEM
    from nlotrajectories_amd.verify import verify_batch

    X, U = [[[0.0] * 5] * 51], [[[0.0] * 2] * 50]
    with pytest.raises(ValueError, match="no obstacles"):
        verify_batch(METRIC_PROBLEM, X, U)
    with pytest.raises(ValueError, match="both"):
        verify_batch(BENCHMARKS["b2"]["problem"], X, U, x0=[[0.0] * 5])
