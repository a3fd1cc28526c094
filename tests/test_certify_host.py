"""nlot_certify_batch / nlot_default_certify_options on the host (no GPU): the C defaults agree with the Python ones,
the flag constants with the header, and every documented refusal comes back as NLOT_ERR_INVALID with its message
before any device call."""
import ctypes as C
import inspect
import os
import re

import pytest


def test_default_certify_options_agree():
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.certify import certify_batch

    o = _abi.NlotCertifyOptions(tol=-7.0, clearance_min=-7.0, decide=-7, max_evals=-7)
    _lib.lib().nlot_default_certify_options(C.byref(o))
    d = _abi.certify_options()
    sig = inspect.signature(certify_batch).parameters
    for k, _ in o._fields_:
        assert getattr(o, k) == getattr(d, k) == sig[k].default, k
    assert (o.tol, o.clearance_min, o.decide, o.max_evals) == (1e-3, 0.0, 0, 0)


def test_certify_flag_constants_match_the_header():
    from nlotrajectories_amd import _abi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = dict(re.findall(r"#define NLOT_CERTIFY_([A-Z]+)\s+(\d+)", open(os.path.join(root, "include", "nlot.h")).read()))
    assert {k: int(v) for k, v in hdr.items()} == {"COLLISION": 1, "CONTAINS": 2, "UNDECIDED": 4, "BUDGET": 8,
                                                   "NONFINITE": 32}
    for k, v in hdr.items():
        assert getattr(_abi, "CERTIFY_" + k) == int(v)


FAKE = C.c_void_p(64)  # a non-null "device pointer": the call must refuse before it could be used
REFUSALS = [
    (dict(ptrs=None), "nlot_certify_batch: null pointer"), (dict(prob=None), "null problem or options"),
    (dict(tol=0.0), "tol must be > 0"), (dict(tol=float("inf")), "tol must be > 0"), (dict(tol=float("nan")), "tol must be > 0"),
    (dict(clearance_min=float("nan")), "clearance_min must be finite"), (dict(decide=2), "decide must be 0 or 1"),
    (dict(max_evals=-1), "max_evals must be"), (dict(max_evals=(1 << 24) + 1), "max_evals must be"),
    (dict(prob="metric"), "n_obs == 0"), (dict(prob="bad"), "invalid problem"),
    (dict(B=0), "B out of range"), (dict(B=(1 << 26) + 1), "B out of range"),
]


@pytest.mark.parametrize("kw,message", REFUSALS)
def test_certify_batch_refuses_bad_arguments_before_the_device(kw, message):
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.problem import BENCHMARKS, METRIC_PROBLEM

    kw = dict(kw)
    prob, ptrs, B = kw.pop("prob", "b2"), kw.pop("ptrs", FAKE), kw.pop("B", 4)
    pc = {"b2": BENCHMARKS["b2"]["problem"], "metric": METRIC_PROBLEM, "bad": BENCHMARKS["b2"]["problem"].with_(N=0), None: None}[prob]
    opt = _abi.certify_options()
    for k, v in kw.items():
        setattr(opt, k, v)  # past certify_options' own conversions
    L = _lib.lib()
    rc = L.nlot_certify_batch(C.byref(pc.to_c()) if pc else None, C.byref(opt), ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, B, None)
    assert rc == -1 and message in L.nlot_last_error().decode()
