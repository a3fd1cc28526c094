"""nlot_scene_sdf_eval / nlot_sdf_metrics on the host (no GPU): the C defaults agree with the Python ones, the struct
sizes and constants match the header, every documented refusal comes back as NLOT_ERR_INVALID with its message
before any device call, the Python wrappers reject bad arguments before they ask for the GPU, and the CLI parser
knows the two new flags."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_sdf_metrics_options_agree():
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.scene_gpu import sdf_metrics

    o = _abi.NlotSdfMetricsOptions(threshold=-7.0, eps=-7.0)
    _lib.lib().nlot_default_sdf_metrics_options(C.byref(o))
    d = _abi.sdf_metrics_options()
    sig = inspect.signature(sdf_metrics).parameters
    for k, _ in o._fields_:
        assert getattr(o, k) == getattr(d, k) == sig[k].default, k
    assert (o.threshold, o.eps) == (0.0, 1e-2)


def test_struct_sizes_and_constants_match_the_header():
    from nlotrajectories_amd import _abi, scene_gpu

    assert C.sizeof(_abi.NlotSdfMetrics) == 64
    assert C.sizeof(_abi.NlotSdfMetricsOptions) == 16
    hdr = open(os.path.join(ROOT, "include", "nlot.h")).read()
    kinds = {k: int(v) for k, v in re.findall(r"#define NLOT_SCENE_([A-Z]+)\s+(\d+)", hdr)}
    assert kinds == {"EXACT": 0, "APPROX": 1}
    assert (_abi.SCENE_EXACT, _abi.SCENE_APPROX) == (kinds["EXACT"], kinds["APPROX"])
    assert scene_gpu.KINDS == {"exact": 0, "approx": 1}
    # the field order of the header's NlotSdfMetrics
    body = re.search(r"typedef struct NlotSdfMetrics \{(.*?)\} NlotSdfMetrics;", hdr, re.S)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"(?:double|int64_t)\s+([^;]+);", body) for n in re.split(r",\s*", decl.strip())]
    assert names == [k for k, _ in _abi.NlotSdfMetrics._fields_]
    src = open(os.path.join(ROOT, "nlotrajectories_amd", "csrc", "nlot_scene.hip")).read()
    assert int(re.search(r"#define NLOT_NEAREST_TILE (\d+)", src)[1]) == scene_gpu.NEAREST_TILE


def test_scene_sdf_eval_refuses_bad_arguments_before_the_device():
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.problem import BENCHMARKS, METRIC_PROBLEM

    L = _lib.lib()
    pc = BENCHMARKS["b2"]["problem"].to_c()
    fake = C.c_void_p(64)  # a non-null "device pointer": the call must refuse before it could be used

    def call(prob=pc, kind=_abi.SCENE_EXACT, pts=fake, P=4, val=fake, grad=None, hess=None):
        rc = L.nlot_scene_sdf_eval(C.byref(prob) if prob is not None else None, kind, pts, P, val, grad, hess, None)
        return rc, L.nlot_last_error().decode()

    for kw in (dict(prob=None), dict(pts=None), dict(val=None)):
        rc, msg = call(**kw)
        assert rc == -1 and "null problem, pts or val" in msg, kw
    for kind in (-1, 2):
        rc, msg = call(kind=kind)
        assert rc == -1 and "kind must be" in msg, kind
    rc, msg = call(prob=METRIC_PROBLEM.to_c())  # a learned-SDF problem: to_c() carries no scene
    assert rc == -1 and "n_obs == 0" in msg
    for P in (0, -1, (1 << 30) + 1):
        rc, msg = call(P=P)
        assert rc == -1 and "P out of range" in msg, P
    for kw in (dict(grad=fake), dict(hess=fake), dict(grad=fake, hess=fake)):
        rc, msg = call(**kw)
        assert rc == -1 and "need NLOT_SCENE_APPROX" in msg, kw
    # a scene that would index outside obs / verts is refused too (nothing on the device checks it)
    bad = BENCHMARKS["b4"]["problem"].to_c()
    bad.obs[0].nv = bad.n_verts + 1
    rc, msg = call(prob=bad)
    assert rc == -1 and "vertex range" in msg
    bad = BENCHMARKS["b2"]["problem"].to_c()
    bad.n_obs = _abi.MAX_OBS + 1
    rc, msg = call(prob=bad)
    assert rc == -1 and "invalid scene" in msg


def test_sdf_metrics_refuses_bad_arguments_before_the_device():
    from nlotrajectories_amd import _abi, _lib

    L = _lib.lib()
    fake = C.c_void_p(64)

    def call(opt=None, P=4, null=None, no_opt=False):
        opt = opt or _abi.sdf_metrics_options()
        a = [fake if null != i else None for i in range(4)]
        rc = L.nlot_sdf_metrics(None if no_opt else C.byref(opt), a[0], a[1], a[2], P, a[3], None)
        return rc, L.nlot_last_error().decode()

    rc, msg = call(no_opt=True)
    assert rc == -1 and msg == "nlot_sdf_metrics: null pointer"
    for i in range(4):
        rc, msg = call(null=i)
        assert rc == -1 and msg == "nlot_sdf_metrics: null pointer", i
    for P in (0, -1, (1 << 30) + 1):
        rc, msg = call(P=P)
        assert rc == -1 and "P out of range" in msg, P
    for eps in (0.0, -1e-2, float("inf"), float("nan")):
        rc, msg = call(_abi.sdf_metrics_options(eps=eps))
        assert rc == -1 and "eps must be finite and > 0" in msg, eps
    for thr in (float("inf"), -float("inf"), float("nan")):
        rc, msg = call(_abi.sdf_metrics_options(threshold=thr))
        assert rc == -1 and "threshold must be finite" in msg, thr


def test_python_wrappers_reject_bad_arguments_before_the_gpu():
    """ValueError for an unknown kind, derivatives of the exact SDF, wrong shapes and an empty scene: none of them
    reaches require_gpu() (this test runs without a GPU)."""
    from nlotrajectories_amd.problem import BENCHMARKS, METRIC_PROBLEM
    from nlotrajectories_amd.scene_gpu import scene_sdf_eval, sdf_metrics

    obs = BENCHMARKS["b2"]["problem"].obstacles
    pts = np.zeros((5, 2))
    with pytest.raises(ValueError, match="kind must be"):
        scene_sdf_eval(obs, pts, kind="smooth")
    with pytest.raises(ValueError, match="derivatives need"):
        scene_sdf_eval(obs, pts, kind="exact", derivatives=True)
    for bad in (np.zeros(5), np.zeros((5, 3)), np.zeros((0, 2)), np.zeros((2, 5, 2))):
        with pytest.raises(ValueError, match="pts must be"):
            scene_sdf_eval(obs, bad)
        with pytest.raises(ValueError, match="pts must be"):
            sdf_metrics(bad, np.zeros(5), np.zeros(5))
    with pytest.raises(ValueError, match="no obstacles"):
        scene_sdf_eval(METRIC_PROBLEM, pts)
    with pytest.raises(ValueError, match="no obstacles"):
        scene_sdf_eval([], pts)
    with pytest.raises(ValueError, match="target must have 5 entries"):
        sdf_metrics(pts, np.zeros(4), np.zeros(5))
    with pytest.raises(ValueError, match="pred must have 5 entries"):
        sdf_metrics(pts, np.zeros(5), np.zeros((5, 2)))
    with pytest.raises(ValueError, match="eps must be"):
        sdf_metrics(pts, np.zeros(5), np.zeros(5), eps=0.0)
    with pytest.raises(ValueError, match="unknown obstacle type"):
        scene_sdf_eval([{"type": "blob"}], pts)


def test_trainer_rejects_an_unknown_sdf_device():
    import torch.nn as nn

    from nlotrajectories_amd.trainer import NNObstacleTrainer

    with pytest.raises(ValueError, match="sdf_device"):
        NNObstacleTrainer([], nn.Linear(2, 1), device="cpu", verbose=False, sdf_device="tpu")
    assert NNObstacleTrainer([], nn.Linear(2, 1), device="cpu", verbose=False).sdf_device == "host"


def test_cli_parser_knows_the_device_flags():
    from nlotrajectories_amd import cli

    a = cli._parser().parse_args(["--config", "x.yaml"])
    assert (a.metrics_device, a.train_sdf_device) == ("host", "host")
    a = cli._parser().parse_args(["--config", "x.yaml", "--metrics-device", "gpu", "--train-sdf-device", "gpu"])
    assert (a.metrics_device, a.train_sdf_device) == ("gpu", "gpu")
    with pytest.raises(SystemExit):
        cli._parser().parse_args(["--config", "x.yaml", "--metrics-device", "tpu"])
    sig = inspect.signature(cli.run_benchmark).parameters
    assert sig["metrics_device"].default == "host" and sig["train_sdf_device"].default == "host"
    assert inspect.signature(cli._metrics).parameters["device"].default == "host"
