"""nlot_scene_sdf_eval / nlot_sdf_metrics on the GPU (csrc/nlot_scene.hip, scene_gpu.py) against the
host restatements of scene.py, the reference-computed golden scene values and the oracle's derivatives.

Bars (none taken from what the kernels give):
  * values: 1e-12 absolute, the bar test_nlp_golden.py holds the oracle to (same formulas, fp64 on both sides);
  * gradient / Hessian: 1e-9 relative to max(1, |ref|) against oracle.sdf_eval (DESIGN.md §4c's bar);
  * metrics: iou and the three counts exact, hausdorff 1e-12 relative (a max of mins with one sqrt), mse / chamfer /
    surface_loss 1e-10 relative (sums of at most 3e4 non-negative fp64 terms: n 2^-53 = 3e-12).  The host asserts
    first that no |value| lies within 1e-9 of eps and no value within 1e-9 of the threshold, so set membership
    cannot differ by rounding.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "nlp_golden.json")))
YAMLS = ["benchmark_1_dot_circle.yaml", "benchmark_2_unicycle_circle.yaml", "benchmark_3_unicycle_convex.yaml",
         "benchmark_4_dot_nonconvex.yaml", "benchmark_5_ackermann_circle.yaml", "benchmark_6_ackermann_wave.yaml"]
# tests/test_branches_gpu.py's discr_s (a group of 18 trapezoids) next to a trapezoid
DISCR_S = [{"type": "discr_s", "center": (0.3, 0.5), "semi_axes": (0.25, 0.2), "width": 0.05, "angle": 3.14,
            "num_arc_points": 10, "margin": 0.01},
           {"type": "trapezoid", "points": [(0.6, 0.05), (0.9, 0.05), (0.85, 0.25), (0.65, 0.25)], "margin": 0.01}]
SCENES = YAMLS + ["discr_s_trapezoid"]
N_SEEDED = 4099


def _config(fn):
    from nlotrajectories_amd.config import Config

    return Config.model_validate(GOLD["configs"][fn])


def scene_obstacles(name):
    return DISCR_S if name == "discr_s_trapezoid" else _config(name).obstacle_dicts()


def scene_points(name):
    """4,099 seeded points of [-1, 2]^2, then every primitive's centre, vertex and edge midpoint."""
    from nlotrajectories_amd.obstacles import expand

    prims, verts = expand(scene_obstacles(name))
    pts = [np.random.default_rng(SCENES.index(name)).uniform(-1.0, 2.0, size=(N_SEEDED, 2))]
    pts.append(np.array([[q["cx"], q["cy"]] for q in prims]))
    for q in prims:
        if q["nv"]:
            V = np.asarray(verts[q["v0"]:q["v0"] + q["nv"]], float)
            pts += [V, 0.5 * (V + np.roll(V, -1, axis=0))]
    pts = np.concatenate(pts)
    if len(pts) % 64 == 0:  # P is deliberately not a multiple of the wave size
        pts = np.concatenate([pts, [[0.123, 0.456]]])
    return pts


_HOST = {}


def host_reference(name):
    """scene.py's values at scene_points(name), computed once and shared."""
    if name not in _HOST:
        from nlotrajectories_amd import scene

        obs, pts = scene_obstacles(name), scene_points(name)
        _HOST[name] = dict(pts=pts, exact=scene.exact_sdf(obs, pts[:, 0], pts[:, 1]),
                           approx=scene.approximated_sdf(obs, pts[:, 0], pts[:, 1]))
        for v in _HOST[name].values():
            v.setflags(write=False)
    return _HOST[name]


# ---- E1 / E2 / E3: the evaluator --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_exact_sdf_matches_scene_py(name):
    from nlotrajectories_amd.scene_gpu import scene_sdf_eval

    h = host_reference(name)
    assert len(h["pts"]) % 64 != 0
    v = scene_sdf_eval(scene_obstacles(name), h["pts"], "exact").cpu().numpy()
    err = np.abs(v - h["exact"]).max()
    print(f"E1 {name}: P = {len(v)}, max |gpu - scene.exact_sdf| = {err:.3e}", flush=True)
    assert err <= 1e-12


@pytest.mark.parametrize("name", SCENES)
def test_approx_sdf_matches_scene_py(name):
    from nlotrajectories_amd.scene_gpu import scene_sdf_eval

    h = host_reference(name)
    v = scene_sdf_eval(scene_obstacles(name), h["pts"], "approx").cpu().numpy()
    err = np.abs(v - h["approx"]).max()
    print(f"E2 {name}: max |gpu - scene.approximated_sdf| = {err:.3e}", flush=True)
    assert err <= 1e-12


@pytest.mark.parametrize("fn", YAMLS)
def test_approx_sdf_matches_the_reference_golden(fn):
    """The reference-computed MultiObstacle.approximated_sdf values of tests/golden/nlp_golden.json at that file's
    own points, read as test_nlp_golden.py reads them (YAML -> Problem)."""
    from nlotrajectories_amd.scene_gpu import scene_sdf_eval

    prob = _config(fn).to_problem().with_(sdf="analytic")
    pts = np.asarray(GOLD["sdf"]["points"])
    v = scene_sdf_eval(prob, pts, "approx").cpu().numpy()
    err = np.abs(v - np.asarray(GOLD["scene_sdf"][fn])).max()
    print(f"E2 golden {fn}: max |gpu - reference| = {err:.3e}", flush=True)
    assert err <= 1e-12


@pytest.mark.parametrize("name", SCENES)
def test_approx_derivatives_match_the_oracle(name):
    """Gradient and Hessian at the seeded points (the centres and vertices are singular points of the smoothed SDF's
    derivatives) against oracle.sdf_eval's [v, gx, gy, hxx, hxy, hyy]."""
    import oracle as O
    from nlotrajectories_amd.problem import Problem
    from nlotrajectories_amd.scene_gpu import scene_sdf_eval

    obs = scene_obstacles(name)
    pts = host_reference(name)["pts"][:N_SEEDED]
    ref = O.sdf_eval(Problem(dynamics="point_2nd", shape="dot", obstacles=obs), pts)
    assert np.isfinite(ref).all()
    v, g, h = (t.cpu().numpy() for t in scene_sdf_eval(obs, pts, "approx", derivatives=True))
    got = np.concatenate([v[:, None], g, h], axis=1)
    rel = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"E2 {name}: max rel err value {rel[:, 0].max():.3e} grad {rel[:, 1:3].max():.3e} "
          f"hess {rel[:, 3:].max():.3e}", flush=True)
    assert rel.max() <= 1e-9
    # the value does not depend on whether the derivatives are asked for
    v0 = scene_sdf_eval(obs, pts, "approx").cpu().numpy()
    assert np.abs(v0 - v).max() <= 1e-12


@pytest.mark.parametrize("kind", ["exact", "approx"])
def test_a_points_outputs_do_not_depend_on_the_batch(kind):
    """P = 1 works, and a 257-point subset evaluated alone is bitwise what the same points give inside the full call."""
    import torch
    from nlotrajectories_amd.scene_gpu import scene_sdf_eval

    def same_bits(a, b):  # NaNs included (the derivatives at a vertex)
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))

    name = "benchmark_6_ackermann_wave.yaml"
    obs, h = scene_obstacles(name), host_reference(name)
    full = scene_sdf_eval(obs, h["pts"], kind)
    idx = np.random.default_rng(3).choice(len(h["pts"]), size=257, replace=False)
    didx = torch.as_tensor(idx, device=full.device)
    sub = scene_sdf_eval(obs, h["pts"][idx], kind)
    assert same_bits(sub, full[didx])
    one = scene_sdf_eval(obs, h["pts"][idx[:1]], kind)
    assert one.shape == (1,) and same_bits(one, sub[:1])
    if kind == "approx":
        fd = scene_sdf_eval(obs, h["pts"], kind, derivatives=True)
        sd = scene_sdf_eval(obs, h["pts"][idx], kind, derivatives=True)
        for a, b in zip(sd, fd):
            assert same_bits(a, b[didx])


def test_grad_with_the_exact_kind_is_refused_on_the_device_path():
    import ctypes as C

    import torch
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.problem import BENCHMARKS

    pc = BENCHMARKS["b2"]["problem"].to_c()
    pts = torch.zeros(8, 2, dtype=torch.float64, device="cuda")
    val = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    grad = torch.full((8, 2), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib().nlot_scene_sdf_eval(C.byref(pc), _abi.SCENE_EXACT, p(pts), 8, p(val), p(grad), None, None)
    assert rc == -1 and "need NLOT_SCENE_APPROX" in _lib.lib().nlot_last_error().decode()
    torch.cuda.synchronize()
    assert bool((val == 7.0).all()) and bool((grad == 7.0).all())  # nothing was launched


# ---- M1 - M3: the metrics on synthetic sets ---------------------------------------------------------------------
EPS, THR = 1e-2, 0.0
P_SYN = 5003  # no multiple of the block sizes (256, 1024)


def synthetic(nT, nQ, seed, eps=EPS):
    """Seeded pts / target / pred with exactly nT entries of |target| < eps and nQ of |pred| < eps: band values of
    magnitude in [0.1, 0.9] eps, the rest in [5, 100] eps, random signs, so every value keeps 0.1 eps from eps and
    from the threshold 0."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.0, 2.0, size=(P_SYN, 2))

    def field(n):
        v = rng.uniform(5 * eps, 100 * eps, size=P_SYN)
        band = rng.choice(P_SYN, size=n, replace=False)
        v[band] = rng.uniform(0.1 * eps, 0.9 * eps, size=n)
        return v * rng.choice([-1.0, 1.0], size=P_SYN)

    return pts, field(nT), field(nQ)


def assert_no_borderline(target, pred, eps, thr):
    """The condition under which set membership cannot differ by rounding (asserted on the host, before the GPU)."""
    for v in (np.asarray(target).ravel(), np.asarray(pred).ravel()):
        assert np.abs(np.abs(v) - eps).min() > 1e-9
        assert np.abs(v - thr).min() > 1e-9


def host_metrics(pts, target, pred, eps=EPS, thr=THR):
    from nlotrajectories_amd import scene

    X, Y = pts[:, 0], pts[:, 1]
    return dict(mse=scene.mse(target, pred), iou=scene.iou(target, pred, thr),
                hausdorff=scene.hausdorff(target, pred, X, Y, eps), chamfer=scene.chamfer(target, pred, X, Y, eps),
                surface_loss=scene.surface_loss(target, pred, eps),
                n_target_surface=int((np.abs(target) < eps).sum()), n_pred_surface=int((np.abs(pred) < eps).sum()),
                n_points=len(target))


def compare_metrics(got, ref, what, evaluators=0.0):
    """M1's bars.  M4 feeds the two sides values of different evaluators, which E1 / E2 hold to evaluators = 1e-12
    of each other: that is added to the hausdorff and chamfer bars, and mse and surface_loss, means of squares of
    values that differ by d <= 2 evaluators (mse: both operands) or evaluators, get the first-order term
    2 sqrt(mean) d + d^2 (benchmark 2's host mse is exactly 0: its one-term soft_min is the identity on the host)."""
    print(what, "gpu", got, "host", ref, flush=True)
    for k in ("iou", "n_target_surface", "n_pred_surface", "n_points"):
        assert got[k] == ref[k], (what, k, got[k], ref[k])

    def sq(k, d):
        return 0.0 if ref[k] is None else 2 * np.sqrt(ref[k]) * d + d * d

    for k, rel, ab in (("hausdorff", 1e-12, evaluators), ("chamfer", 1e-10, evaluators),
                       ("mse", 1e-10, sq("mse", 2 * evaluators)), ("surface_loss", 1e-10, sq("surface_loss", evaluators))):
        if ref[k] is None:
            assert got[k] is None, (what, k, got[k])
        else:
            assert got[k] is not None and abs(got[k] - ref[k]) <= rel * abs(ref[k]) + ab, (what, k, got[k], ref[k])


def _tile():
    from nlotrajectories_amd.scene_gpu import NEAREST_TILE

    return NEAREST_TILE


@pytest.mark.parametrize("case", range(4))
def test_metrics_on_synthetic_sets(case):
    from nlotrajectories_amd.scene_gpu import sdf_metrics

    T = _tile()
    nT, nQ = [(1, 1), (T - 1, T + 1), (2 * T + 3, 5), (5, 2 * T + 3)][case]
    pts, target, pred = synthetic(nT, nQ, seed=10 + case)
    assert_no_borderline(target, pred, EPS, THR)
    ref = host_metrics(pts, target, pred)
    assert (ref["n_target_surface"], ref["n_pred_surface"]) == (nT, nQ) and P_SYN % 256 != 0
    compare_metrics(sdf_metrics(pts, target, pred), ref, f"M1 ({nT}, {nQ})")


def test_metrics_of_empty_sets():
    from nlotrajectories_amd.scene_gpu import sdf_metrics

    pts, target, pred = synthetic(0, 40, seed=20)  # T empty
    assert_no_borderline(target, pred, EPS, THR)
    r = sdf_metrics(pts, target, pred)
    assert r["hausdorff"] is None and r["chamfer"] is None and r["surface_loss"] is None
    assert r["n_target_surface"] == 0 and r["n_pred_surface"] == 40
    compare_metrics(r, host_metrics(pts, target, pred), "M2 T empty")
    pts, target, pred = synthetic(40, 0, seed=21)  # Q empty
    assert_no_borderline(target, pred, EPS, THR)
    r = sdf_metrics(pts, target, pred)
    assert r["hausdorff"] is None and r["chamfer"] is None and r["surface_loss"] is not None
    assert r["n_target_surface"] == 40 and r["n_pred_surface"] == 0
    compare_metrics(r, host_metrics(pts, target, pred), "M2 Q empty")
    # nothing below the threshold on either side: the union is empty, iou = 1
    r = sdf_metrics(pts, np.abs(target), np.abs(pred))
    assert r["iou"] == 1.0
    compare_metrics(r, host_metrics(pts, np.abs(target), np.abs(pred)), "M2 empty union")


def test_metrics_are_reproducible():
    import ctypes as C

    import torch
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.scene_gpu import sdf_metrics

    T = _tile()
    pts, target, pred = synthetic(T + 77, 2 * T + 3, seed=30)
    assert_no_borderline(target, pred, EPS, THR)
    d = [torch.as_tensor(a, device="cuda") for a in (pts, target, pred)]
    outs = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    opt = _abi.sdf_metrics_options()
    for o in outs:
        rc = _lib.lib().nlot_sdf_metrics(C.byref(opt), *(C.c_void_p(t.data_ptr()) for t in d), P_SYN,
                                         C.c_void_p(o.data_ptr()), None)
        assert rc == 0, _lib.lib().nlot_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])  # bitwise
    a = sdf_metrics(pts, target, pred)
    perm = np.random.default_rng(31).permutation(P_SYN)
    b = sdf_metrics(pts[perm], target[perm], pred[perm])
    for k in ("hausdorff", "iou", "n_target_surface", "n_pred_surface", "n_points"):
        assert a[k] == b[k], k
    for k in ("mse", "chamfer", "surface_loss"):
        assert abs(a[k] - b[k]) <= 1e-12 * abs(a[k]), (k, a[k], b[k])


# ---- M4: end to end ---------------------------------------------------------------------------------------------
N_GRID = 160
M4_SCENES = ["benchmark_2_unicycle_circle.yaml", "benchmark_4_dot_nonconvex.yaml", "benchmark_6_ackermann_wave.yaml"]
_GRID = {}


def host_grid(fn):
    """cli._metrics' grid and host SDFs at n = N_GRID, computed once."""
    if fn not in _GRID:
        from nlotrajectories_amd import scene

        obs = _config(fn).obstacle_dicts()
        x = np.linspace(-1.0, 2.0, N_GRID)
        X, Y = np.meshgrid(x, x)
        _GRID[fn] = dict(pts=np.stack([X.ravel(), Y.ravel()], 1), exact=scene.exact_sdf(obs, X, Y).ravel(),
                         approx=scene.approximated_sdf(obs, X, Y).ravel())
    return _GRID[fn]


@pytest.mark.parametrize("fn", M4_SCENES)
def test_scene_metrics_match_the_host_path(fn):
    from nlotrajectories_amd import cli
    from nlotrajectories_amd.scene_gpu import scene_metrics, scene_sdf_eval, sdf_metrics

    cfg, g = _config(fn), host_grid(fn)
    keys = ("mse", "iou", "hausdorff", "chamfer", "surface_loss")
    for eps in (1e-2, 5e-2):
        assert_no_borderline(g["exact"], g["approx"], eps, 0.0)
    # eps = 1e-2: the whole of compute_metrics on each side
    ref = dict(host_metrics(g["pts"], g["exact"], g["approx"], 1e-2), **dict(zip(keys, cli._metrics(cfg, None, n=N_GRID))))
    got = dict(zip(keys, scene_metrics(cfg.obstacle_dicts(), n=N_GRID)))
    compare_metrics(dict(ref, **got), ref, f"M4 {fn} eps 1e-2", evaluators=1e-12)
    # eps = 5e-2 through sdf_metrics, the device's own evaluations as input
    obs = cfg.obstacle_dicts()
    ref = host_metrics(g["pts"], g["exact"], g["approx"], 5e-2)
    got = sdf_metrics(g["pts"], scene_sdf_eval(obs, g["pts"], "exact"), scene_sdf_eval(obs, g["pts"], "approx"), eps=5e-2)
    compare_metrics(got, ref, f"M4 {fn} eps 5e-2", evaluators=1e-12)


def test_wide_bands_exceed_the_tile():
    """M4's eps = 5e-2 case puts both bands above k_nearest's tile in benchmark 4's scene (a host-side fact)."""
    g = host_grid("benchmark_4_dot_nonconvex.yaml")
    assert (np.abs(g["exact"]) < 5e-2).sum() > _tile() and (np.abs(g["approx"]) < 5e-2).sum() > _tile()


def test_scene_metrics_with_the_b6_net():
    """The learned SDF of benchmark 6 as the prediction: one sdf_mlp_eval output feeds both sides."""
    import torch
    from nlotrajectories_amd import _lib
    from nlotrajectories_amd.nn import MlpWeights
    from nlotrajectories_amd.ops import DeviceMlp, sdf_mlp_eval
    from nlotrajectories_amd.scene_gpu import scene_sdf_eval, sdf_metrics

    fn = "benchmark_6_ackermann_wave.yaml"
    g, obs = host_grid(fn), _config(fn).obstacle_dicts()
    mlp = DeviceMlp(MlpWeights.load(os.path.join(_lib.PKG_DIR, "data", "b6_mlp128_seed0.npz")))
    pred = sdf_mlp_eval(mlp, torch.as_tensor(g["pts"], dtype=torch.float32, device="cuda"), derivatives=False)[0]
    pred = pred.to(torch.float64)
    pred_h = pred.cpu().numpy()
    for eps in (1e-2, 5e-2):
        assert_no_borderline(g["exact"], pred_h, eps, 0.0)
        got = sdf_metrics(g["pts"], scene_sdf_eval(obs, g["pts"], "exact"), pred, eps=eps)
        compare_metrics(got, host_metrics(g["pts"], g["exact"], pred_h, eps), f"M4 b6 net eps {eps}", evaluators=1e-12)


# ---- C1: the CLI ------------------------------------------------------------------------------------------------
def test_cli_metrics_device_gpu_writes_the_same_csv(tmp_path):
    """benchmark_2's YAML (tests/test_cli_gpu.py's start / goal, which converges quickly) with --metrics-device gpu and
    host: the same columns, the five metrics to 1e-9 relative (or None on both sides), every other column identical
    but solver_time, which is the wall-clock time of the solve."""
    import yaml
    from nlotrajectories_amd.cli import CSV_HEADER, main

    cfg = yaml.safe_load(open(os.path.join(HERE, "golden", "configs", "benchmark_2_unicycle_circle.yaml")))
    cfg["body"]["start_state"] = [0.0, 0.95, 0.0, 0.0, 0.0]
    cfg["body"]["goal_state"] = [1.0, 0.95, 0.0, 0.0, 0.0]
    f = tmp_path / "benchmark_2_unicycle_circle.yaml"
    f.write_text(yaml.safe_dump(cfg))
    rows = {}
    for dev in ("host", "gpu"):
        out = tmp_path / dev
        main(["--config", str(f), "--initializer", "linear", "--results", str(out), "--metrics-device", dev])
        lines = open(out / "benchmark_2_unicycle_circle_results.csv").read().strip().split("\n")
        assert lines[0] == CSV_HEADER and len(lines) == 2
        rows[dev] = dict(zip(CSV_HEADER.split(","), lines[1].split(",")))
        assert len(rows[dev]) == 20
    metrics = ("mse", "iou", "hausdorff", "chamfer", "surface_loss")
    for k in CSV_HEADER.split(","):
        h, g = rows["host"][k], rows["gpu"][k]
        if k in metrics:
            print("C1", k, "host", h, "gpu", g, flush=True)
            assert (h == g == "None") or abs(float(h) - float(g)) <= 1e-9 * abs(float(h)), k
        elif k != "solver_time":
            assert h == g, k


# ---- T1: the trainer --------------------------------------------------------------------------------------------
def test_trainer_targets_from_the_device():
    import torch.nn as nn
    from nlotrajectories_amd.problem import BENCHMARKS
    from nlotrajectories_amd.trainer import NNObstacleTrainer

    obs = BENCHMARKS["b6"]["problem"].obstacles
    margin = 0.8  # benchmark_6's boundary_fraction, which generate_data passes as sample_points' margin
    data, gaps = {}, []
    for dev in ("host", "gpu"):
        tr = NNObstacleTrainer(obs, nn.Linear(2, 1), device="cpu", boundary_fraction=margin, seed=0, verbose=False,
                               sdf_device=dev)
        if dev == "host":  # record how close a candidate's |sdf| comes to the band's edge
            inner = tr.sdf

            def recording(x, y, inner=inner):
                v = inner(x, y)
                gaps.append(np.abs(np.abs(v) - margin).min())
                return v

            tr.sdf = recording
        data[dev] = tr.generate_data((-0.5, 1.5), (-0.5, 1.5), 4000)
    assert min(gaps) > 1e-9  # then the rejection rounds accept the same candidates on both sides
    assert data["host"][0].shape == (4000, 2)
    assert (data["host"][0] == data["gpu"][0]).all()
    err = float((data["host"][1] - data["gpu"][1]).abs().max())
    print(f"T1: max |host - gpu| fp32 target = {err:.3e}", flush=True)
    assert err <= 1e-7
