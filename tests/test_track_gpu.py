"""tvlqr_batch / track_batch (nlot_tvlqr_batch, nlot_track_batch, csrc/nlot_track.hip) on the GPU against the numpy
restatement of tests/test_track_host.py (f of the six models, the RK4 step, complex-step A and B, the Riccati recursion,
the closed-loop roll with the clamp) and against rollout_batch.

Shapes: N = 24, dt = 0.1, B = 67 (the 16-lane groups of the gains kernel and the G-lane groups of the tracking kernel
fill neither the last wave nor the last block).  Plans are seeded controls rolled from seeded starts.

Tolerances.  Gains: 1e-10 relative to max(1, |ref|): the restatement in fp64 against itself in 80-bit long double
differs by <= 3e-15 on these shapes (|K| up to 21), the bar leaves room for the device libm and summation order and is
far below any formula error.  Closed-loop states and applied controls: 1e-9 (the rollout's 1e-11 times the loop gain
|K| <= 21 over 24 knots, rounded up); the exact SDF is 1-Lipschitz in the point, so the clearance gets the same.
Open-loop equivalence with rollout_batch: 1e-12 (two instantiations of the same arithmetic).

Measured on an MI355X: DESIGN.md §13."""
import functools
import os

import numpy as np
import pytest
from test_rollout_gpu import host_pose_clearance
from test_track_host import ALL_DYNAMICS, T4, host_track, host_tvlqr, seeded_plans, t4_case

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "configs")
B, N, DT, L = 67, 24, 0.1, 0.5
BOUNDS = ((-1.0, 1.0), (-1.0, 1.0))
GAIN_TOL, ROLL_TOL, SAME_TOL = 1e-10, 1e-9, 1e-12
SUB = 8


def _cpu(v):
    return {k: t.cpu().numpy() for k, t in v.items()}


def _circle(c, r, m=0.0):
    return {"type": "circle", "center": tuple(c), "radius": r, "margin": m}


def problem(dyn, shape="dot", **kw):
    from nlotrajectories_amd.problem import Problem

    return Problem(dynamics=dyn, shape=shape, N=N, dt=DT, wheelbase=L, control_bounds=BOUNDS,
                   obstacles=[_circle((0.5, 0.5), 0.2)], **kw)


def weights(nx):
    return (100.0, 100.0) + (1.0,) * (nx - 2)


@functools.lru_cache(maxsize=None)
def case(dyn):
    """(X, U, K, P0, dx0, poses, U_applied, saturated) of a model in numpy, computed once and left unchanged (the
    references are read-only; the inputs stay writable for torch, a test that edits them copies)."""
    X, U = seeded_plans(dyn, B, N, DT, L, seed=11)
    nx = X.shape[-1]
    K, P0 = host_tvlqr(dyn, X, U, DT, L, weights(nx), 1.0, weights(nx))
    dx0 = np.tile([0.02, -0.02] + [0.0] * (nx - 2), (B, 1))
    poses, Ua, sat = host_track(dyn, X, U, K, dx0, DT, L, SUB, BOUNDS)
    for a in (P0, poses, Ua, sat):
        a.setflags(write=False)
    return X, U, K, P0, dx0, poses, Ua, sat


def rel(a, ref):
    return (np.abs(a - ref) / np.maximum(1.0, np.abs(ref))).max()


# ---- T1: gains ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dyn", ALL_DYNAMICS)
def test_gains_match_numpy(dyn):
    from nlotrajectories_amd.tracking import tvlqr_batch

    X, U, K, P0 = case(dyn)[:4]
    nx = X.shape[-1]
    Kg, Pg, st = (t.cpu().numpy() for t in tvlqr_batch(problem(dyn), X, U, q=weights(nx), r=1.0, qf=weights(nx)))
    print(dyn, "max |K|", np.abs(K).max(), "rel err K", rel(Kg, K), "P0", rel(Pg, P0))
    assert (st == 0).all()
    assert rel(Kg, K) <= GAIN_TOL and rel(Pg, P0) <= GAIN_TOL
    assert np.abs(Pg - np.swapaxes(Pg, 1, 2)).max() <= GAIN_TOL * np.abs(P0).max()


# ---- T2: closed-loop states ----------------------------------------------------------------------------------------

T2_CASES = [(d, s, 3) for d in ALL_DYNAMICS for s in ("dot", "rectangle")] + [("unicycle_2nd", "triangle", 2)]


def check_closed_loop(v, p, dyn, edge_points):
    X, U, K, P0, dx0, poses, Ua, sat = case(dyn)
    print(dyn, p.shape, "max |X_roll - numpy|", np.abs(v["X_roll"] - poses[:, ::SUB]).max(), "max |U_applied - numpy|",
          np.abs(v["U_applied"] - Ua).max(), "saturated", int(sat.sum()))
    assert np.abs(v["X_roll"] - poses[:, ::SUB]).max() <= ROLL_TOL
    assert np.abs(v["U_applied"] - Ua).max() <= ROLL_TOL
    assert (v["saturated"] == sat).all()
    knots = poses[:, ::SUB]
    d = np.hypot(knots[..., 0] - X[..., 0], knots[..., 1] - X[..., 1])
    assert np.abs(v["deviation"] - d.max(1)).max() <= ROLL_TOL
    assert np.abs(d[np.arange(B), v["dev_where"]] - d.max(1)).max() <= ROLL_TOL
    assert np.abs(v["goal_error"] - d[:, -1]).max() <= ROLL_TOL
    per_pose = host_pose_clearance(p, p.obstacles, poses.reshape(-1, poses.shape[-1]), edge_points).reshape(B, -1)
    print("  max |clearance - host|", np.abs(v["clearance"] - per_pose.min(1)).max())
    assert np.abs(v["clearance"] - per_pose.min(1)).max() <= ROLL_TOL
    assert ((v["where"] >= 0) & (v["where"] < per_pose.shape[1])).all()
    assert np.abs(per_pose[np.arange(B), v["where"]] - per_pose.min(1)).max() <= ROLL_TOL


@pytest.mark.parametrize("dyn,shape,edge_points", T2_CASES)
def test_closed_loop_matches_numpy(dyn, shape, edge_points):
    """Dot: 1 footprint point, G = 1; rectangle with 3 edge points: 16 points on 16 lanes; triangle with 2: 9 on 16."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.tracking import track_batch

    X, U, K, _, dx0 = case(dyn)[:5]
    p = problem(dyn, shape)
    v = _cpu(track_batch(p, X, U, K=K, dx0=dx0, substeps=SUB, edge_points=edge_points))
    check_closed_loop(v, p, dyn, edge_points)
    assert (v["X_roll"][:, 0] == X[:, 0] + dx0).all()
    assert not (v["flags"] & (_abi.TRACK_NONFINITE | _abi.TRACK_DIVERGED)).any()
    assert (((v["flags"] & _abi.TRACK_SATURATED) != 0) == (v["saturated"] > 0)).all()
    assert (((v["flags"] & _abi.TRACK_COLLISION) != 0) == (v["clearance"] < 0)).all()


def test_device_gains_close_the_loop_too():
    """The two calls chained on the device, as the CLI does: the gains never leave the GPU."""
    from nlotrajectories_amd.tracking import track_batch, tvlqr_batch

    dyn = "ackermann_2nd"
    X, U, _, _, dx0 = case(dyn)[:5]
    p = problem(dyn, "rectangle")
    K, _, st = tvlqr_batch(p, X, U, q=weights(7), r=1.0, qf=weights(7))
    assert (st == 0).all()
    check_closed_loop(_cpu(track_batch(p, X, U, K=K, dx0=dx0, substeps=SUB)), p, dyn, 3)


# ---- T3: open-loop equivalence -------------------------------------------------------------------------------------


@pytest.mark.parametrize("dyn,shape,edge_points", [("point_2nd", "dot", 3), ("unicycle_2nd", "rectangle", 3),
                                                    ("ackermann_2nd", "triangle", 2)])
def test_open_loop_is_the_rollout(dyn, shape, edge_points):
    from nlotrajectories_amd.rollout import rollout_batch
    from nlotrajectories_amd.tracking import track_batch

    X, U = case(dyn)[:2]
    X = X.copy()
    X[:, 1:] += np.random.default_rng(1).uniform(-0.05, 0.05, X[:, 1:].shape)  # a plan the flow leaves
    p = problem(dyn, shape)
    kw = dict(substeps=SUB, edge_points=edge_points, deviation_tol=0.05, goal_tol=0.05)
    t = _cpu(track_batch(p, X, U, clamp=False, **kw))
    r = _cpu(rollout_batch(p, X, U, **kw))
    bitwise = all(t[k].tobytes() == r[k].tobytes() for k in r)
    print(dyn, shape, "bitwise equal to rollout_batch:", bitwise)
    for k in ("X_roll", "clearance", "deviation", "goal_error"):
        assert np.abs(t[k] - r[k]).max() <= SAME_TOL, k
    assert (t["flags"] == r["flags"]).all() and (t["saturated"] == 0).all()
    assert (t["U_applied"] == U).all()
    # where / dev_where: equal, or the two candidates' values differ by less than the tolerance
    poses = host_track(dyn, X, U, None, None, DT, L, SUB)[0]
    per_pose = host_pose_clearance(p, p.obstacles, poses.reshape(-1, poses.shape[-1]), edge_points).reshape(B, -1)
    rows = np.arange(B)
    assert (np.abs(per_pose[rows, t["where"]] - per_pose[rows, r["where"]]) < SAME_TOL).all()
    knots = poses[:, ::SUB]
    d = np.hypot(knots[..., 0] - X[..., 0], knots[..., 1] - X[..., 1])
    assert (np.abs(d[rows, t["dev_where"]] - d[rows, r["dev_where"]]) < SAME_TOL).all()


# ---- T4: feedback helps ----------------------------------------------------------------------------------------------


def test_feedback_helps():
    """A unicycle at plan speeds in [0.5, 1] started 2 cm off in x and -2 cm off in y: the closed loop ends within 0.05 x
    the open loop's final planar error for every instance (the restatement alone: <= 0.012, test_track_host.py)."""
    from nlotrajectories_amd.problem import Problem
    from nlotrajectories_amd.tracking import track_batch, tvlqr_batch

    c = T4
    X, U, dx0, K_host, _, _ = t4_case()
    p = Problem(dynamics=c["dyn"], shape="dot", N=c["N"], dt=c["dt"], control_bounds=BOUNDS)
    K, _, st = tvlqr_batch(p, X, U, q=c["q"], r=c["r"], qf=c["qf"])
    assert (st.cpu().numpy() == 0).all() and rel(K.cpu().numpy(), K_host) <= GAIN_TOL
    kw = dict(dx0=dx0, substeps=c["substeps"], clamp=False)
    opened, closed = _cpu(track_batch(p, X, U, **kw)), _cpu(track_batch(p, X, U, K=K, **kw))
    ratio = closed["goal_error"] / opened["goal_error"]
    print("open-loop final error", opened["goal_error"].min(), opened["goal_error"].max(), "closed", closed["goal_error"].max(),
          "max ratio", ratio.max())
    assert (opened["goal_error"] > 0.01).all() and (ratio <= 0.05).all()
    assert (closed["clearance"] == np.inf).all()  # no scene


# ---- T5: saturation --------------------------------------------------------------------------------------------------


def test_saturation():
    """Bounds +-1, the plan's speed 1.0 exactly, the start 2 cm behind the plan along its heading: the feedback asks for
    more speed than the bound allows."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.tracking import track_batch

    dyn = "unicycle"
    rng = np.random.default_rng(21)
    U = rng.uniform(-0.5, 0.5, (B, N, 2))
    U[..., 0] = 1.0
    X = np.zeros((B, N + 1, 3))
    X[:, 0] = rng.uniform(-0.2, 0.2, (B, 3))
    X = host_track(dyn, X, U, None, None, DT, L, 1)[0]
    K, _ = host_tvlqr(dyn, X, U, DT, L, weights(3), 1.0, weights(3))
    dx0 = np.stack([-0.02 * np.cos(X[:, 0, 2]), -0.02 * np.sin(X[:, 0, 2]), np.zeros(B)], 1)
    p = problem(dyn, "rectangle")
    _, Ua, sat = host_track(dyn, X, U, K, dx0, DT, L, SUB, BOUNDS)
    v = _cpu(track_batch(p, X, U, K=K, dx0=dx0, substeps=SUB))
    print("saturated knots: gpu", v["saturated"].min(), v["saturated"].max(), "numpy", sat.min(), sat.max())
    assert (v["saturated"] >= 1).all() and (v["saturated"] == sat).all()
    assert ((v["flags"] & _abi.TRACK_SATURATED) != 0).all()
    assert (v["U_applied"] >= -1.0).all() and (v["U_applied"] <= 1.0).all()
    assert np.abs(v["U_applied"] - Ua).max() <= ROLL_TOL
    free = _cpu(track_batch(p, X, U, K=K, dx0=dx0, substeps=SUB, clamp=False))
    assert (free["saturated"] == 0).all() and not (free["flags"] & _abi.TRACK_SATURATED).any()
    assert (free["U_applied"].reshape(B, -1).max(1) > 1.0).all()


# ---- T6: one instance, any batch ----------------------------------------------------------------------------------------


def test_an_instance_does_not_depend_on_its_batch():
    from nlotrajectories_amd.tracking import track_batch, tvlqr_batch

    dyn = "unicycle_2nd"
    X, U, K, _, dx0 = case(dyn)[:5]
    p = problem(dyn, "rectangle")
    w = dict(q=weights(5), r=1.0, qf=weights(5))
    gains = lambda X, U: [t.cpu().numpy() for t in tvlqr_batch(p, X, U, **w)]  # noqa: E731
    track = lambda X, U, K, d: _cpu(track_batch(p, X, U, K=K, dx0=d, substeps=SUB))  # noqa: E731
    rv = lambda a: a[::-1].copy()  # noqa: E731
    gf, gr = gains(X, U), gains(rv(X), rv(U))
    tf, tr = track(X, U, K, dx0), track(rv(X), rv(U), rv(K), rv(dx0))
    for b in (0, 3, 17, B - 1):
        go = gains(X[b:b + 1], U[b:b + 1])
        for i, name in enumerate(("K", "P0", "status")):
            assert go[i][0].tobytes() == gf[i][b].tobytes() == gr[i][B - 1 - b].tobytes(), (b, name)
        to = track(X[b:b + 1], U[b:b + 1], K[b:b + 1], dx0[b:b + 1])
        for k in tf:
            assert to[k][0].tobytes() == tf[k][b].tobytes() == tr[k][B - 1 - b].tobytes(), (b, k)


# ---- T7: rejections -----------------------------------------------------------------------------------------------------


def _check_rejected(v, b, flag):
    assert v["flags"][b] == flag and not v["ok"][b]
    assert v["where"][b] == -1 and v["dev_where"][b] == -1 and v["saturated"][b] == -1
    for k in ("clearance", "deviation", "goal_error"):
        assert np.isnan(v[k][b]), k


def test_nonfinite_input():
    """A NaN in X, U, K, dx0 or xg of instance 1 of 3, one at a time: that instance is NONFINITE alone, the others are
    bitwise what they are without it.  The gains kernel rejects a NaN in X or U the same way."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.tracking import track_batch, tvlqr_batch

    dyn = "unicycle_2nd"
    p = problem(dyn, "rectangle")
    X, U, K, _, dx0 = (a[:3] for a in case(dyn)[:5])
    xg = X[:, -1]
    names = ("X", "U", "K", "dx0", "xg")
    run = lambda a: _cpu(track_batch(p, a["X"], a["U"], K=a["K"], dx0=a["dx0"], xg=a["xg"], substeps=SUB))  # noqa: E731
    clean_in = dict(zip(names, (X, U, K, dx0, xg)))
    clean = run(clean_in)
    assert not (clean["flags"] & _abi.TRACK_NONFINITE).any()
    for name in names:
        a = dict(clean_in)
        a[name] = a[name].copy()
        a[name][1].flat[a[name][1].size // 2] = np.nan
        v = run(a)
        _check_rejected(v, 1, _abi.TRACK_NONFINITE)
        for b in (0, 2):
            for k in v:
                assert v[k][b].tobytes() == clean[k][b].tobytes(), (name, b, k)
    w = dict(q=weights(5), r=1.0, qf=weights(5))
    gc = [t.cpu().numpy() for t in tvlqr_batch(p, X, U, **w)]
    for name in ("X", "U"):
        a = dict(X=X.copy(), U=U.copy())
        a[name][1].flat[7] = np.inf
        g = [t.cpu().numpy() for t in tvlqr_batch(p, a["X"], a["U"], **w)]
        assert g[2].tolist() == [0, _abi.TVLQR_NONFINITE, 0]
        assert (g[0][1] == 0).all() and np.isnan(g[1][1]).all()
        for b in (0, 2):
            assert all(g[i][b].tobytes() == gc[i][b].tobytes() for i in range(3)), (name, b)


def test_divergence():
    """Finite input, arithmetic overflow on valid memory.  Gains: a control of 1e200 makes A ~ 1e199 and P overflows
    (checked in numpy first): DIVERGED, K = 0, P0 = NaN.  Tracking: a gain of 1e307 times an offset of 100 overflows
    the control: DIVERGED, with the clamp on.  The neighbours are untouched."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.tracking import track_batch, tvlqr_batch

    dyn = "unicycle"
    p = problem(dyn, "rectangle")
    X, U, K, _, dx0 = (a[:3].copy() for a in case(dyn)[:5])
    w = dict(q=weights(3), r=1.0, qf=weights(3))
    gc = [t.cpu().numpy() for t in tvlqr_batch(p, X, U, **w)]
    Ub = U.copy()
    Ub[1, 5, 0] = 1e200
    Kh, Ph = host_tvlqr(dyn, X, Ub, DT, L, weights(3), 1.0, weights(3))
    assert not np.isfinite(Ph[1]).all() and np.isfinite(Ph[[0, 2]]).all()
    g = [t.cpu().numpy() for t in tvlqr_batch(p, X, Ub, **w)]
    assert g[2].tolist() == [0, _abi.TVLQR_DIVERGED, 0]
    assert (g[0][1] == 0).all() and np.isnan(g[1][1]).all()
    for b in (0, 2):
        assert all(g[i][b].tobytes() == gc[i][b].tobytes() for i in range(3)), b
    opened = _cpu(track_batch(p, X, U, dx0=dx0, substeps=SUB))
    zeroed = _cpu(track_batch(p, X, U, K=g[0], dx0=dx0, substeps=SUB))
    for k in opened:  # zero gains are the open loop
        assert zeroed[k][1].tobytes() == opened[k][1].tobytes(), k

    clean = _cpu(track_batch(p, X, U, K=K, dx0=dx0, substeps=SUB))
    K[1, 0, 0, 0], dx0[1, 0] = 1e307, 100.0
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float64(1e307) * np.float64(100.0))
    v = _cpu(track_batch(p, X, U, K=K, dx0=dx0, substeps=SUB))
    _check_rejected(v, 1, _abi.TRACK_DIVERGED)
    for b in (0, 2):
        for k in v:
            assert v[k][b].tobytes() == clean[k][b].tobytes(), (b, k)


# ---- T8: no scene -----------------------------------------------------------------------------------------------------------


def test_no_scene():
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.tracking import track_batch

    dyn = "unicycle_2nd"
    X, U, K, _, dx0 = case(dyn)[:5]
    p = problem(dyn, "rectangle")
    bare = p.with_(sdf="mlp", obstacles=[])
    v, s = _cpu(track_batch(bare, X, U, K=K, dx0=dx0, substeps=SUB)), _cpu(track_batch(p, X, U, K=K, dx0=dx0, substeps=SUB))
    assert (v["clearance"] == np.inf).all() and (v["where"] == -1).all()
    assert not (v["flags"] & (_abi.TRACK_COLLISION | _abi.TRACK_CONTAINS)).any()
    assert np.isfinite(s["clearance"]).all() and (s["where"] >= 0).all()
    for k in ("X_roll", "U_applied", "deviation", "dev_where", "goal_error", "saturated"):
        assert v[k].tobytes() == s[k].tobytes(), k
    check = case(dyn)
    assert np.abs(v["X_roll"] - check[5][:, ::SUB]).max() <= ROLL_TOL


# ---- T9: the CLI --------------------------------------------------------------------------------------------------------------


def test_cli_track_switch(tmp_path, capsys):
    """run_benchmark(track=True) on the b2 YAML prints five lines after everything it printed before (after --rollout's
    four); without the switch stdout has none of them, and the CSV row is the same either way (but the solver time)."""
    import re

    from nlotrajectories_amd.cli import run_benchmark

    f = os.path.join(CFG, "benchmark_2_unicycle_circle.yaml")
    out = {}
    for name, kw in (("plain", {}), ("track", dict(track=True)), ("both", dict(rollout=True, track=True))):
        d = tmp_path / name
        run_benchmark(f, initializer="linear", results_dir=str(d), metrics=False, **kw)
        txt = capsys.readouterr().out
        csvs = list(d.glob("*.csv"))
        out[name] = (txt.strip().split("\n"), csvs[0].read_text().strip().split("\n") if csvs else [])
    timeless = lambda line: re.sub(r"^(Computation time for the solver:).*", r"\1", line)  # noqa: E731
    plain, track, both = (out[k][0] for k in ("plain", "track", "both"))
    print("\n".join(both))
    assert not any(line.startswith("Tracking") for line in plain)
    assert [timeless(x) for x in track[:len(plain)]] == [timeless(x) for x in plain] and len(track) == len(plain) + 5
    assert [timeless(x) for x in both[:len(plain)]] == [timeless(x) for x in plain] and len(both) == len(plain) + 9
    assert all(line.startswith("Rollout") for line in both[-9:-5])
    for lines in (track, both):
        assert re.fullmatch(r"Tracking clearance: -?[0-9.e+-]+ at knot \d+", lines[-5])
        assert re.fullmatch(r"Tracking deviation: [0-9.e+-]+ at knot \d+", lines[-4])
        assert re.fullmatch(r"Tracking goal error: [0-9.e+-]+", lines[-3])
        assert re.fullmatch(r"Tracking saturated knots: \d+", lines[-2])
        assert re.fullmatch(r"Tracking collision-free: (True|False)", lines[-1])
    assert track[-5:] == both[-5:]  # the same solve, the same gains, the same closed loop
    drop_time = lambda row: [c for i, c in enumerate(row.split(",")) if i != 11]  # noqa: E731  (column 11: solver_time)
    for k in ("track", "both"):
        assert [drop_time(x) for x in out[k][1]] == [drop_time(x) for x in out["plain"][1]]
