"""rollout_batch (nlot_rollout_batch, csrc/nlot_rollout.hip) on the GPU: hand-derived values (a flow that hits what the
plan misses), the order of the integrator, parity of the rolled states of all six dynamics and of the rolled clearance
with the host (numpy sub-stepped RK4 on cli._f, scene.exact_sdf on the footprint points of the rolled poses),
independence of an instance from its batch, consistency with verify_batch, non-finite input and divergence, a problem
without a scene, solves end to end under Euler and RK4 defects, and the CLI switch.

Tolerances.  Rolled states against numpy: 1e-11 (<= 96 RK4 steps x ~50 flops x 1.1e-16 x growth <= e on O(1) states
is about 1.5e-12 in the worst case, rounded up).  The exact SDF is 1-Lipschitz in the point, so the clearance gets the
same 1e-11.  Hand-derived values (RK4 is exact on them): 1e-12."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "configs")
TOL = 1e-11
HAND = 1e-12

# ---- the host side: sub-stepped RK4 in numpy, the footprint points of the rolled poses, scene.exact_sdf ----------


def host_roll(p, x0, U, substeps):
    """All P = N substeps + 1 poses [B, P, nx] of the flow of cli._f from x0 [B, nx] under U [B, N, nu] held constant
    over each interval: classical RK4 steps of size h = dt / substeps."""
    from nlotrajectories_amd.cli import _f

    f = lambda x, u: _f(p, x.T, u.T).T  # noqa: E731  (cli._f is column-wise)
    h = p.dt / substeps
    x = np.array(x0, float)
    poses = [x]
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(U.shape[1]):
            u = U[:, k]
            for _ in range(substeps):
                k1 = f(x, u)
                k2 = f(x + 0.5 * h * k1, u)
                k3 = f(x + 0.5 * h * k2, u)
                k4 = f(x + h * k3, u)
                x = x + h * (k1 + 2 * k2 + 2 * k3 + k4) / 6
                poses.append(x)
    return np.stack(poses, 1)


def footprint_points(problem, poses, edge_points):
    """[P, npp, 2] for poses [P, nx]: the dot, or per edge the transformed corner and edge_points interior points at
    t = j / (edge_points + 1) (verify_batch's footprint; the heading is component 2 of the pose)."""
    if problem.shape == "dot":
        return poses[:, None, :2]
    body = np.array(problem.body)
    c, s = np.cos(poses[:, 2]), np.sin(poses[:, 2])
    wx = poses[:, 0, None] + c[:, None] * body[None, :, 0] - s[:, None] * body[None, :, 1]
    wy = poses[:, 1, None] + s[:, None] * body[None, :, 0] + c[:, None] * body[None, :, 1]
    W = np.stack([wx, wy], -1)
    pts = []
    for i in range(len(body)):
        p0, p1 = W[:, i], W[:, (i + 1) % len(body)]
        for j in range(edge_points + 1):
            t = j / (edge_points + 1)
            pts.append(p0 if j == 0 else (1 - t) * p0 + t * p1)
    return np.stack(pts, 1)


def host_pose_clearance(problem, obstacles, poses, edge_points):
    """Per-pose minimum [P] of scene.exact_sdf over the footprint points of poses [P, nx]."""
    from nlotrajectories_amd import scene

    pts = footprint_points(problem, poses, edge_points)
    return scene.exact_sdf(obstacles, pts[..., 0], pts[..., 1]).min(1)


def host_measures(X, poses, substeps, xg=None):
    """(deviation [B], dev_where [B], goal_error [B]) of the rolled knots poses[:, ::substeps] against the plan X."""
    knots = poses[:, ::substeps]
    d = np.hypot(knots[..., 0] - X[..., 0], knots[..., 1] - X[..., 1])
    g = X[:, -1] if xg is None else xg
    return d.max(1), d.argmax(1), np.hypot(knots[:, -1, 0] - g[:, 0], knots[:, -1, 1] - g[:, 1])


def check_clearance(v, b, per_pose):
    """Clearance to TOL; `where` by value: the host value at the GPU's pose index lies within TOL of the host minimum."""
    c, w = float(v["clearance"][b]), int(v["where"][b])
    print(f"  instance {b}: clearance gpu {c!r} host {per_pose.min()!r} where gpu {w} host {int(per_pose.argmin())}")
    assert abs(c - per_pose.min()) <= TOL
    assert 0 <= w < len(per_pose) and abs(per_pose[w] - per_pose.min()) <= TOL


def check_measures(v, X, poses, substeps, xg=None, rows=None):
    dev, dk, ge = host_measures(X, poses, substeps, xg)
    for b in range(len(X)) if rows is None else rows:
        print(f"  instance {b}: deviation gpu {float(v['deviation'][b])!r} host {dev[b]!r} at {int(v['dev_where'][b])} / "
              f"{int(dk[b])}, goal error gpu {float(v['goal_error'][b])!r} host {ge[b]!r}")
        assert abs(v["deviation"][b] - dev[b]) <= TOL and abs(v["goal_error"][b] - ge[b]) <= TOL
        k = int(v["dev_where"][b])
        d = np.hypot(*(poses[b, k * substeps, :2] - X[b, k, :2]))
        assert 0 <= k < X.shape[1] and abs(d - dev[b]) <= TOL


def random_trajectories(problem, B, seed):
    """xy uniform in [-0.2, 1.3]^2, theta uniform in [-pi, pi], the other states and the controls in [-0.5, 0.5] (the
    construction of the verification tests).  Only X[:, 0] and U matter to the rolled motion."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (B, problem.N + 1, problem.nx))
    X[..., :2] = rng.uniform(-0.2, 1.3, (B, problem.N + 1, 2))
    X[..., 2] = rng.uniform(-np.pi, np.pi, (B, problem.N + 1))
    U = rng.uniform(-0.5, 0.5, (B, problem.N, problem.nu))
    return X, U


def _cpu(v):
    return {k: t.cpu().numpy() for k, t in v.items()}


def _circle(c, r, m=0.0):
    return {"type": "circle", "center": tuple(c), "radius": r, "margin": m}


# ---- R1: the flow hits what the plan misses --------------------------------------------------------------------


def _r1():
    from nlotrajectories_amd.problem import Problem

    p = Problem(dynamics="point_2nd", shape="dot", N=2, dt=0.5, obstacles=[_circle((0.35, 0.0), 0.05)])
    X = np.array([[[0.0, 0, 0, 0], [0.0, 0, 0.5, 0], [0.25, 0, 1.0, 0]]])  # the Euler plan of U = (1, 0)
    U = np.tile([1.0, 0.0], (1, 2, 1))
    return p, X, U


@pytest.mark.parametrize("substeps,clearance,where,hit", [(1, 0.10, 2, False), (2, 0.01875, 3, False),
                                                          (3, 1 / 360 - 0.05, 5, True), (4, -0.0171875, 7, True)])
def test_flow_hits_what_the_plan_misses(substeps, clearance, where, hit):
    """R1: x(t) = t^2 / 2 under u = (1, 0) from rest, and RK4 is exact on it: the rolled knots are x = 0, 0.125, 0.5
    against the Euler plan's 0, 0, 0.25, so deviation = goal_error = 0.25 at knot 2.  The circle (0.35, 0), r 0.05
    lies beyond the plan's end; the flow crosses it between the knots: the poses at t = s / (2 substeps) come
    0.10 (t = 1), 0.01875 (t = 0.75), 1/360 - 0.05 (t = 5/6), -0.0171875 (t = 7/8) close."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.rollout import rollout_batch

    p, X, U = _r1()
    v = _cpu(rollout_batch(p, X, U, substeps=substeps))
    print("substeps", substeps, {k: v[k].tolist() for k in v})
    assert np.abs(v["X_roll"][0, :, 0] - [0.0, 0.125, 0.5]).max() <= HAND
    assert abs(v["deviation"][0] - 0.25) <= HAND and v["dev_where"][0] == 2
    assert abs(v["goal_error"][0] - 0.25) <= HAND
    assert abs(v["clearance"][0] - clearance) <= HAND and v["where"][0] == where
    assert bool(v["flags"][0] & _abi.ROLLOUT_COLLISION) == hit
    assert v["flags"][0] == (_abi.ROLLOUT_COLLISION if hit else 0) and bool(v["ok"][0]) == (not hit)


def test_the_plan_passes_verification_and_thresholds():
    """R1: verify_batch passes the same X, U (the Euler plan has no defect and stays 0.05 clear of the circle);
    deviation_tol = 0.2 and goal_tol = 0.3 set DEVIATION and not GOAL; against the flow's own end point the goal
    error vanishes."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.rollout import rollout_batch
    from nlotrajectories_amd.verify import verify_batch

    p, X, U = _r1()
    ver = _cpu(verify_batch(p, X, U, sub=8))
    print("verify", {k: ver[k].tolist() for k in ver})
    assert ver["flags"][0] == 0 and abs(ver["clearance"][0] - 0.05) <= HAND
    v = _cpu(rollout_batch(p, X, U, substeps=1, deviation_tol=0.2, goal_tol=0.3))
    assert v["flags"][0] == _abi.ROLLOUT_DEVIATION
    v = _cpu(rollout_batch(p, X, U, substeps=4, xg=np.array([[0.5, 0.0, 1.0, 0.0]]), goal_tol=0.3))
    print("goal error against the flow's end", float(v["goal_error"][0]))
    assert v["goal_error"][0] <= HAND and v["flags"][0] == _abi.ROLLOUT_COLLISION


# ---- R2: order ---------------------------------------------------------------------------------------------------


def test_fourth_order():
    """R2: a unicycle under u = (1, 1) from the origin drives the unit circle about (0, 1): after t = 1 it is at
    (sin 1, 1 - cos 1).  The numpy reference's error falls 16-fold per halving of h (2.10e-5, 1.30e-6, 8.13e-8, 5.08e-9
    at substeps 1, 2, 4, 8), and the GPU's end point is the reference's at every substeps.  No scene."""
    from nlotrajectories_amd.problem import Problem
    from nlotrajectories_amd.rollout import rollout_batch

    p = Problem(dynamics="unicycle", shape="dot", N=2, dt=0.5)
    X, U = np.zeros((1, 3, 3)), np.ones((1, 2, 2))
    exact = np.array([np.sin(1.0), 1.0 - np.cos(1.0)])
    err = []
    for substeps in (1, 2, 4, 8):
        host = host_roll(p, X[:, 0], U, substeps)[0, -1]
        v = _cpu(rollout_batch(p, X, U, substeps=substeps))
        err.append(np.hypot(*(host[:2] - exact)))
        print("substeps", substeps, "host error", err[-1], "gpu - host", np.abs(v["X_roll"][0, -1] - host).max())
        assert np.abs(v["X_roll"][0, -1] - host).max() <= TOL
    ratios = [err[i] / err[i + 1] for i in range(3)]
    print("ratios", ratios)
    assert all(12 <= r <= 20 for r in ratios)


# ---- R3: parity of the rolled states, all six dynamics ---------------------------------------------------------

ALL_DYNAMICS = ["point_1st", "point_2nd", "unicycle", "unicycle_2nd", "ackermann", "ackermann_2nd"]


def _r3(dynamics, B, N, shape=None):
    from nlotrajectories_amd.problem import Problem

    shape = shape or ("dot" if dynamics.startswith("point") else "rectangle")
    p = Problem(dynamics=dynamics, shape=shape, N=N, dt=0.1, wheelbase=0.5, control_bounds=((-1, 1), (-1, 1)),
                obstacles=[_circle((0.5, 0.5), 0.2)])
    rng = np.random.default_rng(5)
    U = rng.uniform(-0.5, 0.5, (B, N, 2))
    X = np.zeros((B, N + 1, p.nx))
    X[:, 0] = rng.uniform(-0.2, 0.2, (B, p.nx))
    return p, X, U


@pytest.mark.parametrize("dynamics", ALL_DYNAMICS)
def test_rolled_states_match_numpy(dynamics):
    """R3: B = 5 (the last lane group of a wave or block is partly past B), N = 6, substeps = 3, |u| <= 0.5; then the
    smallest call there is: N = 1, substeps = 1, B = 1."""
    from nlotrajectories_amd.rollout import rollout_batch

    for B, N, substeps in ((5, 6, 3), (1, 1, 1)):
        p, X, U = _r3(dynamics, B, N)
        poses = host_roll(p, X[:, 0], U, substeps)
        v = _cpu(rollout_batch(p, X, U, substeps=substeps))
        print(dynamics, "B", B, "max |X_roll - numpy|", np.abs(v["X_roll"] - poses[:, ::substeps]).max())
        assert np.abs(v["X_roll"] - poses[:, ::substeps]).max() <= TOL
        assert (v["X_roll"][:, 0] == X[:, 0]).all()
        check_measures(v, X, poses, substeps)
        for b in range(B):
            check_clearance(v, b, host_pose_clearance(p, p.obstacles, poses[b], 3))


def test_triangle_body_nine_footprint_points():
    """R3: a triangle with edge_points = 2 has 9 footprint points, not a power of two: a 16-lane group with 7 idle
    lanes."""
    from nlotrajectories_amd.rollout import rollout_batch

    p, X, U = _r3("unicycle_2nd", 5, 6, shape="triangle")
    X[:, 0, :2] += [0.35, 0.3]  # next to the circle
    poses = host_roll(p, X[:, 0], U, 3)
    v = _cpu(rollout_batch(p, X, U, substeps=3, edge_points=2))
    assert np.abs(v["X_roll"] - poses[:, ::3]).max() <= TOL
    for b in range(5):
        check_clearance(v, b, host_pose_clearance(p, p.obstacles, poses[b], 2))


# ---- R4: clearance parity in the scenes ------------------------------------------------------------------------

# (scene, dot body?, seed): N = 7, substeps = 3, edge_points = 2, B = 5.  The seeds were chosen on the CPU so that at
# least two rolled instances collide and at least two are clear (one of each is asserted below, on the host)
N4, SUB4, EP4, B4 = 7, 3, 2, 5
PARITY_CASES = [("b3", False, 10), ("b4", False, 1), ("b5", False, 1), ("b6", False, 0), ("b3", True, 2)]


def parity_problem(scene, dot):
    from nlotrajectories_amd.problem import BENCHMARKS

    p = BENCHMARKS[scene]["problem"].with_(N=N4)
    return p.with_(dynamics="point_2nd", shape="dot") if dot else p


@functools.lru_cache(maxsize=None)
def parity_case(scene, dot, seed):
    """(problem, X, U, poses [B, P, nx], per-pose clearance [B][P]) of a case, computed once on the host."""
    p = parity_problem(scene, dot)
    X, U = random_trajectories(p, B4, seed)
    poses = host_roll(p, X[:, 0], U, SUB4)
    host = [host_pose_clearance(p, p.obstacles, poses[b], EP4) for b in range(B4)]
    for a in (poses, *host):  # shared among the tests; X and U stay writable for torch, a test that edits them copies
        a.setflags(write=False)
    return p, X, U, poses, host


@pytest.mark.parametrize("scene,dot,seed", PARITY_CASES)
def test_rolled_clearance_matches_the_host_scene(scene, dot, seed):
    """R4: circles and squares (b3, b5), a non-convex polygon (b4), grouped trapezoids (b6) with their own bodies and
    dynamics, and b3 with a dot: 12 footprint points on 16 lanes, 1 on 1; B = 5 leaves lane groups past B."""
    from nlotrajectories_amd.rollout import rollout_batch

    p, X, U, poses, host = parity_case(scene, dot, seed)
    mins = np.array([h.min() for h in host])
    assert (mins < 0).sum() >= 1 and (mins > 0).sum() >= 1, mins
    v = _cpu(rollout_batch(p, X, U, substeps=SUB4, edge_points=EP4))
    print(scene, "max |X_roll - numpy|", np.abs(v["X_roll"] - poses[:, ::SUB4]).max())
    assert np.abs(v["X_roll"] - poses[:, ::SUB4]).max() <= TOL
    for b in range(B4):
        check_clearance(v, b, host[b])
    assert ((v["flags"] & 1) != 0).tolist() == (mins < 0).tolist()
    check_measures(v, X, poses, SUB4)


# ---- R5: one instance, any batch ---------------------------------------------------------------------------------


def test_an_instance_does_not_depend_on_its_batch():
    """R5: each instance of R4's b3 case rolled alone (B = 1) gives bitwise the outputs and the X_roll row it has in
    the B = 5 call and in the reversed batch."""
    from nlotrajectories_amd.rollout import rollout_batch

    p, X, U, _, _ = parity_case(*PARITY_CASES[0])
    kw = dict(substeps=SUB4, edge_points=EP4)
    full = _cpu(rollout_batch(p, X, U, **kw))
    rev = _cpu(rollout_batch(p, X[::-1].copy(), U[::-1].copy(), **kw))
    for b in range(B4):
        one = _cpu(rollout_batch(p, X[b:b + 1], U[b:b + 1], **kw))
        for k in full:
            assert one[k][0].tobytes() == full[k][b].tobytes() == rev[k][B4 - 1 - b].tobytes(), (b, k)


# ---- R6: consistency with verify_batch ---------------------------------------------------------------------------


def test_consistent_with_verify_at_one_substep():
    """R6: at substeps = 1 the rolled knots of an RK4 plan are the plan (its defect map is the rollout's step), so the
    deviation vanishes and the clearance is verify_batch's at sub = 1; an obstacle under the chassis is CONTAINS in
    both."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.problem import Problem
    from nlotrajectories_amd.rollout import rollout_batch
    from nlotrajectories_amd.verify import verify_batch

    p, X0, U, _, _ = parity_case(*PARITY_CASES[0])
    p = p.with_(integrator="rk4")
    X = host_roll(p, X0[:, 0], U, 1)
    v = _cpu(rollout_batch(p, X, U, substeps=1, edge_points=EP4))
    ver = _cpu(verify_batch(p, X, U, sub=1, edge_points=EP4))
    print("max |X_roll - X|", np.abs(v["X_roll"] - X).max(), "deviation", v["deviation"].tolist(), "defect",
          ver["defect"].tolist(), "clearance", v["clearance"].tolist(), ver["clearance"].tolist())
    assert np.abs(v["X_roll"] - X).max() <= TOL and (v["deviation"] <= TOL).all()
    assert (ver["defect"] <= TOL).all()
    assert np.abs(v["clearance"] - ver["clearance"]).max() <= 1e-12
    assert ((v["flags"] & _abi.ROLLOUT_COLLISION) != 0).tolist() == ((ver["flags"] & _abi.VERIFY_COLLISION) != 0).tolist()
    body = dict(dynamics="unicycle_2nd", shape="rectangle", length=0.2, width=0.1, N=1, integrator="rk4")
    X, U = np.zeros((1, 2, 5)), np.zeros((1, 1, 2))  # at rest
    for centre, inside in (((0.0, 0.0), True), ((0.5, 0.5), False)):
        q = Problem(obstacles=[_circle(centre, 0.01)], **body)
        v, ver = _cpu(rollout_batch(q, X, U, substeps=1)), _cpu(verify_batch(q, X, U, sub=1))
        print("pillar at", centre, "rollout flags", int(v["flags"][0]), "verify flags", int(ver["flags"][0]))
        assert v["flags"][0] == (_abi.ROLLOUT_CONTAINS if inside else 0)
        assert ver["flags"][0] == (_abi.VERIFY_CONTAINS if inside else 0)
        assert abs(v["clearance"][0] - ver["clearance"][0]) <= 1e-12


# ---- R7: non-finite input, divergence ---------------------------------------------------------------------------


def _check_rejected(v, b, flag):
    assert v["flags"][b] == flag and v["where"][b] == -1 and v["dev_where"][b] == -1 and not v["ok"][b]
    for k in ("clearance", "deviation", "goal_error"):
        assert np.isnan(v[k][b]), k


def test_nonfinite_input():
    """R7: one NaN in X of instance 1 of 3 flags that instance NONFINITE alone, with NaN outputs and -1 indices; the
    other two are what the host computes.  A non-finite control or goal is caught as well."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.rollout import rollout_batch

    p, X, U, poses, host = parity_case(*PARITY_CASES[0])
    X, U = X[:3].copy(), U[:3].copy()
    X[1, 4, 1] = np.nan
    v = _cpu(rollout_batch(p, X, U, substeps=SUB4, edge_points=EP4))
    _check_rejected(v, 1, _abi.ROLLOUT_NONFINITE)
    for b in (0, 2):
        check_clearance(v, b, host[b])
        assert np.abs(v["X_roll"][b] - poses[b, ::SUB4]).max() <= TOL
    check_measures(v, X, poses[:3], SUB4, rows=(0, 2))
    U[2, 0, 0] = np.inf
    xg = X[:, -1].copy()
    xg[0, 3] = np.nan
    v = _cpu(rollout_batch(p, X, U, xg=xg, substeps=SUB4, edge_points=EP4))
    assert v["flags"].tolist() == [_abi.ROLLOUT_NONFINITE] * 3


def test_divergence():
    """R7: a control of 1.7e308 is finite, so the input test passes; k1 + 2 k2 of the velocity overflows in the RK4
    sum and the rolled state is non-finite: DIVERGED alone, NaN outputs, -1 indices.  The neighbours are untouched."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.rollout import rollout_batch

    p, X, U, _, _ = parity_case(*PARITY_CASES[4])  # point_2nd
    X, U = X[:3].copy(), U[:3].copy()
    clean = _cpu(rollout_batch(p, X, U, substeps=SUB4))
    U[1, 2, 0] = 1.7e308
    assert not np.isfinite(host_roll(p, X[:, 0], U, SUB4)[1, -1]).all()
    v = _cpu(rollout_batch(p, X, U, substeps=SUB4))
    _check_rejected(v, 1, _abi.ROLLOUT_DIVERGED)
    for b in (0, 2):
        for k in v:
            assert v[k][b].tobytes() == clean[k][b].tobytes(), (b, k)


# ---- R8: no scene ------------------------------------------------------------------------------------------------


def test_no_scene():
    """R8: METRIC_PROBLEM carries no scene (n_obs == 0): clearance +inf, where -1, neither COLLISION nor CONTAINS; the
    deviation, the goal error and the rolled knots are those of the same call with b3's scene."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.problem import BENCHMARKS, METRIC_PROBLEM
    from nlotrajectories_amd.rollout import rollout_batch

    X, U = random_trajectories(METRIC_PROBLEM, 3, 11)
    v = _cpu(rollout_batch(METRIC_PROBLEM, X, U, deviation_tol=1e-3))
    s = _cpu(rollout_batch(METRIC_PROBLEM, X, U, obstacles=BENCHMARKS["b3"]["problem"].obstacles, deviation_tol=1e-3))
    print("no scene", {k: v[k].tolist() for k in v if k != "X_roll"})
    assert (v["clearance"] == np.inf).all() and (v["where"] == -1).all()
    assert (v["flags"] == _abi.ROLLOUT_DEVIATION).all()  # the random plan is not the flow: the threshold still works
    assert np.isfinite(s["clearance"]).all() and (s["where"] >= 0).all()
    for k in ("deviation", "dev_where", "goal_error", "X_roll"):
        assert v[k].tobytes() == s[k].tobytes(), k
    poses = host_roll(METRIC_PROBLEM, X[:, 0], U, 8)
    assert np.abs(v["X_roll"] - poses[:, ::8]).max() <= TOL
    check_measures(v, X, poses, 8)


# ---- R9: end to end ----------------------------------------------------------------------------------------------


def test_rk4_plans_roll_closer_than_euler_plans():
    """R9: four seeded b2 instances solved with Euler and with RK4 defects, both rolled at substeps = 8.  An instance
    solved under both deviates less from its RK4 plan than from its Euler plan, and the RK4 plans meet the solver's
    own defect bound.  No magnitude is fixed here (measured values: DESIGN.md §11)."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.problem import BENCHMARKS
    from nlotrajectories_amd.rollout import rollout_batch
    from nlotrajectories_amd.sampling import sample_start_goal
    from nlotrajectories_amd.solver import solve_batch
    from nlotrajectories_amd.verify import verify_batch

    p = BENCHMARKS["b2"]["problem"]
    sdf = lambda P: np.sqrt(((np.asarray(P) - 0.5) ** 2).sum(1)) - 0.25  # noqa: E731
    x0, xg = sample_start_goal(p, 4, seed=2, sdf=sdf, lo=(0, 0), hi=(1, 1))
    st, roll = {}, {}
    for integ in ("euler", "rk4"):
        q = p.with_(integrator=integ)
        r = solve_batch(q, x0, xg)
        st[integ] = r["status"].cpu().numpy()
        roll[integ] = _cpu(rollout_batch(q, r["X"], r["U"], xg=xg, substeps=8))
        print(integ, "status", st[integ].tolist(), "deviation", roll[integ]["deviation"].tolist(), "goal error",
              roll[integ]["goal_error"].tolist(), "clearance", roll[integ]["clearance"].tolist(), "flags",
              roll[integ]["flags"].tolist())
        if integ == "rk4":
            defect = verify_batch(q, r["X"], r["U"], x0=x0, xg=xg)["defect"].cpu().numpy()
            print("rk4 defect", defect.tolist())
    both = np.flatnonzero((st["euler"] == _abi.NLOT_SOLVED) & (st["rk4"] == _abi.NLOT_SOLVED))
    assert len(both) >= 1
    for b in both:
        assert roll["rk4"]["deviation"][b] < roll["euler"]["deviation"][b]
    assert (defect[st["rk4"] == _abi.NLOT_SOLVED] <= 1e-4).all()


# ---- R10: the CLI ------------------------------------------------------------------------------------------------


def test_cli_rollout_switch(tmp_path, capsys):
    """R10: run_benchmark(rollout=True) on the b2 YAML prints the four lines after everything it printed before, with
    verify=True after the three verification lines; without the switch stdout has none of them, and the CSV row is the
    same either way (but for the solver time)."""
    import re

    from nlotrajectories_amd.cli import run_benchmark

    f = os.path.join(CFG, "benchmark_2_unicycle_circle.yaml")
    out = {}
    for name, kw in (("plain", {}), ("rollout", dict(rollout=True)), ("both", dict(rollout=True, verify=True))):
        d = tmp_path / name
        run_benchmark(f, initializer="linear", results_dir=str(d), metrics=False, **kw)
        txt = capsys.readouterr().out
        csvs = list(d.glob("*.csv"))
        out[name] = (txt.strip().split("\n"), csvs[0].read_text().strip().split("\n") if csvs else [])
    timeless = lambda line: re.sub(r"^(Computation time for the solver:).*", r"\1", line)  # noqa: E731
    plain, roll, both = (out[k][0] for k in ("plain", "rollout", "both"))
    print("\n".join(both))
    assert not any(line.startswith("Rollout") for line in plain)
    assert [timeless(x) for x in roll[:len(plain)]] == [timeless(x) for x in plain] and len(roll) == len(plain) + 4
    assert [timeless(x) for x in both[:len(plain)]] == [timeless(x) for x in plain] and len(both) == len(plain) + 7
    assert re.match(r"Exact clearance", both[-7]) and re.match(r"Max dynamics defect", both[-6])
    assert re.match(r"Collision-free", both[-5])
    for lines in (roll, both):
        assert re.fullmatch(r"Rollout clearance: -?[0-9.e+-]+ at knot \d+", lines[-4])
        assert re.fullmatch(r"Rollout deviation: [0-9.e+-]+ at knot \d+", lines[-3])
        assert re.fullmatch(r"Rollout goal error: [0-9.e+-]+", lines[-2])
        assert re.fullmatch(r"Rollout collision-free: (True|False)", lines[-1])
    assert roll[-4:] == both[-4:]  # the same solve, the same rollout
    drop_time = lambda row: [c for i, c in enumerate(row.split(",")) if i != 11]  # noqa: E731  (column 11: solver_time)
    for k in ("rollout", "both"):
        assert [drop_time(x) for x in out[k][1]] == [drop_time(x) for x in out["plain"][1]]
