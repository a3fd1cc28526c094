"""GPU batched solver vs the CPU oracle (same NLP, same algorithm, same inputs).

Parity is stated at three levels:
  1. iterates: after k accepted steps (max_iter = k) the GPU and oracle iterates agree to 1e-7 (fp64
     analytic SDF) / 1e-4 (fp32 learned SDF, k <= 3) — the algorithm is the same step for step;
  2. final cost: within 1e-4 relative (BASELINE.json north_star) for every instance both solve into the
     same basin (>= 80 % of them; rounding differences amplified along a nonconvex path can end a few
     instances in a neighbouring local minimum, as two IPOPT builds would);
  3. status: the same outcome on >= 90 % of instances.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _oracle():
    import oracle as O

    return O


STRATEGIES = {"adaptive": {}, "monotone": dict(mu_strategy=0, barrier_tol_factor=10.0)}
# iterate parity also for the variable-bound form (the default is the reference's constraint-row bounds)
ITER_STRATEGIES = {**STRATEGIES, "adaptive_varbounds": dict(general_bounds=0),
                   "monotone_varbounds": dict(mu_strategy=0, barrier_tol_factor=10.0, general_bounds=0)}


@pytest.mark.parametrize("strategy", list(ITER_STRATEGIES))
def test_iterates_match_oracle_b2(strategy):
    O = _oracle()
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.problem import BENCHMARKS
    from nlotrajectories_amd.solver import solve_batch

    b = BENCHMARKS["b2"]
    for k in (1, 2, 5, 10, 20):
        opt = _abi.gpu_options(max_iter=k, **ITER_STRATEGIES[strategy])
        rg = solve_batch(b["problem"], np.array([b["start"]]), np.array([b["goal"]]), options=opt)
        rc = O.solve_one(b["problem"], b["start"], b["goal"], opt=opt)
        assert rg["iters"][0].item() == rc["iters"] == k
        dx = {n: np.abs(rg[n][0].cpu().numpy() - rc[n]).max() for n in ("X", "U", "S")}
        xp = np.array(b["start"], float)
        xp[0] += 1e-13
        rp = O.solve_one(b["problem"], xp, b["goal"], opt=opt)
        sens = max(float(np.abs(rp[n] - rc[n]).max()) for n in ("X", "U", "S"))
        print(strategy, "k", k, "max |gpu - oracle|", dx, "oracle sensitivity", sens)
        # fp64 on both sides; summation orders differ, and the differences grow along the nonconvex path as the
        # oracle's own response to a 1e-13 change of the start does (2.2e-7 at k = 20 with the constraint rows)
        tol = max(1e-7 if k <= 10 else 1e-6, 20 * sens)
        for n in dx:
            assert dx[n] <= tol, (k, n, dx[n])


@pytest.mark.parametrize("strategy", list(ITER_STRATEGIES))
def test_iterates_match_oracle_learned(artefact, strategy):
    O = _oracle()
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.ops import DeviceMlp
    from nlotrajectories_amd.problem import METRIC_PROBLEM
    from nlotrajectories_amd.solver import solve_batch

    mlp, hm = DeviceMlp(artefact), O.HostMlp(artefact)
    x0, xg = [0, 0, 0.785, 0, 0], [1, 1, 0.785, 0, 0]
    for k in (1, 3):
        opt = _abi.gpu_options(max_iter=k, **ITER_STRATEGIES[strategy])
        rg = solve_batch(METRIC_PROBLEM, np.array([x0]), np.array([xg]), mlp=mlp, options=opt)
        rc = O.solve_one(METRIC_PROBLEM, x0, xg, hm, opt=opt)
        np.testing.assert_allclose(rg["X"][0].cpu().numpy(), rc["X"], atol=1e-4)
        np.testing.assert_allclose(rg["U"][0].cpu().numpy(), rc["U"], atol=1e-4)


@pytest.mark.parametrize("strategy", ["adaptive", "adaptive_tol1e-8", "monotone"])
def test_batch_b2_analytic_matches_oracle(strategy):
    """64 seeded b2 instances (analytic SDF).  Adaptive mu at the reference's tol 1e-4 (runner.py:117-120), adaptive mu at
    tol 1e-8, monotone mu at tol 1e-4.  Solve-level parity split by the oracle's own reproducibility
    (tests/outcomes.py): on the instances whose oracle outcome is unchanged by fp64-sized perturbations of the start
    (x0 +- {1, 2, 3, 4}e-13 on x and y) the GPU gives the same status and a final cost within 1e-4 on 100 %; on the
    rest, status agreement at least the lowest perturbed oracle run's."""
    O = _oracle()
    from outcomes import WIDE, check_outcome_parity, oracle_outcomes
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.problem import BENCHMARKS
    from nlotrajectories_amd.sampling import sample_start_goal
    from nlotrajectories_amd.solver import solve_batch

    p = BENCHMARKS["b2"]["problem"]
    sdf = lambda P: np.sqrt(((np.asarray(P) - 0.5) ** 2).sum(1)) - 0.25
    x0, xg = sample_start_goal(p, 64, seed=1, sdf=sdf, lo=(0, 0), hi=(1, 1))
    tight = dict(tol=1e-8, constr_viol_tol=1e-8, compl_inf_tol=1e-8) if strategy == "adaptive_tol1e-8" else {}
    opt = _abi.gpu_options(**STRATEGIES[strategy.split("_")[0]], **tight)
    rg = solve_batch(p, x0, xg, options=opt)
    out = oracle_outcomes(O, p, x0, xg, opt=opt)
    sg, cg = rg["status"].cpu().numpy(), rg["cost"].cpu().numpy()
    info = check_outcome_parity(f"b2 {strategy}", sg, cg, out,
                                min_reproducible={"adaptive": 4, "adaptive_tol1e-8": 6, "monotone": 1}[strategy],
                                widen=lambda i: oracle_outcomes(O, p, x0[i], xg[i], opt=opt, perturbations=WIDE))
    assert ((sg == 0) & (out["status"][0] == 0)).sum() >= 0.5 * len(x0), info


def test_batch_learned_sdf_matches_oracle(artefact):
    """The metric workload (learned SDF, the reference's settings: tol 1e-4, max_iter 1000, adaptive mu, restoration,
    the bounds as constraint rows) on the 128 seeded instances of tests/golden/oracle_outcomes.npz, whose oracle
    outcomes under the fixture's 20 runs (x0, x0 +- 1e-13 e_x, e_y, 15 other orders of the net's fp32 sums) the
    fixture holds (tests/golden/make_oracle_outcomes.py).  Split parity (tests/outcomes.py), per net on its own
    (seq: the oracle's summation order; f32 and the product's split-bf16 MFMA nets): identical status and final cost
    within 1e-4 on every oracle-reproducible instance; on the chaotic ones a status agreement at least the lowest of
    the 19 perturbed runs'."""
    import os

    import oracle as O
    from outcomes import WIDE, net_parity, oracle_outcomes
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.ops import DeviceMlp
    from nlotrajectories_amd.problem import METRIC_PROBLEM
    from nlotrajectories_amd.solver import solve_batch

    f = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_outcomes.npz")))
    out = {k: f[f"metric_{k}"] for k in ("status", "cost", "iters", "xdev")}
    opt = _abi.gpu_options(general_bounds=int(f["general_bounds"]))
    hm = O.HostMlp(artefact)
    widen = lambda i: oracle_outcomes(O, METRIC_PROBLEM, f["metric_x0"][i], f["metric_xg"][i], hm, opt=opt,
                                      perturbations=WIDE)
    res, sol = {}, {}
    for arith in ("seq", "f32", "split_bf16"):
        rg = solve_batch(METRIC_PROBLEM, f["metric_x0"], f["metric_xg"], mlp=DeviceMlp(artefact, arith), options=opt)
        res[arith] = (rg["status"].cpu().numpy(), rg["cost"].cpu().numpy())
        sol[arith] = {k: rg[k].cpu().numpy() for k in ("X", "U", "S")}
        print("metric", arith, "GPU status counts", np.bincount(res[arith][0], minlength=7).tolist(), "oracle",
              np.bincount(out["status"][0], minlength=7).tolist(), flush=True)

    def feasible(arith, i):  # every constraint of the NLP (runner.py:50-103) at the GPU's point, to 1e-4
        X, U, S = (sol[arith][k][i] for k in ("X", "U", "S"))
        p, x0, xg = METRIC_PROBLEM, f["metric_x0"][i], f["metric_xg"][i]
        term = [j for j in range(p.nx) if j != 2]
        F = X[:-1] + p.dt * np.stack([O.dynamics(p, X[k], U[k]) for k in range(p.N)])
        c = np.concatenate([O.corners(p, X[k]) for k in range(p.N + 1)])
        v, _, _ = O.mlp_eval(hm, c, want=False)
        d = np.array([O.soft_min(v[4 * k:4 * k + 4], p.softmin_alpha) for k in range(p.N + 1)])
        (lo0, hi0), (lo1, hi1) = p.control_bounds
        viol = max(np.abs(X[0] - x0).max(), np.abs(X[-1, term] - xg[term]).max(), np.abs(X[1:] - F).max(),
                   -(d + S).min(), -S.min(), (lo0 - U[:, 0]).max(), (U[:, 0] - hi0).max(), (lo1 - U[:, 1]).max(),
                   (U[:, 1] - hi1).max())
        print(f"[parity] metric {arith} instance {i}: cost beyond the oracle's envelope, max constraint violation "
              f"{viol:.2e}", flush=True)
        return viol <= 1e-4

    net_parity("metric (128, max_iter 1000)", out, res, min_reproducible=16, widen=widen, feasible=feasible)


def test_safeguards_iterate_parity(artefact):
    """Second-order corrections on the GPU: two seeded metric instances whose first 10 iterations try 1 and 2
    corrections (oracle counts); GPU and oracle iterates after k iterations agree to 20x the oracle's own
    response to a 1e-13 change of x0 (1e-6 floor)."""
    O = _oracle()
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.ops import DeviceMlp
    from nlotrajectories_amd.problem import METRIC_PROBLEM
    from nlotrajectories_amd.solver import solve_batch

    mlp, hm = DeviceMlp(artefact), O.HostMlp(artefact)
    cases = [([1.005365686594, -0.295618399728, 2.030163010282, 0.0, 0.0],
              [0.739845159389, 0.241155138369, 2.030163010282, 0.0, 0.0]),
             ([0.867448714288, -0.018951007036, 2.54865910057, 0.0, 0.0],
              [-0.040290170163, 0.592694980049, 2.54865910057, 0.0, 0.0])]
    socs = 0
    for x0, xg in cases:
        x0, xg = np.array(x0), np.array(xg)
        for k in (5, 10):
            opt = _abi.gpu_options(max_iter=k)
            rg = solve_batch(METRIC_PROBLEM, x0[None], xg[None], mlp=mlp, options=opt)
            rc = O.solve_one(METRIC_PROBLEM, x0, xg, hm, opt=opt)
            xp = x0.copy()
            xp[0] += 1e-13
            rp = O.solve_one(METRIC_PROBLEM, xp, xg, hm, opt=opt)
            sens = max(float(np.abs(rp[n] - rc[n]).max()) for n in ("X", "U"))
            d = max(float(np.abs(rg[n][0].cpu().numpy() - rc[n]).max()) for n in ("X", "U"))
            print("k", k, "status", rc["status"], "gpu-oracle", d, "oracle sensitivity", sens, "SOC tried", rc["soc_tried"])
            assert rg["status"][0].item() == rc["status"] and rg["iters"][0].item() == rc["iters"]
            assert d <= max(1e-6, 20 * sens)
        socs += rc["soc_tried"]
    assert socs >= 2


@pytest.mark.parametrize("form", ["rows", "varbounds"])
def test_tiny_step_rule_matches_oracle(form):
    """IPOPT's tiny-step rule, made to fire with a large tiny_step_tol: full steps without a line search, and
    STOP_AT_TINY_STEP after two in a row — same iterations and status on the GPU and in the oracle.  The
    start/goal pair runs along the top edge of the square, clear of the obstacle: a well-conditioned path whose
    outcome the oracle reproduces under +-1e-13 changes of the start's x and y in both bound forms (constraint rows:
    STOP_AT_TINY_STEP at 7 iterations, 41 to solve without the rule; variable bounds: 33 and 291).  (The round-4 pair
    (0, 0.924) -> (1, 0.98) is chaotic with the constraint rows: the oracle stops at 29 or solves at 82 / 99 under
    1e-13 changes; pairs grazing the obstacle reach delta_w = 1e6 in their first iteration, where the GPU's and the
    oracle's summation orders part.)"""
    O = _oracle()
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.problem import BENCHMARKS
    from nlotrajectories_amd.solver import solve_batch

    b = BENCHMARKS["b2"]
    th = float(np.arctan2(0.97 - 0.93, 0.9))
    x0, xg = [0.1, 0.93, th, 0.0, 0.0], [1.0, 0.97, th, 0.0, 0.0]
    opt = _abi.gpu_options(tiny_step_tol=0.05, tiny_step_y_tol=1e3, general_bounds=1 if form == "rows" else 0)
    rg = solve_batch(b["problem"], np.array([x0]), np.array([xg]), options=opt)
    rc = O.solve_one(b["problem"], x0, xg, opt=opt)
    print("tiny: oracle", rc["status"], rc["iters"], rc["tiny_steps"], "gpu", rg["status"][0].item(),
          rg["iters"][0].item(), "dX", float(np.abs(rg["X"][0].cpu().numpy() - rc["X"]).max()))
    assert rc["status"] == _abi.NLOT_TINY_STEP and rc["tiny_steps"] >= 2
    assert rg["status"][0].item() == rc["status"] and rg["iters"][0].item() == rc["iters"]
    np.testing.assert_allclose(rg["X"][0].cpu().numpy(), rc["X"], atol=1e-6)


def test_solution_satisfies_constraints():
    """Every instance reported solved satisfies the NLP's equalities and (constraint rows) bounds to 1e-4
    (constr_viol_tol)."""
    O = _oracle()
    from nlotrajectories_amd.problem import BENCHMARKS
    from nlotrajectories_amd.sampling import sample_start_goal
    from nlotrajectories_amd.solver import solve_batch

    p = BENCHMARKS["b2"]["problem"]
    sdf = lambda P: np.sqrt(((np.asarray(P) - 0.5) ** 2).sum(1)) - 0.25
    x0, xg = sample_start_goal(p, 32, seed=2, sdf=sdf, lo=(0, 0), hi=(1, 1))
    r = solve_batch(p, x0, xg)
    X, U, S, st = (r[k].cpu().numpy() for k in ("X", "U", "S", "status"))
    for b in np.where(st == 0)[0]:
        assert np.abs(X[b, 0] - x0[b]).max() < 1e-4
        term = [i for i in range(5) if i != 2]
        assert np.abs(X[b, -1, term] - xg[b, term]).max() < 1e-4
        for k in range(p.N):
            F = X[b, k] + p.dt * O.dynamics(p, X[b, k], U[b, k])
            assert np.abs(X[b, k + 1] - F).max() < 1e-4
        assert (U[b] >= -2 - 1e-4).all() and (U[b] <= 2 + 1e-4).all() and (S[b] >= -1e-4).all()


@pytest.mark.parametrize("case", ["metric", "b2", "b2_many_waves"])
def test_continuous_batching_same_results(artefact, case):
    """NlotSolverOptions.max_active < B (continuous batching: at most max_active instances in flight, the next
    ones admitted as others finish) gives every instance the same status, iterations, cost and trajectory as
    the all-at-once solve, bitwise: an instance's arithmetic does not depend on which others share its steps."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.ops import DeviceMlp
    from nlotrajectories_amd.problem import BENCHMARKS, METRIC_PROBLEM
    from nlotrajectories_amd.sampling import sample_start_goal
    from nlotrajectories_amd.solver import solve_batch

    if case == "metric":
        p, mlp = METRIC_PROBLEM, DeviceMlp(artefact)
        tm = artefact.torch_module()
        sdf = lambda P: tm(torch.tensor(np.asarray(P), dtype=torch.float32)).detach().numpy()[:, 0]
        x0, xg = sample_start_goal(p, 160, seed=3, sdf=sdf)
        slots = 40
    else:
        p, mlp = BENCHMARKS["b2"]["problem"], None
        sdf = lambda P: np.sqrt(((np.asarray(P) - 0.5) ** 2).sum(1)) - 0.25
        x0, xg = sample_start_goal(p, 64 if case == "b2_many_waves" else 48, seed=4, sdf=sdf, lo=(0, 0), hi=(1, 1))
        slots = 2 if case == "b2_many_waves" else 7
    # b2_many_waves: 32 admission waves of 2 instances at max_iter 5: the global step cap is per
    # admission wave, so no instance is left unadmitted
    kw = dict(max_iter=5) if case == "b2_many_waves" else {}
    ra = solve_batch(p, x0, xg, mlp=mlp, options=_abi.gpu_options(**kw))
    rc = solve_batch(p, x0, xg, mlp=mlp, options=_abi.gpu_options(max_active=slots, **kw))
    if case == "b2_many_waves":
        assert (rc["iters"] > 0).all()
    print(case, "statuses", np.bincount(ra["status"].cpu().numpy(), minlength=7).tolist())
    for k in ("status", "iters", "cost", "X", "U", "S"):
        assert torch.equal(ra[k], rc[k]), k


@pytest.mark.parametrize("knobs", [
    # the default caps every k_ric launch at one delta_w attempt (a wrong inertia continues in the next step's launch);
    # uncapped: every attempt in one launch (the default below 2048 active instances until round 5)
    {"NLOT_RIC_TRIES_MIN": "100000000"},
    {"NLOT_RIC_TRIES_MIN": "100000000", "NLOT_RESTO_TRIES": "0"},  # uncapped, the restoration solves too
    {"NLOT_RESTO_TRIES": "0"},                               # capped Newton solves, uncapped restoration solves
    {"NLOT_RESTO_BOUND": "1"},                               # restoration grids of one instance: the stride path
    {"NLOT_SOC_FORK": "1"}, {"NLOT_SOC_FORK": "2"},          # correction chain forked at the step start / after the MLP
    {"NLOT_EARLY_VALUE": "0"},                               # no early value launch (default on since round 4)
    {"NLOT_SPEC_THRESHOLD": "100000", "NLOT_SPEC_BULK": "4"},
    {"NLOT_STEP_KERNEL": "0"},                               # counter copies as D2H / fill / D2D instead of k_step_end
    {"NLOT_PIPE": "1"},                                      # the host synchronises after every step
    {"NLOT_MLP_REUSE": "0"},                                 # the full MLP launch recomputes every forward
    {"NLOT_STREAM_PRIO": "2"},                               # restoration and correction streams at the highest priority
    {"NLOT_RIC_TRIES": "3"},                                 # up to three delta_w attempts per k_ric launch
])
def test_scheduling_knobs_same_results(artefact, knobs, monkeypatch):
    """The solver's scheduling (attempt cap per launch, stream layout, speculation) changes when an instance's work
    runs, never its arithmetic: statuses, iterations, costs and trajectories are bitwise those of the defaults."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.ops import DeviceMlp
    from nlotrajectories_amd.problem import METRIC_PROBLEM
    from nlotrajectories_amd.sampling import sample_start_goal
    from nlotrajectories_amd.solver import solve_batch

    mlp = DeviceMlp(artefact)
    tm = artefact.torch_module()
    sdf = lambda P: tm(torch.tensor(np.asarray(P), dtype=torch.float32)).detach().numpy()[:, 0]
    x0, xg = sample_start_goal(METRIC_PROBLEM, 96, seed=5, sdf=sdf)
    opt = _abi.gpu_options(max_iter=300, max_active=48)
    ra = solve_batch(METRIC_PROBLEM, x0, xg, mlp=mlp, options=opt)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    rb = solve_batch(METRIC_PROBLEM, x0, xg, mlp=mlp, options=opt)
    for k in ("status", "iters", "cost", "X", "U", "S"):
        assert torch.equal(ra[k], rb[k]), (knobs, k)


def test_sampled_timing_stats(artefact):
    """nlot_set_timing(k) (ABI v14): the per-launch event sums cover one global step in k, NlotSolveStats.timed_* count
    those steps and their work; every step (k = 1) times everything; timing never changes the results."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.ops import DeviceMlp
    from nlotrajectories_amd.problem import METRIC_PROBLEM
    from nlotrajectories_amd.sampling import sample_start_goal
    from nlotrajectories_amd.solver import last_stats, set_timing, solve_batch

    mlp = DeviceMlp(artefact)
    tm = artefact.torch_module()
    sdf = lambda P: tm(torch.tensor(np.asarray(P), dtype=torch.float32)).detach().numpy()[:, 0]
    x0, xg = sample_start_goal(METRIC_PROBLEM, 64, seed=6, sdf=sdf)
    opt = _abi.gpu_options(max_iter=200, max_active=32)
    runs = {}
    try:
        for k in (0, 1, 4):
            set_timing(k)
            runs[k] = (solve_batch(METRIC_PROBLEM, x0, xg, mlp=mlp, options=opt), last_stats())
    finally:
        set_timing(0)
    for k in (1, 4):
        for f in ("status", "iters", "cost", "X", "U"):
            assert torch.equal(runs[0][0][f], runs[k][0][f]), (k, f)
    s0, s1, s4 = runs[0][1], runs[1][1], runs[4][1]
    assert s0["timed_steps"] == 0 and s0["mlp_full_ms"] == 0
    assert s1["timing_every"] == 1 and s1["timed_steps"] == s1["iterations"]
    for f in ("points_full", "points_full_reused", "points_value"):
        assert s1[f"timed_{f}"] == s1[f"mlp_{f}"], f
    assert s1["timed_ric_solves"] == s1["ric_solves"]
    n = s4["iterations"]
    want = sum(1 for s in range(n) if s % 4 == (s // 4) % 4)
    assert s4["timing_every"] == 4 and s4["timed_steps"] == want, (s4["timed_steps"], want, n)
    assert 0 < s4["timed_points_full"] < s4["mlp_points_full"] and 0 < s4["timed_points_value"] < s4["mlp_points_value"]
    assert s4["mlp_full_ms"] > 0 and s4["mlp_value_ms"] > 0 and s4["ric_ms"] > 0 and s4["iterate_ms"] > 0
