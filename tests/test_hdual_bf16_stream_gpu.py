"""NLOT_MLP_ARITH_HDUAL_BF16_STREAM (DeviceMlp(w, "hdual_bf16_stream"), kernel mlp_hdual_bf16_stream): the split-bf16
hyper-dual products with the split activations in LDS and the split HxH weights streamed from L2, for smooth nets of
H = 128 and 256 with 1-4 HxH layers.  Checked against torch fp64 autograd of the same module with the tolerances of
tests/test_smooth_mlp.py (value 2e-5 absolute, gradient and Hessian 2e-5 of their largest entry, 5e-5 for SIREN); the
fp32 oracle's own error is printed beside the kernel's, and meets the same tolerances on these nets and points on the
CPU (test_oracle_meets_tolerances: the condition on the inputs)."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch
from test_smooth_mlp import _check, _nets, _torch_f64

# name -> HxH layers: one layer at NQ = 4 under sine, _nets()'s 2-256x3-1, the depth limit at H = 256, H = 128 with 3
# layers, the depth limit there with a Fourier input layer, and the smallest shape "hdual_bf16" refuses
NETS = {"siren_256": 1, "mlp_tanh_256x3": 2, "mlp_sigmoid_256x5": 4, "mlp_tanh_128x4": 3, "fourier_leaky_128x6": 4,
        "mlp_tanh_128x3": 2}
# one lane group's point, a full point group, a ragged one, one past the largest block tile (64 points in value
# launches; 16 or 32 in full ones, which 17 and 65 are past as well), many tiles
POINTS = (1, 16, 17, 65, 1000)


def _weights(name):
    from nlotrajectories_amd.nn import SIREN, FourierMLP, MlpWeights, MultiLayerPerceptron

    # seeds torch; the nets of test_hdual_stream_gpu.py follow in its order (the same weights), then the new one
    nets = _nets()
    nets["siren_256"] = SIREN(2, 256, 1, num_layers=3, omega_0=30)
    nets["mlp_sigmoid_256x5"] = MultiLayerPerceptron(2, 256, 1, 5, "Sigmoid")
    nets["mlp_tanh_128x4"] = MultiLayerPerceptron(2, 128, 1, 4, "Tanh")
    nets["fourier_leaky_128x6"] = FourierMLP(2, 128, 1, num_layers=6, scale=2.0, activation_function="leaky_relu")
    nets["mlp_tanh_128x3"] = MultiLayerPerceptron(2, 128, 1, 3, "Tanh")
    w = MlpWeights.from_module(nets[name])
    assert w.n_hidden == NETS[name]
    return w


@functools.lru_cache(maxsize=None)
def _cases(name):
    """[(points, lambda, torch fp64 reference, fp32 oracle)] per P, from one seeded stream; computed once."""
    import oracle as O

    w, rng, out = _weights(name), np.random.default_rng(2), []
    for P in POINTS:
        pts = rng.uniform(-0.5, 1.5, (P, 2)).astype(np.float32)
        lam = rng.uniform(-2, 2, P).astype(np.float32)
        ov, og, oh = O.mlp_eval(O.HostMlp(w), pts)
        out.append((pts, lam, _torch_f64(w, pts), (ov, og, oh.reshape(-1, 2, 2))))
    return out


@pytest.mark.parametrize("name", list(NETS))
def test_oracle_meets_tolerances(name):
    for _, _, ref, orc in _cases(name):
        _check(*orc, ref, 5e-5 if "siren" in name else 2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_kernel_hdual_bf16_stream_matches_torch_f64(name):
    from nlotrajectories_amd.ops import DeviceMlp, sdf_mlp_eval

    dm = DeviceMlp(_weights(name), "hdual_bf16_stream")
    tol = 5e-5 if "siren" in name else 2e-5
    for pts, lam, ref, orc in _cases(name):
        pt = torch.tensor(pts, device="cuda")
        v, g, h = (t.cpu().numpy() for t in sdf_mlp_eval(dm, pt))
        va, ga, ha = (t.cpu().numpy() for t in sdf_mlp_eval(dm, pt, lam=torch.tensor(lam, device="cuda")))
        vv = sdf_mlp_eval(dm, pt, derivatives=False)[0].cpu().numpy()
        for what, k, o, r in zip(("value", "grad", "hess"), (v, g, h), orc, ref):
            print(f"{name} P={len(pts)} {what}: kernel {np.abs(k - r).max():.3e} oracle {np.abs(o - r).max():.3e}"
                  f" of {np.abs(r).max():.3e}")
        np.testing.assert_array_equal(vv, v)  # the value-only launch is bitwise the full launch's value
        np.testing.assert_array_equal(va, v)
        np.testing.assert_array_equal(h[:, 0, 1], h[:, 1, 0])
        _check(v, g, h, ref, tol)
        _check(va, ga, ha, (ref[0], lam[:, None] * ref[1], lam[:, None, None] * ref[2]), tol)


@pytest.mark.gpu
def test_solver_iterates_hdual_bf16_stream():
    """A seeded 2-256-256-1 net under tanh, its zero level put through the midpoint of the straight path, on the
    streamed split-bf16 kernel (the solver's launches address points through n_dev / P_per / ld): the Newton iterates
    after k = 1, 3 equal the oracle's to 1e-4, or to 20x the oracle's own response to a 1e-13 perturbation of the start
    where that is larger."""
    import oracle as O
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.nn import MlpWeights
    from nlotrajectories_amd.ops import DeviceMlp
    from nlotrajectories_amd.problem import METRIC_PROBLEM
    from nlotrajectories_amd.solver import solve_batch

    w = dataclasses.replace(MlpWeights.random_relu_mlp(256, 1), act=_abi.ACT_TANH)
    w.b_out = -float(O.mlp_eval(O.HostMlp(w), np.array([[0.5, 0.5]], np.float32))[0][0])
    mlp, hm = DeviceMlp(w, "hdual_bf16_stream"), O.HostMlp(w)
    x0, xg = np.array([0, 0, 0.785, 0, 0], float), np.array([1, 1, 0.785, 0, 0], float)
    for k in (1, 3):
        opt = _abi.gpu_options(max_iter=k)
        rg = solve_batch(METRIC_PROBLEM, x0[None], xg[None], mlp=mlp, options=opt)
        rc = O.solve_one(METRIC_PROBLEM, x0, xg, hm, opt=opt)
        rp = O.solve_one(METRIC_PROBLEM, x0 + [1e-13, 0, 0, 0, 0], xg, hm, opt=opt)
        sens = max(float(np.abs(rp[n] - rc[n]).max()) for n in ("X", "U"))
        d = {n: float(np.abs(rg[n][0].cpu().numpy() - rc[n]).max()) for n in ("X", "U")}
        print("k", k, "iters", rc["iters"], rg["iters"][0].item(), d, "oracle sensitivity", sens)
        assert rg["iters"][0].item() == rc["iters"]
        assert max(d.values()) <= max(1e-4, 20 * sens)


@pytest.mark.parametrize("act,hidden,n_hidden", [(0, 128, 1), (1, 128, 0), (1, 64, 1)], ids=["relu", "0_hidden", "64"])
def test_hdual_bf16_stream_refusals(act, hidden, n_hidden):
    """nlot_mlp_create_ex(desc, 6) refuses the shapes mlp_hdual_bf16_stream does not serve before any device call (no
    GPU here), and the message names the arithmetic."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd._lib import lib
    from nlotrajectories_amd.ops import DeviceMlp

    assert DeviceMlp.ARITH["hdual_bf16_stream"] == _abi.MLP_ARITH_HDUAL_BF16_STREAM == 6
    z = np.zeros(128 * 128, np.float32)
    d = _abi.NlotMlpDesc(in_kind=_abi.MLP_IN_LINEAR_RELU, hidden=hidden, n_hidden=n_hidden, act=act, fourier_scale=1.0,
                         b_out=0.0)
    d.A = d.b0 = d.W = d.b = d.w_out = z.ctypes.data_as(C.POINTER(C.c_float))
    assert not lib().nlot_mlp_create_ex(C.byref(d), 6)
    assert "NLOT_MLP_ARITH_HDUAL_BF16_STREAM" in lib().nlot_last_error().decode()
