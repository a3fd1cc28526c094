"""NLOT_MLP_ARITH_HDUAL_MFMA (DeviceMlp(w, "hdual_mfma"), kernel mlp_hdual): smooth-activation nets whose HxH layers
fit in LDS, value / gradient / Hessian forward as hyper-duals through v_mfma_f32 products.  Checked against torch fp64
autograd of the same module with the tolerances of tests/test_smooth_mlp.py (fp32 evaluation of exactly these nets:
value 2e-5 absolute, gradient and Hessian 2e-5 of their largest entry, 5e-5 for SIREN); the fp32 oracle's own error
is printed beside the kernel's.  mlp_tanh_128x2 (H = 128 with two resident layers, the LDS limit) is added after
_nets() so that the weights of the others are the ones the CPU suite checks."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
from test_smooth_mlp import _check, _nets, _torch_f64

NETS = ["fourier_tanh_2x", "fourier_sigmoid", "mlp_sigmoid", "mlp_leaky", "siren", "siren_4", "mlp_tanh_128x2"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NETS)
def test_kernel_hdual_matches_torch_f64(name):
    import oracle as O
    from nlotrajectories_amd.nn import MlpWeights, MultiLayerPerceptron
    from nlotrajectories_amd.ops import DeviceMlp, sdf_mlp_eval

    nets = _nets()
    nets["mlp_tanh_128x2"] = MultiLayerPerceptron(2, 128, 1, 3, "Tanh")
    w = MlpWeights.from_module(nets[name])
    dm = DeviceMlp(w, "hdual_mfma")
    rng = np.random.default_rng(2)
    tol = 5e-5 if "siren" in name else 2e-5
    # one lane group, a full wave tile, a ragged wave, a ragged block tile, many tiles
    for P in (1, 16, 17, 65, 1000):
        pts = rng.uniform(-0.5, 1.5, (P, 2)).astype(np.float32)
        lam = rng.uniform(-2, 2, P).astype(np.float32)
        pt = torch.tensor(pts, device="cuda")
        v, g, h = (t.cpu().numpy() for t in sdf_mlp_eval(dm, pt))
        va, ga, ha = (t.cpu().numpy() for t in sdf_mlp_eval(dm, pt, lam=torch.tensor(lam, device="cuda")))
        vv = sdf_mlp_eval(dm, pt, derivatives=False)[0].cpu().numpy()
        ref = _torch_f64(w, pts)
        orc = O.mlp_eval(O.HostMlp(w), pts)
        for what, k, o, r in zip(("value", "grad", "hess"), (v, g, h), orc, ref):
            print(f"{name} P={P} {what}: kernel {np.abs(k - r).max():.3e} oracle {np.abs(o.reshape(r.shape) - r).max():.3e}"
                  f" of {np.abs(r).max():.3e}")
        np.testing.assert_array_equal(vv, v)  # the value-only launch is bitwise the full launch's value
        np.testing.assert_array_equal(va, v)
        np.testing.assert_array_equal(h[:, 0, 1], h[:, 1, 0])
        _check(v, g, h, ref, tol)
        _check(va, ga, ha, (ref[0], lam[:, None] * ref[1], lam[:, None, None] * ref[2]), tol)


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_solver_iterates_hdual(artefact, act):
    """The artefact's weights under tanh / sigmoid hidden layers on the hyper-dual MFMA kernel (the solver's launches
    address points through n_dev / P_per / ld): the Newton iterates after k = 1, 3 equal the oracle's to 1e-4."""
    import oracle as O
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.ops import DeviceMlp
    from nlotrajectories_amd.problem import METRIC_PROBLEM
    from nlotrajectories_amd.solver import solve_batch

    w = dataclasses.replace(artefact, act={"tanh": _abi.ACT_TANH, "sigmoid": _abi.ACT_SIGMOID}[act])
    mlp, hm = DeviceMlp(w, "hdual_mfma"), O.HostMlp(w)
    x0, xg = [0, 0, 0.785, 0, 0], [1, 1, 0.785, 0, 0]
    for k in (1, 3):
        opt = _abi.gpu_options(max_iter=k)
        rg = solve_batch(METRIC_PROBLEM, np.array([x0]), np.array([xg]), mlp=mlp, options=opt)
        rc = O.solve_one(METRIC_PROBLEM, x0, xg, hm, opt=opt)
        assert rg["iters"][0].item() == rc["iters"]
        np.testing.assert_allclose(rg["X"][0].cpu().numpy(), rc["X"], atol=1e-4)
        np.testing.assert_allclose(rg["U"][0].cpu().numpy(), rc["U"], atol=1e-4)


@pytest.mark.parametrize("act,hidden,n_hidden", [(0, 128, 1), (1, 256, 1), (1, 64, 0), (1, 128, 3)],
                         ids=["relu", "h256", "0_hidden", "h128_3_layers"])
def test_hdual_refusals(act, hidden, n_hidden):
    """nlot_mlp_create_ex(desc, 3) refuses what mlp_hdual does not serve before any device call (no GPU here), and
    the message names what it does."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd._lib import lib

    z = np.zeros(max(n_hidden, 1) * hidden * hidden, np.float32)
    fp = z.ctypes.data_as(C.POINTER(C.c_float))
    d = _abi.NlotMlpDesc(in_kind=_abi.MLP_IN_LINEAR_RELU, hidden=hidden, n_hidden=n_hidden, act=act, fourier_scale=1.0,
                         b_out=0.0)
    d.A = d.b0 = d.W = d.b = d.w_out = fp
    assert not lib().nlot_mlp_create_ex(C.byref(d), _abi.MLP_ARITH_HDUAL_MFMA)
    msg = lib().nlot_last_error().decode()
    assert "NLOT_MLP_ARITH_HDUAL_MFMA" in msg and "128 and 1-2 HxH layers" in msg and "64 and 1-4" in msg
