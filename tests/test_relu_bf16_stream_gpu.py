"""NLOT_MLP_ARITH_SPLIT_BF16_STREAM (DeviceMlp(w, "split_bf16_stream"), kernel mlp_relu_bf16_stream): the ReLU reverse
sweep on split-bf16 MFMA products with the split activations in LDS and the split HxH weights streamed from L2, for ReLU
nets of H = 128 and 256 with 1-4 HxH layers.  Checked against torch fp64 autograd of the same module with the bars of
mlp_checks.check_vs_torch (value 2e-5 of max(1, max |f|), gradient and Hessian 1e-4 of max(1, their largest entry)); the
fp32 oracle's own error is printed beside the kernel's, and meets the same bars on these nets and points on the CPU
(test_oracle_meets_bars: the condition on the inputs, no point within fp32 rounding of a ReLU kink)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

# name -> (HxH layers, block tile): one layer at NQ = 2, the depth limit at H = 128, one layer at NQ = 4, the stress
# net 2-256x4-1, and the two input layers that give a Hessian
NETS = {"mlp_128x2": (1, 192), "mlp_128x5": (4, 192), "mlp_256x2": (1, 96), "stress": (3, 96),
        "fourier_128x5": (3, 192), "fourier_256x3": (1, 96)}


def _weights(name):
    from nlotrajectories_amd.nn import FourierMLP, MlpWeights, MultiLayerPerceptron

    torch.manual_seed(0)
    if name == "stress":
        w = MlpWeights.stress_sdf_mlp(seed=0)
    elif name.startswith("fourier"):
        H, layers = (int(s) for s in name[8:].split("x"))
        w = MlpWeights.from_module(FourierMLP(2, H, 1, num_layers=layers, scale=2.0))
    else:
        H, layers = (int(s) for s in name[4:].split("x"))
        w = MlpWeights.from_module(MultiLayerPerceptron(2, H, 1, layers, "ReLU"))
    assert w.n_hidden == NETS[name][0]
    return w


@functools.lru_cache(maxsize=None)
def _cases(name):
    """[(points, lambda, {with lambda?: torch fp64 value, lam * gradient, lam * Hessian}, fp32 oracle)] per P: one lane
    group's point, a full point group, a ragged one, one past the block tile, many tiles; computed once."""
    import oracle as O

    w, rng, out = _weights(name), np.random.default_rng(2), []
    m = w.torch_module().double()
    for P in (1, 16, 17, NETS[name][1] + 1, 1000):
        pts = rng.uniform(-0.5, 1.5, (P, 2)).astype(np.float32)
        lam = rng.uniform(-2, 2, P).astype(np.float32)
        ref = {}
        for with_lam in (False, True):  # as mlp_checks.check_vs_torch computes it
            x = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
            f = m(x)[:, 0]
            go = torch.tensor(lam if with_lam else np.ones(P), dtype=torch.float64)
            (gr,) = torch.autograd.grad(f, x, grad_outputs=go, create_graph=True)
            hs = [torch.autograd.grad(gr[:, a].sum(), x, retain_graph=True, allow_unused=True)[0] for a in range(2)]
            hs = [torch.zeros_like(x) if h is None else h for h in hs]
            ref[with_lam] = (f.detach().numpy(), gr.detach().numpy(), torch.stack(hs, 1).detach().numpy())
        ov, og, oh = O.mlp_eval(O.HostMlp(w), pts)
        out.append((pts, lam, ref, (ov, og, oh.reshape(-1, 2, 2))))
    return out


def _check(v, g, h, ref):
    for got, want, bar in zip((v, g, h), ref, (2e-5, 1e-4, 1e-4)):
        assert np.abs(got - want).max() <= bar * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", list(NETS))
def test_oracle_meets_bars(name):
    for _, lam, ref, (ov, og, oh) in _cases(name):
        _check(ov, og, oh, ref[False])
        _check(ov, lam[:, None] * og, lam[:, None, None] * oh, ref[True])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_kernel_relu_bf16_stream_matches_torch_f64(name):
    from nlotrajectories_amd.ops import DeviceMlp, sdf_mlp_eval

    dm = DeviceMlp(_weights(name), "split_bf16_stream")
    for pts, lam, ref, orc in _cases(name):
        pt = torch.tensor(pts, device="cuda")
        v, g, h = (t.cpu().numpy() for t in sdf_mlp_eval(dm, pt))
        va, ga, ha = (t.cpu().numpy() for t in sdf_mlp_eval(dm, pt, lam=torch.tensor(lam, device="cuda")))
        vv = sdf_mlp_eval(dm, pt, derivatives=False)[0].cpu().numpy()
        for what, k, o, r in zip(("value", "grad", "hess"), (v, g, h), orc, ref[False]):
            print(f"{name} P={len(pts)} {what}: kernel {np.abs(k - r).max():.3e} oracle {np.abs(o - r).max():.3e}"
                  f" of {np.abs(r).max():.3e}")
        np.testing.assert_array_equal(vv, v)  # the value-only launch is bitwise the full launch's value
        np.testing.assert_array_equal(va, v)
        np.testing.assert_array_equal(h[:, 0, 1], h[:, 1, 0])
        _check(v, g, h, ref[False])
        _check(va, ga, ha, ref[True])


@pytest.mark.gpu
def test_position_independence():
    """The first 17 points of the 1000-point case alone and inside the 1000-point launch: bitwise equal."""
    from nlotrajectories_amd.ops import DeviceMlp, sdf_mlp_eval

    dm = DeviceMlp(_weights("fourier_256x3"), "split_bf16_stream")
    pts, lam = (torch.tensor(a, device="cuda") for a in _cases("fourier_256x3")[-1][:2])
    for a, b in zip(sdf_mlp_eval(dm, pts, lam=lam), sdf_mlp_eval(dm, pts[:17].contiguous(), lam=lam[:17].contiguous())):
        np.testing.assert_array_equal(a[:17].cpu().numpy(), b.cpu().numpy())


@pytest.mark.gpu
def test_solver_iterates_relu_bf16_stream():
    """A seeded ReLU 2-256-256-1 net, its zero level put through the midpoint of the straight path, on the streamed
    split-bf16 kernel (the solver's launches address points through n_dev / P_per / ld): the Newton iterates after
    k = 1, 3 equal the oracle's to 1e-4, or to 20x the oracle's own response to a 1e-13 perturbation of the start where
    that is larger."""
    import oracle as O
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd.nn import MlpWeights
    from nlotrajectories_amd.ops import DeviceMlp
    from nlotrajectories_amd.problem import METRIC_PROBLEM
    from nlotrajectories_amd.solver import solve_batch

    w = MlpWeights.random_relu_mlp(256, 1)
    w.b_out = -float(O.mlp_eval(O.HostMlp(w), np.array([[0.5, 0.5]], np.float32))[0][0])
    mlp, hm = DeviceMlp(w, "split_bf16_stream"), O.HostMlp(w)
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


@pytest.mark.parametrize("act,hidden,n_hidden", [(1, 128, 1), (0, 64, 1), (0, 128, 0)], ids=["tanh", "64", "0_hidden"])
def test_relu_bf16_stream_refusals(act, hidden, n_hidden):
    """nlot_mlp_create_ex(desc, 7) refuses the shapes mlp_relu_bf16_stream does not serve before any device call (no
    GPU here), and the message names the arithmetic."""
    from nlotrajectories_amd import _abi
    from nlotrajectories_amd._lib import lib
    from nlotrajectories_amd.ops import DeviceMlp

    assert DeviceMlp.ARITH["split_bf16_stream"] == _abi.MLP_ARITH_SPLIT_BF16_STREAM == 7
    z = np.zeros(128 * 128, np.float32)
    d = _abi.NlotMlpDesc(in_kind=_abi.MLP_IN_LINEAR_RELU, hidden=hidden, n_hidden=n_hidden, act=act, fourier_scale=1.0,
                         b_out=0.0)
    d.A = d.b0 = d.W = d.b = d.w_out = z.ctypes.data_as(C.POINTER(C.c_float))
    assert not lib().nlot_mlp_create_ex(C.byref(d), 7)
    assert "NLOT_MLP_ARITH_SPLIT_BF16_STREAM" in lib().nlot_last_error().decode()
