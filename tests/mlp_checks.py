"""Checks shared by the GPU tests of the learned-SDF MLP kernels (tests/test_mlp_gpu.py, tests/test_stress_gpu.py)."""
import numpy as np
import torch


def check_vs_torch(w, P=3000, seed=0):
    """Value, lam * gradient and lam * Hessian of net `w` at P seeded points against torch fp64 autograd, and the
    value-only launch against the full launch's value."""
    from nlotrajectories_amd.ops import DeviceMlp, sdf_mlp_eval

    rng = np.random.default_rng(seed)
    pts = rng.uniform(-0.5, 1.5, size=(P, 2)).astype(np.float32)
    lam = rng.uniform(-1, 1, size=P).astype(np.float32)
    d = DeviceMlp(w)
    t = torch.tensor(pts, device="cuda")
    v, g, h = (x.cpu().numpy() for x in sdf_mlp_eval(d, t, lam=torch.tensor(lam, device="cuda")))
    vv, _, _ = sdf_mlp_eval(d, t, derivatives=False)
    m = w.torch_module().double()
    x = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
    f = m(x)[:, 0]
    (gr,) = torch.autograd.grad(f, x, grad_outputs=torch.tensor(lam, dtype=torch.float64), create_graph=True)
    hs = [torch.autograd.grad(gr[:, a].sum(), x, retain_graph=True)[0] for a in range(2)]
    H = torch.stack(hs, 1).detach().numpy()
    f64, g64 = f.detach().numpy(), gr.detach().numpy()
    fs, gs = max(1.0, np.abs(f64).max()), max(1.0, np.abs(g64).max())
    print(w.hidden, w.n_hidden, "max |f| err", np.abs(v - f64).max(), "max |grad| err", np.abs(g - g64).max(),
          "max |H| err", np.abs(h - H).max())
    # fp32 chain through 4 layers of width 256: absolute error relative to max |f| / |grad|
    assert np.abs(v - f64).max() <= 2e-5 * fs
    assert np.abs(g - g64).max() <= 1e-4 * gs
    assert np.abs(h - H).max() <= 1e-4 * max(1.0, np.abs(H).max())
    np.testing.assert_array_equal(vv.cpu().numpy(), v)  # value-only launch == full launch's value
