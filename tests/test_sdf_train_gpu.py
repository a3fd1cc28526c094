"""The learned-SDF training kernels (nlot_sdf_train_steps, nlot_sdf_batch_loss) against the trainer's
loss and torch.optim.Adam in fp64 on the CPU, on seeded points in (-0.5, 1.5)^2 with circle-SDF targets.

The bar of the comparisons: the kernel's max-abs error per tensor against fp64 is within MULT x the same error of
torch fp32 on the CPU, plus one ulp of the tensor's largest magnitude (the project's fp32-equivalence convention is
MULT = 2; the MFMA summation order needs 4.9 on the loss of a one-row batch and 2.2 on a gradient, so MULT = 6, below
the cap of 8; DESIGN.md §14 records the figures).  The data seeds (14 for one step: 2 band rows in 256, none in the
first 100; 32 for four steps) keep every pre-activation of the fp64 run further than 1e-5 from a ReLU kink
(asserted), so both fp32 paths differentiate the same linear piece.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

MULT = 6.0
N_PAR = 17025
HERE = os.path.dirname(os.path.abspath(__file__))


def reference(dtype, ws, we, batches, n_val=0, data_seed=14):
    """Adam steps of trainer._loss over `batches` (row counts, rows taken consecutively) in `dtype` on the CPU:
    the parameters after the last step, its gradient, the losses, the smallest |pre-activation| met, the inputs."""
    from nlotrajectories_amd.nn import MultiLayerPerceptron
    from nlotrajectories_amd.trainer import NNObstacleTrainer

    g = torch.Generator().manual_seed(data_seed)
    pts = (torch.rand(sum(batches) + n_val, 2, generator=g) * 2 - 0.5).float()
    tgt = (torch.linalg.norm(pts.double() - 0.5, dim=1) - 0.35).float().unsqueeze(1)
    model = MultiLayerPerceptron(2, 128, 1, 2, "ReLU")
    tr = NNObstacleTrainer([], model, device="cpu", eikonal_weight=we, surface_loss_weight=ws, seed=0, verbose=False)
    p0 = torch.nn.utils.parameters_to_vector(model.parameters()).detach().clone()
    model.to(dtype)
    opt, losses, zmin, at = torch.optim.Adam(model.parameters(), lr=1e-3), [], float("inf"), 0
    for nb in batches:
        xb, yb = pts[at:at + nb].to(dtype), tgt[at:at + nb].to(dtype)
        at += nb
        with torch.no_grad():
            z1 = model.input_layer(xb)
            zmin = min(zmin, z1.abs().min().item(), model.hidden_layers[0](torch.relu(z1)).abs().min().item())
        loss = tr._loss(xb, yb, torch.nn.MSELoss(), 1e-2, True)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    vec = lambda it: torch.cat([t.detach().reshape(-1) for t in it]).double()  # noqa: E731
    val = [tr._loss(pts[at + i:at + i + 256].to(dtype), tgt[at + i:at + i + 256].to(dtype), torch.nn.MSELoss(), 1e-2,
                    False).item() for i in range(0, n_val, 256)]
    return dict(par=vec(model.parameters()), grad=vec(p.grad for p in model.parameters()) if batches else None,
                losses=losses, zmin=zmin,
                pts=pts, tgt=tgt[:, 0], p0=p0, val=val)


ref = functools.lru_cache(maxsize=None)(reference)
SLICES = dict(W1=slice(0, 256), b1=slice(256, 384), W2=slice(384, 16768), b2=slice(16768, 16896),
              w3=slice(16896, 17024), b3=slice(17024, 17025))


def run_gpu(ws, we, chunks, p0, pts, tgt, M=1, want_grad=False, one_order=False):
    """The kernel over `chunks`, a list of launches, each a list of batch row counts (rows consecutive): the state
    [M, floats], the step losses [M, steps], the last gradient.  A launch gets its own order and first_row = 0, or
    with one_order (M = 1) a prefix of the whole order and first_row where it starts, as the trainer chunks an epoch."""
    from nlotrajectories_amd import _abi, _lib

    L, opt = _lib.lib(), _abi.sdf_train_options(surface_weight=ws, eikonal_weight=we)
    dev = "cuda"
    state = torch.zeros(M, L.nlot_sdf_train_state_floats(C.byref(opt)), device=dev)
    state[:, :N_PAR] = p0.to(dev)
    pts, tgt = pts.to(dev).contiguous(), tgt.to(dev).contiguous()
    n, at, losses = pts.shape[-2], 0, []
    grad = torch.zeros(M, N_PAR, device=dev) if want_grad else None
    for ch in chunks:
        rows = sum(ch)
        first = at if one_order else 0
        order = torch.arange(at - first, at + rows, dtype=torch.int32, device=dev).repeat(M, 1).contiguous()
        out = torch.zeros(M, len(ch), device=dev)
        _lib.check(L.nlot_sdf_train_steps(C.byref(opt), _lib.ptr(state), _lib.ptr(pts), _lib.ptr(tgt), _lib.ptr(order),
                                          n, first, first + rows, _lib.ptr(out), _lib.ptr(grad), M, _lib.stream_ptr()),
                   "train")
        losses.append(out)
        at += rows
    torch.cuda.synchronize()
    return state.cpu(), torch.cat(losses, 1).cpu(), None if grad is None else grad.cpu()


def assert_close(name, got, r64, r32):
    """Per tensor: |got - fp64| <= MULT |fp32 - fp64| + ulp(max |fp64|); the figures are printed first."""
    for k, s in SLICES.items():
        e = (got[s].double() - r64[s]).abs().max().item()
        e32 = (r32[s] - r64[s]).abs().max().item()
        ulp = float(np.spacing(np.float32(r64[s].abs().max().item())))
        print(f"{name} {k}: gpu err {e:.3e}  fp32 err {e32:.3e}  ulp {ulp:.3e}  mag {r64[s].abs().max().item():.3g}")
        assert e <= MULT * e32 + ulp, (name, k, e, e32, ulp)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [256, 100, 1])
@pytest.mark.parametrize("ws,we", [(0.0, 0.0), (1.0, 0.0), (0.0, 0.01), (1.0, 0.01)])
def test_gradient_and_loss_of_one_step(ws, we, nb):
    r64, r32 = ref(torch.float64, ws, we, (nb,)), ref(torch.float32, ws, we, (nb,))
    assert r64["zmin"] > 1e-5
    band = int((r64["tgt"][:nb].abs() < 1e-2).sum())
    assert (band > 0) == (nb == 256)  # one batch with band rows, two without
    _, loss, grad = run_gpu(ws, we, [[nb]], r64["p0"], r64["pts"], r64["tgt"], want_grad=True)
    e, e32 = abs(loss[0, 0].item() - r64["losses"][0]), abs(r32["losses"][0] - r64["losses"][0])
    print(f"loss {r64['losses'][0]:.6g}: gpu err {e:.3e}  fp32 err {e32:.3e}")
    assert e <= MULT * e32 + float(np.spacing(np.float32(r64["losses"][0])))
    assert_close(f"grad ws={ws} we={we} nb={nb}", grad[0], r64["grad"], r32["grad"])


@pytest.mark.gpu
def test_adam_four_steps_last_partial():
    b = (256, 256, 256, 160)
    r64, r32 = ref(torch.float64, 1.0, 0.01, b, 0, 32), ref(torch.float32, 1.0, 0.01, b, 0, 32)
    assert r64["zmin"] > 1e-5
    state, loss, _ = run_gpu(1.0, 0.01, [list(b)], r64["p0"], r64["pts"], r64["tgt"])
    assert state[0, -1:].view(torch.int32).item() == 4
    np.testing.assert_allclose(loss[0].numpy(), r64["losses"], rtol=1e-6)
    assert_close("adam", state[0, :N_PAR], r64["par"], r32["par"])


@pytest.mark.gpu
def test_scheduling_does_not_change_arithmetic():
    b = (256, 256, 256, 160)
    r = ref(torch.float64, 1.0, 0.01, b, 0, 32)
    one, l1, _ = run_gpu(1.0, 0.01, [list(b)], r["p0"], r["pts"], r["tgt"])
    four, l4, _ = run_gpu(1.0, 0.01, [[x] for x in b], r["p0"], r["pts"], r["tgt"])
    assert torch.equal(one.view(torch.int32), four.view(torch.int32)) and torch.equal(l1, l4)
    split, ls, _ = run_gpu(1.0, 0.01, [[256], [256, 256], [160]], r["p0"], r["pts"], r["tgt"], one_order=True)
    assert torch.equal(one.view(torch.int32), split.view(torch.int32)) and torch.equal(l1, ls)  # first_row = 256, 768
    # two different networks (other initial weights, other rows) in one call, and each alone
    p0 = torch.stack([r["p0"], r["p0"].flip(0) * 0.5])
    pts, tgt = torch.stack([r["pts"], r["pts"].flip(0)]), torch.stack([r["tgt"], r["tgt"].flip(0)])
    both, lb, _ = run_gpu(1.0, 0.01, [list(b)], p0, pts, tgt, M=2)
    for m in range(2):
        alone, la, _ = run_gpu(1.0, 0.01, [list(b)], p0[m], pts[m], tgt[m])
        assert torch.equal(both[m].view(torch.int32), alone[0].view(torch.int32)) and torch.equal(lb[m], la[0])
    assert not torch.equal(both[0], both[1])


@pytest.mark.gpu
@pytest.mark.parametrize("ws", [0.0, 1.0])
def test_batch_loss(ws):
    from nlotrajectories_amd import _abi, _lib

    r = ref(torch.float64, ws, 0.0, (), 300)  # the initial fp32 weights in fp64: a full batch and one of 44 rows
    assert [int((r["tgt"][i:i + 256].abs() < 1e-2).sum()) > 0 for i in (0, 256)] == [True, False]
    L, opt = _lib.lib(), _abi.sdf_train_options(surface_weight=ws)
    state = torch.zeros(L.nlot_sdf_train_state_floats(C.byref(opt)), device="cuda")
    state[:N_PAR] = r["p0"].cuda()
    pts, tgt, out = r["pts"].cuda().contiguous(), r["tgt"].cuda().contiguous(), torch.zeros(2, device="cuda")
    _lib.check(L.nlot_sdf_batch_loss(C.byref(opt), _lib.ptr(state), _lib.ptr(pts), _lib.ptr(tgt), 300, _lib.ptr(out), 1,
                                     _lib.stream_ptr()), "batch_loss")
    print("batch loss", out.cpu().tolist(), r["val"])
    np.testing.assert_allclose(out.cpu().numpy(), r["val"], rtol=1e-6)


def _b6_trainer(backend, device):
    from nlotrajectories_amd.config import Config
    from nlotrajectories_amd.trainer import NNObstacleTrainer, model_from_config

    cfg = Config.model_validate(json.load(open(os.path.join(HERE, "golden", "nlp_golden.json")))["configs"][
        "benchmark_6_ackermann_wave.yaml"])
    tr = NNObstacleTrainer(cfg.obstacle_dicts(), model_from_config(cfg.model), device=device, epochs=1, n_samples=2000,
                           boundary_fraction=cfg.model.boundary_fraction, eikonal_weight=cfg.model.eikonal_loss_weight,
                           surface_loss_weight=cfg.model.surface_loss_weight, seed=0, verbose=False, backend=backend)
    assert (tr.surface_loss_weight, tr.eikonal_weight) == (1.0, 0.01)
    return tr, tr.train((-0.5, 1.5), (-0.5, 1.5))


@pytest.mark.gpu
def test_trainer_backend_hip_matches_torch_end_to_end(monkeypatch):
    from nlotrajectories_amd import trainer
    from nlotrajectories_amd.nn import MlpWeights

    monkeypatch.setattr(trainer._HipLoops, "STEPS_PER_LAUNCH", 3)  # the epoch's 8 steps in launches of 3, 3, 2

    hip, model = _b6_trainer("hip", "cuda")
    cpu, _ = _b6_trainer("torch", "cpu")
    print("hip", hip.history, "torch cpu", cpu.history)
    np.testing.assert_allclose(hip.history[0], cpu.history[0], rtol=1e-4)
    w = MlpWeights.from_module(model)
    assert w.hidden == 128 and w.n_hidden == 1


def test_host_validation_refuses_bad_arguments_before_the_device():
    from nlotrajectories_amd import _abi, _lib
    from nlotrajectories_amd.nn import MultiLayerPerceptron
    from nlotrajectories_amd.trainer import NNObstacleTrainer

    L, one = _lib.lib(), C.c_void_p(8)  # a non-null pointer that a refused call never dereferences

    def steps(opt=None, state=one, M=1, n_rows=256, first_row=0):
        opt = opt or _abi.sdf_train_options()
        rc = L.nlot_sdf_train_steps(C.byref(opt), state, one, one, one, 1000, first_row, n_rows, one, None, M, None)
        return rc, L.nlot_last_error().decode()

    for bad in (dict(hidden=64), dict(n_hidden=2), dict(batch=128)):
        rc, msg = steps(_abi.sdf_train_options(**bad))
        assert rc == -1 and "unsupported shape" in msg
        assert L.nlot_sdf_batch_loss(C.byref(_abi.sdf_train_options(**bad)), one, one, one, 10, one, 1, None) == -1
    assert steps(state=None) == (-1, "nlot_sdf_train_steps: null pointer")
    assert steps(M=0)[0] == -1 and "M out of range" in steps(M=0)[1]
    assert steps(n_rows=0)[0] == -1 and "n_rows" in steps(n_rows=0)[1]
    assert steps(n_rows=1000, first_row=100)[0] == -1 and "multiple of 256" in steps(n_rows=1000, first_row=100)[1]
    assert L.nlot_sdf_batch_loss(C.byref(_abi.sdf_train_options()), one, None, one, 10, one, 1, None) == -1
    d = _abi.NlotSdfTrainOptions()
    L.nlot_sdf_train_default_options(C.byref(d))
    assert bytes(d) == bytes(_abi.sdf_train_options()) and L.nlot_sdf_train_state_floats(C.byref(d)) == 3 * N_PAR + 1
    good = lambda: MultiLayerPerceptron(2, 128, 1, 2, "ReLU")  # noqa: E731
    for model, bs, dev in ((MultiLayerPerceptron(2, 128, 1, 2, "Tanh"), 256, "cuda"),
                           (MultiLayerPerceptron(2, 64, 1, 2, "ReLU"), 256, "cuda"), (good(), 128, "cuda"),
                           (good(), 256, "cpu")):  # host tensors must never reach the kernels
        with pytest.raises(ValueError, match='backend="torch"'):
            NNObstacleTrainer([], model, device=dev, batch_size=bs, verbose=False, backend="hip")
