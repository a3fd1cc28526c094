"""bench.py's --dump-outputs and --full, on the CPU: dump_outputs writes the last step's batch of a solve result as
float64 .npy files, the same seeded sample of instances on every call and within its byte bound; --full is off by
default."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _result(total, N=7, nx=5, nu=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(X=torch.rand(total, N + 1, nx, dtype=torch.float64, generator=g),
                U=torch.rand(total, N, nu, dtype=torch.float64, generator=g),
                S=torch.rand(total, N + 1, dtype=torch.float64, generator=g),
                cost=torch.rand(total, dtype=torch.float64, generator=g),
                status=torch.randint(0, 5, (total,), dtype=torch.int32, generator=g),
                iters=torch.randint(0, 1000, (total,), dtype=torch.int32, generator=g))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_last_batch(tmp_path):
    import bench

    r = _result(30)  # 3 timed batches of 10 in one call's result: the last step's batch is rows 20..29
    assert bench.dump_outputs(str(tmp_path), r, 10) == 10
    out = _load(tmp_path)
    assert sorted(out) == sorted(bench.DUMP_KEYS + ("sample_index",))
    np.testing.assert_array_equal(out["sample_index"], np.arange(10))
    for k in bench.DUMP_KEYS:
        assert out[k].dtype == np.float64
        np.testing.assert_array_equal(out[k], r[k][20:].double().numpy())


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    import bench

    r = _result(200)
    per_row = 8 * (8 * 5 + 7 * 2 + 8 + 3)
    n = bench.dump_outputs(str(tmp_path / "a"), r, 100, max_bytes=33 * per_row)
    assert n == 33
    assert bench.dump_outputs(str(tmp_path / "b"), r, 100, max_bytes=33 * per_row) == 33
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    idx = a["sample_index"].astype(int)
    assert len(idx) == 33 and len(set(idx)) == 33 and (np.diff(idx) > 0).all() and idx.min() >= 0 and idx.max() < 100
    assert sum(v.nbytes for k, v in a.items() if k != "sample_index") <= 33 * per_row
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    for k in bench.DUMP_KEYS:
        np.testing.assert_array_equal(a[k], r[k][100 + idx].double().numpy())
    assert bench.DUMP_MAX_BYTES <= 64 << 20


def test_full_is_off_by_default(monkeypatch):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
