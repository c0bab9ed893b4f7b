"""``bench.py --dump-outputs DIR``: the last timed step's outputs as DIR/<name>.npy, float32, at most 64 MB in all, and
``--steps`` as the number of timed steps in all."""
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def test_step_outputs_and_dump_under_the_limit(tmp_path):
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    x = torch.randn(5, 4, requires_grad=True)
    loss = model(x).square().sum()
    loss.backward()
    params = list(model.parameters())
    params[0].grad = None                                   # a parameter that took no gradient: zeros in its place
    arrays = bench.step_outputs(SimpleNamespace(params=params), model, SimpleNamespace(x=x), loss)
    assert sorted(arrays) == ["buffers", "gradients", "loss", "parameters", "x_grad"]
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert arrays["loss"].shape == () and arrays["loss"] == np.float32(loss.item())
    n = sum(p.numel() for p in params)
    assert arrays["parameters"].shape == (n,) and arrays["gradients"].shape == (n,)
    assert not arrays["gradients"][:params[0].numel()].any()
    np.testing.assert_array_equal(arrays["x_grad"], x.grad.reshape(-1).numpy())
    assert arrays["buffers"].shape == (6,)                  # running mean + var; num_batches_tracked is not a float

    bench.dump_outputs(str(tmp_path), arrays)
    for name, a in arrays.items():
        np.testing.assert_array_equal(np.load(tmp_path / f"{name}.npy"), a)


def test_dump_samples_past_the_limit_the_same_way_every_time(tmp_path):
    import bench
    big = np.arange(1000, dtype=np.float32)
    small = np.ones(10, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, limit=2040)
    got = [np.load(tmp_path / d / "big.npy") for d in ("a", "b")]
    np.testing.assert_array_equal(got[0], got[1])
    assert got[0].nbytes + np.load(tmp_path / "a" / "small.npy").nbytes <= 2040
    assert got[0].size < big.size and np.all(np.diff(got[0]) > 0)   # ascending positions of the original
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small[:5])      # a share in proportion


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "7", "--warmup", "1", "--blocks", "3",
                        "--no-roofline", "--no-cpu-baseline", "--no-pipeline", "--no-stress", "--no-model-sweep",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 7 and res["timing"]["steps_per_block"] == [3, 2, 2]
    assert res["timing"]["ms_per_step_min"] <= res["ms_per_step"] <= res["timing"]["ms_per_step_max"]
    files = sorted(os.listdir(out))
    assert files == ["buffers.npy", "gradients.npy", "loss.npy", "parameters.npy", "x_grad.npy"]
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype == np.float32 and np.all(np.isfinite(a)), name
    assert math.isclose(float(arrays["loss"]), res["loss"], rel_tol=0, abs_tol=1e-6)
    assert np.abs(arrays["gradients"]).max() > 0 and np.abs(arrays["x_grad"]).max() > 0
