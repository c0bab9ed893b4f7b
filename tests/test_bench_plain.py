"""``bench.py --gpus 1 --steps K --warmup W`` without ``--full``: the headline and nothing else — no loader-fed runs,
profiler child, rooflines, model sweep, CPU baseline or configs[4] child in the line."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")

FULL_ONLY = ("pipeline", "roofline", "roofline_scatter_standalone", "roofline_mfma", "roofline_step", "profile",
             "model_sweep", "cpu_baseline", "stress", "distributed_step", "rotating_batches")


@pytest.mark.gpu
def test_plain_run_prints_only_the_headline():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "4", "--warmup", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["metric"] == "graphs/s train step (90-ROI brain + GO-SNP)" and res["unit"] == "graphs/s"
    assert res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["steps"] == 4 and res["warmup"] == 1 and res["timing"]["steps_per_block"] == [1, 1, 1, 1]
    assert res["value"] == pytest.approx(res["config"]["graphs_per_gpu"] / res["ms_per_step"] * 1e3, rel=2e-3)
    assert math.isfinite(res["loss"])
    assert [k for k in FULL_ONLY if k in res] == []
