#!/usr/bin/env python3
"""Cost of a captured genetics-only train step (igcn_amd/snps.py) on its fused head + loss launches and without them.

Gene_ontology_network(in 2, layers 2, [5, 5], l_dim 32) alone on the synthetic 3000-node GO DAG (bench.POOL), B = 256
samples of 54 SNPs, dropout on, lambda0 = 1e-5.  ``step``: ms per captured step (snps.GraphedSnpsStep; median of
``--blocks`` blocks of ``--steps`` hot replays, with the spread) on the fused route (ops.SnpsHeadLoss: one launch per
direction, csrc/snps_head.hip) and under IGCN_NO_HEAD_LOSS_FUSED=1 (ops.BatchNorm1dGrouped, ops.linear twice, torch's
sigmoid / binary_cross_entropy / squared error and their backward), both in this process, taking turns block by block.
``launches``: the device kernels one eager step of each route launches (torch.profiler; where the profiler does not
deliver, the libigcn entry points the step calls — which leaves torch's own launches of the unfused route out — and
``launch_count_source`` says which).  The criterion (``fused_not_slower``): the fused route's median is not above the
unfused route's by more than the larger of the two block spreads.

    timeout -k 10 600 python tools/snps_bench.py --out profiles/snps_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from igcn_amd import _lib, snps, synth  # noqa: E402

L_DIM, BATCH = 32, 256


def model_and_batch(dev):
    from igcn_amd.go_model import Gene_ontology_network
    torch.manual_seed(1000)
    go_snps, adj, pool_dim = synth.go_hierarchy(bench.POOL, seed=0)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, dev)
    model = Gene_ontology_network(a_g, a, 2, 2, [5, 5], pool_dim, L_DIM, dev).to(dev)
    model.train()
    rng = np.random.default_rng(1000)
    data = torch.from_numpy(rng.integers(0, 3, (BATCH, 54)).astype(np.float32)).to(dev)
    label = torch.from_numpy((rng.random(BATCH) < 0.5).astype(np.float32)).to(dev)
    return model, data, label


class _route:
    """IGCN_NO_HEAD_LOSS_FUSED for the unfused route: read while a step is built, captured or run eagerly."""

    def __init__(self, fused):
        self.fused = fused

    def __enter__(self):
        if not self.fused:
            os.environ["IGCN_NO_HEAD_LOSS_FUSED"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("IGCN_NO_HEAD_LOSS_FUSED", None)
        return False


def captured_step(dev, fused):
    from igcn_amd.train import FlatAdam
    model, data, label = model_and_batch(dev)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    with _route(fused):
        return snps.GraphedSnpsStep(model, opt, data, label)


def launch_counts(dev, fused):
    """(device kernels, libigcn entry points) of one eager step of the route, after two warm-up steps."""
    from igcn_amd import ops, train
    from igcn_amd.train import FlatAdam
    model, data, label = model_and_batch(dev)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    calls = []
    orig = _lib.call

    def traced(name, *args):
        calls.append(name)
        return orig(name, *args)
    kernels, why = None, None
    with _route(fused):
        for _ in range(2):
            snps.train_step_snps(model, opt, data, label)
        torch.cuda.synchronize()
        for mod in (_lib, ops, train):
            mod.call = traced
        try:
            snps.train_step_snps(model, opt, data, label)
            torch.cuda.synchronize()
        finally:
            for mod in (_lib, ops, train):
                mod.call = orig
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                snps.train_step_snps(model, opt, data, label)
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
            kernels = len([n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]) or None
            if kernels is None:
                why = "the profiler recorded no device kernels"
        except Exception as exc:                       # noqa: BLE001 — the count is a report, the timing is the measurement
            why = f"{type(exc).__name__}: {exc}"
    return kernels, len(calls), ("igcn_snps_head_loss_fwd" in calls, "igcn_snps_head_loss_bwd" in calls), why


def _spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": min(ms), "max": max(ms), "blocks": ms}


def step_ms(dev, blocks, steps, warmup=10):
    steppers = {"fused": captured_step(dev, True), "unfused": captured_step(dev, False)}
    for s in steppers.values():
        for _ in range(warmup):
            s.step()
    ms = {k: [] for k in steppers}
    for _ in range(blocks):                          # the two take turns, block by block
        for k, s in steppers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                s.step()
            torch.cuda.synchronize()
            ms[k].append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    out = {k: _spread(v) for k, v in ms.items()}
    out["loss"] = {k: float(s.loss) for k, s in steppers.items()}
    gain = out["unfused"]["median"] - out["fused"]["median"]
    width = max(out[k]["max"] - out[k]["min"] for k in steppers)
    out["fused_gain_ms"], out["block_spread_ms"] = round(gain, 4), round(width, 4)
    out["fused_not_slower"] = bool(out["fused"]["median"] <= out["unfused"]["median"] + width)
    out["timing"] = f"median of {blocks} blocks of {steps} hot hipGraph replays after {warmup}, the two routes taking turns"
    for k in steppers:
        v = out[k]
        print(f"{k}: {v['median']:.4f} ms per step ({v['min']:.4f} .. {v['max']:.4f})", flush=True)
    print(f"fused route faster by {gain:.4f} ms; widest block spread {width:.4f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON in this file")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.load()
    res = {"shape": {"B": BATCH, "S": 54, "l_dim": L_DIM, "pool": list(bench.POOL), "dropout": True, "lambda0": 1e-5}}
    res["step"] = step_ms(dev, args.blocks, args.steps)
    res["launches"] = {}
    for name, fused in (("fused", True), ("unfused", False)):
        kernels, entry_points, (fwd, bwd), why = launch_counts(dev, fused)
        assert fwd == bwd == fused, (name, fwd, bwd)
        res["launches"][name] = {"device_kernels": kernels, "libigcn_entry_points": entry_points}
        if why:
            res["launches"][name]["profiler"] = why
        print(f"{name}: {kernels} device kernels, {entry_points} libigcn entry points per eager step", flush=True)
    both = all(v["device_kernels"] for v in res["launches"].values())
    res["launches"]["launch_count_source"] = "torch.profiler device kernels" if both else "libigcn entry points"
    key = "device_kernels" if both else "libigcn_entry_points"
    res["launches"]["fewer_by"] = res["launches"]["unfused"][key] - res["launches"]["fused"][key]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
