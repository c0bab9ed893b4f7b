#!/usr/bin/env python3
"""The hidden-32 rows of the reference's default search (main.py:141-145: SGCN_GCN_IMGSNP(L, 32), L = 2..5, attention
width 64 / 96 / 128 / 160) as captured train steps at the headline workload, next to the (2, 16) model the metric is
quoted on — bench.py's --model-sweep for the rows that sweep does not list.

Per model: the step bench.py times (256 graphs x 90 ROIs, the 3000-node GO DAG, two forward passes + seven losses +
backward + Adam, replayed from one hipGraph): ms per step (median / min / max of ``--blocks`` blocks of ``--steps``
replays), graphs/s, cost per graph relative to (2, 16), and the library entry-point calls of one eager step of the same
model (``launches_per_step``: what the capture records, counted at the Python boundary; an entry point may launch more
than one kernel).  A model whose step refuses a shape is recorded with the error text in place of a time.

    timeout -k 10 900 python tools/hidden32_bench.py --out profiles/hidden32_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
MODELS = [(2, 16), (2, 32), (3, 32), (4, 32), (5, 32)]


def _count_calls(model, opt, data):
    """Library entry-point calls of one eager train step."""
    from igcn_amd import _lib, ops, train
    orig, n = _lib.call, [0]

    def counted(name, *a):
        n[0] += 1
        return orig(name, *a)
    mods = (_lib, ops, train)
    try:
        for m in mods:
            m.call = counted
        train.train_step(model, opt, data)
    finally:
        for m in mods:
            m.call = orig
    return n[0]


def model_row(dev, wl, layers, hidden, blocks, steps, warmup):
    import torch
    import bench
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from igcn_amd.train import FlatAdam, GraphedTrainStep, stream_pending
    row = {"layers": layers, "hidden": hidden, "attention_width": layers * hidden}
    model, _ = bench.build_model(dev, wl, layers=layers, hidden=hidden)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    data = Batch.from_data_list(synth.brain_graph_list(wl["graphs"], seed=1000, rois=wl["rois"], tsne_dim=90,
                                                       dense=wl["dense"])).to(dev)
    data.x.requires_grad_(True)
    try:
        step = GraphedTrainStep(model, opt, data)
        for _ in range(warmup):
            step()
        ms = []
        for _ in range(blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / steps)
        row.update(ms_per_step=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                   graphs_per_s=round(wl["graphs"] / statistics.median(ms) * 1e3, 1), loss=round(float(step.loss), 5),
                   loss_finite=bool(torch.isfinite(step.loss)), stream_pending=int(stream_pending()))
        del step
        row["launches_per_step"] = _count_calls(model, opt, data)
    except Exception as exc:                  # noqa: BLE001
        row["error"] = f"{type(exc).__name__}: {exc}"[:300]
    del opt, model
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks: at least five timed blocks")
    import torch
    import bench
    from igcn_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["full"]
    rows = []
    for layers, hidden in MODELS:
        row = model_row(dev, wl, layers, hidden, args.blocks, args.steps, args.warmup)
        base = rows[0].get("ms_per_step") if rows else row.get("ms_per_step")
        if base and "ms_per_step" in row:
            row["cost_per_graph_vs_2x16"] = round(row["ms_per_step"] / base, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "tools/hidden32_bench.py", "device": torch.cuda.get_device_name(0), "workload": wl["name"],
           "graphs": wl["graphs"],
           "timing": f"captured step (GraphedTrainStep), {args.warmup} warm-up replays, then {args.blocks} blocks of "
                     f"{args.steps} replays between host clocks with a device synchronisation; median / min / max of the "
                     "blocks",
           "launches_per_step": "library entry-point calls of one eager step of the same model",
           "entries": rows}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
