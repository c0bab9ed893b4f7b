#!/usr/bin/env python3
"""Cost of a captured GUIDE_IMGSNP train step beside the headline step.

GUIDE_IMGSNP at B = 256 graphs x 90 ROIs (H_0 = 3), the synthetic 3000-node GO DAG (bench.POOL, the GO side of
configs[3]), hidden 16, hidden_linear 32, dropout and the Gumbel gate on, temperature 0.1 as a device scalar, the
trainer's default lambda; and the headline SGCN_GCN_IMGSNP step of bench.py on the same batch.  Each is a
GraphedTrainStep; the two alternate block by block (5 blocks of 20 replays each), and ms per step / graphs per second
are the medians of the blocks, as bench.py reports them.

    timeout -k 10 600 python tools/guide_bench.py --out profiles/guide_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from igcn_amd import _lib, synth  # noqa: E402
from igcn_amd.data import Batch  # noqa: E402


def guide_step(dev, data):
    from igcn_amd.guide_img_snp import GUIDE_IMGSNP
    from igcn_amd.train import FlatAdam, GraphedTrainStep
    torch.manual_seed(1000)
    go_snps, adj, pool_dim = synth.go_hierarchy(bench.POOL, seed=0)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, dev)
    model = GUIDE_IMGSNP(bench.LAYERS, bench.HIDDEN, a_g, a, pool_dim, 32, dev, rois=bench.ROIS, H_0=3,
                         num_classes=3, num_regr=3).to(dev)
    model.train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    return GraphedTrainStep(model, opt, data, temperature=torch.tensor(0.1, device=dev))


def headline_step(dev, data):
    from igcn_amd.train import FlatAdam, GraphedTrainStep
    model, _ = bench.build_model(dev)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    return GraphedTrainStep(model, opt, data)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="replays per block")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.load()
    b = bench.GRAPHS_PER_GPU

    def batch():
        d = Batch.from_data_list(synth.brain_graph_list(b, seed=1000, rois=bench.ROIS, tsne_dim=90)).to(dev)
        d.x.requires_grad_(True)
        return d
    steps = {"guide": guide_step(dev, batch()), "headline": headline_step(dev, batch())}
    for s in steps.values():
        for _ in range(5):
            s()
    torch.cuda.synchronize()
    blocks = {k: [] for k in steps}
    for _ in range(args.blocks):
        for name, s in steps.items():                  # alternating: both see the same state of the box
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s()
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    res = {"device": torch.cuda.get_device_name(0), "graphs_per_step": b, "go_nodes": sum(bench.POOL),
           "timing": f"median of {args.blocks} blocks of {args.steps} hipGraph replays, the two steps alternating"}
    for name, v in blocks.items():
        ms = statistics.median(v)
        res[name] = {"ms_per_step": round(ms, 4), "graphs_per_s": round(b / ms * 1e3, 1),
                     "ms_per_step_blocks": [round(x, 4) for x in v]}
        print(f"{name}: {ms:.3f} ms per step ({b / ms * 1e3:.0f} graphs/s), blocks {[round(x, 3) for x in v]}",
              flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
