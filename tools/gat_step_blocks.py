#!/usr/bin/env python3
"""ms per captured train step of GCN_IMGSNP(ifUseGAT=True) at the headline workload (the ``step_ms.gat`` row of
tools/gat_bench.py), block by block, for the package of ANY checkout: ``--tree DIR`` names the checkout whose
``igcn_amd`` (with its built library) and ``bench.py`` constants are timed — tools/gat_bench.py --parent-tree runs this
file once per tree and turn, each time in a fresh process.  Prints one JSON list: ms per step of every block.
    timeout -k 10 300 python tools/gat_step_blocks.py --tree . --blocks 5 --steps 30
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout to time (default: the one this file is in)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import bench
    from igcn_amd import _lib, synth
    from igcn_amd.data import Batch
    from igcn_amd.gcn_img_snp import GCN_IMGSNP
    from igcn_amd.train import FlatAdam, GraphedTrainStep
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.manual_seed(1000)
    go_snps, adj, pool_dim = synth.go_hierarchy(bench.POOL, seed=0)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, dev)
    model = GCN_IMGSNP(bench.LAYERS, bench.HIDDEN, a_g, a, pool_dim, 32, dev, rois=bench.ROIS, H_0=3, num_classes=3,
                       isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseFeat4Regr=True,
                       isImageOnly=False, isSNPsOnly=False, ifUseGAT=True).to(dev)
    model.train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    data = Batch.from_data_list(synth.brain_graph_list(bench.GRAPHS_PER_GPU, seed=1000, rois=bench.ROIS,
                                                       tsne_dim=90)).to(dev)
    step = GraphedTrainStep(model, opt, data)
    for _ in range(args.warmup):
        step()
    out = []
    for _ in range(args.blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t0) * 1e3 / args.steps, 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
