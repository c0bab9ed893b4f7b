#!/usr/bin/env python3
"""Cost of the GATConv stack next to the SGCN stack, and of a GCN_IMGSNP train step.

  1. us per launch of igcn_gat_stack_fwd / _bwd against igcn_sgcn_stack_fwd / _bwd at B = 256 graphs x 90 ROIs (k = 3
     brain graphs), H0 = 3, F = 16, L = 2: direct C-ABI calls, hot replays of a captured graph (bench._time_graph);
  2. ms per step of GraphedTrainStep for GCN_IMGSNP(ifUseGAT=False / True) at the headline workload (256 graphs, the
     3000-node GO DAG, L = 2, hidden 16, cross-attention), default lambda.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run every GPU step under a time limit, e.g.
    timeout -k 10 600 python tools/gat_bench.py --out profiles/gat_bench.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from igcn_amd import _lib, ops, synth  # noqa: E402
from igcn_amd._lib import call, ptr, stream_ptr  # noqa: E402
from igcn_amd.data import Batch  # noqa: E402

ITERS = 20


def stack_us(dev, g=256, rois=90, h0=3, f=16, layers=2):
    data = Batch.from_data_list(synth.brain_graph_list(g, seed=1, rois=rois, tsne_dim=8)).to(dev)
    plan = ops.plan_for(data)
    n, emax = data.x.shape[0], plan._stack_dims[1]
    x, ew = data.x.contiguous(), data.edge_attr.contiguous()
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen) * 0.3        # noqa: E731
    ws = [rnd(f, h0 if l == 0 else f) for l in range(layers)]
    bs = [rnd(f) for _ in range(layers)]
    gat = [t for l in range(layers) for t in (ws[l], bs[l], rnd(f), rnd(f), rnd(f), rnd(f))]
    wp = (ctypes.c_void_p * layers)(*[w.data_ptr() for w in ws])
    bp = (ctypes.c_void_p * layers)(*[b.data_ptr() for b in bs])
    gp = (ctypes.c_void_p * len(gat))(*[t.data_ptr() for t in gat])
    xcat = torch.empty(n, layers * f, device=dev)
    dxcat = torch.randn(n, layers * f, device=dev, generator=gen)
    dx, dew = torch.empty_like(x), torch.empty_like(ew)
    lib = _lib.load()
    ns, ng = int(lib.igcn_sgcn_stack_param_floats(h0, f, layers)), int(lib.igcn_gat_stack_param_floats(h0, f, layers))
    dps, dpg = torch.empty(ns, device=dev), torch.empty(ng, device=dev)
    scs, scg = torch.empty(g * ns, device=dev), torch.empty(g * ng, device=dev)
    t = plan

    def sgcn_fwd():
        for _ in range(ITERS):
            call("igcn_sgcn_stack_fwd", g, rois, emax, h0, f, layers, ptr(x), ptr(ew), ptr(t.src32), ptr(t.dst32),
                 ptr(t.tgt_ptr), ptr(t.tgt_perm), ptr(t.loop_edge), wp, bp, ptr(xcat), None, stream_ptr())

    def sgcn_bwd():
        for _ in range(ITERS):
            call("igcn_sgcn_stack_bwd", g, rois, emax, h0, f, layers, ptr(x), ptr(ew), ptr(t.src32), ptr(t.dst32),
                 ptr(t.tgt_ptr), ptr(t.tgt_perm), ptr(t.src_ptr), ptr(t.src_perm), ptr(t.loop_edge), wp, bp,
                 ptr(dxcat), None, ptr(dx), ptr(dew), ptr(dps), ptr(scs), None, stream_ptr())

    def gat_fwd():
        for _ in range(ITERS):
            call("igcn_gat_stack_fwd", g, rois, emax, h0, f, layers, ptr(x), ptr(ew), ptr(t.src32), ptr(t.dst32),
                 ptr(t.tgt_ptr), ptr(t.tgt_perm), gp, ptr(xcat), None, stream_ptr())

    def gat_bwd():
        for _ in range(ITERS):
            call("igcn_gat_stack_bwd", g, rois, emax, h0, f, layers, ptr(x), ptr(ew), ptr(t.src32), ptr(t.dst32),
                 ptr(t.tgt_ptr), ptr(t.tgt_perm), ptr(t.src_ptr), ptr(t.src_perm), gp, ptr(dxcat), ptr(dx), ptr(dpg),
                 ptr(scg), None, stream_ptr())

    out = {"shape": dict(graphs=g, rois=rois, h0=h0, f=f, layers=layers, max_edges=emax),
           "lds_bytes": {"gat_fwd": int(lib.igcn_gat_stack_lds_bytes(rois, emax, h0, f, layers, 0)),
                         "gat_bwd": int(lib.igcn_gat_stack_lds_bytes(rois, emax, h0, f, layers, 1)),
                         "sgcn_fwd": int(lib.igcn_sgcn_stack_lds_bytes(rois, emax, h0, f, layers, 0)),
                         "sgcn_bwd": int(lib.igcn_sgcn_stack_lds_bytes(rois, emax, h0, f, layers, 1))}}
    for name, fn in (("sgcn_fwd_us", sgcn_fwd), ("gat_fwd_us", gat_fwd), ("sgcn_bwd_us", sgcn_bwd),
                     ("gat_bwd_us", gat_bwd)):
        out[name] = round(bench._time_graph(fn) / ITERS, 2)
        print(f"{name}: {out[name]:.2f} us per launch (bwd: + its parameter reduce)", flush=True)
    return out


def step_ms(dev, gat, steps=30, warmup=5):
    from igcn_amd.gcn_img_snp import GCN_IMGSNP
    from igcn_amd.train import FlatAdam, GraphedTrainStep
    torch.manual_seed(1000)
    go_snps, adj, pool_dim = synth.go_hierarchy(bench.POOL, seed=0)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, dev)
    model = GCN_IMGSNP(bench.LAYERS, bench.HIDDEN, a_g, a, pool_dim, 32, dev, rois=bench.ROIS, H_0=3, num_classes=3,
                       isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseFeat4Regr=True,
                       isImageOnly=False, isSNPsOnly=False, ifUseGAT=gat).to(dev)
    model.train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    data = Batch.from_data_list(synth.brain_graph_list(bench.GRAPHS_PER_GPU, seed=1000, rois=bench.ROIS,
                                                       tsne_dim=90)).to(dev)
    step = GraphedTrainStep(model, opt, data)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    print(f"GCN_IMGSNP(ifUseGAT={gat}) GraphedTrainStep: {ms:.3f} ms per step ({bench.GRAPHS_PER_GPU} graphs)",
          flush=True)
    return round(ms, 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.load()
    res = {"stacks": stack_us(dev)}
    res["step_ms"] = {"gcn": step_ms(dev, False), "gat": step_ms(dev, True)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
