#!/usr/bin/env python3
"""Cost of the GATConv stack next to the SGCN stack, and of a GCN_IMGSNP train step.

  1. us per launch of igcn_gat_stack_fwd / _bwd against igcn_sgcn_stack_fwd / _bwd at B = 256 graphs x 90 ROIs (k = 3
     brain graphs), H0 = 3, F = 16, L = 2: direct C-ABI calls, hot replays of a captured graph (bench._time_graph);
  2. ms per step of GraphedTrainStep for GCN_IMGSNP(ifUseGAT=False / True) at the headline workload (256 graphs, the
     3000-node GO DAG, L = 2, hidden 16, cross-attention), default lambda.

  3. (``--sgcn``) the edge-attribute gradient and the model that needs it, SGCN_GAT:
     * ``stacks.gat_bwd_ew_us`` beside ``gat_bwd_us`` at the shape of 1., and both again at 512 graphs (``stacks_pair``: the
       stacked (plain | masked) pair of a 256-graph step) — ``ew_over_plain`` is the cost of the extra output;
     * ``sgcn_step``: ms per captured train step (median of ``--blocks`` blocks, with the spread) of SGCN_GAT and SGCN_GCN
       on the same 256-graph batch, and the libigcn entry points one eager step calls (``igcn_calls``; torch's own
       operators — padding, nll_loss, log_softmax — are not counted);
     * ``--parent-tree DIR`` (a checkout of the parent commit WITH its built library): ``regression`` — ``step_ms.gat``'s
       workload timed in blocks by ``tools/gat_step_blocks.py --tree``, a fresh child process per tree and turn, this tree
       and that tree taking turns: the medians and the parent's block-to-block spread.  GCN_IMGSNP(ifUseGAT=True) calls
       igcn_gat_stack_bwd, whose code this comparison watches.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run every GPU step under a time limit, e.g.
    timeout -k 10 600 python tools/gat_bench.py --out profiles/gat_bench.json
    timeout -k 10 900 python tools/gat_bench.py --sgcn --parent-tree ../parent --out profiles/sgcn_gat_bench.json
"""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import subprocess
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


def stack_us(dev, g=256, rois=90, h0=3, f=16, layers=2, with_ew=False, gat_only=False):
    """``with_ew``: also time igcn_gat_stack_bwd_ew (new rows; the others keep their meaning).  ``gat_only``: the two GAT
    backward rows alone."""
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

    def gat_bwd_ew():
        for _ in range(ITERS):
            call("igcn_gat_stack_bwd_ew", g, rois, emax, h0, f, layers, ptr(x), ptr(ew), ptr(t.src32), ptr(t.dst32),
                 ptr(t.tgt_ptr), ptr(t.tgt_perm), ptr(t.src_ptr), ptr(t.src_perm), gp, ptr(dxcat), ptr(dx), ptr(dew),
                 ptr(dpg), ptr(scg), None, stream_ptr())

    out = {"shape": dict(graphs=g, rois=rois, h0=h0, f=f, layers=layers, max_edges=emax),
           "lds_bytes": {"gat_fwd": int(lib.igcn_gat_stack_lds_bytes(rois, emax, h0, f, layers, 0)),
                         "gat_bwd": int(lib.igcn_gat_stack_lds_bytes(rois, emax, h0, f, layers, 1)),
                         "sgcn_fwd": int(lib.igcn_sgcn_stack_lds_bytes(rois, emax, h0, f, layers, 0)),
                         "sgcn_bwd": int(lib.igcn_sgcn_stack_lds_bytes(rois, emax, h0, f, layers, 1))}}
    rows = [("sgcn_fwd_us", sgcn_fwd), ("gat_fwd_us", gat_fwd), ("sgcn_bwd_us", sgcn_bwd), ("gat_bwd_us", gat_bwd)]
    if gat_only:
        rows = rows[3:]
    if with_ew:
        out["lds_bytes"]["gat_bwd_ew"] = int(lib.igcn_gat_stack_lds_bytes(rois, emax, h0, f, layers, 2))
        rows.append(("gat_bwd_ew_us", gat_bwd_ew))
    for name, fn in rows:
        out[name] = round(bench._time_graph(fn) / ITERS, 2)
        print(f"{name} ({g} graphs): {out[name]:.2f} us per launch (bwd: + its parameter reduce)", flush=True)
    if with_ew:
        out["ew_over_plain"] = round(out["gat_bwd_ew_us"] / out["gat_bwd_us"], 4)
    return out


def _blocks_ms(step, blocks, steps, warmup):
    """ms per step of each of ``blocks`` blocks of ``steps`` replays (a synchronise around every block)."""
    for _ in range(warmup):
        step()
    out = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    return out


def _spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": min(ms), "max": max(ms), "blocks": ms}


def _gcn_imgsnp_step(dev, gat):
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
    return GraphedTrainStep(model, opt, data)


@contextlib.contextmanager
def recorded_calls():
    """The names of the libigcn entry points called inside the block, in order (``_lib.call`` and the modules' imported
    names of it, as tests/calltrace.py patches them)."""
    from igcn_amd import train
    seen, orig = [], _lib.call

    def traced(name, *args):
        seen.append(name)
        return orig(name, *args)
    mods = (_lib, ops, train)
    for m in mods:
        m.call = traced
    try:
        yield seen
    finally:
        for m in mods:
            m.call = orig


def sgcn_step(dev, kind, blocks, steps, warmup=10):
    """Captured train step of SGCN_GAT / SGCN_GCN (L = 2, hidden 16, two classes) on 256 graphs of 90 ROIs."""
    from types import SimpleNamespace
    from igcn_amd import train
    from igcn_amd.sgcn import SGCN_GAT, SGCN_GCN
    torch.manual_seed(1000)
    if kind == "gat":
        model = SGCN_GAT(SimpleNamespace(num_features=3, num_classes=2), bench.LAYERS, bench.HIDDEN, rois=bench.ROIS,
                         H_0=3).to(dev)
    else:
        model = SGCN_GCN(None, bench.LAYERS, bench.HIDDEN, rois=bench.ROIS, H_0=3, num_features=3, num_classes=2).to(dev)
    model.train()
    opt = train.FlatAdam(model.parameters(), lr=1e-3)
    graphs = synth.brain_graph_list(bench.GRAPHS_PER_GPU, seed=1000, rois=bench.ROIS, tsne_dim=16, num_classes=2)
    data = Batch.from_data_list(graphs).to(dev)
    # the libigcn entry points of one eager step (host-only switches of the deferral / rider queues left out)
    with recorded_calls() as seen:
        train.train_step(model, opt, Batch.from_data_list(graphs).to(dev))
    calls = [n for n in seen if n not in ("igcn_reduce_defer", "igcn_rider_cancel")]
    res = _spread(_blocks_ms(train.GraphedTrainStep(model, opt, data), blocks, steps, warmup))
    res["igcn_calls"] = len(calls)
    res["igcn_call_names"] = calls
    print(f"SGCN_{kind.upper()} GraphedTrainStep: {res['median']:.3f} ms per step (median of {blocks} blocks of {steps}; "
          f"{res['min']:.3f} .. {res['max']:.3f}), {len(calls)} libigcn calls per step", flush=True)
    return res


def regression(parent_tree, blocks, steps, rounds=2):
    """step_ms.gat's workload on this tree and on ``parent_tree``, fresh child processes taking turns."""
    trees = {"branch": os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parent": os.path.abspath(parent_tree)}
    ms = {"branch": [], "parent": []}
    for _ in range(rounds):
        for name, tree in trees.items():
            r = subprocess.run([sys.executable, os.path.join(trees["branch"], "tools", "gat_step_blocks.py"), "--tree", tree,
                                "--blocks", str(blocks), "--steps", str(steps)], capture_output=True, text=True,
                               timeout=400)
            if r.returncode != 0:
                raise RuntimeError(f"child ({name}) failed with {r.returncode}:\n{r.stderr[-2000:]}")
            got = json.loads(r.stdout.strip().splitlines()[-1])
            print(f"step_ms.gat workload, {name}: {got}", flush=True)
            ms[name] += got
    out = {"workload": "GCN_IMGSNP(ifUseGAT=True) GraphedTrainStep (step_ms.gat), ms per step per block of "
                       f"{steps} replays; {rounds} child processes per tree, taking turns",
           "branch": _spread(ms["branch"]), "parent": _spread(ms["parent"])}
    out["branch_median_within_parent_spread"] = bool(out["parent"]["min"] <= out["branch"]["median"]
                                                     <= out["parent"]["max"])
    print(f"regression: branch median {out['branch']['median']} ms, parent median {out['parent']['median']} ms, parent "
          f"blocks {out['parent']['min']} .. {out['parent']['max']} ms: within = "
          f"{out['branch_median_within_parent_spread']}", flush=True)
    return out


def step_ms(dev, gat, steps=30, warmup=5):
    step = _gcn_imgsnp_step(dev, gat)
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
    ap.add_argument("--sgcn", action="store_true", help="the SGCN_GAT rows (3. above) instead of 1. and 2.")
    ap.add_argument("--parent-tree", default=None, help="with --sgcn: a built checkout of the parent commit to compare "
                                                        "step_ms.gat's workload against")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.load()
    if args.sgcn:
        res = {"stacks": stack_us(dev, with_ew=True, gat_only=True),
               "stacks_pair": stack_us(dev, g=2 * bench.GRAPHS_PER_GPU, with_ew=True, gat_only=True),
               "sgcn_step": {"SGCN_GAT": sgcn_step(dev, "gat", args.blocks, args.steps),
                             "SGCN_GCN": sgcn_step(dev, "gcn", args.blocks, args.steps)}}
        if args.parent_tree:
            res["regression"] = regression(args.parent_tree, args.blocks, args.steps)
    else:
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
