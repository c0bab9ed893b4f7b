#!/usr/bin/env python3
"""Cost of SGCN_Ori's LDS-resident graph stack next to the per-layer route, and of an SGCN_Ori train step.

  1. ``kernels`` — us per launch of igcn_sgcn_ori_fwd / _bwd at 256 and 512 graphs x 90 ROIs (k = 3 brain graphs),
     (H0, F1, F3) = (3, 32, 5): direct C-ABI calls, hot replays of a captured graph (bench._time_graph).  Beside them,
     on the same inputs in the same run, the per-layer route (gcn_norm once, transform + aggregate per layer, ReLU,
     concatenation: only kernels that existed before the fused stack; forward, and forward + backward through autograd)
     and, for orientation, igcn_sgcn_stack_fwd / _bwd at F = 32, L = 2.
  2. ``step`` — ms per captured train step (median of ``--blocks`` blocks, with the spread) of SGCN_Ori(3, 32, 32, 5)
     at 256 graphs on the fused route and on the per-layer route (IGCN_NO_FUSED_SGCN=1 while that step is captured), the
     two taking turns block by block, and of SGCN_GCN(2, 16) on the same batch.
  3. ``--parent-tree DIR`` (a checkout of the parent commit WITH its built library): ``headline`` — ``python bench.py`` in
     a fresh process per tree and turn, this tree and that tree taking turns: ms per step of every run, the medians, the
     parent's spread, and whether the arrays of ``bench.py --dump-outputs`` are bit-identical.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run every GPU step under a time limit, e.g.
    timeout -k 10 600 python tools/ori_bench.py --out profiles/sgcn_ori_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from igcn_amd import _lib, ops, synth  # noqa: E402
from igcn_amd._lib import call, ptr, stream_ptr  # noqa: E402
from igcn_amd.data import Batch  # noqa: E402

ITERS = 20
DIMS = (3, 32, 32, 5)


def kernel_us(dev, g, rois=90, h0=3, f1=32, f3=5, fs=32, ls=2):
    data = Batch.from_data_list(synth.brain_graph_list(g, seed=1, rois=rois, tsne_dim=8)).to(dev)
    plan = ops.plan_for(data)
    plan.check()
    n, emax = data.x.shape[0], plan._stack_dims[1]
    x, ew = data.x.contiguous(), data.edge_attr.contiguous()
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen) * 0.3        # noqa: E731
    w1, b1, w3, b3 = rnd(f1, h0), rnd(f1), rnd(f3, f1), rnd(f3)
    z, acts = torch.empty(g, rois * (f1 + f3), device=dev), torch.empty(n, f3, device=dev)
    dz, dacts = torch.randn(g, rois * (f1 + f3), device=dev, generator=gen), torch.empty(n, f3, device=dev)
    dx, dew = torch.empty_like(x), torch.empty_like(ew)
    lib = _lib.load()
    npar = int(lib.igcn_sgcn_ori_param_floats(h0, f1, f3))
    dpar, scr = torch.empty(npar, device=dev), torch.empty(g * npar, device=dev)
    t = plan

    def ori_fwd():
        for _ in range(ITERS):
            call("igcn_sgcn_ori_fwd", g, rois, emax, h0, f1, f3, ptr(x), ptr(ew), ptr(t.src32), ptr(t.dst32),
                 ptr(t.tgt_ptr), ptr(t.tgt_perm), ptr(t.loop_edge), ptr(w1), ptr(b1), ptr(w3), ptr(b3), ptr(z), ptr(acts),
                 None, stream_ptr())

    def ori_bwd():
        for _ in range(ITERS):
            call("igcn_sgcn_ori_bwd", g, rois, emax, h0, f1, f3, ptr(x), ptr(ew), ptr(t.src32), ptr(t.dst32),
                 ptr(t.tgt_ptr), ptr(t.tgt_perm), ptr(t.src_ptr), ptr(t.src_perm), ptr(t.loop_edge), ptr(w1), ptr(b1),
                 ptr(w3), ptr(b3), ptr(dz), None, ptr(dacts), ptr(dx), ptr(dew), ptr(dpar), ptr(scr), None, stream_ptr())

    # the per-layer route on the same inputs, as SGCN_Ori._graph_stack runs it
    leaves = [v.clone().requires_grad_(True) for v in (x, ew, w1, b1, w3, b3)]

    def per_layer():
        xi, ewi, a1, c1, a3, c3 = leaves
        what, wloop, ts, ss = ops.GcnNorm.apply(ewi, plan)
        h1 = ops.GcnPropagate.apply(ops.linear(xi, a1), what, wloop, c1, plan, True, ts, ss)
        ac = ops.GcnPropagate.apply(ops.linear(h1, a3), what, wloop, c3, plan, False, ts, ss)
        return torch.cat((h1.view(g, -1), torch.relu(ac).view(g, -1)), 1), ac

    def layer_fwd():
        with torch.no_grad():
            for _ in range(ITERS):
                per_layer()

    def layer_fwd_bwd():
        for _ in range(ITERS):
            zz, _ = per_layer()
            torch.autograd.backward(zz, dz, inputs=leaves)

    def ori_fwd_bwd():
        for _ in range(ITERS):
            zz, _ = ops.SgcnOriStack.apply(leaves[0], leaves[1], plan, rois, None, *leaves[2:])
            torch.autograd.backward(zz, dz, inputs=leaves)

    # the uniform stack at F = fs, L = ls, for orientation
    ws = [rnd(fs, h0 if l == 0 else fs) for l in range(ls)]
    bs = [rnd(fs) for _ in range(ls)]
    wp = (ctypes.c_void_p * ls)(*[w.data_ptr() for w in ws])
    bp = (ctypes.c_void_p * ls)(*[b.data_ptr() for b in bs])
    xcat, dxcat = torch.empty(n, ls * fs, device=dev), torch.randn(n, ls * fs, device=dev, generator=gen)
    ns = int(lib.igcn_sgcn_stack_param_floats(h0, fs, ls))
    dps, scs = torch.empty(ns, device=dev), torch.empty(g * ns, device=dev)

    def stack_fwd():
        for _ in range(ITERS):
            call("igcn_sgcn_stack_fwd", g, rois, emax, h0, fs, ls, ptr(x), ptr(ew), ptr(t.src32), ptr(t.dst32),
                 ptr(t.tgt_ptr), ptr(t.tgt_perm), ptr(t.loop_edge), wp, bp, ptr(xcat), None, stream_ptr())

    def stack_bwd():
        for _ in range(ITERS):
            call("igcn_sgcn_stack_bwd", g, rois, emax, h0, fs, ls, ptr(x), ptr(ew), ptr(t.src32), ptr(t.dst32),
                 ptr(t.tgt_ptr), ptr(t.tgt_perm), ptr(t.src_ptr), ptr(t.src_perm), ptr(t.loop_edge), wp, bp,
                 ptr(dxcat), None, ptr(dx), ptr(dew), ptr(dps), ptr(scs), None, stream_ptr())

    out = {"shape": dict(graphs=g, rois=rois, h0=h0, f1=f1, f3=f3, max_edges=emax, stack_f=fs, stack_layers=ls),
           "lds_bytes": {"ori_fwd": int(lib.igcn_sgcn_ori_lds_bytes(rois, emax, h0, f1, f3, 0)),
                         "ori_bwd": int(lib.igcn_sgcn_ori_lds_bytes(rois, emax, h0, f1, f3, 1)),
                         "stack_fwd": int(lib.igcn_sgcn_stack_lds_bytes(rois, emax, h0, fs, ls, 0)),
                         "stack_bwd": int(lib.igcn_sgcn_stack_lds_bytes(rois, emax, h0, fs, ls, 1))}}
    for name, fn in (("ori_fwd_us", ori_fwd), ("ori_bwd_us", ori_bwd), ("ori_fwd_bwd_autograd_us", ori_fwd_bwd),
                     ("per_layer_fwd_us", layer_fwd), ("per_layer_fwd_bwd_autograd_us", layer_fwd_bwd),
                     ("stack_fwd_us", stack_fwd), ("stack_bwd_us", stack_bwd)):
        out[name] = round(bench._time_graph(fn) / ITERS, 2)
        print(f"{name} ({g} graphs): {out[name]:.2f} us (bwd: + its parameter reduce)", flush=True)
    return out


def _spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": min(ms), "max": max(ms), "blocks": ms}


def _block_ms(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / steps, 4)


def _captured_step(dev, kind):
    from igcn_amd import train
    from igcn_amd.sgcn import SGCN_GCN, SGCN_Ori
    torch.manual_seed(1000)
    if kind == "gcn":
        model = SGCN_GCN(None, bench.LAYERS, bench.HIDDEN, rois=bench.ROIS, H_0=3, num_features=3, num_classes=2).to(dev)
    else:
        model = SGCN_Ori(*DIMS, rois=bench.ROIS).to(dev)
    model.train()
    opt = train.FlatAdam(model.parameters(), lr=1e-3)
    graphs = synth.brain_graph_list(bench.GRAPHS_PER_GPU, seed=1000, rois=bench.ROIS, tsne_dim=16, num_classes=2)
    data = Batch.from_data_list(graphs).to(dev)
    if kind == "per_layer":
        os.environ["IGCN_NO_FUSED_SGCN"] = "1"
    try:
        return train.GraphedTrainStep(model, opt, data)
    finally:
        os.environ.pop("IGCN_NO_FUSED_SGCN", None)


def step_ms(dev, blocks, steps, warmup=10):
    steppers = {k: _captured_step(dev, k) for k in ("fused", "per_layer", "gcn")}
    for s in steppers.values():
        for _ in range(warmup):
            s()
    ms = {k: [] for k in steppers}
    for _ in range(blocks):                          # the routes take turns, block by block
        for k, s in steppers.items():
            ms[k].append(_block_ms(s, steps))
    out = {"SGCN_Ori_fused": _spread(ms["fused"]), "SGCN_Ori_per_layer": _spread(ms["per_layer"]),
           "SGCN_GCN_l2h16": _spread(ms["gcn"])}
    gain = out["SGCN_Ori_per_layer"]["median"] - out["SGCN_Ori_fused"]["median"]
    width = out["SGCN_Ori_per_layer"]["max"] - out["SGCN_Ori_per_layer"]["min"]
    out["fused_gain_ms"], out["per_layer_spread_ms"] = round(gain, 4), round(width, 4)
    out["fused_faster_by_more_than_the_spread"] = bool(gain > width)
    for k, v in out.items():
        if isinstance(v, dict):
            print(f"{k} GraphedTrainStep: {v['median']:.4f} ms per step (median of {blocks} blocks of {steps}; "
                  f"{v['min']:.4f} .. {v['max']:.4f})", flush=True)
    print(f"fused route faster by {gain:.4f} ms; per-layer route's block spread {width:.4f} ms", flush=True)
    return out


def headline(parent_tree, steps, warmup, rounds=3):
    """``python bench.py`` on this tree and on ``parent_tree``, fresh child processes taking turns."""
    trees = {"branch": ROOT, "parent": os.path.abspath(parent_tree)}
    runs = {"branch": [], "parent": []}
    dumps = {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds):
            for name, tree in trees.items():
                cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
                if r == 0:
                    dumps[name] = os.path.join(tmp, name)
                    cmd += ["--dump-outputs", dumps[name]]
                p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=400)
                if p.returncode != 0:
                    raise RuntimeError(f"bench.py ({name}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
                line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                runs[name].append({"ms_per_step": line["ms_per_step"], "timing": line.get("timing")})
                print(f"bench.py, {name}: {line['ms_per_step']} ms per step", flush=True)
        import numpy as np
        files = sorted(os.listdir(dumps["parent"]))
        same = files == sorted(os.listdir(dumps["branch"])) and all(
            np.load(os.path.join(dumps["parent"], f)).tobytes() == np.load(os.path.join(dumps["branch"], f)).tobytes()
            for f in files)
    med = {k: statistics.median(r["ms_per_step"] for r in v) for k, v in runs.items()}
    lo = min(r["ms_per_step"] for r in runs["parent"])
    hi = max(r["ms_per_step"] for r in runs["parent"])
    out = {"workload": f"python bench.py --gpus 1 --steps {steps} --warmup {warmup}; {rounds} child processes per tree, "
                       "taking turns", "runs": runs, "median_ms": med, "parent_min_ms": lo, "parent_max_ms": hi,
           "branch_median_within_parent_spread": bool(lo <= med["branch"] <= hi),
           "dump_outputs_files": len(files), "dump_outputs_bit_identical": bool(same)}
    print(f"headline: branch median {med['branch']} ms, parent median {med['parent']} ms, parent runs {lo} .. {hi} ms; "
          f"--dump-outputs bit-identical: {same} ({len(files)} arrays)", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit to run bench.py against")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.load()
    res = {}
    if not args.skip_kernels:
        res["kernels"] = {"g256": kernel_us(dev, 256), "g512": kernel_us(dev, 512)}
    if not args.skip_step:
        res["step"] = step_ms(dev, args.blocks, args.steps)
    if args.parent_tree:
        res["headline"] = headline(args.parent_tree, args.bench_steps, args.bench_warmup)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
