#!/usr/bin/env python3
"""Cost of the exact-fp32 attention core at head_dim 48 / 64 / 80 next to the batched-GEMM + softmax composite it
replaced there, and of the hidden-32 sweep's first wide row as a train step.

  1. ``core`` — us per call at B = 256 samples, Lq = 90 queries, Lk = 400 keys (the GO hierarchy of bench.py: its three
     top levels, 300 + 99 + 1 nodes), H = 2, D = 96 / 128 / 160: ops.AttentionCore forward, and forward + backward
     through autograd, beside the composite expression on the same projected inputs (written out below: two batched
     GEMMs and a softmax forward, autograd's saved [B, H, Lq, Lk] probabilities backward).  Hot replays of a captured
     graph of ``ITERS`` calls, device events around a block of replays; after a warm-up the two forms take turns block by block;
     median and spread of ``--blocks`` blocks each.
  2. ``step`` — ms per captured train step (GraphedTrainStep) of SGCN_GCN_IMGSNP(3, 32, ...) at 256 graphs x 90 ROIs on
     the 3000-node GO DAG (attention width 96, head_dim 48), median and spread of ``--blocks`` blocks.  Where a launch of
     that model refuses the shape, the error text is recorded in place of a time.
  3. ``--parent-tree DIR`` (a checkout of the parent commit WITH its built library): ``step_vs_parent`` — the same step of this tree and of that one, a fresh child process per tree and
     turn (``--tree DIR --step-blocks``), the trees taking turns.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run every GPU step under a time limit, e.g.
    timeout -k 10 600 python tools/attn_wide_bench.py --out profiles/attn_wide_bench.json
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ITERS, REPLAYS = 10, 5                                # calls per captured graph, replays per timed block
WIDTHS = (96, 128, 160)
HEADS, LQ, BATCH = 2, 90, 256
STEP_MODEL = (3, 32)                                  # (layers, hidden): main.py:142-145, the first row above head_dim 32


def _spread(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "blocks": [round(x, digits) for x in v]}


def composite(q, kv, h):
    """softmax(q k^T / sqrt(hd)) v per head from the projection outputs q [B, Lq, D], kv [B, Lk, 2 D] = key | value: what
    SGCN_GCN_IMGSNP._cross_attention runs where the core does not cover the width."""
    import torch
    b, lq, d = q.shape
    lk, hd = kv.shape[1], d // h
    qh = q.view(b, lq, h, hd).transpose(1, 2)
    kvh = kv.view(b, lk, 2, h, hd)
    att = torch.softmax((qh @ kvh[:, :, 0].permute(0, 2, 3, 1)) * (1.0 / math.sqrt(hd)), dim=-1)
    return (att @ kvh[:, :, 1].transpose(1, 2)).transpose(1, 2).reshape(b, lq, d)


def _graph_of(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    return g


def _replay_us(g):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (ITERS * REPLAYS)


def core_us(dev, d, lk, blocks, warmup=3):
    import torch
    from igcn_amd import _lib, ops
    gen = torch.Generator(device=dev).manual_seed(d)
    q = torch.randn(BATCH, LQ, d, device=dev, generator=gen).requires_grad_(True)
    kv = torch.randn(BATCH, lk, 2 * d, device=dev, generator=gen).requires_grad_(True)
    cot = torch.randn(BATCH, LQ, d, device=dev, generator=gen)
    if not ops.attn_core_supported(d, HEADS, LQ, lk):
        raise _lib.IgcnError(f"the attention core does not cover D={d} H={HEADS} Lq={LQ} Lk={lk}")
    forms = {"core": lambda: ops.AttentionCore.apply(q, kv, HEADS), "composite": lambda: composite(q, kv, HEADS)}

    def fwd(f):
        def run():
            with torch.no_grad():
                for _ in range(ITERS):
                    f()
        return run

    def fwd_bwd(f):
        def run():
            for _ in range(ITERS):
                torch.autograd.backward(f(), cot, inputs=[q, kv])
                q.grad = kv.grad = None
        return run
    with torch.no_grad():
        err = float((forms["core"]() - forms["composite"]()).abs().max())
    lib = _lib.load()
    out = {"shape": dict(B=BATCH, H=HEADS, Lq=LQ, Lk=lk, D=d, head_dim=d // HEADS),
           "lds_bytes": {"fwd": int(lib.igcn_attn_core_lds_bytes(d, HEADS, LQ, lk, 0)),
                         "bwd": int(lib.igcn_attn_core_lds_bytes(d, HEADS, LQ, lk, 1))},
           "max_abs_core_minus_composite": err}
    for what, wrap in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
        graphs = {k: _graph_of(wrap(f)) for k, f in forms.items()}
        for g in graphs.values():
            for _ in range(warmup):
                g.replay()
        torch.cuda.synchronize()
        us = {k: [] for k in graphs}
        for _ in range(blocks):                          # the two forms take turns, block by block
            for k, g in graphs.items():
                us[k].append(_replay_us(g))
        row = {k + "_us": _spread(v, 2) for k, v in us.items()}
        gap = row["core_us"]["median"] - row["composite_us"]["median"]
        width = max(row["core_us"]["max"] - row["core_us"]["min"], row["composite_us"]["max"] - row["composite_us"]["min"])
        row["core_minus_composite_us"], row["larger_block_spread_us"] = round(gap, 2), round(width, 2)
        row["core_slower_by_more_than_the_spread"] = bool(gap > width)
        out[what] = row
        print(f"D={d} {what}: core {row['core_us']['median']:.2f} us ({row['core_us']['min']:.2f} .. "
              f"{row['core_us']['max']:.2f}), composite {row['composite_us']['median']:.2f} us "
              f"({row['composite_us']['min']:.2f} .. {row['composite_us']['max']:.2f}); median of {blocks} blocks of "
              f"{ITERS * REPLAYS} hot calls", flush=True)
        del graphs
    return out


def step_blocks(dev, blocks, steps, warmup=10):
    """ms per captured SGCN_GCN_IMGSNP(3, 32) train step, block by block, for the package first on sys.path."""
    import torch
    import bench
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from igcn_amd.train import FlatAdam, GraphedTrainStep
    wl = bench.WORKLOADS["full"]
    model, _ = bench.build_model(dev, wl, layers=STEP_MODEL[0], hidden=STEP_MODEL[1])
    opt = FlatAdam(model.parameters(), lr=1e-3)
    data = Batch.from_data_list(synth.brain_graph_list(BATCH, seed=1000, rois=wl["rois"], tsne_dim=90)).to(dev)
    data.x.requires_grad_(True)
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
        ms.append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    return ms, float(step.loss)


def step_vs_parent(parent_tree, blocks, steps, rounds=3):
    """The step of this tree and of ``parent_tree``: fresh child processes taking turns.  A tree whose model refuses the
    shape is recorded with the error text of its first child and not started again."""
    trees = {"branch": os.path.dirname(HERE), "parent": os.path.abspath(parent_tree)}
    runs, errors = {k: [] for k in trees}, {}
    for _ in range(rounds):
        for name, tree in trees.items():
            if name in errors:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--step-blocks", "--blocks", str(blocks),
                   "--steps", str(steps)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:
                raise RuntimeError(f"step of the {name} tree failed with {p.returncode}:\n{p.stderr[-2000:]}")
            row = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            if "error" in row:
                errors[name] = row["error"]
                print(f"step, {name}: not measured: {row['error']}", flush=True)
                continue
            runs[name].append(row)
            print(f"step, {name}: {statistics.median(row['ms'])} ms (blocks {row['ms']}; loss {row['loss']})", flush=True)
    out = {"workload": f"captured SGCN_GCN_IMGSNP{STEP_MODEL} train step, {BATCH} graphs x 90 ROIs, 3000-node GO DAG; "
                       f"{rounds} child processes per tree taking turns, {blocks} blocks of {steps} replays each",
           "runs": runs, "errors": errors}
    timed = {k: v for k, v in runs.items() if v}
    out["median_ms"] = {k: round(statistics.median(statistics.median(r["ms"]) for r in v), 4) for k, v in timed.items()}
    out["spread_ms"] = {k: [min(x for r in v for x in r["ms"]), max(x for r in v for x in r["ms"])] for k, v in timed.items()}
    if len(timed) == 2:
        out["branch_minus_parent_ms"] = round(out["median_ms"]["branch"] - out["median_ms"]["parent"], 4)
    print(f"step: median ms per step {out['median_ms']}; not measured {sorted(errors)}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="the checkout to time (default: the one this file is in)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit to time the step of")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--step-blocks", action="store_true", help="only the step of --tree: one JSON line (the child mode)")
    ap.add_argument("--skip-core", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks: at least five timed blocks")
    sys.path.insert(0, os.path.abspath(args.tree))       # imports happen after the arguments are read
    import torch
    import bench
    from igcn_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    if args.step_blocks:
        try:
            ms, loss = step_blocks(dev, args.blocks, args.steps)
            print(json.dumps({"ms": ms, "loss": round(loss, 5)}))
        except _lib.IgcnError as exc:                     # a launch the model needs refuses the shape: say which
            print(json.dumps({"error": str(exc)[:300]}))
        return
    lk = sum(bench.POOL[2:])                            # the GO levels the attention reads as keys (bench.py roofline)
    res = {}
    if not args.skip_core:
        res["core"] = {f"D{d}": core_us(dev, d, lk, args.blocks) for d in WIDTHS}
    if not args.skip_step:
        try:
            ms, loss = step_blocks(dev, args.blocks, args.steps)
            res["step"] = {"model": f"SGCN_GCN_IMGSNP{STEP_MODEL}", "graphs": BATCH, "ms_per_step": _spread(ms),
                           "loss": round(loss, 5)}
            print(f"step: {res['step']['ms_per_step']['median']} ms (blocks {ms})", flush=True)
        except _lib.IgcnError as exc:                     # a launch the model needs refuses the shape: say which
            res["step"] = {"model": f"SGCN_GCN_IMGSNP{STEP_MODEL}", "graphs": BATCH, "error": str(exc)[:300]}
            print(f"step: not measured: {exc}", flush=True)
    if args.parent_tree:
        try:
            res["step_vs_parent"] = step_vs_parent(args.parent_tree, args.blocks, args.steps)
        except RuntimeError as exc:
            res["step_vs_parent"] = {"error": str(exc)[-300:]}
            print(f"step_vs_parent: not measured: {str(exc)[-300:]}", flush=True)
    res["device"] = torch.cuda.get_device_name(0)
    res["timing"] = (f"core: device events around {REPLAYS} hot replays of a captured graph of {ITERS} calls per block, 3 warm-up "
                     f"replays, "
                     f"median / min / max of {args.blocks} blocks, the two forms alternating; step: host clock around "
                     f"{args.steps} replays ending in a synchronise, 10 warm-up steps, {args.blocks} blocks")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
