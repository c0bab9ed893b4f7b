#!/usr/bin/env python3
"""Cost of the GO read-out (node-wise linear + BatchNorm over nodes + ReLU) at the attention widths of the hidden-32 sweep,
next to a tensor-library composite of the same function and to the bytes it has to move.

Shape: B = 512 samples (two passes of 256), F = 5 inputs per node, N = 400 nodes, 2 groups, training mode; D = 64 (the
row-coalesced `_q` kernels), 96 / 128 / 160 (the strip kernels k_nlbn_*_w), and D = 32 on the kernels the benchmark's own
step uses, to show that path next to its history under profiles/.  Per width: ops.NodeLinearBN forward, and forward +
backward through autograd, beside ``composite`` below (transpose / matmul / batch_norm per group / relu, autograd's own
backward).  Hot replays of a captured graph of ``ITERS`` calls, device events around a block of ``REPLAYS`` replays; after
a warm-up the two forms take turns block by block; median and spread of ``--blocks`` blocks each.

Byte floor: ``out`` [B, N, D] written once forward; ``dout`` read twice (statistics pass, apply pass) and ``dx`` [B, F, N]
written once backward; x and the per-node vectors are small.  Achieved bytes/s = floor bytes / measured time.

    timeout -k 10 600 python tools/readout_wide_bench.py --out profiles/readout_wide_bench.json
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
ITERS, REPLAYS = 10, 5
B, F, N, GROUPS = 512, 5, 400, 2
WIDTHS = (32, 64, 96, 128, 160)


def _spread(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "blocks": [round(x, digits) for x in v]}


def composite(x, w, gamma, beta, rm, rv, groups):
    import torch
    pre = x.transpose(1, 2) @ w.t()                                       # [B, N, D]
    bg = x.shape[0] // groups
    return torch.cat([torch.relu(torch.nn.functional.batch_norm(pre[g * bg:(g + 1) * bg], rm, rv, gamma, beta, True, 0.1,
                                                                1e-5)) for g in range(groups)])


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


def width_us(dev, d, blocks, warmup=3):
    import torch
    from igcn_amd import ops
    gen = torch.Generator(device=dev).manual_seed(d)
    x = (torch.randn(B, F, N, device=dev, generator=gen) + 0.5).requires_grad_(True)
    w = (torch.randn(d, F, device=dev, generator=gen) * 0.6).requires_grad_(True)
    gamma = torch.ones(N, device=dev, requires_grad=True)
    beta = torch.zeros(N, device=dev, requires_grad=True)
    cot = torch.randn(B, N, d, device=dev, generator=gen)
    leaves = [x, w, gamma, beta]
    stats = {k: (torch.zeros(N, device=dev), torch.ones(N, device=dev)) for k in ("kernel", "composite")}
    forms = {"kernel": lambda: ops.NodeLinearBN.apply(x, w, gamma, beta, *stats["kernel"], True, 0.1, 1e-5, GROUPS),
             "composite": lambda: composite(x, w, gamma, beta, *stats["composite"], GROUPS)}

    def fwd(f):
        def run():
            with torch.no_grad():
                for _ in range(ITERS):
                    f()
        return run

    def fwd_bwd(f):
        def run():
            for _ in range(ITERS):
                torch.autograd.backward(f(), cot, inputs=leaves)
                for t in leaves:
                    t.grad = None
        return run
    with torch.no_grad():
        err = float((forms["kernel"]() - forms["composite"]()).abs().max())
    floor = {"fwd": 4 * B * N * d, "fwd_bwd": 4 * (3 * B * N * d + B * F * N)}
    out = {"shape": dict(B=B, F=F, N=N, D=d, groups=GROUPS), "max_abs_kernel_minus_composite": err,
           "floor_bytes": floor}
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
        row = {k + "_us": _spread(v) for k, v in us.items()}
        for k in graphs:
            row[k + "_floor_GBps"] = round(floor[what] / row[k + "_us"]["median"] * 1e-3, 1)
        gap = row["kernel_us"]["median"] - row["composite_us"]["median"]
        width = max(row["kernel_us"]["max"] - row["kernel_us"]["min"], row["composite_us"]["max"] - row["composite_us"]["min"])
        row["kernel_minus_composite_us"], row["larger_block_spread_us"] = round(gap, 2), round(width, 2)
        row["kernel_faster"] = bool(gap < 0)
        out[what] = row
        print(f"D={d} {what}: kernel {row['kernel_us']['median']:.2f} us ({row['kernel_us']['min']:.2f} .. "
              f"{row['kernel_us']['max']:.2f}; {row['kernel_floor_GBps']} GB/s of the floor's bytes), composite "
              f"{row['composite_us']['median']:.2f} us ({row['composite_us']['min']:.2f} .. "
              f"{row['composite_us']['max']:.2f}); median of {blocks} blocks of {ITERS * REPLAYS} hot calls", flush=True)
        del graphs
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--widths", type=int, nargs="*", default=list(WIDTHS))
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks: at least five timed blocks")
    import torch
    import igcn_amd  # noqa: F401
    from igcn_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    res = {"tool": "tools/readout_wide_bench.py", "device": torch.cuda.get_device_name(0),
           "timing": f"hot: captured graphs of {ITERS} calls, {REPLAYS} replays between two device events per block, "
                     f"kernel and composite taking turns; median / min / max of {args.blocks} blocks, us per call",
           "floor": "out written once forward; dout read twice and dx written once backward",
           "widths": {str(d): width_us(dev, d, args.blocks) for d in args.widths}}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
