#!/usr/bin/env python3
"""Cost of a captured SGCN_GCN_CLUSTERLABEL train step, of its fused two-head loss launch and of its regulariser.

SGCN_GCN_CLUSTERLABEL(2, 16, isCrossAtten=True) at B = 256 graphs x 90 ROIs (H_0 = 1, the reference's default), the
synthetic 3000-node GO DAG (bench.POOL), dropout on, lambda0 = 1e-5.  Three parts:

  1. ``step`` — ms per captured train step (GraphedTrainStep; median of ``--blocks`` blocks of ``--steps`` hot replays,
     with the spread) of the model on its fused route, of the same model under IGCN_NO_HEAD_LOSS_FUSED=1
     (ops.small_linear_pair + log_softmax + nll_loss + the torch reconstruction sum) and of the headline
     SGCN_GCN_IMGSNP step of bench.py on the same batch, the three taking turns block by block;
  2. ``launches`` — us per launch, hot (a hipGraph of 50 launches between two events), of igcn_cluster_head_loss_fwd and
     of igcn_mask_reg3_fwd / _bwd at the step's shapes, and of the headline's narrow-layer launches at theirs
     (igcn_head_loss_gram_fwd, igcn_head_loss_fwd, igcn_small_linear_pair_fwd / _bwd); ``--launches-only`` runs this part alone (an A/B of
     two builds of the library: one run per build, taking turns);
  3. ``--trace fused|unfused`` runs 40 eager train steps of one route and nothing else — the program to put behind
     ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR --``, once per route, in runs of their own;
     ``--summarise DIR_FUSED DIR_UNFUSED`` then lists every kernel whose launches per step differ between the two routes
     with its us per step: the fused launch on one side, the launches it replaces on the other.

    timeout -k 10 600 python tools/clusterlabel_bench.py --out profiles/clusterlabel_bench.json
"""
import argparse
import csv
import glob
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

ITERS, TRACE_STEPS = 50, 40


def _batch(dev, h0):
    d = Batch.from_data_list(synth.brain_graph_list(bench.GRAPHS_PER_GPU, seed=1000, rois=bench.ROIS, h0=h0,
                                                    tsne_dim=90)).to(dev)
    d.x.requires_grad_(True)
    return d


def cluster_model(dev):
    from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
    torch.manual_seed(1000)
    go_snps, adj, pool_dim = synth.go_hierarchy(bench.POOL, seed=0)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, dev)
    model = SGCN_GCN_CLUSTERLABEL(bench.LAYERS, bench.HIDDEN, a_g, a, pool_dim, 32, dev, isCrossAtten=True).to(dev)
    model.train()
    return model


def cluster_step(dev, fused):
    from igcn_amd.train import FlatAdam, GraphedTrainStep
    model = cluster_model(dev)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    if not fused:
        os.environ["IGCN_NO_HEAD_LOSS_FUSED"] = "1"            # (read while the step is captured)
    try:
        return GraphedTrainStep(model, opt, _batch(dev, 1))
    finally:
        os.environ.pop("IGCN_NO_HEAD_LOSS_FUSED", None)


def headline_step(dev):
    from igcn_amd.train import FlatAdam, GraphedTrainStep
    model, _ = bench.build_model(dev)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    return GraphedTrainStep(model, opt, _batch(dev, 3))


def _spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": min(ms), "max": max(ms), "blocks": ms}


def step_ms(dev, blocks, steps, warmup=10):
    steppers = {"clusterlabel_fused": cluster_step(dev, True), "clusterlabel_unfused": cluster_step(dev, False),
                "headline": headline_step(dev)}
    for s in steppers.values():
        for _ in range(warmup):
            s()
    ms = {k: [] for k in steppers}
    for _ in range(blocks):                          # the three take turns, block by block
        for k, s in steppers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                s()
            torch.cuda.synchronize()
            ms[k].append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    out = {k: _spread(v) for k, v in ms.items()}
    gain = out["clusterlabel_unfused"]["median"] - out["clusterlabel_fused"]["median"]
    width = max(v["max"] - v["min"] for k, v in out.items() if k.startswith("clusterlabel"))
    out["fused_gain_ms"], out["block_spread_ms"] = round(gain, 4), round(width, 4)
    out["fused_faster_by_more_than_the_spread"] = bool(gain > width)
    out["timing"] = f"median of {blocks} blocks of {steps} hot hipGraph replays after {warmup}, the steps taking turns"
    for k, v in out.items():
        if isinstance(v, dict):
            print(f"{k}: {v['median']:.4f} ms per step ({v['min']:.4f} .. {v['max']:.4f})", flush=True)
    print(f"fused route faster by {gain:.4f} ms; widest block spread {width:.4f} ms", flush=True)
    return out


def launch_us(dev):
    """The two new launches alone at the step's shapes: B = 256, K = 64, (C1, C2) = (3, 2), S = 54; prob [90, 1], one edge
    mask value per edge of the batch, snps_prob [1, 54]."""
    from igcn_amd._lib import call, ptr, stream_ptr
    lib = _lib.load()
    b, k, c1, c2, s = bench.GRAPHS_PER_GPU, 64, 3, 2, 54
    r = lambda *sh: torch.randn(*sh, device=dev)                             # noqa: E731
    x1, x2, w1, b1, w2, b2 = r(2 * b, k).relu(), r(2 * b, k).relu(), r(c1, k), r(c1), r(c2, k), r(c2)
    keep1, keep2 = ((torch.rand(2 * b, k, device=dev) > 0.5).float() * 2 for _ in range(2))
    y, cy = torch.randint(0, c1, (b,), device=dev), torch.randint(0, c2, (b,), device=dev)
    x_hat, snps = r(2 * b, s), torch.rand(b, s, device=dev)
    nblk = int(lib.igcn_cluster_head_loss_blocks(b, k))
    wcols = c1 * k + c1 + c2 * k + c2
    e = lambda *sh: torch.empty(*sh, device=dev)                             # noqa: E731
    o = [e(2 * b, c1), e(2 * b, c2), e(2 * b, k), e(2 * b, k), e(2 * b, s), e(nblk, 5), e(nblk, wcols), e(1)]

    def head():
        for _ in range(ITERS):
            call("igcn_cluster_head_loss_fwd", b, k, c1, c2, s, ptr(x1), ptr(keep1), ptr(w1), ptr(b1), ptr(x2), ptr(keep2),
                 ptr(w2), ptr(b2), ptr(y), ptr(cy), ptr(x_hat), ptr(snps), 1.0, 1.0, 1e-5, 1, *[ptr(t) for t in o],
                 stream_ptr())
    n_edge = int(_batch(dev, 1).edge_attr.numel())
    prob, em, sp = r(90), torch.rand(n_edge, device=dev).clamp(1e-3, 1 - 1e-3), r(54)
    scratch, gout = e(1024), torch.ones(1, device=dev)
    dp, de, ds = e(90), e(n_edge), e(54)
    hp = (0.1, 0.1, 0.1, 0.1, 5.4, 0.1, 1e-6)

    def reg_fwd():
        for _ in range(ITERS):
            call("igcn_mask_reg3_fwd", 90, n_edge, 54, ptr(prob), ptr(em), ptr(sp), *hp, None, ptr(scratch), stream_ptr())

    def reg_bwd():
        for _ in range(ITERS):
            call("igcn_mask_reg3_bwd", 90, n_edge, 54, ptr(prob), ptr(em), ptr(sp), *hp, ptr(gout), ptr(dp), ptr(de),
                 ptr(ds), stream_ptr())
    out = {"shape": {"B": b, "K": k, "C1": c1, "C2": c2, "S": s, "head_loss_blocks": nblk, "n_edge": n_edge,
                     "mask_reg_blocks": int(lib.igcn_mask_reg_blocks(90 + n_edge + 54))},
           "timing": f"hot: a hipGraph of {ITERS} launches between two events, best of 3, per launch"}
    launches = [("cluster_head_loss_fwd_us", head), ("mask_reg3_fwd_us", reg_fwd), ("mask_reg3_bwd_us", reg_bwd)]
    for name, fn in launches + headline_launches(dev, out["shape"]):
        out[name] = round(bench._time_graph(fn) / ITERS, 2)
        print(f"{name}: {out[name]:.2f} us", flush=True)
    return out


def headline_launches(dev, shape):
    """The headline trainer's narrow-layer launches at its step's shapes: B = 256, K = 64, (C, NR) = (2, 4), S = 54, the
    Gram role on out_z [2B, 40] with tsne [B, 90]; the unfused pair forward / backward on the same 2B rows."""
    import ctypes
    from igcn_amd._lib import call, ptr, stream_ptr
    lib = _lib.load()
    b, k, c, nr, s, rd, groups, t_dim = bench.GRAPHS_PER_GPU, 64, 2, 4, 54, 40, 2, 90
    shape["headline"] = {"B": b, "K": k, "C": c, "NR": nr, "S": s, "RD": rd, "groups": groups, "T": t_dim}
    r = lambda *sh: torch.randn(*sh, device=dev)                             # noqa: E731
    e = lambda *sh: torch.empty(*sh, device=dev)                             # noqa: E731
    x1, x2, w1, b1, w2, b2 = r(2 * b, k).relu(), r(2 * b, k).relu(), r(c, k), r(c), r(nr, k), r(nr)
    keep1, keep2 = ((torch.rand(2 * b, k, device=dev) > 0.5).float() * 2 for _ in range(2))
    y, clin, x_hat, snps = torch.randint(0, c, (b,), device=dev), r(b, nr), r(2 * b, s), torch.rand(b, s, device=dev)
    nblk = int(lib.igcn_head_loss_blocks(b, k))
    o = [e(2 * b, c), e(2 * b, nr), e(2 * b, k), e(2 * b, k), e(2 * b, s), e(nblk, 4), e(nblk, c * k + c + nr * k + nr),
         e(4), e(1)]
    z = r(groups, b, rd)
    gram, tsne = (z @ z.transpose(1, 2)).contiguous(), r(b, t_dim)
    lap, gscr, sym = e(b, b), e(b, 2 * groups), e(groups, b, b)
    lam6, gout = (ctypes.c_float * 6)(1.0, 1.0, 1.0, 1e-5, 0.1, 0.1), (ctypes.c_float * (2 * groups))(*[0.1] * (2 * groups))

    def head_gram():
        for _ in range(ITERS):
            call("igcn_head_loss_gram_fwd", b, k, c, nr, s, ptr(x1), ptr(keep1), ptr(w1), ptr(b1), ptr(x2), ptr(keep2),
                 ptr(w2), ptr(b2), ptr(y), ptr(clin), ptr(x_hat), ptr(snps), lam6, 1.0, 1.0, *[ptr(t) for t in o], b, rd,
                 groups, ptr(gram), ptr(tsne), t_dim, 0.05, ptr(lap), ptr(gscr), gout, ptr(sym), stream_ptr())

    def head_alone():                                # (the head role without the Gram rows: igcn_head_loss_fwd)
        for _ in range(ITERS):
            call("igcn_head_loss_fwd", b, k, c, nr, s, ptr(x1), ptr(keep1), ptr(w1), ptr(b1), ptr(x2), ptr(keep2), ptr(w2),
                 ptr(b2), ptr(y), ptr(clin), ptr(x_hat), ptr(snps), lam6, 1.0, 1.0, *[ptr(t) for t in o], stream_ptr())
    rows = 2 * b
    y1, y2, dy1, dy2, dx1, dx2 = e(rows, c), e(rows, nr), r(rows, c), r(rows, nr), e(rows, k), e(rows, k)
    dwb1, dwb2 = e(c * k + c), e(nr * k + nr)
    s1 = e(int(lib.igcn_small_linear_bwd_scratch_floats(rows, k, c)))
    s2 = e(int(lib.igcn_small_linear_bwd_scratch_floats(rows, k, nr)))

    def pair_fwd():
        for _ in range(ITERS):
            call("igcn_small_linear_pair_fwd", rows, k, c, ptr(x1), ptr(keep1), ptr(w1), ptr(b1), ptr(y1), nr, ptr(x2),
                 ptr(keep2), ptr(w2), ptr(b2), ptr(y2), stream_ptr())

    def pair_bwd():                                  # (the kernel and its two short reductions of block partials)
        for _ in range(ITERS):
            call("igcn_small_linear_pair_bwd", rows, k, c, ptr(x1), ptr(keep1), ptr(w1), ptr(dy1), ptr(dx1), ptr(dwb1),
                 ptr(s1), nr, ptr(x2), ptr(keep2), ptr(w2), ptr(dy2), ptr(dx2), ptr(dwb2), ptr(s2), stream_ptr())
    return [("head_loss_gram_fwd_us", head_gram), ("head_loss_fwd_us", head_alone), ("small_linear_pair_fwd_us", pair_fwd),
            ("small_linear_pair_bwd_us", pair_bwd)]


def trace_workload(dev, route):
    from igcn_amd.train import FlatAdam, train_step
    if route == "unfused":
        os.environ["IGCN_NO_HEAD_LOSS_FUSED"] = "1"
    model = cluster_model(dev)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    data = _batch(dev, 1)
    for _ in range(TRACE_STEPS):
        train_step(model, opt, data)
    torch.cuda.synchronize()
    print(f"{route}: {TRACE_STEPS} eager train steps", flush=True)


def _stats(d):
    path = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
    return {r["Name"]: (int(r["Calls"]) / TRACE_STEPS, float(r["TotalDurationNs"]) / 1e3 / TRACE_STEPS)
            for r in csv.DictReader(open(path))}


def summarise(fused_dir, unfused_dir):
    """Kernels whose launches per step differ between the two traced routes, and each route's whole step."""
    a, b = _stats(fused_dir), _stats(unfused_dir)
    out = {"steps_traced": TRACE_STEPS, "fused_only": {}, "unfused_only": {},
           "kernel_us_per_step": {"fused": round(sum(v[1] for v in a.values()), 1),
                                  "unfused": round(sum(v[1] for v in b.values()), 1)},
           "launches_per_step": {"fused": round(sum(v[0] for v in a.values()), 1),
                                 "unfused": round(sum(v[0] for v in b.values()), 1)}}
    for name in sorted(set(a) | set(b)):
        ca, ta = a.get(name, (0.0, 0.0))
        cb, tb = b.get(name, (0.0, 0.0))
        if abs(ca - cb) < 0.5:
            continue
        side = "fused_only" if ca > cb else "unfused_only"
        out[side][name[:100]] = {"launches_per_step": round(abs(ca - cb), 2), "us_per_step": round(abs(ta - tb), 2)}
    out["fused_launch_us"] = round(sum(v["us_per_step"] for v in out["fused_only"].values()), 2)
    out["replaced_launches_us"] = round(sum(v["us_per_step"] for v in out["unfused_only"].values()), 2)
    print(f"fused route only: {out['fused_launch_us']} us per step in {len(out['fused_only'])} kernel(s); "
          f"unfused route only: {out['replaced_launches_us']} us per step in {len(out['unfused_only'])} kernel(s)")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write (or, with --summarise, extend) the numbers as JSON in this file")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--trace", choices=["fused", "unfused"], default=None)
    ap.add_argument("--launches-only", action="store_true", help="part 2 alone")
    ap.add_argument("--summarise", nargs=2, metavar=("DIR_FUSED", "DIR_UNFUSED"), default=None)
    args = ap.parse_args()
    res = {}
    if args.summarise:
        if args.out and os.path.exists(args.out):
            res = json.load(open(args.out))
        res["kernel_trace"] = summarise(*args.summarise)
    else:
        dev = torch.device("cuda", 0)
        _lib.load()
        if args.trace:
            return trace_workload(dev, args.trace)
        if not args.launches_only:
            res["step"] = step_ms(dev, args.blocks, args.steps)
        res["launches"] = launch_us(dev)
        res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
