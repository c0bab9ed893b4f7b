#!/usr/bin/env python3
"""The heat-kernel GDC launch beside the PPR launch (igcn_gdc_diffuse / igcn_gdc_topk), the GDC-fed captured train step
with either kernel, and the reference-style host loop (scipy.linalg.expm per subject) they replace.

    python3 tools/gdc_heat_bench.py [--graphs 256] [--rois 90] [--out profiles/gdc_heat_bench.json]

Everything is recorded, nothing is gated.  Launch times: device events around ``--reps`` launches into preallocated
outputs, the two kernels taking turns in one process, median (min .. max) of ``--blocks`` blocks.  Needs a GPU."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOP_K, T, ALPHA, DEGREE = 3, 5.0, 0.05, 14              # DEGREE: csrc/gdc_common.h GDC_HEAT_DEGREE


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "blocks": xs}


def host_heat_topk(a, k=TOP_K, t=T):
    """What util_gdc.py does per subject: get_heat_matrix, get_top_k_matrix, coo_matrix."""
    from scipy.linalg import expm
    from scipy.sparse import coo_matrix
    a = a.astype(np.float64)
    d = np.diag(1 / np.sqrt(a.sum(axis=1)))
    s = expm(-t * (np.eye(a.shape[0]) - d @ a @ d))
    s[s.argsort(axis=0)[:a.shape[0] - k], np.arange(a.shape[0])] = 0.0
    norm = s.sum(axis=0)
    norm[norm <= 0] = 1
    coo = coo_matrix(s / norm)
    return np.vstack([coo.row, coo.col]), coo.data.astype(np.float32)


def squarings(a, t=T):
    """The scaling exponent the kernel chooses for this matrix: smallest s with |t H|_1 / 2^s <= 1/2."""
    a = a.astype(np.float64)
    d = 1 / np.sqrt(a.sum(axis=1))
    nrm = t * np.abs(d[:, None] * a * d[None, :]).sum(axis=0).max()
    s = 0
    while nrm > 0.5:
        nrm, s = nrm / 2, s + 1
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--rois", type=int, default=90)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gdc_heat_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gdc_heat_bench: no GPU")
    import bench
    import igcn_amd  # noqa: F401
    from igcn_amd import synth
    from igcn_amd._lib import call, ptr, stream_ptr
    from igcn_amd.data import Batch, Data
    from igcn_amd.loader import DeviceGdcFeeder, UniformGraphStore
    from igcn_amd.train import FlatAdam, GraphedTrainStep
    dev = torch.device("cuda", 0)
    b, r = args.graphs, args.rois
    graphs = synth.brain_graph_list(2 * b, seed=3000, rois=r, tsne_dim=90)
    adj = torch.stack([g.A for g in graphs]).to(dev).contiguous()
    host_adj = [g.A.numpy() for g in graphs[:b]]
    sq = [squarings(a) for a in host_adj]
    res = {"graphs": b, "rois": r, "top_k": TOP_K, "t": T, "alpha": ALPHA, "device": torch.cuda.get_device_name(0),
           "squarings_per_graph": {"min": min(sq), "max": max(sq)}, "taylor_degree": DEGREE}

    # ---- the two launches, taking turns ----------------------------------------------------------------
    ei = torch.empty(2, b * r * TOP_K, dtype=torch.int64, device=dev)
    ew = torch.empty(b * r * TOP_K, dtype=torch.float32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    launch = {
        "heat": lambda: call("igcn_gdc_diffuse", b, r, 1, T, 0, TOP_K, 0.0, ptr(adj), b, None, ptr(ei), ptr(ew),
                             ptr(counts), stream_ptr()),
        "ppr": lambda: call("igcn_gdc_topk", b, r, TOP_K, ALPHA, ptr(adj), ptr(ei), ptr(ew), ptr(counts), stream_ptr()),
    }
    for fn in launch.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {"heat": [], "ppr": []}
    for _ in range(args.blocks):
        for name, fn in launch.items():
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
    res["launch_us"] = {k: stats(v) for k, v in times.items()}
    res["launch_us"]["heat_over_ppr"] = res["launch_us"]["heat"]["median"] / res["launch_us"]["ppr"]["median"]
    rp = (r + 15) // 16 * 16
    flops = sum((DEGREE - 1 + s) * 2 * rp ** 3 for s in sq)                     # the products, padded size
    res["heat_products"] = {"flop_per_batch": flops, "padded_rois": rp,
                            "tflops_over_launch_time": flops / (res["launch_us"]["heat"]["median"] * 1e-6) / 1e12}

    # ---- the GDC-fed captured headline step with either kernel -------------------------------------------
    wl = bench.WORKLOADS["full"]
    if wl["graphs"] == b and wl["rois"] == r:
        model, _ = bench.build_model(dev, wl)
        opt = FlatAdam(model.parameters(), lr=1e-3)
        data = Batch.from_data_list(graphs[:b]).to(dev)
        data.x.requires_grad_(True)
        step = GraphedTrainStep(model, opt, data)
        keep = ("x", "edge_index", "edge_attr", "snps_feat", "y", "clini_score", "tsne_fdim", "clust_y")
        store = UniformGraphStore([Data(**{n: getattr(g, n) for n in keep}) for g in graphs], dev)
        cols = {n: store.cols[n] for n in ("x", "snps_feat", "y", "clini_score", "tsne_fdim", "clust_y")}
        cur = torch.cuda.current_stream()
        total = 3 + args.blocks * args.steps
        feeds = {name: iter(DeviceGdcFeeder(adj, cols, b, total, top_k=TOP_K, alpha=ALPHA, seed=1, kernel=name, t=T))
                 for name in ("heat", "ppr")}

        def consume(batch):
            cur.wait_event(batch.ready)
            step.load(batch)
            batch.release()
            step()
        for feed in feeds.values():
            for _ in range(3):
                consume(next(feed))
        torch.cuda.synchronize()
        fed = {"heat": [], "ppr": []}
        for _ in range(args.blocks):
            for name, feed in feeds.items():
                e0.record()
                for _ in range(args.steps):
                    consume(next(feed))
                e1.record()
                torch.cuda.synchronize()
                fed[name].append(e0.elapsed_time(e1) / args.steps * 1e3)
        res["fed_step_us"] = {k: stats(v) for k, v in fed.items()}
        res["fed_step_us"]["loss_finite"] = bool(torch.isfinite(step.loss).all())
    else:
        res["fed_step_us"] = "not measured: the captured headline step is %d graphs x %d ROIs" % (wl["graphs"], wl["rois"])

    # ---- the host loop it replaces ---------------------------------------------------------------------
    host = []
    with ThreadPoolExecutor(max_workers=args.threads) as ex:
        list(ex.map(host_heat_topk, host_adj[:args.threads]))
        for _ in range(3):
            t0 = time.perf_counter()
            list(ex.map(host_heat_topk, host_adj))
            host.append((time.perf_counter() - t0) * 1e6)
    res["host_scipy_loop_us"] = dict(stats(host), threads=args.threads)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: res[k] for k in ("launch_us", "heat_products", "fed_step_us", "host_scipy_loop_us")}))


if __name__ == "__main__":
    main()
