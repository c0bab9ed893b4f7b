#!/usr/bin/env python3
"""The tiled GDC route (igcn_gdc_diffuse_tiled, csrc/gdc_tiled.hip) at the sizes the LDS-resident kernels refuse, beside
the resident kernels where both fit, and beside the numpy / scipy loop of util_gdc.py's formulas on the host.

    python3 tools/gdc_tiled_bench.py [--out profiles/gdc_tiled_bench.json]

Everything is recorded, nothing is gated.  Call times: device events around ``reps`` eager calls into preallocated outputs
and one preallocated workspace, the routes / kernels of a configuration taking turns in one process, median (min .. max)
of ``--blocks`` blocks.  The fp64 rate of the products: 2 Rp^3 FLOP per product and graph (Rp = R rounded up to 64; a
heat graph counts its own 13 + s products, not the pass-through launches), over the call time less the time of the same
call with no product in it (PPR at alpha = 1: set-up, selection and emission only).  Needs a GPU."""
import argparse
import json
import math
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOP_K, T, ALPHA, DEGREE, TILE = 3, 5.0, 0.05, 14, 64      # csrc/gdc_common.h GDC_HEAT_DEGREE, csrc/gdc_tiled.hip GT_TILE
PPR, HEAT = 0, 1


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "blocks": xs}


def normalised(a):
    a = a.astype(np.float64)
    d = 1 / np.sqrt(a.sum(axis=1))
    return d[:, None] * a * d[None, :]


def host_topk(a, kernel, k=TOP_K):
    """What util_gdc.py does per subject: get_ppr_matrix / get_heat_matrix, get_top_k_matrix, coo_matrix."""
    from scipy.linalg import expm
    from scipy.sparse import coo_matrix
    h, n = normalised(a), a.shape[0]
    s = ALPHA * np.linalg.inv(np.eye(n) - (1 - ALPHA) * h) if kernel == PPR else expm(-T * (np.eye(n) - h))
    s[s.argsort(axis=0)[:n - k], np.arange(n)] = 0.0
    norm = s.sum(axis=0)
    norm[norm <= 0] = 1
    coo = coo_matrix(s / norm)
    return np.vstack([coo.row, coo.col]), coo.data.astype(np.float32)


def squarings(a, t=T):
    nrm, s = t * np.abs(normalised(a)).sum(axis=0).max(), 0
    while nrm > 0.5:
        nrm, s = nrm / 2, s + 1
    return s


def ppr_terms(alpha):
    return 1 if alpha >= 1 else max(1, math.ceil(math.log2(-60 * math.log(2) / math.log(1 - alpha))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gdc_tiled_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gdc_tiled_bench: no GPU")
    import igcn_amd  # noqa: F401
    from igcn_amd import _lib, synth
    from igcn_amd._lib import call, ptr, stream_ptr
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    res = {"device": torch.cuda.get_device_name(0), "top_k": TOP_K, "t": T, "alpha": ALPHA, "configs": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    # (rois, graphs, reps, [(route, kernel)])
    configs = [(512, 32, 60, [("tiled", HEAT), ("tiled", PPR)]),
               (116, 256, 300, [("tiled", HEAT)]),
               (90, 256, 300, [("resident", HEAT), ("tiled", HEAT), ("resident", PPR), ("tiled", PPR)])]
    for r, b, reps, arms in configs:
        graphs = synth.brain_graph_list(b, seed=3000 + r, rois=r, tsne_dim=16)
        host_adj = [g.A.numpy() for g in graphs]
        adj = torch.stack([g.A for g in graphs]).to(dev).contiguous()
        ei = torch.empty(2, b * r * TOP_K, dtype=torch.int64, device=dev)
        ew = torch.empty(b * r * TOP_K, dtype=torch.float32, device=dev)
        counts = torch.empty(b, dtype=torch.int32, device=dev)
        need = max(int(lib.igcn_gdc_tiled_workspace_bytes(b, r, k)) for k in (PPR, HEAT))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rp = (r + TILE - 1) // TILE * TILE
        sq = [squarings(a) for a in host_adj]
        products = {HEAT: sum(DEGREE - 1 + s for s in sq), PPR: b * 2 * (ppr_terms(ALPHA) - 1)}

        def tiled(kernel, param):
            return lambda: call("igcn_gdc_diffuse_tiled", b, r, kernel, param, 0, TOP_K, 0.0, ptr(adj), b, None, ptr(ei),
                                ptr(ew), ptr(counts), ptr(ws), need, stream_ptr())

        def resident(kernel, param):
            return lambda: call("igcn_gdc_diffuse", b, r, kernel, param, 0, TOP_K, 0.0, ptr(adj), b, None, ptr(ei),
                                ptr(ew), ptr(counts), stream_ptr())
        name = {PPR: "ppr", HEAT: "heat"}
        launch = {f"{route}_{name[k]}": (tiled if route == "tiled" else resident)(k, ALPHA if k == PPR else T)
                  for route, k in arms}
        launch["tiled_no_product"] = tiled(PPR, 1.0)
        for fn in launch.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in launch}
        for _ in range(args.blocks):
            for key, fn in launch.items():
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / reps * 1e3)
        cfg = {"rois": r, "padded_rois": rp, "graphs": b, "reps": reps, "workspace_bytes": need,
               "squarings_per_graph": {"min": min(sq), "max": max(sq)},
               "squaring_launches": max(0, math.ceil(math.log2(2 * T * math.sqrt(r)))), "ppr_terms": ppr_terms(ALPHA),
               "call_us": {k: stats(v) for k, v in times.items()}}
        base = cfg["call_us"]["tiled_no_product"]["median"]
        cfg["products"] = {}
        for route, k in arms:
            if route != "tiled":
                continue
            us = cfg["call_us"][f"tiled_{name[k]}"]["median"]
            flop = products[k] * 2 * rp ** 3
            cfg["products"][name[k]] = {"products_in_batch": products[k], "flop_per_batch": flop,
                                        "tflops_over_call_time": flop / (us * 1e-6) / 1e12,
                                        "tflops_over_product_time": flop / ((us - base) * 1e-6) / 1e12}
        # ---- the host loop it replaces, over the same matrices -------------------------------------------------
        cfg["host_loop_us"] = {}
        with ThreadPoolExecutor(max_workers=args.threads) as ex:
            for k in sorted({k for _, k in arms}):
                host = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    list(ex.map(lambda a: host_topk(a, k), host_adj))
                    host.append((time.perf_counter() - t0) * 1e6)
                cfg["host_loop_us"][name[k]] = dict(stats(host), threads=args.threads)
        res["configs"].append(cfg)
        print(json.dumps({"rois": r, "graphs": b, "call_us": {k: v["median"] for k, v in cfg["call_us"].items()},
                          "products": cfg["products"],
                          "host_loop_us": {k: v["median"] for k, v in cfg["host_loop_us"].items()}}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
