#!/usr/bin/env python3
"""Cost of the ROI x ROI connectivity passes — ``model.edge_importance`` (cal_probability's edge mask as dense maps,
kernel/sgcn_img_snp.py:133-151) and ``model.gat_attention`` (the per-edge GATConv attention of every layer as dense maps,
kernel/sgcn.py:235-267) — beside one evaluation forward of the same model on the same batch, in the same process.

Workload: ``SGCN_GAT(2 layers, 16 hidden)``, 256 subjects, 90 ROIs, top-3 diffusion graphs (270 stored edges per
subject).  Every call runs eagerly: per block, device events around ``--steps`` hot calls, wall clock around the same
calls including the final synchronisation; the calls take turns block by block after a warm-up; median and spread of
``--blocks`` blocks.  Beside them the two new launches on their own, timed the same way (ops.edge_dense_map with counts
on a mask computed beforehand, ops.gat_stack_alpha).  Nothing here is a pass / fail threshold.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run under a time limit, e.g.
    timeout -k 10 300 python tools/connectivity_bench.py --out profiles/connectivity_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS, ROIS, LAYERS, HIDDEN = 256, 90, 2, 16


def _spread(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "blocks": [round(x, digits) for x in v]}


def _block_ms(fn, steps):
    """(device ms, wall ms) per call over ``steps`` hot calls."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks: at least five timed blocks")
    sys.path.insert(0, ROOT)
    import torch
    import igcn_amd  # noqa: F401  (import shim: the package directory is ``ig-gcn_amd/``)
    from igcn_amd import _lib, ops, synth
    from igcn_amd.gcn_img_snp import gat_padded_params
    from igcn_amd.sgcn import SGCN_GAT
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("connectivity_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = SGCN_GAT(SimpleNamespace(num_features=3, num_classes=2), LAYERS, HIDDEN, rois=ROIS, H_0=3).to(dev)
    model.eval()
    data = synth.brain_batch(GRAPHS, seed=1000, rois=ROIS).to(dev)
    plan = ops.plan_for(data)
    params = gat_padded_params([model.conv1, *model.convs])[2]

    def forward():
        with torch.no_grad():
            model(data)

    with torch.no_grad():
        e = model.cal_probability(data.x, data.edge_index, data.edge_attr, plan=plan)[3].reshape(-1).contiguous()
    calls = {"edge_importance": lambda: model.edge_importance(data, return_count=True),
             "gat_attention": lambda: model.gat_attention(data),
             "eval_forward": forward,
             "edge_dense_map_launch": lambda: ops.edge_dense_map(e, plan, ROIS, want_count=True),
             "gat_stack_alpha_launch": lambda: ops.gat_stack_alpha(data.x, data.edge_attr, plan, ROIS, *params)}
    for fn in calls.values():                                  # warm-up: plans, allocator, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dev_ms, wall_ms = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(args.blocks):                               # the calls take turns, block by block
        for k, fn in calls.items():
            d, wl = _block_ms(fn, args.steps)
            dev_ms[k].append(d)
            wall_ms[k].append(wl)
    m, cnt = model.edge_importance(data, return_count=True)
    g = model.gat_attention(data)
    emax = plan._stack_dims[1]
    res = {"workload": dict(model=f"SGCN_GAT({LAYERS}, {HIDDEN})", graphs=GRAPHS, rois=ROIS, edges=int(plan.n_edges),
                            max_edges_per_graph=int(emax)),
           "edge_dense_map_tile_columns": int(lib.igcn_edge_dense_map_supported(ROIS, 1)),
           "gat_stack_alpha_tile_columns": int(lib.igcn_gat_stack_alpha_tile(ROIS, emax, 3, HIDDEN, LAYERS)),
           "gat_stack_alpha_lds_bytes": int(lib.igcn_gat_stack_lds_bytes(ROIS, emax, 3, HIDDEN, LAYERS, 0)) +
           ROIS * 4 * int(lib.igcn_gat_stack_alpha_tile(ROIS, emax, 3, HIDDEN, LAYERS)),
           "device_ms_per_call": {k: _spread(v) for k, v in dev_ms.items()},
           "wall_ms_per_call": {k: _spread(v) for k, v in wall_ms.items()},
           "map_shape": list(m.shape), "stored_edges_in_cnt": float(cnt.sum()), "gat_shape": list(g.shape),
           "gat_max_column_sum_error": float((g.double().sum(2) - 1).abs().max()),
           "device": torch.cuda.get_device_name(0),
           "timing": (f"eager calls; device events and wall clock (with the closing synchronisation) around {args.steps} hot "
                      f"calls per block, 3 warm-up calls, median / min / max of {args.blocks} blocks, the calls alternating")}
    med = {k: res["device_ms_per_call"][k]["median"] for k in calls}
    res["edge_importance_over_eval_forward"] = round(med["edge_importance"] / med["eval_forward"], 3)
    res["gat_attention_over_eval_forward"] = round(med["gat_attention"] / med["eval_forward"], 3)
    for k in calls:
        d, wl = res["device_ms_per_call"][k], res["wall_ms_per_call"][k]
        print(f"{k}: {d['median']:.3f} ms on the device ({d['min']:.3f} .. {d['max']:.3f}), {wl['median']:.3f} ms wall; "
              f"median of {args.blocks} blocks of {args.steps} hot calls", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
