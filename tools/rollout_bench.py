#!/usr/bin/env python3
"""Cost of the ROI x SNP association pass (``model.snp_association``: the cross-attention weights times the attention
roll-out of the GO encoder, go_model.py:208-251) beside ``model.attention_weights`` and one evaluation forward of the
same model on the same batch, in the same process.

Workload: bench.py's headline — ``SGCN_GCN_IMGSNP(2, 16)``, 256 subjects, 90 ROIs, the 3000-node GO DAG (400 top-level
terms, 54 SNPs).  Every call runs eagerly (the analysis pass is not captured into a graph): per block, device events
around ``--steps`` hot calls, wall clock around the same calls including the final synchronisation; the three calls take
turns block by block after a warm-up; median and spread of ``--blocks`` blocks.  Beside them the pieces of the pass on
their own, timed the same way: ``Gene_ontology_network.attention_rollout`` (both layers' coefficients and mixing and the
encoder layer between them) and the final batched product.  Nothing here is a pass / fail threshold.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run under a time limit, e.g.
    timeout -k 10 300 python tools/rollout_bench.py --out profiles/rollout_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    import bench
    from igcn_amd import _lib, ops, synth
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    model, _ = bench.build_model(dev)
    model.eval()
    graphs = bench.GRAPHS_PER_GPU
    data = synth.brain_batch(graphs, seed=1000, rois=bench.ROIS).to(dev)
    net = model.go_network
    snps = data.snps_feat.view(-1, 54).float().contiguous()

    def forward():
        with torch.no_grad():
            model(data, None, dev)

    w = model.attention_weights(data, None, dev)
    r_top = net.attention_rollout(snps)
    calls = {"snp_association": lambda: model.snp_association(data, None, dev),
             "attention_weights": lambda: model.attention_weights(data, None, dev),
             "eval_forward": forward,
             "attention_rollout": lambda: net.attention_rollout(snps),
             "final_product": lambda: ops.snp_association(w, r_top)}
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
    assoc = model.snp_association(data, None, dev)
    res = {"workload": dict(model="SGCN_GCN_IMGSNP(2, 16)", graphs=graphs, rois=bench.ROIS, go_nodes=int(net.n_nodes),
                            top_terms=int(net.n_top), snps=54, pool=list(bench.POOL)),
           "rollout_chunk_columns": {f"N{c.n_rows}": int(lib.igcn_go_rollout_chunk(c.n_rows)) for c in net.enc_csr},
           "device_ms_per_call": {k: _spread(v) for k, v in dev_ms.items()},
           "wall_ms_per_call": {k: _spread(v) for k, v in wall_ms.items()},
           "assoc_shape": list(assoc.shape), "max_row_sum": float(assoc.sum(-1).max()),
           "min_entry": float(assoc.min()), "device": torch.cuda.get_device_name(0),
           "timing": (f"eager calls; device events and wall clock (with the closing synchronisation) around {args.steps} hot "
                      f"calls per block, 3 warm-up calls, median / min / max of {args.blocks} blocks, the calls alternating")}
    med = {k: res["device_ms_per_call"][k]["median"] for k in calls}
    res["snp_association_over_attention_weights"] = round(med["snp_association"] / med["attention_weights"], 3)
    res["snp_association_over_eval_forward"] = round(med["snp_association"] / med["eval_forward"], 3)
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
