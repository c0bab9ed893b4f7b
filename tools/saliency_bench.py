#!/usr/bin/env python3
"""Cost of the ROI x modality saliency passes — ``model.input_saliency`` (gradient x input), ``model.integrated_gradients``
(midpoint rule, 16 steps) and ``SGCN_Ori.grad_cam`` — beside one evaluation forward and one eval forward + full backward
(parameter gradients included) of the same model on the same batch, in the same process.

Workload: bench.py's headline — ``SGCN_GCN_IMGSNP(2, 16)``, 256 subjects, 90 ROIs, the 3000-node GO DAG — and, for
Grad-CAM, ``SGCN_Ori(3, 32, 32, 5)`` on the same graphs.  Every call runs eagerly: per block, device events around
``--steps`` hot calls, wall clock around the same calls including the final synchronisation; the calls take turns block
by block after a warm-up; median and spread of ``--blocks`` blocks.  Beside them the two new launches on their own
(igcn_saliency_maps with M = 1 and M = 16, igcn_grad_cam).  Nothing here is a pass / fail threshold.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run under a time limit, e.g.
    timeout -k 10 300 python tools/saliency_bench.py --out profiles/saliency_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IG_STEPS = 16


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


def _measure(calls, blocks, steps):
    import torch
    for fn in calls.values():                                  # warm-up: plans, allocator, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dev_ms, wall_ms = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(blocks):                                    # the calls take turns, block by block
        for k, fn in calls.items():
            d, wl = _block_ms(fn, steps)
            dev_ms[k].append(d)
            wall_ms[k].append(wl)
    return {k: _spread(v) for k, v in dev_ms.items()}, {k: _spread(v) for k, v in wall_ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks: at least five timed blocks")
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from igcn_amd import _lib, ops, synth
    from igcn_amd.sgcn import SGCN_Ori
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("saliency_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    model, _ = bench.build_model(dev)
    model.eval()
    graphs, rois = bench.GRAPHS_PER_GPU, bench.ROIS
    data = synth.brain_batch(graphs, seed=1000, rois=rois).to(dev)
    torch.manual_seed(0)
    ori = SGCN_Ori(3, 32, 32, 5, rois=rois).to(dev).eval()

    def forward(m, *a):
        def run():
            with torch.no_grad():
                m(data, *a)
        return run

    def forward_backward(m, *a):
        def run():
            out = m(data, *a)
            logp = out[0] if isinstance(out, (tuple, list)) else out
            m.zero_grad(set_to_none=True)
            data.x.grad = None
            logp[:, 0].sum().backward()
        return run

    x = data.x.detach()
    dx = torch.randn(IG_STEPS, *x.shape, device=dev)
    acts, grads = torch.randn(graphs * rois, 5, device=dev), torch.randn(graphs * rois, 5, device=dev)
    calls = {"input_saliency": lambda: model.input_saliency(data, None, dev),
             "input_saliency_both": lambda: model.input_saliency(data, None, dev, inputs="both"),
             "integrated_gradients_16": lambda: model.integrated_gradients(data, None, dev, steps=IG_STEPS),
             "eval_forward": forward(model, None, dev),
             "eval_forward_backward": forward_backward(model, None, dev),
             "saliency_maps_launch_m1": lambda: ops.saliency_maps(x, dx[0], rois),
             "saliency_maps_launch_m16": lambda: ops.saliency_maps(x, dx, rois),
             "ori_grad_cam": lambda: ori.grad_cam(data),
             "ori_input_saliency": lambda: ori.input_saliency(data),
             "ori_eval_forward": forward(ori),
             "ori_eval_forward_backward": forward_backward(ori),
             "grad_cam_launch": lambda: ops.grad_cam(acts, grads, rois)}
    dev_ms, wall_ms = _measure(calls, args.blocks, args.steps)
    r = model.integrated_gradients(data, None, dev, steps=IG_STEPS)
    res = {"workload": dict(model="SGCN_GCN_IMGSNP(2, 16)", ori="SGCN_Ori(3, 32, 32, 5)", graphs=graphs, rois=rois,
                            go_nodes=int(model.go_network.n_nodes), ig_steps=IG_STEPS, pool=list(bench.POOL)),
           "device_ms_per_call": dev_ms, "wall_ms_per_call": wall_ms,
           "ig_mean_abs_delta": float(r["delta"].abs().mean()),
           "ig_mean_abs_attr_sum": float(r["attr"].abs().sum((1, 2)).mean()),
           "device": torch.cuda.get_device_name(0),
           "timing": (f"eager calls; device events and wall clock (with the closing synchronisation) around {args.steps} hot "
                      f"calls per block, 3 warm-up calls, median / min / max of {args.blocks} blocks, the calls alternating")}
    med = {k: dev_ms[k]["median"] for k in calls}
    res["input_saliency_over_eval_forward_backward"] = round(med["input_saliency"] / med["eval_forward_backward"], 3)
    res["integrated_gradients_16_over_input_saliency"] = round(med["integrated_gradients_16"] / med["input_saliency"], 3)
    res["ori_grad_cam_over_eval_forward_backward"] = round(med["ori_grad_cam"] / med["ori_eval_forward_backward"], 3)
    for k in calls:
        d, wl = dev_ms[k], wall_ms[k]
        print(f"{k}: {d['median']:.3f} ms on the device ({d['min']:.3f} .. {d['max']:.3f}), {wl['median']:.3f} ms wall; "
              f"median of {args.blocks} blocks of {args.steps} hot calls", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
