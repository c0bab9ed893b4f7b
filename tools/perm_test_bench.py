#!/usr/bin/env python3
"""The max-T permutation test (igcn_amd.stats.permutation_test; csrc/perm_test.hip) at cohort size: S = 874 subjects in
two groups of 437, P = 10 000 relabellings, E = 270 / 4 860 / 36 000 map entries.

    python3 tools/perm_test_bench.py [--out profiles/perm_test_bench.json] [--calls 5]

Everything is recorded, nothing is gated.  Per shape: the wall clock of whole ``permutation_test`` calls (relabellings
drawn outside the call, one warm-up call, median (min .. max) of ``--calls``), the device time of the product launches
alone (igcn_perm_maxsum over all chunks, device events) and the product's rate counted as ONE bf16 product
2 P S E FLOP and as the three plane products the matrix unit executes (x 3).  Beside them, in the same process:
  * the library's exact-fp32 GEMM (ops.gemm_nn) materialising G for one 512-row chunk with a tensor-library epilogue
    (abs, row maximum, comparison with |g_obs|, column count), scaled to P — the only device route to this product
    without the new kernels;
  * the numpy fp64 restatement (member @ z, abs, max, compare, count) for one 512-row chunk on ``--threads`` host
    threads, scaled to P.
Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, N_A, P, CHUNK_REF = 874, 437, 10000, 512
ENTRIES = (270, 4860, 36000)


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "all": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perm_test_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perm_test_bench: no GPU")
    torch.set_num_threads(args.threads)
    import igcn_amd  # noqa: F401
    from igcn_amd import _lib, ops, stats
    _lib.load()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "subjects": S, "group_a": N_A, "permutations": P,
           "chunk": stats.DEFAULT_CHUNK, "reference_chunk": CHUNK_REF, "host_threads": args.threads, "shapes": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    y = torch.zeros(S, dtype=torch.int64, device=dev)
    y[N_A:] = 1
    members = stats.draw_members(S, N_A, P, seed=0, device=dev)
    for e in ENTRIES:
        gen = torch.Generator(device=dev)
        gen.manual_seed(e)
        x = torch.randn(S, e, generator=gen, device=dev) * 1.5 + 2.0
        x[:N_A, ::7] += 0.3
        out = stats.permutation_test(x, y, members=members)                     # warm-up
        torch.cuda.synchronize()
        wall = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            out = stats.permutation_test(x, y, members=members)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        # the product launches alone
        rows = torch.arange(S, device=dev)
        t0 = time.perf_counter()
        _, _, _, planes = ops.perm_prepare(x, rows)
        torch.cuda.synchronize()
        prepare_ms = (time.perf_counter() - t0) * 1e3
        _, g = ops.perm_maxsum(members[:1], planes, e)
        g_obs = g.view(-1).contiguous()
        prod = []
        for _ in range(args.calls):
            e0.record()
            for p0 in range(0, P, stats.DEFAULT_CHUNK):
                ops.perm_maxsum(members[p0:p0 + stats.DEFAULT_CHUNK], planes, e, g_obs)
            e1.record()
            torch.cuda.synchronize()
            prod.append(e0.elapsed_time(e1))
        flop = 2.0 * P * S * e
        # the exact-fp32 GEMM route: G for one chunk, then the epilogue in the tensor library
        z = ops.perm_planes_to_z(planes, S, e)
        m32 = members[:CHUNK_REF].float().contiguous()
        thr = g_obs.abs()

        def gemm_route():
            gg = ops.gemm_nn(m32, z).abs()
            return gg.max(1).values, (gg >= thr[None, :]).sum(0)
        gemm_route()
        torch.cuda.synchronize()
        gemm = []
        for _ in range(args.calls):
            e0.record()
            gemm_route()
            e1.record()
            torch.cuda.synchronize()
            gemm.append(e0.elapsed_time(e1) * P / CHUNK_REF)
        # the numpy fp64 restatement for one chunk
        z64 = z.double().cpu().numpy()
        m64 = members[:CHUNK_REF].cpu().numpy().astype(np.float64)
        thr64 = np.abs(g_obs.double().cpu().numpy())
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            gg = np.abs(m64 @ z64)
            gg.max(1), (gg >= thr64[None, :]).sum(0)
            host.append((time.perf_counter() - t0) * 1e3 * P / CHUNK_REF)
        row = {"entries": e, "significant_at_0.05": int((out["p_fwe"] <= 0.05).sum()),
               "permutation_test_wall_ms": spread(wall), "prepare_wall_ms": prepare_ms,
               "product_launches_ms": spread(prod), "product_flop_single_bf16": flop,
               "tflops_single_product": flop / (spread(prod)["median"] * 1e-3) / 1e12,
               "tflops_three_planes": 3 * flop / (spread(prod)["median"] * 1e-3) / 1e12,
               "fp32_gemm_route_ms_scaled": spread(gemm), "numpy_fp64_ms_scaled": spread(host)}
        res["shapes"].append(row)
        print(json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
        del x, planes, z, out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
