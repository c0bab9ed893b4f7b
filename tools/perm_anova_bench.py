#!/usr/bin/env python3
"""The max-F permutation test (igcn_amd.stats.permutation_anova; k_perm_maxf in csrc/perm_test.hip) at cohort size:
S = 874 subjects in three groups of 292 / 291 / 291 (and one run in five groups), P = 10 000 relabellings,
E = 270 / 4 860 / 36 000 map entries.

    python3 tools/perm_anova_bench.py [--out profiles/perm_anova_bench.json] [--calls 5]

Everything is recorded, nothing is gated.  Per shape: the wall clock of whole ``permutation_anova`` calls (label rows
drawn outside the call, one warm-up call, median (min .. max) of ``--calls``) and the device time of the product launches
alone (igcn_perm_maxf over all chunks, device events), with the rate counted as the K - 1 bf16 products 2 P S E FLOP and
as the three plane products of each that the matrix unit executes (x 3).  Beside them, in the same process:
  * the two-group launches (igcn_perm_maxsum over all chunks) at the same shape: the K - 1 label sets share every load of
    a plane fragment, so K = 3 is expected to cost less than twice this;
  * the library's exact-fp32 GEMM (ops.gemm_nn) materialising the K - 1 G matrices for one 512-row chunk with a
    tensor-library epilogue (squares, weighted sum, row maximum, comparison with b_obs, column count), scaled to P.
Needs a GPU."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, P, CHUNK_REF = 874, 10000, 512
RUNS = (((292, 291, 291), (270, 4860, 36000)), ((175, 175, 175, 175, 174), (4860,)))


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "all": xs}


def timed(e0, e1, fn, calls, scale=1.0):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * scale)
    return spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perm_anova_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perm_anova_bench: no GPU")
    import igcn_amd  # noqa: F401
    from igcn_amd import _lib, ops, stats
    _lib.load()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "subjects": S, "permutations": P, "chunk": stats.DEFAULT_CHUNK,
           "reference_chunk": CHUNK_REF, "shapes": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    chunks = range(0, P, stats.DEFAULT_CHUNK)
    for sizes, entries in RUNS:
        k = len(sizes)
        y = torch.repeat_interleave(torch.arange(k, device=dev), torch.tensor(sizes, device=dev))
        labels = stats.draw_labels(y, P, seed=0, device=dev)
        members = stats.draw_members(S, sizes[0], P, seed=0, device=dev)
        weights = [1.0 / n for n in sizes]
        for e in entries:
            gen = torch.Generator(device=dev)
            gen.manual_seed(e)
            x = torch.randn(S, e, generator=gen, device=dev) * 1.5 + 2.0
            x[:sizes[0], ::7] += 0.3
            x[-sizes[-1]:, ::7] -= 0.15
            groups = tuple(range(k))
            out = stats.permutation_anova(x, y, groups=groups, labels=labels)               # warm-up
            torch.cuda.synchronize()
            wall = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                out = stats.permutation_anova(x, y, groups=groups, labels=labels)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            # the product launches alone, K groups and two groups
            _, _, _, planes = ops.perm_prepare(x, torch.arange(S, device=dev))
            _, b, g = ops.perm_maxf(labels[:1], planes, e, weights, want_g=True)
            b_obs = b.view(-1).contiguous()
            g_obs = ops.perm_maxsum(members[:1], planes, e)[1].view(-1).contiguous()
            prod = timed(e0, e1, lambda: [ops.perm_maxf(labels[p0:p0 + stats.DEFAULT_CHUNK], planes, e, weights, b_obs)
                                          for p0 in chunks], args.calls)
            two = timed(e0, e1, lambda: [ops.perm_maxsum(members[p0:p0 + stats.DEFAULT_CHUNK], planes, e, g_obs)
                                         for p0 in chunks], args.calls)
            # the exact-fp32 GEMM route: the K - 1 G matrices for one chunk, then the epilogue in the tensor library
            z = ops.perm_planes_to_z(planes, S, e)
            ind = [(labels[:CHUNK_REF] == c).float().contiguous() for c in range(k - 1)]

            def gemm_route():
                gs = [ops.gemm_nn(m, z) for m in ind]
                tot = gs[0].clone()
                bb = weights[0] * gs[0] * gs[0]
                for c in range(1, k - 1):
                    bb += weights[c] * gs[c] * gs[c]
                    tot += gs[c]
                bb += weights[k - 1] * tot * tot
                return bb.max(1).values, (bb >= b_obs[None, :]).sum(0)
            gemm = timed(e0, e1, gemm_route, args.calls, scale=P / CHUNK_REF)
            flop = 2.0 * P * S * e * (k - 1)
            row = {"groups": list(sizes), "entries": e, "significant_at_0.05": int((out["p_fwe"] <= 0.05).sum()),
                   "permutation_anova_wall_ms": spread(wall), "product_launches_ms": prod,
                   "two_group_launches_ms": two, "ratio_to_two_group": prod["median"] / two["median"],
                   "product_flop_single_bf16": flop, "tflops_single_product": flop / (prod["median"] * 1e-3) / 1e12,
                   "tflops_three_planes": 3 * flop / (prod["median"] * 1e-3) / 1e12, "fp32_gemm_route_ms_scaled": gemm}
            res["shapes"].append(row)
            print(json.dumps({k_: (v["median"] if isinstance(v, dict) else v) for k_, v in row.items()}), flush=True)
            del x, planes, z, out, ind
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
