#!/usr/bin/env python3
"""The network-based statistic (igcn_amd.stats.network_based_statistic; k_perm_supra in csrc/perm_test.hip,
k_nbs_components in csrc/nbs.hip) at cohort size: S = 874 subjects (437 / 437), R = 90 regions (E = 8 100 entries),
P = 10 000 relabellings, primary threshold 3.1.

    python3 tools/nbs_bench.py [--out profiles/nbs_bench.json] [--calls 5] [--threads 16]

Everything is recorded, nothing is gated.  Wall clock of whole ``network_based_statistic`` calls (relabellings drawn
outside the call, one warm-up call, median (min .. max) of ``--calls``); the device time of the igcn_perm_supra launches
alone and of the igcn_nbs_components launches alone (over all chunks, device events).  Beside them, in the same process:
  * ``stats.permutation_test`` at the same E = 8 100 and its igcn_perm_maxsum launches alone: the yardstick for the bits
    epilogue is the max epilogue on the same tile and main loop;
  * the host route: the numpy fp64 product and a ``scipy.sparse.csgraph.connected_components`` call per relabelling on
    ``--threads`` host threads, for one 512-row chunk, scaled to P (left out where scipy does not import).
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
S, N_A, R, P, T0, CHUNK_REF = 874, 437, 90, 10000, 3.1, 512


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "all": xs}


def timed(e0, e1, fn, calls):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return spread(out)


def wall(fn, calls):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def host_route(z, member, thr, tested, calls):
    """ms, scaled to P: G = member z in fp64, |G| >= thr on the tested entries, the weakly connected components and the
    largest extent of every relabelling of one chunk."""
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None

    def run():
        g = member @ z
        sup = ((np.abs(g) >= thr) & tested[None, :]).reshape(-1, R, R)
        out = np.zeros(len(sup), dtype=np.int64)
        for i, a in enumerate(sup):
            _, lab = connected_components(csr_matrix(a), directed=True, connection="weak")
            out[i] = np.bincount(lab, weights=a.sum(1), minlength=1).max()
        return out

    run()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        run()
        times.append((time.perf_counter() - t0) * 1e3 * P / len(member))
    return spread(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbs_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nbs_bench: no GPU")
    torch.set_num_threads(args.threads)
    import igcn_amd  # noqa: F401
    from igcn_amd import _lib, ops, stats
    _lib.load()
    dev = torch.device("cuda", 0)
    e = R * R
    y = (torch.arange(S, device=dev) >= N_A).long()
    gen = torch.Generator(device=dev)
    gen.manual_seed(e)
    x = torch.randn(S, R, R, generator=gen, device=dev) * 1.5 + 2.0
    hub = torch.arange(1, 13, device=dev)
    x[:N_A, 0, hub] += 0.45                                      # a planted star of 12 moderately shifted connections
    members = stats.draw_members(S, N_A, P, seed=0, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    chunks = range(0, P, stats.DEFAULT_CHUNK)

    out = stats.network_based_statistic(x, y, threshold=T0, members=members)
    whole = wall(lambda: stats.network_based_statistic(x, y, threshold=T0, members=members), args.calls)
    maxt = wall(lambda: stats.permutation_test(x, y, members=members), args.calls)
    fwe = stats.permutation_test(x, y, members=members)["p_fwe"]

    _, _, _, planes = ops.perm_prepare(x.reshape(S, e), torch.arange(S, device=dev))
    thr, flags = out["threshold"][1], out["tested"].reshape(-1)
    g_obs = ops.perm_maxsum(members[:1], planes, e)[1].view(-1).contiguous()
    supra = timed(e0, e1, lambda: [ops.perm_supra(members[p0:p0 + stats.DEFAULT_CHUNK], planes, e, thr, 0, flags)
                                   for p0 in chunks], args.calls)
    maxsum = timed(e0, e1, lambda: [ops.perm_maxsum(members[p0:p0 + stats.DEFAULT_CHUNK], planes, e, g_obs)
                                    for p0 in chunks], args.calls)
    bits = [ops.perm_supra(members[p0:p0 + stats.DEFAULT_CHUNK], planes, e, thr, 0, flags) for p0 in chunks]
    comps = timed(e0, e1, lambda: [ops.nbs_components(b, R) for b in bits], args.calls)

    z = ops.perm_planes_to_z(planes, S, e).double().cpu().numpy()
    host = host_route(z, members[:CHUNK_REF].double().cpu().numpy(), float(thr), flags.cpu().numpy(), args.calls)

    flop = 2.0 * P * S * e
    keep = out["extent"] > 0
    res = {"device": torch.cuda.get_device_name(0), "subjects": S, "groups": [N_A, S - N_A], "regions": R, "entries": e,
           "permutations": P, "threshold_t": T0, "threshold_g": thr, "chunk": stats.DEFAULT_CHUNK,
           "reference_chunk": CHUNK_REF, "host_threads": args.threads,
           "observed_suprathreshold_entries": int(out["supra"].sum()),
           "observed_largest_extent": int(out["extent"].max()),
           "components_at_0.05": int(torch.unique(out["component"][keep & (out["p_fwe"] <= 0.05)]).numel()),
           "null_max_extent": {"median": int(out["null_max"].median()), "max": int(out["null_max"].max())},
           "entries_significant_by_max_t_at_0.05": int((fwe <= 0.05).sum()),
           "network_based_statistic_wall_ms": whole, "permutation_test_wall_ms": maxt,
           "perm_supra_launches_ms": supra, "perm_maxsum_launches_ms": maxsum,
           "supra_over_maxsum": supra["median"] / maxsum["median"], "nbs_components_launches_ms": comps,
           "tflops_single_product_supra": flop / (supra["median"] * 1e-3) / 1e12,
           "host_numpy_scipy_ms_scaled": host}
    print(json.dumps({k: (v["median"] if isinstance(v, dict) and "all" in v else v) for k, v in res.items()}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
