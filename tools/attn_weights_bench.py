#!/usr/bin/env python3
"""Cost of the attention-weights launch (igcn_attn_weights: the head-averaged softmax nn.MultiheadAttention returns next
to its output, kernel/sgcn_img_snp.py:240) beside the forward attention core at the same shape in the same process.

Shapes: B = 256 samples, H = 2, Lq = 90 queries, Lk = 400 keys at D = 32 (the default model width) and D = 128 (a wide
row: head_dim 64).  Per shape: us per call of ops.attention_weights and of ops.AttentionCore's forward — hot replays of
a captured graph of ``ITERS`` calls, device events around a block of replays, the two launches taking turns block by
block after a warm-up; median and spread of ``--blocks`` blocks — and the store rate of the weights launch: the
B * Lq * Lk * 4 bytes it must write over its median time, as a fraction of the write bandwidth of the part (8.0 TB/s HBM3E
peak by specification; 6.1 TB/s measured for plain streaming stores).  The store is the floor of the launch: it reads
(Lq + Lk) * D floats per sample and writes Lq * Lk.  Nothing here is a pass / fail threshold.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run under a time limit, e.g.
    timeout -k 10 300 python tools/attn_weights_bench.py --out profiles/attn_weights_bench.json
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ITERS, REPLAYS = 10, 5                                # calls per captured graph, replays per timed block
SHAPES = ((32, 2, 90, 400), (128, 2, 90, 400))        # (D, H, Lq, Lk)
BATCH = 256
WRITE_TBS = {"hbm3e_peak_spec": 8.0, "plain_stores_measured": 6.1}


def _spread(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "blocks": [round(x, digits) for x in v]}


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


def store_fractions(b, lq, lk, us):
    """(bytes the launch must store, TB/s at ``us`` per call, that rate over each write bandwidth of WRITE_TBS)."""
    nbytes = b * lq * lk * 4
    tbs = nbytes / (us * 1e-6) / 1e12
    return nbytes, tbs, {k: tbs / v for k, v in WRITE_TBS.items()}


def shape_us(dev, d, h, lq, lk, blocks, warmup=3):
    import torch
    from igcn_amd import _lib, ops
    lib = _lib.load()
    if not lib.igcn_attn_weights_supported(d, h, lq, lk):
        raise _lib.IgcnError(f"igcn_attn_weights does not cover D={d} H={h} Lq={lq} Lk={lk}")
    gen = torch.Generator(device=dev).manual_seed(d)
    q = torch.randn(BATCH, lq, d, device=dev, generator=gen)
    kv = torch.randn(BATCH, lk, 2 * d, device=dev, generator=gen)

    def many(f):
        def run():
            with torch.no_grad():
                for _ in range(ITERS):
                    f()
        return run
    graphs = {"weights": _graph_of(many(lambda: ops.attention_weights(q, kv, h))),
              "forward_core": _graph_of(many(lambda: ops.AttentionCore.apply(q, kv, h)))}
    for g in graphs.values():
        for _ in range(warmup):
            g.replay()
    torch.cuda.synchronize()
    us = {k: [] for k in graphs}
    for _ in range(blocks):                              # the two launches take turns, block by block
        for k, g in graphs.items():
            us[k].append(_replay_us(g))
    w = ops.attention_weights(q, kv, h)
    row = {"shape": dict(B=BATCH, D=d, H=h, head_dim=d // h, Lq=lq, Lk=lk),
           "chunk_rows": int(lib.igcn_attn_weights_chunk_rows(d, h, lq, lk)),
           "max_abs_row_sum_minus_1": float((w.sum(-1) - 1).abs().max())}
    row.update({k + "_us": _spread(v) for k, v in us.items()})
    nbytes, tbs, frac = store_fractions(BATCH, lq, lk, row["weights_us"]["median"])
    row["store_bytes"], row["store_TBps"] = nbytes, round(tbs, 3)
    row["store_fraction_of"] = {k: round(v, 3) for k, v in frac.items()}
    row["weights_over_forward_core"] = round(row["weights_us"]["median"] / row["forward_core_us"]["median"], 3)
    print(f"D={d}: weights {row['weights_us']['median']:.2f} us ({row['weights_us']['min']:.2f} .. "
          f"{row['weights_us']['max']:.2f}), forward core {row['forward_core_us']['median']:.2f} us "
          f"({row['forward_core_us']['min']:.2f} .. {row['forward_core_us']['max']:.2f}); stores {nbytes / 1e6:.1f} MB at "
          f"{tbs:.2f} TB/s = {frac['hbm3e_peak_spec']:.2f} of 8.0 TB/s; median of {blocks} blocks of {ITERS * REPLAYS} hot "
          f"calls", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--blocks", type=int, default=7)
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks: at least five timed blocks")
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    from igcn_amd import _lib
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("attn_weights_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    res = {"shapes": {f"D{d}": shape_us(dev, d, h, lq, lk, args.blocks) for d, h, lq, lk in SHAPES}}
    res["device"] = torch.cuda.get_device_name(0)
    res["write_bandwidth_TBps"] = WRITE_TBS
    res["timing"] = (f"device events around {REPLAYS} hot replays of a captured graph of {ITERS} calls per block, 3 warm-up "
                     f"replays, median / min / max of {args.blocks} blocks, the two launches alternating; the same inputs every "
                     "call, so the 36.9 MB output of a call can stay in the 256 MB Infinity Cache: the store rate is what "
                     "the launch achieves on this footprint, not an HBM-only figure")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
