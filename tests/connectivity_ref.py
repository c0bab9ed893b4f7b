"""Restatement of the ROI x ROI connectivity maps (TEST INFRASTRUCTURE): per-edge values scattered into dense
[B, R, R] maps, source row and target column — the orientation of the reference's ``data.A`` and of
``coo_matrix(A).row / .col`` — and the GATConv attention of every layer as such maps, on the float64 GATConv stand-in
(tests/golden/gat_standin.py).

Definitions (a batch of B uniform graphs of R nodes; stored edge k = (s, d), graph b = s // R, i = s % R, j = d % R):
  M[b, i, j]    = sum over the stored copies k of edge (i -> j) of graph b of values[k], in stored order; 0 where none
  cnt[b, i, j]  = the number of stored copies
  G[b, l, i, j] = sum over the stored copies with i != j of alpha_l; G[b, l, j, j] = alpha_l of target j's added loop
                  (stored self-loops are removed by PyG: they contribute 0); every target column sums to 1
"""
import numpy as np
import torch

from gat_standin import gat_conv


def _split(edge_index, b, r):
    s, d = edge_index[0].cpu().long(), edge_index[1].cpu().long()
    g = torch.div(s, r, rounding_mode="floor")
    assert bool((g == torch.div(d, r, rounding_mode="floor")).all()), "an edge leaves its graph"
    assert s.numel() == 0 or (int(g.min()) >= 0 and int(g.max()) < b)
    return g.numpy(), (s % r).numpy(), (d % r).numpy()


def dense_map(values, edge_index, b, r, stored_order_fp32=False):
    """M [B, R, R]: float64 sums, or — ``stored_order_fp32`` — float32 sums taken in stored order (np.add.at applies
    repeated indices one after the other, in index order), the bits a kernel that only moves and adds must give."""
    g, i, j = _split(edge_index, b, r)
    dt = np.float32 if stored_order_fp32 else np.float64
    m = np.zeros((b, r, r), dtype=dt)
    np.add.at(m, (g, i, j), values.detach().cpu().reshape(-1).numpy().astype(dt))
    return torch.from_numpy(m)


def count_map(edge_index, b, r):
    """cnt [B, R, R] as float32 (exact: small integers)."""
    g, i, j = _split(edge_index, b, r)
    m = np.zeros((b, r, r), dtype=np.float32)
    np.add.at(m, (g, i, j), np.float32(1))
    return torch.from_numpy(m)


def dense_map_loop(values, edge_index, b, r, dtype=torch.float64):
    """The same map by the definition, one stored edge after the other (the brute force dense_map is held to)."""
    m = torch.zeros(b, r, r, dtype=dtype)
    cnt = torch.zeros(b, r, r, dtype=torch.float32)
    v = values.detach().cpu().reshape(-1).to(dtype)
    for k in range(edge_index.shape[1]):
        s, d = int(edge_index[0, k]), int(edge_index[1, k])
        assert s // r == d // r
        m[s // r, s % r, d % r] = m[s // r, s % r, d % r] + v[k]
        cnt[s // r, s % r, d % r] += 1
    return m, cnt


def odd_batch(seed=0, b=3, r=7):
    """(edge_index [2, E], values [E]) of three graphs of ``r`` nodes: graph 1 has no edges, graph 0 stores edge (2 -> 5)
    three times (not next to each other) and a self-loop, the edge counts are ragged (13, 0, 14)."""
    assert b == 3 and r >= 6
    g = torch.Generator().manual_seed(seed)
    parts = [torch.randint(0, r, (2, ne), generator=g) + k * r for k, ne in enumerate((9, 0, 14))]
    dup, loop = torch.tensor([[2], [5]]), torch.tensor([[4], [4]])
    parts[0] = torch.cat([dup, parts[0][:, :4], dup, loop, parts[0][:, 4:], dup], 1)
    ei = torch.cat(parts, 1)
    return ei, torch.rand(ei.shape[1], generator=g)


def gat_graphs(b, r, h0, seed, deg=3):
    """``b`` graphs of ``r`` nodes as (x [r, h0], edge_index [2, E], edge_attr [E]) in float32: every target but one
    (``lonely``, which nothing reaches) has ``deg`` distinct incoming edges in a shuffled stored order; one edge is stored
    twice (its copy last but one) and one stored self-loop ends the list.  Returns (graphs, lonely nodes)."""
    rng = np.random.default_rng(seed)
    out, lonely = [], []
    for _ in range(b):
        lone = int(rng.integers(r))
        src, dst = [], []
        for j in range(r):
            if j == lone:
                continue
            others = np.array([i for i in range(r) if i != j])
            for i in rng.choice(others, min(deg, r - 1), replace=False):
                src.append(int(i))
                dst.append(j)
        order = rng.permutation(len(src))
        src, dst = np.array(src)[order], np.array(dst)[order]
        loop = int((lone + 1) % r)
        ei = np.stack([np.concatenate([src, src[:1], [loop]]), np.concatenate([dst, dst[:1], [loop]])])
        out.append((torch.from_numpy(rng.standard_normal((r, h0))).float(), torch.from_numpy(ei).long(),
                    torch.from_numpy(rng.random(ei.shape[1])).float()))
        lonely.append(lone)
    return out, lonely


def gat_maps(x, edge_index, ea, layers, b, r):
    """(G [B, L, R, R], [h_1, ..., h_L]) in float64: ``layers`` = per layer (weight, att_src, att_dst, lin_edge,
    att_edge, bias) as gat_standin.gat_conv takes them; h_l = relu(GATConv_l(h_{l-1})), h_0 = x."""
    h = x.detach().cpu().double()
    ei, ea = edge_index.cpu(), ea.detach().cpu().double().reshape(-1)
    maps, outs = [], []
    for par in layers:
        par = [p.detach().cpu().double() for p in par]
        out, alpha, (src, dst) = gat_conv(h, ei, ea, *par, return_alpha=True)
        g = torch.zeros(b, r, r, dtype=torch.float64)
        g.index_put_((torch.div(src, r, rounding_mode="floor"), src % r, dst % r), alpha, accumulate=True)
        maps.append(g)
        h = torch.relu(out)
        outs.append(h)
    return torch.stack(maps, 1), outs


def aggregate(g_l, h_lin, bias):
    """relu(sum_i G_l[b, i, j] h_lin[b, i] + bias): a layer's output rebuilt from its map — h_lin [B, R, F] = x_l W_l^T."""
    return torch.relu(torch.einsum("bij,bif->bjf", g_l.double(), h_lin.double()) + bias.double())


def assert_alpha_close(got, want, what):
    """|got - want| <= 1e-6 + 1e-4 want element-wise (the bound tests/test_gpu_attn_weights.py holds softmax weights to);
    prints the largest fraction of the bound any element uses before it asserts, and returns it."""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(w.shape)}"
    frac = float(((g - w).abs() / (1e-6 + 1e-4 * w.abs())).max())
    print(f"{what}: largest use of the bound 1e-6 + 1e-4 a: {frac:.3e}")
    assert np.isfinite(frac) and frac <= 1.0, f"{what}: {frac:.3e} of the bound"
    return frac
