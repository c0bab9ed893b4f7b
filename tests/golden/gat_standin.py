"""Restatement of PyG 2.0.2's ``GATConv`` as kernel/gcn_img_snp.py calls it (TEST INFRASTRUCTURE).

``GATConv(in, out, edge_dim=1)`` with the defaults heads=1, concat=True, negative_slope=0.2, dropout=0,
add_self_loops=True, fill_value='mean', bias=True.  PyG is not vendored by the reference and cannot be installed
here, so this was written from PyG 2.0.2's published source, not executed against it: **parity UNPINNED by the
reference**, like the GCNConv stand-in of oracle/pyg_ops.py.  It is pinned only by the hand-computed cases of
tests/test_gat_reference.py.  Two details are the least certain:
  * the 'mean' loop fill is reduced over edge_index[1] (the TARGET of each kept edge);
  * the softmax denominator carries + 1e-16 (torch_geometric.utils.softmax).

One layer, x [N, Fin], edges (src = edge_index[0], dst = edge_index[1]), scalar edge values ea [E]:
  h = x W^T (W = lin_src.weight; lin_dst is the same module), a_s = h . att_src, a_d = h . att_dst,
  c = lin_edge.weight[:, 0] . att_edge;
  edges = every stored edge with src != dst (all stored loops dropped, duplicates kept) + one loop per node n whose
  ea is the mean of the kept edges' ea with dst = n (0 if none), appended after them;
  z = leaky_relu(a_s[src] + a_d[dst] + ea c, 0.2); alpha = exp(z - max_dst z) / (sum_dst exp(z - max_dst z) + 1e-16);
  out[i] = sum_{dst = i} alpha h[src] + bias.
"""
import math

import torch

STATED = ("GATConv = tests/golden/gat_standin.py (PyG 2.0.2 GATConv(heads=1, edge_dim=1, add_self_loops, "
          "fill_value='mean') restated from its source, PyG absent: unpinned; loop fill reduced by edge_index[1]; "
          "softmax denominator + 1e-16)")


def gat_edges(edge_index, ea, num_nodes):
    """(src, dst, ea) after remove_self_loops + add_self_loops(fill_value='mean'): kept edges in stored order, then one
    loop per node in node order."""
    src, dst = edge_index[0], edge_index[1]
    keep = src != dst
    src, dst, ea = src[keep], dst[keep], ea[keep]
    cnt = torch.zeros(num_nodes, dtype=ea.dtype).index_add(0, dst, torch.ones_like(ea))
    tot = torch.zeros(num_nodes, dtype=ea.dtype).index_add(0, dst, ea)
    fill = tot / cnt.clamp(min=1)
    ar = torch.arange(num_nodes, dtype=src.dtype)
    return torch.cat([src, ar]), torch.cat([dst, ar]), torch.cat([ea, fill])


def edge_softmax(z, index, num_nodes):
    """torch_geometric.utils.softmax(z, index): max-subtracted, + 1e-16 in the denominator."""
    zmax = torch.full((num_nodes,), -math.inf, dtype=z.dtype).scatter_reduce(0, index, z.detach(), "amax")
    e = (z - zmax[index]).exp()
    den = torch.zeros(num_nodes, dtype=z.dtype).index_add(0, index, e) + 1e-16
    return e / den[index]


def gat_conv(x, edge_index, ea, weight, att_src, att_dst, lin_edge, att_edge, bias, return_alpha=False):
    """One GATConv forward (parameters as PyG names them; the att_* may be [1, 1, F] or [F], lin_edge [F, 1] or [F])."""
    n = x.shape[0]
    src, dst, ea2 = gat_edges(edge_index.cpu(), ea.reshape(-1).to(x.dtype), n)
    h = x @ weight.t()
    a_s = h @ att_src.reshape(-1)
    a_d = h @ att_dst.reshape(-1)
    c = (lin_edge.reshape(-1) * att_edge.reshape(-1)).sum()
    z = torch.nn.functional.leaky_relu(a_s[src] + a_d[dst] + ea2 * c, 0.2)
    alpha = edge_softmax(z, dst, n)
    out = torch.zeros(n, h.shape[1], dtype=h.dtype).index_add(0, dst, alpha.unsqueeze(1) * h[src]) + bias
    return (out, alpha, (src, dst)) if return_alpha else out


def glorot_(t, fan_in, fan_out):
    a = math.sqrt(6.0 / (fan_in + fan_out))
    with torch.no_grad():
        t.uniform_(-a, a)


class GATConvModule(torch.nn.Module):
    """Drop-in for ``torch_geometric.nn.GATConv(in, out, edge_dim=1)`` with PyG 2.0.2's parameter names:
    ``att_src``, ``att_dst`` [1, 1, out], ``lin_src.weight`` [out, in] (``lin_dst`` IS ``lin_src``: its own state_dict
    key, one tensor), ``lin_edge.weight`` [out, 1], ``att_edge`` [1, 1, out], ``bias`` [out]."""

    def __init__(self, in_channels, out_channels, edge_dim=None, **kwargs):
        super().__init__()
        assert edge_dim == 1 and kwargs.get("heads", 1) == 1
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin_src = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = torch.nn.Parameter(torch.empty(1, 1, out_channels))
        self.att_dst = torch.nn.Parameter(torch.empty(1, 1, out_channels))
        self.lin_edge = torch.nn.Linear(1, out_channels, bias=False)
        self.att_edge = torch.nn.Parameter(torch.empty(1, 1, out_channels))
        self.bias = torch.nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        f = self.out_channels
        glorot_(self.lin_src.weight, self.in_channels, f)
        glorot_(self.lin_edge.weight, 1, f)
        for p in (self.att_src, self.att_dst, self.att_edge):
            glorot_(p, 1, f)
        with torch.no_grad():
            self.bias.zero_()

    def forward(self, x, edge_index, edge_attr):
        return gat_conv(x, edge_index, edge_attr, self.lin_src.weight, self.att_src, self.att_dst,
                        self.lin_edge.weight, self.att_edge, self.bias)
