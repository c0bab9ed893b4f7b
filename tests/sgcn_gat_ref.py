"""float64 restatement of SGCN_GAT's forward (kernel/sgcn.py:235-267) for the tests: cal_probability as
oracle.sgcn_img_snp.edge_and_region_masks states it, the GATConv layers on the stand-in tests/golden/gat_standin.gat_conv
(PyG 2.0.2 GATConv restated from its source: parity unpinned), the dense view of uniform graphs and the two-layer head.
``sd``: parameter name -> tensor (``model.named_parameters()`` names)."""
import torch
import torch.nn.functional as F

from gat_standin import gat_conv
from oracle.sgcn_img_snp import edge_and_region_masks


def _conv(sd, name, h, ei, ea):
    return torch.relu(gat_conv(h, ei, ea, sd[name + ".lin_src.weight"], sd[name + ".att_src"], sd[name + ".att_dst"],
                               sd[name + ".lin_edge.weight"], sd[name + ".att_edge"], sd[name + ".bias"]))


def model_forward(sd, rois, data, is_explain=False):
    """log_softmax [B, C] of a batch of uniform ``rois``-node graphs, dropout off."""
    x, ei, ew = data.x, data.edge_index, data.edge_attr
    if is_explain:
        x, ew, _ = edge_and_region_masks(sd, x, ei, ew, rois)
    hs = [_conv(sd, "conv1", x, ei, ew)]
    i = 0
    while f"convs.{i}.lin_src.weight" in sd:
        hs.append(_conv(sd, f"convs.{i}", hs[-1], ei, ew))
        i += 1
    z = torch.cat(hs, dim=1).reshape(x.shape[0] // rois, -1)          # to_dense_batch of uniform graphs
    h = torch.relu(z @ sd["lin1.weight"].t() + sd["lin1.bias"])
    return F.log_softmax(h @ sd["lin2.weight"].t() + sd["lin2.bias"], dim=-1)
