"""fp64 statements of the cross-attention WEIGHTS (the second output of ``self.multihead_attn(...)``,
kernel/sgcn_img_snp.py:240) for the tests of igcn_attn_weights / SGCN_GCN_IMGSNP.attention_weights.  The oracle is torch
itself: ``torch.nn.MultiheadAttention(D, H, batch_first=True).double()`` with ``need_weights=True,
average_attn_weights=True`` on the CPU; ``weights_fp64`` restates it on projection outputs (what the kernel reads) and
tests/test_attn_weights_reference.py holds the restatement to the module."""
import math

import torch

from oracle import go_network as OG
from oracle.pyg_ops import gcn_conv, to_dense_batch
from oracle.sgcn_img_snp import edge_and_region_masks

# |got - want| <= ATOL + RTOL * want element-wise (the project's 1e-4 parity bound with a floor for tiny probabilities),
# and every row sums to 1 within ROW_TOL
ATOL, RTOL, ROW_TOL = 1e-6, 1e-4, 1e-5


def weights_fp64(q, kv, heads):
    """mean_h softmax(q_h k_h^T / sqrt(hd)) [B, Lq, Lk] (fp64, CPU) from q [B, Lq, D] and kv [B, Lk, 2D] (key | value)."""
    q, kv = q.detach().double().cpu(), kv.detach().double().cpu()
    b, lq, d = q.shape
    lk, hd = kv.shape[1], d // heads
    qh = q.view(b, lq, heads, hd).transpose(1, 2)
    kh = kv.reshape(b, lk, 2, heads, hd)[:, :, 0].permute(0, 2, 3, 1)
    return torch.softmax((qh @ kh) / math.sqrt(hd), dim=-1).mean(dim=1)


def mha_module_weights(query, memory, w, bias, heads):
    """The weights of torch's own module (fp64) for inputs ``query`` [B, Lq, D], ``memory`` [B, Lk, D] and a packed input
    projection (w [3D, D], bias [3D]), and the projection outputs (q, kv) ``weights_fp64`` restates them from."""
    d = w.shape[1]
    mha = torch.nn.MultiheadAttention(d, heads, batch_first=True).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(w.double())
        mha.in_proj_bias.copy_(bias.double())
        query, memory = query.double(), memory.double()
        _, att = mha(query, memory, memory, need_weights=True, average_attn_weights=True)
        q = query @ w[:d].double().t() + bias[:d].double()
        kv = memory @ w[d:].double().t() + bias[d:].double()
    return att, q, kv


def model_weights_fp64(sd, cfg, go_idx, data, is_explain):
    """SGCN_GCN_IMGSNP.forward :207-240 in fp64 up to the attention module, whose weights are returned [B, rois, Ntop].
    ``sd``: an fp64 state dict; ``cfg``: SimpleNamespace(rois, heads); ``data``: an fp64 CPU batch."""
    x, ei, ew, snps = data.x, data.edge_index, data.edge_attr, data.snps_feat
    if is_explain:
        x, ew, _, snps = edge_and_region_masks(sd, x, ei, ew, cfg.rois, snps)
    hs = [torch.relu(gcn_conv(x, ei, ew, sd["conv1.lin.weight"], sd["conv1.bias"]))]
    i = 0
    while f"convs.{i}.lin.weight" in sd:
        hs.append(torch.relu(gcn_conv(hs[-1], ei, ew, sd[f"convs.{i}.lin.weight"], sd[f"convs.{i}.bias"])))
        i += 1
    xcat = torch.cat(hs, dim=1)
    dense, _ = to_dense_batch(xcat, data.batch, float(xcat.min()) - 1)
    _, _, atten_out = OG.go_forward(sd, go_idx, snps, False, False, prefix="go_network.")
    att, _, _ = mha_module_weights(dense, atten_out, sd["multihead_attn.in_proj_weight"],
                                   sd["multihead_attn.in_proj_bias"], cfg.heads)
    return att


def max_errors(got, want):
    """(largest |got - want| / (ATOL + RTOL * want), largest |row sum - 1|) of got [B, Lq, Lk] against fp64 ``want``."""
    g, w = got.detach().double().cpu(), want.double()
    assert tuple(g.shape) == tuple(w.shape), (tuple(g.shape), tuple(w.shape))
    assert bool(torch.isfinite(g).all())
    return float(((g - w).abs() / (ATOL + RTOL * w)).max()), float((g.sum(-1) - 1).abs().max())


def assert_weights(got, want, what=""):
    err, row = max_errors(got, want)
    print(f"{what}: error / bound {err:.3e}, row sum {row:.3e}")
    assert err <= 1.0, f"{what}: |got - want| is {err:.3e} x (1e-6 + 1e-4 want)"
    assert row <= ROW_TOL, f"{what}: a row sums to 1 +- {row:.3e}"
