"""Restatement of SGCN_Ori (kernel/sgcn.py:11-151) and of its graph stack for the tests, on oracle.pyg_ops.gcn_conv; runs
in the dtype of its inputs (the tests use float64).  ``sd``: name -> tensor with the reference's state_dict keys.

  stack(...)            :120-138   h1 = relu(conv1), acts = conv3(h1) (the Grad-CAM tap, pre-ReLU), z = cat(z1, z2)
  model_forward(...)    :111-148   masks (cal_probability :74-85 = oracle.sgcn_img_snp.edge_and_region_masks), the stack,
                                   fc1 -> ReLU -> bn1 -> fc2 -> ReLU -> bn2 -> fc3 -> log_softmax (dropout off, or with
                                   the factors a run recorded: ``keeps``)
  loss_probability      :87-109    = oracle.sgcn.loss_probability (the same formula as SGCN_GCN's)
  train_losses(...)                train() kernel/train_eval_sgcn.py:303-308
  param_shapes(...)                the reference's state_dict keys and shapes
"""
import torch
import torch.nn.functional as F

from oracle.pyg_ops import gcn_conv
from oracle.sgcn import loss_probability  # noqa: F401  (re-exported)
from oracle.sgcn_img_snp import HP, edge_and_region_masks


def stack(x, edge_index, edge_weight, w1, b1, w3, b3, rois):
    """(z [B, rois*F1 + rois*F3], acts [N, F3], h1 [N, F1]) for uniform graphs of ``rois`` nodes."""
    h1 = torch.relu(gcn_conv(x, edge_index, edge_weight, w1, b1))
    acts = gcn_conv(h1, edge_index, edge_weight, w3, b3)
    h3 = torch.relu(acts)
    b = x.shape[0] // rois
    return torch.cat((h1.reshape(b, -1), h3.reshape(b, -1)), 1), acts, h1      # to_dense_batch of uniform graphs


def _bn(x, sd, name, training, stats):
    """BatchNorm1d: batch statistics (biased variance) when training, running statistics otherwise.  ``stats`` (a dict
    or None) receives the batch mean / unbiased variance for the running-statistics update."""
    if training:
        mean, var = x.mean(0), x.var(0, unbiased=False)
        if stats is not None:
            stats[name] = (mean.detach(), x.var(0, unbiased=True).detach())
    else:
        mean, var = sd[name + ".running_mean"].to(x.dtype), sd[name + ".running_var"].to(x.dtype)
    return (x - mean) / torch.sqrt(var + 1e-5) * sd[name + ".weight"] + sd[name + ".bias"]


def model_forward(sd, rois, data, is_explain=False, training=False, stats=None, taps=None, keeps=None):
    """log_softmax [B, C].  ``taps`` (a dict or None) receives final_conv_acts (retaining its gradient).  ``keeps``: None
    (dropout off) or the two factor tensors of Dropout(0.5) behind bn1 [B, 64] and Dropout(0.7) behind bn2 [B, 16] (:144,
    :146), {0, 1 / (1 - p)}, as a training run of the HIP model recorded them."""
    x, ei, ew = data.x, data.edge_index, data.edge_attr
    if is_explain:
        x, ew, _ = edge_and_region_masks(sd, x, ei, ew, rois)
    z, acts, _ = stack(x, ei, ew, sd["conv1.lin.weight"], sd["conv1.bias"], sd["conv3.lin.weight"], sd["conv3.bias"], rois)
    if taps is not None:
        if acts.requires_grad:
            acts.retain_grad()
        taps["acts"] = acts
    h = _bn(torch.relu(z @ sd["fc1.weight"].t() + sd["fc1.bias"]), sd, "bn1", training, stats)
    if keeps is not None:
        assert keeps[0].shape == h.shape, (keeps[0].shape, h.shape)
        h = h * keeps[0].to(h.dtype)
    h = _bn(torch.relu(h @ sd["fc2.weight"].t() + sd["fc2.bias"]), sd, "bn2", training, stats)
    if keeps is not None:
        assert keeps[1].shape == h.shape, (keeps[1].shape, h.shape)
        h = h * keeps[1].to(h.dtype)
    return F.log_softmax(h @ sd["fc3.weight"].t() + sd["fc3.bias"], dim=-1)


def train_losses(sd, rois, data, hp=HP, taps=None):
    """(loss, terms, (out, out_p)) of train(): plain pass, masked pass, regulariser.  ``taps``: {"plain": {}, "masked": {}}."""
    y = data.y.view(-1)
    out = model_forward(sd, rois, data, False, True, taps=None if taps is None else taps["plain"])
    out_p = model_forward(sd, rois, data, True, True, taps=None if taps is None else taps["masked"])
    t = {"ce": F.nll_loss(out, y), "mi": F.nll_loss(out_p, y),
         "prob": loss_probability(sd, data.x, data.edge_index, data.edge_attr, rois, hp)}
    return hp.lamda_ce * t["ce"] + t["prob"] + hp.lamda_mi * t["mi"], t, (out, out_p)


def param_shapes(h0, h1, h2, h3, class_num=2, rois=90):
    shp = {"prob": (rois, h0), "prob_bias": (2 * h0, 1), "edge_prob": (rois, rois),
           "conv1.lin.weight": (h1, h0), "conv1.bias": (h1,), "conv2.lin.weight": (h2, h1), "conv2.bias": (h2,),
           "conv3.lin.weight": (h3, h1), "conv3.bias": (h3,),
           "fc1.weight": (64, rois * h3 + rois * h2), "fc1.bias": (64,), "fc2.weight": (16, 64), "fc2.bias": (16,),
           "fc3.weight": (class_num, 16), "fc3.bias": (class_num,)}
    for name, c in (("bn1", 64), ("bn2", 16)):
        shp.update({f"{name}.weight": (c,), f"{name}.bias": (c,), f"{name}.running_mean": (c,),
                    f"{name}.running_var": (c,), f"{name}.num_batches_tracked": ()})
    return shp
