"""Drop-in ``GCN_IMGSNP`` on the HIP kernels: the unmasked baseline of kernel/gcn_img_snp.py:13-274.

Interface of the reference: constructor kwargs (:15-16, ``num_features``, ``isuseFeat4Regr``, ``ifUseGAT`` included),
``forward(data, temperature, device)`` and its 6-tuple (:145,272), ``consist_loss`` (:122), ``OrthogonalConstraint``
(:137), ``reset_parameters`` (:91), the parameters ``prob``, ``prob_bias``, ``edge_prob``, ``snps_prob`` (the last three
take no gradient: nothing in forward() reads them) and an identical ``state_dict()`` key set — with ``ifUseGAT`` the
PyG 2.0.2 GATConv keys ``<conv>.att_src``, ``.att_dst``, ``.att_edge``, ``.bias``, ``.lin_src.weight``,
``.lin_dst.weight`` (the same tensor as lin_src: one entry of ``parameters()``) and ``.lin_edge.weight``.

forward() is ONE plain pass of SGCN_GCN_IMGSNP's route machinery: no masks, the regression head reads
``cat(out_lin, data.x * prob)`` (:262-266, ``isuseFeat4Regr``: the sibling's ``isuseProb4Regr`` input).  The graph
stack is the sibling's GCNConv stack, or with ``ifUseGAT`` the LDS-resident GAT stack (ops.GatStack: one kernel per
direction; shapes outside it raise ValueError — there is no other GAT path).  train.losses() takes the five-term loss of
kernel/train_eval_gcn_img_snps.py:450-484 for this model.
"""
import math

import torch
import torch.nn.functional as F
from torch.nn import Linear, Parameter

from . import ops
from .sgcn_img_snp import GCNConv, SGCN_GCN_IMGSNP, _grid_width, _unpad

ROIS_REF = 90            # kernel/gcn_img_snp.py:58-83 sizes lin1 / lin1_regr with a literal 90


def _glorot_(t, fan_in, fan_out):
    a = math.sqrt(6.0 / (fan_in + fan_out))
    with torch.no_grad():
        t.uniform_(-a, a)


class GATConv(torch.nn.Module):
    """PyG 2.0.2 ``GATConv(in, out, edge_dim=1)`` as the reference builds it (heads 1, concat, negative_slope 0.2,
    dropout 0, add_self_loops with fill_value 'mean', bias): parameter names, shapes and glorot / zeros initialisation
    of PyG.  ``lin_dst`` is ``lin_src``.  Computed by ops.GatStack for the whole stack, not per layer."""

    def __init__(self, in_channels, out_channels, edge_dim=1):
        super().__init__()
        if edge_dim != 1:
            raise NotImplementedError("GATConv: edge_dim=1 only (the reference's call)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin_src = Linear(in_channels, out_channels, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = Parameter(torch.empty(1, 1, out_channels))
        self.att_dst = Parameter(torch.empty(1, 1, out_channels))
        self.lin_edge = Linear(edge_dim, out_channels, bias=False)
        self.att_edge = Parameter(torch.empty(1, 1, out_channels))
        self.bias = Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        f = self.out_channels
        _glorot_(self.lin_src.weight, self.in_channels, f)
        _glorot_(self.lin_edge.weight, 1, f)
        for p in (self.att_src, self.att_dst, self.att_edge):
            _glorot_(p, 1, f)
        with torch.no_grad():
            self.bias.zero_()

    def kernel_params(self):
        """W, bias, att_src, att_dst, lin_edge, att_edge in the layout igcn_gat_stack_* reads."""
        return [self.lin_src.weight, self.bias, self.att_src.view(-1), self.att_dst.view(-1),
                self.lin_edge.weight.view(-1), self.att_edge.view(-1)]


def gat_padded_params(convs):
    """(f, fp, flat parameter list of ops.GatStack) of the GATConv list ``convs``.  Hidden widths off the kernels' grid
    (10, 5) run padded to fp = the next of 4 / 8 / 16 / 32: W gets zero rows (and zero columns past layer 0), bias and
    the four attention vectors zero entries — the padded h columns are 0, add 0 to every logit and leave 0 through the
    ReLU; ``_unpad`` slices them off the concatenation."""
    f = convs[0].out_channels
    fp = _grid_width(f)
    out = []
    for l, c in enumerate(convs):
        w, *vecs = c.kernel_params()
        if fp != f:
            w = F.pad(w, (0, 0 if l == 0 else fp - f, 0, fp - f))
            vecs = [F.pad(v, (0, fp - f)) for v in vecs]
        out += [w, *vecs]
    return f, fp, out


def gat_stack(convs, x_in, ew_in, plan_g, rois):
    """xcat = cat_l relu(GATConv_l(.)) on the batched plan ``plan_g``: one ops.GatStack launch per direction."""
    f, fp, params = gat_padded_params(convs)
    if not x_in.is_cuda:
        raise ValueError("GAT stack: the GATConv layers run on the GPU kernels only (igcn_gat_stack_*)")
    return _unpad(ops.GatStack.apply(x_in, ew_in, plan_g, rois, *params), f, fp)


def gat_attention(model, convs, data, isExplain=False):
    """The attention coefficients of the GATConv list ``convs`` on a batch, as dense maps [B, L, rois, rois] (fp32; source
    row, target column; ops.gat_stack_alpha): what PyG returns under ``return_attention_weights=True`` and the reference's
    forwards (kernel/gcn_img_snp.py:217-221, kernel/sgcn.py:235-267) never ask for.  The plain pass reads ``data.x`` and
    ``data.edge_attr``; ``isExplain``: ``x * prob`` and ``edge_weight * e`` of ``model.cal_probability``, as the masked
    forward does.  Under ``torch.no_grad()``; reads the parameters and writes nothing of the model."""
    x = data.x
    if x.shape[0] % model.rois:
        raise ValueError(f"every graph must have exactly rois={model.rois} nodes (got {x.shape[0]} nodes)")
    with torch.no_grad():
        plan = ops.plan_for(data)
        plan.flush_pending_check()
        x_in, ew_in = x, data.edge_attr
        if isExplain:
            x_in, ew_in = model.cal_probability(x, data.edge_index, data.edge_attr, plan=plan)[:2]
        return ops.gat_stack_alpha(x_in, ew_in, plan, model.rois, *gat_padded_params(convs)[2])


class GCN_IMGSNP(SGCN_GCN_IMGSNP):
    # one plain pass per step (train.losses dispatches the five-term loss): no batched (plain | masked) sweep
    batched_passes = False
    single_pass = True   # train.losses: the five-term loss; train.Evaluator refuses the model

    def __init__(self, num_layers, hidden, A_g, A, pool_dim, l_dim, device, *args, hidden_linear=64, rois=90, H_0=3,
                 num_features=3, num_classes=2, isCrossAtten=False, isSoftSimilarity=False, rbf_gamma=0.005,
                 graph_pool=False, isuseFeat4Regr=True, num_regr=4, model4eachregr=False, isImageOnly=True,
                 isSNPsOnly=False, ifUseGAT=False, **kwargs):
        if kwargs.get("isMultiFusion"):
            raise ValueError("GCN_IMGSNP has no isMultiFusion variant")
        kwargs.pop("isMultiFusion", None)
        super().__init__(num_layers, hidden, A_g, A, pool_dim, l_dim, device, *args, hidden_linear=hidden_linear,
                         rois=rois, H_0=H_0, num_classes=num_classes, isCrossAtten=isCrossAtten,
                         isSoftSimilarity=isSoftSimilarity, rbf_gamma=rbf_gamma, graph_pool=graph_pool,
                         isuseProb4Regr=isuseFeat4Regr, num_regr=num_regr, model4eachregr=model4eachregr,
                         isImageOnly=isImageOnly, isSNPsOnly=isSNPsOnly, isMultiFusion=False, **kwargs)
        self.isuseFeat4Regr, self.ifUseGAT, self.num_features = isuseFeat4Regr, bool(ifUseGAT), num_features
        conv = (lambda i, o: GATConv(i, o, edge_dim=1)) if self.ifUseGAT else GCNConv
        # (assignment to the registered names keeps the sibling's module order, so state_dict() lists the same keys)
        self.conv1 = conv(num_features, hidden)
        for i in range(len(self.convs)):
            self.convs[i] = conv(hidden, hidden)
        if not graph_pool:
            # :66-83 size the head inputs with 90 ROIs whatever ``rois`` is (the reference's trainer has 90)
            d_img = ROIS_REF * num_layers * hidden
            d_lin = d_img if isImageOnly else (l_dim + 54 if isSNPsOnly else d_img + l_dim)
            d_reg = d_lin + (ROIS_REF * H_0 if isuseFeat4Regr and not isSNPsOnly else 0)
            if self.lin1.in_features != d_lin:
                self.lin1 = Linear(d_lin, hidden_linear)
            if self.lin1_regr.in_features != d_reg:
                self.lin1_regr = Linear(d_reg, hidden_linear)

    def forward(self, data, temperature=None, device=None):
        """:145-272.  Returns (log_softmax, x_hat, out_z, out_lin, linear_outf, our_reg)."""
        return self._forward_grouped(data, temperature, device, (False,))[0]

    def forward_pair(self, data, temperature=None, device=None):
        raise NotImplementedError("GCN_IMGSNP runs one plain pass per step (no isExplain pass)")

    def edge_importance(self, data, weighted=False, return_count=False):
        raise ValueError("edge_importance: GCN_IMGSNP trains no masks (prob_bias takes no gradient and nothing in its "
                         "forward reads it)")

    def gat_attention(self, data, isExplain=False):
        """``gat_attention`` (this module) of the one plain pass; needs ``ifUseGAT``."""
        if isExplain:
            raise ValueError("GCN_IMGSNP has one plain pass (no masked pass)")
        if not self.ifUseGAT:
            return super().gat_attention(data)
        return gat_attention(self, self._gcn_convs, data)

    def _image_route(self, data, plan, flags):
        if flags != (False,):
            raise ValueError("GCN_IMGSNP has one plain pass (no masked pass)")
        if not self.ifUseGAT:
            return super()._image_route(data, plan, flags)
        fan = False
        plan.flush_pending_check()
        if getattr(plan, "dense_blocks", False) and data.x.is_cuda:
            ops.call("igcn_rider_flush", ops.stream_ptr())
        plan.flush_pending_build()
        return self._generic_route, fan

    def _stack(self, x_in, ew_in, plan, g, fan):
        if not self.ifUseGAT:
            return super()._stack(x_in, ew_in, plan, g, fan)
        return gat_stack(self._gcn_convs, x_in, ew_in, plan.replicate(g), self.rois), None
