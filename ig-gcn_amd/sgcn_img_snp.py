"""Drop-in ``SGCN_GCN_IMGSNP`` on the HIP kernels.

Mirrors the interface of the reference's kernel/sgcn_img_snp.py: constructor kwargs (:15-17),
``forward(data, temperature, device, isExplain=False)`` and its 6-tuple (:207,307), ``cal_probability``
(:133), ``loss_probability`` (:153), ``consist_loss`` (:183), ``OrthogonalConstraint`` (:198),
``reset_parameters`` (:104), the attributes read by util/output.py:21-23 (``prob``, ``snps_prob``,
``prob_bias``) and an identical ``state_dict()`` key set (PyG-2.0.2 GCNConv keys ``<conv>.lin.weight``,
``<conv>.bias``).

What changes underneath: one ``GraphPlan`` per batch shared by both passes and the mask loss; gcn_norm
once per pass instead of once per layer; scatter-aggregate / masks / dense transforms are libigcn kernels;
the two ``x.min().item()`` host syncs of :225,293 are gone (every graph has exactly ``rois`` nodes, so
to_dense_batch is a view); OrthogonalConstraint uses the Gram identity (B x B instead of (R*D)^2).
"""
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F
from torch.nn import Linear, Parameter, init

from . import ops, switches
from .go_model import Gene_ontology_network


class GCNConv(torch.nn.Module):
    """GCNConv(in, out) with PyG 2.0.2's parameter names; forward = MFMA transform + scatter-aggregate."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = Linear(in_channels, out_channels, bias=False)
        self.bias = Parameter(torch.zeros(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))        # PyG glorot
        with torch.no_grad():
            self.lin.weight.uniform_(-a, a)
            self.bias.zero_()

    def forward(self, x, plan, coef, relu=False, bf16=False):
        what, wloop, tstream, sstream = coef
        h = ops.linear(x, self.lin.weight, bf16=bf16)
        return ops.GcnPropagate.apply(h, what, wloop, self.bias, plan, relu, tstream, sstream)


_WIDE = (4, 8, 16, 32, 64)          # widths the 16-byte-per-lane kernels (and the LDS-resident stack, <= 32) cover
_MODES = {(False,): "plain", (True,): "masked", (False, True): "both"}       # explain flags -> ops.DenseSgcn's mode


def _grid_width(f):
    """The kernels' width for GCNConv width ``f``: the next width of ``_WIDE`` (``f`` itself when it is on it)."""
    return f if f in _WIDE else next((w for w in _WIDE if w >= f), f)


def _padded_params(convs):
    """(f, fp, [W_0, b_0, W_1, b_1, ...]) of the GCNConv list ``convs``.  Hidden widths off the kernels' grid (the
    reference's sweep has hidden = 10 and 5, main.py:152-158) run PADDED to fp = ``_grid_width(f)``: zero rows / columns
    in the weights and zero bias entries keep the extra activation columns exactly 0 through ReLU and the next layer,
    every kernel moves 16 bytes per lane, and the padding is sliced away once, at the concatenation (``_unpad``)."""
    f = convs[0].out_channels
    fp = _grid_width(f)
    ws = [c.lin.weight for c in convs]
    bs = [c.bias for c in convs]
    if fp != f:
        ws = [F.pad(w, (0, 0 if l == 0 else fp - f, 0, fp - f)) for l, w in enumerate(ws)]
        bs = [F.pad(b, (0, fp - f)) for b in bs]
    return f, fp, [t for pair in zip(ws, bs) for t in pair]


def _unpad(xcat, f, fp):
    """The concatenation [n, L*fp] of a padded stack as [n, L*f]."""
    return xcat if fp == f else xcat.view(xcat.shape[0], -1, fp)[:, :, :f].reshape(xcat.shape[0], -1)


def sgcn_stack(convs, x_in, ew_in, plan_g, rois, fused=True, bf16=False, dual=False):
    """xcat = cat_l relu(GCNConv_l(.)) (kernel/sgcn_img_snp.py:218-224, kernel/sgcn.py:370-377) for the GCNConv list
    ``convs`` on the batched plan ``plan_g``, at the kernels' width (``_padded_params``).  Small uniform graphs take the
    LDS-resident stack (igcn_sgcn_stack_*: one kernel per direction); everything else gcn_norm once + (MFMA transform,
    scatter-aggregate) per layer."""
    f, fp, wb = _padded_params(convs)
    if (fused and not bf16 and x_in.is_cuda
            and ops.sgcn_stack_supported(plan_g, rois, x_in.shape[1], fp, len(convs))):
        if dual and fp == f:
            # two autograd handles of one buffer for the model's two consumers: their gradients meet inside the backward
            # kernel (ops.SgcnStack), not in an autograd add in front of it
            return ops.SgcnStack.apply(x_in, ew_in, plan_g, -rois, *wb)
        xcat = ops.SgcnStack.apply(x_in, ew_in, plan_g, rois, *wb)
    else:
        coef = ops.GcnNorm.apply(ew_in, plan_g)                       # once per pass (PyG: once per layer)
        what, wloop, tstream, sstream = coef
        h, hs = x_in, []
        for w, b in zip(wb[::2], wb[1::2]):
            h = ops.GcnPropagate.apply(ops.linear(h, w, bf16=bf16), what, wloop, b, plan_g, True, tstream, sstream)
            hs.append(h)
        xcat = ops.concat_cols(hs)
    xcat = _unpad(xcat, f, fp)
    return (xcat, xcat) if dual else xcat


def masked_inputs(model, data, plan, flags, stacked, snps_feat=None, aliases=None):
    """(x_in, ew_in, snps_in, e): the GCNConv stack's inputs for the passes ``flags`` (True: masked) stacked pass-major,
    and the masked pass's edge mask.  ``stacked``: the train step's (plain | masked) pair, whose two halves the mask launch
    writes itself (ops.EdgeMaskStacked), reading ``aliases`` = (x, prob, snps_prob) if given (ops.GradFan)."""
    x, edge_index, edge_weight = data.x, data.edge_index, data.edge_attr
    if stacked:
        x_m, prob_m, sp_m = aliases or (x, model.prob, None)
        x_in, ew_in, e = ops.EdgeMaskStacked.apply(x_m, prob_m, model.prob_bias, edge_weight, plan, model.rois)
        snps_in = None if snps_feat is None else ops.SnpsMask.apply(snps_feat, sp_m, True)[0]
        return x_in, ew_in, snps_in, e
    plain, masked, e = (x, edge_weight, snps_feat), None, None
    if any(flags):
        snps = () if snps_feat is None else (snps_feat,)
        x_m, ew_m, _, e, *snps_m = model.cal_probability(x, edge_index, edge_weight, *snps, plan=plan)
        masked = (x_m, ew_m, snps_m[0] if snps_m else None)
    passes = [masked if f else plain for f in flags]
    x_in, ew_in, snps_in = (ts[0] if len(ts) == 1 or ts[0] is None else torch.cat(ts, dim=0) for ts in zip(*passes))
    return x_in, ew_in, snps_in, e


def edge_importance(model, data, weighted=False, return_count=False):
    """The learned connective-importance mask of ``model.cal_probability`` (kernel/sgcn_img_snp.py:133-151; kernel/sgcn.py
    :198-209,321-332) of every subject as a dense region x region map [B, rois, rois] (fp32) — source row, target column:
    the orientation of the reference's ``data.A``, so a map overlays it.  ``weighted``: ``edge_weight * e``, the weight the
    masked pass's convolutions consume, instead of ``e``; ``return_count``: also the number of stored copies of every edge,
    (map, cnt).  The stored copies of an edge are summed in stored order; 0 where no edge is stored.  Two launches under
    ``torch.no_grad()`` — the model's own mask launch (igcn_edge_mask_fwd; batches of complete graphs take it too) and
    ops.edge_dense_map — that read the parameters and write nothing of the model."""
    x = data.x
    if x.shape[0] % model.rois:
        raise ValueError(f"every graph must have exactly rois={model.rois} nodes (got {x.shape[0]} nodes)")
    with torch.no_grad():
        plan = ops.plan_for(data)
        plan.flush_pending_check()
        _, ewm, _, e = model.cal_probability(x, data.edge_index, data.edge_attr, plan=plan)[:4]
        return ops.edge_dense_map((ewm if weighted else e).reshape(-1), plan, model.rois, return_count)


class _ImageBranch(NamedTuple):
    """What an image route hands the rest of the forward."""
    xcat: torch.Tensor                  # cat_l relu(GCNConv_l(.)) of every pass, [g*n, L*hidden]
    xcat_img: torch.Tensor              # a second handle of xcat for the image head input (_dual_consumer), or None
    snps_in: torch.Tensor               # the GO network's input: the SNP batch of every pass
    prob_h: torch.Tensor                # prob and data.x as the head inputs read them (ops.GradFan aliases or the
    x_h: torch.Tensor                   # tensors themselves)
    edge_prob: torch.Tensor = None      # the masked pass's edge mask (last_edge_prob)
    reg: torch.Tensor = None            # loss_probability's partial sums, reduced inside the route's launches
    fan: tuple = None                   # (prob, snps_prob) gradient aliases loss_probability must read


class _Handoff(NamedTuple):
    """What a forward leaves for loss_probability: the identity of its inputs (``_reg_key``), the regulariser it reduced
    with the hp it used, and the gradient aliases a recomputed regulariser reads — the last two handed out once."""
    key: tuple = (None,) * 4
    hp: tuple = None
    reg: torch.Tensor = None
    fan: tuple = None


def rbf_kernel_torch(X, Y, gamma=0.015):
    """util/image_cluster.py:15-31."""
    return torch.exp(-gamma * torch.cdist(X, Y, p=2) ** 2)


class SGCN_GCN_IMGSNP(torch.nn.Module):
    def __init__(self, num_layers, hidden, A_g, A, pool_dim, l_dim, device, *args, hidden_linear=64, rois=90,
                 H_0=3, num_classes=2, isCrossAtten=False, isSoftSimilarity=False, rbf_gamma=0.005,
                 graph_pool=False, isuseProb4Regr=False, num_regr=4, model4eachregr=False, isImageOnly=True,
                 isSNPsOnly=False, isMultiFusion=False, **kwargs):
        super().__init__()
        if graph_pool and not (isCrossAtten and not isImageOnly and not isSNPsOnly and not isuseProb4Regr):
            # the reference's graph_pool branch (:230-235,246-252) only runs for this flag combination: without
            # cross-attention :247 indexes shape[2] of a 2-D tensor, and the other heads feed lin1 / lin1_regr
            # (3*L*h + l_dim inputs, :51-54) tensors of a different width
            raise ValueError("graph_pool=True needs isCrossAtten=True, isImageOnly=False, isSNPsOnly=False, "
                             "isuseProb4Regr=False (the only combination the reference's forward() runs)")
        if model4eachregr:
            raise NotImplementedError("model4eachregr=True is not built")
        self.device = device
        self.isCrossAtten, self.isSoftSimilarity, self.rbf_gamma = isCrossAtten, isSoftSimilarity, rbf_gamma
        self.model4eachregr, self.isuseProb4Regr = model4eachregr, isuseProb4Regr
        self.isImageOnly, self.isSNPsOnly, self.isMultiFusion = isImageOnly, isSNPsOnly, isMultiFusion
        self.num_regr, self.rois, self.prob_dim, self.graph_pool = num_regr, rois, H_0, graph_pool
        self.input = None
        self.conv1 = GCNConv(H_0, hidden)
        self.convs = torch.nn.ModuleList()
        n_l = 2
        dim_att = hidden
        n_more = (num_layers - 1) if isCrossAtten else (num_layers - 1)
        for _ in range(n_more):
            self.convs.append(GCNConv(hidden, hidden))
        if isCrossAtten:
            dim_att = hidden * num_layers
            self.pool = pool_dim[0]
            self.multihead_attn = torch.nn.MultiheadAttention(dim_att, 2, batch_first=True)
        d_img = rois * num_layers * hidden
        if graph_pool:                                                    # :51-54
            self.lin1 = Linear(3 * num_layers * hidden + l_dim, hidden_linear)
            d_reg = 3 * num_layers * hidden + l_dim
        elif isImageOnly:
            self.lin1 = Linear(d_img, hidden_linear)
            d_reg = d_img + (rois * H_0 if isuseProb4Regr else 0)
        elif isSNPsOnly:
            self.lin1 = Linear(l_dim + 54, hidden_linear)
            d_reg = l_dim + 54
        else:
            self.lin1 = Linear(d_img + l_dim, hidden_linear)
            d_reg = d_img + l_dim + (rois * H_0 if isuseProb4Regr else 0)
        self.lin1_regr = Linear(d_reg, hidden_linear)
        self.lin2 = Linear(hidden_linear, num_classes)
        self.lin2_regr = Linear(hidden_linear, num_regr)
        self.batch_norm_1d = torch.nn.BatchNorm1d(d_img + l_dim)          # unused by forward (as in the reference)
        self.prob = Parameter(torch.empty(rois, H_0))
        self.prob_bias = Parameter(torch.empty(H_0 * 2, 1))
        self.edge_prob = Parameter(torch.empty(rois, rois))               # unused by forward
        self.snps_prob = Parameter(torch.empty(1, 54))
        for p in (self.prob_bias, self.prob, self.edge_prob, self.snps_prob):
            init.kaiming_uniform_(p, a=math.sqrt(5))
        self.go_network = Gene_ontology_network(A_g, A, 2, n_l, [5, 5], pool_dim, l_dim, device,
                                                dim_snps_atten=dim_att)
        self.batch_norm = torch.nn.BatchNorm1d(num_layers * hidden)       # unused by forward
        self._dropout_enabled = True
        # BASELINE configs[4]: the dense feature transforms (GCNConv.lin, the attention projections, lin1 /
        # lin1_regr) with bf16 operands on the matrix cores, fp32 accumulation (igcn_gemm_bf16); default fp32
        self.bf16_transforms = bool(kwargs.get("bf16_transforms", False))
        # one LDS-resident kernel per direction for the whole SGCN stack when the batch allows it (small uniform
        # graphs); IGCN_NO_FUSED_SGCN=1 keeps the per-layer kernels (A/B runs, tests of the unfused path)
        self.fused_sgcn_stack = not switches.on("IGCN_NO_FUSED_SGCN")
        # loss_probability's constants as the dense-block path needs them at FORWARD time (it reduces the mask
        # regulariser inside its first edge pass): (l1_x, ent_x, l1_e, ent_e, eps) — sgcn_hyperparameters.py:18-21;
        # train.losses sets them from the ``hp`` it is given
        self._reg_hp = (0.1, 0.1, 0.1, 0.1, 1e-6)
        self._handoff = _Handoff()

    def reset_parameters(self):
        self.conv1.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        for m in (self.lin1, self.lin2, self.lin1_regr, self.lin2_regr):
            m.reset_parameters()
        with torch.no_grad():
            for p in (self.prob_bias, self.prob, self.edge_prob, self.snps_prob):
                init.kaiming_uniform_(p, a=math.sqrt(5))

    # ---- masks / regularisers --------------------------------------------------------------------
    def _plan(self, data_or_ei, n_nodes=None):
        if torch.is_tensor(data_or_ei):
            return ops.GraphPlan(data_or_ei, n_nodes)
        return ops.plan_for(data_or_ei)

    def cal_probability(self, x, edge_index, edge_weight, snps_feat=None, plan=None):
        plan = plan if plan is not None else ops.GraphPlan(edge_index, x.shape[0])
        xm, ewm, e = ops.EdgeMask.apply(x, self.prob, self.prob_bias, edge_weight, plan, self.rois)
        if snps_feat is not None:
            if snps_feat.is_cuda and snps_feat.dim() == 2 and snps_feat.shape[1] == self.snps_prob.numel():
                snps_m, sp = ops.SnpsMask.apply(snps_feat, self.snps_prob, False)   # sigmoid + multiply, one launch
                return xm, ewm, self.prob, e, snps_m, sp
            sp = torch.sigmoid(self.snps_prob)
            return xm, ewm, self.prob, e, snps_feat * sp, sp
        return xm, ewm, self.prob, e

    @staticmethod
    def _l1_entropy(p, eps):
        n = p.numel()
        l1 = p.norm(p=1) / n
        ent = -torch.sum(p * torch.log(p + eps) + (1 - p) * torch.log((1 - p) + eps)) / n
        return l1, ent

    def loss_probability(self, x, edge_index, edge_weight, hp, eps=1e-6, plan=None, edge_prob=None, partials=False):
        """:153-181 as one fused reduction (igcn_mask_reg_*).  ``edge_prob`` lets the train step reuse the mask
        the explain pass already computed; ``partials``: the un-reduced workgroup sums (ops.LossHead adds them up)."""
        h = self._handoff
        self._handoff = _Handoff(h.key)                               # handed out at most once per forward
        key = self._reg_key(x, edge_weight)
        if (h.reg is not None and (edge_prob is None or edge_prob is self.last_edge_prob)
                and h.hp == (float(hp.lamda_x_l1), float(hp.lamda_x_ent), float(hp.lamda_e_l1),
                             float(hp.lamda_e_ent), float(eps))
                and h.key == key):
            # the forward of the masked pass has already reduced every term ON THESE INPUTS: the dense-block path (edge
            # mask never materialised) or the stacked sweep's mask launch (ops.EdgeMaskStacked with reg_hp).  Anything
            # else — another batch, a second call, parameters that moved since — is recomputed from the arguments, as
            # the reference does (:153-181)
            return h.reg if partials else h.reg.sum()
        if edge_prob is not None and edge_prob is self.last_edge_prob and key[:4] != h.key[:4]:
            edge_prob = None                                          # the mask of another batch: do not reuse it
        if edge_prob is None:
            _, _, _, edge_prob = self.cal_probability(x, edge_index, edge_weight, plan=plan)
        # inside a train step the forward has handed out gradient aliases of prob / snps_prob (ops.GradFan)
        prob, sprob = h.fan or (self.prob, self.snps_prob)
        return ops.MaskRegulariser.apply(prob, edge_prob, sprob, hp.lamda_x_l1, hp.lamda_x_ent,
                                         hp.lamda_e_l1, hp.lamda_e_ent, eps, partials)

    def _reg_key(self, x, edge_weight):
        """Identity of what a cached mask / regulariser was computed from: the batch tensors and the parameter
        versions (torch.optim bumps ``_version``; FlatAdam's kernels do not, which is why the cache is also
        single-use)."""
        return (x.data_ptr(), tuple(x.shape), edge_weight.data_ptr(), tuple(edge_weight.shape),
                self.prob._version, self.prob_bias._version, self.snps_prob._version)

    def laplacian(self, n, tsne_result=None):
        """D - W of consist_loss (:188-193): RBF similarity of the t-SNE embedding, or all-ones."""
        soft = self.isSoftSimilarity and tsne_result is not None
        return ops.rbf_laplacian(tsne_result if soft else None, n, self.rbf_gamma, self.prob.device)

    def batch_losses(self, s, lap, groups=1):
        """(consist_loss(s), OrthogonalConstraint(s)) from ONE B x B Gram matrix s s^T (igcn_gram_loss_*):
        tr(s^T Lap s) = sum_ij Lap_ij G_ij and ||Wn^T Wn - I||_F^2 = sum_ij G_ij^2/(G_ii G_jj) - 2B + R*D."""
        c, o = ops.GramLosses.apply(s, lap, groups)
        return (c[0], o[0]) if groups == 1 else (c, o)

    def consist_loss(self, s, tsne_result=None):
        """:183-196."""
        if len(s) == 0:
            return 0
        return self.batch_losses(s, self.laplacian(s.shape[0], tsne_result))[0]

    def OrthogonalConstraint(self, w):
        """:198-205 (the Laplacian factor is irrelevant for this term)."""
        return self.batch_losses(w, torch.zeros(w.shape[0], w.shape[0], device=w.device))[1]

    def _drop(self, x, p):
        return F.dropout(x, p, True) if (self.training and self._dropout_enabled) else x

    def _cross_attention(self, query, memory, relu_owed=False, defer_out_proj=False):
        """relu(nn.MultiheadAttention(D, 2, batch_first=True)(query, memory, memory)[0]) (:240-241) with the
        parameters of ``self.multihead_attn``: MFMA-GEMM projections (key and value as one GEMM) around the attention
        core igcn_attn_core_*, which works on the projection outputs in place (matrix cores, head_dim <= 96: the
        attention of every row of the reference's sweeps, the hidden-32 rows included — their memory comes from the wide
        GO read-out kernels, attention width 64..160: DESIGN.md section 8); wider heads use a batched GEMM + softmax
        composite."""
        mha = self.multihead_attn
        d, h = mha.embed_dim, mha.num_heads
        b, lq, lk = query.shape[0], query.shape[1], memory.shape[1]
        w, bias = mha.in_proj_weight, mha.in_proj_bias
        bf = self.bf16_transforms
        if ops.attn_core_supported(d, h, lq, lk):
            # projections + core as one autograd node: parameters taken whole (leaves: ONE [3D, D] / [3D] gradient,
            # deferrable partial sums), key / value bias gradients in closed form
            o = ops.ProjectedAttention.apply(query, memory, w, bias, h, bf)
        else:
            # head_dim > 96 (outside the core's coverage): plain batched-GEMM + softmax composite.  Deliberately not
            # the library's fused SDPA kernels (known issues)
            q, kv = ops.InProj.apply(query, memory, w, bias, bf)             # [B, Lq, D], [B, Lk, 2D] = key | value
            hd = d // h
            qh = q.view(b, lq, h, hd).transpose(1, 2)
            kvh = kv.view(b, lk, 2, h, hd)
            att = torch.softmax((qh @ kvh[:, :, 0].permute(0, 2, 3, 1)) * (1.0 / math.sqrt(hd)), dim=-1)
            o = (att @ kvh[:, :, 1].transpose(1, 2)).transpose(1, 2).reshape(b, lq, d)
        if defer_out_proj:
            return o                     # relu(out_proj(.)) is computed by the head-input launch (ops.OutProjHeadInputs)
        if relu_owed:
            # the head-input kernel (the one consumer of this output) takes the ReLU backward and the bias gradient
            return ops.LinearReluOwed.apply(o.reshape(-1, d), mha.out_proj.weight, mha.out_proj.bias, bf).view(b, lq, d)
        return ops.linear(o, mha.out_proj.weight, mha.out_proj.bias, relu=True, bf16=bf)   # F.relu(...) of :242, fused

    # ---- forward ---------------------------------------------------------------------------------
    def forward(self, data, temperature=None, device=None, isExplain=False):
        """:207-307.  Returns (log_softmax, x_hat, out_z, out_lin, linear_outf, our_reg)."""
        return self._forward_grouped(data, temperature, device, (bool(isExplain),))[0]

    def forward_pair(self, data, temperature=None, device=None):
        """The two forward passes of one train step (train() :521,523: plain, then isExplain=True) as ONE batched
        sweep over 2B samples / a 2-copy block-diagonal graph.  Numerically the same two passes: every sample is
        independent except through BatchNorm, whose batch statistics are taken per pass (``groups=2``) and whose
        running statistics are updated plain-then-masked.  Halves the launch count of a step and lets autograd
        produce every parameter gradient once instead of adding two per-pass contributions."""
        return self._forward_grouped(data, temperature, device, (False, True))

    def _check_config(self, masked):
        """Raises for a configuration a subclass's forward cannot run (SGCN_GCN_CLUSTERLABEL); nothing to refuse here."""

    def attention_weights(self, data, temperature=None, device=None, isExplain=False):
        """The second output of ``self.multihead_attn(batch_x, atten_out, atten_out)`` (:240), which the reference's
        forward discards: the head-averaged cross-attention weights [B, rois, Ntop] (fp32) — how strongly every brain
        region attends to every top-level GO term.  The image branch and the GO network run as in ``forward`` — in eval
        mode under ``torch.no_grad()``: BatchNorm on its running statistics, no dropout — up to the packed input
        projection (at the forward's projection precision); ops.attention_weights then forms the probabilities the
        attention cores never do.  The model is left as it was: ``training``, parameters, buffers, random state; the
        hand-over to ``loss_probability`` and ``last_edge_prob`` are reset as after an evaluation sweep."""
        return self._attention_pass("attention_weights", data, temperature, device, isExplain, lambda w, snps_in: w)

    def snp_association(self, data, temperature=None, device=None, isExplain=False):
        """The ROI x SNP association map of every subject, [B, rois, 54] (fp32, non-negative, rows summing to at most
        1): ``attention_weights`` — region to top-level GO term — times the attention roll-out of the GO encoder from
        those terms down to the SNPs (``Gene_ontology_network.attention_rollout``: go_model.py:208-251, the per-sample
        edge attention and self-importance of both encoder layers and the learnable SNP -> GO encoding).  Same pass, same
        contract as ``attention_weights`` (eval mode, no_grad, the model left as it was); the product is one launch of
        the library's exact-fp32 batched GEMM (ops.snp_association)."""
        return self._snp_association(data, temperature, device, isExplain)[0]

    def edge_importance(self, data, weighted=False, return_count=False):
        """``edge_importance`` (this module) of a batch: the dense [B, rois, rois] form of ``cal_probability``'s edge mask."""
        return edge_importance(self, data, weighted, return_count)

    def gat_attention(self, data, isExplain=False):
        raise ValueError(f"gat_attention: {self.__class__.__name__} has GCNConv layers (no attention coefficients)")

    def input_saliency(self, data, temperature=None, device=None, target=None, isExplain=False, inputs="image",
                       normalize=False):
        """Gradient x input of every subject — which regions, in which imaging modality, drive its class: what
        ``data.x.requires_grad = True`` (:210-211) is there for.  One eval-mode forward and one backward of the target
        class's log-probability (first output; a one-hot cotangent serves the whole batch).  Returns a dict: ``attr``
        [B, rois, H0] = x * d score / d x, ``roi`` [B, rois] = sum_h |attr|, ``target`` [B] (int64) and, with ``inputs``
        "snps" or "both", ``snps`` [B, 54] = snps_feat * d score / d snps_feat.  ``target``: None (the predicted class,
        taken on the device), an int, or an int64 tensor [B] (``data.y``).  ``normalize``: every subject divided by its
        largest ``roi`` (``snps``: by its largest entry's magnitude).  The model is left as it was (``saliency``
        module); no parameter gradient is formed."""
        from . import saliency
        return saliency.input_saliency(self, data, temperature, device, target, isExplain, inputs, normalize)

    def integrated_gradients(self, data, temperature=None, device=None, target=None, isExplain=False, inputs="image",
                             normalize=False, steps=16, baseline=None):
        """Integrated gradients by the midpoint rule, alpha_m = (m + 1/2) / steps, from ``baseline`` (None: zeros,
        [rois, H0] or [B * rois, H0]) to ``data.x``; with ``inputs`` "snps" / "both" the SNP vector moves from zero by
        the same alpha ("snps": the SNP vector alone — no ``attr`` / ``roi``).  The dict of ``input_saliency`` plus
        ``delta`` [B] = sum attr (+ sum snps) - (score(x) - score(baseline)), the quadrature gap (of the un-normalised
        attributions; returned, never gated).  ``target=None`` is the prediction at the unscaled input.  ``steps``
        forward / backward passes run one after another on the batch's one plan and igcn_saliency_maps reduces their
        stacked gradients."""
        from . import saliency
        return saliency.integrated_gradients(self, data, temperature, device, target, isExplain, inputs, normalize,
                                             steps, baseline)

    def grad_cam(self, data, target=None, isExplain=False, normalize=True):
        from . import saliency
        return saliency.grad_cam(self, data, target, isExplain, normalize)     # (raises: SGCN_Ori's taps only)

    def _snp_association(self, data, temperature=None, device=None, isExplain=False):
        """(assoc [B, rois, 54], r_top [B, Ntop, 54]) of one batch: ``snp_association`` with the roll-out it used."""
        def tail(w, snps_in):
            r_top = self.go_network.attention_rollout(snps_in, temperature, device)
            return ops.snp_association(w, r_top), r_top
        return self._attention_pass("snp_association", data, temperature, device, isExplain, tail)

    def _attention_pass(self, name, data, temperature, device, isExplain, tail):
        """The pass ``attention_weights`` and ``snp_association`` share: refuse a model without cross-attention, run
        the image branch, the GO network and the in-projection in eval mode under no_grad, form the weights w, return
        ``tail(w, snps_in)`` (``snps_in``: the SNP features the GO network saw) and restore the model."""
        if not self.isCrossAtten or self.isImageOnly or self.isSNPsOnly:
            raise ValueError(f"{name}: the model has no cross-attention (needs isCrossAtten=True, "
                             "isImageOnly=False, isSNPsOnly=False)")
        flags = (bool(isExplain),)
        self._check_config(any(flags))
        x = data.x
        if x.shape[0] % self.rois:
            raise ValueError(f"every graph must have exactly rois={self.rois} nodes (got {x.shape[0]} nodes)")
        was = self.training
        self.eval()
        try:
            with torch.no_grad():
                plan = ops.plan_for(data, keep_pending=True)
                route, fan = self._image_route(data, plan, flags)
                img = route(data, plan, flags, fan)
                batch_x = img.xcat.view(x.shape[0] // self.rois, self.rois, -1)
                atten_out = self.go_network(img.snps_in, temperature, device, groups=1, extra_dropout=[])[3]
                mha = self.multihead_attn
                q, kv = ops.InProj.apply(batch_x, atten_out, mha.in_proj_weight, mha.in_proj_bias, self.bf16_transforms)
                return tail(ops.attention_weights(q.contiguous(), kv.contiguous(), mha.num_heads), img.snps_in)
        finally:
            self.last_edge_prob, self._handoff = None, _Handoff()     # no later loss_probability is served from this batch
            self.train(was)

    def predraw_dropout(self, data, groups=2):
        """The dropout masks of the next training sweep over ``data`` (``groups`` passes batched: the train step's plain |
        masked pair), drawn as a RIDER of the launch that follows on this stream — a captured step queues them in front
        of its per-graph plan build (train.GraphedTrainStep), whose grid then carries the mask generation."""
        if not (self.training and self._dropout_enabled) or not data.x.is_cuda:
            return
        gb = groups * (data.x.shape[0] // self.rois)
        self.go_network.predraw_dropout(gb, data.x.device, self._head_dropout(gb), groups)

    def _head_dropout(self, rows):
        """[(shape, p), ...]: the two heads' dropout sites (:300, :303) for a sweep of ``rows`` samples, drawn by the GO
        network's mask launch (``extra_dropout``)."""
        hl = self.lin1.weight.shape[0]
        return [((rows, hl), 0.5), ((rows, hl), 0.3)]

    def _forward_grouped(self, data, temperature, device, explain_flags, split=True, raw_scores=False, on_out_z=None,
                         heads_to_loss=False):
        """``on_out_z(out_z)``: called once the fused features exist and BEFORE the heads' first layers are launched — a
        train step queues the Gram products of its batch losses there, as riders of that launch (ops.gram_rider).
        ``heads_to_loss`` (with ``split=False``): where ops.HeadLoss covers the output layers, lin2 / lin2_regr are NOT
        applied here — the first output is the tuple ("heads", features, factors, features_regr, factors_regr) and the
        last None: the caller's loss launch runs them (train._losses_batched)."""
        x = data.x
        x.requires_grad = True                                        # :210 — populates data.x.grad
        self.input = x
        n = x.shape[0]
        if n % self.rois:
            raise ValueError(f"every graph must have exactly rois={self.rois} nodes (got {n} nodes)")
        flags = tuple(explain_flags)
        bsz, g = n // self.rois, len(flags)
        plan = ops.plan_for(data, keep_pending=True)
        self.last_edge_prob, self._handoff = None, _Handoff()     # (nothing of the last forward outlives this one)
        route, fan = self._image_route(data, plan, flags)
        img = route(data, plan, flags, fan)
        self.last_edge_prob = img.edge_prob
        self._handoff = _Handoff(self._reg_key(x, data.edge_attr),
                                 None if img.reg is None else tuple(float(v) for v in self._reg_hp), img.reg, img.fan)
        batch_x = img.xcat.view(g * bsz, self.rois, -1)               # to_dense_batch == view (:226)
        if self.graph_pool:                                           # :230-235 mean | max | add over a graph's nodes
            img_out = ops.GraphPool.apply(img.xcat, self.rois)
        else:
            img_out = (img.xcat if img.xcat_img is None else img.xcat_img).view(g * bsz, -1)
        head_drop = self._head_dropout(g * bsz) if (self.training and self._dropout_enabled) else []
        latent, x_hat, _, atten_out = self.go_network(img.snps_in, temperature, device, groups=g, extra_dropout=head_drop)
        out_z, out_lin, feat = self._fusion(data, img, img_out, batch_x, latent, atten_out, bsz, g)
        if on_out_z is not None:
            on_out_z(out_z)
        return self._heads(x_hat, out_z, out_lin, feat, bool(head_drop), bsz, g, split, raw_scores, heads_to_loss)

    # ---- image routes ----------------------------------------------------------------------------
    @property
    def _gcn_convs(self):
        return [self.conv1, *self.convs]

    @property
    def _dual_consumer(self):
        """xcat feeds the attention query AND the image head input: two handles of it, one gradient sum in the backward."""
        return self.isCrossAtten and not self.graph_pool and not self.isImageOnly and not self.isSNPsOnly

    def _image_route(self, data, plan, flags):
        """(route, fan): the ``_*_route`` method that runs this forward's image branch, and whether ops.GradFan hands
        out gradient aliases (prob, data.x and snps_prob have several consumers: one summed gradient each).  Readies the
        plan for the route on the way: the dense-block kernels take a pending structure check, and the one-launch front
        a pending build, inside their own launches; for every other route they are launched here."""
        x, snps_feat, convs = data.x, data.snps_feat, self._gcn_convs
        fan = x.is_cuda and torch.is_grad_enabled() and not switches.on("IGCN_NO_GRAD_FAN")
        mode = _MODES.get(flags)
        snps_fit = snps_feat is not None and snps_feat.dim() == 2 and snps_feat.shape[1] == self.snps_prob.numel()
        snps_ok = snps_fit and snps_feat.is_cuda
        if (mode is not None and x.is_cuda and (snps_ok or mode == "plain")
                and not switches.on("IGCN_NO_DENSE_BLOCKS")
                and ops.dense_sgcn_supported(plan, self.rois, x.shape[1], convs[0].out_channels, len(convs))):
            plan.flush_pending_build()
            return self._dense_route, fan
        plan.flush_pending_check()
        if getattr(plan, "dense_blocks", False) and x.is_cuda:
            ops.call("igcn_rider_flush", ops.stream_ptr())        # (a dropout rider the step queued for ops.DenseSgcn)
        pair = flags == (False, True) and x.is_cuda
        reg_in_mask = fan and self._reg_hp is not None and not switches.on("IGCN_NO_MASK_REG_FUSED")
        if (pair and snps_ok and reg_in_mask and self.fused_sgcn_stack and not self.bf16_transforms
                and ops.sgcn_front_supported(plan, self.rois, x.shape[1], _grid_width(convs[0].out_channels),
                                             len(convs), snps_feat, self.snps_prob)):
            return self._front_route, fan
        plan.flush_pending_build()
        if pair and snps_fit:
            return (self._stacked_reg_route if reg_in_mask else self._stacked_route), fan
        return self._generic_route, fan

    def _dense_route(self, data, plan, flags, fan):
        """Complete graphs (a dense adjacency as COO): masks, gcn_norm, every GCNConv and the mask regulariser of the
        pass(es) on the dense blocks — no plan arrays, no per-edge intermediates (ops.DenseSgcn)."""
        x, snps_feat, mode = data.x, data.snps_feat, _MODES[flags]
        wb = [t for c in self._gcn_convs for t in (c.lin.weight, c.bias)]
        prob_d, sp_d, sp_m, x_d = self.prob, self.snps_prob, self.snps_prob, x
        prob_h, x_h = self.prob, x
        if fan and mode != "plain":
            # prob (dense path: mask + regulariser; head inputs), snps_prob (regulariser; SNP mask) and data.x (dense
            # path; head inputs) have two consumers each: their gradients meet in ONE sum per tensor (ops.GradFan —
            # a deferred final reduction for these leaves) instead of a library add each
            prob_d, prob_h = ops.GradFan.apply(self.prob, 2)
            sp_d, sp_m = ops.GradFan.apply(self.snps_prob, 2)
            x_d, x_h = ops.GradFan.apply(x, 2)
        dual = fan and self._dual_consumer
        xcat, regp, *xcat_img = ops.DenseSgcn.apply(x_d, data.edge_attr, prob_d, self.prob_bias, sp_d, mode,
                                                    -self.rois if dual else self.rois, self._reg_hp, plan, *wb)
        snps_in = snps_feat if mode == "plain" else ops.SnpsMask.apply(snps_feat, sp_m, mode == "both")[0]
        return _ImageBranch(xcat, xcat_img[0] if dual else None, snps_in, prob_h, x_h,
                            reg=None if mode == "plain" else regp)

    def _front_route(self, data, plan, flags, fan):
        """The train step's (plain | masked) pair on small uniform graphs: plan build, masks, regulariser, SNP mask and
        the GCNConv stack of both passes as ONE launch (ops.SgcnFront)."""
        return self._stacked_reg_route(data, plan, flags, fan, front=True)

    def _stacked_reg_route(self, data, plan, flags, fan, front=False):
        """The train step's (plain | masked) pair with loss_probability AND the SNP mask riding in the mask launch
        (ops.EdgeMaskStacked with reg_hp / snps_feat; ``front``: ops.SgcnFront, which also builds the plan and runs the
        stack): prob then has two consumers (that launch; the head inputs), data.x likewise, snps_prob one."""
        prob_m, prob_h = ops.GradFan.apply(self.prob, 2)
        x_m, x_h = ops.GradFan.apply(data.x, 2)
        mask = (x_m, prob_m, self.prob_bias, data.edge_attr, plan, self.rois, self.snps_prob, self._reg_hp,
                data.snps_feat)
        if front:
            f, fp, wb = _padded_params(self._gcn_convs)
            xcat, xcat_img, e, regp, snps_in = ops.SgcnFront.apply(*mask, data.edge_index, *wb)
            xcat, xcat_img = _unpad(xcat, f, fp), (xcat_img if self._dual_consumer and fp == f else None)
        else:
            x_in, ew_in, e, regp, snps_in = ops.EdgeMaskStacked.apply(*mask)
            xcat, xcat_img = self._stack(x_in, ew_in, plan, len(flags), fan)
        # (the plain half of the stacked SNP batch is data: its gradient is never read — ops.SparseMap skips it)
        bsz = data.x.shape[0] // self.rois
        snps_in._igcn_grad_rows = (bsz, 2 * bsz)
        return _ImageBranch(xcat, xcat_img, snps_in, prob_h, x_h, e, regp)

    def _stacked_route(self, data, plan, flags, fan):
        """The train step's (plain | masked) pair, loss_probability left to the loss: the mask launch writes both halves
        of the stacked batch itself, the SNP mask is a launch of its own.  prob (mask, head inputs, regulariser), data.x
        (mask, head inputs) and snps_prob (mask, regulariser) each feed several ops: ops.GradFan hands out aliases and
        sums their gradients in one launch per tensor."""
        prob_m = prob_h = self.prob
        x_m = x_h = data.x
        sp_m, reg_fan = self.snps_prob, None
        if fan:
            prob_m, prob_h, prob_r = ops.GradFan.apply(self.prob, 3)
            x_m, x_h = ops.GradFan.apply(data.x, 2)
            sp_m, sp_r = ops.GradFan.apply(self.snps_prob, 2)
            reg_fan = (prob_r, sp_r)
        x_in, ew_in, snps_in, e = masked_inputs(self, data, plan, flags, True, data.snps_feat, (x_m, prob_m, sp_m))
        return _ImageBranch(*self._stack(x_in, ew_in, plan, len(flags), fan), snps_in, prob_h, x_h, e, fan=reg_fan)

    def _generic_route(self, data, plan, flags, fan):
        """Any other sweep: cal_probability for a masked pass, the passes' inputs concatenated."""
        x_in, ew_in, snps_in, e = masked_inputs(self, data, plan, flags, False, data.snps_feat)
        return _ImageBranch(*self._stack(x_in, ew_in, plan, len(flags), fan), snps_in, self.prob, data.x, e)

    def _stack(self, x_in, ew_in, plan, g, fan):
        """sgcn_stack on the plan of ``g`` copies of the batch -> (xcat, its handle for the image head input or None)."""
        dual = fan and self._dual_consumer
        out = sgcn_stack(self._gcn_convs, x_in, ew_in, plan.replicate(g), self.rois, self.fused_sgcn_stack,
                         self.bf16_transforms, dual=dual)
        return out if dual else (out, None)

    # ---- fusion and heads ------------------------------------------------------------------------
    def _fusion(self, data, img, img_out, batch_x, latent, atten_out, bsz, g):
        """The image and SNP features fused into the heads' inputs (:236-297) -> (out_z, out_lin, feat)."""
        use_prob = self.isuseProb4Regr and not self.isImageOnly and not self.isSNPsOnly
        x_flat, prob_flat = (img.x_h.view(bsz, -1), img.prob_h.view(-1)) if use_prob else (None, None)
        owed = fuse_proj = False
        if self.isCrossAtten:
            # out_cross has one consumer, the head-input launch, when nothing else reads it: that launch then also takes
            # relu(out_proj)'s mask and bias gradient (ops.LinearReluOwed)
            owed = (self._dual_consumer and torch.is_grad_enabled()
                    and self.multihead_attn.out_proj.bias is not None
                    and ops.relu_owed_supported(self.multihead_attn.embed_dim, img_out.shape[1])
                    and img_out.shape[1] == batch_x.shape[1] * self.multihead_attn.embed_dim
                    and ops.head_inputs_supported(img_out, img_out, latent, x_flat, prob_flat))
            fuse_proj = owed and ops.outproj_head_inputs_supported(self.multihead_attn.embed_dim, img_out.shape[1])
            out_cross = self._cross_attention(batch_x, atten_out, relu_owed=owed, defer_out_proj=fuse_proj)
            if self.graph_pool:                                       # :246-252
                out_cross = ops.GraphPool.apply(out_cross.reshape(g * bsz * self.rois, -1), self.rois)
            else:
                out_cross = out_cross.reshape(g * bsz, -1)
        else:
            out_cross = torch.cat((img_out, latent), -1)
        if self.isImageOnly:
            out_z = out_lin = img_out
        elif self.isSNPsOnly:
            out_z, out_lin = latent, torch.cat((img.snps_in, latent), -1)
        elif ops.head_inputs_supported(img_out, out_cross, latent, x_flat, prob_flat):       # :284-297 in one launch
            if fuse_proj:                                             # out_cross is still the attention output here
                op = self.multihead_attn.out_proj
                out_z, out_lin, feat, _ = ops.OutProjHeadInputs.apply(out_cross, op.weight, op.bias, img_out, latent,
                                                                      x_flat, prob_flat, bsz, self.bf16_transforms)
            else:
                out_z, out_lin, feat = ops.HeadInputs.apply(img_out, out_cross, latent, x_flat, prob_flat, bsz,
                                                            self.multihead_attn.out_proj.bias if owed else None)
            return out_z, out_lin, (feat if use_prob else out_lin)
        else:
            out_z = (img_out + out_cross) / 2
            out_lin = torch.cat((out_z, latent), -1)
        if self.isuseProb4Regr and not self.isSNPsOnly:
            img_feat = (data.x.view(bsz, self.rois, -1) * self.prob).reshape(bsz, -1)      # :293-297
            return out_z, out_lin, torch.cat((out_lin, img_feat if g == 1 else img_feat.repeat(g, 1)), -1)
        return out_z, out_lin, out_lin

    def _heads(self, x_hat, out_z, out_lin, feat, head_drop, bsz, g, split, raw_scores, heads_to_loss):
        """lin1 | lin1_regr (:299, :302), then lin2 | lin2_regr (:289-290, :300-301) — or, with ``heads_to_loss``, the
        features and dropout masks the loss launch applies the output layers to."""
        keep1, keep2 = self.go_network.extra_masks if head_drop and self.go_network.extra_masks[0] is not None \
            else (None, None)
        # the first layers of the two heads are independent: one grouped launch each way
        hin1, hin2 = out_lin, feat
        self._cut = None
        if getattr(self, "_cut_heads", False) and torch.is_grad_enabled() and out_lin.requires_grad:
            # two-bucket gradient exchange (train.backward_two_buckets): the heads take DETACHED copies of their inputs, so
            # that a first backward sweep ends at them (the heads' parameter gradients — 4/5 of the bucket — are complete
            # and on the wire while the second sweep runs through the rest of the model)
            hin1 = out_lin.detach().requires_grad_(True)
            hin2 = hin1 if feat is out_lin else feat.detach().requires_grad_(True)
            self._cut = [(out_lin, hin1)] + ([] if feat is out_lin else [(feat, hin2)])
        linear_outf, reg = ops.linear_pair(hin1, self.lin1.weight, self.lin1.bias, hin2, self.lin1_regr.weight,
                                           self.lin1_regr.bias, relu=True, bf16=self.bf16_transforms)
        if (heads_to_loss and not split and not (head_drop and keep1 is None)
                and ops.head_loss_supported(linear_outf, self.lin2.weight, reg, self.lin2_regr.weight, keep1, keep2)):
            return (("heads", linear_outf, keep1, reg, keep2), x_hat, out_z, out_lin, linear_outf, None)
        if head_drop and keep1 is None:               # the GO network's own dropout is switched off: library masks
            logits = ops.linear(self._drop(linear_outf, 0.5), self.lin2.weight, self.lin2.bias)
            our_reg = ops.linear(self._drop(reg, 0.3), self.lin2_regr.weight, self.lin2_regr.bias)
        else:                                         # (one launch for both)
            logits, our_reg = ops.small_linear_pair(linear_outf, self.lin2.weight, self.lin2.bias, keep1,
                                                    reg, self.lin2_regr.weight, self.lin2_regr.bias, keep2)
        # raw_scores: the caller takes log_softmax itself (ops.LossHead does it inside the loss kernel)
        outs = (logits if raw_scores else F.log_softmax(logits, dim=-1), x_hat, out_z, out_lin, linear_outf, our_reg)
        if not split:
            return outs                                               # stacked [g*B, ...] (pass-major)
        if g == 1:
            return [outs]
        return [tuple(t[k * bsz:(k + 1) * bsz] for t in outs) for k in range(g)]

    def head_parameters(self):
        """The parameters of the two MLP heads (:284-305) — consecutive in ``parameters()``, 4/5 of the model's weights,
        and the first whose gradients a backward pass completes: the early bucket of the two-bucket gradient exchange."""
        return [p for m in (self.lin1, self.lin1_regr, self.lin2, self.lin2_regr) for p in m.parameters()]

    def __repr__(self):
        return self.__class__.__name__
