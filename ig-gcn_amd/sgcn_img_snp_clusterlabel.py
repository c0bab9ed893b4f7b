"""Drop-in ``SGCN_GCN_CLUSTERLABEL`` on the HIP kernels: the cluster-label model of
kernel/sgcn_img_snp_clusterlabel.py:13-231, trained by kernel/train_eval_sgcn_clusterlabel.py:365-447.

Interface of the reference: constructor (:15), ``forward(data, temperature, device, isExplain=False)`` and its 4-tuple
(log_softmax classify, log_softmax cluster, x_hat, out_z) (:157-228), ``cal_probability`` (:94), ``loss_probability``
(:114, whose L1 terms are normalised differently from the headline model's), ``consist_loss`` (:146), the ``input`` /
``data.x.grad`` side effects and an identical ``state_dict()`` key set (``batch_norm``, ``edge_prob`` and the literal 90
in the ``lin1_*`` widths included).

What runs: everything up to the fusion is ``SGCN_GCN_IMGSNP``'s (masks, LDS-resident GCN stack, GO network,
cross-attention, the head-input launch — the reference's ``out_z`` here is that model's ``out_lin``).  Behind it the two
first layers are one ``ops.linear_pair`` launch; inside a train step the two output layers, both log-softmaxes, the four
cross-entropy terms, the reconstruction term and the backward of all of it are ONE launch (``ops.ClusterHeadLoss``,
csrc/cluster.hip); anywhere else (eval, IGCN_NO_HEAD_LOSS_FUSED=1, shapes the launch refuses) ``ops.small_linear_pair`` +
``log_softmax``.  ``train.losses`` takes the six-term loss of the cluster trainer for this model.

Limits (ValueError from ``forward``, as the reference cannot run them either): ``isCrossAtten=False`` (:194,208 add
tensors of width W and W + l_dim), ``rois != 90`` (:46,50 size the heads for 90 ROIs) and ``num_features != H_0`` with a
masked pass (:98,103 multiply x by prob [rois, H_0] and project 2 D columns with prob_bias [2 H_0, 1]).
"""
import torch
import torch.nn.functional as F
from torch.nn import Linear

from . import ops, switches
from .sgcn_img_snp import GCNConv, SGCN_GCN_IMGSNP, _Handoff, _ImageBranch, _grid_width, _padded_params, _unpad


class SGCN_GCN_CLUSTERLABEL(SGCN_GCN_IMGSNP):
    clusterlabel = True      # train.losses: kernel/train_eval_sgcn_clusterlabel.py's loss; train.Evaluator refuses the model

    def __init__(self, num_layers, hidden, A_g, A, pool_dim, l_dim, device, *args, hidden_linear=64, rois=90, H_0=1,
                 num_features=1, num_classes=3, num_cluster=2, isCrossAtten=False, isPredictCluster=True, **kwargs):
        super().__init__(num_layers, hidden, A_g, A, pool_dim, l_dim, device, hidden_linear=hidden_linear, rois=rois,
                         H_0=H_0, num_classes=num_classes, isCrossAtten=isCrossAtten, isSoftSimilarity=False,
                         isImageOnly=False, isSNPsOnly=False, **kwargs)
        # the headline's heads make way for the two classification heads (:46-52: 90 ROIs, whatever ``rois`` says)
        del self.lin1, self.lin1_regr, self.lin2, self.lin2_regr, self.batch_norm_1d
        self.num_features, self.num_classes, self.num_cluster = num_features, num_classes, num_cluster
        self.isPredictCluster = isPredictCluster
        self.final_conv_acts = None
        self.final_conv_grads = None
        if num_features != H_0:
            self.conv1 = GCNConv(num_features, hidden)
        d_in = 90 * num_layers * hidden + l_dim
        self.lin1_classify = Linear(d_in, hidden_linear)
        self.lin2_classify = Linear(hidden_linear, num_classes)
        self.lin1_cluster = Linear(d_in, hidden_linear)
        self.lin2_cluster = Linear(hidden_linear, num_cluster)

    def reset_parameters(self):
        self.conv1.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        for m in (self.lin1_classify, self.lin2_classify, self.lin1_cluster, self.lin2_cluster):
            m.reset_parameters()
        with torch.no_grad():
            for p in (self.prob_bias, self.prob, self.edge_prob, self.snps_prob):
                torch.nn.init.kaiming_uniform_(p, a=5 ** 0.5)

    def activations_hook(self, grad):
        self.final_conv_grads = grad

    def head_parameters(self):
        return [p for m in (self.lin1_classify, self.lin2_classify, self.lin1_cluster, self.lin2_cluster)
                for p in m.parameters()]

    # ---- what the reference cannot run -----------------------------------------------------------
    def _check_config(self, masked):
        if not self.isCrossAtten:
            raise ValueError("SGCN_GCN_CLUSTERLABEL: isCrossAtten=False cannot run — the reference's forward adds img_out "
                             "[B, W] to cat(img_out, latent) [B, W + l_dim] (kernel/sgcn_img_snp_clusterlabel.py:194,208)")
        if self.rois != 90:
            raise ValueError(f"SGCN_GCN_CLUSTERLABEL: rois must be 90 (got {self.rois}) — lin1_classify / lin1_cluster are "
                             "sized for 90 ROIs whatever ``rois`` says (kernel/sgcn_img_snp_clusterlabel.py:46,50)")
        if masked and self.num_features != self.prob_dim:
            raise ValueError(f"SGCN_GCN_CLUSTERLABEL: a masked pass needs num_features == H_0 (got {self.num_features} and "
                             f"{self.prob_dim}) — cal_probability projects 2 * num_features columns with prob_bias "
                             "[2 * H_0, 1] (kernel/sgcn_img_snp_clusterlabel.py:102-103)")

    # ---- regulariser -----------------------------------------------------------------------------
    def loss_probability(self, x, edge_index, edge_weight, hp, eps=1e-6, plan=None, edge_prob=None, partials=False):
        """:114-144 as one fused reduction (igcn_mask_reg3_*): the edge term and the three entropy terms are means, as the
        headline model's; ``f_sum_loss`` is the sum over prob divided by its ROWS (the mean times H_0) and
        ``snps_sum_loss`` the sum over snps_prob divided by ONE row (the mean times 54).  ``edge_prob`` lets the train
        step reuse the mask the explain pass wrote; the regulariser a forward of this class may have reduced along the
        way carries the headline model's normalisation and is never used."""
        h = self._handoff
        self._handoff = _Handoff(h.key)                               # (gradient aliases are handed out once)
        key = self._reg_key(x, edge_weight)
        same = key[:4] == h.key[:4]
        if edge_prob is not None and edge_prob is self.last_edge_prob and not same:
            edge_prob = None                                          # the mask of another batch: do not reuse it
        if edge_prob is None:
            _, _, _, edge_prob = self.cal_probability(x, edge_index, edge_weight, plan=plan)
        prob, sprob = (h.fan if same and h.fan else None) or (self.prob, self.snps_prob)
        l1 = float(hp.lamda_x_l1)
        return ops.MaskRegulariser3.apply(prob, edge_prob, sprob, l1 * self.prob.shape[1], hp.lamda_x_ent, hp.lamda_e_l1,
                                          hp.lamda_e_ent, l1 * self.snps_prob.shape[1], hp.lamda_x_ent, eps, partials)

    def consist_loss(self, s, tsne_result=None):
        """:146-155 (all-ones similarity)."""
        if len(s) == 0:
            return 0
        return self.batch_losses(s, self.laplacian(s.shape[0], None))[0]

    # ---- forward ---------------------------------------------------------------------------------
    def forward(self, data, temperature=None, device=None, isExplain=False):
        """:157-228.  Returns (log_softmax classify, log_softmax cluster, x_hat, out_z)."""
        return self._forward_grouped(data, temperature, device, (bool(isExplain),))[0]

    def _forward_grouped(self, data, temperature, device, explain_flags, **kw):
        self._check_config(any(explain_flags))
        return super()._forward_grouped(data, temperature, device, explain_flags, **kw)

    def _head_dropout(self, rows):
        """Both heads drop at p = 0.5 (:221,225)."""
        hl = self.lin1_classify.weight.shape[0]
        return [((rows, hl), 0.5), ((rows, hl), 0.5)]

    def _image_route(self, data, plan, flags):
        """SGCN_GCN_IMGSNP's choice without the dense-block route, which never materialises the edge mask this model's
        regulariser reads."""
        x, snps_feat, convs = data.x, data.snps_feat, self._gcn_convs
        fan = x.is_cuda and torch.is_grad_enabled() and not switches.on("IGCN_NO_GRAD_FAN")
        snps_fit = snps_feat is not None and snps_feat.dim() == 2 and snps_feat.shape[1] == self.snps_prob.numel()
        plan.flush_pending_check()
        if getattr(plan, "dense_blocks", False) and x.is_cuda:
            ops.call("igcn_rider_flush", ops.stream_ptr())
        pair = flags == (False, True) and x.is_cuda
        reg_in_mask = fan and not switches.on("IGCN_NO_MASK_REG_FUSED")
        if (pair and snps_fit and snps_feat.is_cuda and reg_in_mask and self.fused_sgcn_stack and not self.bf16_transforms
                and ops.sgcn_front_supported(plan, self.rois, x.shape[1], _grid_width(convs[0].out_channels),
                                             len(convs), snps_feat, self.snps_prob)):
            return self._front_route, fan
        plan.flush_pending_build()
        if pair and snps_fit:
            return (self._stacked_reg_route if reg_in_mask else self._stacked_route), fan
        return self._generic_route, fan

    def _stacked_reg_route(self, data, plan, flags, fan, front=False):
        """SGCN_GCN_IMGSNP's stacked (plain | masked) launch — the plan build, the masks, the SNP mask and, ``front``, the
        GCNConv stack.  The regulariser that launch reduces has the headline's weights: its partials are dropped, and
        loss_probability reads the edge mask the launch wrote through gradient aliases of prob / snps_prob handed out
        here (three consumers of prob: this launch, the head inputs, the regulariser; two of snps_prob)."""
        prob_m, prob_h, prob_r = ops.GradFan.apply(self.prob, 3)
        sp_m, sp_r = ops.GradFan.apply(self.snps_prob, 2)
        x_m, x_h = ops.GradFan.apply(data.x, 2)
        mask = (x_m, prob_m, self.prob_bias, data.edge_attr, plan, self.rois, sp_m, self._reg_hp, data.snps_feat)
        if front:
            f, fp, wb = _padded_params(self._gcn_convs)
            xcat, xcat_img, e, _, snps_in = ops.SgcnFront.apply(*mask, data.edge_index, *wb)
            xcat, xcat_img = _unpad(xcat, f, fp), (xcat_img if self._dual_consumer and fp == f else None)
        else:
            x_in, ew_in, e, _, snps_in = ops.EdgeMaskStacked.apply(*mask)
            xcat, xcat_img = self._stack(x_in, ew_in, plan, len(flags), fan)
        bsz = data.x.shape[0] // self.rois
        snps_in._igcn_grad_rows = (bsz, 2 * bsz)
        return _ImageBranch(xcat, xcat_img, snps_in, prob_h, x_h, e, None, (prob_r, sp_r))

    def _heads(self, x_hat, out_z, out_lin, feat, head_drop, bsz, g, split, raw_scores, heads_to_loss):
        """lin1_classify | lin1_cluster as one launch (:218,224), then lin2_classify | lin2_cluster and the two
        log-softmaxes (:222-228) — or, with ``heads_to_loss``, the features and dropout factors the fused loss launch
        applies the output layers to.  The reference's ``out_z`` is ``out_lin`` of the shared fusion."""
        go = self.go_network
        keep1, keep2 = go.extra_masks if head_drop and go.extra_masks[0] is not None else (None, None)
        # isPredictCluster=False: the cluster head sees zeros (:220)
        hin2 = out_lin if self.isPredictCluster else torch.zeros_like(out_lin)
        self._cut = None
        f1, f2 = ops.linear_pair(out_lin, self.lin1_classify.weight, self.lin1_classify.bias, hin2,
                                 self.lin1_cluster.weight, self.lin1_cluster.bias, relu=True, bf16=self.bf16_transforms)
        w1, b1, w2, b2 = (self.lin2_classify.weight, self.lin2_classify.bias, self.lin2_cluster.weight,
                          self.lin2_cluster.bias)
        if (heads_to_loss and not split and g == 2 and not (head_drop and keep1 is None)
                and ops.cluster_head_loss_supported(f1, w1, f2, w2, keep1, keep2)):
            return (("heads", f1, keep1, f2, keep2), None, x_hat, out_lin)
        if head_drop and keep1 is None:               # the GO network's own dropout is switched off: library masks
            s1 = ops.linear(self._drop(f1, 0.5), w1, b1)
            s2 = ops.linear(self._drop(f2, 0.5), w2, b2)
        else:                                         # (one launch for both)
            s1, s2 = ops.small_linear_pair(f1, w1, b1, keep1, f2, w2, b2, keep2)
        outs = (F.log_softmax(s1, dim=-1), F.log_softmax(s2, dim=-1), x_hat, out_lin)
        if not split:
            return outs                                               # stacked [g*B, ...] (pass-major)
        if g == 1:
            return [outs]
        return [tuple(t[k * bsz:(k + 1) * bsz] for t in outs) for k in range(g)]
