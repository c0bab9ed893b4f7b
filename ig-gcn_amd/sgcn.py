"""Drop-ins for the image-only models of the reference's kernel/sgcn.py: ``SGCN_GCN`` (:272-388), its attention twin
``SGCN_GAT`` (:154-270) and the original ``SGCN_Ori`` (:11-151), the one model that fills the Grad-CAM surface.

``SGCN_GCN`` — the image-only sibling of the hot path on the same kernels: masks (igcn_edge_mask_*), one gcn_norm per
pass, MFMA feature transforms, scatter-aggregate, the (R*D -> hidden_linear -> classes) head on the split-K GEMM, and
the mask regulariser as one reduction.

Same constructor signature (``dataset`` is accepted and ignored exactly as in the reference), the same
``forward(data, isExplain=False) -> log_softmax [B, C]``, ``cal_probability`` (:321), ``loss_probability``
(:334; note the node-mask L1 term is divided by ``rois`` here, not by ``rois*H_0`` as in
kernel/sgcn_img_snp.py:160) and the same ``state_dict()`` keys.  ``lin1`` takes ``rois * num_layers * hidden``
inputs (the reference hard-codes 90 at :285, i.e. it only works for rois=90; identical there).

``forward_pair`` runs the plain and the masked pass of train() (kernel/train_eval_sgcn.py:303-306) as one
sweep over a 2-copy block-diagonal batch — there is no BatchNorm in this model, so the two passes do not
interact at all.

``SGCN_GAT`` is the same model with PyG GATConv(in, hidden, edge_dim=1) layers (``gcn_img_snp.GATConv``): masks, head,
regulariser and the stacked pair are shared (``_ImageOnly``), the graph stack is the LDS-resident GAT stack
(ops.GatStack: one kernel per direction for both passes).  The masked pass's edge attribute ``edge_weight * edge_prob``
is trained through it: igcn_gat_stack_bwd_ew returns d(loss)/d(edge attribute) — ``prob_bias`` gets its only task
gradient there.  The constructor reads ``dataset.num_features`` / ``dataset.num_classes`` (:163,168) and sizes ``lin1``
with the reference's literal 90 (:167).  Shapes outside the GAT stack raise ValueError; there is no second GAT path.
GATConv parity rests on the restatement of PyG 2.0.2's GATConv in tests/golden/gat_standin.py (PyG itself is unpinned).

``SGCN_Ori(H_0, H_1, H_2, H_3)`` — conv1 (H_0 -> H_1), ReLU, conv3 (H_1 -> H_3) whose PRE-ReLU output is
``final_conv_acts``, ReLU, and the head fc1 -> ReLU -> bn1 -> Dropout(0.5) -> fc2 -> ReLU -> bn2 -> Dropout(0.7) -> fc3
(ReLU in front of BatchNorm, :143-147) on cat(z1, z2), two node-major blocks.  The graph stack is one LDS-resident
kernel per direction (ops.SgcnOriStack: two independent widths, the tap and its gradient leave the kernels directly);
``IGCN_NO_FUSED_SGCN=1``, or a batch that kernel does not cover, takes gcn_norm once + (transform, aggregate) per layer.
``final_conv_grads`` is d(loss)/d(final_conv_acts) after a backward (the reference fills it through a hook, :71-72,125).
``conv2`` exists for its state_dict keys only (:121 is commented out in the reference) and ``fc1`` takes
``rois*H_3 + rois*H_2`` inputs (:20): a forward with H_1 != H_2 raises ValueError.
"""
import math


import torch
import torch.nn.functional as F
from torch.nn import Linear, Parameter, init

from . import ops, switches
from .gcn_img_snp import ROIS_REF, GATConv, gat_attention, gat_stack
from .sgcn_img_snp import GCNConv, _grid_width, edge_importance, masked_inputs, sgcn_stack


class _ImageOnly(torch.nn.Module):
    """What SGCN_GCN and SGCN_GAT share: the mask parameters, cal_probability / loss_probability, the head, and the
    plain / masked / stacked-pair forward around the subclass's graph stack (``_stack``)."""

    def _build(self, conv, num_features, num_classes, num_layers, hidden, hidden_linear, rois, H_0, lin1_rois):
        self.input = None
        self.rois, self.prob_dim = rois, H_0
        self.conv1 = conv(num_features, hidden)
        self.convs = torch.nn.ModuleList(conv(hidden, hidden) for _ in range(num_layers - 1))
        self.lin1 = Linear(lin1_rois * num_layers * hidden, hidden_linear)
        self.lin2 = Linear(hidden_linear, num_classes)
        self.prob = Parameter(torch.empty(rois, H_0))
        self.prob_bias = Parameter(torch.empty(H_0 * 2, 1))
        self.edge_prob = Parameter(torch.empty(rois, rois))               # unused by forward (as in the reference)
        self._init_masks()
        self._dropout_enabled = True
        self.batched_passes = True
        self.last_edge_prob = None

    def _init_masks(self):
        with torch.no_grad():
            for p in (self.prob_bias, self.prob, self.edge_prob):
                init.kaiming_uniform_(p, a=math.sqrt(5))

    def reset_parameters(self):
        self.conv1.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()
        self._init_masks()

    def cal_probability(self, x, edge_index, edge_weight, plan=None):
        """:321-332 (SGCN_GAT: :198-209) -> (x*prob, edge_weight*e, prob, e)."""
        plan = plan if plan is not None else ops.GraphPlan(edge_index, x.shape[0])
        xm, ewm, e = ops.EdgeMask.apply(x, self.prob, self.prob_bias, edge_weight, plan, self.rois)
        return xm, ewm, self.prob, e

    def loss_probability(self, x, edge_index, edge_weight, hp, eps=1e-6, plan=None, edge_prob=None):
        """:334-358 (SGCN_GAT: :211-233) (no SNP term; node-mask L1 = sum|sigmoid(prob)| / rois)."""
        if edge_prob is None:
            _, _, _, edge_prob = self.cal_probability(x, edge_index, edge_weight, plan=plan)
        none = self.prob.new_empty(0)
        return ops.MaskRegulariser.apply(self.prob, edge_prob, none, hp.lamda_x_l1 * self.prob_dim, hp.lamda_x_ent,
                                         hp.lamda_e_l1, hp.lamda_e_ent, eps)

    def forward(self, data, isExplain=False):
        """:360-388 (SGCN_GAT: :235-267)."""
        return self._forward_grouped(data, (bool(isExplain),))[0]

    def forward_pair(self, data):
        """(model(data), model(data, True)) of train() kernel/train_eval_sgcn.py:303,305 as one batched sweep."""
        return self._forward_grouped(data, (False, True))

    def _forward_grouped(self, data, explain_flags):
        # nothing of the last forward outlives this one: its edge mask holds that step's whole autograd graph.  Seen with
        # SGCN_GAT: a step captured right after an eager one (train.EpochTrainer) crashed at the end of the capture, after
        # torch's warning that an AccumulateGrad node of an earlier iteration, kept alive, sat on another stream; with the
        # mask dropped here the same run passes.  SGCN_GCN runs this same code (tests/test_gpu_sgcn_gat.py runs both
        # through fit_epoch)
        self.last_edge_prob = None
        x = data.x
        x.requires_grad = True                                         # :362 — populates data.x.grad
        self.input = x
        n = x.shape[0]
        if n % self.rois:
            raise ValueError(f"every graph must have exactly rois={self.rois} nodes (got {n} nodes)")
        bsz, g = n // self.rois, len(explain_flags)
        plan = ops.plan_for(data)
        plan.flush_pending_check()
        self._check_stack(plan, x, explain_flags)
        # the train step's (plain | masked) pair: the mask launch writes both halves of the stacked batch itself
        stacked = tuple(explain_flags) == (False, True) and x.is_cuda
        x_in, ew_in, _, self.last_edge_prob = masked_inputs(self, data, plan, explain_flags, stacked)
        xcat = self._stack(x_in, ew_in, plan.replicate(g))
        z = xcat.view(g * bsz, -1)                                    # to_dense_batch == view (:378-381)
        f1 = ops.linear(z, self.lin1.weight, self.lin1.bias, relu=True)
        if self.training and self._dropout_enabled:
            f1 = F.dropout(f1, 0.5, True)
        logp = F.log_softmax(ops.linear(f1, self.lin2.weight, self.lin2.bias), dim=-1)
        return [logp[k * bsz:(k + 1) * bsz] for k in range(g)] if g > 1 else [logp]

    def edge_importance(self, data, weighted=False, return_count=False):
        """``sgcn_img_snp.edge_importance`` of a batch: the dense [B, rois, rois] form of ``cal_probability``'s edge mask."""
        return edge_importance(self, data, weighted, return_count)

    def gat_attention(self, data, isExplain=False):
        raise ValueError(f"gat_attention: {self.__class__.__name__} has GCNConv layers (no attention coefficients)")

    def input_saliency(self, data, temperature=None, device=None, target=None, isExplain=False, inputs="image",
                       normalize=False):
        """``SGCN_GCN_IMGSNP.input_saliency`` of an image-only model: gradient x input of the target class's
        log-probability, a dict of ``attr`` [B, rois, H0], ``roi`` [B, rois] and ``target`` [B]; ``temperature`` and
        ``device`` are accepted for the sibling's signature, ``inputs`` other than "image" raises ValueError."""
        from . import saliency
        return saliency.input_saliency(self, data, temperature, device, target, isExplain, inputs, normalize)

    def integrated_gradients(self, data, temperature=None, device=None, target=None, isExplain=False, inputs="image",
                             normalize=False, steps=16, baseline=None):
        """``SGCN_GCN_IMGSNP.integrated_gradients`` of an image-only model (midpoint rule; ``delta`` [B] in the dict)."""
        from . import saliency
        return saliency.integrated_gradients(self, data, temperature, device, target, isExplain, inputs, normalize,
                                             steps, baseline)

    def grad_cam(self, data, target=None, isExplain=False, normalize=True):
        """The Grad-CAM map [B, rois] of ``SGCN_Ori``'s taps (kernel/sgcn.py:124-126): relu(sum_k alpha_k acts_k) with
        alpha the node mean of d score / d acts, of an eval-mode pass and the target class's log-probability
        (igcn_grad_cam).  Every other class raises ValueError: the reference never fills ``final_conv_acts`` there."""
        from . import saliency
        return saliency.grad_cam(self, data, target, isExplain, normalize)

    def _check_stack(self, plan, x, explain_flags):
        pass

    def __repr__(self):
        return self.__class__.__name__


class SGCN_GCN(_ImageOnly):
    def __init__(self, dataset, num_layers, hidden, *args, hidden_linear=64, rois=90, H_0=3, num_features=3,
                 num_classes=2, **kwargs):
        super().__init__()
        self._build(GCNConv, num_features, num_classes, num_layers, hidden, hidden_linear, rois, H_0, rois)

    def _stack(self, x_in, ew_in, plan_g):
        return sgcn_stack([self.conv1, *self.convs], x_in, ew_in, plan_g, self.rois,
                          not switches.on("IGCN_NO_FUSED_SGCN"))


class SGCN_GAT(_ImageOnly):
    def __init__(self, dataset, num_layers, hidden, *args, hidden_linear=64, rois=90, H_0=3, **kwargs):
        super().__init__()
        self._build(lambda i, o: GATConv(i, o, edge_dim=1), dataset.num_features, dataset.num_classes, num_layers,
                    hidden, hidden_linear, rois, H_0, ROIS_REF)

    def _check_stack(self, plan, x, explain_flags):
        """Refuse, before any launch, what the GAT stack does not cover (the sentence of ops.gat_stack_limits)."""
        why = ops.gat_stack_limits(plan, self.rois, x.shape[1], _grid_width(self.conv1.out_channels),
                                   1 + len(self.convs),
                                   ew_grad=torch.is_grad_enabled() and any(explain_flags))
        if why is not None:
            raise ValueError(f"GAT stack: {why}")

    def gat_attention(self, data, isExplain=False):
        """``gcn_img_snp.gat_attention`` of the plain or the masked pass: [B, L, rois, rois]."""
        return gat_attention(self, [self.conv1, *self.convs], data, isExplain)

    def _stack(self, x_in, ew_in, plan_g):
        return gat_stack([self.conv1, *self.convs], x_in, ew_in, plan_g, self.rois)


class SGCN_Ori(_ImageOnly):
    def __init__(self, H_0, H_1, H_2, H_3, class_num=2, hidden_size=64, rois=90):
        super().__init__()
        self.input = None
        self.final_conv_acts = None
        self.final_conv_pair_acts = None
        self._tap, self._fired = None, None
        self.rois, self.prob_dim = rois, H_0
        self.dim1, self.dim2, self.dim3 = rois * H_3 + rois * H_2, 64, 16              # :20-22
        self.conv1 = GCNConv(H_0, H_1)
        self.conv2 = GCNConv(H_1, H_2)                                   # unused by forward (:121), kept for its keys
        self.conv3 = GCNConv(H_1, H_3)
        self.fc1 = Linear(self.dim1, self.dim2)
        self.bn1 = torch.nn.BatchNorm1d(self.dim2)
        self.fc2 = Linear(self.dim2, self.dim3)
        self.bn2 = torch.nn.BatchNorm1d(self.dim3)
        self.fc3 = Linear(self.dim3, class_num)
        self.prob = Parameter(torch.empty(rois, H_0))
        self.prob_bias = Parameter(torch.empty(H_0 * 2, 1))
        self.edge_prob = Parameter(torch.empty(rois, rois))               # unused by forward (as in the reference)
        self._init_masks()
        self._dropout_enabled = True
        self.batched_passes = True
        self.last_edge_prob = None

    def reset_parameters(self):
        for m in (self.conv1, self.conv2, self.conv3, self.fc1, self.fc2, self.fc3, self.bn1, self.bn2):
            m.reset_parameters()
        self._init_masks()

    @property
    def final_conv_grads(self):
        """d(loss)/d(final_conv_acts) of the last backward (None before one).  After ``forward_pair`` it is the PLAIN
        pass's, as the reference's two calls leave it: both hooks write the attribute and the plain pass's fires last."""
        tap = self._fired
        if tap is None or tap.grads is None:
            return None
        return tap.grads[:tap.grads.shape[0] // tap.passes]

    def _tap_fired(self, tap):
        self._fired = tap

    @property
    def final_conv_pair(self):
        """((acts, grads) of pass 0, (acts, grads) of pass 1) of the last ``forward_pair`` — one entry after a single
        pass; ``grads`` is None until a backward has run."""
        if self.final_conv_pair_acts is None:
            return None
        g = None if self._tap is None else self._tap.grads
        n = self.final_conv_pair_acts[0].shape[0]
        return tuple((a, None if g is None else g[i * n:(i + 1) * n]) for i, a in enumerate(self.final_conv_pair_acts))

    def _graph_stack(self, x_in, ew_in, plan_g, tap):
        """(z [passes*B, rois*H_1 + rois*H_3], acts [passes*N, H_3]) of :120-138."""
        w1, b1, w3, b3 = self.conv1.lin.weight, self.conv1.bias, self.conv3.lin.weight, self.conv3.bias
        if (not switches.on("IGCN_NO_FUSED_SGCN") and x_in.is_cuda
                and ops.sgcn_ori_supported(plan_g, self.rois, x_in.shape[1], w1.shape[0], w3.shape[0])):
            return ops.SgcnOriStack.apply(x_in, ew_in, plan_g, self.rois, tap, w1, b1, w3, b3)
        what, wloop, tstream, sstream = ops.GcnNorm.apply(ew_in, plan_g)          # once for both layers
        h1 = ops.GcnPropagate.apply(ops.linear(x_in, w1), what, wloop, b1, plan_g, True, tstream, sstream)
        acts = ops.GcnPropagate.apply(ops.linear(h1, w3), what, wloop, b3, plan_g, False, tstream, sstream)
        if acts.requires_grad:
            acts.register_hook(tap.publish)                                # stores a reference: nothing waits
        g = x_in.shape[0] // self.rois
        return torch.cat((h1.view(g, -1), torch.relu(acts).view(g, -1)), 1), acts

    def _bn(self, x, bn, groups, p):
        keep = None
        if self.training and self._dropout_enabled:
            keep = F.dropout(torch.ones_like(x), p, True)                  # the factors {0, 1/(1-p)}, applied by the kernel
        return ops.BatchNorm1dGrouped.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, self.training,
                                            bn.momentum, bn.eps, 0, groups, keep)

    def _forward_grouped(self, data, explain_flags):
        if self.conv2.out_channels != self.conv1.out_channels:
            raise ValueError(f"SGCN_Ori: fc1 takes rois*H_3 + rois*H_2 inputs (kernel/sgcn.py:20) but the forward feeds it "
                             f"rois*H_3 + rois*H_1: H_1={self.conv1.out_channels} != H_2={self.conv2.out_channels}")
        # nothing of the last forward outlives this one (see _ImageOnly._forward_grouped): the tap is a node of that
        # step's autograd graph, and a step captured right after an eager one must not find that graph alive.  What a
        # backward has published (final_conv_grads) is a plain tensor and stays until the next backward replaces it.
        self.last_edge_prob = None
        self.final_conv_acts = self.final_conv_pair_acts = self._tap = None
        x = data.x
        x.requires_grad = True                                         # :113 — populates data.x.grad
        self.input = x
        n = x.shape[0]
        if n % self.rois:
            raise ValueError(f"every graph must have exactly rois={self.rois} nodes (got {n} nodes)")
        bsz, g = n // self.rois, len(explain_flags)
        plan = ops.plan_for(data)
        plan.flush_pending_check()
        stacked = tuple(explain_flags) == (False, True) and x.is_cuda
        x_in, ew_in, _, self.last_edge_prob = masked_inputs(self, data, plan, explain_flags, stacked)
        tap = ops.TapGrads(self._tap_fired)
        tap.passes = g
        z, acts = self._graph_stack(x_in, ew_in, plan.replicate(g), tap)
        self._tap = tap
        self.final_conv_pair_acts = tuple(acts[k * n:(k + 1) * n] for k in range(g))
        self.final_conv_acts = self.final_conv_pair_acts[-1]           # the reference's last call (the masked pass) wins
        h = self._bn(ops.linear(z, self.fc1.weight, self.fc1.bias, relu=True), self.bn1, g, 0.5)       # :143-144
        h = self._bn(ops.linear(h, self.fc2.weight, self.fc2.bias, relu=True), self.bn2, g, 0.7)       # :145-146
        if self.training:
            torch._foreach_add_([bn.num_batches_tracked for bn in (self.bn1, self.bn2)], g)
        logp = F.log_softmax(ops.linear(h, self.fc3.weight, self.fc3.bias), dim=-1)
        return [logp[k * bsz:(k + 1) * bsz] for k in range(g)] if g > 1 else [logp]
