"""Drop-in ``Gene_ontology_network`` of GUIDE_IMGSNP on the HIP kernels: kernel/guide_go_model.py.

The GUIDE variant of the GO network differs from kernel/go_model.py in its activations and its latent MLP
(guide_go_model.py:103,112,117-157): every activation is ``nn.PReLU()`` (one learnable slope per module), the latent MLP
is ``Linear -> BN(32) -> PReLU -> Dropout(0.5) -> Linear`` with nothing behind its last layer, and the unused
``classification`` module is built with PReLU.  Constructor, ``forward(data, T, device) -> (latent, x_D, [zeros(3)],
atten_out)`` and the ``state_dict()`` key set are the reference's.  The hierarchy's index structures, the gene encoding /
decoding and the attention layers are those of ``igcn_amd.go_model`` (this class subclasses it); the PReLU blocks run
on csrc/guide.hip:

* LayerNorm over nodes + PReLU + Dropout2d + pooling (w_act, w_act_out): ops.NodesLayerNormPReLU behind the plain
  layer kernels (ops.GoAttention / ops.GoDecode) — the unfused route; the LDS-resident layer + LayerNorm backward of
  the ReLU network has no PReLU form (GUIDE_IMGSNP);
* conc + B, conc_D + B_D and the latent MLP's BN(32): ops.BatchNormPReLU;
* conc_for_attention: GUIDE discards its output.  It is computed (returned detached) and, in training, its BatchNorm's
  running statistics advance as in the reference; no gradient reaches its parameters.
"""
import torch
import torch.nn as nn

from . import go_model, ops
from .go_model import N_SNPS


class Gene_ontology_network(go_model.Gene_ontology_network):
    def __init__(self, A_g, A, in_f_dim, n_l, f_dim, pool_dim, l_dim, device, dim_snps_atten=5):
        super().__init__(A_g, A, in_f_dim, n_l, f_dim, pool_dim, l_dim, device, dim_snps_atten=dim_snps_atten)
        fd, n_top, n = self.f_dim, self.n_top, self.n_nodes
        lin = lambda i, o: nn.Linear(i, o, bias=False)       # noqa: E731
        self.w_act = nn.ModuleList([nn.PReLU() for _ in range(n_l)])
        self.w_act_out = nn.ModuleList([nn.PReLU() for _ in range(n_l)])
        self.conc_for_attention = nn.Sequential(lin(fd[-1], dim_snps_atten), nn.BatchNorm1d(n_top), nn.PReLU())
        self.B = nn.Sequential(nn.BatchNorm1d(n_top), nn.PReLU(), nn.Dropout(0.5))
        self.B_D = nn.Sequential(nn.BatchNorm1d(n), nn.PReLU(), nn.Dropout(0.5))
        self.latent = nn.Sequential(lin(n_top, 32), nn.BatchNorm1d(32), nn.PReLU(), nn.Dropout(0.5), lin(32, l_dim))
        self.classification = nn.Sequential(nn.BatchNorm1d(l_dim + N_SNPS), nn.PReLU(), nn.Dropout(0.5),
                                            lin(l_dim + N_SNPS, 16), nn.PReLU(), nn.Dropout(0.3),
                                            nn.Linear(16, 1, bias=True), nn.Sigmoid())
        # BatchNorms of an enclosing model whose num_batches_tracked ride in this network's mask launch
        self.outer_bns = ()

    def _batch_counters(self):
        bns = (self.conc_for_attention[1], self.B[0], self.B_D[0], self.latent[1]) + tuple(self.outer_bns)
        return [bn.num_batches_tracked for bn in bns if bn.track_running_stats and bn.num_batches_tracked is not None]

    def predraw_dropout(self, *a, **kw):
        raise NotImplementedError("the GUIDE GO network draws its masks in its forward")

    def attention_rollout(self, *a, **kw):
        raise NotImplementedError("attention_rollout runs the encoder of go_model.py (LayerNorm + ReLU blocks); the GUIDE "
                                  "GO network's PReLU blocks are not covered")

    def forward(self, data, T=None, device=None, extra_dropout=()):
        """``extra_dropout`` [(shape, p), ...]: dropout sites of the caller drawn by the same launch; their factors are
        left in ``self.extra_masks``."""
        bsz, dev = data.shape[0], data.device
        self._counters_done = False
        masks, self.extra_masks = self._dropout_masks(bsz, dev, extra_dropout)
        keeps = masks["ln"]
        # gene encoding (:208-215)
        x = ops.SparseMap.apply(data, self.gene_csr, *self.t)                            # [B, in_f, N]
        # encoder (:219-251): layer, then LayerNorm + PReLU + Dropout2d + pooling
        for j in range(self.n_l):
            y = ops.GoAttention.apply(x, self.w_inc[j].weight, self.w_s_loop[j].weight, self.w_att_in[j].weight,
                                      self.w_att_s[j].weight, self.enc_csr[j])
            x = ops.NodesLayerNormPReLU.apply(y, self.G_B[j].weight, self.G_B[j].bias, self.w_act[j].weight, keeps[j],
                                              self.pool[j], self.G_B[j].eps)
        # read-outs (:254-255); conc_for_attention's output is discarded by GUIDE_IMGSNP: no autograd node
        ca = self.conc_for_attention
        with torch.no_grad():
            atten_out = ops.bn_prelu_forward(x, ca[0].weight, ca[1], ca[2].weight, self.training)[0]
        inp_out = ops.BatchNormPReLU.apply(x, self.conc.weight, self.B[0].weight, self.B[0].bias, self.B[1].weight,
                                           self.B[0], self.training, masks["inp"])                   # [B, n_top]
        # decoder (:258-275)
        for j in range(self.n_l):
            y = ops.GoDecode.apply(x, self.w_out[j].weight, self.w_s_loop_out[j].weight, self.dec_csr[j])
            x = ops.NodesLayerNormPReLU.apply(y, self.G_B_D[j].weight, self.G_B_D[j].bias, self.w_act_out[j].weight,
                                              keeps[self.n_l + j], 0, self.G_B_D[j].eps)
        # gene decoding (:278-282)
        out_d = ops.BatchNormPReLU.apply(x, self.conc_D.weight, self.B_D[0].weight, self.B_D[0].bias, self.B_D[1].weight,
                                         self.B_D[0], self.training, masks["out_d"])                 # [B, N]
        x_d = ops.SparseMap.apply(out_d, self.gene_t_csr, self.t_D[0]).squeeze(1)               # [B, 54]
        # latent projection (:138-144,285)
        h = ops.linear(inp_out, self.latent[0].weight)
        h = ops.BatchNormPReLU.apply(h, None, self.latent[1].weight, self.latent[1].bias, self.latent[2].weight,
                                     self.latent[1], self.training, masks["h"])
        latent = ops.linear(h, self.latent[4].weight)
        if self.training and not self._counters_done:    # (with dropout on, the mask launch has advanced them already)
            cnt = self._batch_counters()
            if cnt:
                torch._foreach_add_(cnt, 1)
        zeros3 = getattr(self, "_zeros3", None)          # placeholder of the reference's unused third output
        if zeros3 is None or zeros3.device != dev:
            zeros3 = self._zeros3 = torch.zeros(3, device=dev)
        return latent, x_d, [zeros3], atten_out
