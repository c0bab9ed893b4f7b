"""Drop-in ``GUIDE_IMGSNP`` on the HIP kernels: the gated-image + GO baseline of kernel/guide_img_snp.py:13-138.

Interface of the reference: constructor (:15-16: ``hidden_linear``, ``num_regr``, ``num_features`` and the flags it stores
but never reads — ``isCrossAtten``, ``isSoftSimilarity``, ``graph_pool``, ``isuseFeat4Regr``, ``isImageOnly``,
``isSNPsOnly``, ``ifUseGAT``), ``forward(data, temperature, device)`` and its 8-tuple (:78-135), ``reset_parameters`` (a
no-op, :72), the ``prob`` / ``input`` side effects and an identical ``state_dict()`` key set (the unused ``batch_norm``
included).  ``train.losses`` takes the five-term loss of kernel/train_eval_guide_img_snps.py:450-487 for this model.

What runs:
* the GO branch, igcn_amd.guide_go_model.Gene_ontology_network, whose mask launch also draws this model's five dropout
  sites (encoder_i_N, the two of decoder_i_N, the two heads) and advances the decoder BatchNorms' counters;
* the image gate and encoder_i_N, ops.GuideGate: one launch per direction (csrc/guide.hip).  The Gumbel noise comes from
  the library's counter-based generator with a device counter of its own (``_gate_state``), so a captured step draws
  afresh at every replay; ``_gate_noise`` [B, K, 2] imposes noise instead (parity tests);
* decoder_i_N: ops.BatchNormPReLU between the GEMM entry points (ops.linear); the heads: ops.linear.
Limits (ValueError): ``l_dim == 32`` (latent = (latent_g + latent_n) / 2 adds [B, l_dim] to [B, 32]); every graph of a batch
has ``rois`` nodes (the reference pads shorter graphs after a host sync; its data never needs it); rois * H_0 <= 1024 and
hidden_linear <= 64 (the gate kernel); a training forward needs the temperature.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn import Linear

from . import ops
from .guide_go_model import Gene_ontology_network

GATE_K_MAX, GATE_H_MAX = 1024, 64          # igcn_guide_gate_supported: K = rois * H_0, H = hidden_linear (latent 32)


class GUIDE_IMGSNP(nn.Module):
    guide = True             # train.losses: kernel/train_eval_guide_img_snps.py's loss; train.Evaluator refuses the model
    batched_passes = False   # one plain pass per step

    def __init__(self, num_layers, hidden, A_g, A, pool_dim, l_dim, device, *args, hidden_linear=32, rois=90, H_0=3,
                 num_features=3, num_classes=2, isCrossAtten=False, isSoftSimilarity=False, rbf_gamma=0.005,
                 graph_pool=False, isuseFeat4Regr=True, num_regr=3, model4eachregr=False, isImageOnly=True,
                 isSNPsOnly=False, ifUseGAT=False, **kwargs):
        super().__init__()
        if int(l_dim) != 32:
            raise ValueError(f"GUIDE_IMGSNP: l_dim must be 32 (the GO latent [B, l_dim] is averaged with the image latent "
                             f"[B, 32]); got {l_dim}")
        k = rois * H_0
        if k > GATE_K_MAX or hidden_linear > GATE_H_MAX:
            raise ValueError(f"GUIDE_IMGSNP: the gate kernel takes rois * H_0 <= {GATE_K_MAX} and hidden_linear <= "
                             f"{GATE_H_MAX}; got {k} and {hidden_linear}")
        self.device = device
        self.isCrossAtten, self.isSoftSimilarity, self.rbf_gamma = isCrossAtten, isSoftSimilarity, rbf_gamma
        self.isuseFeat4Regr, self.model4eachregr = isuseFeat4Regr, model4eachregr
        self.isImageOnly, self.isSNPsOnly, self.ifUseGAT = isImageOnly, isSNPsOnly, ifUseGAT
        self.num_regr, self.num_features, self.hidden_linear = num_regr, num_features, hidden_linear
        self.input = None
        self.final_conv_acts = None
        self.final_conv_grads = None
        self.rois, self.prob_dim = rois, H_0
        self.graph_pool = graph_pool
        self.latent_dim = 32
        self.lin1 = Linear(self.latent_dim, hidden_linear)
        self.lin1_regr = Linear(self.latent_dim, hidden_linear)
        self.lin2 = Linear(hidden_linear, num_classes)
        self.lin2_regr = Linear(hidden_linear, num_regr)
        self.encoder_i_N = nn.Sequential(nn.Linear(k, hidden_linear, bias=False), nn.PReLU(), nn.Dropout(0.4),
                                         nn.Linear(hidden_linear, self.latent_dim, bias=False))
        self.decoder_i_N = nn.Sequential(nn.BatchNorm1d(self.latent_dim), nn.PReLU(), nn.Dropout(0.4),
                                         nn.Linear(self.latent_dim, hidden_linear, bias=False),
                                         nn.BatchNorm1d(hidden_linear), nn.PReLU(), nn.Dropout(0.4),
                                         nn.Linear(hidden_linear, k, bias=False))
        self.bias_n = nn.ParameterList([nn.Parameter(0.1 * (2 * torch.rand(k, 2) - 1))])
        self.prob = [0, 0]
        self.go_network = Gene_ontology_network(A_g, A, 2, 2, [5, 5], pool_dim, l_dim, device, dim_snps_atten=hidden)
        self.go_network.outer_bns = (self.decoder_i_N[0], self.decoder_i_N[4])
        self.batch_norm = nn.BatchNorm1d(num_layers * hidden)
        self._dropout_enabled = True
        self._gate_noise = None      # [B, K, 2] device tensor: imposed Gumbel noise instead of the generator's draw
        self.last_gate = None        # (z1, s0 s1) [B, K, 2] of the last training forward

    def reset_parameters(self):
        pass

    def _check_batch(self, data):
        x = data.x
        b = int(data.num_graphs)
        if (x.dim() != 2 or x.shape[0] != b * self.rois or x.shape[1] != self.prob_dim
                or getattr(data, "_max_nodes", self.rois) != self.rois):
            raise ValueError(f"GUIDE_IMGSNP: every graph of a batch must have rois = {self.rois} nodes of H_0 = "
                             f"{self.prob_dim} features (got x {tuple(x.shape)} for {b} graphs)")
        return b

    def forward(self, data, temperature=None, device=None):
        """:78-135.  Returns (log_softmax, x_hat, latent, latent, linear_outf, our_reg, [img_out, decoded], [imp_N[:, 1]])."""
        b = self._check_batch(data)
        if self.training and temperature is None:
            raise ValueError("GUIDE_IMGSNP: a training forward needs the Gumbel-softmax temperature")
        x = data.x
        if x.is_leaf and not x.requires_grad:
            x.requires_grad_(True)                                    # :80 — populates data.x.grad
        self.input = x
        k, h = self.rois * self.prob_dim, self.hidden_linear
        img = x.view(b, k)
        go = self.go_network
        extra = [((b, h), 0.4), ((b, self.latent_dim), 0.4), ((b, h), 0.4), ((b, h), 0.5), ((b, h), 0.3)]
        latent_g, x_hat, _, _ = go(data.snps_feat, temperature, device, extra_dropout=extra)
        k_enc, k_dec1, k_dec2, k_h1, k_h2 = go.extra_masks if self._dropout_enabled else [None] * 5
        state = None
        if self.training and self._gate_noise is None:
            state = getattr(self, "_gate_state", None)
            if state is None or state.state.device != x.device:
                state = self._gate_state = ops.DropoutState(x.device)
        enc = self.encoder_i_N
        latent_n, imp1, self.last_gate = ops.GuideGate.apply(img, self.bias_n[0], enc[0].weight, enc[1].weight,
                                                             enc[3].weight, k_enc, temperature, self.training,
                                                             self._gate_noise, state)
        latent = (latent_g + latent_n) / 2
        dec = self.decoder_i_N
        t = ops.BatchNormPReLU.apply(latent, None, dec[0].weight, dec[0].bias, dec[1].weight, dec[0], self.training, k_dec1)
        t = ops.linear(t, dec[3].weight)
        t = ops.BatchNormPReLU.apply(t, None, dec[4].weight, dec[4].bias, dec[5].weight, dec[4], self.training, k_dec2)
        decoded = ops.linear(t, dec[7].weight)
        self.prob = [imp1.detach()]
        linear_outf = ops.linear(latent, self.lin1.weight, self.lin1.bias, relu=True)
        logits = ops.linear(linear_outf, self.lin2.weight, self.lin2.bias, keep=k_h1)
        reg = ops.linear(latent, self.lin1_regr.weight, self.lin1_regr.bias, relu=True)
        reg = ops.linear(reg, self.lin2_regr.weight, self.lin2_regr.bias, keep=k_h2)
        return F.log_softmax(logits, dim=-1), x_hat, latent, latent, linear_outf, reg, [img, decoded], [imp1]

    def __repr__(self):
        return self.__class__.__name__
