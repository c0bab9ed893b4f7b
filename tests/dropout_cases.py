"""The dropout-on configurations the GPU tests compare with the float64 oracle under the step's own masks, and what a
test without a GPU needs of them (tests/test_oracle_dropout.py's negative control runs the oracle at these very shapes,
seeds and stream counter): the site lists of the models' mask launches, the masks of a counter as an oracle.dropout
feed, and the CPU side of each configuration.

A dropout-on comparison never reads torch's generator: the GPU tests SET the mask generator's stream counter
(``go_network._drop_state.state[0] = COUNTER``), so the masks of every configuration are known here.
"""
from types import SimpleNamespace

import numpy as np
import torch

from _weights import seeded_state
from oracle import dropout as OD
from oracle import go_network as OG

COUNTER = (7 << 32) + 20231                      # the high word takes part in the hash
LOSS_TOL = 1e-4                                  # loss and terms: LOSS_TOL * max(1, |ref|)
MARGIN = 100 * LOSS_TOL                          # what other masks must move the loss by, at the least (same scale)
# The control that swaps the two passes' row ranges reads the terms (``gap``): the issue of the c + 1 control's factor does
# not arise there — of 492 (graph seed, counter) pairs tried, none gave 100 LOSS_TOL on both controls (the plain and the
# masked pass differ by the region / edge masks only, so their ``ce`` / ``mi`` lie close together).  What the control has
# to show is that a HIP value within LOSS_TOL of one evaluation cannot be within LOSS_TOL of the other — a gap above
# 2 LOSS_TOL — and it asks for ten times that.
ROWS_MARGIN = 20 * LOSS_TOL
SMALL_POOL, LARGE_POOL = (300, 120, 60, 19, 1), (1800, 800, 300, 99, 1)
LAM = [1.0, 1.0, 0.5, 1.5e-6, 0.1, 0.2]
HEADLINE = dict(rois=90, layers=2, hidden=16, h0=3, bsz=8, graph_seed=79, go_seed=1, state_seed=5, hidden_linear=64)
GUIDE = dict(hidden=10, bsz=8, seed=97, rois=90, h0=3, hidden_linear=32, tau=0.1, pool=LARGE_POOL)
CLUSTER_TAGS, CLUSTER_B = ("h0_3", "nopredict"), 8


def go_sites(pool, b, extra=(), n_l=2, hidden=32):
    """[(shape, p), ...] of one mask launch for ``b`` rows, in ``Gene_ontology_network._dropout_masks``' order: the
    encoder and decoder LayerNorm sites ([b, nodes of the level], p = 0.4), inp_out [b, n_top], out_D [b, N], the latent
    hidden layer [b, 32] (p = 0.5), then the caller's."""
    n = sum(pool)
    enc = [n - sum(pool[:i]) for i in range(n_l)]
    dec = [n - sum(pool[:n_l - i - 1]) for i in range(n_l)]
    sites = [((b, m), 0.4) for m in enc + dec]
    sites += [((b, n - sum(pool[:n_l])), 0.5), ((b, n), 0.5), ((b, hidden), 0.5)]
    return sites + [(tuple(s), p) for s, p in extra]


def headline_sites(pool, rows):
    hl = HEADLINE["hidden_linear"]
    return go_sites(pool, rows, [((rows, hl), 0.5), ((rows, hl), 0.3)])


def cluster_sites(pool, rows, hl=64):
    return go_sites(pool, rows, [((rows, hl), 0.5), ((rows, hl), 0.5)])


def guide_sites(b):
    h, latent = GUIDE["hidden_linear"], 32
    return go_sites(GUIDE["pool"], b, [((b, h), 0.4), ((b, latent), 0.4), ((b, h), 0.4), ((b, h), 0.5), ((b, h), 0.3)])


def gap(own, other, what="loss"):
    """How far two evaluations (loss, terms) are apart, in units of max(1, |own|): of the loss, or (``what="terms"``) of
    the term that moved most.  Swapping the two passes' rows leaves the headline loss almost where it was — ``reg``,
    ``recon`` and ``cluster`` are means over both passes and ``ce`` / ``mi`` carry equal weights — while ``ce`` and ``mi``
    themselves trade places: that control reads the terms."""
    rel = lambda a, b: abs(float(a) - float(b)) / max(1.0, abs(float(a)))          # noqa: E731
    if what == "loss":
        return rel(own[0], other[0])
    return max(rel(own[1][k], other[1][k]) for k in own[1])


def feed(sites, counter, heads):
    """The feed of the launch ``sites`` at stream counter ``counter``; ``heads``: the names of the caller's sites."""
    return OD.feed_of(sites, OD.masks(sites, counter), OD.go_site_names(2, heads))


def cpu_batch(graphs, dtype=torch.float64):
    from igcn_amd.data import Batch
    dd = Batch.from_data_list(graphs)
    dd.x = dd.x.to(dtype).requires_grad_(True)
    for k in ("edge_attr", "snps_feat", "tsne_fdim", "clini_score"):
        if getattr(dd, k, None) is not None:
            setattr(dd, k, getattr(dd, k).to(dtype))
    return dd


def headline_model(pool, device, **kw):
    """SGCN_GCN_IMGSNP at the headline shape on ``device`` (a CPU instance serves for its state's shapes) and the
    hierarchy it was built on."""
    from igcn_amd import synth
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    c = HEADLINE
    go_snps, adj, pool_dim = synth.go_hierarchy(pool, seed=c["go_seed"])
    a_g, a = synth.go_sparse_inputs(go_snps, adj, device)
    model = SGCN_GCN_IMGSNP(c["layers"], c["hidden"], a_g, a, pool_dim, 32, device, rois=c["rois"], H_0=c["h0"],
                            num_classes=3, isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3,
                            isuseProb4Regr=True, isImageOnly=False, isSNPsOnly=False, **kw).to(device)
    return model, go_snps, adj


def headline_cpu(pool):
    """(cfg, index sets, fp32 state, graphs) of the headline configuration on ``pool``: what
    tests/test_gpu_model.py::train_mode_vs_oracle builds from the same seeds."""
    from igcn_amd import synth
    c = HEADLINE
    model, go_snps, adj = headline_model(pool, "cpu")
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, c["state_seed"])
    idx = OG.go_index_sets(*synth.go_sparse_inputs(go_snps, adj), list(pool), 2)
    graphs = synth.brain_graph_list(c["bsz"], seed=c["graph_seed"], rois=c["rois"], h0=c["h0"], tsne_dim=16)
    cfg = SimpleNamespace(num_layers=c["layers"], rois=c["rois"], image_only=False, rbf_gamma=0.01)
    return cfg, idx, sd, graphs


def guide_setup(hidden, bsz, seed, device, pool=LARGE_POOL, rois=90, h0=3, hidden_linear=32, tau=0.1):
    """(model on ``device``, float32 state, index sets, graphs, noise [B, K, 2]) of a GUIDE_IMGSNP configuration: every
    PReLU slope a seeded positive value (its decisions show in its output), the gate's Gumbel noise moved 1e-3 off a
    hard-decision tie (as tests/golden/make_golden_guide.py)."""
    import guide_ref
    from igcn_amd import synth
    from igcn_amd.guide_img_snp import GUIDE_IMGSNP
    go_snps, adj, pool_dim = synth.go_hierarchy(pool, seed=seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, device)
    model = GUIDE_IMGSNP(2, hidden, a_g, a, pool_dim, 32, device, rois=rois, H_0=h0, num_classes=3, num_regr=3,
                         hidden_linear=hidden_linear).to(device)
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, seed, model.state_dict())
    rng = np.random.default_rng(seed + 1)
    for k in sorted(sd):
        if k.endswith(".weight") and tuple(sd[k].shape) == (1,):
            sd[k] = torch.tensor([rng.uniform(0.1, 0.6)], dtype=torch.float32)
    idx = OG.go_index_sets(*synth.go_sparse_inputs(go_snps, adj), list(pool), 2)
    graphs = synth.brain_graph_list(bsz, seed=seed + 10, rois=rois, top_k=3, tsne_dim=16)
    k = rois * h0
    g = guide_ref.gumbel_noise(seed + 20, bsz, k).astype(np.float64)
    logit = np.log(torch.softmax(sd["bias_n.0"].double(), 1).numpy())
    w = (logit[None] + g) / tau
    g[..., 1] += np.where(np.abs(w[..., 1] - w[..., 0]) < 1e-3, 0.05, 0.0)
    return model, sd, idx, graphs, g.astype(np.float32)


class recorded_masks:
    """Record what ``ops.dropout_masks`` was asked for and returned: ``calls`` = [(sites, tensors, ride), ...].  The
    tensors are read AFTER the step has synchronised (a rider's are filled by the plan build's launch)."""

    def __init__(self, monkeypatch):
        from igcn_amd import ops
        self.calls = []
        real = ops.dropout_masks

        def spy(sites, state, counters=(), inc=0, ride=False):
            out = real(sites, state, counters, inc, ride=ride)
            self.calls.append(([(tuple(int(d) for d in s), float(p)) for s, p in sites], list(out), bool(ride)))
            return out
        monkeypatch.setattr(ops, "dropout_masks", spy)

    def arrays(self, k):
        torch.cuda.synchronize()
        return [t.detach().cpu().numpy() for t in self.calls[k][1]]


def assert_masks_rebuilt(sites, arrays, counter, what=""):
    """The recorded factors equal, bit for bit, what the generator's contract gives for ``counter`` on the host."""
    want = OD.masks(sites, counter)
    assert len(want) == len(arrays), (what, len(want), len(arrays))
    for k, (g, w) in enumerate(zip(arrays, want)):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), \
            f"{what}: site {k} {sites[k]} differs from the masks of counter {counter} in {int((g != w).sum())} entries"


def set_counter(go, counter=COUNTER):
    """Give the GO network a mask generator at a known stream counter; returns the state."""
    from igcn_amd import ops
    st = getattr(go, "_drop_state", None)
    if st is None or not st.state.is_cuda:
        st = go._drop_state = ops.DropoutState(torch.device("cuda", torch.cuda.current_device()))
    st.state.zero_()
    st.state[0] = counter
    return st
