"""Every ``IGCN_*`` environment switch the package reads, in one table (INTEGRATION §4 documents each row).

Each A/B switch selects the older code path that a fusion replaced, so the fused path can be checked against it; the
value ``"1"`` means on and nothing else does.  Host switches are read on every use (a test may flip one with
``monkeypatch`` inside a process); the library bits are read once, when ``_lib.load()`` hands ``library_mask()`` to
``igcn_configure``.  A name that is not in the table raises, so a misspelled switch fails instead of doing nothing.
"""
import os

# host switches: read by the Python layer on every use
HOST = {
    "IGCN_NO_FUSED_SGCN": "per-layer SGCN kernels instead of the LDS-resident stack",
    "IGCN_NO_FRONT_FUSED": "plan build, mask launch and SGCN stack forward as three launches, not igcn_sgcn_front_fwd",
    "IGCN_NO_MASK_BWD_FUSED": "front backward: the mask's node pass as its own launch, not in the stack backward's masked copy",
    "IGCN_PLAN_REPLICATE_LAUNCH": "LDS plans: the two-pass replica by a launch of its own after each build, not filled by it",
    "IGCN_NO_DENSE_BLOCKS": "complete graphs: the general sorted-plan kernels instead of the dense-block path",
    "IGCN_NO_DROPOUT_RIDER": "captured step: the dropout masks as a launch of their own, not riding in the plan build",
    "IGCN_NO_DEFER": "every gradient reduction of the backward launched on the spot instead of one deferred launch",
    "IGCN_NO_GEMM_GROUPS": "one launch per dense product instead of the grouped launches",
    "IGCN_NO_GRAM_RIDER": "the batch losses' Gram products as their own launch, not riders of the heads' GEMM launch",
    "IGCN_NO_GRAM_LOSS_PAIRED": "the Gram losses as their own launch, not extra workgroups of the head-loss launch",
    "IGCN_NO_READOUT_PAIR": "the two read-outs of the encoder output as two ops instead of the paired launches",
    "IGCN_NO_GRAD_FAN": "multi-consumer tensors: autograd's pairwise gradient adds instead of ops.GradFan",
    "IGCN_NO_MASK_REG_FUSED": "loss_probability and the SNP mask as their own launches, not in the stacked mask launch",
    "IGCN_NO_PROJ_FUSED": "the attention in-projection through the grouped GEMM instead of the streaming kernels",
    "IGCN_NO_PROJ_BIAS_FUSED": "in-projection backward: the bias gradients as their own launch, not in the streaming pass",
    "IGCN_NO_HEAD_FUSED": "the heads' first-layer backward through the grouped GEMM instead of igcn_head_bwd_pair",
    "IGCN_NO_RELU_OWED": "relu(out_proj(.)): its own ReLU-mask / bias-gradient pass, not igcn_head_inputs_bwd_relu",
    "IGCN_NO_OUTPROJ_FUSED": "relu(out_proj(.)) as a GEMM launch before igcn_head_inputs_fwd, not inside it",
    "IGCN_NO_LINEAR_BN_FUSED": "latent MLP: the wide layer's split-K slab sums as their own launch, not in its BatchNorm",
    "IGCN_NO_LN_FUSED": "GO layers: the LayerNorm backward as its own launches, not inside the attention backward",
    "IGCN_NO_LOSS_HEAD_FUSED": "the loss head's backward as its own launch also under the cached unit gradient",
    "IGCN_NO_HEAD_LOSS_FUSED": "lin2 / lin2_regr, log-softmax and loss head as two launches, not igcn_head_loss_fwd",
    "IGCN_LN_AFFINE_NOW": "LayerNorm affine gradients launched inside their layer's backward, not queued to its end",
    "IGCN_SPMM_DVAL_NOW": "map value gradients launched inside their layer's backward, not queued to its end",
    "IGCN_SNP_GRAD_ALL": "SNP -> gene map backward: every row of the input gradient, also those nothing reads",
    "IGCN_SPARSE_MAPS": "SNP <-> GO maps: the LDS-tiled CSR kernels at every batch size",
    "IGCN_DENSE_MAPS": "SNP <-> GO maps: the dense-image + GEMM formulation at every batch size",
}

# library bits: in the bit order of IGCN_OPT_* (csrc/common.h); read once, when the library loads
LIBRARY = (
    ("IGCN_NO_TILED_LISTS", "dense graphs: wave-per-list walks instead of the tiled node-lane kernels"),
    ("IGCN_PROPAGATE_NO_LDS", "dense graphs: the wave-per-target aggregation instead of the LDS-staged one"),
    ("IGCN_SPMM_NO_LDS", "SNP <-> GO maps: the first (untiled) CSR kernels"),
    ("IGCN_GO_ATTN_CM", "GO attention backward and decoder: the global-memory kernels even when a sample fits LDS"),
    ("IGCN_DEBUG_REDUCE", "print every deferred reduction at the flush (a diagnostic: changes no number)"),
    ("IGCN_ATTN_FP32_CORE", "bf16 feature transforms: keep the fp32 attention core instead of the bf16-operand one"),
    ("IGCN_ATTN_BWD_TWICE", "exact-fp32 attention backward: the two-orientation kernel instead of the shared-tile one"),
    ("IGCN_ATTN_EXACT_FP32", "attention core, head_dim 16: the exact-fp32 MFMA kernels instead of the split-bf16 ones"),
    ("IGCN_NO_MAP_FUSED", "gene decoding: the read-out's apply pass and the map forward as two launches, not one"),
)

# integer knobs handed to igcn_configure: sweep parameters of tools/gemm_sweep.py, exempt from the switch tests (they
# tune a tile size; no path is A/B-compared)
KNOBS = {
    "IGCN_GEMM_BN": "> 0: cap of the GEMM tile width",
    "IGCN_ATTN_CHUNK": "> 0: rows per LDS chunk of the streamed attention kernels (also disables the split core)",
}

# diagnostics: print, change no number, exempt from the switch tests
DIAGNOSTICS = {
    "IGCN_DEBUG_SYNC": "announce every entry point on stderr and synchronise after it (read by _lib at import)",
    "IGCN_DEBUG_REDUCE": "library bit 4: print every deferred reduction at the flush",
}

EXEMPT = frozenset(KNOBS) | frozenset(DIAGNOSTICS)
ALL = frozenset(HOST) | frozenset(n for n, _ in LIBRARY) | EXEMPT


def on(name):
    """Host switch ``name`` is set to "1" (read now: tests flip these inside one process)."""
    if name not in HOST:
        raise KeyError(f"{name} is not a host switch of igcn_amd (switches.HOST)")
    return os.environ.get(name) == "1"


def library_mask(env=os.environ):
    """The ``options`` bit mask of ``igcn_configure`` for environment ``env``: bit k is LIBRARY[k] set to "1"."""
    return sum(1 << bit for bit, (name, _) in enumerate(LIBRARY) if env.get(name) == "1")


def knob(name, env=os.environ):
    """Integer knob ``name`` (0: unset or empty)."""
    if name not in KNOBS:
        raise KeyError(f"{name} is not an integer knob of igcn_amd (switches.KNOBS)")
    return int(env.get(name) or 0)
