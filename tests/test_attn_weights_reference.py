"""CPU checks of the attention-weights feature (kernel/sgcn_img_snp.py:240, the second output of
``self.multihead_attn``): the fp64 restatement the GPU tests compare with equals torch's own module, the C ABI declares
and binds the new entry points, the host-only shape queries answer without a GPU, and a model without cross-attention
refuses before anything is launched."""
import os

import pytest
import torch

import attn_map_ref as R
from conftest import ROOT
from igcn_amd import _lib

NAMES = ("igcn_attn_weights_supported", "igcn_attn_weights_chunk_rows", "igcn_attn_weights", "igcn_attn_map_accumulate")


@pytest.mark.parametrize("d,h,lq,lk", [(32, 2, 90, 29), (20, 2, 90, 400), (192, 2, 17, 53)])
def test_restatement_equals_torch_module(d, h, lq, lk):
    g = torch.Generator().manual_seed(d + lk)
    query, memory = torch.randn(2, lq, d, generator=g), torch.randn(2, lk, d, generator=g)
    w, bias = torch.randn(3 * d, d, generator=g) / d ** 0.5, torch.randn(3 * d, generator=g)
    want, q, kv = R.mha_module_weights(query, memory, w, bias, h)
    got = R.weights_fp64(q, kv, h)
    assert tuple(got.shape) == (2, lq, lk)
    assert float((got - want).abs().max()) <= 1e-15
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-14


def test_header_and_binding_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "igcn.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name


def _lib_or_build():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_supported_shapes_host_only():
    lib = _lib_or_build()
    for shape in ((32, 2, 90, 400), (20, 2, 90, 400), (192, 2, 300, 53), (64, 2, 270, 400)):
        assert lib.igcn_attn_weights_supported(*shape) != 0, shape
    assert lib.igcn_attn_weights_supported(200, 2, 90, 400) == 0
    assert lib.igcn_attn_weights_supported(33, 2, 90, 400) == 0          # D is no multiple of H


def test_chunk_rows_host_only():
    lib = _lib_or_build()
    assert lib.igcn_attn_weights_chunk_rows(32, 2, 90, 400) == 0         # the default width keeps 400 keys resident
    ch = lib.igcn_attn_weights_chunk_rows(192, 2, 17, 100000)
    assert ch > 0 and ch % 16 == 0
    assert lib.igcn_attn_weights_chunk_rows(192, 2, 17, ch) == 0         # exactly one chunk: resident
    assert lib.igcn_attn_weights_chunk_rows(192, 2, 17, ch + 5) == ch
    assert lib.igcn_attn_weights_chunk_rows(200, 2, 90, 400) == 0        # not covered


def test_model_without_cross_attention_refuses_before_any_launch(monkeypatch):
    from types import SimpleNamespace

    from calltrace import record_calls
    from igcn_amd import synth
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    go_snps, adj, pool_dim = synth.go_hierarchy((60, 30, 20, 9, 1), seed=2)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cpu")
    model = SGCN_GCN_IMGSNP(2, 8, a_g, a, pool_dim, 32, "cpu", rois=90, H_0=3, num_classes=3, isImageOnly=True)
    seen = record_calls(monkeypatch)
    was = model.training
    with pytest.raises(ValueError, match="cross-attention"):
        model.attention_weights(SimpleNamespace(x=torch.zeros(90, 3)))
    assert seen == [] and model.training == was
