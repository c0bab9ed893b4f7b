"""CPU checks of SGCN_Ori (kernel/sgcn.py:11-151) against the fixture captured from the reference
(tests/golden/sgcn_ori.npz, written by tests/golden/make_golden_sgcn_ori.py): the fixture itself and its sign condition,
the drop-in's state_dict, the float64 restatement tests/sgcn_ori_ref.py at the bounds tests/test_oracle_golden.py holds
the SGCN_GCN restatement to, and the host-only parts of the new entry points."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import assert_matches, golden_group
from _weights import seeded_state
from igcn_amd import synth
from igcn_amd.data import Batch

import sgcn_ori_ref as REF

TAGS = ["h32_5", "h16_8"]
DIMS = {"h32_5": (3, 32, 32, 5), "h16_8": (3, 16, 16, 8)}


def _cfg(store, tag):
    rois, h0, h1, h2, h3, b_eval, b_train, seed, top_k = [int(v) for v in store[f"{tag}/cfg"]]
    return rois, (h0, h1, h2, h3), b_eval, b_train, seed, top_k


def _probe(outs, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal(tuple(o.shape))).float() for o in outs]


def _leaf_state(sd):
    out = {}
    for k, v in sd.items():
        v = v.detach().clone()
        if v.dtype.is_floating_point:
            v = v.double()
            if "running_" not in k:
                v.requires_grad_(True)
        out[k] = v
    return out


def _data64(graphs):
    data = Batch.from_data_list(graphs)
    data.x = data.x.double().requires_grad_(True)
    data.edge_attr = data.edge_attr.double()
    return data


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_reloads_and_the_tap_has_both_signs(golden, tag):
    store = golden("sgcn_ori")
    rois, dims, b_eval, b_train, seed, top_k = _cfg(store, tag)
    assert dims == DIMS[tag] and (rois, b_eval, b_train, top_k) == (90, 4, 32, 3)
    assert "SGCN_Ori" in str(store["meta"])
    for mode in ("eval", "train"):
        for explain in (0, 1):
            sub = f"{tag}/{mode}/explain{explain}"
            frac = float(store[sub + "/cam/neg_frac"])
            assert 0.2 <= frac <= 0.8, (sub, frac)
            cam = golden_group(store, sub + "/cam")
            assert {"final_conv_acts", "final_conv_grads", "neg_frac"} <= set(cam)
            if mode == "eval":                       # stored in full: the share is recomputed; the tap's gradient is
                acts, grads = cam["final_conv_acts"], cam["final_conv_grads"]          # exactly 0 where ReLU closes
                assert acts.shape == grads.shape == (b_eval * rois, dims[3])
                assert float((acts < 0).mean()) == pytest.approx(frac, abs=1e-12)
                assert np.abs(grads[acts < 0]).max() == 0 and np.abs(grads[acts > 0]).max() > 0
    fr = store[f"{tag}/step/cam/neg_frac"]
    assert fr.shape == (2,) and bool(((fr >= 0.2) & (fr <= 0.8)).all()), fr
    assert int(store[f"{tag}/step/buffers/bn1.num_batches_tracked"]) == 2


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_keys_and_shapes_equal_the_references(golden, tag):
    from igcn_amd.sgcn import SGCN_Ori
    store = golden("sgcn_ori")
    rois, dims, *_ = _cfg(store, tag)
    model = SGCN_Ori(*dims, rois=rois)
    sd = model.state_dict()
    keys = store[f"{tag}/state_keys"].tolist()
    assert sorted(sd) == keys
    shapes = dict(zip(keys, store[f"{tag}/state_shapes"].tolist()))
    for k in keys:
        assert ",".join(str(d) for d in sd[k].shape) == shapes[k], k
    assert REF.param_shapes(*dims, rois=rois).keys() == sd.keys()
    for k, s in REF.param_shapes(*dims, rois=rois).items():
        assert tuple(sd[k].shape) == tuple(s), k
    assert repr(model) == "SGCN_Ori" and model.final_conv_acts is None and model.final_conv_grads is None
    # prob is kaiming-initialised (:43-49), not left at its zeros
    assert float(model.prob.detach().abs().max()) > 0
    model.reset_parameters()
    assert sorted(model.state_dict()) == keys


def test_fc1_takes_h2_not_h1():
    from igcn_amd.sgcn import SGCN_Ori
    model = SGCN_Ori(3, 32, 16, 5, rois=90)
    assert model.fc1.in_features == 90 * 5 + 90 * 16                 # kernel/sgcn.py:20
    assert tuple(model.conv2.lin.weight.shape) == (16, 32) and tuple(model.conv3.lin.weight.shape) == (5, 32)
    data = Batch.from_data_list(synth.brain_graph_list(2, seed=1, rois=90, top_k=3, tsne_dim=16, num_classes=2))
    with pytest.raises(ValueError, match="H_1=32 != H_2=16"):
        model(data)
    with pytest.raises(ValueError, match="H_1=32 != H_2=16"):
        model.forward_pair(data)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("explain", [False, True])
def test_fp64_restatement_matches_reference(golden, tag, mode, explain):
    """Bounds of test_sgcn_only_matches_reference: logp 1e-5, gradients 5e-4 (floor 1e-4); the tap and its gradient
    likewise."""
    store = golden("sgcn_ori")
    rois, dims, b_eval, b_train, seed, top_k = _cfg(store, tag)
    sd = _leaf_state(seeded_state(REF.param_shapes(*dims, rois=rois), seed))
    bsz = b_train if mode == "train" else b_eval
    data = _data64(synth.brain_graph_list(bsz, seed=seed + 10, rois=rois, top_k=top_k, tsne_dim=16, num_classes=2))
    taps = {}
    out = REF.model_forward(sd, rois, data, explain, training=(mode == "train"), taps=taps)
    sub = f"{tag}/{mode}/explain{int(explain)}"
    assert_matches(out, golden_group(store, sub + "/out")["logp"], 1e-5, "logp")
    (out * _probe([out], seed + 3)[0].double()).sum().backward()
    wg = golden_group(store, sub + "/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), 5e-4, "grad data.x")
    assert ("prob_bias" in wg) == explain and "conv2.bias" not in wg and "edge_prob" not in wg
    for k, w in wg.items():
        assert_matches(sd[k].grad, w, 5e-4, "grad " + k, floor=1e-4)
    cam = golden_group(store, sub + "/cam")
    assert_matches(taps["acts"], cam["final_conv_acts"], 1e-5, "final_conv_acts")
    assert_matches(taps["acts"].grad, cam["final_conv_grads"], 5e-4, "final_conv_grads")


@pytest.mark.parametrize("tag", TAGS)
def test_fp64_restatement_train_loss_matches_reference(golden, tag):
    """Bounds of test_sgcn_only_train_loss_matches_reference; after the two calls final_conv_acts is the masked pass's and
    final_conv_grads the plain pass's."""
    store = golden("sgcn_ori")
    rois, dims, b_eval, b_train, seed, top_k = _cfg(store, tag)
    sd = _leaf_state(seeded_state(REF.param_shapes(*dims, rois=rois), seed))
    data = _data64(synth.brain_graph_list(b_train, seed=seed + 10, rois=rois, top_k=top_k, tsne_dim=16, num_classes=2))
    taps = {"plain": {}, "masked": {}}
    loss, terms, _ = REF.train_losses(sd, rois, data, taps=taps)
    ref = float(store[f"{tag}/step/loss"])
    assert abs(float(loss) - ref) <= 1e-5 * max(1.0, abs(ref))
    for k, v in terms.items():
        assert abs(float(v) - float(store[f"{tag}/step/term/{k}"])) <= 1e-5, k
    loss.backward()
    wg = golden_group(store, f"{tag}/step/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), 5e-4, "grad data.x")
    for k, w in wg.items():
        assert_matches(sd[k].grad, w, 5e-4, "grad " + k, floor=1e-5)
    cam = golden_group(store, f"{tag}/step/cam")
    assert_matches(taps["masked"]["acts"], cam["final_conv_acts"], 1e-5, "final_conv_acts (masked pass)")
    assert_matches(taps["plain"]["acts"].grad, cam["final_conv_grads"], 5e-4, "final_conv_grads (plain pass)")


def test_lds_sizes_and_param_floats():
    from igcn_amd import _lib
    lib = _lib.load()
    for backward in (0, 1):
        assert 0 < lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 5, backward) <= 150 * 1024
    assert lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 5, 0) < lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 5, 1)
    # a width off the grid costs its next multiple of 4, not the next of 4 / 8 / 16 / 32: 5 stays far below 32
    assert lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 5, 1) <= lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 8, 1)
    assert lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 9, 1) > lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 8, 1)
    assert lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 5, 1) < lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 32, 1) - 30000
    assert lib.igcn_sgcn_ori_param_floats(3, 32, 5) == 32 * 3 + 32 + 5 * 32 + 5
    # its LDS sizes as they were before the staged-graph / gcn_norm layout moved to csrc/gcn_lds.h
    assert [lib.igcn_sgcn_ori_lds_bytes(90, 270, 3, 32, 5, b) for b in (0, 1)] == [36976, 79680]
    assert [lib.igcn_sgcn_ori_lds_bytes(7, 40, 3, 5, 10, b) for b in (0, 1)] == [2704, 10512]
    # the uniform stack keeps its LDS sizes (the values its build gave before this kernel existed)
    assert lib.igcn_sgcn_stack_lds_bytes(90, 270, 3, 16, 2, 0) == 30032
    assert lib.igcn_sgcn_stack_lds_bytes(90, 270, 3, 16, 2, 1) == 78528


def test_sgcn_ori_supported_refusals():
    from igcn_amd import ops
    plan = SimpleNamespace(_stack_dims=(90, 270))
    assert ops.sgcn_ori_supported(plan, 90, 3, 32, 5)
    assert ops.sgcn_ori_supported(plan, 90, 8, 5, 10)
    assert not ops.sgcn_ori_supported(plan, 90, 3, 64, 5)            # F1 = 64
    assert not ops.sgcn_ori_supported(plan, 90, 3, 32, 33)
    assert not ops.sgcn_ori_supported(plan, 90, 9, 32, 5)            # H0 = 9
    assert not ops.sgcn_ori_supported(plan, 80, 3, 32, 5)            # another graph size than the plan's
    assert not ops.sgcn_ori_supported(SimpleNamespace(), 90, 3, 32, 5)               # no per-graph plan
    assert not ops.sgcn_ori_supported(SimpleNamespace(_stack_dims=None), 90, 3, 32, 5)
    assert not ops.sgcn_ori_supported(SimpleNamespace(_stack_dims=(2000, 40000)), 2000, 3, 32, 32)   # does not fit LDS
