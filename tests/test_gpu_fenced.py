"""The existing fp64 / bit-exact oracles, run again under fenced, poisoned allocations (tests/fenced.py).

Every device buffer a kernel of this library touches is allocated in Python, and each allocation promises two things no
value test sees: the kernel writes no more than this (an overrun of a few words, or of one ragged tile, lands in the
caching allocator's 512-byte rounding or in a neighbouring block), and the kernel writes every element that is read or
returned later (a fresh ``torch.empty`` usually holds zeros, a recycled one the right answer of the previous call).

Each case of CASES names an existing test function (or one of the three small oracles of this module, for routes no
existing test takes) and ONE of its existing parameter tuples (and, where the test's
module keeps the kernels' RESULTS or a built model in a module-level dict, the name of that dict: it is emptied before
each of the two runs, so that both launch, and put back afterwards).  The function is imported
and called directly — with the ``ops`` module, a ``monkeypatch`` / ``tmp_path`` of its own and the fixtures of its module
— once plain and once inside ``fenced()``, both under ``calltrace.record_calls``.  Asserted:

* the fenced run passes the function's own assertions (``assert_matches`` rejects non-finite values and ``torch.equal``
  rejects NaN, so a returned word that nobody wrote fails as a value);
* every fence is intact (``fenced.check()``);
* both runs launched the same entry points with the same small arguments in the same order: the shim changes no route
  (``val_stride`` arguments excepted: ops.SparseMap passes the distance between two parameter tensors, an address);
* no CUDA allocation went past the shim except in the categories it counts (``fenced.passed``).

Left out, because the shim would not be exercised or the run would not be right under it:
* tests that start child processes (``test_attention_cores_are_deterministic_and_agree``, the ``*_variants_agree``
  tests, ``dp_*``): the patch does not reach the child;
* captured-graph tests: allocations under capture are passed through (the fills would become graph nodes);
* multi-device tests;
* the deferred-reduction tests that manage their own streams: the fills are ordered on the allocating stream only.
The bench-size tuples (3000-node hierarchy, 23040 rows, 70001 rows) are left out as well: every case takes seconds.

The last test is the coverage ledger: every line of ``ig-gcn_amd/*.py`` that holds one of the patched idioms was hit by
a fenced run of this module, or stands in EXEMPT with its reason.  A new op gets a case here.
"""
import importlib
import inspect
import os
import re
import sys

import pytest
import torch

from calltrace import record_calls
from fenced import fenced

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (20, 10, 6, 3, 1)
MID = (300, 120, 60, 19, 1)
ODD = (1801, 800, 300, 99, 1)


def _row(names, rows, cid, **more):
    """The tuple of ``rows`` whose first entry is ``cid``, as keyword arguments (``names``: the parametrize string)."""
    return lambda m: dict(zip(names.split(","), next(r for r in getattr(m, rows) if r[0] == cid)), **more)


OPS = "test_gpu_ops"
CASES = [
    # ------------------------------------------------------------------------------------------- test_gpu_ops.py
    (OPS, "test_graph_plan_bit_exact", dict(n=7, e=0, seed=0)),
    (OPS, "test_graph_plan_bit_exact", dict(n=90, e=270, seed=1)),
    (OPS, "test_edge_mask_fwd_bwd", dict(bsz=2, rois=17, h0=5, seed=2, deg=6)),
    (OPS, "test_gcn_layer_fwd_bwd", dict(n=12, e=40, fin=3, fout=16, loops=True, multi=True, seed=0)),
    (OPS, "test_gcn_layer_fwd_bwd", dict(n=64, e=500, fin=5, fout=7, loops=True, multi=True, seed=3)),
    (OPS, "test_gemm_nt_nn_tn", dict(m=5, n=7, k=9)),
    (OPS, "test_gemm_nt_nn_tn", dict(m=1000, n=33, k=130)),
    (OPS, "test_gemm_nt_nn_tn", dict(m=4100, n=48, k=48)),
    (OPS, "test_gemm_bf16_operands_fp32_accumulate", dict(m=100, n=37, k=50)),
    (OPS, "test_linear_fwd_bwd", dict(rows=9, fin=4, fout=2, relu=False, bias=True)),
    (OPS, "test_linear_fwd_bwd", dict(rows=130, fin=256, fout=4, relu=False, bias=False)),
    (OPS, "test_linear_fwd_bwd", dict(rows=1000, fin=7, fout=12, relu=True, bias=True)),
    (OPS, "test_linear_fwd_bwd", dict(rows=300, fin=5, fout=64, relu=True, bias=False)),
    (OPS, "test_head_inputs", dict(bsz=5, g=1, w=40, l=6, rois=4, use_prob=True, used=(0, 1, 1))),
    (OPS, "test_relu_owed_layer_and_head_inputs", dict(bsz=5, g=1, rois=12, d=16, l=10, use_prob=False)),
    (OPS, "test_relu_owed_layer_and_head_inputs", dict(bsz=3, g=2, rois=7, d=2, l=4, use_prob=True)),
    (OPS, "test_in_proj_packed_projection", dict(b=3, lq=7, lk=5, d=16)),
    (OPS, "test_in_proj_packed_projection", dict(b=6, lq=90, lk=40, d=32)),          # d = 32: igcn_proj_bwd_pair
    (OPS, "test_projected_attention_matches_multihead_attention", dict(b=3, lq=17, lk=70, d=32, h=4)),
    (OPS, "test_proj_bwd_one_pass", dict(m=4613, n=32, k=32)),
    (OPS, "test_proj_bwd_one_pass", dict(m=1000, n=96, k=48)),
    (OPS, "test_proj_fwd_streaming_pair", dict(m1=90, m2=400, kd=32)),
    (OPS, "test_proj_fwd_streaming_pair", dict(m1=1, m2=1, kd=48)),
    (OPS, "test_go_attention_layer", dict(bsz=4, pool=SMALL, fin=2, seed=0)),
    (OPS, "test_go_attention_layer", dict(bsz=5, pool=(40, 20, 9, 2, 1), fin=5, seed=2)),
    (OPS, "test_nodes_layernorm", dict(bsz=3, f=5, n=40, pool=20, with_keep=False)),
    (OPS, "test_nodes_layernorm", dict(bsz=4, f=2, n=257, pool=0, with_keep=True)),
    (OPS, "test_go_decoder_layer", dict(bsz=4, pool=SMALL, layer=0, seed=0)),
    (OPS, "test_go_decoder_layer", dict(bsz=4, pool=SMALL, layer=1, seed=1)),
    (OPS, "test_go_decoder_layer", dict(bsz=130, pool=MID, layer=0, seed=7)),
    (OPS, "test_go_attention_with_layernorm_backward_in_one_launch",
     dict(bsz=4, pool=SMALL, layer=0, with_keep=True, seed=0)),
    (OPS, "test_go_attention_with_layernorm_backward_in_one_launch",
     dict(bsz=2, pool=ODD, layer=0, with_keep=True, seed=5)),                 # 3001 nodes: the two-pass fallback
    (OPS, "test_go_decoder_with_layernorm_backward_in_one_launch",
     dict(bsz=4, pool=SMALL, layer=0, with_keep=True, seed=0)),
    (OPS, "test_go_decoder_with_layernorm_backward_in_one_launch",
     dict(bsz=2, pool=ODD, layer=1, with_keep=True, seed=6)),
    (OPS, "test_sparse_map_encode_decode", dict(bsz=4, pool=SMALL, seed=0, dense=False)),
    (OPS, "test_sparse_map_encode_decode", dict(bsz=4, pool=SMALL, seed=0, dense=True)),
    (OPS, "test_sparse_map_reads_channel_vectors_at_a_stride", {}),
    (OPS, "test_adam_matches_torch", {}),
    (OPS, "test_node_linear_bn", dict(bsz=6, f=5, n=11, d=5, training=True, groups=1)),
    (OPS, "test_node_linear_bn", dict(bsz=9, f=5, n=77, d=32, training=True, groups=1)),
    (OPS, "test_node_linear_bn", dict(bsz=12, f=2, n=130, d=1, training=True, groups=2)),
    (OPS, "test_node_linear_bn", dict(bsz=8, f=5, n=70, d=16, training=True, groups=2)),
    (OPS, "test_node_linear_bn", dict(bsz=6, f=5, n=77, d=32, training=False, groups=1)),
    (OPS, "test_batchnorm1d_grouped", dict(bsz=10, c=7, training=True, relu=False, groups=2)),
    (OPS, "test_batchnorm1d_grouped", dict(bsz=9, c=5, training=False, relu=True, groups=1)),
    (OPS, "test_batchnorm1d_grouped", dict(bsz=96, c=8, training=True, relu=True, groups=3)),
    (OPS, "test_batchnorm1d_grouped_without_relu_applies_the_dropout_factors", dict(p=0.7, groups=2, rows=33, c=5)),
    (OPS, "test_plan_replicate_equals_plan_of_the_doubled_graph", {}),
    (OPS, "test_segmented_rebuild_refills_the_replica_plan", {}),
    (OPS, "test_mask_regulariser", {}),
    (OPS, "test_stacked_masks_carry_the_regulariser", dict(bsz=3, rois=10, h0=3, deg=6, with_snps=False)),
    (OPS, "test_stacked_masks_carry_the_regulariser", dict(bsz=2, rois=17, h0=5, deg=6, with_snps=True)),
    (OPS, "test_gram_losses", dict(bsz=7, rd=40, soft=True)),
    (OPS, "test_gram_losses", dict(bsz=32, rd=300, soft=False)),
    (OPS, "test_gram_losses_grouped", {}),
    (OPS, "test_gram_loss_forward_prepares_the_backward_for_the_announced_upstream", {}),
    (OPS, "test_segmented_plan_is_bit_identical_to_the_sorted_plan", dict(n_graphs=8, seed=1)),
    (OPS, "test_segmented_plan_ragged_graphs_and_loops", {}),
    (OPS, "test_tiled_plan_is_bit_identical_to_a_stable_sort", dict(sizes=(90, 90), edges=(270, 4097))),
    (OPS, "test_propagate_dense_graph_variants", dict(hint=64)),
    (OPS, "test_propagate_lds_staged_dense_fwd_bwd", dict(g=3, r=64, f=16, density=1.0, cross=False)),
    (OPS, "test_propagate_lds_staged_dense_fwd_bwd", dict(g=2, r=130, f=8, density=1.0, cross=False)),
    (OPS, "test_attention_core", dict(bsz=3, lq=10, lk=9, d=8)),
    (OPS, "test_attention_core", dict(bsz=3, lq=7, lk=5, d=32)),
    (OPS, "test_attention_core", dict(bsz=2, lq=17, lk=130, d=32)),
    (OPS, "test_attention_core", dict(bsz=3, lq=21, lk=19, d=10)),
    (OPS, "test_attention_core", dict(bsz=2, lq=33, lk=50, d=24)),
    (OPS, "test_attention_core_bf16_operands", dict(bsz=1, lq=7, lk=5)),
    (OPS, "test_attention_core_bf16_operands", dict(bsz=3, lq=50, lk=37)),
    (OPS, "test_attention_core_split_bf16_vs_fp64", dict(bsz=1, lq=7, lk=5, amp=1.0)),
    (OPS, "test_attention_core_split_bf16_vs_fp64", dict(bsz=3, lq=37, lk=203, amp=1.0)),
    (OPS, "test_loss_head_matches_composite", {}),
    (OPS, "test_head_loss_one_launch_equals_heads_plus_loss_head",
     dict(b=37, k=64, c=3, nr=3, drop=True, upstream=1.0, lazy=False)),
    (OPS, "test_gemm_f32_batched", dict(m=70, n=33, k=131, batch=3, sk=2, form="nt")),
    (OPS, "test_gemm_f32_batched", dict(m=5, n=7, k=32, batch=4, sk=1, form="nn")),
    (OPS, "test_gemm_group_matches_single_products", dict(rows=70, fin=33, fout=5)),
    (OPS, "test_node_linear_bn_pair_matches_two_readouts", dict(groups=2, training=True)),
    (OPS, "test_small_linear_pair_matches_two_layers", {}),
    (OPS, "test_head_bwd_one_pass", dict(rows=37, k1=34, k2=70, relu=True)),
    (OPS, "test_linear_pair_matches_two_linears", {}),
    (OPS, "test_loss_head_from_scores_and_partials", {}),
    (OPS, "test_loss_head_forward_writes_the_unit_upstream_gradients", dict(from_logits=True)),
    (OPS, "test_graph_pool_mean_max_add", dict(g=7, r=13, d=5, seed=3)),
    (OPS, "test_fused_sgcn_stack_fwd_bwd", dict(g=3, r=10, h0=3, f=4, layers=2, deg=3, loops="some")),
    (OPS, "test_fused_sgcn_stack_fwd_bwd", dict(g=3, r=9, h0=3, f=16, layers=2, deg=3, loops="some")),
    (OPS, "test_front_kernel_equals_plan_build_mask_and_stack",
     dict(g=3, r=24, h0=1, f=8, layers=3, deg=4, loops="multi")),
    (OPS, "test_dropout_masks_one_launch", {}),
    (OPS, "test_dropout_masks_ride_in_the_plan_builds_launch", {}),
    (OPS, "test_grad_fan_sums_the_consumers_gradients_in_one_launch", {}),
    (OPS, "test_fused_stack_adds_a_second_consumers_gradient_on_load", {}),
    (OPS, "test_consumers_apply_the_dropout_factors", {}),
    # ------------------------------------------------------------------------------------------- the other op-level oracles
    ("test_gpu_gat", "test_gat_stack_vs_fp64_standin", dict(layers=3, hidden=10, h0=3)),
    ("test_gpu_gat", "test_model_vs_reference_golden", dict(name="gcn_imgsnp_gat", tag="l3h10")),
    ("test_gpu_gat", "test_model_vs_reference_golden", dict(name="gcn_imgsnp_gcn", tag="l3h10")),
    ("test_gpu_sgcn_gat", "test_gat_stack_edge_gradient_vs_fp64_standin", dict(layers=3, hidden=10, h0=3)),
    ("test_gpu_sgcn_gat", "test_stacked_pair_equals_two_passes", dict(layers=3, hidden=10)),
    ("test_gpu_sgcn_gat", "test_sgcn_gat_train_step_vs_reference_golden", dict(tag="l3h10", batched=True)),
    ("test_gpu_sgcn_gat", "test_sgcn_gat_train_step_vs_reference_golden", dict(tag="l3h10", batched=False)),
    ("test_gpu_sgcn_ori", "test_stack_kernels_vs_fp64", dict(widths=(3, 5, 10), kind="r7"), ("_STACK_CACHE",)),
    ("test_gpu_sgcn_ori", "test_stack_kernels_vs_fp64", dict(widths=(3, 32, 5), kind="r90x3"), ("_STACK_CACHE",)),
    ("test_gpu_sgcn_ori", "test_both_routes_vs_fp64_in_eval_mode", dict(route="per_layer", explain=True)),
    ("test_gpu_sgcn_ori", "test_sgcn_ori_train_step_vs_reference_golden", dict(tag="h16_8", batched=True)),
    ("test_gpu_dense", "test_dense_sgcn_vs_fp64_oracle", dict(mode="both", rois=64, n_graphs=3, layers=2)),
    ("test_gpu_guide", "test_nodes_ln_prelu_vs_fp64", dict(a=-0.3)),
    ("test_gpu_guide", "test_bn_prelu_vs_fp64", dict(a=-0.3, f=5)),
    ("test_gpu_guide", "test_bn_prelu_vs_fp64", dict(a=0.25, f=0)),
    ("test_gpu_guide", "test_node_linear_bn_prelu_wide_forward_vs_fp64", {}),
    ("test_gpu_guide", "test_gate_encoder_vs_fp64", dict(training=True)),
    ("test_gpu_guide", "test_model_train_vs_reference_golden", dict(tag="h10")),
    ("test_gpu_guide_oracle", "test_model_train_vs_fp64_oracle", dict(tag="h10_b32"), ("_SETUP",)),
    ("test_gpu_guide_oracle", "test_model_eval_vs_fp64_oracle", dict(tag="h10_b32"), ("_SETUP",)),
    ("test_gpu_snps", "test_snps_head_loss_vs_fp64", dict(b=30, l=5)),
    ("test_gpu_snps", "test_snps_head_loss_autograd_function", {}),
    ("test_gpu_snps", "test_model_vs_reference_golden", dict(tag="main20", mode="train", route="fused")),
    ("test_gpu_snps", "test_model_vs_reference_golden", dict(tag="main20", mode="train", route="unfused")),
    ("test_gpu_snps", "test_evaluation_against_host_metrics", {}),
    ("test_gpu_clusterlabel", "test_cluster_head_loss_vs_fp64", dict(b=33, k=4)),
    ("test_gpu_clusterlabel", "test_cluster_head_loss_autograd_function", dict(predict=True, lazy=False)),
    ("test_gpu_clusterlabel", "test_mask_reg3_vs_fp64", dict(n_snps=1, n_prob=270, n_edge=257)),
    ("test_gpu_clusterlabel", "test_mask_regulariser3_autograd_function", {}),
    ("test_gpu_clusterlabel", "test_train_step_vs_reference_golden", dict(tag="h0_3", route="fused")),
    ("test_gpu_clusterlabel", "test_train_step_vs_reference_golden", dict(tag="h0_1", route="unfused")),
    ("test_gpu_head_loss", "test_loss_head_vs_fp64",
     _row("cid,b,c,nr,s,lam_name,amp,offset", "LOSS_HEAD_CASES", "scalar_walk", from_logits=True)),
    ("test_gpu_head_loss", "test_head_loss_vs_fp64",
     _row("cid,b,k,c,nr,s,keep,lam_name", "HEAD_LOSS_CASES", "k16_ragged", lazy=False)),
    ("test_gpu_head_loss", "test_paired_head_loss_and_gram_launch_vs_fp64",
     _row("cid,b,k,c,nr,s,keep,lam_name", "PAIRED", "k64_ragged")),
    ("test_gpu_readout_wide", "test_wide_node_linear_bn_vs_fp64", dict(bsz=9, n=77, d=96, training=True, groups=1),
     ("_REF",)),
    ("test_gpu_readout_wide", "test_wide_node_linear_bn_vs_fp64", dict(bsz=2, n=33, d=160, training=True, groups=2),
     ("_REF",)),
    ("test_gpu_attn_wide", "test_attention_core_wide_vs_fp64", dict(d=66, h=2, bsz=2, lq=7, lk=5)),
    ("test_gpu_attn_wide", "test_attention_core_wide_vs_fp64", dict(d=192, h=4, bsz=2, lq=40, lk=70)),
    ("test_gpu_attn_wide", "test_projected_attention_wide_vs_fp64", dict(d=96, b=3, lq=90, lk=130)),
    ("test_gpu_hidden32", "test_hidden32_vs_oracle", dict(layers=2)),
    ("test_gpu_hidden32", "test_hidden32_train_mode_vs_oracle", {}),
    ("test_gpu_map_fused", "test_readout_apply_and_decode_map_as_one_launch_bit_for_bit",
     dict(groups=2, with_keep=True, training=True)),
    ("test_gpu_attn_weights", "test_kernel_vs_fp64", dict(case="unaligned_rows", b=3)),
    ("test_gpu_attn_weights", "test_map_accumulate_vs_numpy", {}),
    ("test_gpu_attn_weights", "test_model_vs_fp64", dict(layers=4, hidden=5)),
    ("test_gpu_attn_weights", "test_attention_maps_vs_fp64", {}),
    ("test_gpu_rollout", "test_coeffs_vs_fp64", dict(fin=5, b=3)),
    ("test_gpu_rollout", "test_two_layers_and_the_product_vs_fp64", dict(b=3)),
    ("test_gpu_rollout", "test_final_product_vs_fp64", dict(rois=7, n_top=13)),
    ("test_gpu_rollout", "test_model_vs_fp64", dict(explain=True)),
    ("test_gpu_rollout", "test_association_maps_vs_per_batch_means", {}),
    ("test_gpu_connectivity", "test_dense_map_bit_for_bit", dict(name="odd")),
    ("test_gpu_connectivity", "test_edge_importance_vs_fp64_oracle", dict(kind="imgsnp", rois=7, h0=3)),
    ("test_gpu_connectivity", "test_gat_stack_alpha_vs_fp64", dict(f=4, layers=3, rois=5, h0=1)),
    ("test_gpu_connectivity", "test_sgcn_gat_attention_vs_restatement", dict(explain=True, hidden=10)),
    ("test_gpu_connectivity", "test_connectivity_maps_from_the_masks", dict(weighted=True, symmetric=True)),
    ("test_gpu_connectivity", "test_connectivity_maps_from_the_gat_attention", dict(explain=False, symmetric=True)),
    ("test_gpu_saliency", "test_saliency_maps_kernel_vs_restatement", dict(b=3, r=90, h0=3, m=1, base_form="rois")),
    ("test_gpu_saliency", "test_grad_cam_kernel_vs_restatement", dict(b=2, r=90, k=33)),
    ("test_gpu_saliency", "test_sgcn_gcn_saliency_and_ig_vs_oracle", dict(explain=True)),
    ("test_gpu_saliency", "test_sgcn_ori_saliency_and_grad_cam_vs_oracle", dict(explain=False)),
    ("test_gpu_saliency", "test_imgsnp_saliency_vs_oracle", dict(explain=True)),
    ("test_gpu_saliency", "test_imgsnp_integrated_gradients_over_both_modalities", {}),
    ("test_gpu_saliency", "test_saliency_maps_over_a_ragged_loader", dict(case="gradcam")),
    ("test_gpu_saliency", "test_input_saliency_is_the_tested_input_gradient_times_x", dict(kind="imgsnp", explain=True)),
    ("test_gpu_saliency", "test_input_saliency_is_the_tested_input_gradient_times_x", dict(kind="sgcn_gcn", explain=False)),
    ("test_gpu_sgcn_ori", "test_gradient_on_acts_joins_at_the_tap", {}, ("_STACK_CACHE",)),
    ("test_gdc", "test_gdc_kernel_vs_reference_golden", {}),
    ("test_gdc", "test_gdc_batch_vs_oracle", dict(bsz=7, rois=40, k=5)),
    ("test_gpu_feeders", "test_one_launch_gather_equals_from_data_list", {}),
    ("test_gpu_feeders", "test_feeder_hands_over_every_subject_once_per_epoch", dict(kind="device")),
    ("test_gpu_feeders", "test_dense_feeder_equals_the_pre_transform_of_the_drawn_subjects", {}),
    ("test_gpu_epoch", "test_literal_train_body_with_torch_adam_vs_reference_golden", {}),
    ("test_gpu_clusterlabel", "test_train_step_vs_reference_golden", dict(tag="nopredict", route="unfused")),
    ("test_gpu_knn_impute", "test_kernel_matches_the_restatement", dict(shape=(37, 11, 9, 3))),
    ("test_gpu_knn_impute", "test_index_route_gives_the_bits_of_the_dense_call", {}),
    ("test_gpu_knn_impute", "test_knn_imputer_class", {}),
    ("test_gpu_knn_impute", "test_end_to_end_lists_store_batch_and_step", {}),
    ("test_gpu_cluster_labels", "test_sqdist_and_joint_p", dict(shape=(65, 12))),
    ("test_gpu_cluster_labels", "test_gradient_z_kl_and_update", dict(shape=(65, 12))),
    ("test_gpu_cluster_labels", "test_kmeans_from_a_given_init", dict(shape=(65, 270, 2))),
    ("test_gpu_cluster_labels", "test_kmeans_plusplus_indices", dict(case=((96, 2, 3), 3))),
    ("test_gpu_cluster_labels", "test_cluster_labels_recover_blobs", dict(blob=(3, 37, 5, 8.0, 0))),
    ("test_gpu_cluster_labels", "test_wss_curve_decreases", {}),
    ("test_gpu_cluster_labels", "test_label_store_batch_and_train_step", {}),
    ("test_gpu_eval", "test_evaluate_matches_the_eager_eval_functions_and_the_oracle", dict(classes=2, regr=4)),
    ("test_gpu_eval", "test_device_metrics_match_the_restatement", dict(classes=2, regr=4, nan_target=2)),
    ("test_gpu_eval", "test_metrics_kernel_on_many_rows", dict(n=257, C=2, case="nan_score")),
    ("test_gpu_fenced", "_linear_pair_of_two_widths", {}),
    ("test_gpu_fenced", "_gcn_norm_with_one_upstream_absent", {}),
    ("test_gpu_fenced", "_dense_sgcn_regulariser_alone", {}),
    # ------------------------------------------------------------------------------------------- eager train steps
    ("test_gpu_model", "test_go_network_vs_reference_golden", dict(name="go_tiny", mode="train", maps="default")),
    ("test_gpu_model", "test_go_network_vs_reference_golden", dict(name="go_tiny", mode="train", maps="csr")),
    ("test_gpu_model", "test_full_model_vs_reference_golden", dict(name="var_graph_pool", mode="train", explain=True)),
    ("test_gpu_model", "test_full_model_vs_reference_golden", dict(name="var_snps_only", mode="train", explain=False)),
    ("test_gpu_model", "test_train_step_vs_reference_golden", dict(name="full_tiny", batched=True)),
    ("test_gpu_model", "test_train_step_vs_reference_golden", dict(name="full_tiny", batched=False)),
    ("test_gpu_model", "test_train_step_vs_reference_golden", dict(name="var_image_only", batched=True)),
    ("test_gpu_model", "test_sgcn_only_train_step_vs_reference_golden", dict(batched=True)),
    ("test_gpu_model", "test_full_model_dense_graphs_vs_oracle", dict(rois=96, bsz=4)),
    ("test_gpu_model", "test_eval_passes_vs_oracle", {}),
    # heads of two widths (2 classes, 4 scores): ops.LinearPair's backward takes one bias-gradient launch per head
    ("test_gpu_model", "test_train_mode_at_the_trainers_heads_vs_oracle", dict(case="trainer")),
    # the latent MLP's wide layer takes ops.LinearBN1d only when its product is split: K >= 128 inputs, a 1800-node pool
    ("test_gpu_model", "test_full_model_vs_oracle_larger", dict(bsz=16, pool=(1800, 800, 300, 99, 1), explain=True)),
    # ------------------------------------------------------------------------------------------- dense-block forms
    # (appended: the ids of the cases whose parameters come from a table carry their position in this list)
    # the pipelined form | odd R / 64 with 12 rows of `dup` in the backward workspace | L = 4 with H0 = 1
    ("test_gpu_dense_forms", "test_dense_forms_vs_fp64_oracle", dict(rois=256, n_graphs=2, layers=2, h0=3, mode="both")),
    ("test_gpu_dense_forms", "test_dense_forms_vs_fp64_oracle", dict(rois=192, n_graphs=8, layers=2, h0=3, mode="both")),
    ("test_gpu_dense_forms", "test_dense_forms_vs_fp64_oracle", dict(rois=128, n_graphs=2, layers=4, h0=1, mode="masked")),
]

# ------------------------------------------------------------------------------------------- routes no existing test takes
def _linear_pair_of_two_widths():
    """ops.linear_pair with first layers of DIFFERENT widths (12 and 64 outputs over 34 and 70 inputs, 37 rows): the
    backward takes one igcn_bias_grad launch per head, each with its own mask, bias gradient and scratch.  No model builds
    such a pair, so no oracle test reaches the route.  Against float64 at test_gpu_ops.py's 1e-4 (fp32 dot products of
    at most 70 terms: K * 2^-24 = 4e-6 of the sum of magnitudes)."""
    import numpy as np
    from conftest import assert_matches
    from igcn_amd import ops
    rng = np.random.default_rng(12)
    t = lambda *shape: torch.from_numpy(rng.standard_normal(shape)).float()            # noqa: E731
    host = [t(37, 34), t(12, 34) / 6, t(12), t(37, 70), t(64, 70) / 8, t(64)]
    c1, c2 = t(37, 12), t(37, 64)
    dev = [v.cuda().requires_grad_(True) for v in host]
    y1, y2 = ops.linear_pair(*dev, relu=True)
    got = torch.autograd.grad((y1 * c1.cuda()).sum() + (y2 * c2.cuda()).sum(), dev)
    ref = [v.double().requires_grad_(True) for v in host]
    z1 = torch.relu(ref[0] @ ref[1].t() + ref[2])
    z2 = torch.relu(ref[3] @ ref[4].t() + ref[5])
    want = torch.autograd.grad((z1 * c1.double()).sum() + (z2 * c2.double()).sum(), ref)
    assert_matches(y1, z1.detach().numpy(), 1e-4, "y1")
    assert_matches(y2, z2.detach().numpy(), 1e-4, "y2")
    for g, w, name in zip(got, want, ("dx1", "dw1", "db1", "dx2", "dw2", "db2")):
        assert_matches(g, w.numpy(), 1e-4, name)


def _gcn_norm_with_one_upstream_absent():
    """ops.GcnNorm when the loss reads only one of (what, what_loop): the backward stands a zeros tensor in for the absent
    gradient.  Exactly the bits of the backward that is handed explicit zeros (the values themselves:
    test_gcn_layer_fwd_bwd)."""
    import numpy as np
    from igcn_amd import ops
    from test_gpu_ops import _rand_graph
    rng = np.random.default_rng(3)
    ei, w = _rand_graph(rng, 64, 500, loops=True, multi_loops=True)
    plan = ops.GraphPlan(ei.cuda(), 64)
    for absent in (0, 1):
        ew = w.cuda().requires_grad_(True)
        outs = ops.GcnNorm.apply(ew, plan)[:2]
        cot = [torch.from_numpy(rng.standard_normal(tuple(o.shape))).float().cuda() for o in outs]
        cot[absent].zero_()
        want, = torch.autograd.grad(outs, ew, grad_outputs=cot, retain_graph=True)
        got, = torch.autograd.grad(outs[1 - absent], ew, grad_outputs=cot[1 - absent])
        assert bool(torch.isfinite(got).all()) and bool(got.abs().max() > 0) and torch.equal(got, want), absent


def _dense_sgcn_regulariser_alone():
    """ops.DenseSgcn (masked pass, 2 complete graphs of 64 ROIs, one layer) under a loss that reads the mask regulariser
    only: the backward stands a zeros tensor in for xcat's absent gradient.  Exactly the bits of the backward that is
    handed explicit zeros (the values themselves: test_dense_sgcn_vs_fp64_oracle)."""
    import numpy as np
    from igcn_amd import ops
    from test_gpu_dense import _batch
    rng = np.random.default_rng(65)
    rois, h0, f = 64, 3, 16
    b = _batch(2, rois, seed=rois).to("cuda")
    plan = ops.plan_for(b)
    assert plan.dense_blocks and ops.dense_sgcn_supported(plan, rois, h0, f, 1)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s)).float().cuda()                 # noqa: E731
    host = [b.x.clone(), t(rois, h0) * 0.7, t(2 * h0, 1) * 0.8, t(1, 54), t(f, h0) * 0.6, t(f) * 0.2]
    got = []
    for explicit in (False, True):
        x, prob, pb, sp, w, bias = leaves = [v.clone().requires_grad_(True) for v in host]
        xcat, regp = ops.DenseSgcn.apply(x, b.edge_attr, prob, pb, sp, "masked", rois, (0.1, 0.3, 0.2, 0.15, 1e-6), None,
                                         w, bias)
        loss = 0.37 * regp.sum() + ((xcat * torch.zeros_like(xcat)).sum() if explicit else 0.0)
        got.append(torch.autograd.grad(loss, leaves, allow_unused=True))
    assert bool(torch.isfinite(got[0][0]).all()) and bool(got[0][1].abs().max() > 0)
    for name, a, e in zip(("dx", "dprob", "dprob_bias", "dsnps_prob", "dW", "db"), *got):
        assert (a is None) == (e is None) and (a is None or torch.equal(a, e)), name


# Lines of ig-gcn_amd/*.py that hold a patched idiom and that no fenced case reaches, one reason each.  The admissible
# reasons: capture-only path | multi-device path | CPU-side tensor | child-process-only switch | a route above a stated
# size threshold.  Two more kinds stand here, named as what they are, because no case CAN make the shim check them:
# a ``zeros`` that stands in for an absent upstream gradient (the kernel only READS it, fences see writes, and the
# kernel itself runs fenced in the case that has the gradient), and a zero-dim scalar that no kernel is handed.
_CPU = "CPU-side tensor: "
_PARAM = _CPU + "a module's constructor builds its parameters on the host; .to(device) / .cuda() moves them"
_ABSENT = ("absent upstream gradient: a zeros operand the backward kernel only reads; that kernel's outputs and scratch "
           "are fenced by the case that has the gradient: ")
EXEMPT = {
    "ig-gcn_amd/capture.py:78": "capture-only path: the captured step's own copy of FlatAdam's pointer table",
    "ig-gcn_amd/data.py:102": _CPU + "Batch.from_data_list builds the batch vector on the host",
    "ig-gcn_amd/gcn_img_snp.py:46": _PARAM, "ig-gcn_amd/gcn_img_snp.py:47": _PARAM,
    "ig-gcn_amd/gcn_img_snp.py:49": _PARAM, "ig-gcn_amd/gcn_img_snp.py:50": _PARAM,
    "ig-gcn_amd/go_model.py:66": _PARAM, "ig-gcn_amd/go_model.py:67": _PARAM,
    "ig-gcn_amd/sgcn.py:58": _PARAM, "ig-gcn_amd/sgcn.py:59": _PARAM, "ig-gcn_amd/sgcn.py:60": _PARAM,
    "ig-gcn_amd/sgcn.py:215": _PARAM, "ig-gcn_amd/sgcn.py:216": _PARAM, "ig-gcn_amd/sgcn.py:217": _PARAM,
    "ig-gcn_amd/sgcn_img_snp.py:33": _PARAM, "ig-gcn_amd/sgcn_img_snp.py:214": _PARAM,
    "ig-gcn_amd/sgcn_img_snp.py:215": _PARAM, "ig-gcn_amd/sgcn_img_snp.py:216": _PARAM,
    "ig-gcn_amd/sgcn_img_snp.py:217": _PARAM,
    "ig-gcn_amd/ops.py:1808": _CPU + "Csr builds its row pointers on the host before the upload",
    "ig-gcn_amd/ops.py:1811": _CPU + "Csr builds its transposed row pointers on the host before the upload",
    "ig-gcn_amd/ops.py:1814": _CPU + "Csr pads an empty host index list before the upload",
    "ig-gcn_amd/ops.py:1830": _CPU + "the GO attention walk order is laid out in a host buffer, then uploaded",
    "ig-gcn_amd/train.py:116": _CPU + "FlatAdam's pinned host copies of the pointer table",
    "ig-gcn_amd/train.py:1500": _CPU + "eval_scores_of works on .cpu() copies of the evaluation's rows",
    "ig-gcn_amd/ops.py:670": _ABSENT + "test_front_kernel_equals_plan_build_mask_and_stack",
    "ig-gcn_amd/ops.py:3525": _ABSENT + "test_gate_encoder_vs_fp64 (test_gpu_guide.py)",
    "ig-gcn_amd/saliency.py:131": _ABSENT[:24] + ": a zeros stand-in for an input the model does not read, returned, no kernel",
    "ig-gcn_amd/snps.py:99": "no kernel operand: the zero-dim reconstruction term of the unfused route when lambda0 == 0.0; "
                             "composed by torch, handed to no kernel",
    "ig-gcn_amd/train.py:592": "no kernel operand: a zero-dim placeholder taken once per process (whichever test first "
                               "runs a train step), only its device, dtype and shape are read",
}

IDIOM = re.compile(r"\btorch\.(empty|empty_like|zeros|zeros_like|full)\(|\.new_(empty|zeros)\(")
_HIT, _RAN, _FIXTURES, _ADDRESS_ARGS = set(), set(), {}, {}


def _params(case, mod):
    return case[2](mod) if callable(case[2]) else dict(case[2])


def _case_id(case):
    p = case[2]
    mod = case[0][9:] if case[0].startswith("test_gpu_") else case[0][5:]
    if callable(p):
        return f"{mod}.{case[1][5:]}[{CASES.index(case)}]"
    if not case[1].startswith("test_"):
        return "own." + case[1].lstrip("_")
    return f"{mod}.{case[1][5:]}[" + "-".join(str(v).replace(" ", "") for v in p.values()) + "]"


def _is_existing_tuple(fn, params):
    """Every parametrize mark of ``fn`` holds the tuple that ``params`` gives its argument names."""
    left = set(params)
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [n.strip() for n in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        rows = []
        for r in mark.args[1]:
            values = r.values if hasattr(r, "marks") and hasattr(r, "values") else (r if len(names) > 1 else (r,))
            rows.append(tuple(values))
        want = tuple(params[n] for n in names)
        if not any(tuple(r) == want for r in rows):
            return False
        left -= set(names)
    return not left


def _fixture(mod, name, request):
    """A fixture of the test's own module (``first_layer``), built once; else one of conftest's (``golden``)."""
    obj = getattr(mod, name, None)
    if obj is None:
        return request.getfixturevalue(name)
    if (mod.__name__, name) not in _FIXTURES:
        make = obj._get_wrapped_function() if hasattr(obj, "_get_wrapped_function") else getattr(obj, "__wrapped__", obj)
        _FIXTURES[(mod.__name__, name)] = make()
    return _FIXTURES[(mod.__name__, name)]


def _address_args():
    """{entry point: positions in a recorded call} of the ``val_stride`` parameters declared in include/igcn.h: the floats
    between the per-channel value vectors, which for separately allocated parameters is a difference of addresses."""
    if not _ADDRESS_ARGS:
        with open(os.path.join(ROOT, "include", "igcn.h")) as fh:
            text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
        for name, args in re.findall(r"\b(igcn_\w+)\s*\(([^;{]*?)\)\s*;", text):
            at = [i + 1 for i, a in enumerate(args.split(",")) if a.split() and a.split()[-1].lstrip("*") == "val_stride"]
            if at:
                _ADDRESS_ARGS[name] = at
        assert "igcn_image_put" in _ADDRESS_ARGS
    return _ADDRESS_ARGS


def _routes(seen):
    masked = _address_args()
    return [tuple("*" if i in masked.get(c[0], ()) else a for i, a in enumerate(c)) for c in seen]


def _run(case, request, tmp_path, shim):
    from igcn_amd import ops
    mod = importlib.import_module(case[0])
    fn = getattr(mod, case[1])
    params = _params(case, mod)
    kept = {name: dict(getattr(mod, name)) for name in (case[3] if len(case) > 3 else ())}
    try:
        for name in kept:
            getattr(mod, name).clear()
        return _call(fn, mod, params, request, tmp_path, shim, ops)
    finally:
        for name, saved in kept.items():
            getattr(mod, name).clear()
            getattr(mod, name).update(saved)


def _call(fn, mod, params, request, tmp_path, shim, ops):
    with pytest.MonkeyPatch.context() as mp:
        args = {}
        for name in inspect.signature(fn).parameters:
            if name in params:
                args[name] = params[name]
            elif name == "ops":
                args[name] = ops
            elif name == "monkeypatch":
                args[name] = mp
            elif name == "tmp_path":
                args[name] = tmp_path / ("fenced" if shim else "plain")
                args[name].mkdir()
            else:
                args[name] = _fixture(mod, name, request)
        from igcn_amd import _lib, gdc  # noqa: F401  (gdc: imported before the patch, or it would keep the patched name)
        real = _lib.call
        seen = record_calls(mp)
        for name, m in list(sys.modules.items()):           # gdc, comm: their own imported name of _lib.call
            if name.startswith("igcn_amd.") and getattr(m, "call", None) is real:
                mp.setattr(m, "call", _lib.call)
        if not shim:
            fn(**args)
            return seen, None
        with fenced() as f:
            fn(**args)
        return seen, f


def test_every_case_names_an_existing_parameter_tuple():
    bad = []
    for case in CASES:
        mod = importlib.import_module(case[0])
        if not _is_existing_tuple(getattr(mod, case[1]), _params(case, mod)):
            bad.append(_case_id(case))
    assert not bad, bad
    assert len({_case_id(c) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_oracle_passes_inside_fences(case, request, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()
    plain, _ = _run(case, request, tmp_path, shim=False)
    inside, f = _run(case, request, tmp_path, shim=True)          # raises on the oracle's own assertions or on a breach
    plain, inside = _routes(plain), _routes(inside)
    assert inside, "the fenced run launched nothing: it checked nothing"
    first = next((i for i, (a, b) in enumerate(zip(plain, inside)) if a != b), min(len(plain), len(inside)))
    assert plain == inside, (f"the fenced run took another route: {len(plain)} / {len(inside)} launches, first "
                             f"difference at {first}: {plain[first:first + 1]} vs {inside[first:first + 1]}")
    assert f.passed["other"] == 0, f.other_sites
    # everything on the GPU that was not fenced falls in a counted category; a run that fenced nothing checked nothing
    assert f.records, "no allocation went through the shim"
    _HIT.update(s for s in f.sites if s.startswith("ig-gcn_amd" + os.sep))
    _RAN.add(_case_id(case))


def _sites():
    out = {}
    pkg = os.path.join(ROOT, "ig-gcn_amd")
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as fh:
                for no, line in enumerate(fh, 1):
                    if IDIOM.search(line.split("#")[0]):
                        out[f"ig-gcn_amd/{name}:{no}"] = line.strip()
    return out


def test_exemptions_name_real_sites_and_give_a_reason():
    sites = _sites()
    assert not [s for s in EXEMPT if s not in sites], "exempt lines that hold no allocation idiom (the file moved on?)"
    assert all(len(r.strip()) > 10 for r in EXEMPT.values())


def test_ledger_every_allocation_site_is_fenced_or_exempt():
    if _RAN != {_case_id(c) for c in CASES}:
        pytest.skip("the ledger needs every fenced case of this module in the same session")
    sites = _sites()
    missing = sorted(s for s in sites if s not in _HIT and s not in EXEMPT)
    stale = sorted(s for s in EXEMPT if s in _HIT)
    print(f"ledger: {len(sites)} sites, {len(_HIT & set(sites))} hit, {len(EXEMPT)} exempt")
    assert not missing, "allocation sites no fenced case reached (add a case, or an exemption with its reason):\n" + \
        "\n".join(f"  {s}: {sites[s]}" for s in missing)
    assert not stale, f"exempt sites that a fenced case does reach: {stale}"
