"""What the warm-up steps of a captured step change and its constructor must put back (igcn_amd/capture.py): clones of
it, taken before the construction, and the comparison after it."""
import torch


def rollback_state(model, opt):
    """({name: clone}, ``_has_state``) of the optimiser's flat state, every module buffer and the counter of every mask
    generator reachable from ``model``."""
    from igcn_amd import ops
    tensors = {k: getattr(opt, k) for k in ("flat", "exp_avg", "exp_avg_sq", "step_count")}
    tensors.update({"buffer " + k: b for k, b in model.named_buffers()})
    tensors.update({f"generator {name}.{k}".replace(" .", " "): v.state for name, m in model.named_modules()
                    for k, v in vars(m).items() if isinstance(v, ops.DropoutState)})
    return {k: t.detach().clone() for k, t in tensors.items()}, list(opt._has_state)


def assert_rolled_back(model, opt, before):
    (want, has), (got, has_now) = before, rollback_state(model, opt)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k, t in got.items():
        assert torch.equal(t, want[k]), k
    assert has_now == has


def graphed_train_step_case(two_graphs):
    """``train.GraphedTrainStep`` on a small SGCN_GCN_IMGSNP with every dropout ON, after one eager step (non-zero Adam
    moments, a live mask generator, parameters the loss does not reach still without state): its construction leaves no
    trace.  ``two_graphs``: ``distributed=True, world_size=1`` on a single-rank process group of this process's own."""
    import os
    import igcn_amd  # noqa: F401
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    from igcn_amd.train import FlatAdam, GraphedTrainStep, train_step
    if two_graphs:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29578")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(0)
        torch.distributed.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    go_snps, adj, pool_dim = synth.go_hierarchy((60, 30, 20, 9, 1), seed=2)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    torch.manual_seed(3)
    model = SGCN_GCN_IMGSNP(2, 8, a_g, a, pool_dim, 32, "cuda", rois=90, H_0=3, num_classes=3, isSoftSimilarity=True,
                            rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseProb4Regr=True, isImageOnly=False,
                            isSNPsOnly=False).cuda().train()
    assert model._dropout_enabled and model.go_network._dropout_enabled
    lam = [1.0, 1.0, 0.5, 1.5e-6, 0.1, 0.2]
    opt = FlatAdam(model.parameters(), lr=1e-3)
    train_step(model, opt, Batch.from_data_list(synth.brain_graph_list(6, seed=50, rois=90, tsne_dim=16)).to("cuda"), lam)
    static = Batch.from_data_list(synth.brain_graph_list(6, seed=51, rois=90, tsne_dim=16)).to("cuda")
    static.x.requires_grad_(True)
    before = rollback_state(model, opt)
    assert "generator go_network._drop_state" in before[0] and bool(before[0]["exp_avg"].any())
    assert any(before[1]) and not all(before[1])
    kw = dict(distributed=True, world_size=1) if two_graphs else {}
    step = GraphedTrainStep(model, opt, static, lam, warmup=2, **kw)
    assert (step.g_opt is not None) == two_graphs and step.g_rest is None
    assert_rolled_back(model, opt, before)
    if two_graphs:
        torch.distributed.destroy_process_group()
