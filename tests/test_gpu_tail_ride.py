"""The gene read-out whose launches carry the latent MLP's BatchNorm stages (ops.GeneTail, igcn_gene_tail_*) against the
separate ops it replaces (ops.NodeLinearBN with its map rider, ops.LinearBN1d / ops.linear + ops.BatchNorm1dGrouped).

The passengers run the same kernel bodies on the same operands in other workgroups, so everything must be EQUAL bit for
bit (``torch.equal``): outputs, saved statistics, running statistics after one and two steps, every gradient.  The model's
own routing code runs (``Gene_ontology_network._gene_tail`` with ``tail_ride`` on and off) on a stand-in that holds just
the modules that method reads, so that the map can have three rows (the model's has the 54 SNPs).

Shapes: the smallest at which each path exists — N = 40 nodes, J = 3 map rows, nnz = 30 (> 8 J: the fused apply-and-map
launch), n_top = 5 read-out inputs, hidden 32, l_dim = 4 (the second product on the narrow-output kernel; l_dim = 8: on
the GEMM), B = 8 in 2 groups.  Every host grid here (1 x 2 statistics workgroups, 8 apply-and-map workgroups) is smaller
than the 32 passengers in front of it.  A 3 x 8 map has 24 cells, not the 25 the fused launch asks for (nnz > 8 J), so
the case of one partly filled node block takes N = 11, the smallest N with 30 distinct cells in three rows.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

STATS = {"NodeLinearBNBackward": ((4, 5),), "BatchNorm1dGroupedBackward": ((3, 4),), "LinearBN1dBackward": ((5, 6),),
         "GeneTailBackward": ((4, 5), (12, 13), (20, 21))}


def _tail(n, j, nnz, n_top, hidden, l_dim, seed):
    """A Gene_ontology_network that holds only what ``_gene_tail`` reads: the D = 1 read-out, its map, the latent MLP."""
    from igcn_amd import ops
    from igcn_amd.go_model import Gene_ontology_network
    rng = np.random.default_rng(seed)
    cells = np.sort(rng.permutation(j * n)[:nnz])            # row-major, unique (ops.Csr)
    net = Gene_ontology_network.__new__(Gene_ontology_network)
    nn.Module.__init__(net)
    net.gene_t_csr = ops.Csr(torch.from_numpy(cells // n), torch.from_numpy(cells % n), j, n, "cuda")
    t = lambda *s: torch.from_numpy(rng.standard_normal(s)).float()                     # noqa: E731
    lin = lambda i, o: nn.Linear(i, o, bias=False)                                      # noqa: E731
    net.t_D = nn.ParameterList([nn.Parameter(1.0 + 0.1 * t(nnz))])
    net.conc_D = lin(2, 1)
    net.B_D = nn.Sequential(nn.BatchNorm1d(n), nn.ReLU(), nn.Dropout(0.5))
    net.latent = nn.Sequential(lin(n_top, hidden), nn.BatchNorm1d(hidden), nn.ReLU(), nn.Dropout(0.5),
                               lin(hidden, l_dim), nn.BatchNorm1d(l_dim), nn.ReLU())
    with torch.no_grad():
        for p in net.parameters():
            if p is not net.t_D[0]:
                p.copy_(t(*p.shape) * 0.5 + (1.0 if p.dim() == 1 else 0.0))
        for m in net.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.copy_(t(*m.running_mean.shape) * 0.1)
                m.running_var.copy_(1.0 + 0.2 * t(*m.running_var.shape).abs())
    return net.cuda()


def _inputs(b, n, n_top, hidden, seed, keep_h=True):
    rng = np.random.default_rng(seed + 100)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s)).float().cuda()              # noqa: E731
    keep = lambda *s: torch.from_numpy((rng.random(s) < 0.5) * 2.0).float().cuda()      # noqa: E731
    masks = {"out_d": keep(b, n), "h": keep(b, hidden) if keep_h else None}
    return t(b, 2, n), t(b, n_top).abs(), masks


def _saved_stats(roots):
    """{channels: (mean, rstd)} of every BatchNorm behind ``roots``, off the autograd nodes' saved tensors."""
    out, todo, seen = {}, [r.grad_fn for r in roots], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        for i, k in STATS.get(type(fn).__name__, ()):
            mean, rstd = fn.saved_tensors[i], fn.saved_tensors[k]
            assert mean.shape[1] not in out
            out[mean.shape[1]] = (mean.clone(), rstd.clone())
        todo += [f for f, _ in fn.next_functions]
    return out


def _steps(net, x0, inp0, masks, groups, ride, steps=2, defer=False, cot_seed=5):
    """``steps`` forward + backward passes of ``net._gene_tail``; everything the two routes must agree on, per step."""
    from igcn_amd import ops
    got = []
    for _ in range(steps):
        x, inp = x0.clone().requires_grad_(True), inp0.clone().requires_grad_(True)
        net._tracked = []
        x_d, latent = net._gene_tail(x, inp, masks, groups, ride)
        rng = np.random.default_rng(cot_seed)
        c = [torch.from_numpy(rng.standard_normal(tuple(o.shape))).float().cuda() for o in (x_d, latent)]
        loss = (x_d * c[0]).sum() + (latent * c[1]).sum()
        fused = type(latent.grad_fn).__name__ == "GeneTailBackward"
        stats = _saved_stats([x_d, latent])
        names = ["dx", "dinp"] + ["grad " + k for k, _ in net.named_parameters()]
        leaves = [x, inp] + list(net.parameters())
        if defer:                        # (autograd.grad hands back the op's own buffers: the flush fills them)
            with ops.deferred_reductions():
                grads = torch.autograd.grad(loss, leaves)
        else:
            grads = torch.autograd.grad(loss, leaves)
        torch.cuda.synchronize()
        res = {"x_d": x_d.detach().clone(), "latent": latent.detach().clone()}
        res.update({k: g.clone() for k, g in zip(names, grads)})
        res.update({"buffer " + k: v.clone() for k, v in net.state_dict().items() if "running" in k})
        for ch, (m, r) in stats.items():
            res[f"mean[{ch}]"], res[f"rstd[{ch}]"] = m, r
        got.append((fused, res))
    return got


def _assert_equal(a, b, what):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), (what, k)
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


def _both(monkeypatch, n=40, j=3, nnz=30, n_top=5, hidden=32, l_dim=4, b=8, groups=2, training=True, defer=False,
          keep_h=True, expect_fused=True):
    monkeypatch.setenv("IGCN_SPARSE_MAPS", "1")                 # (8 samples would take the dense-image maps: no rider)
    base = _tail(n, j, nnz, n_top, hidden, l_dim, seed=n + b).train(training)
    x, inp, masks = _inputs(b, n, n_top, hidden, seed=b, keep_h=keep_h)
    if not training:
        masks = {"out_d": None, "h": None}
    runs = {}
    for ride in (True, False):
        net = copy.deepcopy(base)
        net.gene_t_csr = base.gene_t_csr
        runs[ride] = _steps(net, x, inp, masks, groups, ride, defer=defer)
    for step, ((fused, on), (plain, off)) in enumerate(zip(runs[True], runs[False])):
        assert fused == expect_fused and not plain
        assert len([k for k in on if k.startswith("mean[")]) == 3
        _assert_equal(on, off, f"step {step}")
    if training:                                              # the running statistics moved, twice
        first, second = runs[True][0][1], runs[True][1][1]
        assert all(not torch.equal(first[k], second[k]) for k in first if k.startswith("buffer "))
    return runs


@pytest.mark.parametrize("l_dim", [4, 8])
@pytest.mark.parametrize("defer", [False, True])
def test_tail_ride_equals_the_separate_ops_bit_for_bit(monkeypatch, l_dim, defer):
    """Outputs, saved mean / rstd of the three BatchNorms, running statistics after one and after two steps, every
    parameter gradient and both input gradients; the dropout factors sit on the hidden layer and on the read-out, none
    on the second layer.  ``defer``: the backward inside ops.deferred_reductions, as the train step runs it."""
    _both(monkeypatch, l_dim=l_dim, defer=defer)


def test_host_grid_of_one_node_block_and_fewer_nodes_than_passengers(monkeypatch):
    _both(monkeypatch, n=11)


def test_one_group(monkeypatch):
    _both(monkeypatch, groups=1)


def test_no_dropout_factors_on_the_hidden_layer(monkeypatch):
    _both(monkeypatch, keep_h=False)


def test_evaluation_mode_launches_the_first_passenger_alone(monkeypatch):
    """No statistics pass in evaluation mode: BatchNorm 1 gets its own launch from the same entry point; the running
    statistics stay put."""
    runs = _both(monkeypatch, training=False)
    first, second = runs[True][0][1], runs[True][1][1]
    assert all(torch.equal(first[k], second[k]) for k in first if k.startswith("buffer "))


def test_groups_beyond_the_register_kernels_take_the_separate_ops(monkeypatch):
    """B / groups = 1025: igcn_bn1d_fwd_supported is false, ``gene_tail_supported`` with it, and ``tail_ride`` changes
    nothing."""
    from igcn_amd import _lib
    assert not _lib.load().igcn_gene_tail_supported(2, 1, 40, 3, 30, 2050, 2)
    assert _lib.load().igcn_gene_tail_supported(2, 1, 40, 3, 30, 2048, 2)
    _both(monkeypatch, b=2050, expect_fused=False)


def test_fused_op_inside_fenced_poisoned_allocations(monkeypatch):
    """Every buffer of the fused op between fences and poisoned (tests/fenced.py): nothing written outside, nothing
    returned unwritten, the same bits as the plain run."""
    from fenced import fenced
    monkeypatch.setenv("IGCN_SPARSE_MAPS", "1")
    base = _tail(40, 3, 30, 5, 32, 4, seed=3).train()
    x, inp, masks = _inputs(8, 40, 5, 32, seed=8)
    plain = _steps(copy.deepcopy(base), x, inp, masks, 2, True, steps=1)[0]
    with fenced() as f:
        inside = _steps(copy.deepcopy(base), x, inp, masks, 2, True, steps=1)[0]
        f.check()
    assert plain[0] and inside[0] and f.records
    _assert_equal(inside[1], plain[1], "fenced")


def test_captured_and_replayed_twice_equals_eager(monkeypatch):
    """Forward and backward of the fused op captured with torch.cuda.graph and replayed twice: the outputs and gradients
    of the second replay and the running statistics after the warm-up pass and both replays equal three eager steps."""
    monkeypatch.setenv("IGCN_SPARSE_MAPS", "1")
    base = _tail(40, 3, 30, 5, 32, 4, seed=11).train()
    x0, inp0, masks = _inputs(8, 40, 5, 32, seed=9)
    eager = _steps(copy.deepcopy(base), x0, inp0, masks, 2, True, steps=3)[-1]
    assert eager[0]
    net = copy.deepcopy(base)
    x, inp = x0.clone().requires_grad_(True), inp0.clone().requires_grad_(True)
    leaves = [x, inp] + list(net.parameters())
    rng = np.random.default_rng(5)
    c = [torch.from_numpy(rng.standard_normal(s)).float().cuda() for s in ((8, 3), (8, 4))]

    def step():
        net._tracked = []
        x_d, latent = net._gene_tail(x, inp, masks, 2, True)
        assert type(latent.grad_fn).__name__ == "GeneTailBackward"
        return x_d, latent, torch.autograd.grad((x_d * c[0]).sum() + (latent * c[1]).sum(), leaves)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                  # warm-up: one eager step's running statistics
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x_d, latent, grads = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    got = {"x_d": x_d, "latent": latent, "dx": grads[0], "dinp": grads[1]}
    got.update({"grad " + k: g for (k, _), g in zip(net.named_parameters(), grads[2:])})
    got.update({"buffer " + k: v for k, v in net.state_dict().items() if "running" in k})
    want = {k: v for k, v in eager[1].items() if k in got}
    _assert_equal(got, want, "replay")


def test_forward_rides_in_a_capture_only_unless_told(monkeypatch):
    """The whole GO network (75 nodes, 54 SNPs, 8 samples): ``forward`` keeps the separate ops in an eager step, takes
    ops.GeneTail with ``tail_ride=True`` and — the class attribute — inside a stream capture; the eager routes agree bit
    for bit in every output and gradient."""
    from igcn_amd import synth
    from igcn_amd.go_model import Gene_ontology_network
    monkeypatch.setenv("IGCN_SPARSE_MAPS", "1")
    assert Gene_ontology_network.tail_ride is True
    pool = (40, 20, 10, 4, 1)
    go_snps, adj, pool_dim = synth.go_hierarchy(pool, seed=2, p_snp=0.25)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    torch.manual_seed(4)
    base = Gene_ontology_network(a_g, a, 2, 2, [5, 5], pool_dim, 8, "cuda").cuda().train()
    base._dropout_enabled = False
    snps = torch.from_numpy(np.random.default_rng(1).integers(0, 3, (8, 54))).float().cuda()
    fused = lambda out: type(out[0].grad_fn).__name__ == "GeneTailBackward"               # noqa: E731
    got = {}
    for ride in (None, True):
        net = copy.deepcopy(base)
        out = net(snps, None, "cuda", tail_ride=ride)
        assert fused(out) == bool(ride)
        (out[0].sum() + 0.5 * out[1].sum() + 0.25 * out[3].sum()).backward()
        got[ride] = {"latent": out[0].detach(), "x_d": out[1].detach(), "att": out[3].detach()}
        got[ride].update({k: p.grad for k, p in net.named_parameters() if p.grad is not None})
        got[ride].update({k: v for k, v in net.state_dict().items() if "running" in k})
    _assert_equal(got[True], got[None], "forward")
    net = copy.deepcopy(base)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net(snps, None, "cuda")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = net(snps, None, "cuda")
    assert fused(out)
    net.tail_ride = False
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        assert not fused(net(snps, None, "cuda"))
