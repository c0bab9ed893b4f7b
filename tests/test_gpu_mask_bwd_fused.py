"""The backward of ops.SgcnFront on sparse (k-NN) graphs as igcn_sgcn_stack_bwd_mask — the masked copy's workgroups of
the stack backward do the edge-mask backward's node pass out of LDS — against the route it replaces
(IGCN_NO_MASK_BWD_FUSED=1: igcn_sgcn_stack_bwd on the 2-copy plan, then igcn_edge_mask_bwd_reg) on the same build:

  * every gradient bit for bit, except prob_bias's: its partial rows are one per graph and no longer one per 64
    consecutive nodes, so it is held to the project's gradient bound (DESIGN: "gradients 1e-3" of the tensor's scale) and
    to being bit-identical from run to run and between eager and captured replay;
  * graphs whose 64-node blocks straddle graphs (R = 90), empty lists, lists of 9 entries (three trips of a lane's
    stride loop), stored self-loops, a graph with fewer edges than Emax;
  * a refused graph, a captured step, and the calls each route makes.

The host-side checks at the end need no GPU."""
import types

import numpy as np
import pytest
import torch

from conftest import assert_matches
from igcn_amd import ops

SWITCH = "IGCN_NO_MASK_BWD_FUSED"
HP = (0.1, 0.2, 0.15, 0.05, 1e-6)
NS = 11                                                   # SNPs
PB = 2                                                    # position of prob_bias among the leaves
BENCH_BWD_LDS_BYTES = 78528                               # igcn_sgcn_stack_lds_bytes(90, 270, 3, 16, 2, 1) before this route existed


def _knn_graph(rng, r, h0, k=3):
    """Every node receives edges from k distinct other nodes (a k-NN list), in shuffled stored order."""
    src = np.concatenate([rng.choice(np.delete(np.arange(r), i), k, replace=False) for i in range(r)])
    dst = np.repeat(np.arange(r), k)
    return _data(rng, r, h0, src, dst)


def _data(rng, r, h0, src, dst):
    from igcn_amd.data import Data
    order = rng.permutation(len(src))
    ei = torch.from_numpy(np.vstack([np.asarray(src)[order], np.asarray(dst)[order]])).long()
    return Data(x=torch.from_numpy(rng.random((r, h0)) + 0.1).float(), edge_index=ei,
                edge_attr=torch.from_numpy(rng.random(ei.shape[1]) + 0.05).float())


def _hand_graph(rng, r, h0):
    """Node 0 has no in-edges, node 1 no out-edges; node 2 sends 9 edges and receives 9 (parallel edges among them);
    nodes 4 and 5 carry a stored self-loop, node 6 two of them."""
    others = [3, 4, 5, 6, 7, 8, 9]
    src = [2] * 9 + others + [5, 6] + [0, 0, 3, 7] + [4, 5, 6, 6]
    dst = others + [3, 4] + [2] * 9 + [3, 9, 1, 1] + [4, 5, 6, 6]
    return _data(rng, r, h0, src, dst)


def _ring_graph(rng, r, h0):
    """r edges: fewer than every other graph of the batch has, so fewer than Emax."""
    return _data(rng, r, h0, np.arange(r), (np.arange(r) + 1) % r)


def _case(g, r, h0, layers, f, seed=0, big_last=False):
    """g k-NN graphs between the two hand-made ones; ``big_last``: one more graph behind them, with the most edges."""
    rng = np.random.default_rng(seed + 1000 * g + 10 * r + h0 + 7 * f)
    graphs = [_ring_graph(rng, r, h0)] + [_knn_graph(rng, r, h0) for _ in range(g)] + [_hand_graph(rng, r, h0)]
    if big_last:
        graphs.append(_knn_graph(rng, r, h0, k=4))
    t = lambda a: torch.from_numpy(np.asarray(a)).float().cuda()                     # noqa: E731
    nb = len(graphs)
    n, ne = nb * r, sum(int(d.edge_index.shape[1]) for d in graphs)
    par = dict(prob=t(rng.standard_normal((r, h0))), pb=t(rng.standard_normal((2 * h0, 1))),
               snps=t(rng.standard_normal((1, NS))),
               ws=[t(rng.standard_normal((f, h0 if l == 0 else f)) / np.sqrt(h0 if l == 0 else f)) for l in range(layers)],
               bs=[t(0.3 * rng.standard_normal(f)) for _ in range(layers)])
    cot = dict(xcat=t(rng.standard_normal((2 * n, layers * f))), xcat2=t(rng.standard_normal((2 * n, layers * f))),
               e=t(rng.standard_normal(ne)), reg=t(np.full(nb, 3.0)), full=t(rng.standard_normal((2 * nb, NS))))
    return dict(graphs=graphs, r=r, h0=h0, f=f, layers=layers, par=par, cot=cot, feat=t(rng.random((nb, NS))), n=n, ne=ne)


def _leaves(c, batch, x_grad=True):
    p = c["par"]
    leaves = [batch.x.clone().requires_grad_(x_grad), p["prob"].clone().requires_grad_(True),
              p["pb"].clone().requires_grad_(True), p["snps"].clone().requires_grad_(True)]
    leaves += [w.clone().requires_grad_(True) for pair in zip(p["ws"], p["bs"]) for w in pair]
    return leaves


def _grads(c, batch, plan, leaves, use=("xcat", "e", "reg", "full")):
    """d(sum of the used outputs . their cotangents) / d(leaves) through ops.SgcnFront."""
    x, prob, pb, snps, *wb = leaves
    plan.rebuild(batch.edge_index, lazy=True)
    assert ops.sgcn_front_supported(plan, c["r"], c["h0"], c["f"], c["layers"], c["feat"], snps)
    out = dict(zip(("xcat", "xcat2", "e", "reg", "full"),
                   ops.SgcnFront.apply(x, prob, pb, batch.edge_attr, plan, c["r"], snps, HP, c["feat"], batch.edge_index, *wb)))
    wanted = [v for v in leaves if v.requires_grad]
    return torch.autograd.grad([out[k] for k in use], wanted, [c["cot"][k] for k in use], allow_unused=True)


def _run(c, monkeypatch, unfused, use=("xcat", "e", "reg", "full"), x_grad=True, before_backward=None):
    from calltrace import record_calls
    from igcn_amd.data import Batch
    with monkeypatch.context() as mp:
        if unfused:
            mp.setenv(SWITCH, "1")
        seen = record_calls(mp)
        batch = Batch.from_data_list(c["graphs"]).to("cuda")
        plan = ops.plan_for(batch)
        if before_backward:
            before_backward(plan)
        grads = _grads(c, batch, plan, _leaves(c, batch, x_grad), use)
        torch.cuda.synchronize()
        return grads, [s for s in seen if "bwd" in s[0]], int(plan.status[0].item())


def _bwd_names(calls):
    return [s[0] for s in calls]


def _compare(want, got, again, what, pb_at=PB):
    """unfused | fused | fused again"""
    assert len(want) == len(got) == len(again)
    for i, (w, a, b) in enumerate(zip(want, got, again)):
        assert (w is None) == (a is None) == (b is None), (what, i)
        if w is None:
            continue
        assert torch.equal(a, b), f"{what}: leaf {i} differs between two runs of the fused route"
        if i == pb_at:
            err = float((a.double() - w.double()).abs().max())
            print(f"{what}: prob_bias gradient, fused vs unfused: max abs err {err:.3e}, scale {float(w.abs().max()):.3e}")
            assert_matches(a, w.cpu().numpy(), 1e-3, f"{what}: grad prob_bias")
        else:
            assert torch.equal(a, w), f"{what}: leaf {i}: max abs err {float((a - w).abs().max()):.3e}"


VARIANTS = {
    "all": dict(),
    "no regulariser upstream": dict(use=("xcat", "e", "full")),
    "no d_e": dict(use=("xcat", "reg", "full")),
    "dxcat2": dict(use=("xcat", "xcat2", "e", "reg", "full")),
    "only dxcat2 and d_e": dict(use=("xcat2", "e")),
    "x takes no gradient": dict(x_grad=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("layers,f", [(1, 4), (2, 16), (3, 8)])
@pytest.mark.parametrize("h0", [1, 3])
@pytest.mark.parametrize("g,r", [(1, 10), (3, 10), (5, 10), (1, 90), (3, 90), (5, 90)])
def test_fused_route_gives_the_unfused_gradients(monkeypatch, g, r, h0, layers, f):
    c = _case(g, r, h0, layers, f)
    assert min(int(d.edge_index.shape[1]) for d in c["graphs"]) < max(int(d.edge_index.shape[1]) for d in c["graphs"])
    for name, kw in VARIANTS.items():
        want, calls0, st0 = _run(c, monkeypatch, True, **kw)
        got, calls1, st1 = _run(c, monkeypatch, False, **kw)
        again, _, _ = _run(c, monkeypatch, False, **kw)
        assert st0 == st1 == 0
        # the switch keeps exactly the two calls of before; the fused route makes one
        assert _bwd_names(calls0) == ["igcn_sgcn_stack_bwd", "igcn_edge_mask_bwd_reg"], (name, calls0)
        assert _bwd_names(calls1) == ["igcn_sgcn_stack_bwd_mask"], (name, calls1)
        x_grad = kw.get("x_grad", True)
        assert (calls1[0][40] is None) == (not x_grad), name       # the dx argument: no dx, no dx workgroups
        _compare(want, got, again, f"{name} (G={g}+2, R={r}, H0={h0}, L={layers}, F={f})", pb_at=PB if x_grad else PB - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("r,h0,layers,f", [(10, 3, 2, 16), (90, 1, 1, 4)])
def test_a_refused_graph_contributes_zeros_on_both_routes(monkeypatch, r, h0, layers, f):
    """The stack backward is sized for fewer edges than the batch's last graph has — max_edges below a graph's count, as
    the stack kernels' status tests provoke it: both routes flag it with the same status word; the
    fused route leaves exact zeros where that graph's contributions go, i.e. what the batch without that graph gives
    (no regulariser upstream: its edge term is scaled by the batch's edge count)."""
    from igcn_amd.data import Batch
    c = _case(3, r, h0, layers, f, seed=5, big_last=True)
    counts = [int(d.edge_index.shape[1]) for d in c["graphs"]]
    assert counts[-1] == max(counts) and counts[-1] > max(counts[:-1])
    use = ("xcat", "e", "full")

    def shrink(plan):
        plan.replicate(2)._stack_dims = (r, max(counts[:-1]))

    want, _, st0 = _run(c, monkeypatch, True, use=use, before_backward=shrink)
    got, _, st1 = _run(c, monkeypatch, False, use=use, before_backward=shrink)
    assert st0 == st1 == 2
    n1 = c["n"] - r
    assert torch.equal(got[0][:n1], want[0][:n1]) and int((got[0][n1:] != 0).sum()) == 0
    for a, w in zip(got[4:], want[4:]):                      # the stack's parameter gradients
        assert torch.equal(a, w)
    # the batch without the refused graph
    d = dict(c, graphs=c["graphs"][:-1], n=n1, ne=c["ne"] - counts[-1], feat=c["feat"][:-1].contiguous())
    n, nb, cot = c["n"], len(counts), c["cot"]
    d["cot"] = dict(xcat=torch.cat([cot["xcat"][:n1], cot["xcat"][n:n + n1]]), e=cot["e"][:d["ne"]].contiguous(),
                    full=torch.cat([cot["full"][:nb - 1], cot["full"][nb:2 * nb - 1]]))
    ref, _, st2 = _run(d, monkeypatch, False, use=use)
    assert st2 == 0
    assert torch.equal(got[0][:n1], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])


@pytest.mark.gpu
def test_captured_fused_route_replays_the_eager_bits(monkeypatch):
    """torch.cuda.graph around forward + backward of the fused route; the parameters change in place between replays."""
    from igcn_amd.data import Batch
    c = _case(3, 90, 3, 2, 16, seed=9)
    batch = Batch.from_data_list(c["graphs"]).to("cuda")
    plan = ops.plan_for(batch)
    leaves = _leaves(c, batch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _grads(c, batch, plan, leaves)                       # warm-up: allocations, the replica plan
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _grads(c, batch, plan, leaves)
    for step in range(2):
        with torch.no_grad():
            for i, v in enumerate(leaves):
                v.mul_(1.0 + 0.05 * (step + 1)).add_(0.01 * (i + 1))
        graph.replay()
        torch.cuda.synchronize()
        got = [v.clone() for v in captured]
        eager = _grads(c, batch, plan, leaves)
        torch.cuda.synchronize()
        for i, (a, w) in enumerate(zip(got, eager)):
            assert torch.equal(a, w), (step, i)
    assert int(plan.status[0].item()) == 0


# ---- host side: no GPU ---------------------------------------------------------------------------------------------
def _fake_plan(r=90, emax=270, graphs=4, edges_per_node=3, dense_blocks=False):
    return types.SimpleNamespace(_stack_dims=(r, emax), n_nodes=graphs * r, n_edges=graphs * r * edges_per_node,
                                 dense_blocks=dense_blocks)


def test_dispatch_condition(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    assert ops.mask_bwd_fused_supported(_fake_plan(), 90, 3, 16, 2)
    assert not ops.mask_bwd_fused_supported(_fake_plan(dense_blocks=True), 90, 3, 16, 2)
    assert not ops.mask_bwd_fused_supported(_fake_plan(emax=90 * 16, edges_per_node=16), 90, 3, 16, 2)   # the <64> node kernel's
    assert ops.mask_bwd_fused_supported(_fake_plan(emax=90 * 15, edges_per_node=15), 90, 3, 16, 2)
    for f in (3, 12, 64):                                    # outside the stack's widths
        assert not ops.mask_bwd_fused_supported(_fake_plan(), 90, 3, f, 2)
    assert not ops.mask_bwd_fused_supported(_fake_plan(), 45, 3, 16, 2)         # not the plan's graph size
    monkeypatch.setenv(SWITCH, "1")
    assert not ops.mask_bwd_fused_supported(_fake_plan(), 90, 3, 16, 2)
    monkeypatch.setenv(SWITCH, "0")
    assert ops.mask_bwd_fused_supported(_fake_plan(), 90, 3, 16, 2)


def test_backward_lds_at_the_bench_shape_is_unchanged():
    """R = 90, Emax = 270 (k = 3), H0 = 3, F = 16, L = 2: the node pass lives in blocks that are dead by then."""
    from igcn_amd import _lib
    assert int(_lib.load().igcn_sgcn_stack_lds_bytes(90, 270, 3, 16, 2, 1)) == BENCH_BWD_LDS_BYTES
