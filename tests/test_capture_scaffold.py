"""The host-side protocol of a captured step (igcn_amd/capture.py) on stand-ins: the per-shape cache, the roll-back of
the warm-up steps and the hand-over of the gradient-pointer table.  No GPU: nothing here loads the library."""
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from igcn_amd import capture, ops, train


# ---- ShapeCache ------------------------------------------------------------------------------------------------------
# the script of signatures and, per (capture_after, max_graphs), what becomes of each step, worked out by hand:
# e = eager, c = captured and replayed, r = replayed.  ``c`` arrives when both slots are taken: eager for good.
SCRIPT = "ababab" + "cacc"
OUTCOME = {(0, 1): "cerere" + "eree", (0, 2): "ccrrrr" + "eree",
           (1, 1): "eecere" + "eree", (1, 2): "eeccrr" + "eree",
           (2, 1): "eeeece" + "eree", (2, 2): "eeeecc" + "eree"}


@pytest.mark.parametrize("capture_after, max_graphs", sorted(OUTCOME))
def test_shape_cache_builds_a_shape_once_on_its_sighting_and_stops_at_max_graphs(capture_after, max_graphs):
    cache = capture.ShapeCache(capture_after, max_graphs)
    built, want = [], {"eager": 0, "captured": 0, "replayed": 0}
    for sig, what in zip(SCRIPT, OUTCOME[capture_after, max_graphs]):
        loaded = []

        def build():
            built.append(sig)
            return ("captured", sig)
        g = cache.lookup(sig, True, build, loaded.append)
        want["eager"] += what == "e"
        want["captured"] += what == "c"
        want["replayed"] += what in "cr"
        assert cache.counts == want, (sig, what, cache.counts)
        assert (g, loaded) == ((None, []) if what == "e" else (("captured", sig), [("captured", sig)]))
    assert built == list("ab")[:max_graphs] and list(cache.steps) == built     # each exactly once
    assert all(cache.seen[sig] == capture_after + 1 for sig in built)          # ... on that sighting


def test_shape_cache_counts_by_hand():
    cache = capture.ShapeCache(1, 2)
    steps = [("a", {"eager": 1, "captured": 0, "replayed": 0}),
             ("a", {"eager": 1, "captured": 1, "replayed": 1}),
             ("b", {"eager": 2, "captured": 1, "replayed": 1}),
             ("c", {"eager": 3, "captured": 1, "replayed": 1}),
             ("c", {"eager": 3, "captured": 2, "replayed": 2}),
             ("b", {"eager": 4, "captured": 2, "replayed": 2}),      # the third shape: no room, eager for good
             ("b", {"eager": 5, "captured": 2, "replayed": 2}),
             ("a", {"eager": 5, "captured": 2, "replayed": 3})]
    for sig, want in steps:
        cache.lookup(sig, True, lambda: object(), lambda g: None)
        assert cache.counts == want, (sig, cache.counts)
    assert set(cache.steps) == {"a", "c"}


def test_shape_cache_never_builds_what_is_not_graphable_and_falls_back_when_load_refuses():
    cache = capture.ShapeCache(0, 2)

    def never():
        raise AssertionError("built")
    for k in range(4):
        assert cache.lookup("a", False, never, never) is None
        assert cache.counts == {"eager": k + 1, "captured": 0, "replayed": 0}
    g = cache.lookup("a", True, lambda: "A", lambda g: None)
    assert g == "A" and cache.counts == {"eager": 4, "captured": 1, "replayed": 1}
    assert cache.lookup("a", True, never, lambda g: False) is None       # the captured object refused this batch
    assert cache.counts == {"eager": 5, "captured": 1, "replayed": 1}
    with pytest.raises(ValueError):                                      # an error of the hand-over passes through

        def refuse(g):
            raise ValueError("shape")
        cache.lookup("a", True, never, refuse)
    assert cache.counts == {"eager": 5, "captured": 1, "replayed": 1}


# ---- rolled_back ---------------------------------------------------------------------------------------------------
def _state(values):
    s = object.__new__(ops.DropoutState)            # (the constructor asks the library for the counter's size)
    s.state = torch.tensor(values, dtype=torch.int64)
    return s


class _Leaf(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(3, 2)
        self._noise_source = _state([11, 12, 13])   # an attribute name none of the models uses, two levels down


class _Child(nn.Module):
    def __init__(self):
        super().__init__()
        self.leaf = _Leaf()
        self._drop_state = _state([5, 6])


class _Model(nn.Module):
    def __init__(self):
        super().__init__()
        self.bn = nn.BatchNorm1d(4)
        self.go_network = _Child()
        self._gate_state = _state([7])


def _optimizer():
    g = torch.Generator().manual_seed(3)
    return SimpleNamespace(flat=torch.randn(9, generator=g), exp_avg=torch.randn(9, generator=g),
                           exp_avg_sq=torch.rand(9, generator=g), step_count=torch.tensor([4], dtype=torch.int64),
                           _has_state=[True, False, True])


def _everything(model, opt):
    gens = [model._gate_state, model.go_network._drop_state, model.go_network.leaf._noise_source]
    return [opt.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_count, *model.buffers(), *(s.state for s in gens)]


def _warm_up(model, opt):
    """What warm-up steps do to the state: every tensor overwritten in place, the flags flipped."""
    with torch.no_grad():
        for t in _everything(model, opt):
            t.copy_(t * 3 + 1)
    opt._has_state = [not h for h in opt._has_state]


@pytest.fixture
def stream_log(monkeypatch):
    """torch.cuda's streams and the library's rider queue replaced by a log of what ``rolled_back`` asks of them."""
    log = []

    class _Stream:
        def __init__(self, name="side"):
            self.name = name

        def wait_stream(self, other):
            log.append(f"{self.name} waits for {other.name}")

    class _On:
        def __init__(self, stream):
            self.stream = stream

        def __enter__(self):
            log.append(f"on {self.stream.name}")

        def __exit__(self, *exc):
            log.append(f"off {self.stream.name}")

    main = _Stream("main")
    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: main)
    monkeypatch.setattr(torch.cuda, "stream", _On)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: log.append("synchronize"))
    monkeypatch.setattr(train, "forget_riders", lambda model: log.append(("forget_riders", model)))
    return log


def test_rolled_back_restores_optimizer_buffers_and_every_generator_bit_for_bit(stream_log):
    model, opt = _Model(), _optimizer()
    model.bn.running_mean.add_(0.25)
    model.bn.num_batches_tracked.add_(2)
    tensors = _everything(model, opt)
    assert len(tensors) == 4 + 3 + 3
    before, has = [t.clone() for t in tensors], list(opt._has_state)
    with capture.rolled_back(model, opt):
        _warm_up(model, opt)
        assert all(not torch.equal(t, b) for t, b in zip(tensors, before)) and opt._has_state != has
    for t, b in zip(tensors, before):                # (the same tensors, written in place; the nested generator under a
        assert torch.equal(t, b)                     # name of its own among them)
    assert opt._has_state == has


def test_rolled_back_leaves_a_replaced_and_a_new_generator_alone(stream_log):
    model, opt = _Model(), _optimizer()
    old = model.go_network._drop_state
    with capture.rolled_back(model, opt):
        _warm_up(model, opt)
        model.go_network._drop_state = new = _state([100, 101])  # (the warm-up made a new one: another device, say)
        model.bn._born_in_warmup = born = _state([42])
        tripled = old.state.clone()
    assert torch.equal(new.state, torch.tensor([100, 101])) and torch.equal(born.state, torch.tensor([42]))
    assert torch.equal(old.state, tripled)                       # nobody's counter any more: not written to either
    assert torch.equal(model._gate_state.state, torch.tensor([7]))


def test_rolled_back_runs_the_body_on_a_side_stream_then_forgets_the_riders_and_synchronizes(stream_log):
    model, opt = _Model(), _optimizer()
    with capture.rolled_back(model, opt):
        stream_log.append("warm-up")
    assert stream_log == ["side waits for main", "on side", "warm-up", "off side", "main waits for side",
                          ("forget_riders", model), "synchronize"]


# ---- GradTable -------------------------------------------------------------------------------------------------------
class _Adam:
    """The part of ``train.FlatAdam`` a GradTable touches."""

    def __init__(self):
        self.params = [nn.Parameter(torch.zeros(2, 3)), nn.Parameter(torch.zeros(4)), nn.Parameter(torch.zeros(1))]
        self.table = torch.zeros(3, dtype=torch.int64)
        self._table_live, self._table_owner, self._hyper_version = [False] * 3, None, 0
        self.refreshed = []

    def refresh_table(self, owner=None, table=None):
        self._table_owner = owner
        self._table_live = [p.grad is not None for p in self.params]
        self.refreshed.append(table)


def _sealed():
    opt = _Adam()
    t = capture.GradTable(opt)
    assert t.table is not opt.table and t.table.shape == opt.table.shape
    opt.params[0].grad, opt.params[1].grad = torch.ones(2, 3), torch.ones(4)
    t.seal()
    assert len(opt.refreshed) == 1 and opt.refreshed[0] is t.table
    return opt, t, [p.grad for p in opt.params]


def test_grad_table_seal_refuses_a_non_contiguous_gradient():
    opt = _Adam()
    t = capture.GradTable(opt)
    opt.params[0].grad = torch.ones(3, 2).t()
    with pytest.raises(capture._lib.IgcnError, match="not contiguous"):
        t.seal()
    assert opt.refreshed == []


def test_grad_table_claim_raises_when_the_hyper_parameters_moved_or_a_tick_is_open():
    opt, t, _ = _sealed()
    owner = object()
    opt._hyper_version += 1
    with pytest.raises(RuntimeError, match="betas / eps of the optimiser changed after the capture"):
        t.claim(owner)
    opt._hyper_version -= 1
    opt._ticked = True
    with pytest.raises(RuntimeError, match="an eager backward advanced the step counter"):
        t.claim(owner)
    assert opt._table_owner is None                              # a refused claim re-points nothing
    opt._ticked = False
    assert t.claim(owner) is True and opt._table_owner is owner


def test_grad_table_claim_repoints_only_when_the_owner_differs():
    opt, t, grads = _sealed()
    owner, other = object(), object()
    # an eager step took the table and the gradients
    opt._table_owner, opt._table_live = other, [True, True, True]
    for p in opt.params:
        p.grad = torch.zeros_like(p)
    assert t.claim(owner) is True
    assert opt._table_owner is owner and opt._table_live == [True, True, False] and opt._table_live is not t.live
    assert all(p.grad is g for p, g in zip(opt.params, grads))
    # still the owner: nothing is touched, whatever it holds
    mine = torch.full((4,), 2.0)
    opt.params[1].grad, opt._table_live = mine, [False, False, False]
    assert t.claim(owner) is False
    assert opt.params[1].grad is mine and opt._table_live == [False, False, False]
