"""The host-side protocol of a captured step, spelled once: the capture context, the roll-back of the warm-up steps, the
hand-over of the optimiser's gradient-pointer table between captured and eager steps, the one-captured-object-per-batch-
shape cache, and the trainer kept on the optimiser.  ``train.GraphedTrainStep``, ``snps.GraphedSnpsStep``, the two epoch
trainers and ``train.Evaluator`` keep only what is theirs: their inputs, their warm-up loop, what they capture."""
import contextlib
import weakref

import torch

from . import _lib


class _capture:
    """``torch.cuda.graph`` with the cyclic garbage collector held off while the capture is open.  torch collects once on
    entry; a collection that starts DURING the capture — any allocation of the step, on this thread or on the autograd
    engine's — may finalise an object whose destructor the runtime refuses inside a capture (another captured step's
    hipGraph: every GraphedTrainStep sits in a reference cycle with its optimiser's pointer table, so it dies whenever the
    collector gets to it) and the process aborts."""

    def __init__(self, graph, **kw):
        self.ctx = torch.cuda.graph(graph, **kw)

    def __enter__(self):
        import gc
        self.was = gc.isenabled()
        self.ctx.__enter__()            # (synchronises, collects once, empties the allocator cache, begins the capture)
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        try:
            return self.ctx.__exit__(*exc)
        finally:
            if self.was:
                gc.enable()


@contextlib.contextmanager
def rolled_back(model, opt):
    """``with rolled_back(model, opt): <warm-up steps>`` — the body (eager steps: allocator and library warm-up) runs on a
    side stream and is undone afterwards, so N replays equal N eager steps: the optimiser state, every module buffer
    (BatchNorm statistics, ``num_batches_tracked``) and the device counter of every mask generator are cloned before and
    written back after it.  The counters are not registered buffers: every ``ops.DropoutState`` held by a module of
    ``model`` is found by type, wherever a model keeps it — a shape captured in the middle of an epoch must not shift the
    masks of every later step against an eager run.  A counter is written back only while the attribute still
    holds the same object; a generator that first comes into being during the warm-up is left alone."""
    from . import ops
    from .train import forget_riders
    tensors = [opt.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_count, *model.buffers()]
    states = [(m, k, v) for m in model.modules() for k, v in vars(m).items() if isinstance(v, ops.DropoutState)]
    saved = [t.clone() for t in tensors]
    saved_states = [v.state.clone() for _, _, v in states]
    saved_has = list(opt._has_state)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        yield
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for dst, src in zip(tensors, saved):
            dst.copy_(src)
        for (m, k, v), src in zip(states, saved_states):
            if getattr(m, k, None) is v:
                v.state.copy_(src)
    opt._has_state = saved_has
    forget_riders(model)
    torch.cuda.synchronize()


class GradTable:
    """A captured step's OWN gradient-pointer table: the captured Adam / pack kernels read ``table``, so captured steps of
    one optimiser (the shapes of an epoch, two alternating input sets) never re-upload anything when they take turns.
    ``seal()`` after the capture, ``claim(owner)`` before every replay."""

    def __init__(self, opt):
        self.opt = opt
        self.table = torch.zeros_like(opt.table)

    def seal(self):
        opt = self.opt
        # the captured gradient tensors keep their addresses — which only helps if the table can point AT them: a
        # non-contiguous gradient would be copied by refresh_table, and the replays would never update the copy
        for p in opt.params:
            if p.grad is not None and not p.grad.is_contiguous():
                raise _lib.IgcnError("graphed step: a parameter gradient is not contiguous "
                                     f"(shape {tuple(p.shape)}, strides {p.grad.stride()})")
        opt.refresh_table(table=self.table)
        # the parameters' ``.grad`` belong to whoever stepped last: an eager step (the ragged last batch of an epoch) or
        # another captured step re-points them, and ``claim`` puts this graph's own back before it replays
        self.live = list(opt._table_live)
        self.grads = [p.grad for p in opt.params]
        self.hyper_version = opt._hyper_version

    def claim(self, owner):
        """True when the parameters' ``.grad`` had to be pointed back at this step's tensors."""
        opt = self.opt
        if opt._hyper_version != self.hyper_version:
            raise RuntimeError("graphed step: betas / eps of the optimiser changed after the capture (they are by-value "
                               "launch arguments; only the learning rate is read from device memory) — rebuild the step")
        if getattr(opt, "_ticked", False):
            raise RuntimeError("graphed step: an eager backward advanced the step counter and no optimizer.step() "
                               "followed it")
        if opt._table_owner is owner:
            return False
        opt._table_owner = owner                        # (host book-keeping only: the device table is this graph's own)
        opt._table_live = list(self.live)
        for p, g in zip(opt.params, self.grads):
            p.grad = g
        return True


class ShapeCache:
    """One captured object per batch SHAPE: a signature is captured (``build()``) once it has been met ``capture_after``
    times while capturable, as long as fewer than ``max_graphs`` are held; until then, and beyond that, ``lookup`` answers
    None and the batch runs eagerly.  ``counts``: batches run eagerly / captures made / batches replayed."""

    def __init__(self, capture_after, max_graphs):
        self.capture_after, self.max_graphs = int(capture_after), int(max_graphs)
        self.steps, self.seen = {}, {}               # signature -> captured object / times met without one
        self.counts = {"replayed": 0, "eager": 0, "captured": 0}

    def lookup(self, sig, graphable, build, load):
        """The captured object of ``sig`` with the batch handed over (``load(g)``; an exception of it passes through),
        or None: not captured (yet), or ``load`` answered False — it refused the batch."""
        g = self.steps.get(sig)
        if g is None and graphable:
            n = self.seen.get(sig, 0)
            self.seen[sig] = n + 1
            if n >= self.capture_after and len(self.steps) < self.max_graphs:
                g = self.steps[sig] = build()
                self.counts["captured"] += 1
        if g is not None and load(g) is False:
            g = None
        self.counts["eager" if g is None else "replayed"] += 1
        return g


def kept_trainer(optimizer, slot, key, make, model, comm=None):
    """The trainer of ``key`` (which names ``model`` and ``comm`` by ``id``) kept in ``optimizer.__dict__[slot]``, made
    by ``make()`` the first time: calling a ``fit_epoch`` once per epoch re-uses the captured steps.  The model and the
    communicator are held by weak reference, so an id() recycled after garbage collection cannot alias."""
    cache = optimizer.__dict__.setdefault(slot, {})
    tr = cache.get(key)
    if tr is not None and (tr._model_ref() is not model or (comm is not None and tr._comm_ref() is not comm)):
        tr = None                                             # the id belonged to an object that is gone
    if tr is None:
        tr = cache[key] = make()
        tr._model_ref = weakref.ref(model)
        tr._comm_ref = weakref.ref(comm) if comm is not None else (lambda: None)
    return tr
