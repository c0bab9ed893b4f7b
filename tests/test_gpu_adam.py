"""Every form of the Adam step against the float64 oracle of tests/adam_ref.py, seams included.

One parameter set serves all forms (adam_ref.case_inputs): tensors of 1, 3, 4, 5, 17, C-1, C, C+1, C+4, 2C+3, 3C, (5, 413)
and (7, 5) floats plus one that never gets a gradient, C = igcn_adam_chunk(), in ONE FlatAdam so that a single launch covers
every chunk seam and every ragged quad.  Moments are seeded through the optimiser's own views (v >= m^2, several decades,
zero for t = 1, nonzero on the tensor without a gradient), the counter is set to t - 1.  Gradients: |g| log-uniform
1e-4 .. 1e2, a band with 1e-9 <= |g * grad_scale| <= 1e-7 (where eps decides), every seventh element exactly zero, one whole
tensor zero with zero moments; most are fresh allocations, one is a contiguous view at a 4-byte offset of a larger buffer (the
scalar path, across two seams), one a view at a 16-byte offset, one is handed over transposed (refresh_table makes it
contiguous).

Forms, each from the same seeded state, each judged per tensor by adam_ref.check at t in {1, 2, 3, 10, 1000, 20000} x the
three hyper-parameter sets of adam_ref.HYPERS:

  blocks          FlatAdam.step() in table mode                                   igcn_adam_step_blocks
  multi           the (96, n_tensors) grid on the optimiser's own table           igcn_adam_step_multi
  multi_ticked    the same, counter advanced by the caller                        igcn_adam_step_multi_ticked
  flat            pack_grads() then step(grad_scale, from_flat=True)              igcn_pack_grads, igcn_adam_step
  flat_ticked     the same, counter advanced by the caller                        igcn_adam_step_ticked
  trainer_ticked  deferred_reductions(tick=step_count), then a ticked step()      igcn_reduce_flush_tick, ..._blocks(ticked=1)

tol_u is 4 x the float32 yardstick's own worst error on the same inputs at the same t (floor 8 * 2^-24), computed here from
the inputs alone — never from a kernel's output.  After every form: step_count == t, the gradient tensors bit-identical, the
tensor without a gradient bit-identical under the table forms (stepped with g = 0 under the flat ones, like the oracle), the
padding between parameters exactly zero in flat / exp_avg / exp_avg_sq.

Measured worst errors (MI355X; 'u' = what is left of |p - p'| after the half ulp of the last subtraction, over S_u; the
yardstick's own figure on these inputs beside it; m over S_m, v relative):

                                t = 1     t = 2     t = 3     t = 10    t = 1000  t = 20000    m         v
  blocks, multi, multi_ticked,
  trainer_ticked (identical)  u   2.12e-07  3.54e-06  3.43e-06  4.07e-07  1.98e-07  2.05e-07     1.15e-07  1.70e-07
  flat, flat_ticked           u   2.12e-07  3.58e-06  3.43e-06  4.07e-07  2.11e-07  2.27e-07     1.15e-07  1.70e-07
  the float32 yardstick       u   2.66e-07  3.61e-06  3.24e-06  4.54e-07  2.61e-07  2.65e-07

  (the worst of the three hyper-parameter sets in every cell).  No form is further from the oracle than 1.06 x the yardstick
  (t = 3; 0.72 .. 1.00 x elsewhere) against the factor 4 allowed: the device's powf, sqrtf and division round like numpy's,
  and the figures at t = 2, 3 are the rounding of b2^t in 1 - b2^t, not the kernels'.  m and v stay under 3 * 2^-24 of their
  scales (bound 4 * 2^-24).  The chained test (8 eager steps + 3 replays) reaches u 3.50e-06, m 1.15e-07, v 1.53e-07.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu

FORMS = ["blocks", "multi", "multi_ticked", "flat", "flat_ticked", "trainer_ticked"]
TABLE_FORMS = ("blocks", "multi", "multi_ticked", "trainer_ticked")
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib, ops, train
    lib = _lib.load()          # raises if libigcn.so is missing: no fallback
    return SimpleNamespace(lib=_lib, ops=ops, train=train, chunk=int(lib.igcn_adam_chunk()))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _set_grads(opt, grads):
    """Hand the gradients over the way autograd might: fresh allocations, two views into larger buffers, a transposed view."""
    for k, (p, g) in enumerate(zip(opt.params, grads)):
        if g is None:
            p.grad = None
            continue
        n = g.size
        if k in (R.I_OFF4, R.I_OFF16):
            skip = 1 if k == R.I_OFF4 else 4
            buf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=p.device)
            view = buf[skip:skip + n]
            view.copy_(torch.from_numpy(g.reshape(-1)))
            p.grad = view.view_as(p)
            assert p.grad.is_contiguous() and p.grad.data_ptr() % 16 == (4 * skip) % 16
        elif k == R.I_TRANSPOSED:
            p.grad = torch.from_numpy(np.ascontiguousarray(g.T)).to(p.device).t()
            assert not p.grad.is_contiguous()
        else:
            p.grad = torch.from_numpy(g).to(p.device)
            assert p.grad.data_ptr() % 16 == 0


def _setup(env, t, hyper, seed=0):
    case = R.case_inputs(t, hyper, chunk=env.chunk, seed=seed)
    lr, b1, b2, eps, _ = hyper
    params = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in case["p"]]
    opt = env.train.FlatAdam(params, lr=lr, betas=(b1, b2), eps=eps)
    assert not opt.flat_grads and opt._blocks is not None
    with torch.no_grad():
        for k, (o, p) in enumerate(zip(opt._offs, opt.params)):
            n = p.numel()
            opt.exp_avg[o:o + n].copy_(torch.from_numpy(case["m"][k].reshape(-1)))
            opt.exp_avg_sq[o:o + n].copy_(torch.from_numpy(case["v"][k].reshape(-1)))
        opt.step_count.fill_(t - 1)
    _set_grads(opt, case["g"])
    return opt, case


def _download(opt):
    torch.cuda.synchronize()
    return tuple(x.detach().cpu().numpy().copy() for x in (opt.flat, opt.exp_avg, opt.exp_avg_sq))


def _per_tensor(opt, state):
    return [tuple(a[o:o + p.numel()] for a in state) for o, p in zip(opt._offs, opt.params)]


def _padding(opt):
    pad = np.ones(opt.flat.numel(), dtype=bool)
    for o, p in zip(opt._offs, opt.params):
        pad[o:o + p.numel()] = False
    return pad


def _hyper_of(opt, grad_scale):
    """What the optimiser hands the kernels, as the oracle's hyper tuple (the rate as float(lr), which lr_dev holds)."""
    return (opt.lr, opt.betas[0], opt.betas[1], opt.eps, grad_scale)


def _run(env, opt, form, gs):
    call, ptr, sp = env.lib.call, env.lib.ptr, env.lib.stream_ptr
    hyper = (ptr(opt.lr_dev), float(opt.betas[0]), float(opt.betas[1]), float(opt.eps), float(gs))
    nt = len(opt.params)
    if form == "blocks":
        opt.step(grad_scale=gs)
    elif form in ("multi", "multi_ticked"):
        opt.refresh_table()
        if form == "multi_ticked":
            opt.step_count.add_(1)                   # the caller advances the counter; the ticked call must not
        call("igcn_adam_step_multi" + form[5:], nt, ptr(opt.table), ptr(opt.numel), ptr(opt.step_count), *hyper, sp())
    elif form in ("flat", "flat_ticked"):
        opt.pack_grads()
        if form == "flat":
            opt.step(grad_scale=gs, from_flat=True)
        else:
            opt.step_count.add_(1)
            call("igcn_adam_step_ticked", opt.flat.numel(), ptr(opt.flat), ptr(opt.grad), ptr(opt.exp_avg),
                 ptr(opt.exp_avg_sq), ptr(opt.step_count), *hyper, sp())
    elif form == "trainer_ticked":                   # the route train_step takes: the backward's flush advances the counter
        with env.ops.deferred_reductions(tick=opt.step_count):
            pass
        opt._ticked = True
        opt.step(grad_scale=gs)
        assert opt._ticked is False
    else:
        raise AssertionError(form)


def _judge(opt, before, grads, hyper, t, tol_u, form, what):
    """Everything a step must leave behind; returns the worst errors over the tensors."""
    after = _download(opt)
    assert int(opt.step_count.item()) == t, f"{what}: step_count {int(opt.step_count.item())}, expected {t}"
    worst = {"u": 0.0, "m": 0.0, "v": 0.0}
    for k, (b, a, g) in enumerate(zip(_per_tensor(opt, before), _per_tensor(opt, after), grads)):
        name = f"{what} tensor {k} {tuple(opt.params[k].shape)}"
        if g is None and form in TABLE_FORMS:
            R.check_untouched(a, b, name)
            continue
        gk = np.zeros_like(b[0]) if g is None else g.reshape(-1)     # the flat form steps it with g = 0
        err = R.check(*a, b, gk, hyper, t, tol_u, name)
        worst = {key: max(worst[key], err[key]) for key in worst}
    pad = _padding(opt)
    for name, a in zip(("flat", "exp_avg", "exp_avg_sq"), after):
        assert not _bits(a)[pad].any(), f"{what}: padding of {name} is no longer zero"
    for k, (p, g) in enumerate(zip(opt.params, grads)):
        if g is None:
            assert p.grad is None
        else:
            assert np.array_equal(_bits(p.grad.detach().cpu().numpy()), _bits(g)), f"{what}: gradient {k} was written"
    return worst


@pytest.mark.parametrize("t", R.STEPS)
@pytest.mark.parametrize("hname", list(R.HYPERS))
@pytest.mark.parametrize("form", FORMS)
def test_adam_form_matches_fp64_oracle(env, form, hname, t):
    hyper = R.HYPERS[hname]
    opt, case = _setup(env, t, hyper)
    tol_u, yard = R.case_tol(case, hyper, t)
    before = _download(opt)
    for got, want in zip(_per_tensor(opt, before), zip(case["p"], case["m"], case["v"])):       # the seeding took
        assert all(np.array_equal(_bits(a), _bits(b.reshape(-1))) for a, b in zip(got, want))
    _run(env, opt, form, hyper[4])
    worst = _judge(opt, before, case["g"], _hyper_of(opt, hyper[4]), t, tol_u, form, f"{form} [{hname}, t={t}]")
    print(f"\nadam {form:<14} {hname:<7} t={t:<5} u {worst['u']:.2e} of S_u (yardstick {yard:.2e}, tol_u {tol_u:.2e}, "
          f"{worst['u'] / max(yard, R.U24):.2f} x yardstick)  m {worst['m']:.2e}  v {worst['v']:.2e}")


# ------------------------------------------------------------------------------------------------ igcn_pack_grads
def _expected_bucket(opt, grads, lo, hi):
    want = np.full(opt.grad.numel(), SENTINEL, dtype=np.float32)
    for k in range(lo, hi):
        o, n = opt._offs[k], opt.params[k].numel()
        want[o:o + n] = 0.0 if grads[k] is None else grads[k].reshape(-1)
    return want


def test_pack_grads_writes_exactly_its_range(env):
    hyper = R.HYPERS["default"]
    opt, case = _setup(env, 2, hyper)
    nt = len(opt.params)
    lo, hi = 5, R.I_OFF4 + 1                          # strictly inside; the misaligned view is the last of the middle range,
    assert 0 < lo < hi < nt and R.I_NOGRAD >= hi      # the tensor without a gradient sits in the last one
    first = True
    for a, b in ((0, nt), (0, lo), (lo, hi), (hi, nt)):
        opt.grad.fill_(SENTINEL)
        out = opt.pack_grads(refresh=first, lo=a, hi=b)       # (the two-bucket exchange refreshes once, too)
        first = False
        torch.cuda.synchronize()
        assert out is opt.grad
        got, want = opt.grad.cpu().numpy(), _expected_bucket(opt, case["g"], a, b)
        assert np.array_equal(_bits(got), _bits(want)), \
            f"pack_grads[{a}, {b}): {int((_bits(got) != _bits(want)).sum())} slots differ, first at " \
            f"{int(np.argmax(_bits(got) != _bits(want)))}"
    opt.grad.fill_(SENTINEL)
    opt.pack_grads(refresh=False, lo=lo, hi=lo)               # an empty range writes nothing
    torch.cuda.synchronize()
    assert np.array_equal(_bits(opt.grad.cpu().numpy()), _bits(_expected_bucket(opt, case["g"], 0, 0)))
    for k, (p, g) in enumerate(zip(opt.params, case["g"])):
        if g is not None:
            assert np.array_equal(_bits(p.grad.detach().cpu().numpy()), _bits(g)), k


# ------------------------------------------------------------------------------------------------ chained steps
def _case_of(opt, state, grads):
    per = _per_tensor(opt, state)
    return {"p": [b[0] for b in per], "m": [b[1] for b in per], "v": [b[2] for b in per], "g": grads}


def test_chained_eager_and_replayed_steps_each_match_one_oracle_step(env):
    """Eight eager steps with new gradients each, then ``opt.step(refresh=False)`` captured once (a single stream, no
    branches) and replayed three times over gradient tensors that keep their addresses, the rate halved between the second
    and the third replay.  Every step is judged from the device's OWN state in front of it (download, one fp64 step,
    compare), so no error accumulates into the bound: this pins the counter — one per step and per replay — and the
    device-scalar rate on the route the trainer takes."""
    hyper = R.HYPERS["default"]
    opt, case = _setup(env, 1, hyper)
    shapes = case["shapes"]
    rng = np.random.default_rng(11)
    worst = {"u": 0.0, "m": 0.0, "v": 0.0}

    def judged(t, grads, step, what):
        nonlocal worst
        before = _download(opt)
        h = _hyper_of(opt, 1.0)
        tol_u, _ = R.case_tol(_case_of(opt, before, grads), h, t)
        step()
        err = _judge(opt, before, grads, h, t, tol_u, "blocks", what)
        worst = {key: max(worst[key], err[key]) for key in worst}

    for t in range(1, 9):
        grads = R.gradients(rng, shapes, 1.0)
        _set_grads(opt, grads)
        judged(t, grads, opt.step, f"eager step {t}")

    grads = R.gradients(rng, shapes, 1.0)
    _set_grads(opt, grads)
    opt.refresh_table()                                        # (makes the transposed one contiguous: its address stays)
    static = [p.grad for p in opt.params]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with env.train._capture(graph):
        opt.step(refresh=False)
    torch.cuda.synchronize()
    assert int(opt.step_count.item()) == 8                     # the capture itself runs nothing
    lr0 = opt.lr
    for r in range(3):
        if r == 2:
            opt.param_groups[0]["lr"] = 0.5 * opt.param_groups[0]["lr"]
        grads = R.gradients(rng, shapes, 1.0)
        for s, g in zip(static, grads):
            if g is not None:
                s.copy_(torch.from_numpy(g))
        assert all(p.grad is s for p, s in zip(opt.params, static))
        judged(9 + r, grads, graph.replay, f"replay {r + 1}")
    assert opt.lr == 0.5 * lr0 and float(opt.lr_dev.item()) == float(np.float32(0.5 * lr0))
    print(f"\nadam chained (8 eager + 3 replays): u {worst['u']:.2e} of S_u  m {worst['m']:.2e}  v {worst['v']:.2e}")
