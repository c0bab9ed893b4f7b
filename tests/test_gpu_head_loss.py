"""The launches that close a train step — ops.LossHead (k_loss_head_fwd, one workgroup of 1024 threads, and
k_loss_head_bwd) and ops.HeadLoss (k_head_loss_fwd, 256 threads and 1024 / K rows per workgroup; k_head_loss_gram_fwd, the
same with the Gram losses as a second role of the grid; igcn_loss_final) — against the float64 reference of
tests/head_loss_ref.py at every head shape the kernels take another path for: the binary / four-target heads of the
trainer, one class, K / 4 from 1 to 64, ragged last workgroups, the scalar and the 16-byte reconstruction walks, second
trips of every loop of the one-workgroup kernel, more than 1024 partial rows, and lambda_loss[0] = 0.

Bounds (the ones this kernel family has in tests/test_gpu_ops.py): outputs and gradients 1e-5 of the reference's largest
magnitude (floor 1e-7), the loss and each term 1e-5 * max(1e-3, |reference|).  The worst figure per kernel and quantity is
printed when the module finishes (DESIGN.md section 2 records them)."""
import numpy as np
import pytest
import torch

import head_loss_ref as R
from calltrace import record_calls

pytestmark = pytest.mark.gpu

L_TEST, HP_TEST = [0.7, 1.0, 0.5, 1.5e-3, 0.1, 0.2], (1.3, 0.8)
L_MAIN, L_TRAINER, HP_ONE = [0, 1, 0.5, 1.5e-6, 0.1, 0], [1, 1, 1, 2.5e-6, 0.2, 0.2], (1.0, 1.0)
LAMS = {"L_TEST": (L_TEST, HP_TEST), "L_MAIN": (L_MAIN, HP_ONE), "L_TRAINER": (L_TRAINER, HP_ONE)}
TOL, FLOOR, TERM_FLOOR, UP = 1e-5, 1e-7, 1e-3, 1.7
WORST = {}                                           # (kernel, quantity) -> (worst error / scale, case)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()
    yield
    print("\nworst error relative to the reference's scale, per kernel and quantity:")
    for (kernel, what), (err, case) in sorted(WORST.items()):
        print(f"  {kernel:28s} {what:24s} {err:.3e}   ({case})")


def _note(kernel, what, rel, case):
    if rel > WORST.get((kernel, what), (-1.0, ""))[0]:
        WORST[(kernel, what)] = (rel, case)


def close(kernel, what, got, want, case):
    """conftest.assert_matches(got, want, TOL, floor=FLOOR), with the figure recorded before it is judged."""
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    assert tuple(g.shape) == tuple(w.shape), (what, tuple(g.shape), tuple(w.shape))
    scale = max(float(w.abs().max()) if w.numel() else 0.0, FLOOR)
    err = float((g - w).abs().max()) if w.numel() else 0.0
    _note(kernel, what, err / scale, case)
    assert np.isfinite(err) and err <= TOL * scale, f"{case}: {what}: max abs err {err:.3e}, rel {err / scale:.3e} > {TOL}"


def close_scalar(kernel, what, got, want, case):
    got, want = float(got.detach() if torch.is_tensor(got) else got), float(want)
    scale = max(TERM_FLOOR, abs(want))
    _note(kernel, what, abs(got - want) / scale, case)
    assert abs(got - want) <= TOL * scale, f"{case}: {what}: {got!r} vs {want!r} (rel {abs(got - want) / scale:.3e} > {TOL})"


def _unit():
    from igcn_amd import ops
    from igcn_amd.train import _unit_grad
    unit = _unit_grad(torch.zeros((), device="cuda"))                # the train step's cached d loss / d loss = 1
    assert unit is not None and unit.data_ptr() in ops.UNIT_GRAD_PTRS
    return unit


def _f32(rng, *shape, scale=1.0, uniform=False):
    a = rng.random(shape) if uniform else rng.standard_normal(shape)
    return torch.from_numpy((scale * a).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------- ops.LossHead
#        id                  B    C  NR  S   lambda       score amplitude, x_hat 4 bytes into a larger buffer
LOSS_HEAD_CASES = [
    ("smallest",             1,   2, 4, 54, "L_TEST",    3, False),
    ("scalar_walk",          37,  2, 4, 54, "L_TEST",    3, False),
    ("scalar_walk-main",     37,  2, 4, 54, "L_MAIN",    3, False),
    ("scalar_walk-trainer",  37,  2, 4, 54, "L_TRAINER", 3, False),
    ("scalar_walk-sharp",    37,  2, 4, 54, "L_TEST",    30, False),      # saturated softmax, exp underflows
    ("vector_walk",          36,  4, 1, 54, "L_TEST",    3, False),
    ("vector_walk-offset",   36,  4, 1, 54, "L_TEST",    3, True),        # same sizes, misaligned: the scalar walk
    ("one_class",            40,  1, 1, 7,  "L_TEST",    3, False),       # log_softmax = 0, ce = 0; odd S
    ("rows_1024",            512, 3, 3, 54, "L_TEST",    3, False),       # 2B = 1024; 13 824 quads: second batch of eight
    ("rows_1200",            600, 2, 4, 54, "L_TEST",    3, False),       # second trip of the row loops, second batch of
    ("rows_1200-main",       600, 2, 4, 54, "L_MAIN",    3, False),       # four, 1200 / 1100 partial rows
    ("rows_1200-trainer",    600, 2, 4, 54, "L_TRAINER", 3, False),
]
_LOSS_HEAD_REF = {}


def _loss_head_case(cid, b, c, nr, s, amp, from_logits):
    """Host inputs (float32, seeded) and the float64 reference for an upstream gradient of one: computed once per case."""
    key = (cid, from_logits)
    if key not in _LOSS_HEAD_REF:
        rng = np.random.default_rng(1000 * b + 10 * c + nr + amp)
        gram_rows, prob_rows = (1200, 1100) if b == 600 else (b, 19)
        scores = _f32(rng, 2 * b, c, scale=amp)
        if not from_logits:
            scores = torch.log_softmax(scores.double(), -1).float()
        ins = dict(scores=scores, reg=_f32(rng, 2 * b, nr), x_hat=_f32(rng, 2 * b, s),
                   gram=_f32(rng, gram_rows, 4, uniform=True), prob=_f32(rng, prob_rows, uniform=True))
        fixed = dict(y=torch.from_numpy(rng.integers(0, c, b)), clin=_f32(rng, b * nr, uniform=True),
                     snps=_f32(rng, b, s, uniform=True))
        assert all(bool(torch.isfinite(t).all()) for t in ins.values())
        _LOSS_HEAD_REF[key] = (ins, fixed, {})
    return _LOSS_HEAD_REF[key]


@pytest.mark.parametrize("from_logits", [True, False], ids=["scores", "logp"])
@pytest.mark.parametrize("cid,b,c,nr,s,lam_name,amp,offset", LOSS_HEAD_CASES, ids=[c[0] for c in LOSS_HEAD_CASES])
def test_loss_head_vs_fp64(monkeypatch, cid, b, c, nr, s, lam_name, amp, offset, from_logits):
    """ops.LossHead on raw scores and on log-probabilities, Gram terms and regulariser as partial rows: log_softmax, the
    loss, the seven terms and the gradients the FORWARD writes for the cached unit upstream (igcn_loss_head_fwd_grads, no
    backward launch) and those of igcn_loss_head_bwd for an upstream of 1.7 — all against float64."""
    from igcn_amd import ops
    lam, (hp_ce, hp_mi) = LAMS[lam_name]
    ins, fixed, refs = _loss_head_case(cid.split("-")[0] + ("-sharp" if amp != 3 else ""), b, c, nr, s, amp, from_logits)
    if lam_name not in refs:
        refs[lam_name] = R.loss_head(ins["scores"], fixed["y"], ins["reg"], fixed["clin"], ins["x_hat"], fixed["snps"],
                                     ins["gram"], ins["prob"], lam, hp_ce, hp_mi, 1.0, from_logits)
    ref = refs[lam_name]
    case = f"LossHead {cid} {'scores' if from_logits else 'logp'}"
    unit = _unit()
    names = ("scores", "reg", "x_hat", "gram", "prob")
    y, clin, snps = (fixed[k].cuda() for k in ("y", "clin", "snps"))
    seen = record_calls(monkeypatch)
    for upstream in (1.0, UP):
        leaves = {k: ins[k].cuda().requires_grad_(True) for k in names}
        if offset:
            buf = torch.zeros(2 * b * s + 1, device="cuda")
            buf[1:] = ins["x_hat"].cuda().reshape(-1)
            leaves["x_hat"] = buf[1:].view(2 * b, s).detach().requires_grad_(True)
            assert leaves["x_hat"].data_ptr() % 16 == 4 and leaves["x_hat"].is_contiguous()
        elif (b * s) % 4 == 0:
            assert leaves["x_hat"].data_ptr() % 16 == 0 and snps.data_ptr() % 16 == 0
        del seen[:]
        out = ops.LossHead.apply(leaves["scores"], y, leaves["reg"], clin, leaves["x_hat"], snps, leaves["gram"],
                                 leaves["prob"], lam, hp_ce, hp_mi, from_logits)
        go = unit if upstream == 1.0 else torch.full((), upstream, device="cuda")
        grads = torch.autograd.grad(out[0], [leaves[k] for k in names], grad_outputs=go)
        torch.cuda.synchronize()
        called = [c_[0] for c_ in seen]
        assert "igcn_loss_head_fwd_grads" in called and ("igcn_loss_head_bwd" in called) == (upstream != 1.0), called
        kern = "k_loss_head_fwd" if upstream == 1.0 else "k_loss_head_bwd"
        if upstream == 1.0:
            if from_logits:
                close(kern, "log_softmax", out[2], ref["logp"], case)
                if c == 1:
                    assert float(out[2].abs().max()) == 0.0
            close_scalar(kern, "loss", out[0], ref["loss"], case)
            for j, name in enumerate(R.TERMS):
                close_scalar(kern, "term " + name, out[1][j], ref["terms"][j], case)
            if c == 1 or lam[0] == 0:
                assert float(out[1][0]) == 0.0 and float(out[1][1]) == 0.0
        for name, g in zip(names, grads):
            want = ref["grads"][name]
            if want is None:                         # lam[0] == 0: the class scores are not part of the loss
                assert name == "scores" and lam[0] == 0
                assert tuple(g.shape) == tuple(ins[name].shape) and float(g.abs().max()) == 0.0, case
                continue
            close(kern, "d " + name, g, upstream * want, f"{case} upstream {upstream}")


# ---------------------------------------------------------------------------------------------------------- ops.HeadLoss
#        id              B    K    C  NR  S   keep   lambda
HEAD_LOSS_CASES = [
    ("k4",               1,   4,   1, 1, 7,  False, "L_TEST"),            # K / 4 = 1: 256 rows per workgroup, 2 live
    ("k8_nobias",        33,  8,   4, 1, 5,  False, "L_TEST"),            # K / 4 = 2, lin2.bias = None
    ("k32",              5,   32,  2, 4, 54, False, "L_TEST"),
    ("k16_ragged",       129, 16,  4, 4, 54, True,  "L_TEST"),            # 64 rows per workgroup, the last one holds 2
    ("k64_ragged",       37,  64,  2, 4, 54, True,  "L_TEST"),            # 16 rows per workgroup, the last one holds 10
    ("k64_ragged-main",  37,  64,  2, 4, 54, True,  "L_MAIN"),
    ("k64_ragged-trainer", 37, 64, 2, 4, 54, True,  "L_TRAINER"),
    ("k256",             3,   256, 3, 2, 54, True,  "L_TEST"),            # K / 4 = 64: one row per wave
    ("step",             256, 64,  2, 4, 54, True,  "L_TEST"),            # the step's own size, the trainer's heads
    ("step-main",        256, 64,  2, 4, 54, True,  "L_MAIN"),
    ("step-trainer",     256, 64,  2, 4, 54, True,  "L_TRAINER"),
]
HEAD_NAMES = ("hf", "w2", "b2", "hr", "w2r", "b2r", "x_hat", "gram", "prob")
_HEAD_LOSS_REF = {}


def _head_loss_case(cid, b, k, c, nr, s, keep, rd=None):
    """Host inputs and (per lambda set) the float64 reference for an upstream gradient of one: computed once per shape.
    ``rd``: also ``out_z`` [2B, rd] and ``tsne`` [B, 16] for the paired launch, whose Gram partials replace ``gram``."""
    key = (cid, rd)
    if key not in _HEAD_LOSS_REF:
        rng = np.random.default_rng(100000 * k + 100 * b + 10 * c + nr)
        def kp(p):
            return torch.from_numpy(((rng.random((2 * b, k)) > p) / (1 - p)).astype(np.float32)) if keep else None
        ins = dict(hf=_f32(rng, 2 * b, k).relu(), w2=_f32(rng, c, k, scale=0.3),
                   b2=None if "nobias" in cid else _f32(rng, c, scale=0.1), hr=_f32(rng, 2 * b, k).relu(),
                   w2r=_f32(rng, nr, k, scale=0.3), b2r=_f32(rng, nr, scale=0.1), x_hat=_f32(rng, 2 * b, s),
                   gram=_f32(rng, 7, 4, uniform=True), prob=_f32(rng, 11, uniform=True))
        fixed = dict(keep1=kp(0.5), keep2=kp(0.3), y=torch.from_numpy(rng.integers(0, c, b)),
                     clin=_f32(rng, b * nr, uniform=True), snps=_f32(rng, b, s, uniform=True))
        if rd is not None:
            fixed["out_z"] = _f32(rng, 2 * b, rd) + 0.3
            fixed["tsne"] = _f32(rng, b, 16, scale=3.0, uniform=True)
        _HEAD_LOSS_REF[key] = (ins, fixed, {})
    return _HEAD_LOSS_REF[key]


def _head_loss_ref(ins, fixed, refs, lam_name):
    if lam_name not in refs:
        lam, (hp_ce, hp_mi) = LAMS[lam_name]
        refs[lam_name] = R.head_loss(ins["hf"], fixed["keep1"], ins["w2"], ins["b2"], ins["hr"], fixed["keep2"], ins["w2r"],
                                     ins["b2r"], fixed["y"], fixed["clin"], ins["x_hat"], fixed["snps"], ins["gram"],
                                     ins["prob"], lam, hp_ce, hp_mi, 1.0)
    return refs[lam_name]


def _dev(t):
    return None if t is None else t.cuda()


def _run_head_loss(ops, ins, fixed, lam, hp, lazy, upstream, unit, gram=None, job=None, extra=()):
    """One ops.HeadLoss evaluation and its backward; ``lazy``: the loss value's last step is issued by the backward, inside
    ``deferred_reductions``, and everything is read after the block.  Returns (outputs, {name: gradient})."""
    leaves = {k: ins[k].cuda().requires_grad_(True) for k in HEAD_NAMES if ins[k] is not None}
    out = ops.HeadLoss.apply(leaves["hf"], _dev(fixed["keep1"]), leaves["w2"], leaves.get("b2"), leaves["hr"],
                             _dev(fixed["keep2"]), leaves["w2r"], leaves["b2r"], fixed["y"].cuda(), fixed["clin"].cuda(),
                             leaves["x_hat"], fixed["snps"].cuda(), leaves["gram"] if gram is None else gram, leaves["prob"],
                             lam, hp[0], hp[1], lazy, job)
    if gram is not None:
        del leaves["gram"]
    names = list(leaves)
    go = unit if upstream == 1.0 else torch.full((), upstream, device="cuda")
    targets = [leaves[k] for k in names] + list(extra)
    if lazy:
        with ops.deferred_reductions():
            grads = torch.autograd.grad(out[0], targets, grad_outputs=go)
    else:
        grads = torch.autograd.grad(out[0], targets, grad_outputs=go)
    torch.cuda.synchronize()
    return out, dict(zip(names + [f"extra{i}" for i in range(len(extra))], grads))


def _check_head_loss(kern, case, out, grads, ref, lam, upstream, skip_terms=()):
    loss, terms, logp, reg = out
    close(kern, "log_softmax", logp, ref["logp"], case)
    close(kern, "regression outputs", reg, ref["reg"], case)
    if not skip_terms:
        close_scalar(kern, "loss", loss, ref["loss"], case)
    for j, name in enumerate(R.TERMS):
        if name not in skip_terms:
            close_scalar(kern, "term " + name, terms[j], ref["terms"][j], case)
    if lam[0] == 0:
        assert float(terms[0]) == 0.0 and float(terms[1]) == 0.0, case
    for name in HEAD_NAMES:
        want = ref["grads"][name]
        if name not in grads:
            assert name == "gram" or want is None, name
            continue
        if want is None:                                 # lam[0] == 0: the classifier branch is not part of the loss
            assert lam[0] == 0 and name in ("hf", "w2", "b2") and float(grads[name].abs().max()) == 0.0, (case, name)
            continue
        close(kern, "d " + name, grads[name], upstream * want, f"{case} upstream {upstream}")


@pytest.mark.parametrize("lazy", [False, True], ids=["eager_value", "lazy_value"])
@pytest.mark.parametrize("cid,b,k,c,nr,s,keep,lam_name", HEAD_LOSS_CASES, ids=[c[0] for c in HEAD_LOSS_CASES])
def test_head_loss_vs_fp64(monkeypatch, cid, b, k, c, nr, s, keep, lam_name, lazy):
    """ops.HeadLoss (igcn_head_loss_fwd + igcn_loss_final): log_softmax, the regression outputs, the loss, the seven terms
    and the gradients of both feature blocks, both weights, both biases, x_hat, the Gram partials and the regulariser
    partials, for the cached unit upstream and for 1.7, with the loss value issued at once and lazily — against float64."""
    from igcn_amd import _lib, ops
    lam, hp = LAMS[lam_name]
    ins, fixed, refs = _head_loss_case(cid.split("-")[0], b, k, c, nr, s, keep)
    ref = _head_loss_ref(ins, fixed, refs, lam_name)
    unit = _unit()
    assert _lib.load().igcn_head_loss_supported(k, c, nr) == 1
    assert ops.head_loss_supported(ins["hf"].cuda(), ins["w2"].cuda(), ins["hr"].cuda(), ins["w2r"].cuda(),
                                   _dev(fixed["keep1"]), _dev(fixed["keep2"]))
    assert _lib.load().igcn_head_loss_blocks(b, k) == -(-2 * b // (1024 // k))
    seen = record_calls(monkeypatch)
    for upstream in (1.0, UP):
        del seen[:]
        out, grads = _run_head_loss(ops, ins, fixed, lam, hp, lazy, upstream, unit)
        called = [c_[0] for c_ in seen]
        assert "igcn_head_loss_fwd" in called and "igcn_loss_final" in called and "igcn_loss_head_fwd" not in called, called
        _check_head_loss("k_head_loss_fwd", f"HeadLoss {cid} lazy={lazy}", out, grads, ref, lam, upstream)
        assert ("b2" in grads) == (ins["b2"] is not None)


def test_head_loss_label_outside_the_classes_poisons_the_loss_only():
    """A label equal to C: the loss is NaN (F.nll_loss would raise on the host); log_softmax, the regression outputs and
    the regression and reconstruction gradients stay finite and equal to float64's."""
    from igcn_amd import ops
    cid, b, k, c, nr, s, keep, lam_name = HEAD_LOSS_CASES[4]
    lam, hp = LAMS[lam_name]
    ins, fixed, refs = _head_loss_case(cid, b, k, c, nr, s, keep)
    ref = _head_loss_ref(ins, fixed, refs, lam_name)
    bad = dict(fixed, y=fixed["y"].clone())
    bad["y"][b // 2] = c
    out, grads = _run_head_loss(ops, ins, bad, lam, hp, False, 1.0, _unit())
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[1][0]))
    case = "HeadLoss label = C"
    close("k_head_loss_fwd", "log_softmax", out[2], ref["logp"], case)
    close("k_head_loss_fwd", "regression outputs", out[3], ref["reg"], case)
    for name in ("hr", "w2r", "b2r", "x_hat"):
        close("k_head_loss_fwd", "d " + name, grads[name], ref["grads"][name], case)
    for j in (2, 3, 4, 5, 6):
        assert bool(torch.isfinite(out[1][j])), j
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())


@pytest.mark.parametrize("k,c,nr", [(6, 2, 4), (48, 2, 4), (512, 2, 4), (64, 5, 4), (64, 2, 5)],
                         ids=["K6", "K48", "K512", "C5", "NR5"])
def test_head_loss_refuses_what_it_does_not_cover(k, c, nr):
    """K not a multiple of four, K / 4 not a power of two, K / 4 > 64, more than four classes or targets: the launch does
    not cover the heads, ``ops.head_loss_supported`` sends the model to small_linear_pair + LossHead (which computes them:
    checked against float64 here), and asking ops.HeadLoss for them is an error, not another route."""
    from igcn_amd import _lib, ops
    b, s = 3, 54
    _unit()
    rng = np.random.default_rng(k + c + nr)
    ins = dict(hf=_f32(rng, 2 * b, k).relu(), w2=_f32(rng, c, k, scale=0.3), b2=_f32(rng, c, scale=0.1),
               hr=_f32(rng, 2 * b, k).relu(), w2r=_f32(rng, nr, k, scale=0.3), b2r=_f32(rng, nr, scale=0.1),
               x_hat=_f32(rng, 2 * b, s), gram=_f32(rng, 7, 4, uniform=True), prob=_f32(rng, 11, uniform=True))
    fixed = dict(keep1=None, keep2=None, y=torch.from_numpy(rng.integers(0, c, b)), clin=_f32(rng, b * nr, uniform=True),
                 snps=_f32(rng, b, s, uniform=True))
    assert _lib.load().igcn_head_loss_supported(k, c, nr) == 0
    assert _lib.load().igcn_head_loss_supported(64, 2, 4) == 1
    dev = {n: t.cuda().requires_grad_(True) for n, t in ins.items()}
    assert not ops.head_loss_supported(dev["hf"], dev["w2"], dev["hr"], dev["w2r"], None, None)
    with pytest.raises(_lib.IgcnError):
        _run_head_loss(ops, ins, fixed, L_TEST, HP_TEST, False, 1.0, _unit())
    # the chain the model takes instead
    logits, reg = ops.small_linear_pair(dev["hf"], dev["w2"], dev["b2"], None, dev["hr"], dev["w2r"], dev["b2r"], None)
    loss, terms, logp = ops.LossHead.apply(logits, fixed["y"].cuda(), reg, fixed["clin"].cuda(), dev["x_hat"],
                                           fixed["snps"].cuda(), dev["gram"], dev["prob"], L_TEST, *HP_TEST, True)
    grads = dict(zip(HEAD_NAMES, torch.autograd.grad(loss, [dev[n] for n in HEAD_NAMES], grad_outputs=_unit())))
    ref = R.head_loss(ins["hf"], None, ins["w2"], ins["b2"], ins["hr"], None, ins["w2r"], ins["b2r"], fixed["y"],
                      fixed["clin"], ins["x_hat"], fixed["snps"], ins["gram"], ins["prob"], L_TEST, *HP_TEST)
    _check_head_loss("small_linear_pair + LossHead", f"chain K={k} C={c} NR={nr}", (loss, terms, logp, reg), grads, ref,
                     L_TEST, 1.0)


PAIRED = [c for c in HEAD_LOSS_CASES if c[0].split("-")[0] in ("k64_ragged", "step")]


@pytest.mark.parametrize("cid,b,k,c,nr,s,keep,lam_name", PAIRED, ids=[c[0] for c in PAIRED])
def test_paired_head_loss_and_gram_launch_vs_fp64(monkeypatch, cid, b, k, c, nr, s, keep, lam_name):
    """igcn_head_loss_gram_fwd, reached as train._losses_batched reaches it: ops.GramLosses hands its launch over as a job
    (``hold``) and ops.HeadLoss runs it as a second role of its own grid.  Everything test_head_loss_vs_fp64 checks, with
    the cluster and orthogonality terms and d out_z against float64 oracle.sgcn_img_snp.consist_loss /
    orthogonal_constraint on out_z [2B, 40] and tsne [B, 16]; the recorded calls show the paired entry point ran and
    neither single launch did."""
    from igcn_amd import ops
    from oracle import sgcn_img_snp as OS
    lam, hp = LAMS[lam_name]
    rd, gamma = 40, 0.01
    ins, fixed, refs = _head_loss_case(cid.split("-")[0], b, k, c, nr, s, keep, rd)
    if "gram" not in refs:
        z = fixed["out_z"].double().requires_grad_(True)
        t64 = fixed["tsne"].double()
        c1, c2 = OS.consist_loss(z[:b], t64, gamma), OS.consist_loss(z[b:], t64, gamma)
        o1 = OS.orthogonal_constraint(z[:b])
        refs["gram"] = (z, torch.stack([c1, o1, c2, torch.zeros((), dtype=torch.float64)]))
    z, g4 = refs["gram"]
    key = "paired " + lam_name
    if key not in refs:
        refs[key] = R.head_loss(ins["hf"], fixed["keep1"], ins["w2"], ins["b2"], ins["hr"], fixed["keep2"], ins["w2r"],
                                ins["b2r"], fixed["y"], fixed["clin"], ins["x_hat"], fixed["snps"], g4.detach().view(1, 4),
                                ins["prob"], lam, hp[0], hp[1], 1.0)
        dz = torch.autograd.grad(lam[4] * (g4[0] + g4[2]) / 2 + lam[5] * g4[1], z, retain_graph=True)[0]
        refs[key]["grads"]["out_z"] = dz
    ref = refs[key]
    unit = _unit()
    seen = record_calls(monkeypatch)
    for upstream in (1.0, UP):
        del seen[:]
        out_z = fixed["out_z"].cuda().requires_grad_(True)
        job = {}
        gram = ops.GramLosses.apply(out_z, None, 2, "partials", (fixed["tsne"].cuda(), gamma), ops.unit_dgram(lam), None,
                                    job)
        assert "gram" in job and tuple(gram.shape) == (b, 4)
        assert not [c_ for c_ in seen if c_[0].startswith("igcn_gram_loss")], seen       # handed over, not launched
        out, grads = _run_head_loss(ops, ins, fixed, lam, hp, True, upstream, unit, gram=gram, job=job["gram"],
                                    extra=(out_z,))
        called = [c_[0] for c_ in seen]
        assert "igcn_head_loss_gram_fwd" in called and "igcn_head_loss_fwd" not in called \
            and "igcn_gram_loss_fwd_rbf_unit" not in called, called
        # a unit upstream takes the S the forward wrote; any other one the Gram loss backward kernel
        assert ("igcn_gram_loss_bwd" in called) == (upstream != 1.0), called
        case = f"paired {cid}"
        _check_head_loss("k_head_loss_gram_fwd", case, out, grads, ref, lam, upstream)
        close("k_head_loss_gram_fwd", "d out_z", grads["extra0"], upstream * ref["grads"]["out_z"],
              f"{case} upstream {upstream}")
        parts = gram.detach().double().cpu().sum(0)
        close_scalar("k_head_loss_gram_fwd", "consist (plain pass)", parts[0], g4[0], case)
        close_scalar("k_head_loss_gram_fwd", "orth (plain pass)", parts[1], g4[1], case)
        close_scalar("k_head_loss_gram_fwd", "consist (masked pass)", parts[2], g4[2], case)
