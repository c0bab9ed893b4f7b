"""ops.NodeLinearBN at the attention widths of the hidden-32 sweep (D = 64 on the row-coalesced `_q` kernels, D = 80..160
on the strip kernels k_nlbn_*_w, csrc/readout.hip) against the fp64 torch restatement test_node_linear_bn uses, at that
test's bounds: out / running statistics 1e-4, dx / dW / dgamma / dbeta 3e-4 with floor 1e-6, all scale-relative.

Shapes: the smallest at which each mechanism of the kernels can break —
  (6, 11, 1, train)    fewer nodes than one wave covers, samples per group not a multiple of 4
  (9, 77, 1, train), (6, 77, 1, eval)   shadow lanes in the last workgroup, both backward formulas
  (2, 33, 2, train)    one sample per group, three of four waves idle
  (80, 70, 2, train)   10 chunks per group on the statistics grid, above the 8-chunk clamp of the coalesced grid
  (5, 1, 1, train)     a single node
  (512, 400, 2, train) the benchmark's read-out, 32 chunks per group (D = 160 only)
D = 80, 112, 144 (a short last strip: D % 32 == 16) run on the shadow-lane shape.

ReLU decisions.  The derivative of the function jumps where a BatchNorm output crosses zero, and among the 1.8 M outputs of
(80, 70, 2) at D = 160 — 32.8 M at the benchmark's shape — some lie within fp32 rounding of zero, where fp32 and fp64
arithmetic may land on different sides (measured against the unmodified fp64 restatement: one such element at (80, 70, 2),
D = 160, moves dx by 1.3e-2 and dW by 5.3e-3 of their scales; at (512, 400, 2) dx 4.9e-3, dbeta 5.7e-4).  As the model tests
do (conftest.relu_forced, test_full_model_vs_oracle_larger), the kernels' decisions — ``out > 0`` — are imposed on the fp64
restatement INSIDE a band of 2e-5 of the tensor's largest pre-activation; outside the band the two must agree, the number
of imposed decisions is capped at one plus one per million outputs (fp32 rounding of ~1e-7 of the scale times a density of
order one per unit of scale gives a few per ten million), and the bounds stay as they are.  The wide kernels evaluate the
decision with the forward's own instruction sequence (ro_w_pre / ro_w_y), so forward, dgamma / dbeta and dx / dW stand on
the same decisions."""
import numpy as np
import pytest
import torch

from conftest import assert_matches

pytestmark = pytest.mark.gpu

TOL = 1e-4
MAIN = (64, 96, 128, 160)
SHAPES = [(6, 11, 1, True), (9, 77, 1, True), (6, 77, 1, False), (2, 33, 2, True), (80, 70, 2, True), (5, 1, 1, True)]
CASES = ([(b, n, d, t, g) for (b, n, g, t) in SHAPES for d in MAIN]
         + [(9, 77, d, True, 1) for d in (80, 112, 144)] + [(512, 400, 160, True, 2)])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


@pytest.fixture(scope="module")
def ops():
    from igcn_amd import ops
    return ops


_REF = {}


def _inputs(bsz, n, d, f=5):
    rng = np.random.default_rng(n + d)
    x = torch.from_numpy(rng.standard_normal((bsz, f, n)) + 0.5).float()
    w = torch.from_numpy(rng.standard_normal((d, f)) * 0.6).float()
    gamma = torch.from_numpy(1 + 0.2 * rng.standard_normal(n)).float()
    beta = torch.from_numpy(0.2 * rng.standard_normal(n)).float()
    rm0 = torch.from_numpy(0.1 * rng.standard_normal(n)).float()
    rv0 = torch.from_numpy(1 + 0.3 * rng.random(n)).float()
    cot = torch.from_numpy(rng.standard_normal((bsz, n, d))).float()
    return dict(inputs=(x, w, gamma, beta), rm0=rm0, rv0=rv0, cot=cot)


def _reference(c, training, groups, decided):
    """The fp64 restatement of test_node_linear_bn with the decisions ``decided`` [B, N, D] imposed inside the band."""
    from conftest import relu_forced
    ref_in = [t.double().requires_grad_(True) for t in c["inputs"]]
    rm, rv = c["rm0"].double().clone(), c["rv0"].double().clone()
    pre = ref_in[0].transpose(1, 2) @ ref_in[1].t()                       # [B,N,D]
    bg = pre.shape[0] // groups                                           # groups == successive module calls
    forced = {g: decided[g * bg:(g + 1) * bg] for g in range(groups)}     # one torch.relu call per group
    with relu_forced(forced, band=2e-5) as rf:
        out_ref = torch.cat([torch.relu(torch.nn.functional.batch_norm(
            pre[g * bg:(g + 1) * bg], rm, rv, ref_in[2], ref_in[3], training, 0.1, 1e-5)) for g in range(groups)])
    g_ref = torch.autograd.grad((out_ref * c["cot"].double()).sum(), ref_in)
    return dict(out=out_ref.detach().numpy(), grads=[g.numpy() for g in g_ref], rm=rm.numpy(), rv=rv.numpy(),
                flips=rf.flips, mismatch_outside=rf.mismatch_outside)


def _case(ops, bsz, n, d, training, groups):
    """Inputs, the kernels' results and the fp64 reference of one case (computed once, left unchanged)."""
    key = (bsz, n, d, training, groups)
    if key not in _REF:
        c = _inputs(bsz, n, d)
        c["got"] = _run(ops, c, training, groups)
        c.update(_reference(c, training, groups, c["got"][0].detach().cpu() > 0))
        _REF[key] = c
    return _REF[key]


def _run(ops, c, training, groups):
    dev = [t.cuda().requires_grad_(True) for t in c["inputs"]]
    rmg, rvg = c["rm0"].cuda(), c["rv0"].cuda()
    out = ops.NodeLinearBN.apply(dev[0], dev[1], dev[2], dev[3], rmg, rvg, training, 0.1, 1e-5, groups)
    g = torch.autograd.grad((out * c["cot"].cuda()).sum(), dev)
    return out, g, rmg, rvg


def _rel(got, want, floor=0.0):
    w = torch.from_numpy(np.asarray(want)).double()
    scale = max(float(w.abs().max()), floor, 1e-30)
    return float((got.detach().cpu().double() - w).abs().max()) / scale


@pytest.mark.parametrize("bsz,n,d,training,groups", CASES)
def test_wide_node_linear_bn_vs_fp64(ops, bsz, n, d, training, groups):
    c = _case(ops, bsz, n, d, training, groups)
    out, g, rmg, rvg = c["got"]
    names = ("dx", "dW", "dgamma", "dbeta")
    print(f"\n[B={bsz} N={n} D={d} train={training} groups={groups}] imposed decisions {c['flips']}, disagreeing outside "
          f"the band {c['mismatch_outside']}; rel err out {_rel(out, c['out']):.2e} "
          + " ".join(f"{nm} {_rel(a, b, 1e-6):.2e}" for nm, a, b in zip(names, g, c["grads"]))
          + f" running_mean {_rel(rmg, c['rm']):.2e} running_var {_rel(rvg, c['rv']):.2e}")
    assert c["mismatch_outside"] == 0 and c["flips"] <= 1 + out.numel() // 1000000, (c["mismatch_outside"], c["flips"])
    assert_matches(out, c["out"], TOL, "out")
    for got, want, nm in zip(g, c["grads"], names):
        assert_matches(got, want, 3e-4, nm, floor=1e-6)
    assert_matches(rmg, c["rm"], TOL, "running_mean")
    assert_matches(rvg, c["rv"], TOL, "running_var")


def test_wide_readout_is_deterministic(ops):
    """Forward + backward twice at (9, 77, 1, train), D = 96: partial rows summed in a fixed order, no atomics."""
    c = _inputs(9, 77, 96)
    first = _run(ops, c, True, 1)
    second = _run(ops, c, True, 1)
    for a, b in zip((first[0], *first[1], first[2], first[3]), (second[0], *second[1], second[2], second[3])):
        assert torch.equal(a, b)


def test_unsupported_width_names_the_supported_set(ops):
    from igcn_amd._lib import IgcnError
    x = torch.zeros(4, 5, 8, device="cuda")
    w = torch.zeros(176, 5, device="cuda")
    one, zero = torch.ones(8, device="cuda"), torch.zeros(8, device="cuda")
    assert not ops.node_linear_bn_supported(5, 176)
    with pytest.raises(IgcnError, match=r"unsupported \(F=5, D=176\); supported: F=5 with D in .* multiple of 16 from 64 "
                                        r"to 160"):
        ops.NodeLinearBN.apply(x, w, one, zero, zero.clone(), one.clone(), True, 0.1, 1e-5, 1)
