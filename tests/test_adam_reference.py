"""CPU checks of tests/adam_ref.py, the oracle tests/test_gpu_adam.py holds the Adam kernels to:

* the float64 oracle with true double betas IS torch.optim.Adam (float64 parameters, 12 steps, the rate halved after the
  sixth, one parameter that never receives a gradient): <= 1e-12 relative on parameters and both moments;
* how far the FLOAT betas / rate / eps of the C ABI move a step from true doubles — the documented distance between this ABI
  and torch: <= 2e-5 of S_u on the update and <= 2e-5 relative on exp_avg_sq (measured 6.7e-6 and 1.3e-5 on
  the GPU test's inputs, the latter from 1 - float32(0.999));
* sensitivity: ``check`` at the tolerance the yardstick yields on the GPU test's own inputs rejects every mutated copy of
  the oracle below, and accepts the oracle rounded to float32 and the float32 yardstick itself.
"""
import numpy as np
import pytest
import torch

import adam_ref as R


# ------------------------------------------------------------------------------------------------ the oracle is torch's Adam
def test_fp64_oracle_is_torch_adam():
    rng = np.random.default_rng(7)
    shapes = [(7, 5), (33,), (2, 3, 4), (129,), (6,)]
    no_grad = 4
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p = [rng.standard_normal(s) for s in shapes]
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in p]
    opt = torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    m = [np.zeros(s) for s in shapes]
    v = [np.zeros(s) for s in shapes]
    for t in range(1, 13):
        if t == 7:
            lr *= 0.5
            for group in opt.param_groups:
                group["lr"] = 0.5 * group["lr"]
        for k, s in enumerate(shapes):
            if k == no_grad:
                ps[k].grad = None
                continue
            g = rng.standard_normal(s) * 10.0 ** rng.integers(-3, 2)
            ps[k].grad = torch.from_numpy(g.copy())
            p[k], m[k], v[k], _ = R.adam_step_fp64(p[k], g, m[k], v[k], t, lr, b1, b2, eps, 1.0, float_hyper=False)
        opt.step()
    state = opt.state_dict()["state"]
    assert no_grad not in state
    assert np.array_equal(ps[no_grad].detach().numpy(), p[no_grad])
    for k in range(len(shapes)):
        if k == no_grad:
            continue
        assert float(state[k]["step"]) == 12
        for name, got, want in (("param", ps[k].detach().numpy(), p[k]), ("exp_avg", state[k]["exp_avg"].numpy(), m[k]),
                                ("exp_avg_sq", state[k]["exp_avg_sq"].numpy(), v[k])):
            rel = np.abs(got - want) / np.abs(want)
            assert rel.max() <= 1e-12, f"{name}[{k}]: {rel.max():.3e}"


# ------------------------------------------------------------------------------------------------ float betas vs true betas
@pytest.mark.parametrize("t", R.STEPS)
@pytest.mark.parametrize("hname", list(R.HYPERS))
def test_float_hyperparameters_stay_within_2e5_of_true_ones(hname, t):
    hyper = R.HYPERS[hname]
    case = R.case_inputs(t, hyper)
    p, m, v = (R.flat_of(case[k]) for k in ("p", "m", "v"))
    g = R.flat_of(case["g"], fill=case["p"])
    _, _, v_f, u_f = R.adam_step_fp64(p, g, m, v, t, *hyper)
    _, _, v_d, u_d = R.adam_step_fp64(p, g, m, v, t, *hyper, float_hyper=False)
    _, s_u, _ = R.scales(g, m, v, t, *hyper)
    on = s_u > 0
    d_u = float((np.abs(u_f - u_d)[on] / s_u[on]).max())
    d_v = float((np.abs(v_f - v_d)[v_d > 0] / v_d[v_d > 0]).max())
    print(f"float vs true hyper-parameters [{hname}, t={t}]: update {d_u:.2e} of S_u, exp_avg_sq {d_v:.2e} relative")
    assert d_u <= 2e-5 and d_v <= 2e-5, (d_u, d_v)


# ------------------------------------------------------------------------------------------------ sensitivity
def _mutant(kind, p, g, m, v, t, hyper, chunk=R.CHUNK):
    """(p', m', v') of a mutated copy of the oracle, float64 from float-valued hyper-parameters."""
    lr, b1, b2, eps, gs = (float(np.float32(h)) for h in hyper)
    shape = np.shape(p)
    p, g, m, v = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (p, g, m, v))
    if kind == "t_minus_1":
        t = t - 1
    elif kind == "t_plus_1":
        t = t + 1
    elif kind == "betas_swapped":
        b1, b2 = b2, b1
    gg = g * gs
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * (gs * g * g if kind == "scale_once_in_square" else gg * gg)
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1, bc2 = np.float64(1.0) - np.float64(b1) ** t, np.float64(1.0) - np.float64(b2) ** t      # (0 at t = 0)
        if kind == "eps_before_correction":
            denom = (np.sqrt(v1) + eps) / np.sqrt(bc2)
        elif kind == "correction_without_sqrt":
            denom = np.sqrt(v1) / bc2 + eps
        else:
            denom = np.sqrt(v1) / np.sqrt(bc2) + eps
        p1 = p - lr / bc1 * m1 / denom
    if kind == "seam_element_skipped":
        p1[chunk], m1[chunk], v1[chunk] = p[chunk], m[chunk], v[chunk]
    elif kind == "ragged_tail_skipped":
        k = p.size - p.size % 4
        p1[k:], m1[k:], v1[k:] = p[k:], m[k:], v[k:]
    return tuple(a.astype(np.float32).reshape(shape) for a in (p1, m1, v1))


FORMULA_MUTANTS = ["eps_before_correction", "correction_without_sqrt", "t_minus_1", "t_plus_1", "scale_once_in_square",
                   "betas_swapped"]
# Both hyper-parameter sets with grad_scale != 1 (mutant (d) is the oracle itself at 1).  With b2 = 0.99, b2^1000 = 4e-5:
# mutants (a)-(c) sit within float32 rounding of the oracle there, so that set is judged at t = 1 and 10.
SENS_CASES = [("half", 1), ("half", 10), ("half", 1000), ("wide", 1), ("wide", 10)]


@pytest.fixture(scope="module", params=SENS_CASES, ids=lambda c: f"{c[0]}-t{c[1]}")
def sens(request):
    hname, t = request.param
    hyper = R.HYPERS[hname]
    case = R.case_inputs(t, hyper)
    tol_u, _ = R.case_tol(case, hyper, t)
    return hyper, t, case, tol_u


def _judge(step, sens, only=None):
    """Run ``step`` on every tensor with a gradient and hand the result to check; the number of tensors check rejects."""
    hyper, t, case, tol_u = sens
    rejected = 0
    for k, g in enumerate(case["g"]):
        if g is None or (only is not None and k not in only):
            continue
        before = (case["p"][k], case["m"][k], case["v"][k])
        got = step(*before, g, k)
        try:
            R.check(*got, before, g, hyper, t, tol_u, f"tensor {k}")
        except AssertionError:
            rejected += 1
    return rejected


def test_check_accepts_the_rounded_oracle_and_the_yardstick(sens):
    hyper, t, _, _ = sens

    def rounded(p, m, v, g, k):
        return tuple(a.astype(np.float32) for a in R.adam_step_fp64(p, g, m, v, t, *hyper)[:3])

    def yard(p, m, v, g, k):
        return R.adam_step_fp32(p, g, m, v, t, *hyper)[:3]

    assert _judge(rounded, sens) == 0
    assert _judge(yard, sens) == 0


@pytest.mark.parametrize("kind", FORMULA_MUTANTS)
def test_check_rejects_formula_mutants(sens, kind):
    hyper, t, case, _ = sens
    n = sum(g is not None for g in case["g"])
    rejected = _judge(lambda p, m, v, g, k: _mutant(kind, p, g, m, v, t, hyper), sens)
    assert rejected >= 1, f"{kind} survives at t={t}: the inputs are too tame"
    print(f"{kind}: rejected on {rejected} of {n} tensors")


def test_check_rejects_a_skipped_seam_element_and_a_skipped_ragged_tail(sens):
    hyper, t, case, _ = sens
    past_seam = [k for k, s in enumerate(case["shapes"]) if int(np.prod(s)) > R.CHUNK and k != R.I_NOGRAD]
    ragged = [k for k, s in enumerate(case["shapes"]) if int(np.prod(s)) % 4 and k not in (R.I_NOGRAD, R.I_ZERO)]
    assert len(past_seam) >= 4 and len(ragged) >= 6
    for k in past_seam:                                             # every tensor that reaches a seam, one by one
        assert _judge(lambda p, m, v, g, _: _mutant("seam_element_skipped", p, g, m, v, t, hyper), sens, only=[k]) == 1, k
    for k in ragged:
        assert _judge(lambda p, m, v, g, _: _mutant("ragged_tail_skipped", p, g, m, v, t, hyper), sens, only=[k]) == 1, k


def test_a_gradientless_tensor_stepped_with_zeros_is_rejected(sens):
    hyper, t, case, tol_u = sens
    k = R.I_NOGRAD
    assert case["g"][k] is None
    before = (case["p"][k], case["m"][k], case["v"][k])
    assert np.count_nonzero(before[1]) and np.count_nonzero(before[2])      # seeded: a zero state would hide it
    R.check_untouched(before, before, "identity")
    got = tuple(a.astype(np.float32) for a in R.adam_step_fp64(*before[:1], np.zeros_like(before[0]), *before[1:], t, *hyper)[:3])
    with pytest.raises(AssertionError):
        R.check_untouched(got, before, "stepped with zeros")


def test_scales_and_ulp():
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(0.75) == 2.0 ** -24 and R.ulp32(0.0) == 2.0 ** -149
    assert R.ulp32(-3.0) == float(np.spacing(np.float32(3.0)))
    # m' cancels, the scales do not
    s_m, s_u, v1 = R.scales(np.float32([-9.0]), np.float32([1.0]), np.float32([4.0]), 5, 1e-3, 0.9, 0.999, 1e-8, 1.0)
    assert abs(s_m[0] - 1.8) < 1e-6 and s_u[0] > 0 and v1[0] > 0
    _, m1, _, upd = R.adam_step_fp64(np.float32([0.0]), np.float32([-9.0]), np.float32([1.0]), np.float32([4.0]), 5, 1e-3, 0.9,
                                    0.999, 1e-8, 1.0)
    assert abs(m1[0]) < 1e-6 and abs(upd[0]) < 1e-6 * s_u[0] * 10
