"""The Adam step of include/igcn.h (igcn_adam_step*, k_adam / k_adam_multi / k_adam_blocks in csrc/misc.hip) in plain
numpy: the float64 oracle, the float32 yardstick, the error scales and the one check every form is held to.

  adam_step_fp64(...)   torch.optim.Adam's single-tensor form (amsgrad off, weight_decay 0) in float64.  ``lr``, ``b1``,
                        ``b2``, ``eps`` and ``grad_scale`` are the FLOAT values the C ABI receives, widened to double: the
                        entry points take ``float``, so this is the operation the kernel is asked to do.
                        ``float_hyper=False`` keeps them true doubles (what torch.optim.Adam does; tests/test_adam_reference.py
                        measures the distance between the two).
  adam_step_fp32(...)   the same expression evaluated in numpy float32.  NOT a second oracle: the yardstick that says how far
                        a correct fp32 evaluation sits from the oracle (the float32 rounding of b2^t inside 1 - b2^t is
                        amplified by b2^t / (1 - b2^t) at small t).
  scales(...)           the cancellation-free magnitudes errors are judged against: S_m = |b1 m| + |(1-b1) gs g|,
                        S_u = lr/(1-b1^t) S_m / (sqrt(v')/sqrt(1-b2^t) + eps), and v' itself.  (|upd| is no scale: m' cancels
                        when b1 m ~ -(1-b1) g and the relative error of ANY fp32 evaluation is then unbounded.)
  yardstick_tol(...)    tol_u = 4 x the worst |upd_fp32 - upd| / S_u of the yardstick on the same inputs at the same t, floor
                        8 * 2^-24.  The yardstick's error is taken on the UPDATE it returns, not on p - upd: the last
                        subtraction rounds by up to ulp32(p')/2, which at p = O(1) is 1e-4 of S_u and would loosen tol_u a
                        hundredfold; check() grants that half ulp separately.
  check(...)            |m - m'| <= 4 * 2^-24 S_m ; |v - v'| <= 4 * 2^-24 v' ; |p - p'| <= tol_u S_u + ulp32(p')/2 ; where
                        S_u = 0 (gradient and first moment both zero) p and m are bit-identical to before, and so is v
                        where it was zero (a nonzero v next to a zero m still decays to b2 v, under the bound on v).
                        Every element takes part in every comparison.
  case_inputs(...)      the seeded parameter set of tests/test_gpu_adam.py (every chunk seam, ragged quads, a tensor without
                        a gradient, a zero tensor, the eps band), shared with the sensitivity tests of
                        tests/test_adam_reference.py so that the mutants are judged on the inputs the kernels get.
"""
import numpy as np

U24 = 2.0 ** -24
TOL_M = 4 * U24
TOL_V = 4 * U24
TOL_U_FLOOR = 8 * U24
YARD_FACTOR = 4.0
CHUNK = 1024            # igcn_adam_chunk() today; the GPU tests read the library's value and pass it in

# (lr, b1, b2, eps, grad_scale): the three hyper-parameter sets of the GPU cases
HYPERS = {
    "default": (1e-3, 0.9, 0.999, 1e-8, 1.0),
    "half": (1e-3, 0.9, 0.999, 1e-8, 0.5),
    "wide": (3e-2, 0.8, 0.99, 1e-3, 0.25),
}
STEPS = (1, 2, 3, 10, 1000, 20000)


def _hyper64(hyper, float_hyper=True):
    if float_hyper:
        return tuple(float(np.float32(h)) for h in hyper)
    return tuple(float(h) for h in hyper)


def adam_step_fp64(p, g, m, v, t, lr, b1, b2, eps, grad_scale, float_hyper=True):
    """(p', m', v', upd) of one step at counter value ``t`` (1 for the first step), float64."""
    lr, b1, b2, eps, gs = _hyper64((lr, b1, b2, eps, grad_scale), float_hyper)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g = g * gs
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    upd = lr / (1.0 - b1 ** t) * m1 / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** t) + eps)
    return p - upd, m1, v1, upd


def adam_step_fp32(p, g, m, v, t, lr, b1, b2, eps, grad_scale):
    """The same expression with every operation in numpy float32."""
    f = np.float32
    lr, b1, b2, eps, gs, one, tf = f(lr), f(b1), f(b2), f(eps), f(grad_scale), f(1), f(t)
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    g = g * gs
    m1 = b1 * m + (one - b1) * g
    v1 = b2 * v + (one - b2) * g * g
    bc1 = one - np.power(b1, tf, dtype=np.float32)
    bc2 = one - np.power(b2, tf, dtype=np.float32)
    upd = (lr / bc1) * (m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps))
    out = (p - upd, m1, v1, upd)
    assert all(a.dtype == np.float32 for a in out)
    return out


def scales(g, m, v, t, lr, b1, b2, eps, grad_scale):
    """(S_m, S_u, v') in float64, float-valued hyper-parameters."""
    lr, b1, b2, eps, gs = _hyper64((lr, b1, b2, eps, grad_scale))
    g, m, v = (np.asarray(a, dtype=np.float64) for a in (g, m, v))
    s_m = np.abs(b1 * m) + np.abs((1.0 - b1) * gs * g)
    v1 = b2 * v + (1.0 - b2) * (gs * g) ** 2
    s_u = lr / (1.0 - b1 ** t) * s_m / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** t) + eps)
    return s_m, s_u, v1


def ulp32(x):
    """Spacing of float32 at |x| (x float64): 2^(e-23) inside the normal range, 2^-149 below it."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)                                               # |x| = f * 2^e, f in [0.5, 1)
    return np.ldexp(1.0, np.where(x == 0, -149, np.maximum(e - 24, -149)))


def yardstick_error(before, g, hyper, t):
    """Worst |upd_fp32 - upd| / S_u of adam_step_fp32 over the elements with S_u > 0."""
    p, m, v = before
    _, _, _, u64 = adam_step_fp64(p, g, m, v, t, *hyper)
    _, _, _, u32 = adam_step_fp32(p, g, m, v, t, *hyper)
    _, s_u, _ = scales(g, m, v, t, *hyper)
    on = s_u > 0
    return float((np.abs(u32.astype(np.float64) - u64)[on] / s_u[on]).max()) if on.any() else 0.0


def yardstick_tol(before, g, hyper, t):
    return max(YARD_FACTOR * yardstick_error(before, g, hyper, t), TOL_U_FLOOR)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def check(got_p, got_m, got_v, before, g, hyper, t, tol_u, what):
    """Hold one tensor's (p, m, v) after a step to the oracle; ``before`` = (p, m, v) in front of it, all float32 arrays
    of one shape.  Returns the worst errors in units of their scales: {'u': ..., 'm': ..., 'v': ...} — 'u' is what is
    left of |p - p'| after the half ulp of the final subtraction, over S_u."""
    p0, m0, v0 = (np.asarray(a, dtype=np.float32).reshape(-1) for a in before)
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    got_p, got_m, got_v = (np.asarray(a, dtype=np.float32).reshape(-1) for a in (got_p, got_m, got_v))
    assert got_p.shape == got_m.shape == got_v.shape == p0.shape == m0.shape == v0.shape == g.shape, what
    assert np.isfinite(got_p).all() and np.isfinite(got_m).all() and np.isfinite(got_v).all(), f"{what}: not finite"
    p1, m1, v1, _ = adam_step_fp64(p0, g, m0, v0, t, *hyper)
    s_m, s_u, _ = scales(g, m0, v0, t, *hyper)

    def worst(err, bound, name):
        bad = err > bound
        if bad.any():
            k = int(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)))
            raise AssertionError(f"{what}: {name}[{k}] off by {err[k]:.3e}, bound {bound[k]:.3e} "
                                 f"({int(bad.sum())} of {err.size} elements; t={t}, g={g[k]!r}, m={m0[k]!r}, v={v0[k]!r})")

    e_m = np.abs(got_m.astype(np.float64) - m1)
    e_v = np.abs(got_v.astype(np.float64) - v1)
    e_p = np.abs(got_p.astype(np.float64) - p1)
    half = 0.5 * ulp32(p1)
    worst(e_m, TOL_M * s_m, "exp_avg")
    worst(e_v, TOL_V * v1, "exp_avg_sq")
    worst(e_p, tol_u * s_u + half, "param")
    still = s_u == 0                                   # gradient and first moment both zero: nothing may move
    if still.any():
        assert np.array_equal(_bits(got_p)[still], _bits(p0)[still]), f"{what}: a parameter moved under S_u = 0"
        assert np.array_equal(_bits(got_m)[still], _bits(m0)[still]), f"{what}: exp_avg moved under S_u = 0"
        flat = still & (v0 == 0)
        assert np.array_equal(_bits(got_v)[flat], _bits(v0)[flat]), f"{what}: exp_avg_sq moved under S_u = 0"
    on = ~still
    rel = lambda e, s, w: float((e[w] / s[w]).max()) if w.any() else 0.0      # noqa: E731
    return {"u": rel(np.maximum(e_p - half, 0.0), s_u, on), "m": rel(e_m, s_m, on), "v": rel(e_v, v1, v1 > 0)}


def check_untouched(got, before, what):
    """A tensor without a gradient under a table form: p, m and v bit-identical."""
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, before):
        assert np.array_equal(_bits(a).reshape(-1), _bits(b).reshape(-1)), f"{what}: {name} of a tensor without a gradient moved"


# ------------------------------------------------------------------------------------------------ the shared inputs
def case_shapes(chunk=CHUNK):
    c = chunk
    return [(1,), (3,), (4,), (5,), (17,), (c - 1,), (c,), (c + 1,), (c + 4,), (2 * c + 3,), (3 * c,), (5, 413), (7, 5), (37,)]


# roles by position in case_shapes()
I_OFF16, I_OFF4, I_TRANSPOSED, I_ZERO, I_NOGRAD = 8, 9, 11, 12, 13


def _loguniform(rng, n, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)) * rng.choice([-1.0, 1.0], n)


def gradients(rng, shapes, grad_scale):
    """One gradient per tensor (None for the one without): |g| log-uniform 1e-4 .. 1e2; every fifth element (from 2) in
    the band 1e-9 <= |g * grad_scale| <= 1e-7, where eps = 1e-8 decides the update; every seventh (from 3: never the
    only element of a tensor or its whole ragged tail) exactly zero; one tensor zero throughout."""
    out = []
    for k, s in enumerate(shapes):
        n = int(np.prod(s))
        if k == I_NOGRAD:
            out.append(None)
            continue
        g = _loguniform(rng, n, 1e-4, 1e2)
        band = np.arange(n) % 5 == 2
        g[band] = _loguniform(rng, int(band.sum()), 1e-9, 1e-7) / grad_scale
        g[np.arange(n) % 7 == 3] = 0.0
        if k == I_ZERO:
            g[:] = 0.0
        out.append(g.astype(np.float32).reshape(s))
    return out


def case_inputs(t, hyper, chunk=CHUNK, seed=0):
    """{'shapes', 'p', 'm', 'v', 'g'}: lists of float32 arrays, one per tensor of case_shapes(chunk).  Parameters span
    1e-6 .. 1 (so that ulp32(p')/2 does not hide the update), moments are zero for t = 1 and otherwise follow the
    gradient's band (v >= m^2, several decades); the tensor without a gradient keeps nonzero moments at every t, the
    zero tensor zero ones."""
    rng = np.random.default_rng([seed, t])
    shapes = case_shapes(chunk)
    gs = float(hyper[4])
    g = gradients(rng, shapes, gs)
    p, m, v = [], [], []
    for k, s in enumerate(shapes):
        n = int(np.prod(s))
        pk = _loguniform(rng, n, 1e-6, 1.0)
        mk = _loguniform(rng, n, 1e-5, 1e1)
        band = np.arange(n) % 5 == 2
        mk[band] = _loguniform(rng, int(band.sum()), 1e-9, 1e-7)
        mk[np.arange(n) % 11 == 3] = 0.0             # a zero first moment under a live gradient (and under a zero one)
        mk = mk.astype(np.float32)
        vk = (mk.astype(np.float64) ** 2 * np.exp(rng.uniform(0.0, np.log(1e3), n))).astype(np.float32)
        vk = np.maximum(vk, (mk * mk).astype(np.float32))           # v >= m^2 after the rounding too
        if (t == 1 and k != I_NOGRAD) or k == I_ZERO:
            mk[:] = 0.0
            vk[:] = 0.0
        p.append(pk.astype(np.float32).reshape(s))
        m.append(mk.reshape(s))
        v.append(vk.reshape(s))
    return {"shapes": shapes, "p": p, "m": m, "v": v, "g": g}


def flat_of(arrays, fill=None):
    """All tensors as one vector (a missing gradient as zeros), for the yardstick."""
    parts = []
    for k, a in enumerate(arrays):
        parts.append(np.zeros(int(np.prod(fill[k].shape)), np.float32) if a is None else np.asarray(a, np.float32).reshape(-1))
    return np.concatenate(parts)


def case_tol(case, hyper, t):
    """(tol_u, the yardstick's own worst error / S_u) of a case, over every element of every tensor."""
    before = tuple(flat_of(case[k]) for k in ("p", "m", "v"))
    g = flat_of(case["g"], fill=case["p"])
    y = yardstick_error(before, g, hyper, t)
    return max(YARD_FACTOR * y, TOL_U_FLOOR), y
