"""numpy restatement of the two recurrences of the tiled GDC route (csrc/gdc_tiled.hip) — TEST INFRASTRUCTURE ONLY.
Both diffusion matrices from fp64 matrix products with non-negative terms, the number of terms J and the scaling
exponent s chosen as the kernels choose them:

    H = D^-1/2 A D^-1/2,  D = diag(row sums of A)
    PPR   alpha (I - G)^-1 = alpha prod_{j<J} (I + G^(2^j)),  G = (1 - alpha) H,  J = ceil(log2(ln 2^-60 / ln(1 - alpha)))
          Q <- G, P <- I + G;  J - 1 times:  Q <- Q Q,  P <- P + P Q
    heat  e^-t expm(t H):  X = t H / 2^s, s the smallest s >= 0 with |X|_1 <= 1/2 (capped at the number of squarings the
          host launches, ceil(log2(2 t sqrt(R)))); T_14 = I + X / 14, T_j = I + X T_(j+1) / j; then s squarings

Held to oracle/gdc.ppr_matrix (numpy's inverse) and tests/gdc_heat_ref.heat_matrix (scipy's expm) by
tests/test_gdc_tiled_reference.py.
"""
import math

import numpy as np

HEAT_DEGREE = 14
ALPHA_MIN = 1e-3          # the smallest alpha of the interface: J(1e-3) = 16
MAX_ROIS = 512
TILE = 64                 # matrices are padded to a multiple of this


def ppr_terms(alpha):
    if alpha >= 1.0:
        return 1
    return max(1, math.ceil(math.log2((-60.0 * math.log(2.0)) / math.log(1.0 - alpha))))


def heat_max_squarings(t, rois):
    return max(0, math.ceil(math.log2(2.0 * t * math.sqrt(rois))))


def normalised(adj):
    adj = np.asarray(adj, dtype=np.float64)
    d = 1.0 / np.sqrt(adj.sum(axis=1))
    return (d[:, None] * adj) * d[None, :]


def heat_norm(adj, t):
    """|t H|_1: what the scaling exponent is chosen from."""
    return float(np.abs(t * normalised(adj)).sum(axis=0).max())


def heat_exponent(adj, t):
    nrm, s, smax = heat_norm(adj, t), 0, heat_max_squarings(t, np.asarray(adj).shape[0])
    while nrm > 0.5 and s < smax:
        nrm *= 0.5
        s += 1
    return s


def ppr_matrix(adj, alpha):
    g = (1.0 - alpha) * normalised(adj)
    q, p = g, np.eye(g.shape[0]) + g
    for _ in range(ppr_terms(alpha) - 1):
        q = q @ q
        p = p + p @ q
    return alpha * p


def heat_matrix(adj, t):
    s = heat_exponent(adj, t)
    x = (t * normalised(adj)) * math.ldexp(1.0, -s)
    eye = np.eye(x.shape[0])
    tm = eye + x / HEAT_DEGREE
    for j in range(HEAT_DEGREE - 1, 0, -1):
        tm = eye + (x @ tm) * (1.0 / j)
    for _ in range(s):
        tm = tm @ tm
    return math.exp(-t) * tm


def diffusion_matrix(adj, kernel, param):
    return ppr_matrix(adj, param) if kernel == "ppr" else heat_matrix(adj, param)


def workspace_bytes(graphs, rois, kernel):
    """What include/igcn.h states for igcn_gdc_tiled_workspace_bytes."""
    rp = (rois + TILE - 1) // TILE * TILE
    return graphs * ((4 if kernel == "ppr" else 3) * rp * rp * 8 + 32 * rp + 80)
