"""Adversarial sparse structures, fp64 references and case tables for the GO sparse kernels (csrc/go.hip,
csrc/spmm_long.h): the SNP <-> GO maps, the attention encoder layer and the decoder layer.

CPU only, deterministic from a seed.  Three parts:

a) ``make`` and the named recipes: row-major unique ``(rows, cols)`` as ``ops.Csr`` requires, with list lengths placed
   on the constants the kernels branch on — SPMM_HEAVY = GO_HEAVY = 12 (13 entries and more: the whole wave walks the
   list), the four-entry unrolled walks, the 64 * SPMM_LU = 192-entry prefix of the long walk;
b) the fp64 references of the map, the two layers and the layer + LayerNorm blocks (one oracle: tests/test_gpu_ops.py
   imports them too);
c) the case tables of tests/test_gpu_go_structures.py, each row naming the route it is there for
   (tests/test_go_structures_reference.py asserts on the CPU, through igcn_spmm_route / igcn_go_route, that it takes it).
"""
from collections import namedtuple

import numpy as np
import torch

PLANTED = (12, 13, 63, 64, 65, 192, 193, 230)
# list-length distribution of the ``short`` recipe: 0-4 entries, a third of the lists empty, mean 1.5 (the real DAG)
SHORT_P = (0.33, 0.20, 0.20, 0.17, 0.10)
# mirrors of csrc/go.hip: `#define GO_DEC_COLCAP 4096` (column indices of a decoder workgroup's rows kept in LDS up to
# that many) and `GO_DEC_T * GO_DEC_ITERS` = 1024 * 3 (rows per workgroup of k_go_decode_fwd_lds)
GO_DEC_COLCAP = 4096
GO_DEC_ROWS = 1024 * 3

Structure = namedtuple("Structure", "rows cols n_rows n_cols planted_rows planted_cols empty_row empty_col")


def _finish(pairs, n_rows, n_cols, planted_rows=None, planted_cols=None, empty_row=None, empty_col=None):
    rc = np.asarray(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    key = np.unique(rc[:, 0] * n_cols + rc[:, 1])
    return Structure(torch.from_numpy(key // n_cols), torch.from_numpy(key % n_cols), n_rows, n_cols,
                     dict(planted_rows or {}), dict(planted_cols or {}), empty_row, empty_col)


def _positions(n, count, rng):
    """``count`` distinct list ids in [0, n) (fewer when n is small): the first two inside one aligned group of 64 (one
    wave of the thread-per-list kernels), the last one n - 1, the others anywhere."""
    count = min(count, max(n - 1, 0))                  # one list stays free for the empty one
    if count <= 0:
        return []
    first = []
    if count >= 3:
        lo = 64 * int(rng.integers(0, max(n // 64, 1)))
        width = min(64, n - 1 - lo)
        if width >= 2:
            first = [lo + width // 8, lo + width * 5 // 8]
    taken = set(first) | {n - 1}
    others = [i for i in rng.permutation(n).tolist() if i not in taken][:count - len(first) - 1]
    return first + others + [n - 1]


def _planted_order(lengths, cap):
    """The capped lengths, longest first, the two shortest swapped: the first two (one wave) and the last (the last
    list) are longer than 12 whenever at least three are."""
    lens = sorted((min(int(x), cap) for x in lengths), reverse=True)
    return lens[:-2] + [lens[-1], lens[-2]] if len(lens) >= 3 else lens


def make(n_rows, n_cols, lengths, seed, planted_rows=(), planted_cols=(), row_range=None):
    """Row-major unique (rows, cols).  ``lengths``: a callable rng -> int array [n_rows] of the ordinary lists' lengths.
    ``planted_rows`` / ``planted_cols``: exact lengths of planted row / column lists, each capped at what the other
    dimension offers once the planted lists of the other side and one EMPTY row and column are set aside.  Planted rows
    take no entry in a planted column and vice versa, so both lengths are exact; ordinary rows may gain one entry per
    planted column.  ``row_range`` = (lo, hi): planted rows lie inside it."""
    rng = np.random.default_rng(seed)
    lo, hi = row_range if row_range is not None else (0, n_rows)
    pc = _positions(n_cols, len(planted_cols), rng)
    pr = [lo + r for r in _positions(hi - lo, len(planted_rows), rng)]
    planting = bool(pc or pr)
    empty_col = next(c for c in rng.permutation(n_cols).tolist() if c not in set(pc)) if planting else None
    empty_row = next(r for r in rng.permutation(n_rows).tolist() if r not in set(pr)) if planting else None
    out_c, out_r = set(pc) | {empty_col}, set(pr) | {empty_row}
    free_cols = np.asarray([c for c in range(n_cols) if c not in out_c], dtype=np.int64)
    free_rows = np.asarray([r for r in range(n_rows) if r not in out_r], dtype=np.int64)
    pairs = set()
    base = np.asarray(lengths(rng), dtype=np.int64)
    assert base.shape == (n_rows,)
    for r in free_rows.tolist():
        k = min(int(base[r]), free_cols.size)
        if k:
            pairs.update((r, int(c)) for c in rng.choice(free_cols, k, replace=False))
    got_r, got_c = {}, {}
    for r, want in zip(pr, _planted_order(planted_rows[:len(pr)] if len(pr) < len(planted_rows) else planted_rows,
                                          free_cols.size)):
        pairs.update((r, int(c)) for c in rng.choice(free_cols, want, replace=False))
        got_r[r] = want
    for c, want in zip(pc, _planted_order(planted_cols[:len(pc)] if len(pc) < len(planted_cols) else planted_cols,
                                          free_rows.size)):
        pairs.update((int(r), c) for r in rng.choice(free_rows, want, replace=False))
        got_c[c] = want
    return _finish(pairs, n_rows, n_cols, got_r, got_c, empty_row, empty_col)


def _short_lengths(n, p=SHORT_P):
    return lambda rng: rng.choice(len(p), size=n, p=np.asarray(p) / sum(p))


def short(n_rows, n_cols, seed):
    """List lengths 0-4, about a third of the rows empty."""
    return make(n_rows, n_cols, _short_lengths(n_rows), seed)


def planted(n_rows, n_cols, seed, lengths=PLANTED):
    """``short`` plus planted row lists and planted column lists of exactly ``lengths`` entries (capped), two of each
    side inside one aligned group of 64 lists, one on the last row and one on the last column, an empty row and column."""
    return make(n_rows, n_cols, _short_lengths(n_rows), seed, planted_rows=lengths, planted_cols=lengths)


def long(n_rows, n_cols, seed, planted_rows=(), spread=24):
    """Every row has at least 9 entries (nnz > 8 n_rows); the LAST rows carry the planted lengths, in the order given."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(9, 9 + spread, size=n_rows)
    plant = {}
    for k, want in enumerate(planted_rows):
        if k < n_rows:
            plant[n_rows - 1 - k] = min(int(want), n_cols)
            lens[n_rows - 1 - k] = plant[n_rows - 1 - k]
    pairs = set()
    for r in range(n_rows):
        k = min(int(lens[r]), n_cols)
        pairs.update((r, int(c)) for c in rng.choice(n_cols, k, replace=False))
    return _finish(pairs, n_rows, n_cols, plant)


def exact(n_rows, n_cols, nnz, seed):
    """Exactly ``nnz`` entries, anywhere (the nnz = 8 I | 8 I + 1 boundary of the list-length switch)."""
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice(n_rows * n_cols, nnz, replace=False)).astype(np.int64)
    return Structure(torch.from_numpy(key // n_cols), torch.from_numpy(key % n_cols), n_rows, n_cols, {}, {}, None, None)


def square_short(n, seed):
    return short(n, n, seed)


def square_planted(n, seed):
    """N x N, mean degree about 1.5 as in the real DAG, plus the planted row and column lists."""
    return planted(n, n, seed)


def decoder(n_rows, n_cols, head, seed):
    """Decoder structure (n_rows >= n_cols; the layer adds its self term on the last n_cols rows) with the planted lists.
    ``head`` sets how many entries the first GO_DEC_ROWS rows (the first workgroup of k_go_decode_fwd_lds) hold, on
    either side of GO_DEC_COLCAP with a margin of 2x: "dense" (2-5 per row: more than 2 * GO_DEC_COLCAP when there are
    GO_DEC_ROWS rows), "sparse" (0-2 per row, planted rows behind row GO_DEC_ROWS when there are that many: fewer than
    GO_DEC_COLCAP / 2)."""
    assert n_rows >= n_cols and head in ("dense", "sparse")
    if head == "dense":
        return make(n_rows, n_cols, lambda rng: rng.integers(2, 6, size=n_rows), seed, PLANTED, PLANTED)
    rng_rows = (GO_DEC_ROWS, n_rows) if n_rows > GO_DEC_ROWS + 16 else None
    return make(n_rows, n_cols, _short_lengths(n_rows, (0.80, 0.15, 0.05)), seed, PLANTED, PLANTED, row_range=rng_rows)


def head_entries(s):
    """Entries of the first GO_DEC_ROWS rows."""
    return int((s.rows < GO_DEC_ROWS).sum())


# ------------------------------------------------------------------------------------------------ fp64 references
def map_ref(rows, cols, n_rows, x, val):
    """y[b, c, i] = sum_{k in row i} val[c, k] x[b, cols[k]]; x [B, J], val [C, nnz] -> [B, C, n_rows]."""
    return torch.stack([torch.zeros(x.shape[0], n_rows, dtype=x.dtype).index_add(1, rows, x[:, cols] * val[c])
                        for c in range(val.shape[0])], dim=1)


def attn_ref(row, col, xd, w_inc, w_s, a_in, a_s):
    """GO attention encoder layer (go_model.py:226-244); xd [B, N, fin] -> [B, N, fout]."""
    bsz, nj, fout = xd.shape[0], xd.shape[1], w_inc.shape[0]
    x_in, x_s = xd @ w_inc.t(), xd @ w_s.t()
    v = torch.exp(torch.tanh(torch.cat([x_in[:, row], x_in[:, col]], 2) @ a_in.t())).squeeze(2)
    z = torch.zeros(bsz, nj, dtype=xd.dtype).index_add(1, row, v)
    alpha = v / z[:, row]
    return torch.zeros(bsz, nj, fout, dtype=xd.dtype).index_add(1, row, alpha.unsqueeze(2) * x_in[:, col]) \
        + x_s * torch.sigmoid(x_s @ a_s.t())


def decode_ref(row, col, n_rows, n_cols, xd, w_out, w_sout):
    """GO decoder layer (go_model.py:262-272): mean aggregation + the self term on the last n_cols rows;
    xd [B, n_cols, fin] -> [B, n_rows, fout]."""
    bsz, fout = xd.shape[0], w_out.shape[0]
    deg = torch.zeros(n_rows, dtype=xd.dtype).index_add(0, row, torch.ones(row.numel(), dtype=xd.dtype))
    agg = torch.zeros(bsz, n_rows, fout, dtype=xd.dtype).index_add(
        1, row, (xd @ w_out.t())[:, col] / deg[row].view(1, -1, 1))
    pad = torch.zeros_like(agg)
    pad[:, n_rows - n_cols:] = xd @ w_sout.t()
    return agg + pad


def ln_block_ref(y, gamma, beta, keep, pool):
    """fp64 dropout(relu(LayerNorm_over_nodes(y)))[:, pool:] for y [B, N, f] (go_model.py:246-251)."""
    z = torch.relu(torch.nn.functional.layer_norm(y.transpose(1, 2), (y.shape[1],), gamma, beta, 1e-5))
    if keep is not None:
        z = z * keep.double().unsqueeze(1)
    return z[:, :, pool:]


def attn_ln_ref(row, col, keep, pool, xd, w_inc, w_s, a_in, a_s, gamma, beta):
    return ln_block_ref(attn_ref(row, col, xd, w_inc, w_s, a_in, a_s), gamma, beta, keep, pool)


def decode_ln_ref(row, col, n_rows, n_cols, keep, xd, w_out, w_sout, gamma, beta):
    return ln_block_ref(decode_ref(row, col, n_rows, n_cols, xd, w_out, w_sout), gamma, beta, keep, 0)


def dense_of(rows, cols, n_rows, n_cols):
    """The 0/1 dense image [n_rows, n_cols] (fp64) of a structure: the cross-check of the references above."""
    a = torch.zeros(n_rows, n_cols, dtype=torch.float64)
    a[rows, cols] = 1.0
    return a


# ------------------------------------------------------------------------------------------------ case tables
# routes, as igcn_spmm_route / igcn_go_route name them (include/igcn.h)
LONG_LDS, TILED, WAVE, THREAD, DVAL_LDS, DVAL_GLOBAL = 0, 1, 2, 3, 4, 5
PASS_FWD, PASS_DX, PASS_DVAL = 0, 1, 2
OP_ATTN_BWD, OP_DECODE_FWD, OP_DECODE_BWD = 0, 1, 2
LDS, GLOBAL = 0, 1
BIG_LDS = 64 * 1024

# name, B, C, I, J, build() -> Structure, forward route, dx route, (dval route, tile), what the row is there for
MapCase = namedtuple("MapCase", "name B C I J build fwd dx dval why")
MAP_CASES = [
    MapCase("1", 11, 2, 300, 54, lambda: planted(300, 54, 101), TILED, LONG_LDS, (DVAL_LDS, 4),
            "dx sums over C in the long walk; dval tile 4 with a ragged last tile (11 = 2 * 4 + 3)"),
    MapCase("2", 9, 2, 41, 54, lambda: short(41, 54, 102), TILED, TILED, (DVAL_GLOBAL, 0),
            "dx: the two-channel loop of rows_tiled; dval global because I < J with C = 2"),
    MapCase("3", 9, 3, 300, 200, lambda: short(300, 200, 103), TILED, TILED, (DVAL_LDS, 4),
            "C = 3: the generic channel loop of rows_tiled (dx)"),
    MapCase("4a", 3, 1, 600, 1024, lambda: planted(600, 1024, 104), TILED, TILED, (DVAL_LDS, 4),
            "forward tiled at its limit of 1024 columns; dval with the column side long"),
    MapCase("4b", 3, 1, 600, 1025, lambda: planted(600, 1025, 105), THREAD, TILED, (DVAL_LDS, 4),
            "forward thread-per-row past 1024 columns, heavy rows present"),
    MapCase("5a", 3, 2, 512, 700, lambda: planted(512, 700, 106), TILED, TILED, (DVAL_GLOBAL, 0),
            "dx tiled at C * I = 1024"),
    MapCase("5b", 3, 2, 513, 700, lambda: planted(513, 700, 107), TILED, THREAD, (DVAL_GLOBAL, 0),
            "dx thread-per-column past C * I = 1024, heavy columns present"),
    MapCase("6-I1", 5, 1, 1, 3001, lambda: long(1, 3001, 108, (193,)), LONG_LDS, TILED, (DVAL_LDS, 4),
            "long walk, one list of 193 = 192 + 1; operand of 3001 floats: scalar staging"),
    MapCase("6-I54", 5, 1, 54, 3001, lambda: long(54, 3001, 109, (192, 193, 230, 700)), LONG_LDS, TILED, (DVAL_LDS, 4),
            "long walk: 54 lists (< one stride of 56), prefix boundary 192 | 193, a 700-entry list on the last rows"),
    MapCase("6-I57", 5, 1, 57, 3001, lambda: long(57, 3001, 110, (192, 193, 230, 700)), LONG_LDS, TILED, (DVAL_LDS, 4),
            "long walk: 57 lists = one stride of NWV * SPMM_RM = 56 and one more"),
    MapCase("7", 3, 1, 20, 20000, lambda: long(20, 20000, 111), LONG_LDS, TILED, (DVAL_LDS, 1),
            "forward long_lds above 64 KB of LDS; dval tile 1"),
    MapCase("8", 2, 1, 4, 38404, lambda: long(4, 38404, 112), WAVE, TILED, (DVAL_GLOBAL, 0),
            "forward wave-per-row: the operand vector is 16 bytes above 150 KB; dval tile 0"),
    MapCase("9", 2, 2, 19204, 6, lambda: exact(19204, 6, 3000, 113), TILED, WAVE, (DVAL_GLOBAL, 0),
            "dx wave-per-column: C * I floats are above 150 KB"),
    MapCase("10", 3, 2, 10000, 54, lambda: planted(10000, 54, 114), TILED, LONG_LDS, (DVAL_LDS, 1),
            "dx long_lds above 64 KB of LDS; dval tile 1 with the row side long"),
    MapCase("11", 3, 1, 10000, 8, lambda: short(10000, 8, 115), TILED, LONG_LDS, (DVAL_LDS, 3), "dval tile 3"),
    MapCase("12", 3, 2, 7000, 8, lambda: short(7000, 8, 116), TILED, LONG_LDS, (DVAL_LDS, 2), "dval tile 2"),
    MapCase("13", 3, 1, 100, 300, lambda: exact(100, 300, 800, 117), TILED, TILED, (DVAL_LDS, 4),
            "nnz = 8 I: still the short-list kernel"),
    MapCase("14", 3, 1, 100, 300, lambda: exact(100, 300, 801, 118), LONG_LDS, TILED, (DVAL_LDS, 4),
            "nnz = 8 I + 1: the long walk"),
]
MAP_BY_NAME = {c.name: c for c in MAP_CASES}
# LDS launches above 64 KB (the kernel's limit is raised first): (case, pass)
MAP_BIG_LDS = [("7", PASS_FWD), ("10", PASS_DX), ("7", PASS_DVAL), ("10", PASS_DVAL)]

# fin, N, (route, threads, passes): both sides of every switch point of k_go_attn_bwd_lds<FIN, FOUT, MAXIT, T>
EncCase = namedtuple("EncCase", "fin n route")
ENC_CASES = [EncCase(2, n, r) for n, r in (
    (512, (LDS, 512, 1)), (513, (LDS, 512, 2)), (1024, (LDS, 512, 2)), (1025, (LDS, 512, 3)), (1536, (LDS, 512, 3)),
    (1537, (LDS, 512, 4)), (1860, (LDS, 512, 4)), (1861, (LDS, 1024, 2)), (2048, (LDS, 1024, 2)), (2049, (LDS, 1024, 3)),
    (3072, (LDS, 1024, 3)), (3073, (LDS, 1024, 4)), (3720, (LDS, 1024, 4)), (3721, (GLOBAL, 256, 0)))] + \
    [EncCase(5, n, r) for n, r in (
        (512, (LDS, 512, 1)), (513, (LDS, 512, 2)), (1024, (LDS, 512, 2)), (1025, (LDS, 512, 3)), (1460, (LDS, 512, 3)),
        (1461, (LDS, 1024, 2)), (2048, (LDS, 1024, 2)), (2049, (LDS, 1024, 3)), (2924, (LDS, 1024, 3)),
        (2925, (GLOBAL, 256, 0)))]
# every (fin, threads, passes) the LDS-resident backward can run with in default mode (the table of switch points)
ENC_REACHABLE = {(2, 512, p) for p in (1, 2, 3, 4)} | {(2, 1024, p) for p in (2, 3, 4)} | \
                {(5, 512, p) for p in (1, 2, 3)} | {(5, 1024, p) for p in (2, 3)}
# walk-order identity check: one case per workgroup size
ENC_WALK_ORDER = [(2, 1536), (2, 2049)]
# encoder + LayerNorm (2 -> 5): N, pool, igcn_go_attn_ln_fused_ok
ENC_LN_CASES = [(1024, 512, 1), (1536, 768, 1), (1860, 928, 1), (2048, 1024, 1), (3720, 1860, 1),
                (3724, 1860, 0),       # global: the two-pass fallback
                (1862, 928, 0)]        # N % 4 != 0: fallback

# Nin, Nout, fout, head, forward (route, workgroups per sample), backward at B = 130 (route, threads), ln_fused_ok
DecCase = namedtuple("DecCase", "nin nout fout head fwd bwd ln_ok")
DEC_CASES = [
    DecCase(1200, 4000, 5, "dense", (LDS, 2), (LDS, 1024), 1),      # two forward workgroups per sample: bx = 1
    DecCase(1200, 4000, 5, "sparse", (LDS, 2), (LDS, 1024), 1),
    DecCase(600, 6200, 5, "dense", (LDS, 3), (GLOBAL, 256), 0),     # three forward workgroups; backward beyond LDS
    DecCase(600, 6200, 5, "sparse", (LDS, 3), (GLOBAL, 256), 0),
    DecCase(1842, 2000, 5, "sparse", (LDS, 1), (LDS, 1024), 1),     # forward: 5 * 1842 = 9210 <= 9212 floats
    DecCase(1843, 2000, 5, "sparse", (GLOBAL, 0), (LDS, 1024), 1),  # forward: 9215 floats, global
    DecCase(512, 2120, 5, "dense", (LDS, 1), (LDS, 512), 0),        # backward T switch: 512 threads up to here
    DecCase(512, 2121, 5, "dense", (LDS, 1), (LDS, 1024), 0),       # one more output node: 1024
    DecCase(513, 2121, 5, "sparse", (LDS, 1), (LDS, 1024), 0),      # one more input node: 1024
    DecCase(400, 4256, 5, "sparse", (LDS, 2), (LDS, 1024), 0),      # backward LDS up to here
    DecCase(400, 4257, 5, "sparse", (LDS, 2), (GLOBAL, 256), 0),    # global
    DecCase(512, 6740, 2, "sparse", (LDS, 3), (LDS, 512), 0),       # 5 -> 2: the butterfly parameter-gradient path
]
DEC_BATCHES = (3, 130)       # thread-per-node backward | one workgroup per sample
