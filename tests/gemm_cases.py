"""The case table of the GEMM leaf sweep (csrc/gemm.hip), shared by tests/test_gemm_plan.py (CPU: which template
instantiation the host code picks for each case, queried through igcn_gemm_plan) and tests/test_gpu_gemm_leaves.py
(GPU: every case against an exact integer oracle).  Plain Python: no torch, no device.

A case is one call of igcn_gemm_f32 / igcn_gemm_bf16.  The operands live at an element offset (0, 1 or 2 floats) from a
16-byte-aligned base, A and B are k-contiguous ([rows, K] storage) or row-contiguous ([K, rows] storage), C has a padded
leading dimension.  Every case names the leaf (bn, vw, pf, arf, brf) it was built to reach; the CPU test holds the plan
query to it, so a change of the launch heuristics that moves a case to another leaf fails there and the table gets a new
shape.

How the recipe reaches a leaf:
  bn   (M, N): N <= 16 -> 16, N <= 32 -> 32, M >= 32768 -> 64, otherwise 16 while there are fewer than 128 tiles
  vw   a k-contiguous operand reads 4 / 2 / 1 floats per load by K mod 4, a row-contiguous one by its row count mod 4;
       a pointer at an odd float offset forces 1, at 2 floats at most 2; the narrower operand decides
  pf   1 for one or two 32-deep K steps per slice, 2 above
"""
from collections import namedtuple

Case = namedtuple("Case", "name M N K arf brf offa offb offc pad split bias act bf16 leaf")

# sum_form values of igcn_gemm_plan (include/igcn.h)
SUM_NONE, SUM_WALK, SUM_TREE, SUM_FINAL, SUM_LEFT = 0, 1, 2, 3, 4
ACT_FINAL, ACT_LEAVE = 0x100, 0x200

# (M, N) by tile width and by what the row counts allow a row-contiguous operand:
#   "s4": M % 4 == N % 4 == 0        "m2": M % 4 == 2        "n2": N % 4 == 2       "m1" / "n1": odd M / odd N
SHAPES = {
    16: {"s4": [(132, 16), (132, 12)], "m2": (130, 16), "n2": None, "m1": (63, 48), "n1": (130, 7)},
    32: {"s4": [(132, 32), (132, 32)], "m2": (66, 30), "n2": (66, 30), "m1": (65, 32), "n1": (130, 17)},
    64: {"s4": [(32768, 64), (32768, 64)], "m2": None, "n2": None, "m1": (32773, 33), "n1": (32773, 33)},
}

# K by (K mod 4 class, pf): (unsplit K with few steps, unsplit K with more steps, (K, forced split_k))
#   pf 1: 1 and 2 steps; split into slices of 1-2 steps (K = 64 / 2: one step per slice, a single LDS buffer)
#   pf 2: 3 and 4-6 steps with ragged tails; split 160 / 2 -> kps 96: slices of 3 and 2 steps, 162 -> 3 + 3, 161 -> 3 + 3
KS = {
    (4, 1): (32, 64, (64, 2)), (2, 1): (2, 34, (66, 2)), (1, 1): (31, 33, (65, 2)),
    (4, 2): (96, 160, (160, 2)), (2, 2): (66, 162, (162, 2)), (1, 2): (97, 161, (161, 2)),
}
KS_ALT = {     # a second set, used by the layouts where K does not drive vw (so every K of the recipe list is met)
    (4, 1): (4, 64, (128, 3)), (2, 1): (34, 2, (98, 3)), (1, 1): (1, 33, (97, 3)),
    (4, 2): (128, 96, (160, 2)), (2, 2): (98, 66, (162, 2)), (1, 2): (65, 161, (193, 2)),
}


def _recipe(bn, arf, brf, vw):
    """((M, N), K mod 4 class, offa, offb) that gives vector width `vw` to layout (arf, brf) at tile width `bn`."""
    s = SHAPES[bn]
    s4 = s["s4"][arf ^ brf]
    if not arf and not brf:                         # both k-contiguous: K alone decides
        shape = {4: s4, 2: s["m2"] or s4, 1: s["n1"]}[vw]
        return shape, vw, 0, 0
    if arf and not brf:                             # A by its rows, B by K
        if vw == 4:
            return s4, 4, 0, 0
        if vw == 2:
            return (s["m2"], 4, 0, 0) if s["m2"] else (s4, 2, 0, 0)
        return s["m1"], 4, 0, 0
    if brf and not arf:                             # B by its rows, A by K
        if vw == 4:
            return s4, 4, 0, 0
        if vw == 2:
            return (s["n2"], 4, 0, 0) if s["n2"] else (s4, 4, 2, 0)      # A only 8-byte aligned
        return s["n1"], 4, 0, 0
    if vw == 4:                                     # both row-contiguous: K is free
        return s4, 4, 0, 0
    if vw == 2:
        return (s["m2"], 2, 0, 0) if s["m2"] else (s4, 1, 0, 2)          # B only 8-byte aligned
    return (s["n1"], 1, 0, 0) if bn != 64 else (s4, 4, 1, 0)             # bn 64: A only 4-byte aligned


def _leaf_cases():
    out = []
    i = 0
    for bn in (16, 32, 64):
        for arf in (0, 1):
            for brf in (0, 1):
                for vw in (4, 2, 1):
                    for pf in (1, 2):
                        (m, n), kc, offa, offb = _recipe(bn, arf, brf, vw)
                        ks = (KS_ALT if (arf and brf) or i % 2 else KS)[(kc, pf)]
                        leaf = (bn, vw, pf, arf, brf)
                        for j, kk in enumerate(ks):
                            k, split = kk if isinstance(kk, tuple) else (kk, 1)
                            i += 1
                            out.append(Case(f"f32-bn{bn}-vw{vw}-pf{pf}-a{arf}b{brf}-{j}", m, n, k, arf, brf, offa, offb,
                                            offc=i % 3, pad=(0, 1, 3, 4)[i % 4], split=split, bias=i % 2, act=(i // 2) % 2,
                                            bf16=0, leaf=leaf))
    return out


def _bf16_cases():
    out = []
    i = 0
    for bn in (16, 32, 64):
        for vw in (4, 2, 1):
            for arf, brf in ((0, 0), (1, 0), (0, 1), (1, 1)):
                (m, n), kc, offa, offb = _recipe(bn, arf, brf, vw)
                for pf in (1, 2):                    # (the bf16 kernel has no pf parameter: short and long K loops)
                    k, split = KS[(kc, pf)][1], 1
                    if arf == brf:
                        k, split = KS[(kc, pf)][2]
                    i += 1
                    out.append(Case(f"bf16-bn{bn}-vw{vw}-a{arf}b{brf}-pf{pf}", m, n, k, arf, brf, offa, offb, offc=i % 3,
                                    pad=(0, 1, 3, 4)[i % 4], split=split, bias=i % 2, act=(i // 2) % 2, bf16=1,
                                    leaf=(bn, vw)))
    return out


def _c(name, m, n, k, arf=0, brf=0, offa=0, offb=0, offc=0, pad=0, split=1, bias=0, act=0, bf16=0, leaf=None):
    return Case(name, m, n, k, arf, brf, offa, offb, offc, pad, split, bias, act, bf16, leaf)


# Named edges: name -> (case, {plan field: value}) — what the case is named for, asserted by the CPU test.
def _named():
    e = []
    # K = 193 three ways: kps = 96, the last slice is ONE element = one step inside a pf 2 kernel with two LDS buffers
    e.append((_c("k193-split3", 130, 7, 193, split=3, offc=1, pad=3, leaf=(16, 1, 2, 0, 0)),
              {"split_eff": 3, "kps": 96, "last_steps": 1, "sum_form": SUM_WALK}))
    e.append((_c("k193-split3-bf16", 130, 7, 193, split=3, pad=1, bias=1, bf16=1, leaf=(16, 1)),
              {"split_eff": 3, "kps": 96, "last_steps": 1, "sum_form": SUM_WALK}))
    # more than 32 slabs over few outputs: the block-per-output tree; with a bias the column walk over > 32 slabs
    e.append((_c("tree-34", 5, 7, 1088, split=34, leaf=(16, 4, 1, 0, 0)),
              {"split_eff": 34, "kps": 32, "last_steps": 1, "sum_form": SUM_TREE}))
    e.append((_c("walk-34-bias", 5, 7, 1088, split=34, bias=1, leaf=(16, 4, 1, 0, 0)),
              {"split_eff": 34, "kps": 32, "last_steps": 1, "sum_form": SUM_WALK}))
    e.append((_c("walk-34-ldc", 5, 7, 1088, split=34, pad=1, offc=2, leaf=(16, 4, 1, 0, 0)),
              {"split_eff": 34, "kps": 32, "sum_form": SUM_WALK}))
    e.append((_c("tree-34-bf16", 5, 7, 1088, split=34, bf16=1, leaf=(16, 4)),
              {"split_eff": 34, "kps": 32, "sum_form": SUM_TREE}))
    # a split clamped by K / 32
    e.append((_c("clamp-7-to-3", 66, 30, 96, split=7, act=1, bias=1, pad=4, leaf=(32, 4, 1, 0, 0)),
              {"split_eff": 3, "kps": 32, "last_steps": 1, "sum_form": SUM_WALK}))
    e.append((_c("clamp-3-to-1", 66, 30, 33, split=3, leaf=(32, 1, 1, 0, 0)),
              {"split_eff": 1, "kps": 64, "last_steps": 2, "sum_form": SUM_NONE}))
    # a ragged last slice: 98 / 3 -> kps 64, two slices of 64 and 34
    e.append((_c("ragged-98-3", 132, 12, 98, split=3, arf=1, brf=1, leaf=(16, 4, 1, 1, 1)),
              {"split_eff": 2, "kps": 64, "last_steps": 2, "sum_form": SUM_WALK}))
    # the parameter-gradient flag: the deferred / final row sum
    e.append((_c("final-2", 132, 16, 128, split=2, arf=1, brf=1, act=ACT_FINAL, leaf=(16, 4, 1, 1, 1)),
              {"split_eff": 2, "kps": 64, "sum_form": SUM_FINAL}))
    e.append((_c("final-2-ldc", 132, 16, 128, split=2, arf=1, brf=1, act=ACT_FINAL, pad=4, leaf=(16, 4, 1, 1, 1)),
              {"split_eff": 2, "sum_form": SUM_WALK}))
    e.append((_c("final-unsplit", 66, 30, 64, act=ACT_FINAL, bias=1, leaf=(32, 4, 1, 0, 0)),
              {"split_eff": 1, "sum_form": SUM_NONE}))
    # leave the slabs (away from LinearBN1d's one shape)
    e.append((_c("leave-3", 130, 17, 161, split=3, act=ACT_LEAVE, leaf=(32, 1, 1, 0, 0)),
              {"split_eff": 3, "kps": 64, "last_steps": 2, "sum_form": SUM_LEFT}))
    e.append((_c("leave-5", 63, 48, 160, split=5, arf=1, act=ACT_LEAVE, leaf=(16, 1, 1, 1, 0)),
              {"split_eff": 5, "kps": 32, "sum_form": SUM_LEFT}))
    e.append((_c("leave-1", 63, 48, 40, split=2, brf=1, act=ACT_LEAVE, leaf=(16, 4, 1, 0, 1)),
              {"split_eff": 1, "sum_form": SUM_NONE}))
    # degenerate strides: one row of a "row-contiguous" operand has sam == sak == 1 and is NOT row fast
    e.append((_c("m1-rowcontig-a", 1, 16, 64, arf=1, bias=1, leaf=(16, 1, 1, 0, 0)), {"arf": 0}))
    e.append((_c("n1-rowcontig-b", 132, 1, 64, brf=1, pad=3, leaf=(16, 1, 1, 0, 0)), {"brf": 0}))
    e.append((_c("one-by-one", 1, 1, 1, bias=1, act=1, offc=1, leaf=(16, 1, 1, 0, 0)), {"split_eff": 1}))
    e.append((_c("one-by-one-rr", 1, 1, 97, arf=1, brf=1, leaf=(16, 1, 2, 0, 0)), {"arf": 0, "brf": 0}))
    # K = 0: act(bias), no operand is read
    e.append((_c("k0-bias-relu", 130, 7, 0, bias=1, act=1, pad=1, offc=1, leaf=(16, 4, 1, 0, 0)),
              {"split_eff": 1, "kps": 32, "sum_form": SUM_NONE}))
    e.append((_c("k0-nobias", 66, 30, 0, split=3, leaf=(32, 4, 1, 0, 0)), {"split_eff": 1, "sum_form": SUM_NONE}))
    e.append((_c("k0-bf16", 130, 7, 0, bias=1, bf16=1, offc=2, pad=3, leaf=(16, 4)), {"split_eff": 1}))
    # pointer offsets as the projections pass them (w[d:], d * d odd): 4-byte aligned operands and output
    e.append((_c("odd-offsets", 132, 32, 64, offa=1, offb=1, offc=1, bias=1, leaf=(32, 1, 1, 0, 0)), {}))
    e.append((_c("odd-offset-c-only", 132, 32, 64, offc=1, leaf=(32, 4, 1, 0, 0)), {}))
    e.append((_c("8-byte-b", 132, 32, 128, offb=2, arf=1, offc=2, pad=4, leaf=(32, 2, 2, 1, 0)), {}))
    return e


NAMED = _named()
F32_LEAF_CASES = _leaf_cases()
BF16_LEAF_CASES = _bf16_cases()
CASES = F32_LEAF_CASES + BF16_LEAF_CASES + [c for c, _ in NAMED]

ALL_F32_LEAVES = {(bn, vw, pf, a, b) for bn in (16, 32, 64) for vw in (4, 2, 1) for pf in (1, 2) for a in (0, 1)
                  for b in (0, 1)}
ALL_BF16_LEAVES = {(bn, vw) for bn in (16, 32, 64) for vw in (4, 2, 1)}


def strides(c):
    """(sam, sak, sbn, sbk) of a case: k-contiguous storage [rows, K], row-contiguous storage [K, rows]."""
    sam, sak = (1, c.M) if c.arf else (c.K, 1)
    sbn, sbk = (1, c.N) if c.brf else (c.K, 1)
    return sam, sak, sbn, sbk


def ldc(c):
    return c.N + c.pad


def bn_of(c):
    return c.leaf[0]


# ---------------------------------------------------------------------------------------------------- grouped launches
# A member: (M, N, K, arf, brf, off (floats, all three pointers), bias, act, split_k).  A group: (name, bf16, members,
# (bn, vw, pf) it was built to reach or None for a fallback to single launches).
def _m(m, n, k, arf=0, brf=0, off=0, bias=0, act=0, split=1):
    return (m, n, k, arf, brf, off, bias, act, split)


_BIG = 32768
GROUPS = [
    ("bn16-vw4-pf1", 0, [_m(132, 16, 64), _m(132, 12, 32, 1, 1, bias=1, act=1)], (16, 4, 1)),
    # mixed: one member wants bn 32; 3 K steps next to exactly 1; all four layout pairs; two split members with different
    # output shapes (one shared column-walk launch) next to two unsplit ones
    ("bn16-vw4-pf2-mixed", 0, [_m(132, 32, 96), _m(132, 16, 32, 1, 0), _m(132, 12, 128, 0, 1, split=2),
                               _m(132, 16, 160, 1, 1, bias=1, act=1, split=2)], (16, 4, 2)),
    ("bn16-vw2-pf1", 0, [_m(130, 16, 64, 1, 1), _m(130, 7, 34)], (16, 2, 1)),
    # a split parameter gradient (0x100) next to a plainly split member and an unsplit one
    ("bn16-vw2-pf2-final", 0, [_m(130, 16, 98, 1, 0), _m(130, 7, 162, act=ACT_FINAL, split=2),
                               _m(132, 16, 66, 0, 1, split=2)], (16, 2, 2)),
    ("bn32-vw4-pf1", 0, [_m(132, 32, 64, bias=1), _m(132, 32, 32, 1, 1)], (32, 4, 1)),
    ("bn32-vw4-pf2", 0, [_m(132, 32, 128, 0, 1), _m(132, 32, 96, 1, 0), _m(132, 32, 32)], (32, 4, 2)),
    ("bn32-vw2-pf1", 0, [_m(66, 30, 64, 1, 1), _m(66, 30, 34), _m(132, 32, 64, off=2)], (32, 2, 1)),
    ("bn32-vw2-pf2", 0, [_m(66, 30, 98, split=3), _m(66, 30, 162, bias=1)], (32, 2, 2)),
    ("bn32-tree", 0, [_m(5, 32, 1088, split=34), _m(132, 32, 64)], (32, 4, 1)),
    ("bn64-vw4-pf1", 0, [_m(_BIG, 48, 32), _m(_BIG, 48, 32, 1, 1, bias=1, act=1)], (64, 4, 1)),
    ("bn64-vw4-pf2", 0, [_m(_BIG, 48, 32), _m(_BIG, 48, 96, 0, 1)], (64, 4, 2)),
    ("bn64-vw2-pf1", 0, [_m(_BIG, 48, 32, off=2), _m(_BIG, 48, 34)], (64, 2, 1)),
    ("bn64-vw2-pf2", 0, [_m(_BIG, 48, 98), _m(_BIG, 48, 32, 1, 0)], (64, 2, 2)),
    ("bf16-bn16-vw4", 1, [_m(132, 16, 64), _m(132, 12, 96, 1, 1, bias=1, act=1), _m(132, 16, 128, 0, 1, split=2)],
     (16, 4, 0)),
    ("bf16-bn16-vw2", 1, [_m(130, 16, 98, 1, 0), _m(130, 7, 162, split=2)], (16, 2, 0)),
    ("bf16-bn32-vw4", 1, [_m(132, 32, 64, bias=1), _m(132, 32, 32, 1, 1)], (32, 4, 0)),
    ("bf16-bn32-vw2", 1, [_m(66, 30, 64, 1, 1), _m(66, 30, 34)], (32, 2, 0)),
    ("bf16-bn64-vw4", 1, [_m(_BIG, 48, 32), _m(_BIG, 48, 32, 0, 1)], (64, 4, 0)),
    ("bf16-bn64-vw2", 1, [_m(_BIG, 48, 34), _m(_BIG, 48, 32, 1, 1)], (64, 2, 0)),
    # not groupable: a single member; a member that only allows scalar loads
    ("single", 0, [_m(132, 16, 64, bias=1)], None),
    ("vw1-member", 0, [_m(130, 7, 33, bias=1, act=1), _m(132, 16, 128, split=2)], None),
    ("vw1-member-bf16", 1, [_m(132, 16, 64, off=1), _m(132, 16, 64)], None),
]

ALL_F32_GROUP_LEAVES = {(bn, vw, pf) for bn in (16, 32, 64) for vw in (4, 2) for pf in (1, 2)}
ALL_BF16_GROUP_LEAVES = {(bn, vw, 0) for bn in (16, 32, 64) for vw in (4, 2)}


def member_strides(mem):
    m, n, k, arf, brf = mem[:5]
    sam, sak = (1, m) if arf else (k, 1)
    sbn, sbk = (1, n) if brf else (k, 1)
    return sam, sak, sbn, sbk


def group_table(members, bf16, addr):
    """The [n][16] int64 table of igcn_gemm_f32_grouped.  addr(i, what, floats) -> address of member i's buffer `what`
    ('a', 'b', 'bias', 'c', 'scratch') of at least `floats` floats, 16-byte aligned; the member's offset is added here."""
    t = []
    for i, mem in enumerate(members):
        m, n, k, arf, brf, off, bias, act, split = mem
        sam, sak, sbn, sbk = member_strides(mem)
        t += [m, n, k, addr(i, "a", m * k + off) + 4 * off, sam, sak, addr(i, "b", n * k + off) + 4 * off, sbn, sbk,
              (addr(i, "bias", n + off) + 4 * off) if bias else 0, addr(i, "c", m * n + off) + 4 * off, n, act, split,
              addr(i, "scratch", max(1, split) * m * n) if split > 1 else 0, bf16]
    return t
