"""CPU checks of the GEMM launch plan (csrc/gemm.hip gemm_plan, queried through igcn_gemm_plan / igcn_gemm_group_plan):
the shared case table (tests/gemm_cases.py) reaches EVERY template instantiation of the four product kernels and every
slab-sum form, each case lands on the leaf it was built for, and the named edge cases have the plan they are named for.
Coverage is a condition: a change of the launch heuristics that makes a leaf unreachable from the table fails here, and
the table gets a new shape.  No GPU, no compute calls."""
import ctypes
import os

import pytest

import gemm_cases as gc
from igcn_amd import _lib

BASE = 4096                                                   # a synthetic 16-byte-aligned address; never dereferenced


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def plan_of(lib, c, a_addr=None, b_addr=None):
    sam, sak, sbn, sbk = gc.strides(c)
    out = (ctypes.c_int64 * 8)()
    rc = lib.igcn_gemm_plan(c.bf16, c.M, c.N, c.K, BASE + 4 * c.offa if a_addr is None else a_addr, sam, sak,
                            (2 * BASE) + 4 * c.offb if b_addr is None else b_addr, sbn, sbk, gc.ldc(c), c.bias, c.act,
                            c.split, out)
    assert rc == 0, (c.name, lib.igcn_last_error())
    return dict(zip(("bn", "vw", "pf", "arf", "brf", "split_eff", "kps", "sum_form"), (int(v) for v in out)))


def leaf_of(p, bf16):
    return (p["bn"], p["vw"]) if bf16 else (p["bn"], p["vw"], p["pf"], p["arf"], p["brf"])


def test_table_is_small_and_names_are_unique():
    names = [c.name for c in gc.CASES]
    assert len(set(names)) == len(names)
    # one case per (f32 leaf x {few steps, more steps, split}) + the bf16 leaves + the named edges: not a cross product
    assert len(gc.F32_LEAF_CASES) == 72 * 3 and len(gc.CASES) < 400, len(gc.CASES)
    for c in gc.CASES:
        assert c.offa in (0, 1, 2) and c.offb in (0, 1, 2) and c.offc in (0, 1, 2) and c.pad in (0, 1, 3, 4), c.name


def test_every_case_runs_the_leaf_it_was_built_for(lib):
    for c in gc.CASES:
        p = plan_of(lib, c)
        assert leaf_of(p, c.bf16) == c.leaf, (c.name, p)


def test_table_reaches_all_72_f32_and_9_bf16_leaves(lib):
    f32 = {leaf_of(plan_of(lib, c), 0) for c in gc.CASES if not c.bf16}
    assert f32 == gc.ALL_F32_LEAVES and len(f32) == 72, sorted(gc.ALL_F32_LEAVES ^ f32)
    bf16 = {leaf_of(plan_of(lib, c), 1) for c in gc.CASES if c.bf16}
    assert bf16 == gc.ALL_BF16_LEAVES and len(bf16) == 9, sorted(gc.ALL_BF16_LEAVES ^ bf16)
    # per f32 leaf: one and two (pf 1) or three and more (pf 2) K steps unsplit, and a split product
    for leaf in gc.ALL_F32_LEAVES:
        mine = [(c, plan_of(lib, c)) for c in gc.F32_LEAF_CASES if c.leaf == leaf]
        steps = {-(-c.K // 32) for c, p in mine if p["split_eff"] == 1}
        assert len(steps) == 2 and (max(steps) <= 2 if leaf[2] == 1 else min(steps) >= 3), (leaf, steps)
        assert any(p["split_eff"] > 1 for _, p in mine), leaf


def test_every_slab_sum_form_occurs(lib):
    forms = {plan_of(lib, c)["sum_form"] for c in gc.CASES}
    assert forms == {gc.SUM_NONE, gc.SUM_WALK, gc.SUM_TREE, gc.SUM_FINAL, gc.SUM_LEFT}, forms
    for bf16 in (0, 1):
        assert {gc.SUM_WALK, gc.SUM_TREE} <= {plan_of(lib, c)["sum_form"] for c in gc.CASES if c.bf16 == bf16}


def test_named_edges_have_the_plan_they_are_named_for(lib):
    for c, want in gc.NAMED:
        p = plan_of(lib, c)
        last = c.K - (p["split_eff"] - 1) * p["kps"]
        p["last_steps"] = -(-last // 32)
        for key, v in want.items():
            assert p[key] == v, (c.name, key, p)
        assert 0 <= last <= p["kps"] and (c.K == 0 or last > 0), (c.name, p)     # the last slice is never empty


def test_split_helpers_agree_with_the_plan(lib):
    for c in gc.CASES:
        p = plan_of(lib, c)
        assert lib.igcn_gemm_effective_split(c.K, c.split) == p["split_eff"], c.name
        assert p["kps"] % 32 == 0 and p["kps"] * (p["split_eff"] - 1) < max(c.K, 1) <= p["kps"] * p["split_eff"], c.name
        # the split the library prefers, passed back as callers do: honoured as it is (it never exceeds K / 32), with
        # the tile width igcn_gemm_f32_split_k counted its tiles with
        pref = lib.igcn_gemm_f32_split_k(c.M, c.N, c.K)
        q = plan_of(lib, c._replace(split=pref, act=c.act & 0xff))
        assert q["split_eff"] == lib.igcn_gemm_effective_split(c.K, pref) and q["bn"] == p["bn"], c.name
        assert pref == 1 or (c.K >= 128 and q["split_eff"] <= pref <= c.K // 32), (c.name, pref)


def test_plan_reads_only_the_low_address_bits(lib):
    """The same plan at another (never mapped) base address with the same low bits; a 4-byte offset narrows the loads."""
    for c in gc.CASES[::7]:
        assert plan_of(lib, c) == plan_of(lib, c, a_addr=(1 << 40) + 4 * c.offa, b_addr=(3 << 40) + 4 * c.offb), c.name
    c = gc.CASES[0]._replace(M=132, N=32, K=64, arf=0, brf=0, offa=0, offb=0, split=1)
    assert [plan_of(lib, c._replace(offa=o))["vw"] for o in (0, 1, 2)] == [4, 1, 2]
    assert [plan_of(lib, c._replace(offb=o))["vw"] for o in (0, 1, 2)] == [4, 1, 2]


def test_plan_refuses_what_the_launch_refuses(lib):
    out = (ctypes.c_int64 * 8)()
    for m, n, k, split in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, -1, 1), (4, 4, 4, 0)):
        assert lib.igcn_gemm_plan(0, m, n, k, BASE, k, 1, BASE, k, 1, n, 0, 0, split, out) != 0
    assert lib.igcn_gemm_plan(0, 4, 4, 4, BASE, 4, 1, BASE, 4, 1, 4, 0, 0, 1, None) != 0


def group_plan(lib, members, bf16):
    table = gc.group_table(members, bf16, lambda i, what, floats: BASE * (1 + 8 * i + "a b bias c scratch".split().index(what)))
    arr = (ctypes.c_int64 * len(table))(*table)
    out = (ctypes.c_int64 * 4)()
    rc = lib.igcn_gemm_group_plan(len(members), arr, out)
    return rc, tuple(int(v) for v in out)


def test_grouped_table_reaches_all_12_and_6_leaves_and_the_fallbacks(lib):
    f32, bf16, fallbacks = set(), set(), 0
    for name, is_bf16, members, want in gc.GROUPS:
        rc, (bn, vw, pf, grouped) = group_plan(lib, members, is_bf16)
        assert rc == 0, name
        if want is None:
            assert grouped == 0, name
            fallbacks += 1
            continue
        assert grouped == 1 and (bn, vw, pf) == want, (name, bn, vw, pf)
        (bf16 if is_bf16 else f32).add((bn, vw, pf))
    assert f32 == gc.ALL_F32_GROUP_LEAVES and len(f32) == 12
    assert bf16 == gc.ALL_BF16_GROUP_LEAVES and len(bf16) == 6
    assert fallbacks >= 2
    assert any(len(m) == 1 for _, _, m, w in gc.GROUPS if w is None)             # n == 1
    assert any(len(m) > 1 for _, _, m, w in gc.GROUPS if w is None)              # a member with scalar loads only


def test_group_members_differ_as_the_mixed_groups_promise(lib):
    """The mixed groups: members whose OWN plans differ in tile width, K steps, layouts and slab sums."""
    def own(mem):
        m, n, k, arf, brf, off, bias, act, split = mem
        c = gc.Case("member", m, n, k, arf, brf, off, off, off, 0, split, bias, act, 0, None)
        return plan_of(lib, c)
    mixed = dict((g[0], g[2]) for g in gc.GROUPS)["bn16-vw4-pf2-mixed"]
    plans = [own(m) for m in mixed]
    assert {p["bn"] for p in plans} == {16, 32} and {p["pf"] for p in plans} == {1, 2}
    assert {(p["arf"], p["brf"]) for p in plans} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(-(-m[2] // 32) == 1 for m in mixed) and any(p["pf"] == 2 for p in plans)
    walks = [m for m, p in zip(mixed, plans) if p["sum_form"] == gc.SUM_WALK]
    assert len(walks) == 2 and len({(m[0], m[1]) for m in walks}) == 2          # one shared sum, two output shapes
    assert sum(p["split_eff"] == 1 for p in plans) == 2
    final = dict((g[0], g[2]) for g in gc.GROUPS)["bn16-vw2-pf2-final"]
    assert sorted(own(m)["sum_form"] for m in final) == [gc.SUM_NONE, gc.SUM_WALK, gc.SUM_FINAL]
    tree = dict((g[0], g[2]) for g in gc.GROUPS)["bn32-tree"]
    assert own(tree[0])["sum_form"] == gc.SUM_TREE


def test_group_plan_refuses_bad_tables(lib):
    ok = [gc._m(132, 16, 64)] * 5
    assert group_plan(lib, ok, 0)[0] != 0                                         # n = 5
    assert group_plan(lib, [gc._m(132, 16, 64), gc._m(132, 16, 0)], 0)[0] != 0    # K = 0 in a member
    assert group_plan(lib, ok[:2], 0)[0] == 0
