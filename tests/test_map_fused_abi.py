"""Host side of the read-out + gene-decoding fusion (no GPU): igcn_node_linear_bn_apply_map_ok at the workload's shapes
and under the library option bit, and the new entry points in the header and the binding."""
import os
import re

from conftest import ROOT
from igcn_amd import _lib, switches

HEADER = os.path.join(ROOT, "include", "igcn.h")
NEW = ("igcn_node_linear_bn_apply_map_ok", "igcn_node_linear_bn_apply_map_fwd")


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_new_entry_points_are_declared_and_bound():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    lib = _lib_loaded()
    for name in NEW:
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", src)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name


def test_option_bit_is_the_next_one():
    names = [n for n, _ in switches.LIBRARY]
    assert names[-1] == "IGCN_NO_MAP_FUSED" and switches.library_mask({"IGCN_NO_MAP_FUSED": "1"}) == 256


def test_query_at_the_workload_shapes_and_under_the_option_bit():
    """The D = 1 read-out joins the decoding at (3000 nodes, 54 SNPs) and at the 10 000-node stress DAG (40 KB of LDS);
    a row beyond 64 KB, other read-out shapes and a map with short rows (igcn_spmm_fwd takes the tiled kernel there, in
    another order): 0.  Option bit 8 (IGCN_NO_MAP_FUSED) and the untiled CSR kernels: 0."""
    lib = _lib_loaded()
    ro = lib.igcn_node_linear_bn_apply_map_ok
    restore = (switches.library_mask(), switches.knob("IGCN_GEMM_BN"), switches.knob("IGCN_ATTN_CHUNK"))
    try:
        lib.igcn_configure(0, 0, 0)
        assert ro(2, 1, 3000, 54, 8000) == 1 and ro(2, 1, 10000, 54, 27000) == 1
        assert ro(2, 1, 20000, 54, 50000) == 0           # 80 KB: the row does not fit
        assert ro(5, 1, 3000, 54, 8000) == 0 and ro(2, 5, 3000, 54, 8000) == 0
        assert ro(2, 1, 3000, 54, 8 * 54) == 0
        for mask in (256, 4):
            lib.igcn_configure(mask, 0, 0)
            assert ro(2, 1, 3000, 54, 8000) == 0 and ro(2, 1, 10000, 54, 27000) == 0
    finally:
        lib.igcn_configure(*restore)
