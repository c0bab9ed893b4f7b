"""CPU checks of the one-owner rule: igcn_amd/_lib.py derives its ctypes table, the ABI revision and the kernel limits
from include/igcn.h, and every limit Python hands out under a public name is the header's macro.  The parser is run on
synthetic header text; the values expected of the real header are restated here (the independent side)."""
import ctypes
import os

import pytest

from igcn_amd import _lib, ops, snps

I, L, Z, F, D, U, P = (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float, ctypes.c_double, ctypes.c_uint,
                       ctypes.c_void_p)

SYNTHETIC = """
/* int igcn_in_a_block_comment(int a); */
// int igcn_in_a_line_comment(int a);
#define IGCN_ABI_VERSION 7
#define IGCN_NEGATIVE (-3)
#define IGCN_BARE_NEGATIVE -4
#define IGCN_SHIFTED (1 << 20)
#define IGCN_FLAG 8u
#define OTHER_PREFIX 5
#  define IGCN_INDENTED 12   /* trailing comment */
int igcn_version(void);
int igcn_empty();
const char* igcn_last_error(void);
const char *igcn_spaced_star(void);
size_t igcn_three_lines(int64_t n_nodes,   // first
                        const float* x /*[N, F]*/, size_t bytes,
                        unsigned options, double t, float eps);
int igcn_parts(int n, const float* const* parts /*HOST array*/, void* stream);
int igcn_unnamed(int, const int k, float);
"""


def test_parser_on_synthetic_header_text():
    sig, lim = _lib.parse_header(SYNTHETIC)
    assert set(sig) == {"igcn_version", "igcn_empty", "igcn_last_error", "igcn_spaced_star", "igcn_three_lines",
                        "igcn_parts", "igcn_unnamed"}
    assert sig["igcn_version"] == (I, []) and sig["igcn_empty"] == (I, [])
    assert sig["igcn_last_error"] == (ctypes.c_char_p, []) and sig["igcn_spaced_star"] == (ctypes.c_char_p, [])
    assert sig["igcn_three_lines"] == (Z, [L, P, Z, U, D, F])
    assert sig["igcn_parts"] == (I, [I, P, P]) and sig["igcn_unnamed"] == (I, [I, I, F])
    # plain decimal literals only, optionally negative or parenthesised: an expression or a suffixed literal is no limit
    assert lim == {"IGCN_ABI_VERSION": 7, "IGCN_NEGATIVE": -3, "IGCN_BARE_NEGATIVE": -4, "IGCN_INDENTED": 12}


@pytest.mark.parametrize("arg", ["long n", "uint8_t flag", "hipStream_t stream", "int32_t k", "short", "unsigned long n",
                                 "unsigned long long seed", "unsigned char c", "unsigned int n", "float x[4]",
                                 "const float x[]", "int a b"])
def test_unknown_scalar_type_raises_naming_the_prototype(arg):
    with pytest.raises(_lib.IgcnError) as e:
        _lib.parse_header(f"int igcn_ok(int a);\nint igcn_bad_one(int a, {arg}, float b);\n")
    assert "igcn_bad_one" in str(e.value) and arg in str(e.value)


@pytest.mark.parametrize("text", [
    "int64_t igcn_bad_one(int a);",                         # a return type the binding does not map
    "void igcn_bad_one(int a);",
    "static inline int igcn_bad_one(int a);",
    "int igcn_bad_one(int a) { return a; }",                # a definition
    "int igcn_bad_one(void (*callback)(int), int a);",      # an argument list the parser cannot split
])
def test_a_declaration_that_cannot_be_bound_raises_naming_it(text):
    with pytest.raises(_lib.IgcnError) as e:
        _lib.parse_header("int igcn_ok(int a);\n" + text + "\nint igcn_after(void);\n")
    assert "igcn_bad_one" in str(e.value) and "igcn_ok" not in str(e.value)


def test_missing_header_raises_naming_the_path(tmp_path):
    path = str(tmp_path / "include" / "igcn.h")
    with pytest.raises(_lib.IgcnError) as e:
        _lib.read_header(path)
    assert path in str(e.value)


def test_header_is_found_beside_the_package():
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "..", "include",
                                                           "igcn.h"))
    sig, lim = _lib.read_header()
    assert sig == _lib.SIGNATURES and lim == _lib.LIMITS


# the value of every limit the kernels and Python share, as the header must state it
EXPECTED = {
    "IGCN_COPY_MULTI_MAX": 16,
    "IGCN_LDS_BUDGET_BYTES": 150 * 1024, "IGCN_LDS_MAX_BYTES": 160 * 1024,
    "IGCN_MAX_H0": 8, "IGCN_STACK_MAX_LAYERS": 4, "IGCN_STACK_MIN_WIDTH": 4, "IGCN_STACK_MAX_WIDTH": 32,
    "IGCN_SEG_MAX_NODES": 1024, "IGCN_SEG_MAX_EDGES": 4096,
    "IGCN_SALIENCY_MAX_ROIS": 512, "IGCN_SALIENCY_MAX_ELEMS": 8192, "IGCN_SALIENCY_MAX_STEPS": 4096,
    "IGCN_GRAD_CAM_MAX_WIDTH": 160,
    "IGCN_EVAL_MAX_ROWS": 65536,
    "IGCN_TSNE_MIN_S": 4, "IGCN_TSNE_MAX_S": 4096, "IGCN_TSNE_MAX_D": 1024,
    "IGCN_KMEANS_MAX_N": 65536, "IGCN_KMEANS_MAX_D": 1024, "IGCN_KMEANS_MAX_K": 16, "IGCN_KMEANSPP_MAX_TRIALS": 8,
    "IGCN_PERM_MIN_S": 4, "IGCN_PERM_MAX_S": 4096, "IGCN_PERM_MAX_E": 1 << 20, "IGCN_PERM_MAX_P": 65536,
    "IGCN_PERM_MAX_G_ROWS": 8,
}


def test_limits_hold_the_abi_revision_and_every_shared_limit():
    assert _lib.LIMITS["IGCN_ABI_VERSION"] == _lib.ABI_VERSION == 441
    for name, value in EXPECTED.items():
        assert _lib.LIMITS[name] == value, name
    assert (_lib.LIMITS["IGCN_OK"], _lib.LIMITS["IGCN_ERR_BADARG"], _lib.LIMITS["IGCN_ERR_UNSUPPORTED"]) == (0, -1, -3)


PUBLIC = {
    "IGCN_LDS_BUDGET_BYTES": [(ops, "LDS_BUDGET_BYTES"), (ops, "GAT_LDS_BYTES")],
    "IGCN_MAX_H0": [(ops, "MAX_H0"), (ops, "GAT_MAX_H0")],
    "IGCN_STACK_MAX_LAYERS": [(ops, "STACK_MAX_LAYERS"), (ops, "GAT_MAX_LAYERS")],
    "IGCN_STACK_MAX_WIDTH": [(ops, "STACK_MAX_WIDTH")],
    "IGCN_SEG_MAX_NODES": [(ops.GraphPlan, "SEG_MAX_NODES")], "IGCN_SEG_MAX_EDGES": [(ops.GraphPlan, "SEG_MAX_EDGES")],
    "IGCN_SALIENCY_MAX_ROIS": [(ops, "SALIENCY_MAX_ROIS")], "IGCN_SALIENCY_MAX_ELEMS": [(ops, "SALIENCY_MAX_ELEMS")],
    "IGCN_SALIENCY_MAX_STEPS": [(ops, "SALIENCY_MAX_STEPS")], "IGCN_GRAD_CAM_MAX_WIDTH": [(ops, "GRAD_CAM_MAX_WIDTH")],
    "IGCN_EVAL_MAX_ROWS": [(snps, "EVAL_MAX_ROWS")],
    "IGCN_TSNE_MIN_S": [(ops, "TSNE_MIN_S")], "IGCN_TSNE_MAX_S": [(ops, "TSNE_MAX_S")],
    "IGCN_TSNE_MAX_D": [(ops, "TSNE_MAX_D")],
    "IGCN_KMEANS_MAX_N": [(ops, "KMEANS_MAX_N")], "IGCN_KMEANS_MAX_D": [(ops, "KMEANS_MAX_D")],
    "IGCN_KMEANS_MAX_K": [(ops, "KMEANS_MAX_K")], "IGCN_KMEANSPP_MAX_TRIALS": [(ops, "KMEANSPP_MAX_TRIALS")],
    "IGCN_PERM_MIN_S": [(ops, "PERM_MIN_S")], "IGCN_PERM_MAX_S": [(ops, "PERM_MAX_S")],
    "IGCN_PERM_MAX_E": [(ops, "PERM_MAX_E")], "IGCN_PERM_MAX_P": [(ops, "PERM_MAX_P")],
    "IGCN_PERM_MAX_G_ROWS": [(ops, "PERM_MAX_G_ROWS")],
}


def test_every_public_python_name_equals_its_macro():
    for macro, names in PUBLIC.items():
        for owner, name in names:
            assert getattr(owner, name) == _lib.LIMITS[macro] == EXPECTED[macro], (macro, name)
    assert ops.GAT_WIDTHS == ops.STACK_WIDTHS == (4, 8, 16, 32)
    assert set(PUBLIC) | {"IGCN_COPY_MULTI_MAX", "IGCN_LDS_MAX_BYTES", "IGCN_STACK_MIN_WIDTH"} == set(EXPECTED)


def test_abi_version_equals_the_built_library():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert int(_lib.load().igcn_version()) == _lib.ABI_VERSION
