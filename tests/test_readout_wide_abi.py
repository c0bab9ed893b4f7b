"""igcn_node_linear_bn_supported (csrc/readout.hip): which (inputs per node F, outputs per node D) the GO read-out
kernels accept — the widths they had, and every multiple of 16 from 64 to 160 (dim_snps_atten of the reference's hidden-32
sweep, and of 4 / 5 layers at hidden 16) — and that the backward's scratch size at the benchmark's read-out did not move.
Loads the library and calls host-side functions only: nothing is launched."""
import pytest

WIDE = (64, 80, 96, 112, 128, 144, 160)
# RO_DISPATCH before the wide kernels
BEFORE = [(5, d) for d in (32, 48, 30, 20, 16, 12, 24, 10, 8, 6, 4, 3, 2, 5, 1)] + [(2, 1)]


@pytest.fixture(scope="module")
def lib():
    from igcn_amd import _lib
    return _lib.load()          # raises if libigcn.so is missing: no fallback


@pytest.mark.parametrize("d", WIDE)
def test_wide_readouts_are_accepted(lib, d):
    assert int(lib.igcn_node_linear_bn_supported(5, d)) == 1


@pytest.mark.parametrize("f,d", BEFORE)
def test_widths_covered_before_are_accepted(lib, f, d):
    assert int(lib.igcn_node_linear_bn_supported(f, d)) == 1


@pytest.mark.parametrize("f,d", [(5, 7), (5, 176), (3, 96)])
def test_other_shapes_are_refused(lib, f, d):
    assert int(lib.igcn_node_linear_bn_supported(f, d)) == 0


def test_ops_answers_what_the_library_answers():
    from igcn_amd import ops
    assert ops.node_linear_bn_supported(5, 96) and ops.node_linear_bn_supported(2, 1)
    assert not ops.node_linear_bn_supported(5, 176) and not ops.node_linear_bn_supported(3, 96)


def test_backward_scratch_of_the_benchmark_readout_is_unchanged(lib):
    """B = 512 (two passes of 256), N = 400, D = 32: stats 2*32*2*400 + 2*2*400, the dpre rows 512*400*32 and the GEMM
    slabs 16*512*32*5 the sizing function has always reserved there, + 68 (measured on the library built from the commit
    before the wide kernels: 7 917 188)."""
    assert int(lib.igcn_node_linear_bn_bwd_scratch_floats(512, 5, 400, 32, 2)) == 7917188


@pytest.mark.parametrize("d", WIDE[1:])
def test_backward_scratch_of_a_wide_readout_is_what_its_kernels_use(lib, d):
    """Chunk partials [32][2][2][400] + group sums [2][2][400], then one [D, 5] weight-gradient row per workgroup of 8
    nodes and (at most) 8 chunks per group, + 68 floats of alignment room."""
    want = 32 * 2 * 2 * 400 + 2 * 2 * 400 + 50 * 2 * 8 * d * 5 + 68
    assert int(lib.igcn_node_linear_bn_bwd_scratch_floats(512, 5, 400, d, 2)) == want
