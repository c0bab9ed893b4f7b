"""igcn_attn_core_lds_bytes at head_dim 33..96 (csrc/attn_core.hip, csrc/attn_mfma.hip): which shapes the exact-fp32
attention core accepts, which of its two forms (LDS-resident, streamed) a shape takes, and that the sizes of the widths
it already covered did not move.  Loads the library and calls its host-side sizing function only: nothing is launched."""
import pytest

CHUNKED = 96 * 1024          # what igcn_attn_core_lds_bytes reports for the streamed form


@pytest.fixture(scope="module")
def lds_bytes():
    from igcn_amd import _lib
    lib = _lib.load()          # raises if libigcn.so is missing: no fallback
    return lambda *a: int(lib.igcn_attn_core_lds_bytes(*a))


@pytest.mark.parametrize("d", [66, 80, 96, 128, 160, 192])
@pytest.mark.parametrize("backward", [0, 1])
def test_wide_heads_are_accepted(lds_bytes, d, backward):
    """head_dim 33, 40, 48, 64, 80, 96 at two heads."""
    assert lds_bytes(d, 2, 40, 70, backward) != 0


@pytest.mark.parametrize("d", [194, 256])
@pytest.mark.parametrize("backward", [0, 1])
def test_heads_above_96_are_refused(lds_bytes, d, backward):
    """head_dim 97 and 128."""
    assert lds_bytes(d, 2, 40, 70, backward) == 0


def test_form_follows_the_size(lds_bytes):
    """head_dim 48: 40 x 70 keeps K, V, Q, dO of a head in LDS (49-float rows: 2 * 80 * 49 floats forward, + 2 * 48 * 49
    + 2 * 48 + 4 backward); 130 x 400 would need 214 KB and is streamed."""
    fwd, bwd = lds_bytes(96, 2, 40, 70, 0), lds_bytes(96, 2, 40, 70, 1)
    assert fwd == 2 * 80 * 49 * 4 and bwd == (2 * 80 * 49 + 2 * 48 * 49 + 2 * 48 + 4) * 4
    for v in (fwd, bwd):
        assert 0 < v <= 150 * 1024 and v != CHUNKED
    assert lds_bytes(96, 2, 130, 400, 0) == CHUNKED and lds_bytes(96, 2, 130, 400, 1) == CHUNKED


def test_padded_width_above_32_is_the_next_multiple_of_16(lds_bytes):
    """The size reported is the size launched: head_dim 33 and 40 share the 48-column kernels' 49-float rows, 80 has
    81-float rows (not 84 or 96)."""
    assert lds_bytes(66, 2, 40, 70, 1) == lds_bytes(80, 2, 40, 70, 1) == lds_bytes(96, 2, 40, 70, 1)
    assert lds_bytes(160, 2, 40, 70, 0) == 2 * 80 * 81 * 4


def test_sizes_of_the_widths_covered_before_are_unchanged(lds_bytes):
    """head_dim 16 (forward: unpadded 16-float rows), and head_dim 10 padded to 12 (13-float rows)."""
    assert lds_bytes(32, 2, 90, 400, 0) == 51200
    assert lds_bytes(32, 2, 90, 400, 1) == 68240
    assert lds_bytes(20, 2, 90, 400, 0) == 41600
    assert lds_bytes(20, 2, 90, 400, 1) == 52368
