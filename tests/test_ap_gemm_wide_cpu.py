"""CPU: the prefill GEMM entry points accept 5 to 8 bits (csrc/ap_gemm_wide.hip behind gq_anyprec_gemm / gq_anyprec_gemm_ws): the
width is admitted before the pointers are looked at, the other refusals are those of the 2..4-bit path, and no K split is planned."""
import pytest

torch = pytest.importorskip("torch")


def _gemm(S, N, K, bits):
    from guidedquant_amd import _lib
    return _lib.lib().gq_anyprec_gemm(None, None, None, None, S, N, K, bits, None)


@pytest.mark.parametrize("bits", [5, 6, 7, 8])
def test_wide_bits_are_admitted_and_null_pointers_refused(bits):
    from guidedquant_amd import _lib
    assert _gemm(16, 128, 1024, bits) == _lib.GQ_EINVAL


@pytest.mark.parametrize("bits", [1, 9])
def test_bits_outside_2_to_8_are_not_supported(bits):
    from guidedquant_amd import _lib
    assert _gemm(16, 128, 1024, bits) == _lib.GQ_ENOTSUP


def test_k_must_be_a_multiple_of_64_at_wide_bits_too():
    from guidedquant_amd import _lib
    assert _gemm(16, 128, 96, 6) == _lib.GQ_ENOTSUP


@pytest.mark.parametrize("bits", [1, 5, 6, 7, 8, 9])
def test_no_workspace_is_asked_for_outside_2_to_4_bits(bits):
    """5..8 bits are served in a single pass (one tile shape, no split K); other widths are not served at all"""
    from guidedquant_amd import _lib
    for S, N, K in [(128, 4096, 4096), (100, 4096, 14336), (512, 6144, 4096)]:
        assert _lib.lib().gq_anyprec_gemm_ws_bytes(S, N, K, bits) == 0
