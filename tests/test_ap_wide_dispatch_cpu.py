"""CPU (host logic): the dry AP-GEMV dispatch (gq_debug_ap_plan_route, gq_anyprec_handover_plan) at 5 to 8 bits.  The decode step's
launch forms of Llama 8B and 70B go to ap_wide.hip's kernel in both modes, with no workspace and no statistics hand-over; what that
kernel does not serve (K % 128 != 0, M > 1, GQ_AP_FORCE_GENERIC=1) stays on the generic kernel, whose fused forms are refused."""
import ctypes
import os

import pytest

from guidedquant_amd import _lib

EPI_RESIDUAL, PRO_SILU_MUL, EPI_SILU_PAIRS = 1, 2, 4
SHAPES = {"8B": {"wqkv": (6144, 4096), "wo": (4096, 4096), "w1w3": (28672, 4096), "w2": (4096, 14336)},
          "70B": {"wqkv": (10240, 8192), "wo": (8192, 8192), "w1w3": (57344, 8192), "w2": (8192, 28672)}}
# the decode step's launch forms (model.py): (matrix, RMSNorm prologue, epilogue flags); w2 with GQ_NATIVE_PAIRS=0 takes the SiLU * up prologue
FORMS = [("wqkv", True, 0), ("wo", False, EPI_RESIDUAL), ("w1w3", True, EPI_SILU_PAIRS), ("w2", False, EPI_RESIDUAL),
         ("w2", False, PRO_SILU_MUL | EPI_RESIDUAL)]
DECODE = [(model, bits, name, *SHAPES[model][name], norm, epi) for model in SHAPES for bits in (5, 6, 7, 8) for name, norm, epi in FORMS]


def _id(row):
    model, bits, name, N, K, norm, epi = row
    return f"{model}-{bits}b-{name}-{'n' if norm else ''}{epi}"


@pytest.fixture(params=[0, 1], ids=["default", "exact"])
def L(request):
    L = _lib.lib()
    os.environ.pop("GQ_AP_FORCE_GENERIC", None)
    L.gq_reset_env_cache()
    L.gq_set_ap_mode(request.param)
    yield L
    L.gq_set_ap_mode(-1)
    os.environ.pop("GQ_AP_FORCE_GENERIC", None)
    L.gq_reset_env_cache()


@pytest.mark.parametrize("row", DECODE, ids=_id)
def test_decode_forms_plan_the_wide_kernel(L, row):
    _, bits, _, N, K, norm, epi = row
    assert _lib.ap_plan_route(N, K, bits, 1, norm, epi) == ("wide", 1, 0)
    assert L.gq_anyprec_gemv_fused_ws_bytes(N, K, bits, epi) == 0
    assert L.gq_anyprec_handover_plan(N, K, bits, 1 if norm else 0, epi) == 0
    # a workspace handed in anyway changes nothing
    assert _lib.ap_plan_route(N, K, bits, 1, norm, epi, 1 << 20)[0] == "wide"


@pytest.mark.parametrize("bits", [5, 6, 7, 8])
@pytest.mark.parametrize("K", [128, 1152, 4608, 11008, 32768])
def test_other_whole_quad_rows_plan_the_wide_kernel(L, bits, K):
    for N in (1, 2, 1000, 4097):
        assert _lib.ap_plan_route(N, K, bits)[0] == "wide"
        assert _lib.ap_plan_route(N, K, bits, 1, True, EPI_RESIDUAL)[0] == "wide"
    assert _lib.ap_plan_route(1000, K, bits, 1, False, EPI_SILU_PAIRS)[0] == "wide"


@pytest.mark.parametrize("bits", [5, 6, 7, 8])
def test_what_the_wide_kernel_does_not_serve_stays_generic(L, bits):
    for K in (96, 4128, 14368, 32768 + 128):
        assert _lib.ap_plan_route(4096, K, bits) == ("generic", 1, 0)
        # the generic kernel has no fused forms
        with pytest.raises(RuntimeError):
            _lib.ap_plan_route(4096, K, bits, 1, True, 0)
    for M in (2, 8):
        assert _lib.ap_plan_route(4096, 4096, bits, M) == ("generic", 1, 0)


@pytest.mark.parametrize("bits", [5, 6, 7, 8])
def test_force_generic_still_forces_the_generic_kernel(L, bits):
    os.environ["GQ_AP_FORCE_GENERIC"] = "1"
    L.gq_reset_env_cache()
    assert _lib.ap_plan_route(4096, 14336, bits) == ("generic", 1, 0)
    assert _lib.ap_plan_route(6144, 4096, bits, 1, False, EPI_RESIDUAL) == ("generic", 1, 0)
    with pytest.raises(RuntimeError):
        _lib.ap_plan_route(6144, 4096, bits, 1, True, 0)
    r = (ctypes.c_uint32 * 3)()
    assert L.gq_debug_ap_plan_route(28672, 4096, bits, 1, 1, EPI_SILU_PAIRS, 0, r) != 0


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_narrow_widths_never_plan_the_wide_kernel(L, bits):
    for model in SHAPES:
        for name, norm, epi in FORMS:
            N, K = SHAPES[model][name]
            assert _lib.ap_plan_route(N, K, bits, 1, norm, epi)[0] != "wide"
