"""CPU (host logic): the dry AP-GEMV dispatch (gq_debug_ap_plan_route: every decision of a real launch, nothing launched) sends every
launch the benchmark makes to the kernel family tests/dispatch_table.py lists, and the exact mode sends it to an exact-order kernel.  The
dispatch reads its GQ_* knobs from the environment as a real run does: a knob that moves a launch fails the row it moves.  No device is
touched (256 CUs are assumed without one: the MI355X's count)."""
import ctypes

import pytest

from dispatch_table import EPI_RESIDUAL, ROWS, W2_NO_WS_ROUTE, row_id
from guidedquant_amd import _lib


@pytest.fixture
def L():
    L = _lib.lib()
    L.gq_reset_env_cache()
    L.gq_set_ap_mode(0)
    yield L
    L.gq_set_ap_mode(-1)


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_default_route(L, row):
    model, bits, name, N, K, norm, epi, ws, route = row
    if name == "w2":
        assert L.gq_anyprec_gemv_fused_ws_bytes(N, K, bits, epi) == ws, "the workspace the model allocates for w2 moved"
    got = _lib.ap_plan_route(N, K, bits, 1, norm, epi, ws)
    assert got[0] == route, f"{row_id(row)} plans {got[0]}, the table says {route}"
    assert got[1] == (2 if route in ("plane-chain", "stream-ksplit") else 1)
    if ws:
        assert _lib.ap_plan_route(N, K, bits, 1, norm, epi, 0)[0] == W2_NO_WS_ROUTE


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_exact_mode_route(L, row):
    model, bits, name, N, K, norm, epi, ws, route = row
    L.gq_set_ap_mode(1)
    fam, launches, variant = _lib.ap_plan_route(N, K, bits, 1, norm, epi, 0)
    assert fam in ("exact", "pair-table", "generic"), f"{row_id(row)} plans {fam} in the exact mode"
    assert launches == 1
    # the exact variant is the one gq_debug_exact_plan_ex reports
    if fam != "generic":
        plan = (ctypes.c_uint32 * 7)()
        pro = 1 if norm else 0
        assert L.gq_debug_exact_plan_ex(N, K, bits, pro, epi, plan) == 0
        assert variant == plan[6] and (fam == "pair-table") == (plan[6] == 2)


def test_last_route_follows_the_dry_dispatch(L):
    assert _lib.ap_plan_route(4096, 4096, 2, 1, False, EPI_RESIDUAL)[0] == _lib.ap_last_route()[0]
    # a rejected launch records no route
    assert L.gq_debug_ap_plan_route(4096, 4096, 9, 1, 0, 0, 0, (ctypes.c_uint32 * 3)()) != 0
    assert _lib.ap_last_route() == ("none", 0, 0)
