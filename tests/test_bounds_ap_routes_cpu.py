"""CPU (host logic): the dry AP-GEMV dispatch reproduces the route table of tests/test_bounds_ap_gemv_gpu.py -- every (case, form) and
every batch size lands on the kernel family the guarded GPU test expects, under the knobs that test sets.  No device is touched."""
import os

import pytest

import test_bounds_ap_gemv_gpu as t
from guidedquant_amd import _lib


@pytest.fixture(autouse=True)
def _restore_env():
    saved = {k: v for k, v in os.environ.items() if k.startswith("GQ_")}
    yield
    for k in [k for k in os.environ if k.startswith("GQ_")]:
        del os.environ[k]
    os.environ.update(saved)
    _lib.lib().gq_reset_env_cache()
    _lib.lib().gq_set_ap_mode(-1)


@pytest.mark.parametrize("case", t.CASES, ids=t.case_id)
def test_case_routes(case):
    fam, bits, N, K, forms, batch = case
    t.set_env(fam)
    launches = 2 if fam == "plane-chain" else 1
    for form, norm, flags in t.case_forms(case):
        got = _lib.ap_plan_route(N, K, bits, 1, norm, flags, 0)
        assert got[:2] == (fam, launches), f"{t.case_id(case)} {form} plans {got}"
    for M in batch:
        got = _lib.ap_plan_route(N, K, bits, M, False, 0, 0)
        assert got[:2] == (fam, launches), f"{t.case_id(case)} M = {M} plans {got}"
    if fam == "stream" and N % 2:   # the residual epilogue at an odd N is declined by the stream kernel: the plane kernels serve it
        for norm, flags in ((False, 1), (True, 1), (False, 3)):
            assert _lib.ap_plan_route(N, K, bits, 1, norm, flags, 0)[0] in ("plane", "plane-local")


def test_the_table_covers_every_reachable_family():
    reached = {c[0] for c in t.CASES} | {"stream-ksplit"}
    assert reached == set(_lib.AP_ROUTES) - {"none", "stream-qkv-rope"}
    for c in t.CASES:
        assert c[2] % 16 != 0
    for fam in reached - {"stream-ksplit"}:
        ns = {c[2] for c in t.CASES if c[0] == fam}
        assert any(n % 4 for n in ns) and any(n % 2 for n in ns) and any(n % 2 == 0 and n % 32 for n in ns)


@pytest.mark.parametrize("N,K,kslice", t.KSPLIT_CASES)
def test_ksplit_routes(N, K, kslice):
    t.set_env("stream-ksplit", GQ_ST_KSLICE=kslice)
    nb = _lib.lib().gq_anyprec_gemv_fused_ws_bytes(N, K, 2, 1)
    assert nb == (K // (4096 if kslice == 0 and K % 4096 == 0 else 2048)) * N * 4
    for flags in (0, 1):
        assert _lib.ap_plan_route(N, K, 2, 1, False, flags, nb)[:2] == ("stream-ksplit", 2)
        assert _lib.ap_plan_route(N, K, 2, 1, False, flags, nb - 4)[0] == "plane-chain"   # a workspace one float short is not used
    assert any(n % 4 for n, _, _ in t.KSPLIT_CASES)
