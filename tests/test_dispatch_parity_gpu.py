"""GPU: every AP-GEMV launch the benchmark makes (tests/dispatch_table.py), on the route the default dispatch gives it, against the oracle.

For each row the launch runs in the default mode, in the form the decode step issues it (RMSNorm prologue, residual or gate/up pair
epilogue, the w2 workspace where the model allocates one), and in the exact mode, which the decode step runs without a workspace.  Each
launch asserts its route -- the real one (gq_debug_ap_last_route) equals the dry one (gq_debug_ap_plan_route), and both equal the table --
and then its result against the envelope of that route:
  - exact-order kernels (exact, pair-table, generic): bit-identical to oracle.ap_gemv_f16 of the numpy restatement of the fused op;
  - fast kernels: tests/ap_helpers._check_fast, with two fp16 roundings for the two-launch plane chain and one for everything else;
  - residual epilogue: bit-identical to the fp16 add of the residual and the plain launch's result (model.py:311-313) -- except on the
    two-launch plane chain, which adds the residual to its first K-half (four fp16 roundings against the oracle's halves);
  - pair epilogue: the unpaired launch of the same matrix takes the same route, and the pairs are silu_mul_ref of its even and odd rows --
    bit for bit on the dq and stream kernels, within one rounding of a SiLU quotient perturbed by 2^-16 on the kernels that evaluate it
    with __expf (plane, exact; tests/test_ap_exact_fused_gpu.check_pairs).
Rows checked: the first and last 32, both edge rows (16 g, 16 g + 15) of 64 row groups spread over N, and random rows (>= 256 in all).
The activations are hidden-state-like (a few massive channels); the exact mode's RMSNorm launches take the dyadic inputs whose normalised
values round unambiguously (tests/test_ap_exact_fused_gpu.dyadic_rmsnorm_input)."""
import os

import numpy as np
import pytest

from ap_helpers import _check_fast, half_add, rmsnorm_ref, silu_mul_ref
from dispatch_table import EPI_RESIDUAL, EPI_SILU_PAIRS, ROWS, W2_NO_WS_ROUTE, row_id
from test_ap_exact_fused_gpu import check_pairs, dyadic_rmsnorm_input
from test_ap_fused_gpu import _hidden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 1e-5
EXACT_FAMILIES = ("exact", "pair-table", "generic")


@pytest.fixture(autouse=True)
def _default_mode():
    from guidedquant_amd import _lib
    _lib.lib().gq_set_ap_mode(-1)
    yield
    _lib.lib().gq_set_ap_mode(-1)
    os.environ.pop("GQ_DQ", None)
    _lib.lib().gq_reset_env_cache()


class _Matrix:
    """one quantized matrix on cuda:0, launched through gq_anyprec_gemv_fused_ws (no workspace: gq_anyprec_gemv_fused's path)"""

    def __init__(self, N, K, bits, seed):
        from guidedquant_amd import pack
        rng = np.random.default_rng(seed)
        self.N, self.K, self.bits = N, K, bits
        self.q = pack.random_planes(N, K, bits, seed=seed)
        self.lut = np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1)
        self.qd, self.lutd = torch.from_numpy(self.q).cuda(), torch.from_numpy(self.lut).cuda()

    def __call__(self, x, nw=None, eps=EPS, res=None, flags=0, ws_bytes=0):
        """(output, real route, dry route) of one launch"""
        from guidedquant_amd import _lib
        L = _lib.lib()
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float16)).cuda()  # noqa: E731
        xd, nwd, rsd = dev(x), dev(nw), dev(res)
        out = torch.full((self.N // 2 if flags & EPI_SILU_PAIRS else self.N, ), float("nan"), dtype=torch.float16, device="cuda")
        ws = torch.full((ws_bytes // 4, ), float("nan"), dtype=torch.float32, device="cuda") if ws_bytes else None
        dry = _lib.ap_plan_route(self.N, self.K, self.bits, 1, nw is not None, flags, ws_bytes)
        rc = L.gq_anyprec_gemv_fused_ws(xd.data_ptr(), out.data_ptr(), self.qd.data_ptr(), self.lutd.data_ptr(), self.N, self.K, self.bits,
                                        nwd.data_ptr() if nwd is not None else None, eps, rsd.data_ptr() if rsd is not None else None, flags,
                                        ws.data_ptr() if ws is not None else None, ws_bytes, _lib.current_stream_ptr())
        _lib.check(rc, "gq_anyprec_gemv_fused_ws")
        real = _lib.ap_last_route()
        torch.cuda.synchronize()
        return out.cpu().numpy(), real, dry

    def sub(self, rows):
        return np.ascontiguousarray(self.q[:, rows, :]), self.lut[rows]


def _sample_rows(rng, N):
    """the first and last 32 rows, both edge rows of 64 row groups spread evenly over N, random rows up to >= 256 in all; closed under
    (2i, 2i + 1) so that the pair outputs of the sample can be checked"""
    groups = np.linspace(0, N // 16 - 1, 64).astype(np.int64)
    r = np.concatenate([np.arange(32), np.arange(N - 32, N), 16 * groups, 16 * groups + 15, rng.integers(0, N, 96)])
    r = np.unique(np.concatenate([r & ~1, (r & ~1) + 1]))
    assert r.size >= 256 and r.max() < N
    return r


def _route_ok(real, dry, want, what):
    assert real == dry, f"{what}: the launch ran {real}, the dry dispatch plans {dry}"
    allowed = (want, ) if isinstance(want, str) else want
    assert real[0] in allowed, f"{what}: ran the {real[0]} kernel, the table says {' / '.join(allowed)}"


def _check_launch(oracle, m, row, route, rng, ws_bytes, exact):
    """run the row's launch (and the unfused / unpaired twin it is checked against) on `route`; assert routes and results"""
    model, bits, name, N, K, norm, epi, _, _ = row
    rows = _sample_rows(rng, N)
    qs, ls = m.sub(rows)
    nround = 2.0 if route == "plane-chain" else 1.0
    tag = f"{row_id(row)} {'exact' if exact else 'default'} mode"

    def fast_or_exact(got, xin, fam):
        if fam in EXACT_FAMILIES:
            want = oracle.ap_gemv_f16(xin, qs, ls, bits)[0]
            assert np.array_equal(got[rows].view(np.uint16), want.view(np.uint16)), f"{tag}: not bit-identical to the reference order"
        else:
            _check_fast(got, xin, m.q, m.lut, bits, oracle, rows=rows, nround=nround)

    if norm:
        if exact:
            x, nw, eps = dyadic_rmsnorm_input(rng, K)
        else:
            x, nw, eps = _hidden(rng, K), (1 + 0.1 * rng.normal(0, 1, K)).astype(np.float16), EPS
        y, real, dry = m(x, nw=nw, eps=eps, ws_bytes=ws_bytes)
        _route_ok(real, dry, route, f"{tag}, unpaired" if epi & EPI_SILU_PAIRS else tag)
        assert np.isfinite(y[rows].astype(np.float32)).all()
        fast_or_exact(y, rmsnorm_ref(x, nw, eps), real[0])
        if epi & EPI_SILU_PAIRS:
            o, real_p, dry_p = m(x, nw=nw, eps=eps, flags=epi)
            _route_ok(real_p, dry_p, real[0], f"{tag}, pairs (the unpaired launch's family)")
            idx = np.unique(rows // 2)
            if real_p[0] in ("dq", "stream"):
                assert np.array_equal(o[idx].view(np.uint16), silu_mul_ref(y[2 * idx], y[2 * idx + 1]).view(np.uint16)), f"{tag}: pairs"
            else:
                check_pairs(o, y, idx, f"{tag}: pairs")
        return
    x = _hidden(rng, K)
    plain, real, dry = m(x, ws_bytes=ws_bytes)
    _route_ok(real, dry, route, f"{tag}, plain")
    fast_or_exact(plain, x, real[0])
    if epi & EPI_RESIDUAL:
        res = _hidden(rng, N)
        got, real_r, dry_r = m(x, res=res, flags=epi, ws_bytes=ws_bytes)
        _route_ok(real_r, dry_r, route, tag)
        if real_r[0] != "plane-chain":
            assert np.array_equal(got.view(np.uint16), half_add(res, plain).view(np.uint16)), f"{tag}: residual epilogue"
            return
        # the chain adds the residual to its first K-half: out = fp16(fp16(res + fp16(y1)) + fp16(y2)), four roundings, each <= 2^-11 of
        # the value rounded (tests/test_ap_fused_gpu.py::test_residual_epilogue_two_launch_k_split)
        k1 = ((K // 2 + 1023) // 1024) * 1024
        y1 = oracle.ap_gemv_f64(x[:k1], np.ascontiguousarray(qs[:, :, :k1 // 32]), ls, bits)[0]
        y2 = oracle.ap_gemv_f64(x[k1:], np.ascontiguousarray(qs[:, :, k1 // 32:]), ls, bits)[0]
        r = res[rows].astype(np.float64)
        scale = np.abs(oracle.ap_dequant(qs, ls, bits).astype(np.float64)) @ np.abs(x.astype(np.float64))
        tol = 2.0**-11 * 1.002 * (np.abs(y1) + np.abs(y2) + np.abs(r + y1) + np.abs(r + y1 + y2)) + 1e-5 * scale + 1e-7
        assert (np.abs(got[rows].astype(np.float64) - (r + y1 + y2)) <= tol).all(), f"{tag}: residual epilogue"


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_benchmarked_launch_on_its_route(oracle, row):
    from guidedquant_amd import _lib
    model, bits, name, N, K, norm, epi, ws, route = row
    seed = 1009 * bits + N + 7 * K + (1 if norm else 0)
    m = _Matrix(N, K, bits, seed)
    rng = np.random.default_rng(seed)
    _check_launch(oracle, m, row, route, rng, ws, exact=False)
    if ws:  # (and without the workspace: the two-launch chain)
        _check_launch(oracle, m, row, W2_NO_WS_ROUTE, rng, 0, exact=False)
    _lib.check(_lib.lib().gq_set_ap_mode(1), "gq_set_ap_mode")
    assert _lib.lib().gq_anyprec_gemv_fused_ws_bytes(N, K, bits, epi) == 0  # (the exact mode's decode step has no workspace)
    _check_launch(oracle, m, row, EXACT_FAMILIES, rng, 0, exact=True)


def test_dq_switched_off_moves_the_8b_4bit_w1w3_launch(oracle):
    """sensitivity: with GQ_DQ=0 the 8B 4-bit w1w3 launch leaves the dq kernel -- real and dry route alike -- and its result passes the
    envelope of the route it takes instead"""
    from guidedquant_amd import _lib
    row = next(r for r in ROWS if r[:3] == ("8B", 4, "w1w3"))
    os.environ["GQ_DQ"] = "0"
    _lib.lib().gq_reset_env_cache()
    _, bits, _, N, K, norm, epi, ws, route = row
    assert route == "dq"
    moved = _lib.ap_plan_route(N, K, bits, 1, norm, epi, ws)
    assert moved[0] != "dq"
    m = _Matrix(N, K, bits, 4242)
    _check_launch(oracle, m, row, moved[0], np.random.default_rng(4242), ws, exact=False)
