"""GPU: the Any-Precision GEMV at 5 to 8 bits (ap_wide.hip::ap_gemv_wide_kernel), in both modes, against the reference chain bit for
bit: the plain launch on every Llama 8B / 70B decode shape (sampled rows against oracle.ap_gemv_f16, every row against the generic
kernel under GQ_AP_FORCE_GENERIC=1), small and odd shapes, LNQ-like heavy-tailed layers, and every fused form the decode step issues
(RMSNorm and SiLU * up prologues, residual and gate / up pair epilogues) through gq_anyprec_gemv_fused, _fused_ws and _fused_ho.
At 7 and 8 bits the rows of more than 4096 weights take the reference's K-split reduction (anyprec.cu:611)."""
import os

import numpy as np
import pytest

import test_ap_exact_fused_gpu as ef
from ap_helpers import assert_route, half_add, lnq_like_layer, run_fused

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BITS = [5, 6, 7, 8]
MODES = [0, 1]
GQ_EPI_RESIDUAL, GQ_PRO_SILU_MUL, GQ_EPI_SILU_PAIRS = 1, 2, 4
LLAMA = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (10240, 8192), (8192, 8192), (57344, 8192), (8192, 28672)]


def _lib():
    from guidedquant_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _reset():
    yield
    L = _lib().lib()
    L.gq_set_ap_mode(-1)
    os.environ.pop("GQ_AP_FORCE_GENERIC", None)
    L.gq_reset_env_cache()


def _mode(mode):
    _lib().check(_lib().lib().gq_set_ap_mode(mode), "gq_set_ap_mode")


def _force_generic(on):
    if on:
        os.environ["GQ_AP_FORCE_GENERIC"] = "1"
    else:
        os.environ.pop("GQ_AP_FORCE_GENERIC", None)
    _lib().lib().gq_reset_env_cache()


def _gemv(xt, qt, lt, bits, N):
    from guidedquant_amd import ap_gemv
    out = torch.full((1, 1, N), float("nan"), dtype=torch.float16, device=xt.device)
    ap_gemv.anyprec_gemv(xt.reshape(1, 1, -1), out, qt, lt, bits)
    route = _lib().ap_last_route()
    torch.cuda.synchronize()
    return out.reshape(N).cpu().numpy(), route


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("N,K", LLAMA)
def test_plain_llama_shapes(oracle, bits, N, K):
    """sampled rows against the oracle; every row against the generic kernel"""
    from guidedquant_amd import pack
    d = torch.device("cuda:0")
    rng = np.random.default_rng(bits * 1000 + N + K)
    q = pack.random_planes(N, K, bits, seed=bits * 31 + N)
    lut = np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1)
    x = rng.normal(0, 1, K).astype(np.float16)
    rows = np.unique(np.concatenate([np.arange(0, 40), np.arange(N - 40, N), rng.integers(0, N, 64)]))
    want = oracle.ap_gemv_f16(x, np.ascontiguousarray(q[:, rows, :]), lut[rows], bits)[0]
    qt, lt, xt = torch.from_numpy(q).to(d), torch.from_numpy(lut).to(d), torch.from_numpy(x).to(d)
    del q
    outs = []
    for mode in MODES:
        _mode(mode)
        got, route = _gemv(xt, qt, lt, bits, N)
        assert route[:2] == ("wide", 1), route
        ef._eq(got[rows], want, f"mode {mode}")
        outs.append(got)
    _force_generic(True)
    slow, route = _gemv(xt, qt, lt, bits, N)
    assert route[0] == "generic"
    for got in outs:
        ef._eq(got, slow, "wide vs generic kernel")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("N,K", [(1, 128), (7, 384), (64, 1024), (33, 1152), (20, 4608), (12, 11008), (9, 14336), (4, 5120), (3, 32768)])
def test_plain_small_shapes(oracle, bits, N, K):
    """odd N, one-quad rows, partial last chunks, the longest rows; LUTs and activations over many binades"""
    d = torch.device("cuda:0")
    rng = np.random.default_rng(bits * 7919 + N * 131 + K)
    codes = rng.integers(0, 1 << bits, (N, K), dtype=np.uint8)
    q = oracle.ap_pack(codes, bits)
    lut = (rng.normal(0, 1, (N, 1 << bits)) * 10.0**rng.integers(-5, 1, (N, 1))).astype(np.float16)
    x = (rng.normal(0, 1, K) * 10.0**rng.integers(-3, 2, K)).astype(np.float16)
    want = oracle.ap_gemv_f16(x, q, lut, bits)[0]
    qt, lt, xt = torch.from_numpy(q).to(d), torch.from_numpy(lut).to(d), torch.from_numpy(x).to(d)
    for mode in MODES:
        _mode(mode)
        got, route = _gemv(xt, qt, lt, bits, N)
        assert route[:2] == ("wide", 1), route
        ef._eq(got, want, f"mode {mode}")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("N,K", [(4096, 4096), (2048, 14336)])
def test_lnq_like_layers(oracle, bits, N, K):
    """skewed codes, outlier centroids, massive-activation channels"""
    q, lut, x = lnq_like_layer(N, K, bits, seed=bits + N)
    want = oracle.ap_gemv_f16(x, q, lut, bits)[0]
    for mode in MODES:
        _mode(mode)
        ef._eq(run_fused(x, q, lut, bits, expect="wide"), want, f"mode {mode}")


def _entry_points(x, q, lut, bits, norm_weight=None, eps=1e-5, residual=None, flags=0, out_elems=None):
    """the launch through gq_anyprec_gemv_fused_ws (no workspace: there is none at these widths) and gq_anyprec_gemv_fused_ho (null
    hand-over pointers, as the decode step passes them); both must run the wide kernel"""
    L = _lib().lib()
    d = torch.device("cuda:0")
    N, K = q.shape[1], q.shape[2] * 32
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float16)).to(d)  # noqa: E731
    xt, lt, nw, rs = t(x), t(lut), t(norm_weight), t(residual)
    qt = torch.from_numpy(np.ascontiguousarray(q)).to(d)
    p = lambda a: a.data_ptr() if a is not None else None  # noqa: E731
    assert L.gq_anyprec_gemv_fused_ws_bytes(N, K, bits, flags) == 0
    outs = []
    for ho in (False, True):
        out = torch.full((out_elems or N, ), float("nan"), dtype=torch.float16, device=d)
        if ho:
            rc = L.gq_anyprec_gemv_fused_ho(p(xt), p(out), p(qt), p(lt), N, K, bits, p(nw), eps, p(rs), flags, None, 0, None, None,
                                            _lib().current_stream_ptr())
        else:
            rc = L.gq_anyprec_gemv_fused_ws(p(xt), p(out), p(qt), p(lt), N, K, bits, p(nw), eps, p(rs), flags, None, 0, _lib().current_stream_ptr())
        _lib().check(rc, "fused_ho" if ho else "fused_ws")
        assert_route("wide")
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    return outs


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("N,K", [(6144, 4096), (4096, 14336), (1000, 8192), (4098, 4608), (520, 28672), (1000, 128)])
def test_fused_forms_match_the_reference_chain(bits, N, K):
    """every fused form against the reference's separate ops + the oracle chain (inputs with unambiguous rounding points:
    test_ap_exact_fused_gpu.py), in both modes; the _ws and _ho entry points give the same bits"""
    f = ef._forms(N, K, bits, seed=N * 7 + K + bits)
    q, lut, rows, res = f["q"], f["lut"], f["rows"], f["res"]
    x, nw, eps, gu = f["x"], f["nw"], f["eps"], f["gu"]
    forms = [(dict(x=x, norm_weight=nw, eps=eps), f["y_n"]), (dict(x=gu, flags=GQ_PRO_SILU_MUL), f["y_s"]),
             (dict(x=x, norm_weight=nw, eps=eps, residual=res, flags=GQ_EPI_RESIDUAL), half_add(res[rows], f["y_n"])),
             (dict(x=gu, residual=res, flags=GQ_PRO_SILU_MUL | GQ_EPI_RESIDUAL), half_add(res[rows], f["y_s"]))]
    for mode in MODES:
        _mode(mode)
        ef.check_all_forms(N, K, bits, f, f" (mode {mode})")
        for kw, want in forms:
            got = run_fused(expect="wide", q=q, lut=lut, bits=bits, **kw)
            ef._eq(got[rows], want, f"mode {mode} {sorted(kw)}")
            for o in _entry_points(q=q, lut=lut, bits=bits, **kw):
                ef._eq(o, got, f"mode {mode} _ws / _ho {sorted(kw)}")
        if N % 2 == 0:
            y_full = np.zeros(N, np.float16)
            y_full[rows] = f["y_n"]
            kw = dict(x=x, norm_weight=nw, eps=eps, flags=GQ_EPI_SILU_PAIRS, out_elems=N // 2)
            o = run_fused(expect="wide", q=q, lut=lut, bits=bits, **kw)
            ef.check_pairs(o, y_full, np.unique(rows // 2), f"RMSNorm + pairs (mode {mode})")
            for o2 in _entry_points(q=q, lut=lut, bits=bits, **kw):
                ef._eq(o2, o, f"mode {mode} _ws / _ho pairs")
