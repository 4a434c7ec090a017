"""GPU: the QTIP entries with every buffer guard-banded and poisoned (tests/guarded.py) at their smallest and raggedest shapes:
gq_qtip_matvec, gq_qtip_decompress, gq_qtip_gemm / gq_qtip_gemm_ws (with forced K splits and token tiles), gq_hadamard and the
one-launch gq_qtip_linear with every pointer inside GqQtipIn / GqQtipOut guarded.  M in {32, 96} x K in {32, 96, 160, 1056} (one tile
block; 3, 5 and 33 tile blocks of 32 columns: the ragged chunks test_qtip_gpu.test_matvec_ragged_chunks_and_many_items shows are
served), S in {9, 33}.  Results against the oracle's decode exactly as tests/test_qtip_gpu.py and tests/test_qtip_gemm_gpu.py check
them (bit identity for the decode, 2e-6 * sum|w||x| + 1e-7 for the products); guards: exact equality."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
from test_qtip_gemm_gpu import _bound, _recipe, _x  # noqa: E402
from test_qtip_gpu import _check as check_matvec  # noqa: E402
from test_qtip_gpu import _fused_linear, _rand_qlinear  # noqa: E402

MS, KS, SS = (32, 96), (32, 96, 160, 1056), (9, 33)
KNOBS = ("GQ_QTIP_GEMM_KSPLIT", "GQ_QTIP_GEMM_CF")


def _L():
    from guidedquant_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _env():
    for k in KNOBS:
        os.environ.pop(k, None)
    _L().lib().gq_reset_env_cache()
    yield
    for k in KNOBS:
        os.environ.pop(k, None)
    _L().lib().gq_reset_env_cache()


_decoded = {}


def _problem(oracle, R, M, K):
    """(compressed, tlut, the oracle's decode): made once per shape"""
    if (R, M, K) not in _decoded:
        comp, tlut = _recipe(R, M, K, seed=42 + R + M + K)
        _decoded[(R, M, K)] = (comp, tlut, oracle.qtip_decode(comp, tlut, M, K, R))
    return _decoded[(R, M, K)]


@pytest.mark.parametrize("R", [2, 3, 4])
def test_guarded_matvec_and_decompress(oracle, R):
    L = _L()
    for M in MS:
        for K in KS:
            comp, tlut, W = _problem(oracle, R, M, K)
            x = _x(1, K, seed=K)[0]
            g = guarded.Guards()
            cb, tb, xb = g.inp("compressed", comp), g.inp("codebook", tlut), g.inp("x", x)
            ob, wb = g.out("out", 4 * M), g.out("W", 2 * M * K)
            L.check(L.lib().gq_qtip_matvec(ob.ptr(), cb.ptr(), xb.ptr(), tb.ptr(), M, K, R, L.current_stream_ptr()), "gq_qtip_matvec")
            L.check(L.lib().gq_qtip_decompress(wb.ptr(), cb.ptr(), tb.ptr(), M, K, R, L.current_stream_ptr()), "gq_qtip_decompress")
            g.check()
            check_matvec(ob.numpy(np.float32), comp, tlut, x, M, K, R, oracle)
            assert np.array_equal(wb.numpy(np.uint16, (M, K)), W.view(np.uint16)), (M, K)


def _gemm_guarded(comp, tlut, x, M, R, ws):
    L = _L()
    S, K = x.shape
    g = guarded.Guards()
    cb, tb, xb = g.inp("compressed", comp), g.inp("codebook", tlut), g.inp("x", x)
    ob = g.out("out", 4 * S * M)
    nb = 0
    if ws:
        nb = int(L.lib().gq_qtip_gemm_ws_bytes(S, M, K, R))
        wb = g.out("workspace", nb)
        rc = L.lib().gq_qtip_gemm_ws(ob.ptr(), cb.ptr(), xb.ptr(), tb.ptr(), S, M, K, R, wb.ptr(), nb, L.current_stream_ptr())
    else:
        rc = L.lib().gq_qtip_gemm(ob.ptr(), cb.ptr(), xb.ptr(), tb.ptr(), S, M, K, R, L.current_stream_ptr())
    L.check(rc, "gq_qtip_gemm")
    g.check()
    return ob.numpy(np.float32, (S, M)), nb


def _check_gemm(got, W, x):
    ref, scale = _bound(W, x)
    err = np.abs(got.astype(np.float64) - ref.T)
    assert (err <= 2e-6 * scale.T + 1e-7).all(), float((err / (scale.T + 1e-30)).max())


@pytest.mark.parametrize("cf", [None, 4, 8])
@pytest.mark.parametrize("ksplit", [None, 2, 3])
@pytest.mark.parametrize("R", [2, 3, 4])
def test_guarded_qtip_gemm(oracle, R, ksplit, cf):
    """ksplit None: the planner's own choice for these short grids; 2 / 3: forced -- K = 1056 (33 tile blocks) then runs uneven
    ranges (17 + 16, 11 + 11 + 11), the narrower K fewer ranges than asked (each holds at least 8 tile blocks: none).  The workspace
    has exactly gq_qtip_gemm_ws_bytes bytes under the same environment, possibly none."""
    L = _L()
    if ksplit is not None:
        os.environ["GQ_QTIP_GEMM_KSPLIT"] = str(ksplit)
    if cf is not None:
        os.environ["GQ_QTIP_GEMM_CF"] = str(cf)
    L.lib().gq_reset_env_cache()
    for M in MS:
        for K in KS:
            comp, tlut, W = _problem(oracle, R, M, K)
            for S in SS:
                x = _x(S, K, seed=S + K)
                one, _ = _gemm_guarded(comp, tlut, x, M, R, ws=False)
                _check_gemm(one, W, x)
                got, nb = _gemm_guarded(comp, tlut, x, M, R, ws=True)
                if ksplit is not None:
                    ranges = {2: 2, 3: 3}[ksplit] if K == 1056 else 1
                    assert nb == (ranges * S * M * 4 if ranges > 1 else 0), (nb, S, M, K)
                _check_gemm(got, W, x)
                if not nb:
                    assert np.array_equal(got.view(np.uint32), one.view(np.uint32))


@pytest.mark.parametrize("rows,n", [(1, 2), (3, 32), (1, 64), (5, 1024), (2, 8192)])
def test_guarded_hadamard(rows, n):
    L = _L()
    rng = np.random.default_rng(rows + n)
    X = rng.normal(0, 1, (rows, n)).astype(np.float32)
    i = np.arange(n)
    b = i[:, None] & i[None, :]
    par = np.zeros_like(b)
    for k in range(14):
        par ^= (b >> k) & 1
    H = (1 - 2 * par).astype(np.float64)   # Sylvester order
    scale = 1.0 / np.sqrt(n)
    g = guarded.Guards()
    xb, yb = g.inp("x", X), g.out("y", 4 * rows * n)
    L.check(L.lib().gq_hadamard(xb.ptr(), yb.ptr(), rows, n, scale, L.current_stream_ptr()), "gq_hadamard")
    g.check()
    assert np.array_equal(xb.numpy(np.float32, (rows, n)), X)   # out of place: the input is left alone
    np.testing.assert_allclose(yb.numpy(np.float32, (rows, n)), scale * (X.astype(np.float64) @ H), rtol=2e-5, atol=2e-5)   # (test_hadamard_goldens)


@pytest.mark.parametrize("Ms,K,pro,ks,R", [([256], 128, 0, 1, 2), ([32, 64], 64, 1, 1, 3), ([64], 256, 2, 2, 4), ([128, 32, 32], 32, 1, 1, 2)])
def test_guarded_qtip_linear_one_launch(Ms, K, pro, ks, R):
    """gq_qtip_linear with x, x2, norm_weight, the counters and every pointer of GqQtipIn / GqQtipOut (trellis, SU, tlut, the split-K
    sums, SV32, resid, out) guarded; bit-identical to the two-launch form on plain tensors (test_one_launch_linear_equals_two_launches)."""
    L = _L()
    d = torch.device("cuda:0")
    mods = [_rand_qlinear(K, M, R, seed=100 * R + i + M + K) for i, M in enumerate(Ms)]
    gen = torch.Generator(device="cpu").manual_seed(K + sum(Ms))
    x = (torch.randn(K, generator=gen) * 0.7).half().to(d)
    x2 = torch.randn(K, generator=gen).half().to(d)
    normw = (1 + 0.2 * torch.randn(K, generator=gen)).half().to(d)
    resid = torch.randn(Ms[0], generator=gen).half().to(d) if len(Ms) == 1 else None
    g = guarded.Guards()
    xb, x2b, nwb = g.inp("x", x), g.inp("x2", x2), g.inp("norm_weight", normw)
    rb = g.inp("resid", resid)
    ctr = g.inp("counters", torch.zeros(len(Ms), dtype=torch.int32))
    ain, aout = (L.GqQtipIn * len(Ms))(), (L.GqQtipOut * len(Ms))()
    outs = []
    for i, m in enumerate(mods):
        tr, su, tl = g.inp(f"trellis{i}", m.trellis), g.inp(f"SU{i}", m.SU.float()), g.inp(f"tlut{i}", m.tlut.data)
        sv = g.inp(f"SV32_{i}", m.SV.float() * 32.0)
        y32, ob = g.out(f"y32_{i}", 4 * ks * Ms[i]), g.out(f"out{i}", 2 * Ms[i])
        ain[i] = L.GqQtipIn(tr.ptr(), su.ptr(), tl.ptr(), y32.ptr(), Ms[i])
        aout[i] = L.GqQtipOut(y32.ptr(), sv.ptr(), guarded.ptr(rb), ob.ptr(), Ms[i], ks)
        outs.append(ob)
    for _ in range(2):   # the finishing block resets its counter: a second launch finds them zero
        L.check(L.lib().gq_qtip_linear(xb.ptr(), x2b.ptr(), nwb.ptr(), 1e-5, pro, K, R, len(Ms), ain, aout, ks, ctr.ptr(), L.current_stream_ptr()),
                "gq_qtip_linear")
    g.check()
    assert int(ctr.view(torch.int32).abs().sum()) == 0
    # the two-launch form on plain tensors
    su = [m.SU.float().contiguous() for m in mods]
    sv = [(m.SV.float() * 32.0).contiguous() for m in mods]
    y2 = [torch.full((ks * M, ), float("nan"), dtype=torch.float32, device=d) for M in Ms]
    o2 = [torch.full((M, ), float("nan"), dtype=torch.float16, device=d) for M in Ms]
    bin_ = (L.GqQtipIn * len(Ms))(*[L.GqQtipIn(m.trellis.data_ptr(), su[i].data_ptr(), m.tlut.data_ptr(), y2[i].data_ptr(), Ms[i]) for i, m in enumerate(mods)])
    bout = (L.GqQtipOut * len(Ms))(*[L.GqQtipOut(y2[i].data_ptr(), sv[i].data_ptr(), resid.data_ptr() if resid is not None else None, o2[i].data_ptr(),
                                                 Ms[i], ks) for i in range(len(Ms))])
    L.check(L.lib().gq_qtip_linear_in(x.data_ptr(), x2.data_ptr(), normw.data_ptr(), 1e-5, pro, K, R, len(Ms), bin_, 0, None, ks, None), "in")
    L.check(L.lib().gq_qtip_linear_out(len(Ms), bout, None), "out")
    torch.cuda.synchronize()
    for a, b in zip(o2, outs):
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(a.view(torch.int16), b.view(torch.int16, a.shape))
