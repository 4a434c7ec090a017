"""The tail of the local-image GEMV's decode instance (`ap_plane_local_kernel<2, 0, 1, true>`: the 2-bit wo / w2 launches): when the
block's last wave has no chunk to multiply it owns the epilogue lanes, with its lane's Moebius coefficient and its residual element
staged BEFORE the last block barrier (csrc/ap_plane.hip, TAIL).  Which values are added, and in which order, is what
`plane_epilogue` does on wave 0 -- so every output must equal, bit for bit, the general instance of the same launch (GQ_PL_SPEC=0:
code the staged tail does not touch), and lie inside the fast-mode envelope of ap_helpers._check_fast.

Shapes: the smallest at which the tail can go wrong.  Rows 16 (one block), 48 (three), 40 (ragged: `row < N` masks lanes of the last
block).  K = 1024 .. 14336 gives 1, 2, 4, 8 and 14 chunks: both arms of the partial-sum reads (CS < 8 and CS >= 8), a last wave
without an item (K <= 8192) and one whose item lies past the last chunk (14336); K = 16384 gives every wave a chunk, so the block
keeps the wave-0 epilogue.  Every buffer is guard-banded and poisoned (tests/guarded.py)."""
import os

import numpy as np
import pytest

import guarded
from ap_helpers import FAST_KNOBS, _check_fast, _fast, assert_route, half_add, run_fused_guarded

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GQ_EPI_RESIDUAL = 1
BITS = 2
ROWS = (16, 48, 40)
KS = (1024, 2048, 4096, 8192, 14336, 16384)


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    from guidedquant_amd import _lib
    _lib.lib().gq_set_ap_mode(-1)
    for k in FAST_KNOBS + ("GQ_PL_SPEC", ):
        os.environ.pop(k, None)
    _lib.lib().gq_reset_env_cache()


def _instance(spec):
    """fast mode, the local-image kernel wherever it serves the shape; spec = 0: its general instance"""
    os.environ["GQ_PL_SPEC"] = str(spec)
    _fast(local=1)


_LAYERS = {}


def _layer(N, K):
    """LUT rows that differ per row; a vector with massive channels in the first and the last chunk (extracted elements: the hot
    list of the first and of the last multiplying wave); a residual with large and small entries.  Made once per shape."""
    if (N, K) not in _LAYERS:
        from guidedquant_amd import pack
        rng = np.random.default_rng(1000 * N + K)
        q = pack.random_planes(N, K, BITS, seed=N + K)
        lut = np.sort(rng.normal(0, 0.02, (N, 1 << BITS)) * rng.uniform(0.5, 4.0, (N, 1)), axis=1).astype(np.float16)
        x = rng.normal(0, 1, K)
        x[[5, K - 3]] = [900.0, -1300.0]
        resid = rng.normal(0, 1, N)
        resid[::5] *= 30.0
        _LAYERS[(N, K)] = (q, lut, x.astype(np.float16), resid.astype(np.float16))
    return _LAYERS[(N, K)]


_GENERAL = {}


def _general(N, K, with_resid):
    """the general instance's output of the shape's launch (the reference of the bit-for-bit comparison), computed once"""
    key = (N, K, with_resid)
    if key not in _GENERAL:
        q, lut, x, resid = _layer(N, K)
        _instance(0)
        kw = dict(residual=resid, flags=GQ_EPI_RESIDUAL) if with_resid else {}
        _GENERAL[key] = run_fused_guarded(x, q, lut, BITS, expect="plane-local", **kw)
    return _GENERAL[key]


@pytest.mark.parametrize("with_resid", [True, False])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", ROWS)
def test_decode_instance_equals_general_instance(oracle, N, K, with_resid):
    q, lut, x, resid = _layer(N, K)
    want = _general(N, K, with_resid)
    _instance(1)
    kw = dict(residual=resid, flags=GQ_EPI_RESIDUAL) if with_resid else {}
    got = run_fused_guarded(x, q, lut, BITS, expect="plane-local", **kw)
    assert np.isfinite(got.astype(np.float32)).all()  # (an output nobody wrote keeps the poison: NaN)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), np.flatnonzero(got.view(np.uint16) != want.view(np.uint16))
    if with_resid:
        # one fp16 add behind the fp16-rounded product: the plain launch of the same instance, then the add
        plain = run_fused_guarded(x, q, lut, BITS, expect="plane-local")
        assert np.array_equal(got.view(np.uint16), half_add(resid, plain).view(np.uint16))
    else:
        _check_fast(got, x, q, lut, BITS, oracle)


@pytest.mark.parametrize("K", [1024, 14336])
def test_residual_is_added_in_fp16(K):
    """rows whose product is exactly 2049 (a constant LUT row 2.0 -- coefficient 2 on sum(x), 0 on the plane sums -- and sum(x) =
    1024.5) with a residual of 1: fp16(2049) = 2048 and 2048 + 1 rounds back to 2048 in fp16, an fp32 add would give 2050"""
    from guidedquant_amd import pack
    N = 40
    rng = np.random.default_rng(K)
    q = pack.random_planes(N, K, BITS, seed=K)
    lut = np.sort(rng.normal(0, 0.02, (N, 1 << BITS)).astype(np.float16), axis=1)
    pinned = np.arange(0, N, 3)
    lut[pinned] = np.float16(2.0)
    x = np.zeros(K, dtype=np.float16)
    x[:1024] = 1.0
    x[K - 1] += np.float16(0.5)
    resid = np.ones(N, dtype=np.float16)
    out = {}
    for spec in (0, 1):
        _instance(spec)
        out[spec] = run_fused_guarded(x, q, lut, BITS, residual=resid, flags=GQ_EPI_RESIDUAL, expect="plane-local")
    assert (out[1][pinned] == np.float16(2048.0)).all(), out[1][pinned]
    assert np.array_equal(out[1].view(np.uint16), out[0].view(np.uint16))


def _launcher(g, tag, x, q, lut, resid):
    """a closure that issues the shape's launch on the current stream into an output of its own (poisoned until then)"""
    from guidedquant_amd import _lib
    N, K = q.shape[1], q.shape[2] * 32
    p = guarded.ptr
    xb, qb, lb = g.inp("x" + tag, x), g.inp("q" + tag, np.ascontiguousarray(q)), g.inp("lut" + tag, lut)
    rb, out = g.inp("resid" + tag, resid), g.out("out" + tag, 2 * N)

    def launch():
        _lib.check(_lib.lib().gq_anyprec_gemv_fused(p(xb), p(out), p(qb), p(lb), N, K, BITS, None, 1e-5, p(rb), GQ_EPI_RESIDUAL if resid is not None else 0,
                                                    _lib.current_stream_ptr()), "gq_anyprec_gemv_fused")
        assert_route("plane-local")

    return launch, out


@pytest.mark.parametrize("K", [4096, 14336])
def test_repeated_launches_and_captured_graph(K):
    """the same launch twice in a row into different outputs, then four launches (two residuals, none, the first again) eagerly
    and inside one captured graph: a staged coefficient or residual element that outlived its launch would show"""
    from guidedquant_amd._graphs import capture, release
    N = 40
    q, lut, x, resid = _layer(N, K)
    resid2 = (-resid * np.float16(0.5) + np.float16(3.0)).astype(np.float16)
    want = [_general(N, K, True), None, _general(N, K, False)]
    _instance(0)
    want[1] = run_fused_guarded(x, q, lut, BITS, residual=resid2, flags=GQ_EPI_RESIDUAL, expect="plane-local")
    order = [0, 1, 2, 0]
    _instance(1)
    g = guarded.Guards()
    twice = [_launcher(g, f"t{i}", x, q, lut, resid) for i in range(2)]
    for launch, _ in twice:
        launch()
    eager = [_launcher(g, f"e{i}", x, q, lut, (resid, resid2, None)[o]) for i, o in enumerate(order)]
    for launch, _ in eager:
        launch()
    graph = [_launcher(g, f"g{i}", x, q, lut, (resid, resid2, None)[o]) for i, o in enumerate(order)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with capture(gr, stream=s):
            for launch, _ in graph:
                launch()
    torch.cuda.current_stream().wait_stream(s)
    gr.replay()
    g.check()
    release(gr)
    for _, out in twice:
        assert np.array_equal(out.numpy(np.uint16), want[0].view(np.uint16))
    for what, runs in (("eager", eager), ("graph", graph)):
        for (_, out), o in zip(runs, order):
            assert np.array_equal(out.numpy(np.uint16), want[o].view(np.uint16)), (what, o)
