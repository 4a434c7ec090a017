"""GPU: both prefill GEMMs (gq_anyprec_gemm / gq_anyprec_gemm_ws: csrc/ap_gemm.hip at 2..4 bits, csrc/ap_gemm_wide.hip at 5..8) at
ragged shapes with every buffer guard-banded and poisoned (tests/guarded.py): x, qweight and lut flush against a poisoned guard, out
and the split-K workspace pre-filled with the poison between two guards.  The workspace has exactly gq_anyprec_gemm_ws_bytes bytes
under the same environment.  Results are checked with test_ap_gemm_gpu._check (fp32 accumulation, one fp16 rounding), split against
single pass with the bound test_gemm_split_k_on_short_grids states, on that test's kind of layer (its absolute term, 1e-4, is a
statement about centroids of 0.02 and unit activations: on the wide-range layers of test_gemm_random, sums of several hundred, two
fp32 summation orders differ by more than that while both pass _check); the guard assertions are exact equality.

Shapes: S in {2, 33, 129, 257} x N in {36, 130, 261} x K in {64, 1088, 2304}: token, row and K tails of every tile (128 / 256 rows
and tokens), K = 64 / 1088 on the first kernel and 2304 on the pipelined one; N = 261 is odd, so S * N is odd for odd S and the
split-K reduction (gemm_reduce_kernel) takes its scalar branch.  Forced splits (GQ_GEMM_KSPLIT x GQ_GEMM_KSHAPE) at K = 2304 (9
groups of 256: ranges of 5 + 4) and K = 4352 (17 groups: 9 + 8, 6 + 6 + 5, 5 + 5 + 5 + 2) run uneven K ranges.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
from test_ap_gemm_gpu import _check  # noqa: E402

SS, NS, KS = (2, 33, 129, 257), (36, 130, 261), (64, 1088, 2304)
KNOBS = ("GQ_GEMM_SHAPE", "GQ_GEMM_KSPLIT", "GQ_GEMM_KSHAPE")


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


@pytest.fixture(autouse=True)
def _env():
    from guidedquant_amd import _lib
    for k in KNOBS:
        os.environ.pop(k, None)
    _lib.lib().gq_reset_env_cache()
    yield
    for k in KNOBS:
        os.environ.pop(k, None)
    _lib.lib().gq_reset_env_cache()


def _set(**kv):
    from guidedquant_amd import _lib
    for k, v in kv.items():
        os.environ[k] = str(v)
    _lib.lib().gq_reset_env_cache()


_layers, _xs = {}, {}


def _layer(oracle, bits, N, K):
    """(qweight, lut) of one problem, made once and shared by every test that uses it"""
    if (bits, N, K) not in _layers:
        rng = np.random.default_rng(bits * 977 + N + K)
        q = oracle.ap_pack(rng.integers(0, 1 << bits, (N, K), dtype=np.uint8), bits)
        lut = (rng.normal(0, 1, (N, 1 << bits)) * 10.0**rng.integers(-3, 1, (N, 1))).astype(np.float16)
        _layers[(bits, N, K)] = (q, lut)
    return _layers[(bits, N, K)]


def _narrow_layer(bits, N, K):
    """the layer of test_ap_gemm_gpu.test_gemm_split_k_on_short_grids, whose bound the split comparison uses"""
    if ("narrow", bits, N, K) not in _layers:
        from guidedquant_amd import pack
        rng = np.random.default_rng(bits + N + K)
        q = pack.random_planes(N, K, bits, seed=bits * 17 + N)
        _layers[("narrow", bits, N, K)] = (q, np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1))
    return _layers[("narrow", bits, N, K)]


def _narrow_x(S, K):
    if ("narrow", S, K) not in _xs:
        _xs[("narrow", S, K)] = np.random.default_rng(S + K).normal(0, 1, (S, K)).astype(np.float16)
    return _xs[("narrow", S, K)]


def _x(S, K):
    if (S, K) not in _xs:
        rng = np.random.default_rng(S * 31 + K)
        _xs[(S, K)] = (rng.normal(0, 1, (S, K)) * np.where(rng.random((S, K)) < 0.02, 20.0, 1.0)).astype(np.float16)
    return _xs[(S, K)]


def gemm_guarded(X, q, lut, bits, ws):
    """ws False: gq_anyprec_gemm; True: gq_anyprec_gemm_ws with exactly gq_anyprec_gemm_ws_bytes bytes (possibly none: a zero-length
    payload between its guards).  Returns (out, workspace bytes)."""
    from guidedquant_amd import _lib
    L = _lib.lib()
    S, K = X.shape
    N = q.shape[1]
    g = guarded.Guards()
    xb, qb, lb = g.inp("x", X), g.inp("qweight", q), g.inp("lut", lut)
    out = g.out("out", 2 * S * N)
    nb = 0
    if ws:
        nb = int(L.gq_anyprec_gemm_ws_bytes(S, N, K, bits))
        wb = g.out("workspace", nb)
        rc = L.gq_anyprec_gemm_ws(xb.ptr(), out.ptr(), qb.ptr(), lb.ptr(), S, N, K, bits, wb.ptr(), nb, _lib.current_stream_ptr())
    else:
        rc = L.gq_anyprec_gemm(xb.ptr(), out.ptr(), qb.ptr(), lb.ptr(), S, N, K, bits, _lib.current_stream_ptr())
    _lib.check(rc, "gq_anyprec_gemm")
    g.check()
    return out.numpy(np.float16, (S, N)), nb


def _split_close(split, one):
    """the bound of test_ap_gemm_gpu.test_gemm_split_k_on_short_grids"""
    diff = np.abs(split.astype(np.float32) - one.astype(np.float32))
    assert (diff <= 2.0**-10 * np.abs(split.astype(np.float32)) + 1e-4).all()


@pytest.mark.parametrize("shape", [None, 0, 14, 24, 18])
@pytest.mark.parametrize("bits", [2, 3, 4, 5, 6, 7, 8])
def test_guarded_gemm_every_tile_shape(oracle, bits, shape):
    """shape None: the dispatcher's own choice, which plans a K split for these short grids at K = 2304 (2..4 bits); a number:
    GQ_GEMM_SHAPE forces the tile (no split is planned then: the workspace is empty and must stay untouched)"""
    if shape is not None:
        _set(GQ_GEMM_SHAPE=shape)
    for K in KS:
        for N in NS:
            q, lut = _layer(oracle, bits, N, K)
            for S in SS:
                X = _x(S, K)
                one, _ = gemm_guarded(X, q, lut, bits, ws=False)
                _check(one, X, q, lut, bits, oracle)
                got, nb = gemm_guarded(X, q, lut, bits, ws=True)
                assert (nb > 0) == (shape is None and bits <= 4 and K == 2304), (nb, S, N, K)
                if nb:
                    assert nb == 2 * S * N * 4   # (9 groups of 256 weights: at most 2 ranges of >= 1024)
                    _check(got, X, q, lut, bits, oracle)
                else:
                    assert np.array_equal(got.view(np.uint16), one.view(np.uint16))


@pytest.mark.parametrize("kshape", [14, 18])
@pytest.mark.parametrize("ksplit", [2, 3, 5])
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_guarded_gemm_forced_uneven_splits(oracle, bits, ksplit, kshape):
    """GQ_GEMM_KSPLIT x GQ_GEMM_KSHAPE.  The planner caps the range count at (K / 256) / 4 and evens the ranges out: K = 2304 gives
    2 ranges (5 + 4 groups) whatever is asked, K = 4352 gives 2 (9 + 8), 3 (6 + 6 + 5) and, asked for 5, 4 ranges (5 + 5 + 5 + 2).  The workspace holds exactly that many
    S x N planes, every one of them is written (the poison would surface in the sum) and nothing behind them is."""
    expect = {2304: {2: 2, 3: 2, 5: 2}, 4352: {2: 2, 3: 3, 5: 4}}
    for K in (2304, 4352):
        for N in NS:
            q, lut = _narrow_layer(bits, N, K)
            for S in SS:
                X = _narrow_x(S, K)
                _set(GQ_GEMM_KSPLIT=ksplit, GQ_GEMM_KSHAPE=kshape)
                got, nb = gemm_guarded(X, q, lut, bits, ws=True)
                assert nb == expect[K][ksplit] * S * N * 4, (nb, S, N, K)
                _check(got, X, q, lut, bits, oracle)
                _set(GQ_GEMM_KSPLIT=1)
                one, nb1 = gemm_guarded(X, q, lut, bits, ws=True)
                assert nb1 == 0
                _check(one, X, q, lut, bits, oracle)
                _split_close(got, one)


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_guarded_gemm_planned_split_against_single_pass(oracle, bits):
    """the planner's own split of these short grids (K = 2304: two ranges; K = 4352: up to four) against the single pass"""
    from guidedquant_amd import _lib
    for K in (2304, 4352):
        for N in NS:
            q, lut = _narrow_layer(bits, N, K)
            for S in SS:
                X = _narrow_x(S, K)
                assert _lib.lib().gq_anyprec_gemm_ws_bytes(S, N, K, bits) >= 2 * S * N * 4
                got, nb = gemm_guarded(X, q, lut, bits, ws=True)
                one, _ = gemm_guarded(X, q, lut, bits, ws=False)
                _check(got, X, q, lut, bits, oracle)
                _split_close(got, one)
