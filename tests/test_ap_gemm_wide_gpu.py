"""GPU parity: the fused-dequant prefill GEMM at 5 to 8 bits (csrc/ap_gemm_wide.hip behind gq_anyprec_gemm) against the oracle's
dequantised matrix times x in float64.  The arithmetic is that of the 2..4-bit kernel whatever the width -- fp32 accumulation over all
of K, one fp16 rounding -- so the tolerance is the one of tests/test_ap_gemm_gpu.py::_check:
    |got - exact| <= 2^-11 * 1.001 * |exact| + 1e-5 * sum|x||w| + 1e-7."""
import os

import numpy as np
import pytest

from conftest import golden_files

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WIDE = [5, 6, 7, 8]


def _gemm(x, q, lut, bits):
    from guidedquant_amd import ap_gemv
    d = torch.device("cuda:0")
    out = ap_gemv.anyprec_gemm(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float16)).to(d), torch.from_numpy(np.ascontiguousarray(q)).to(d),
                               torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float16)).to(d), bits)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_w(got, x, W):
    W = np.asarray(W).astype(np.float64)
    X = np.asarray(x, dtype=np.float16).astype(np.float64)
    ref = X @ W.T
    scale = np.abs(X) @ np.abs(W).T
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got.astype(np.float32)).all()
    assert (err <= 2.0**-11 * 1.001 * np.abs(ref) + 1e-5 * scale + 1e-7).all(), (err / (scale + 1e-30)).max()


def _check(got, x, q, lut, bits, oracle, rows=None):
    if rows is not None:
        q, lut, got = np.ascontiguousarray(q[:, rows, :]), lut[rows], got[:, rows]
    _check_w(got, x, oracle.ap_dequant(np.ascontiguousarray(q[:bits]), lut, bits))


def _random_case(oracle, rng, bits, N, K, S):
    """the recipe of tests/test_ap_gemm_gpu.py::test_gemm_random: per-row LUT scales 10^(-3..0), 2 % of the activations x 20"""
    codes = rng.integers(0, 1 << bits, (N, K), dtype=np.uint8)
    q = oracle.ap_pack(codes, bits)
    lut = (rng.normal(0, 1, (N, 1 << bits)) * 10.0**rng.integers(-3, 1, (N, 1))).astype(np.float16)
    X = (rng.normal(0, 1, (S, K)) * np.where(rng.random((S, K)) < 0.02, 20.0, 1.0)).astype(np.float16)
    return q, lut, X


# one-hot positions at N = 70, K = 1088 (a whole chunk: byte lane c holds the weights 256 c .. 256 c + 255; a 64-weight tail chunk:
# byte lane c holds 1024 + 16 c .. + 15): first and last weight of every byte lane of both chunks, the chunk boundary, word and byte
# boundaries inside a lane, the last weight of the row
_ONE_HOT = [0, 255, 256, 511, 512, 767, 768, 1023, 1024, 1039, 1040, 1055, 1056, 1071, 1072, 1087,
            1, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 129, 254, 257, 300, 510, 513, 700, 766, 769, 1000, 1022, 1025, 1086]


@pytest.mark.parametrize("bits", WIDE)
def test_decode_is_exact(oracle, bits):
    """lut[n][c] = c and one-hot tokens: out[s][n] IS the code of weight k_s of row n -- plane order, MSB-first bit order, byte-lane
    and word addressing and the table lookup, with no tolerance"""
    N, K, S = 70, 1088, 40
    assert len(_ONE_HOT) == S == len(set(_ONE_HOT))
    rng = np.random.default_rng(bits)
    codes = rng.integers(0, 1 << bits, (N, K), dtype=np.uint8)
    assert len(np.unique(codes)) == 1 << bits
    q = oracle.ap_pack(codes, bits)
    lut = np.tile(np.arange(1 << bits, dtype=np.float16), (N, 1))
    X = np.zeros((S, K), dtype=np.float16)
    X[np.arange(S), _ONE_HOT] = 1.0
    got = _gemm(X, q, lut, bits)
    assert got.shape == (S, N)
    assert np.array_equal(got.astype(np.int32), codes[:, _ONE_HOT].T.astype(np.int32))


def _golden_cases(oracle, bits):
    """(qweight, lut, W, x) of every reference-generated fixture of this width the kernel serves (K % 64 == 0); a width without one
    gets the same kind of case from the oracle's packer (W = lut[codes])"""
    cases = []
    for p in golden_files("ap_b"):
        g = np.load(p)
        if int(g["bits"]) == bits and (g["qweight"].shape[2] * 32) % 64 == 0:
            cases.append((g["qweight"], g["lut"], g["W"], g["x"].reshape(1, -1)))
    if not cases:
        rng = np.random.default_rng(100 + bits)
        N, K = 4, {5: 1088, 7: 4160, 8: 2112}.get(bits, 2048)
        codes = rng.integers(0, 1 << bits, (N, K), dtype=np.uint8)
        lut = np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1)
        cases.append((oracle.ap_pack(codes, bits), lut, np.take_along_axis(lut, codes.astype(np.int64), axis=1), rng.normal(0, 1, (1, K)).astype(np.float16)))
    return cases


@pytest.mark.parametrize("bits", WIDE)
def test_gemm_goldens(oracle, bits):
    cases = _golden_cases(oracle, bits)
    assert len(cases) >= 1
    for q, lut, W, x in cases:
        K = q.shape[2] * 32
        rng = np.random.default_rng(1)
        X = np.concatenate([x.astype(np.float16), rng.normal(0, 1, (6, K)).astype(np.float16)])
        _check_w(_gemm(X, q, lut, bits), X, W)


@pytest.mark.parametrize("bits", WIDE)
@pytest.mark.parametrize("N,K,S", [(36, 64, 3), (200, 1088, 33), (130, 2048, 129), (64, 11008, 77), (100, 1984, 260)])
def test_gemm_tails(oracle, bits, N, K, S):
    """row / token / K tails: N not a multiple of 128 (or 4), S not a multiple of 128, tail chunks of 64 .. 960 weights"""
    q, lut, X = _random_case(oracle, np.random.default_rng(bits * 977 + N + K + S), bits, N, K, S)
    _check(_gemm(X, q, lut, bits), X, q, lut, bits, oracle)


@pytest.mark.parametrize("bits", [5, 8])
@pytest.mark.parametrize("N,K,S", [(6144, 4096, 512), (4096, 14336, 130)])
def test_gemm_model_width_sampled_rows(oracle, bits, N, K, S):
    from guidedquant_amd import pack
    rng = np.random.default_rng(bits + N + K)
    q = pack.random_planes(N, K, bits, seed=bits * 31 + N)
    lut = np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1)
    X = rng.normal(0, 1, (S, K)).astype(np.float16)
    got = _gemm(X, q, lut, bits)
    rows = np.unique(np.concatenate([np.arange(0, 40), np.arange(N - 40, N), rng.integers(0, N, 64)]))
    _check(got, X, q, lut, bits, oracle, rows=rows)


@pytest.mark.parametrize("bits", WIDE)
def test_no_split_and_one_tile_shape_at_wide_bits(oracle, bits):
    """5..8 bits have one tile shape and no K split: no workspace is planned (short grids included), GQ_GEMM_SHAPE changes nothing,
    and the workspace entry point given a buffer anyway computes the single pass"""
    from guidedquant_amd import _lib
    L = _lib.lib()
    for S, N, K in [(128, 4096, 4096), (100, 4096, 14336), (33, 1000, 2048), (512, 6144, 4096), (130, 96, 768)]:
        assert L.gq_anyprec_gemm_ws_bytes(S, N, K, bits) == 0
    N, K, S = 96, 768, 130
    q, lut, X = _random_case(oracle, np.random.default_rng(bits * 131 + N), bits, N, K, S)
    base = _gemm(X, q, lut, bits)
    _check(base, X, q, lut, bits, oracle)
    d = torch.device("cuda:0")
    xt, qt, lt = (torch.from_numpy(np.ascontiguousarray(a)).to(d) for a in (X, q, lut))
    out, ws = torch.empty(S, N, dtype=torch.float16, device=d), torch.empty(4 * S * N * 4, dtype=torch.uint8, device=d)
    _lib.check(L.gq_anyprec_gemm_ws(xt.data_ptr(), out.data_ptr(), qt.data_ptr(), lt.data_ptr(), S, N, K, bits, ws.data_ptr(), ws.numel(), None), "gq_anyprec_gemm_ws")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), base.view(np.uint16))
    os.environ["GQ_GEMM_SHAPE"] = "18"
    L.gq_reset_env_cache()
    try:
        forced = _gemm(X, q, lut, bits)
    finally:
        os.environ.pop("GQ_GEMM_SHAPE", None)
        L.gq_reset_env_cache()
    assert np.array_equal(forced.view(np.uint16), base.view(np.uint16))


def test_gemm_is_deterministic_and_row_independent(oracle):
    from guidedquant_amd import pack
    bits, N, K = 7, 1024, 4096
    rng = np.random.default_rng(5)
    q = pack.random_planes(N, K, bits, seed=9)
    lut = np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1)
    X = rng.normal(0, 1, (200, K)).astype(np.float16)
    a, b = _gemm(X, q, lut, bits), _gemm(X, q, lut, bits)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    c = _gemm(X[37:150], q, lut, bits)
    assert np.array_equal(a[37:150].view(np.uint16), c.view(np.uint16))


def _under(mode, fn):
    prev = os.environ.get("GQ_PREFILL_FUSED")
    os.environ["GQ_PREFILL_FUSED"] = mode
    try:
        return fn()
    finally:
        if prev is None:
            del os.environ["GQ_PREFILL_FUSED"]
        else:
            os.environ["GQ_PREFILL_FUSED"] = prev


def test_aplinear_takes_the_fused_gemm_at_6_bits(oracle, monkeypatch):
    from guidedquant_amd import ap_gemv
    from guidedquant_amd.APLinear import APLinear
    d = torch.device("cuda:0")
    bits, N, K = 6, 512, 2048
    rng = np.random.default_rng(2)
    codes = rng.integers(0, 1 << bits, (N, K), dtype=np.uint8)
    q, lut = oracle.ap_pack(codes, bits), rng.normal(0, 0.03, (N, 1 << bits)).astype(np.float16)
    lin = APLinear(K, N, bits, device=d)
    lin.load_state_dict({"qweight": torch.from_numpy(q), "lut": torch.from_numpy(lut)})
    xs = torch.from_numpy(rng.normal(0, 1, (1, 70, K)).astype(np.float16)).to(d)
    calls, real = [], ap_gemv.anyprec_gemm
    monkeypatch.setattr(ap_gemv, "anyprec_gemm", lambda *a: (calls.append(a[3]), real(*a))[1])
    y = _under("1", lambda: lin(xs))
    assert calls == [bits]
    assert tuple(y.shape) == (1, 70, N) and y.dtype == torch.float16
    _check(y.cpu().numpy()[0], xs.cpu().numpy()[0], q, lut, bits, oracle)
    y0 = _under("0", lambda: lin(xs))
    assert calls == [bits]  # (the two steps)
    assert float((y.float() - y0.float()).abs().max()) <= 2e-2 * float(y0.float().abs().max())


@pytest.mark.parametrize("precision", [5, 8])
def test_anyprecision_linear_takes_the_fused_gemm(oracle, precision):
    """an 8-bit parent served at precision p: the first p planes and lut{p}"""
    from guidedquant_amd.AnyPrecisionLinear import AnyPrecisionLinear
    d = torch.device("cuda:0")
    N, K, supported = 512, 2048, [4, 5, 6, 7, 8]
    rng = np.random.default_rng(precision)
    codes = rng.integers(0, 256, (N, K), dtype=np.uint8)
    q = oracle.ap_pack(codes, 8)
    luts = {b: rng.normal(0, 0.03, (N, 1 << b)).astype(np.float16) for b in supported}
    lin = AnyPrecisionLinear(K, N, supported, bias=False, device=d, dtype=torch.float16)
    lin.load_state_dict({"qweight": torch.from_numpy(q), **{f"lut{b}": torch.from_numpy(luts[b]) for b in supported}})
    xs = torch.from_numpy(rng.normal(0, 1, (1, 70, K)).astype(np.float16)).to(d)
    y = _under("1", lambda: lin(xs, precision=precision))
    assert tuple(y.shape) == (1, 70, N) and y.dtype == torch.float16
    _check(y.cpu().numpy()[0], xs.cpu().numpy()[0], q, luts[precision], precision, oracle)
    y0 = _under("0", lambda: lin(xs, precision=precision))
    assert float((y.float() - y0.float()).abs().max()) <= 2e-2 * float(y0.float().abs().max())


@pytest.mark.parametrize("precision", [5, 8])
def test_prompt_pass_of_an_8_bit_parent(precision):
    """prefill_native of the fused decoder at precision 5 / 8: every linear through the fused GEMM against every linear through
    dequantise + matmul -- the bounds tests/test_prefill_native_gpu.py puts on two prompt passes that differ in summation order"""
    pytest.importorskip("transformers")
    from test_decode_wide_gpu import _parent8_model
    d = torch.device("cuda:0")
    m = _parent8_model(seed=5, D=256, I=512, H=4, KV=2, V=512, Lr=2)
    dec = m.native_decoder(precision)
    assert dec.layers[0].attention.wqkv.bitwidth == precision
    S = 24
    dec.setup_caches(1, S + 8)
    assert dec.native_ready()
    g = torch.Generator(device=d).manual_seed(precision)
    idx = torch.randint(0, dec.config.vocab_size, (1, S), dtype=torch.int32, device=d, generator=g)
    pos = torch.arange(S, dtype=torch.int32, device=d)
    assert dec.prefill_ready(idx)
    with torch.no_grad():
        fused = _under("1", lambda: dec.prefill_native(idx, pos, start=0, last_only=False).float().clone())
        steps = _under("0", lambda: dec.prefill_native(idx, pos, start=0, last_only=False).float().clone())
    torch.cuda.synchronize()
    assert torch.isfinite(fused).all()
    scale = steps.abs().max().item()
    assert (fused - steps).abs().max().item() <= 1e-2 * scale, ((fused - steps).abs().max().item(), scale)
    assert ((fused - steps).norm() / steps.norm()).item() <= 3e-3
    assert int(fused[0, -1].argmax()) == int(steps[0, -1].argmax())
