"""GPU: the QTIP prompt path -- gq_qtip_decompress bit for bit against the reference's decode_compressed goldens and the
oracle, gq_qtip_gemm against the float64 product of the oracle's decode (the matvec's bound, test_qtip_gpu.py), against
gq_qtip_matvec row by row, split-K against the single pass, and the bs > 8 route of QuantizedLinear.forward."""
import numpy as np
import pytest

from conftest import golden_files

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

D = "cuda:0"


def _recipe(R, M, K, seed=42):
    """the reference kernel test's recipe (qtip/qtip-kernels/test_decompress_matvec.py:251-305)"""
    torch.manual_seed(seed)
    comp = torch.randint(torch.iinfo(torch.int32).min, torch.iinfo(torch.int32).max, (R * M * K // 32, ), dtype=torch.int32)
    tlut = torch.clamp(torch.randn(512, 2) / 16, -1, 1).to(torch.float16)
    return comp.numpy(), tlut.numpy()


def _x(S, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.clamp(torch.randn(S, K, generator=g) / 16, -1, 1).to(torch.float16).numpy()


def _gemm(comp, tlut, x, M, R, ws=True):
    from guidedquant_amd import _lib
    S, K = x.shape
    c = torch.from_numpy(np.ascontiguousarray(comp)).to(D)
    t = torch.from_numpy(np.ascontiguousarray(tlut)).to(D)
    xx = torch.from_numpy(np.ascontiguousarray(x)).to(D)
    out = torch.full((S, M), float("nan"), dtype=torch.float32, device=D)
    L = _lib.lib()
    nb = L.gq_qtip_gemm_ws_bytes(S, M, K, R) if ws else 0
    w = torch.empty(max(nb // 4, 4), dtype=torch.float32, device=D)
    rc = L.gq_qtip_gemm_ws(out.data_ptr(), c.data_ptr(), xx.data_ptr(), t.data_ptr(), S, M, K, R, w.data_ptr() if nb else None, nb,
                           _lib.current_stream_ptr())
    _lib.check(rc, "gq_qtip_gemm_ws")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bound(W, x):
    Wd, xd = W.astype(np.float64), x.astype(np.float64)
    return Wd @ xd.T, np.abs(Wd) @ np.abs(xd).T


@pytest.mark.parametrize("path", golden_files("qtip_R"))
def test_decompress_goldens_bit_exact(path):
    from guidedquant_amd.qtip import decompress
    g = np.load(path)
    R, m, k = int(g["R"]), int(g["m"]), int(g["k"])
    W = decompress(torch.from_numpy(g["compressed"]).to(D), torch.from_numpy(g["tlut"]).to(D), m, k, R).cpu().numpy()
    assert np.array_equal(W.view(np.uint16), g["W"].view(np.uint16))


@pytest.mark.parametrize("R", [2, 3, 4])
@pytest.mark.parametrize("M,K", [(4096, 4096), (11008, 4096), (4096, 11008)])
def test_decompress_reference_recipe_bit_exact(oracle, R, M, K):
    from guidedquant_amd.qtip import decompress
    comp, tlut = _recipe(R, M, K)
    W = decompress(torch.from_numpy(comp).to(D), torch.from_numpy(tlut).to(D), M, K, R).cpu().numpy()
    assert np.array_equal(W.view(np.uint16), oracle.qtip_decode(comp, tlut, M, K, R).view(np.uint16))


@pytest.mark.parametrize("R", [2, 3, 4])
@pytest.mark.parametrize("M,K", [(64, 96), (256, 256), (4096, 4096), (11008, 4096), (4096, 11008)])
def test_gemm_against_float64(oracle, R, M, K):
    comp, tlut = _recipe(R, M, K)
    W = oracle.qtip_decode(comp, tlut, M, K, R)
    for S in (1, 9, 16, 17, 100, 128, 513):
        if M * K > 4096 * 4096 and S not in (17, 128, 513):
            continue  # (the large shapes: one short, one full and one ragged token tile)
        x = _x(S, K, seed=S)
        got = _gemm(comp, tlut, x, M, R)
        ref, scale = _bound(W, x)
        err = np.abs(got.astype(np.float64) - ref.T)
        assert (err <= 2e-6 * scale.T + 1e-7).all(), (S, float((err / (scale.T + 1e-30)).max()))


@pytest.mark.parametrize("R", [2, 3, 4])
def test_gemm_rows_equal_the_matvec(oracle, R):
    from guidedquant_amd.qtip import qtip_kernels
    M, K, S = 4096, 4096, 17
    comp, tlut = _recipe(R, M, K, seed=7)
    x = _x(S, K, seed=3)
    got = _gemm(comp, tlut, x, M, R)
    W = oracle.qtip_decode(comp, tlut, M, K, R)
    _, scale = _bound(W, x)
    c, t = torch.from_numpy(comp).to(D), torch.from_numpy(tlut).reshape(-1).to(D)
    fn = getattr(qtip_kernels, f"decompress_matvec_16_9_{R}_1_{M}_1_{K}")
    for s in range(S):
        out = torch.zeros((M, 1), dtype=torch.float32, device=D)
        fn(out, c, torch.from_numpy(x[s].reshape(K, 1)).to(D), t)
        mv = out.cpu().numpy()[:, 0].astype(np.float64)
        assert (np.abs(got[s].astype(np.float64) - mv) <= 2 * 2e-6 * scale[:, s] + 2e-7).all(), s


@pytest.mark.parametrize("R", [2, 4])
def test_gemm_split_k_and_determinism(oracle, R):
    from guidedquant_amd import _lib
    M, K, S = 4096, 4096, 128
    assert _lib.lib().gq_qtip_gemm_ws_bytes(S, M, K, R) > 0  # a short grid: the split is planned
    comp, tlut = _recipe(R, M, K, seed=11)
    x = _x(S, K, seed=5)
    split = _gemm(comp, tlut, x, M, R, ws=True)
    single = _gemm(comp, tlut, x, M, R, ws=False)
    W = oracle.qtip_decode(comp, tlut, M, K, R)
    _, scale = _bound(W, x)
    assert (np.abs(split.astype(np.float64) - single) <= 2 * 2e-6 * scale.T + 2e-7).all()
    assert np.array_equal(split.view(np.uint32), _gemm(comp, tlut, x, M, R, ws=True).view(np.uint32))
    assert np.array_equal(single.view(np.uint32), _gemm(comp, tlut, x, M, R, ws=False).view(np.uint32))


def _linear(R, N=512, K=256, seed=0):
    from guidedquant_amd.qtip import QuantizedLinear
    rng = np.random.default_rng(seed + R)
    lin = QuantizedLinear(K, N, 16, 16, 16, R, 2, 9, 'quantlut_sym', device=D)
    trellis = rng.integers(-2**15, 2**15, lin.trellis.shape, dtype=np.int64).astype(np.int16)
    tlut = np.clip(rng.normal(0, 1 / 16, (512, 2)), -1, 1).astype(np.float16)
    SU = np.sign(rng.normal(0, 1, K)).astype(np.float16)
    SV = (np.sign(rng.normal(0, 1, N)) * rng.uniform(0.5, 1.5, N)).astype(np.float32)
    lin.load_state_dict({"trellis": torch.from_numpy(trellis), "tlut": torch.from_numpy(tlut), "SU": torch.from_numpy(SU),
                         "SV": torch.from_numpy(SV), "rcp": torch.tensor(0), "tp_rank": torch.tensor(8)})
    return lin, trellis, tlut, SU, SV


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("S", [9, 64])
def test_quantized_linear_batched_against_oracle_chain(oracle, R, S):
    """the oracle chain of test_qtip_gpu.py::test_quantized_linear_forward, row by row"""
    N, K = 512, 256
    lin, trellis, tlut, SU, SV = _linear(R, N, K)
    x = np.random.default_rng(100 + S).normal(0, 1, (1, S, K)).astype(np.float16)
    with torch.no_grad():
        y = lin(torch.from_numpy(x).to(D)).float().cpu().numpy().reshape(S, N)
    W = oracle.qtip_decode(trellis.view(np.int32).reshape(-1), tlut, N, K, R).astype(np.float64)
    for s in range(S):
        xs = x[0, s].astype(np.float64) * SU.astype(np.float64)
        xh = oracle.matmul_hadU(xs.astype(np.float32)[None], None, transpose=True)[0].astype(np.float64) / 32
        z = W @ xh.astype(np.float16).astype(np.float64)
        zh = oracle.matmul_hadU(z.astype(np.float32)[None], None)[0].astype(np.float64)
        ref = zh * (SV.astype(np.float64) * 32)
        assert np.abs(y[s] - ref).max() <= 2e-3 * np.abs(ref).max() + 1e-4, s


@pytest.mark.parametrize("R", [2, 4])
def test_quantized_linear_routes(monkeypatch, R):
    lin, *_ = _linear(R, seed=1)
    rng = np.random.default_rng(9)
    with torch.no_grad():
        for S in (2, 8):  # bs <= 8: today's row loop, whatever GQ_QTIP_GEMM says
            x = torch.from_numpy(rng.normal(0, 1, (1, S, 256)).astype(np.float16)).to(D)
            monkeypatch.setenv("GQ_QTIP_GEMM", "1")
            a = lin(x)
            monkeypatch.setenv("GQ_QTIP_GEMM", "0")
            assert torch.equal(a, lin(x))
        for S in (9, 40, 300):  # (300: the two-step form of the batched op)
            x = torch.from_numpy(rng.normal(0, 1, (1, S, 256)).astype(np.float16)).to(D)
            monkeypatch.setenv("GQ_QTIP_GEMM", "1")
            a = lin(x).float()
            monkeypatch.setenv("GQ_QTIP_GEMM", "0")
            b = lin(x).float()
            assert float((a - b).abs().max()) <= 2e-3 * float(b.abs().max()) + 1e-4


def test_quantized_linear_gemm_route_is_taken(monkeypatch):
    """bs > 8 launches quip_lib::qtip_gemm, not the per-row matvec ops"""
    from torch.profiler import profile, ProfilerActivity
    lin, *_ = _linear(2, seed=2)
    x = torch.zeros((1, 12, 256), dtype=torch.float16, device=D)
    monkeypatch.setenv("GQ_QTIP_GEMM", "1")
    with torch.no_grad(), profile(activities=[ProfilerActivity.CPU]) as p:
        lin(x)
    names = [e.name for e in p.events()]
    assert any("quip_lib::qtip_gemm" in n for n in names)
    assert not any("decompress_matvec_qtip" in n for n in names)


def test_opcheck_qtip_gemm():
    from torch.library import opcheck
    import guidedquant_amd.qtip  # noqa: F401  (registers the op)
    M, K, R = 256, 256, 3
    comp, tlut = _recipe(R, M, K)
    x = torch.from_numpy(_x(24, K, seed=1)).to(D)
    opcheck(torch.ops.quip_lib.qtip_gemm.default, (torch.from_numpy(comp).to(D), x, torch.from_numpy(tlut).to(D), M, R))


def test_compile_fullgraph_qtip_gemm():
    M, K, R = 256, 256, 2
    comp, tlut = _recipe(R, M, K)
    c, t = torch.from_numpy(comp).to(D), torch.from_numpy(tlut).to(D)
    x = torch.from_numpy(_x(16, K, seed=2)).to(D)

    def f(c, x, t):
        return torch.ops.quip_lib.qtip_gemm(c, x, t, M, R) * 2

    want = f(c, x, t)
    got = torch.compile(f, fullgraph=True, backend="eager")(c, x, t)
    assert torch.equal(got, want)


def test_qtip_gemm_two_step_rows(oracle):
    """from GQ_QTIP_TWO_STEP_S rows on the batched op decodes to a dense W and runs one matmul with an fp32 output"""
    M, K, R, S = 512, 1024, 3, 300
    comp, tlut = _recipe(R, M, K, seed=5)
    x = _x(S, K, seed=6)
    got = torch.ops.quip_lib.qtip_gemm(torch.from_numpy(comp).to(D), torch.from_numpy(x).to(D), torch.from_numpy(tlut).to(D), M, R)
    assert got.dtype == torch.float32 and got.shape == (S, M)
    ref, scale = _bound(oracle.qtip_decode(comp, tlut, M, K, R), x)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref.T)
    assert (err <= 1e-5 * scale.T + 1e-7).all(), float((err / (scale.T + 1e-30)).max())


def _prefill_model(monkeypatch, tmp_path, inter):
    from guidedquant_amd import model as gm, qtip
    from guidedquant_amd.generate import load_model
    if inter == 11008:  # (the factor width of Llama-2-7b's MLP: the caller's table, as test_qtip_native_decode_with_factor_width)
        import os
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "had_n11008.npz"))
        np.savez(tmp_path / "tables.npz", had172=g["hadK"])
        monkeypatch.setenv("GQ_HADAMARD_TABLES", str(tmp_path / "tables.npz"))
    qtip._tables = None
    gm.transformer_configs["qtip-prefill-test"] = dict(model_name="llama-qtip-prefill-test", block_size=128, vocab_size=512, n_layer=2,
                                                       n_head=8, dim=1024, intermediate_size=inter, n_local_heads=8)
    try:
        torch.manual_seed(0)
        m = load_model("qtip-prefill-test", D, "qtip", 2, random_init=True)
    finally:
        del gm.transformer_configs["qtip-prefill-test"]
        qtip._tables = None
    with torch.device(D):
        m.setup_caches(max_batch_size=1, max_seq_length=64)
    return m


@pytest.mark.parametrize("inter", [2048, 11008])
def test_prefill_native_qtip_then_native_decode(monkeypatch, tmp_path, inter):
    m = _prefill_model(monkeypatch, tmp_path, inter)
    assert m._native_kind() == "qtip"
    S = 24
    g = torch.Generator().manual_seed(inter)
    idx = torch.randint(0, 512, (1, S), generator=g, dtype=torch.int32).to(D)
    pos = torch.arange(S, dtype=torch.int32, device=D)
    assert m.prefill_ready(idx)
    nxt = [5, 99, 311]

    def caches():
        return [(b.attention.kv_cache.k_cache[:, :, :S].clone(), b.attention.kv_cache.v_cache[:, :, :S].clone()) for b in m.layers]

    with torch.no_grad():
        ref = m(idx, pos).float()[0, -1]
        ref_kv = caches()
        ref_dec = [m(torch.tensor([[t]], dtype=torch.int32, device=D), torch.tensor([S + i], dtype=torch.int32, device=D)).float().reshape(-1)
                   for i, t in enumerate(nxt)]
        for b in m.layers:
            b.attention.kv_cache.k_cache.zero_()
            b.attention.kv_cache.v_cache.zero_()
        got = m.prefill_native(idx, pos, start=0, last_only=True).float().reshape(-1)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got).all())
        assert float((got - ref).abs().max()) <= 2e-2 * float(ref.abs().max())
        assert int(got.argmax()) == int(ref.argmax())
        for (k0, v0), (k1, v1) in zip(ref_kv, caches()):
            assert torch.allclose(k1.float(), k0.float(), rtol=1e-2, atol=1e-2)
            assert torch.allclose(v1.float(), v0.float(), rtol=1e-2, atol=1e-2)
        for i, t in enumerate(nxt):
            out = m.decode_native(torch.tensor([t], dtype=torch.int32, device=D), torch.tensor([S + i], dtype=torch.int32, device=D)).float().reshape(-1)
            torch.cuda.synchronize()
            err = float((out - ref_dec[i]).abs().max()) / (float(ref_dec[i].abs().max()) + 1e-9)
            assert err < 2e-2, (i, err)


def test_generate_prefill_takes_the_native_pass_for_qtip(monkeypatch, tmp_path):
    from guidedquant_amd import generate
    m = _prefill_model(monkeypatch, tmp_path, 2048)
    idx = torch.arange(1, 17, dtype=torch.int32, device=D).reshape(1, -1)
    pos = torch.arange(16, dtype=torch.int32, device=D)
    calls = []
    orig = m.prefill_native
    monkeypatch.setattr(m, "prefill_native", lambda *a, **k: calls.append(1) or orig(*a, **k))
    with torch.no_grad():
        generate.prefill(m, idx, pos, temperature=1.0, top_k=1)
    assert calls == [1]
