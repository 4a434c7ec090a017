"""GPU: the remaining entries with every buffer guard-banded and poisoned (tests/guarded.py): the LUT-GEMM GEMV (both entries, both
block sizes of the workspace form), the device packer and dequantiser, the embedding lookup and the statistics kernels, and one
split and one roped decode attention launch with guards around `out` and the split workspace as well.  Every result against the
checker the entry already has: bit identity with the oracle (LUT-GEMM, packer, dequantiser), equality with the table row, the
sum-of-squares check of tests/test_handover_gpu.py, the count probe of tests/attn_probes.py.  Guards: exact equality."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes as ap  # noqa: E402
import guarded  # noqa: E402


def _L():
    from guidedquant_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _env():
    yield
    os.environ.pop("GQ_LG_SMALL_BLOCKS", None)
    _L().lib().gq_reset_env_cache()


@pytest.mark.parametrize("small", [None, 0])   # GQ_LG_SMALL_BLOCKS: the default (16 outputs per block for these N) / 0 (the wide block)
@pytest.mark.parametrize("bits", [1, 4, 8])
def test_guarded_lutgemm(oracle, bits, small):
    """gq_lutgemm_gemv and gq_lutgemm_gemv_ws (workspace of exactly 64 * K bytes, poisoned): out is ACCUMULATED INTO, so it starts as
    zeros between its guards"""
    L = _L()
    if small is not None:
        os.environ["GQ_LG_SMALL_BLOCKS"] = str(small)
    L.lib().gq_reset_env_cache()
    for N in (17, 300):
        for K in (32, 544):
            for gs in (32, K):
                rng = np.random.default_rng(bits * 100 + N + K + gs)
                q = rng.integers(-2**31, 2**31, (K // 32, bits, N), dtype=np.int64).astype(np.int32)
                alpha = (rng.random((K // gs, bits, N)) * 0.01).astype(np.float16)
                qb = rng.normal(0, 0.01, (K // gs, N)).astype(np.float16)
                x = rng.normal(0, 1, K).astype(np.float16)
                want = oracle.lutgemm_f16(x, q, alpha, qb, bits, gs)
                for ws in (False, True):
                    g = guarded.Guards()
                    xb, qwb, ab, bb = g.inp("x", x), g.inp("qweight", q), g.inp("alpha", alpha), g.inp("q_bias", qb)
                    ob = g.inp("out", np.zeros(N, np.float16))
                    if ws:
                        wb = g.out("workspace", 64 * K)
                        rc = L.lib().gq_lutgemm_gemv_ws(xb.ptr(), ob.ptr(), qwb.ptr(), ab.ptr(), bb.ptr(), N, K, bits, gs, wb.ptr(), 64 * K,
                                                        L.current_stream_ptr())
                    else:
                        rc = L.lib().gq_lutgemm_gemv(xb.ptr(), ob.ptr(), qwb.ptr(), ab.ptr(), bb.ptr(), N, K, bits, gs, L.current_stream_ptr())
                    L.check(rc, "gq_lutgemm_gemv")
                    g.check()
                    assert np.array_equal(ob.numpy(np.uint16), want.view(np.uint16)), (N, K, gs, ws)


@pytest.mark.parametrize("bits", [2, 3, 4, 5, 6, 7, 8])
def test_guarded_pack_and_dequant(oracle, bits):
    L = _L()
    N = 5
    for K in (96, 1056):
        rng = np.random.default_rng(bits + K)
        codes = rng.integers(0, 1 << bits, (N, K), dtype=np.uint8)
        lut = rng.normal(0, 1, (N, 1 << bits)).astype(np.float16)
        q = oracle.ap_pack(codes, bits)
        g = guarded.Guards()
        cb, lb = g.inp("codes", codes), g.inp("lut", lut)
        qb = g.out("qweight", 4 * bits * N * (K // 32))
        L.check(L.lib().gq_anyprec_pack(cb.ptr(), qb.ptr(), N, K, bits, L.current_stream_ptr()), "gq_anyprec_pack")
        wb = g.out("W", 2 * N * K)
        L.check(L.lib().gq_anyprec_dequant(qb.ptr(), lb.ptr(), wb.ptr(), N, K, bits, L.current_stream_ptr()), "gq_anyprec_dequant")
        g.check()
        assert np.array_equal(qb.numpy(np.uint32, q.shape), q.view(np.uint32))
        assert np.array_equal(wb.numpy(np.uint16, (N, K)), oracle.ap_dequant(q, lut, bits).view(np.uint16))
        assert np.array_equal(wb.numpy(np.uint16, (N, K)), np.take_along_axis(lut, codes.astype(np.int64), axis=1).view(np.uint16))


def _check_ssq(values, ssq):
    """tests/test_handover_gpu.py: every slot written, their total the sum of squares"""
    want = (values.astype(np.float64)**2).sum()
    assert np.isfinite(ssq).all() and abs(ssq.astype(np.float64).sum() - want) <= 1e-5 * want


@pytest.mark.parametrize("dim", [8, 520])
def test_guarded_embed_lookup(dim):
    L = _L()
    V = 7
    table = np.random.default_rng(dim).normal(0, 1, (V, dim)).astype(np.float16)
    for tok in (0, V - 1):
        for ho in (False, True):
            g = guarded.Guards()
            tb, kb = g.inp("table", table), g.inp("token", np.array([tok], np.int32))
            ob = g.out("out", 2 * dim)
            if ho:
                sb = g.out("ssq_out", 4 * L.SSQ_SLOTS)
                rc = L.lib().gq_embed_lookup_ho(kb.ptr(), tb.ptr(), ob.ptr(), dim, V, sb.ptr(), L.current_stream_ptr())
            else:
                rc = L.lib().gq_embed_lookup(kb.ptr(), tb.ptr(), ob.ptr(), dim, V, L.current_stream_ptr())
            L.check(rc, "gq_embed_lookup")
            g.check()
            assert np.array_equal(ob.numpy(np.uint16), table[tok].view(np.uint16))
            if ho:
                _check_ssq(table[tok], sb.numpy(np.float32))


@pytest.mark.parametrize("n", [1, 8, 1000, 1025, 4100])
def test_guarded_ssq_rows(n):
    """fewer values than slots, one more than the slots, a ragged count of several rounds"""
    L = _L()
    x = np.random.default_rng(n).normal(0, 3, n).astype(np.float16)
    g = guarded.Guards()
    xb, sb = g.inp("x", x), g.out("ssq_out", 4 * L.SSQ_SLOTS)
    L.check(L.lib().gq_ssq_rows(xb.ptr(), n, sb.ptr(), L.current_stream_ptr()), "gq_ssq_rows")
    g.check()
    _check_ssq(x, sb.numpy(np.float32))


@pytest.mark.parametrize("form", ["split", "roped"])
@pytest.mark.parametrize("hd,pos,ns", [(64, 700, 3), (128, 300, 4), (64, 40, 1)])
def test_guarded_attention(form, hd, pos, ns):
    """the count probe (every cached row exactly once; stale rows behind the position hold NaN / Inf) with qkv / q, pos, the tables,
    both caches, out and the split workspace -- exactly [n_head][n_split][head_dim + 2] floats, poisoned -- between guards.  (64, 700, 3)
    and (128, 300, 4): more than two passes, so the splits and the combine run; (64, 40, 1): one block per head, no workspace."""
    L = _L()
    d = torch.device("cuda:0")
    H, Hkv = 4, 2
    max_seq, scale = pos + 5, ap.default_scale(hd)
    geo = ap.geometry(hd, pos, ns)
    assert geo.solo is False and geo.eff_split == ns
    cos = sin = None
    kw = {}
    if form == "split":
        from test_attn_probes_gpu import _rope_tables, _rots
        cos, sin = (t[:max_seq].contiguous() for t in _rope_tables(hd))
        rq, rk, _ = _rots(form, hd, pos)
        kw = dict(rot_q=rq, rot_k=rk)
    p = ap.count_probe(H, Hkv, hd, pos, max_seq, device=d, **kw)
    g = guarded.Guards()
    kc, vc = p.K.clone(), p.V.clone()
    if form == "split":   # the current row comes from the launch, not from the cache
        kc[:, pos] = float("nan")
        vc[:, pos] = float("nan")
    kb, vb, pb = g.inp("k_cache", kc), g.inp("v_cache", vc), g.inp("pos", torch.tensor([pos], dtype=torch.int32))
    ob = g.out("out", 2 * H * hd)
    wb = g.out("workspace", 4 * H * ns * (hd + 2)) if ns > 1 else None
    st = L.current_stream_ptr()
    if form == "roped":
        qb = g.inp("q", p.q.contiguous())
        rc = L.lib().gq_attn_decode_roped(qb.ptr(), pb.ptr(), kb.ptr(), vb.ptr(), ob.ptr(), H, Hkv, hd, max_seq, scale, ns, guarded.ptr(wb), st)
    else:
        qb = g.inp("qkv", torch.cat((p.q_in.reshape(-1), p.k_in.reshape(-1), p.v_in.reshape(-1))).contiguous())
        cb, sb = g.inp("cos", cos), g.inp("sin", sin)
        rc = L.lib().gq_attn_decode_split(qb.ptr(), pb.ptr(), cb.ptr(), sb.ptr(), kb.ptr(), vb.ptr(), ob.ptr(), H, Hkv, hd, max_seq, scale, ns,
                                          guarded.ptr(wb), st)
    L.check(rc, form)
    g.check()
    ap.check_exact(ob.view(torch.float16, (H, hd)), p)
    assert torch.equal(kb.view(torch.int16, p.K.shape), p.K.view(torch.int16)) and torch.equal(vb.view(torch.int16, p.V.shape), p.V.view(torch.int16))
