"""GPU: gq_attn_decode_roped_kv8r (csrc/decode.hip) and gq_attn_prefill_kv8r (csrc/prefill_attn.hip) on guard-banded buffers, with the caches,
positions, windows and fp16 launches of test_kv8_attn_gpu.py.  fp16(code) * 2^e is an fp16 value, so a launch equals the fp16 launch on a
cache holding code * 2^e BIT FOR BIT; the exponent bytes are drawn per (KV head, row) over 112 .. 134, rows no query may read hold 0xff / 0x00.
Count probe: K = 0, V one-hot (code of 1.0) with e = -15 + (5 t + 3 g) % 23 in row t: a byte taken from another row or head shows."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes as ap  # noqa: E402
import kv8_model as k8  # noqa: E402
import test_kv8_attn_gpu as t8  # noqa: E402
from guarded import Guards  # noqa: E402


def _exps(Hkv, n, seed, lo=0, hi=None):
    """exponent bytes uint8 [Hkv, n], random over 112 .. 134 in the rows [lo, hi), 0xff / 0x00 alternating outside (never read)"""
    e = torch.randint(112, 135, (Hkv, n), generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(torch.uint8)
    stale = torch.tensor([0xFF, 0x00], dtype=torch.uint8)[torch.arange(n) % 2].expand(Hkv, n)
    t = torch.arange(n)
    return torch.where((t >= lo) & (t < (n if hi is None else hi)), e, stale)


def _f16(codes, exps):
    """the fp16 cache that holds code * 2^e (rows with a stale byte: the scale 1.0 -- no query reads them in either launch)"""
    from guidedquant_amd.model import fp8_row_scale
    e = torch.where((exps >= 112) & (exps <= 134), exps, torch.full_like(exps, 127))
    v = k8.TABLE[codes.long()] * fp8_row_scale(e)[..., None]
    assert torch.equal(v.half().float().nan_to_num(), v.nan_to_num())
    return v.half().to(t8._dev())


def _decode(L, _lib, q, Kc, Vc, Ke, Ve, pos, H, Hkv, hd, ns, window):
    g = Guards()
    b = [g.inp(n, t) for n, t in (("q", q), ("pos", torch.tensor([pos], dtype=torch.int32)), ("kc", Kc), ("vc", Vc), ("ke", Ke), ("ve", Ve))]
    out, ws = g.out("out", H * hd * 2), (g.out("ws", H * ns * (hd + 2) * 4) if ns > 1 else None)
    rc = L.gq_attn_decode_roped_kv8r(*[x.ptr() for x in b], out.ptr(), H, Hkv, hd, Kc.shape[1], ap.default_scale(hd), ns, ws.ptr() if ws is not None else None,
                                     window, _lib.current_stream_ptr())
    g.check()
    _lib.check(rc, "gq_attn_decode_roped_kv8r")
    return out.view(torch.float16, (H, hd)).clone()


@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=t8.HEADS_IDS)
def test_decode_launch_equals_the_fp16_launch_bit_for_bit(H, Hkv, hd):
    from guidedquant_amd import _lib
    L = _lib.lib()
    q = (t8._q(H, hd).float() * 2.0**-8).half()  # (scores of a few units against K values up to 57344: every attended row keeps a weight)
    n = 0
    for window in t8._windows(hd)[:3]:
        for ns in t8.SPLITS:
            for pos in t8._positions(hd, ns):
                lo = t8._lo(pos, window)
                Kc, Vc = t8._with_stale(t8._codes(Hkv, hd, "k", 0x7E), lo, pos), t8._with_stale(t8._codes(Hkv, hd, "v", 0x7E), lo, pos)
                Ke, Ve = _exps(Hkv, Kc.shape[1], 1, lo, pos + 1), _exps(Hkv, Kc.shape[1], 2, lo, pos + 1)
                got = _decode(L, _lib, q, Kc, Vc, Ke, Ve, pos, H, Hkv, hd, ns, window)
                want = t8._decode16(L, _lib, q.to(t8._dev()), _f16(Kc, Ke), _f16(Vc, Ve), pos, H, Hkv, hd, ns, window)
                assert torch.isfinite(want.float()).all(), (window, ns, pos)
                assert torch.equal(t8._bits(got), t8._bits(want)), "window %d n_split %d pos %d: %d element(s) differ, worst %d fp16 steps" % (
                    window, ns, pos, int((t8._bits(got) != t8._bits(want)).sum()), int(ap.ulp_distance(got, want).max()))
                n += 1
    print("H%d/%d hd%d: %d launches bit-identical" % (H, Hkv, hd, n))


@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=t8.HEADS_IDS)
def test_decode_count_probe_every_row_with_its_own_exponent(H, Hkv, hd):
    from guidedquant_amd import _lib
    L = _lib.lib()
    max_seq = t8._max_seq(hd)
    e = -15 + (5 * torch.arange(max_seq)[None, :] + 3 * torch.arange(Hkv)[:, None]) % 23  # [Hkv, max_seq]
    for window in (0, t8._pass(hd) + 3):
        for ns in t8.SPLITS:
            for pos in t8._positions(hd, ns):
                lo = t8._lo(pos, window)
                p = ap.count_probe(H, Hkv, hd, pos, max_seq)
                Vc = t8._with_stale(torch.where(p.V == 1.0, k8.ONE_CODE, 0).to(torch.uint8), lo, pos)
                Kc = t8._with_stale(torch.zeros_like(Vc), lo, pos)
                t = torch.arange(max_seq)
                Ve = torch.where((t >= lo) & (t <= pos), (e + 127).to(torch.uint8), _exps(Hkv, max_seq, 0, 0, 0))
                got = _decode(L, _lib, p.q, Kc, Vc, _exps(Hkv, max_seq, 3, lo, pos + 1), Ve, pos, H, Hkv, hd, ns, window)
                mean = (p.V.double() * torch.exp2(e.double())[..., None])[:, lo:pos + 1].sum(1) / (pos + 1 - lo)
                want = mean.repeat_interleave(H // Hkv, dim=0).half()
                d = ap.ulp_distance(got.cpu(), want)
                assert int(d.max()) <= 1, (window, ns, pos, int(d.argmax()), int(d.max()))


def _prefill(L, _lib, q, Kc, Vc, Ke, Ve, S, start, H, Hkv, hd, window):
    g = Guards()
    b = [g.inp(n, t) for n, t in (("q", q), ("kc", Kc), ("vc", Vc), ("ke", Ke), ("ve", Ve))]
    bo = g.out("out", S * H * hd * 2)
    rc = L.gq_attn_prefill_kv8r(*[x.ptr() for x in b], bo.ptr(), S, start, H, Hkv, hd, Kc.shape[1], ap.default_scale(hd), window, None)
    g.check()
    _lib.check(rc, "gq_attn_prefill_kv8r")
    return bo.view(torch.float16, (S, H * hd)).clone()


@pytest.mark.parametrize("S,start,window", t8.PREFILL_CASES, ids=["S%d-start%d-W%d" % c for c in t8.PREFILL_CASES])
@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=t8.HEADS_IDS)
def test_prefill_launch_equals_the_fp16_launch_bit_for_bit(H, Hkv, hd, S, start, window):
    from guidedquant_amd import _lib
    L = _lib.lib()
    q = (torch.randn(H, S, hd, generator=torch.Generator().manual_seed(S + start)) * 2.0**-12).half()
    Kc, Vc = t8._prefill_caches(Hkv, hd, S, start, window)
    Ke, Ve = _exps(Hkv, Kc.shape[1], 4, 0, start + S), _exps(Hkv, Kc.shape[1], 5, 0, start + S)
    got = _prefill(L, _lib, q, Kc, Vc, Ke, Ve, S, start, H, Hkv, hd, window)
    want = t8._prefill16(L, _lib, q, _f16(Kc, Ke), _f16(Vc, Ve), S, start, H, Hkv, hd, window)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(t8._bits(got), t8._bits(want)), "%d element(s) differ, worst %d fp16 steps" % (int((t8._bits(got) != t8._bits(want)).sum()),
                                                                                                    int(ap.ulp_distance(got, want).max()))
