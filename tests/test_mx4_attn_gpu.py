"""GPU: gq_attn_decode_roped_mx4 (csrc/decode.hip) and gq_attn_prefill_mx4 (csrc/prefill_attn.hip) on guard-banded buffers.  Every
e2m1(code) * 2^e with e in -15 .. 13 is an fp16 value, so a launch equals gq_attn_decode_roped / _window (gq_attn_prefill) on an fp16 cache
that holds the dequantised values (tests/mx4_model.py) BIT FOR BIT.  Codes are random bytes, exponent bytes random per block over 112 .. 140
(a byte taken from another block, row or head shows); rows no query may read hold 0xff codes and 0xff / 0x8c bytes (NaN, -49152).  Contexts: 1, either
side of one pass and of two passes (the solo rule), a few passes; n_split 1, 2, 3 and 8 (splits behind the context; the grouped-head
instance where the group is 4); no window, one inside the context, one beyond the cache."""
import numpy as np
import pytest

import mx4_model as mx

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes as ap  # noqa: E402
import test_kv8_attn_gpu as t8  # noqa: E402
from guarded import Guards  # noqa: E402

HEADS = [(8, 2, 64), (4, 2, 64), (8, 2, 128), (4, 4, 128)]  # (n_head, n_kv_head, head_dim): groups of 4, 2, 4, 1
IDS = ["H%d-Hkv%d-hd%d" % h for h in HEADS]
PREFILL_CASES = [(65, 0, 0), (70, 59, 0), (64, 64, 24)]  # (S, start, window): a tile boundary, a ragged last tile, a window


def _cache(Hkv, n, hd, seed, lo, hi):
    """(codes uint8 [Hkv, n, hd / 2], exponent bytes uint8 [Hkv, n, hd / 32]) random in the rows [lo, hi), stale outside"""
    rng = np.random.default_rng(seed)
    codes, exps = rng.integers(0, 256, (Hkv, n, hd // 2), dtype=np.uint8), rng.integers(112, 141, (Hkv, n, hd // 32), dtype=np.uint8)
    stale = (np.arange(n) < lo) | (np.arange(n) >= hi)
    codes[:, stale], exps[:, stale] = 0xFF, np.where(np.arange(n) % 2 == 0, 0xFF, 0x8C).astype(np.uint8)[None, stale, None]
    return codes, exps


def _f16(codes, exps):
    v = mx.dequant(codes, exps)
    assert np.array_equal(v.astype(np.float16).astype(np.float64), v, equal_nan=True)  # (exact in fp16)
    return torch.from_numpy(v.astype(np.float16)).to(t8._dev())


def _decode(L, _lib, q, K, V, pos, H, Hkv, hd, ns, window):
    g = Guards()
    b = [g.inp(n, t) for n, t in (("q", q), ("pos", torch.tensor([pos], dtype=torch.int32)), ("kc", K[0]), ("vc", V[0]), ("ke", K[1]), ("ve", V[1]))]
    out, ws = g.out("out", H * hd * 2), (g.out("ws", H * ns * (hd + 2) * 4) if ns > 1 else None)
    rc = L.gq_attn_decode_roped_mx4(*[x.ptr() for x in b], out.ptr(), H, Hkv, hd, K[0].shape[1], ap.default_scale(hd), ns, ws.ptr() if ws is not None else None,
                                    window, _lib.current_stream_ptr())
    g.check()
    _lib.check(rc, "gq_attn_decode_roped_mx4")
    return out.view(torch.float16, (H, hd)).clone()


def _same(got, want, what):
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), "%s: NaN in %d / %d elements" % (what, int(gn.sum()), int(wn.sum()))
    bad = (t8._bits(got) != t8._bits(want)) & ~wn
    assert not bool(bad.any()), "%s: %d element(s) differ, worst %d fp16 steps" % (what, int(bad.sum()), int(ap.ulp_distance(got[~wn], want[~wn]).max()))


@pytest.mark.parametrize("H,Hkv,hd", HEADS, ids=IDS)
def test_decode_launch_equals_the_fp16_launch_bit_for_bit(H, Hkv, hd):
    from guidedquant_amd import _lib
    L = _lib.lib()
    P = t8._pass(hd)
    max_seq = 4 * P + 16
    q = (t8._q(H, hd).float() * 2.0**-8).half()  # (scores of a few units against K values up to 49152: many rows keep a weight)
    for window in (0, P + 3, max_seq + 7):
        for ns in (1, 2, 3, 8):
            for pos in (0, P - 2, P - 1, P, 2 * P - 1, 2 * P, 4 * P + 5, max_seq - 1):
                lo = t8._lo(pos, window)
                K, V = _cache(Hkv, max_seq, hd, 1, lo, pos + 1), _cache(Hkv, max_seq, hd, 2, lo, pos + 1)
                got = _decode(L, _lib, q, K, V, pos, H, Hkv, hd, ns, window)
                want = t8._decode16(L, _lib, q.to(t8._dev()), _f16(*K), _f16(*V), pos, H, Hkv, hd, ns, window)
                assert torch.isfinite(want.float()).all(), (window, ns, pos)
                _same(got, want, "window %d n_split %d pos %d" % (window, ns, pos))


@pytest.mark.parametrize("which", ["k", "v"])
@pytest.mark.parametrize("H,Hkv,hd", HEADS[1:3], ids=IDS[1:3])
def test_a_block_with_the_byte_ff_reads_back_as_nan_on_both_sides(H, Hkv, hd, which):
    from guidedquant_amd import _lib
    L = _lib.lib()
    pos, max_seq, ns = 70, 80, 1
    K, V = _cache(Hkv, max_seq, hd, 3, 0, pos + 1), _cache(Hkv, max_seq, hd, 4, 0, pos + 1)
    (K if which == "k" else V)[1][1, 37, hd // 32 - 1] = 0xFF  # (KV head 1, row 37, the last block)
    got = _decode(L, _lib, t8._q(H, hd), K, V, pos, H, Hkv, hd, ns, 0)
    want = t8._decode16(L, _lib, t8._q(H, hd).to(t8._dev()), _f16(*K), _f16(*V), pos, H, Hkv, hd, ns, 0)
    _same(got, want, which)
    nan = torch.isnan(got).cpu()
    expect = torch.zeros(H, hd, dtype=torch.bool)
    expect[H // Hkv:, (hd - 32 if which == "v" else 0):] = True  # (k: the scores of the group's heads; v: the block's outputs of them)
    assert torch.equal(nan, expect)


def test_decode_past_the_cache_gives_nan():
    from guidedquant_amd import _lib
    H, Hkv, hd = HEADS[0]
    K, V = _cache(Hkv, 40, hd, 5, 0, 40), _cache(Hkv, 40, hd, 6, 0, 40)
    for ns in (1, 3):
        got = _decode(_lib.lib(), _lib, t8._q(H, hd), K, V, 40, H, Hkv, hd, ns, 0)
        assert bool((t8._bits(got) == 0x7E00).all())


@pytest.mark.parametrize("S,start,window", PREFILL_CASES, ids=["S%d-start%d-W%d" % c for c in PREFILL_CASES])
@pytest.mark.parametrize("H,Hkv,hd", HEADS[1:], ids=IDS[1:])
def test_prefill_launch_equals_the_fp16_launch_bit_for_bit(H, Hkv, hd, S, start, window):
    from guidedquant_amd import _lib
    L = _lib.lib()
    T = start + S
    q = (torch.randn(H, S, hd, generator=torch.Generator().manual_seed(S + start)) * 2.0**-12).half()
    K, V = _cache(Hkv, T + 3, hd, 7, 0, T), _cache(Hkv, T + 3, hd, 8, 0, T)
    g = Guards()
    b = [g.inp(n, t) for n, t in (("q", q), ("kc", K[0]), ("vc", V[0]), ("ke", K[1]), ("ve", V[1]))]
    bo = g.out("out", S * H * hd * 2)
    rc = L.gq_attn_prefill_mx4(*[x.ptr() for x in b], bo.ptr(), S, start, H, Hkv, hd, T + 3, ap.default_scale(hd), window, None)
    g.check()
    _lib.check(rc, "gq_attn_prefill_mx4")
    want = t8._prefill16(L, _lib, q, _f16(*K), _f16(*V), S, start, H, Hkv, hd, window)
    assert torch.isfinite(want.float()).all()
    _same(bo.view(torch.float16, (S, H * hd)).clone(), want, "prefill")
