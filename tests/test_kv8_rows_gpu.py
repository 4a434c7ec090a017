"""GPU: the row write of the fp8 KV cache (csrc/prefill.hip, gq_rope_cache_rows_kv8) through the C ABI on guard-banded buffers
(tests/guarded.py), pinned to the fp16 entries:

  q_out        bit-equal to gq_rope_cache_rows / gq_qknorm_rope_cache_rows (the bias form: gq_rope_cache_rows on rows the bias was added
               to in fp16)
  cache bytes  at the written rows EQUAL the host model of the write rule (kv8_model.quantize) applied to the rows the fp16 entry
               wrote; every other byte of the caches still holds the 0x7f they were filled with; the guard bands hold.
Inputs carry columns scaled by 600 (values that clamp at 448 * scale) and by 2^-11 (values that land below 2^-9 and flush or take the
subnormal codes).  S in {1, 3, 17} at max_seq 40 with positions 0, max_seq - 1 and one >= max_seq (not written) in the launch."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import kv8_model as k8  # noqa: E402
from guarded import Guards  # noqa: E402

MAX_SEQ = 40
EPS = 1e-6


def _L():
    from guidedquant_amd import _lib
    return _lib


def _tables(hd):
    inv = 1.0 / (500000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    fr = torch.outer(torch.arange(MAX_SEQ, dtype=torch.float32), inv)
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().half().contiguous(), emb.sin().half().contiguous()


def _positions(S):
    """the launches of a case: lists of S distinct positions that together hold 0, max_seq - 1 and one >= max_seq"""
    if S == 1:
        return [[0], [MAX_SEQ - 1], [MAX_SEQ + 2]]
    fill = [p for p in range(3, MAX_SEQ - 1, 2)][:S - 3]
    return [[0, MAX_SEQ + 5, MAX_SEQ - 1] + fill]


def _inputs(S, H, Hkv, hd, form, seed):
    g = torch.Generator().manual_seed(seed)
    W = (H + 2 * Hkv) * hd
    col = torch.ones(W)
    col[3::7] = 600.0      # clamps (|x| * inv beyond 448 at both scale sets)
    col[5::11] = 2.0**-11  # below 2^-9
    qkv = (torch.randn(S, W, generator=g) * col).half()
    qw = kw = bias = None
    if form == "qknorm":   # (the norm makes every head unit-size: the magnitudes come back through the weights)
        wcol = torch.ones(hd)
        wcol[3::7], wcol[5::11] = 600.0, 2.0**-11
        qw = (0.5 + torch.rand(hd, generator=g)).half()
        kw = ((0.5 + torch.rand(hd, generator=g)) * wcol).half()
    if form == "bias":
        bias = (torch.randn(W, generator=g) * 0.5 * col).half()  # (of the size of its column: the small columns stay small)
    return qkv, qw, kw, bias


@pytest.mark.parametrize("scales", ["ones", "free"])
@pytest.mark.parametrize("form", ["plain", "qknorm", "bias"])
@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=["H%d-Hkv%d-hd%d" % h for h in k8.HEADS])
@pytest.mark.parametrize("S", [1, 3, 17])
def test_rows_against_the_fp16_entry_and_the_write_rule(S, H, Hkv, hd, form, scales):
    _lib = _L()
    L = _lib.lib()
    cos, sin = _tables(hd)
    if scales == "ones":
        ks, vs = torch.ones(Hkv), torch.ones(Hkv)
    else:  # no powers of two, different per head
        ks = torch.tensor([0.37, 2.9, 1.3, 0.051][:Hkv])
        vs = torch.tensor([2.9, 0.37, 0.77, 5.3][:Hkv])
    k_inv, v_inv = torch.reciprocal(ks), torch.reciprocal(vs)
    qkv, qw, kw, bias = _inputs(S, H, Hkv, hd, form, 100 * S + hd + H)
    clamped = flushed = 0
    for pos in _positions(S):
        posd = torch.tensor(pos, dtype=torch.int32)
        # ---- the fp16 entry (caches and q_out poisoned: 0x7e7e is a NaN)
        g16 = Guards()
        rows16 = (qkv + bias) if form == "bias" else qkv  # (one fp16 add per element)
        b = dict(qkv=g16.inp("qkv", rows16), pos=g16.inp("pos", posd), cos=g16.inp("cos", cos), sin=g16.inp("sin", sin),
                 qw=g16.inp("qw", qw), kw=g16.inp("kw", kw))
        q16, kc16, vc16 = g16.out("q", H * S * hd * 2), g16.out("kc", Hkv * MAX_SEQ * hd * 2), g16.out("vc", Hkv * MAX_SEQ * hd * 2)
        if form == "qknorm":
            rc = L.gq_qknorm_rope_cache_rows(b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q16.ptr(), kc16.ptr(), vc16.ptr(), S, H, Hkv, hd,
                                             MAX_SEQ, b["qw"].ptr(), b["kw"].ptr(), EPS, None)
        else:
            rc = L.gq_rope_cache_rows(b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q16.ptr(), kc16.ptr(), vc16.ptr(), S, H, Hkv, hd, MAX_SEQ, None)
        _lib.check(rc, "fp16 entry")
        g16.check()
        # ---- the fp8 entry (caches filled with 0x7f)
        g8 = Guards()
        c = dict(qkv=g8.inp("qkv", qkv), pos=g8.inp("pos", posd), cos=g8.inp("cos", cos), sin=g8.inp("sin", sin), qw=g8.inp("qw", qw),
                 kw=g8.inp("kw", kw), bias=g8.inp("bias", bias), k_inv=g8.inp("k_inv", k_inv), v_inv=g8.inp("v_inv", v_inv))
        fill = torch.full((Hkv, MAX_SEQ, hd), k8.NAN_CODE, dtype=torch.uint8)
        kc8, vc8 = g8.inp("kc", fill), g8.inp("vc", fill)
        q8 = g8.out("q", H * S * hd * 2)
        opt = lambda x: None if x is None else x.ptr()  # noqa: E731
        rc = L.gq_rope_cache_rows_kv8(c["qkv"].ptr(), c["pos"].ptr(), c["cos"].ptr(), c["sin"].ptr(), q8.ptr(), kc8.ptr(), vc8.ptr(), c["k_inv"].ptr(),
                                      c["v_inv"].ptr(), S, H, Hkv, hd, MAX_SEQ, opt(c["qw"]), opt(c["kw"]), EPS, opt(c["bias"]), None)
        _lib.check(rc, "gq_rope_cache_rows_kv8")
        g8.check()
        assert torch.equal(q8.view(torch.int16).cpu(), q16.view(torch.int16).cpu()), "q_out differs from the fp16 entry's"
        written = sorted(p for p in pos if p < MAX_SEQ)
        for name, got, ref16, inv in (("k", kc8, kc16, k_inv), ("v", vc8, vc16, v_inv)):
            got = got.view(torch.uint8, (Hkv, MAX_SEQ, hd)).cpu()
            ref = ref16.view(torch.float16, (Hkv, MAX_SEQ, hd)).cpu()[:, written]
            assert torch.isfinite(ref.float()).all()
            want = fill.clone()
            want[:, written] = k8.quantize(ref, inv[:, None, None])
            bad = got != want
            assert not bool(bad.any()), "%s cache: %d byte(s) differ, first at %r" % (name, int(bad.sum()), torch.nonzero(bad)[0].tolist())
            mag = (ref.float() * inv[:, None, None]).abs()
            clamped += int((mag > 448.0).sum())
            flushed += int(((mag < 2.0**-9) & (mag > 0)).sum())
    assert clamped > 0 and flushed > 0, (clamped, flushed)  # (the case exercises the clamp and the codes below 2^-9)


def test_argument_checks_write_nothing():
    _lib = _L()
    L = _lib.lib()
    H, Hkv, S = 4, 2, 2
    for hd, qw, bias, want in ((96, False, False, _lib.GQ_ENOTSUP), (32, False, False, _lib.GQ_ENOTSUP), (64, True, True, _lib.GQ_EINVAL)):
        g = Guards()
        W = (H + 2 * Hkv) * hd
        cos = torch.ones(MAX_SEQ, hd, dtype=torch.float16)
        b = dict(qkv=g.inp("qkv", torch.ones(S, W, dtype=torch.float16)), pos=g.inp("pos", torch.tensor([0, 1], dtype=torch.int32)), cos=g.inp("cos", cos),
                 sin=g.inp("sin", cos), inv=g.inp("inv", torch.ones(Hkv)), w=g.inp("w", torch.ones(hd, dtype=torch.float16)),
                 bias=g.inp("bias", torch.ones(W, dtype=torch.float16)))
        q, kc, vc = g.out("q", H * S * hd * 2), g.out("kc", Hkv * MAX_SEQ * hd), g.out("vc", Hkv * MAX_SEQ * hd)
        rc = L.gq_rope_cache_rows_kv8(b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q.ptr(), kc.ptr(), vc.ptr(), b["inv"].ptr(), b["inv"].ptr(),
                                      S, H, Hkv, hd, MAX_SEQ, b["w"].ptr() if qw else None, b["w"].ptr() if qw else None, EPS,
                                      b["bias"].ptr() if bias else None, None)
        g.check()
        assert rc == want, (hd, rc)
        for o in (q, kc, vc):
            assert bool((o.view(torch.uint8) == 0x7E).all())  # the poison pattern, untouched
