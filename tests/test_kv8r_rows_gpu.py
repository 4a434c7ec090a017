"""GPU: gq_rope_cache_rows_kv8r (csrc/prefill.hip) on guard-banded buffers: q_out bit-equal to the fp16 entries', codes and exponent bytes at
the written rows EQUAL to model.fp8_row_quantize of the rows the fp16 entry wrote (a NaN element: either NaN code), every other byte of the
caches and the exponent tensors untouched.  The v part carries the hand-picked rows of test_kv8r_host_cpu.py, the rest spans 2^-11 .. 600 by
column; S in {1, 3, 17} from position 5 at max_seq 40, one position >= max_seq (not written) where S > 1."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import kv8_model as k8  # noqa: E402
from guarded import Guards, ptr  # noqa: E402
from test_kv8r_host_cpu import ROWS  # noqa: E402

MAX_SEQ, START, EPS, FILL_EXP = 40, 5, 1e-6, 0x33


@pytest.mark.parametrize("form", ["plain", "qknorm", "bias"])
@pytest.mark.parametrize("H,Hkv,hd", k8.HEADS, ids=["H%d-Hkv%d-hd%d" % h for h in k8.HEADS])
@pytest.mark.parametrize("S", [1, 3, 17])
def test_rows_against_the_fp16_entry_and_the_host_model(S, H, Hkv, hd, form):
    from guidedquant_amd import _lib
    from guidedquant_amd.model import fp8_row_quantize, fp8_row_scale
    L = _lib.lib()
    g = torch.Generator().manual_seed(100 * S + hd + H)
    W = (H + 2 * Hkv) * hd
    col = torch.ones(W)
    col[3::7], col[5::11] = 600.0, 2.0**-11
    qkv = (torch.randn(S, W, generator=g) * col).half()
    names = list(ROWS)
    for i in range(S * Hkv):  # the hand-picked rows as v vectors, all of them over the S = 17 cases
        r = torch.cat([ROWS[names[(i * hd // 64 + j) % len(names)]] for j in range(hd // 64)])
        qkv[i // Hkv, (H + Hkv + i % Hkv) * hd:(H + Hkv + i % Hkv + 1) * hd] = r
    frq = 1.0 / (500000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    emb = torch.outer(torch.arange(MAX_SEQ, dtype=torch.float32), frq).repeat(1, 2)
    cos, sin = emb.cos().half(), emb.sin().half()
    qw = kw = bias = None
    if form == "qknorm":
        qw, kw = (0.5 + torch.rand(hd, generator=g)).half(), ((0.5 + torch.rand(hd, generator=g)) * col[:hd]).half()
    if form == "bias":
        bias = (torch.randn(W, generator=g) * 0.5 * col).half()
        bias[(H + Hkv) * hd:] = 0  # (the hand-picked v rows stay what they are)
    pos = list(range(START, START + S))
    if S > 1:
        pos[1] = MAX_SEQ + 5
    posd = torch.tensor(pos, dtype=torch.int32)
    written = [p for p in pos if p < MAX_SEQ]
    # ---- the fp16 entry
    g16 = Guards()
    b = [g16.inp(n, t) for n, t in (("qkv", (qkv + bias) if form == "bias" else qkv), ("pos", posd), ("cos", cos), ("sin", sin))]
    q16, kc16, vc16 = g16.out("q", H * S * hd * 2), g16.out("kc", Hkv * MAX_SEQ * hd * 2), g16.out("vc", Hkv * MAX_SEQ * hd * 2)
    shape = (S, H, Hkv, hd, MAX_SEQ)
    if form == "qknorm":
        rc = L.gq_qknorm_rope_cache_rows(*[x.ptr() for x in b], q16.ptr(), kc16.ptr(), vc16.ptr(), *shape, g16.inp("qw", qw).ptr(), g16.inp("kw", kw).ptr(), EPS, None)
    else:
        rc = L.gq_rope_cache_rows(*[x.ptr() for x in b], q16.ptr(), kc16.ptr(), vc16.ptr(), *shape, None)
    _lib.check(rc, "fp16 entry")
    g16.check()
    # ---- the per-row entry: caches filled with the NaN code, exponent tensors with a byte no row produces
    g8 = Guards()
    c = [g8.inp(n, t) for n, t in (("qkv", qkv), ("pos", posd), ("cos", cos), ("sin", sin))]
    fill, fille = torch.full((Hkv, MAX_SEQ, hd), k8.NAN_CODE, dtype=torch.uint8), torch.full((Hkv, MAX_SEQ), FILL_EXP, dtype=torch.uint8)
    kc8, vc8, ke8, ve8 = g8.inp("kc", fill), g8.inp("vc", fill), g8.inp("k_exp", fille), g8.inp("v_exp", fille)
    q8 = g8.out("q", H * S * hd * 2)
    rc = L.gq_rope_cache_rows_kv8r(*[x.ptr() for x in c], q8.ptr(), kc8.ptr(), vc8.ptr(), ke8.ptr(), ve8.ptr(), *shape, ptr(g8.inp("qw", qw)), ptr(g8.inp("kw", kw)),
                                   EPS, ptr(g8.inp("bias", bias)), None)
    _lib.check(rc, "gq_rope_cache_rows_kv8r")
    g8.check()
    assert torch.equal(q8.view(torch.int16).cpu(), q16.view(torch.int16).cpu()), "q_out differs from the fp16 entry's"
    for name, got, gote, ref16 in (("k", kc8, ke8, kc16), ("v", vc8, ve8, vc16)):
        ref = ref16.view(torch.float16, (Hkv, MAX_SEQ, hd)).cpu()[:, written]
        codes, byte = fp8_row_quantize(ref)
        want, wante = fill.clone(), fille.clone()
        want[:, written], wante[:, written] = codes, byte
        got, gote = got.view(torch.uint8, (Hkv, MAX_SEQ, hd)).cpu(), gote.view(torch.uint8, (Hkv, MAX_SEQ)).cpu()
        bade = gote != wante
        assert not bool(bade.any()), "%s exponents: %d differ, first at %r" % (name, int(bade.sum()), torch.nonzero(bade)[0].tolist())
        nan = torch.zeros_like(want, dtype=torch.bool)
        nan[:, written] = torch.isnan(ref)
        bad = torch.where(nan, (got & 0x7F) != k8.NAN_CODE, got != want)
        assert not bool(bad.any()), "%s codes: %d byte(s) differ, first at %r" % (name, int(bad.sum()), torch.nonzero(bad)[0].tolist())
        if name == "v":  # the saturation at 448 * 2^7: what the fp16 cache holds as 65504 reads 57344
            top = ref.float().abs() == 65504.0
            deq = k8.TABLE[codes.long()] * fp8_row_scale(byte)[..., None]
            assert (S < 17 or bool(top.any())) and bool((deq[top].abs() == 57344.0).all())

