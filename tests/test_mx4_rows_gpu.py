"""GPU: gq_rope_cache_rows_mx4 (csrc/prefill.hip) on guard-banded buffers against the numpy model tests/mx4_model.py applied to what the fp16
entry (gq_rope_cache_rows / gq_qknorm_rope_cache_rows) leaves in an fp16 cache: q_out, codes and exponent bytes byte-equal, every other byte
of the poisoned caches untouched.  The v rows carry the edge blocks of test_mx4_host_cpu.py (ties, 6 * 2^e and a step above, zeros,
subnormals, 49152, 65504, NaN, Inf); positions 0, max_seq - 1 and one >= max_seq, which is not written."""
import numpy as np
import pytest

import mx4_model as mx
from test_mx4_host_cpu import BLOCKS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from guarded import Guards, ptr  # noqa: E402

MAX_SEQ, EPS, H, HKV, FILL, FILL_EXP = 24, 1e-6, 4, 2, 0x5A, 0x33
POSITIONS = {1: [[0], [MAX_SEQ - 1], [MAX_SEQ + 5]], 5: [[0, MAX_SEQ + 5, 7, MAX_SEQ - 1, 8]]}


@pytest.mark.parametrize("form", ["plain", "qknorm", "bias"])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("S", [1, 5])
def test_rows_against_the_fp16_entry_and_the_numpy_model(S, hd, form):
    from guidedquant_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(100 * S + hd)
    W, nb = (H + 2 * HKV) * hd, hd // 32
    col = torch.ones(W)
    col[3::7], col[5::11] = 600.0, 2.0**-11
    blocks = list(BLOCKS.values())
    frq = 1.0 / (500000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    emb = torch.outer(torch.arange(MAX_SEQ, dtype=torch.float32), frq).repeat(1, 2)
    cos, sin = emb.cos().half(), emb.sin().half()
    qw = kw = bias = None
    if form == "qknorm":
        qw, kw = (0.5 + torch.rand(hd, generator=g)).half(), ((0.5 + torch.rand(hd, generator=g)) * col[:hd]).half()
    if form == "bias":
        bias = (torch.randn(W, generator=g) * 0.5 * col).half()
        bias[(H + HKV) * hd:] = 0  # (the edge blocks of the v rows stay what they are)
    for li, pos in enumerate(POSITIONS[S]):
        qkv = (torch.randn(S, W, generator=g) * col).half()
        first = 16 * (S == 1) + 4 * li  # (the S = 5 launch takes the blocks from 0 on in its written rows, the S = 1 launches the rest)
        for i, s in enumerate(s for s in range(S) if pos[s] < MAX_SEQ or S == 1):
            for kvh in range(HKV):
                v = np.concatenate([blocks[(first + (i * HKV + kvh) * nb + j) % len(blocks)] for j in range(nb)])
                qkv[s, (H + HKV + kvh) * hd:(H + HKV + kvh + 1) * hd] = torch.from_numpy(v)
        posd = torch.tensor(pos, dtype=torch.int32)
        written = [p for p in pos if p < MAX_SEQ]
        shape = (S, H, HKV, hd, MAX_SEQ)
        # ---- the fp16 entry
        g16 = Guards()
        b = [g16.inp(n, t) for n, t in (("qkv", (qkv + bias) if form == "bias" else qkv), ("pos", posd), ("cos", cos), ("sin", sin))]
        q16, kc16, vc16 = g16.out("q", H * S * hd * 2), g16.out("kc", HKV * MAX_SEQ * hd * 2), g16.out("vc", HKV * MAX_SEQ * hd * 2)
        if form == "qknorm":
            rc = L.gq_qknorm_rope_cache_rows(*[x.ptr() for x in b], q16.ptr(), kc16.ptr(), vc16.ptr(), *shape, g16.inp("qw", qw).ptr(), g16.inp("kw", kw).ptr(), EPS, None)
        else:
            rc = L.gq_rope_cache_rows(*[x.ptr() for x in b], q16.ptr(), kc16.ptr(), vc16.ptr(), *shape, None)
        _lib.check(rc, "fp16 entry")
        g16.check()
        # ---- the MXFP4 entry over poisoned caches
        g4 = Guards()
        c = [g4.inp(n, t) for n, t in (("qkv", qkv), ("pos", posd), ("cos", cos), ("sin", sin))]
        fill, fille = np.full((HKV, MAX_SEQ, hd // 2), FILL, dtype=np.uint8), np.full((HKV, MAX_SEQ, nb), FILL_EXP, dtype=np.uint8)
        kc4, vc4, ke4, ve4 = g4.inp("kc", fill), g4.inp("vc", fill), g4.inp("k_exp", fille), g4.inp("v_exp", fille)
        q4 = g4.out("q", H * S * hd * 2)
        rc = L.gq_rope_cache_rows_mx4(*[x.ptr() for x in c], q4.ptr(), kc4.ptr(), vc4.ptr(), ke4.ptr(), ve4.ptr(), *shape, ptr(g4.inp("qw", qw)), ptr(g4.inp("kw", kw)),
                                      EPS, ptr(g4.inp("bias", bias)), None)
        _lib.check(rc, "gq_rope_cache_rows_mx4")
        g4.check()
        assert np.array_equal(q4.numpy(np.uint16), q16.numpy(np.uint16)), "q_out differs from the fp16 entry's"
        for name, got, gote, ref16 in (("k", kc4, ke4, kc16), ("v", vc4, ve4, vc16)):
            want, wante = fill.copy(), fille.copy()
            if written:
                want[:, written], wante[:, written] = mx.quantize(ref16.numpy(np.float16, (HKV, MAX_SEQ, hd))[:, written])
            gote, got = gote.numpy(np.uint8, wante.shape), got.numpy(np.uint8, want.shape)
            assert np.array_equal(gote, wante), "%s exponents at %r: first difference at %r" % (name, pos, np.argwhere(gote != wante)[0].tolist())
            assert np.array_equal(got, want), "%s codes at %r: %d byte(s) differ, first at %r" % (name, pos, int((got != want).sum()), np.argwhere(got != want)[0].tolist())
        assert S != 5 or (wante == 0xFF).any(), "the NaN and Inf blocks are in the S = 5 launch"


def test_other_head_dims_are_declined_and_write_nothing():
    from guidedquant_amd import _lib
    L = _lib.lib()
    g = Guards()
    z = [g.inp(n, torch.zeros(8 * 96, dtype=torch.float16)) for n in ("qkv", "cos", "sin")]
    pos = g.inp("pos", torch.zeros(1, dtype=torch.int32))
    outs = [g.out(n, 4 * 96 * 2) for n in ("q", "kc", "vc", "ke", "ve")]
    rc = L.gq_rope_cache_rows_mx4(z[0].ptr(), pos.ptr(), z[1].ptr(), z[2].ptr(), *[o.ptr() for o in outs], 1, 4, 2, 96, 8, None, None, EPS, None, None)
    g.check()
    assert rc == _lib.GQ_ENOTSUP and all(bool((o.view(torch.uint8) == 0x7E).all()) for o in outs)
