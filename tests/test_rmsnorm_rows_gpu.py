"""GPU: every finite fp16 value through the RMSNorm sites that write their result element by element -- the prompt row kernel
(gq_rmsnorm_rows, with and without the residual add in front), the QK-norm of the prompt row writer (gq_qknorm_rope_cache_rows: q_out and
the written k rows) and the QK-norm of the decode attention (gq_attn_decode_split_qknorm: the k row it writes) -- against the candidate
sets of tests/rmsnorm_model.py: per element the one or two fp16 outputs the contract n = fp16(x * rs), out = fp16(n * w) admits when the
site's fp32 scale rs lies within the interval derived from its code (rmsnorm_model.SITES / grant).  Bit patterns are compared.

inputs     rmsnorm_model.banded / interleaved / gauss (the 63 488 finite patterns; Gaussians at 2^-12, 1, 2^10), weights without powers
           of two in +-[0.5, 2), eps 1e-5 and 1e-6.  Buffers are guard-banded (tests/guarded.py).
rows       D in {8, 520, 2048, 16384}; zeros compare with their sign (x * rs and n * w fix it).  With delta, x is overwritten by
           half_add(x, delta), bit for bit, and the norm is checked on that sum.
QK-norm    hd 64 and 128, banded and interleaved; the cos table is all ones and the sin table all zeros, so the rotation is
           x * 1 + (-+y) * 0 = x by value: +0 and -0 compare equal (the sum with the signed zero of the partner decides the sign), and so
           do they in the cache.  The decode kernel's normalised q feeds the scores only and is not observable element-wise:
           tests/test_qknorm_attn_gpu.py keeps covering it; here H = Hkv = 8 heads take 8 rows of the arrangement per launch.
The last test prints, per site: draws, outputs that were not the primary candidate, the multi-candidate share, subnormal and zero
outputs seen.  The interleaved runs must see both subnormals and zeros (asserted).

Measured on an MI355X -- no value outside its candidates (both eps, all arrangements and sizes together):
  site         draws      non-primary   two candidates   subnormal outputs   zero outputs   grant
  rows         3 029 344  93            0.57 %           357 731             126 332        2^-18.66
  qkn-rows     1 015 808  14            0.14 %           174 220             54 416         2^-20.29
  qkn-decode     507 904  20            0.08 %            86 340             27 208         2^-21.08
(a non-primary output is one whose fp32 scale rounded an fp16 tie the other way than fp32(scale64): the sites' sums run in their own order.)
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import halfsweep_model as hs  # noqa: E402
import rmsnorm_model as rm  # noqa: E402
from ap_helpers import half_add  # noqa: E402
from guarded import Guards  # noqa: E402

STATS = {}


def _L():
    from guidedquant_amd import _lib
    return _lib


def _record(site, arr, out, cand, zero_signs, what):
    """assert out within cand; add the tallies to STATS[site]; the interleaved runs must have seen subnormals and zeros"""
    ok, npri = hs.in_candidates(out, cand, zero_signs=zero_signs)
    bad = np.argwhere(~ok)
    _, _, nmulti, nsub, nzero = rm.tally(out, cand)
    s = STATS.setdefault(site, [0, 0, 0, 0, 0])
    for i, v in enumerate((out.size, int(npri.sum()), nmulti, nsub, nzero)):
        s[i] += v
    print(f"{site} {what} {arr}: {out.size} draws, {int(npri.sum())} non-primary, {nmulti} with two candidates, {nsub} subnormal, {nzero} zero outputs")
    assert bad.shape[0] == 0, "%s %s %s: %d outputs outside their candidates; (index, got, lower, primary, upper) bits: %s" % (
        site, what, arr, bad.shape[0], [(tuple(i), ) + tuple(hex(hs.bits(a)[tuple(i)]) for a in (out, cand[0], cand[1], cand[2])) for i in bad[:6]])
    if arr == "interleaved":
        assert nsub > 0 and nzero > 0, (nsub, nzero)


# ------------------------------------------------------------------------------------------------ gq_rmsnorm_rows
@pytest.mark.parametrize("with_delta", [False, True], ids=["plain", "delta"])
@pytest.mark.parametrize("D", [8, 520, 2048, 16384])
@pytest.mark.parametrize("arr", ["banded", "interleaved", "gauss"])
def test_rmsnorm_rows(arr, D, with_delta):
    _lib = _L()
    x, w = (rm.gauss(D, rows=max(4, 4096 // D)) if arr == "gauss" else rm.ARRANGEMENTS[arr](D)), rm.weights(D)
    S = x.shape[0]
    delta = rm.delta_for(x) if with_delta else None
    for eps in rm.EPSS:
        g = Guards()
        xb, wb, db = g.inp("x", x), g.inp("w", w), g.inp("delta", delta)
        ob = g.out("out", 2 * S * D)
        _lib.check(_lib.lib().gq_rmsnorm_rows(xb.ptr(), db.ptr() if db is not None else None, wb.ptr(), ob.ptr(), S, D, eps, _lib.current_stream_ptr()),
                   "gq_rmsnorm_rows")
        g.check()
        xin = x
        if with_delta:
            xin = half_add(x, delta)
            assert np.isfinite(xin).all()
            assert np.array_equal(hs.bits(xb.numpy(np.float16, (S, D))), hs.bits(xin)), "the written-back x + delta is one fp16 add"
        else:
            assert np.array_equal(hs.bits(xb.numpy(np.float16, (S, D))), hs.bits(x)), "x is left alone"
        out = ob.numpy(np.float16, (S, D))
        _record("rows", arr, out, rm.candidates(xin, w, eps, D, "rows"), True, f"D {D} eps {eps}" + (" +delta" if with_delta else ""))


# ------------------------------------------------------------------------------------------------ QK-norm, the prompt row writer
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("arr", ["banded", "interleaved"])
def test_qknorm_rows(arr, hd):
    """S tokens of one q head and one k head: token s has row s of the arrangement as q and row S - 1 - s as k; v is zero"""
    _lib = _L()
    x = rm.ARRANGEMENTS[arr](hd)
    S = x.shape[0]
    qw, kw = rm.weights(hd, seed=5), rm.weights(hd, seed=6)
    qkv = np.concatenate([x, x[::-1], np.zeros_like(x)], axis=1)
    pos = np.arange(S, dtype=np.int32)
    one = np.ones((S, hd), dtype=np.float16)
    for eps in rm.EPSS:
        g = Guards()
        b = dict(qkv=g.inp("qkv", qkv), pos=g.inp("pos", pos), cos=g.inp("cos", one), sin=g.inp("sin", np.zeros_like(one)), qw=g.inp("qw", qw),
                 kw=g.inp("kw", kw))
        q, kc, vc = g.out("q", 2 * S * hd), g.out("kc", 2 * S * hd), g.out("vc", 2 * S * hd)
        rc = _lib.lib().gq_qknorm_rope_cache_rows(b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q.ptr(), kc.ptr(), vc.ptr(), S, 1, 1, hd, S,
                                                  b["qw"].ptr(), b["kw"].ptr(), eps, _lib.current_stream_ptr())
        _lib.check(rc, "gq_qknorm_rope_cache_rows")
        g.check()
        assert (hs.bits(vc.numpy(np.float16)) == 0).all()
        _record("qkn-rows", arr, q.numpy(np.float16, (S, hd)), rm.candidates(x, qw, eps, hd, "qkn-rows"), False, f"q_out hd {hd} eps {eps}")
        _record("qkn-rows", arr, kc.numpy(np.float16, (S, hd)), rm.candidates(x[::-1], kw, eps, hd, "qkn-rows"), False, f"k rows hd {hd} eps {eps}")


# ------------------------------------------------------------------------------------------------ QK-norm, the decode attention
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("arr", ["banded", "interleaved"])
def test_qknorm_decode_writes_the_normalised_k_row(arr, hd):
    """H = Hkv = 8: a launch normalises 8 rows of the arrangement as the k heads of one token and writes them at its position.  q is a
    unit Gaussian, v and the cache in front are zero: the attention output is finite and not looked at."""
    _lib = _L()
    L = _lib.lib()
    H, MS = 8, 16
    x = rm.ARRANGEMENTS[arr](hd)
    R = x.shape[0]
    assert R % H == 0
    d = torch.device("cuda:0")
    qw, kw = rm.weights(hd, seed=5), rm.weights(hd, seed=6)
    tq, tk = torch.from_numpy(qw).to(d), torch.from_numpy(kw).to(d)
    cos, sin = torch.ones(MS, hd, dtype=torch.float16, device=d), torch.zeros(MS, hd, dtype=torch.float16, device=d)
    qrand = np.random.default_rng(hd).normal(0, 1, (H, hd)).astype(np.float16)
    out = torch.zeros(H * hd, dtype=torch.float16, device=d)
    for eps in rm.EPSS:
        got = np.zeros_like(x)
        for t in range(R // H):
            p = t % MS
            rows = x[t * H:(t + 1) * H]
            qkv = torch.from_numpy(np.concatenate([qrand.reshape(-1), rows.reshape(-1), np.zeros(H * hd, dtype=np.float16)])).to(d)
            pos = torch.tensor([p], dtype=torch.int32, device=d)
            kc = torch.zeros(H, MS, hd, dtype=torch.float16, device=d)
            vc = torch.zeros_like(kc)
            _lib.check(L.gq_attn_decode_split_qknorm(qkv.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                                     out.data_ptr(), H, H, hd, MS, 1.0 / math.sqrt(hd), 1, None, tq.data_ptr(), tk.data_ptr(), eps,
                                                     _lib.current_stream_ptr()), "gq_attn_decode_split_qknorm")
            torch.cuda.synchronize()
            k = kc.cpu().numpy()
            got[t * H:(t + 1) * H] = k[:, p]
            k[:, p] = 0
            assert not k.any(), "only the row of the position is written"
        assert torch.isfinite(out.float()).all()
        _record("qkn-decode", arr, got, rm.candidates(x, kw, eps, hd, "qkn-decode"), False, f"k row hd {hd} eps {eps}")


def test_print_the_tallies():
    """(last in the file) per site: draws, non-primary outputs, the multi-candidate share, subnormal and zero outputs seen"""
    for site, (n, npri, nmulti, nsub, nzero) in sorted(STATS.items()):
        print(f"{site}: {n} draws, {npri} non-primary, multi-candidate share {nmulti / n:.4f}, {nsub} subnormal and {nzero} zero outputs; grant 2^{math.log2(rm.grant(site)):.2f}")
        assert npri <= nmulti
