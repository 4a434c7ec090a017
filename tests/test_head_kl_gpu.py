"""GPU: the KL head gq_head_kl (csrc/head_kl.hip) through the C ABI, on guard-banded, poisoned buffers (tests/guarded.py), against a
float64 evaluation of its definition.

xp, xq in {-1, -0.5, 0, 0.5, 1} and W in k / 8, |k| <= 8: every product is a multiple of 1 / 16 and every partial sum stays below 2^12 of
them, so the fp32 accumulators are exact in any order and the kernel's fp16 logits ARE the rounded exact sums.  top1_p / top1_q must
equal the model's (ties included: the lowest id).  kl, lse_p, lse_q lie within the worst case of a V-term fp32 sum, per row
    |dkl|  <= (V + 16) 2^-23 (1 + max_v |lp - lq|) + 2^-22 (|lse_p| + |lse_q|)        |dlse| <= (V + 16) 2^-23 + 2^-22 |lse|
(derived: sequential-sum error (n - 1) u sum |t_i| with u = 2^-24, normalised terms, and a few ulp per exp / log; a dropped tile or a
missed rescale misses it by orders of magnitude).  xq is an independent draw, xp with a few entries changed, or xp itself -- and then kl
is exactly 0.0 and the two top1 agree.  The shapes: one token; a ragged second row tile with a ragged, odd last W tile; three ranges; more
ranges than tiles (empty ranges contribute the neutral element)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from guarded import Guards, ptr  # noqa: E402

SHAPES = [(1, 1, 64, 1), (129, 257, 64, 1), (130, 385, 192, 3), (17, 300, 128, 5)]


def _L():
    from guidedquant_amd import _lib
    return _lib


def _case(S, V, D, kind):
    rng = np.random.default_rng(S * 1000 + V)
    xp = (rng.integers(-2, 3, (S, D)) / 2.0).astype(np.float16)
    W = (rng.integers(-8, 9, (V, D)) / 8.0).astype(np.float16)
    xq = xp.copy()
    if kind == "independent":
        xq = (rng.integers(-2, 3, (S, D)) / 2.0).astype(np.float16)
    elif kind == "near":
        xq[rng.integers(0, S, 3 * S), rng.integers(0, D, 3 * S)] = 0.5
    return xp, xq, W


def _model(xp, xq, W):
    """float64: (kl, lse_p, lse_q, top1_p, top1_q, max |lp - lq|) of the fp16-rounded exact logits"""
    lp = (xp.astype(np.float64) @ W.astype(np.float64).T).astype(np.float16).astype(np.float64)
    lq = (xq.astype(np.float64) @ W.astype(np.float64).T).astype(np.float16).astype(np.float64)
    zp = lp.max(1) + np.log(np.exp(lp - lp.max(1, keepdims=True)).sum(1))
    zq = lq.max(1) + np.log(np.exp(lq - lq.max(1, keepdims=True)).sum(1))
    kl = (np.exp(lp - zp[:, None]) * (lp - lq)).sum(1) - zp + zq
    return kl, zp, zq, lp.argmax(1), lq.argmax(1), np.abs(lp - lq).max(1)


def _run(xp, xq, W, splits, D=None, ws_cut=0):
    L = _L()
    S, V = xp.shape[0], W.shape[0]
    D = xp.shape[1] if D is None else D
    nws = int(L.lib().gq_head_kl_ws_bytes(S, V, D, splits))
    g = Guards()
    bp, bq, bw = g.inp("xp", xp), g.inp("xq", xq), g.inp("W", W)
    outs = [g.out(n, 4 * S) for n in ("kl", "lse_p", "lse_q", "top1_p", "top1_q")]
    bws = g.out("ws", max(nws - ws_cut, 4))
    rc = L.lib().gq_head_kl(bp.ptr(), bq.ptr(), bw.ptr(), S, V, D, *[ptr(o) for o in outs], splits, bws.ptr(), max(nws - ws_cut, 0), None)
    g.check()
    return (rc, *[o.numpy(t).copy() for o, t in zip(outs, (np.float32, np.float32, np.float32, np.int32, np.int32))])


@pytest.mark.parametrize("kind", ["independent", "near", "equal"])
@pytest.mark.parametrize("S,V,D,splits", SHAPES, ids=["S%d-V%d-D%d-x%d" % c for c in SHAPES])
def test_kl_head_against_float64(S, V, D, splits, kind):
    xp, xq, W = _case(S, V, D, kind)
    kl, zp, zq, tp, tq, dmax = _model(xp, xq, W)
    rc, gkl, gzp, gzq, gtp, gtq = _run(xp, xq, W, splits)
    assert rc == 0, _L().lib().gq_last_error()
    assert np.array_equal(gtp, tp) and np.array_equal(gtq, tq)
    e_kl, e_p, e_q = np.abs(gkl - kl), np.abs(gzp - zp), np.abs(gzq - zq)
    b_kl = (V + 16) * 2.0**-23 * (1 + dmax) + 2.0**-22 * (np.abs(zp) + np.abs(zq))
    print("S%d V%d D%d splits %d %s: worst |dkl| / bound %.3e, |dlse_p| %.3e, |dlse_q| %.3e, mean kl %.4f"
          % (S, V, D, splits, kind, (e_kl / b_kl).max(), e_p.max(), e_q.max(), kl.mean()))
    assert (e_kl <= b_kl).all()
    assert (e_p <= (V + 16) * 2.0**-23 + 2.0**-22 * np.abs(zp)).all() and (e_q <= (V + 16) * 2.0**-23 + 2.0**-22 * np.abs(zq)).all()
    if kind == "equal":
        assert (gkl == 0.0).all() and np.array_equal(gtp, gtq) and np.array_equal(gzp.view(np.uint32), gzq.view(np.uint32))
    elif V > 1:
        assert kl.max() > 1e-3  # (the case does measure a divergence)


def test_unsupported_d_and_short_workspace_write_nothing():
    L = _L()
    z = np.zeros((5, 96), dtype=np.float16)
    rc, *outs = _run(z, z, np.zeros((40, 96), dtype=np.float16), 1)
    assert rc == L.GQ_ENOTSUP and all((o.view(np.uint8) == 0x7E).all() for o in outs)
    xp, xq, W = _case(15, 128, 64, "near")
    rc, *outs = _run(xp, xq, W, 2, ws_cut=4)
    assert rc == L.GQ_EINVAL and all((o.view(np.uint8) == 0x7E).all() for o in outs)
    assert L.lib().gq_head_kl_ws_bytes(15, 128, 64, 2) == 2 * 15 * 9 * 4
