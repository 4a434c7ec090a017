"""GPU: the scoring head gq_head_nll (csrc/head_nll.hip) through the C ABI, on guard-banded, poisoned buffers (tests/guarded.py: the
outputs and the workspace are left poisoned, the guards are checked after every call), against the float64 host model of
tests/head_nll_model.py.

  exact      xn in {-1, 0, 1} / 4, W in {-2 .. 2} / 8: every logit is a multiple of 1 / 32, exact in any summation order
             (test_head_nll_model_cpu.py asserts it), so the kernel's fp16 logits ARE the model's.  top1 must equal the model's exactly,
             ties included (3 - 13 % of the rows tie; the single row of (1, 40, 64) does); a row with target -1 is exactly 0.0.
             lse and logprob: |got - float64| <= 4 x REF_ERR = 3.84e-6, where REF_ERR = 9.6e-7 is the largest error of torch's own fp32
             cross_entropy / logsumexp against float64 on the same logits (measured on the CPU: 9.55e-7, asserted in
             test_head_nll_model_cpu.py); the factor 4 covers what the online form adds to a one-pass fp32 softmax: one exp rounding
             of the rescale per tile and per split on top of the terms' own.
             Every shape runs with splits 0, 1, 2, 3 and tiles + 1 (one split holds no column).
  round-off  xn = randn, W = 0.05 randn: the summation order may move a logit by one fp16 step, so |dlogprob| <= 2 ulp16(max |logit| of
             the row) -- one for the target, one for the largest term of the sum -- and top1 is compared on the rows whose float64
             top-two gap is at least 2 ulp16 (at most 10 % of the rows may be left out; seed 2 leaves out 0 of 70 and 2 of 129).
  range      one column at +30000 in the last tile of the last split, every other at -30000: finite, lse == that logit.
  lse / top1 NULL leave logprob unchanged; D = 96 is GQ_ENOTSUP, a short workspace GQ_EINVAL, and neither writes anything.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import head_nll_model as hm  # noqa: E402
from guarded import Guards, ptr  # noqa: E402
from head_nll_model import EXACT_SHAPES, REF_ERR  # noqa: E402

BOUND = 4.0 * REF_ERR


def _L():
    from guidedquant_amd import _lib
    return _lib


def _run(xn, W, target, splits, want_lse=True, want_top1=True, ws_cut=0, D=None):
    """one call; (rc, logprob, lse, top1) as numpy (None where not asked for), guards checked"""
    L = _L()
    S, V = xn.shape[0], W.shape[0]
    D = xn.shape[1] if D is None else D
    nws = int(L.lib().gq_head_nll_ws_bytes(S, V, D, splits))
    g = Guards()
    bx, bw, bt = g.inp("xn", xn), g.inp("W", W), g.inp("target", np.asarray(target, dtype=np.int32))
    blp = g.out("logprob", 4 * S)
    blse = g.out("lse", 4 * S) if want_lse else None
    btop = g.out("top1", 4 * S) if want_top1 else None
    bws = g.out("ws", max(nws - ws_cut, 4))
    rc = L.lib().gq_head_nll(bx.ptr(), bw.ptr(), bt.ptr(), S, V, D, blp.ptr(), ptr(blse), ptr(btop), splits, bws.ptr(), max(nws - ws_cut, 0), None)
    g.check()
    return (rc, blp.numpy(np.float32).copy(), blse.numpy(np.float32).copy() if want_lse else None,
            btop.numpy(np.int32).copy() if want_top1 else None)


def _poisoned(a):
    return bool((a.view(np.uint8) == 0x7E).all())


_EXACT = {}


def _exact(S, V, D):
    if (S, V, D) not in _EXACT:
        xn, W = hm.exact_case(S, V, D)
        _EXACT[(S, V, D)] = (xn, W, hm.logits16(xn, W))
    return _EXACT[(S, V, D)]


def _splits_of(V):
    return (0, 1, 2, 3, (V + hm.BV - 1) // hm.BV + 1)


@pytest.mark.parametrize("S,V,D", EXACT_SHAPES, ids=["S%d-V%d-D%d" % c for c in EXACT_SHAPES])
def test_exact_family(S, V, D):
    xn, W, l64 = _exact(S, V, D)
    for n, splits in enumerate(_splits_of(V)):
        t = hm.targets(S, V, hm.split_ranges(V, max(splits, 1)), seed=n)
        lse, lp, top1 = hm.model(l64, t)
        rc, glp, glse, gtop = _run(xn, W, t, splits)
        assert rc == 0, _L().lib().gq_last_error()
        assert np.isfinite(glp).all() and np.isfinite(glse).all()
        e_lse, e_lp = np.abs(glse.astype(np.float64) - lse).max(), np.abs(glp.astype(np.float64) - lp).max()
        print("S%d V%d D%d splits %d: |dlse| %.3e  |dlogprob| %.3e  (torch fp32: %.3e, bound %.3e)" % (S, V, D, splits, e_lse, e_lp, REF_ERR, BOUND))
        assert np.array_equal(gtop.astype(np.int64), top1), (splits, np.flatnonzero(gtop != top1)[:8])
        assert (glp[t < 0] == 0.0).all() and not np.signbit(glp[t < 0]).any()
        assert e_lse <= BOUND and e_lp <= BOUND, (splits, e_lse, e_lp)


@pytest.mark.parametrize("S,V,D", [(70, 2088, 256), (129, 4104, 512)])
def test_roundoff_family(S, V, D):
    xn, W = hm.roundoff_case(S, V, D, seed=2)
    l64 = hm.logits16(xn, W)
    srt = np.sort(l64, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) >= 2.0 * hm.ulp16(srt[:, -1])
    assert clear.mean() >= 0.9
    tol = 2.0 * hm.ulp16(np.abs(l64).max(axis=1))
    for n, splits in enumerate((0, 3)):
        t = hm.targets(S, V, hm.split_ranges(V, max(splits, 1)), seed=n)
        lse, lp, top1 = hm.model(l64, t)
        rc, glp, glse, gtop = _run(xn, W, t, splits)
        assert rc == 0, _L().lib().gq_last_error()
        d = np.abs(glp.astype(np.float64) - lp)
        print("S%d V%d D%d splits %d: worst |dlogprob| / (2 ulp16) %.3f, top1 compared on %d of %d rows" % (S, V, D, splits, (d / tol).max(), clear.sum(), S))
        assert (d <= tol).all(), (splits, (d / tol).max())
        assert (np.abs(glse.astype(np.float64) - lse) <= tol).all()
        assert np.array_equal(gtop[clear].astype(np.int64), top1[clear])
        assert (glp[t < 0] == 0.0).all()


def test_range_one_column_far_above_the_rest():
    S, V, D = 3, 300, 64  # three tiles; splits = 2: tiles {0, 1} and {2}
    hot = 299
    xn = np.ones((S, D), dtype=np.float16)
    W = np.full((V, D), -468.75, dtype=np.float16)  # 64 x 468.75 = 30000, an fp16 value
    W[hot] = 468.75
    t = np.array([hot, 5, -1], dtype=np.int32)
    rc, lp, lse, top1 = _run(xn, W, t, 2)
    assert rc == 0, _L().lib().gq_last_error()
    assert np.isfinite(lp).all() and np.isfinite(lse).all()
    assert (lse == 30000.0).all() and (top1 == hot).all()
    assert lp[0] == 0.0 and lp[1] == -60000.0 and lp[2] == 0.0


def test_null_lse_and_top1_leave_logprob_unchanged():
    S, V, D = 65, 2088, 256
    xn, W, l64 = _exact(S, V, D)
    t = hm.targets(S, V, hm.split_ranges(V, 2))
    rc, lp, lse, top1 = _run(xn, W, t, 2)
    assert rc == 0
    for want_lse, want_top1 in ((False, True), (True, False), (False, False)):
        rc2, lp2, lse2, top2 = _run(xn, W, t, 2, want_lse=want_lse, want_top1=want_top1)
        assert rc2 == 0, _L().lib().gq_last_error()
        assert np.array_equal(lp2.view(np.uint32), lp.view(np.uint32))
        assert lse2 is None or np.array_equal(lse2.view(np.uint32), lse.view(np.uint32))
        assert top2 is None or np.array_equal(top2, top1)


def test_unsupported_d_and_short_workspace_write_nothing():
    L = _L()
    xn = np.zeros((5, 96), dtype=np.float16)
    W = np.zeros((40, 96), dtype=np.float16)
    t = np.zeros(5, dtype=np.int32)
    rc, lp, lse, top1 = _run(xn, W, t, 1)
    assert rc == L.GQ_ENOTSUP and _poisoned(lp) and _poisoned(lse) and _poisoned(top1)
    xn, W, _ = _exact(15, 128, 64)
    t = np.zeros(15, dtype=np.int32)
    rc, lp, lse, top1 = _run(xn, W, t, 2, ws_cut=4)
    assert rc == L.GQ_EINVAL and _poisoned(lp) and _poisoned(lse) and _poisoned(top1)
    assert L.lib().gq_head_nll_ws_bytes(15, 128, 64, 2) == 2 * 15 * 5 * 4
