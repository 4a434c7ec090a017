"""GPU: gq_head_nll_topn (csrc/head_nll.hip) through the C ABI on guard-banded, poisoned buffers (tests/guarded.py), against the float64
host model of tests/head_nll_model.py on its EXACT family: every logit is a multiple of 1 / 32 in any summation order, so the kernel's
fp16 logits are the model's, ties are plentiful (five values of W, three of xn) and no comparison needs a tolerance.
  ids      == the model's stable descending order (value descending, id ascending), for every `splits`: 1, 3 at V = 1000, and one more
              than the vocabulary has tiles (a split without a tile merges);
  top_lps  == float32(logit) - lse from the RETURNED lse, bit for bit; the listed target's entry == logprob bit for bit;
  logprob / lse / top1 bit-equal to gq_head_nll's with the same `splits`; a second launch bit-equal; V = 7 under n = 20 fills -1 / -inf.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import head_nll_model as hm  # noqa: E402
from guarded import Guards  # noqa: E402
from test_head_nll_gpu import _poisoned, _run as plain_run  # noqa: E402


def _L():
    from guidedquant_amd import _lib
    return _lib


def _run(xn, W, target, n, splits, ws_cut=0, D=None):
    """one call: (rc, logprob, lse, top1, top_ids [S, n'], top_lps [S, n']) as numpy, n' = max(n, 1), guards checked"""
    L = _L()
    S, V = xn.shape[0], W.shape[0]
    D = xn.shape[1] if D is None else D
    nws = int(L.lib().gq_head_nll_topn_ws_bytes(S, V, D, splits, n))
    g = Guards()
    bx, bw, bt = g.inp("xn", xn), g.inp("W", W), g.inp("target", np.asarray(target, dtype=np.int32))
    out = {k: g.out(k, 4 * S) for k in ("logprob", "lse", "top1")}
    bid, blp = g.out("top_ids", 4 * S * max(n, 1)), g.out("top_lps", 4 * S * max(n, 1))
    bws = g.out("ws", max(nws - ws_cut, 4))
    rc = L.lib().gq_head_nll_topn(bx.ptr(), bw.ptr(), bt.ptr(), S, V, D, out["logprob"].ptr(), out["lse"].ptr(), out["top1"].ptr(), n, bid.ptr(), blp.ptr(),
                                  splits, bws.ptr(), max(nws - ws_cut, 0), None)
    g.check()
    return (rc, out["logprob"].numpy(np.float32).copy(), out["lse"].numpy(np.float32).copy(), out["top1"].numpy(np.int32).copy(),
            bid.numpy(np.int32, (S, max(n, 1))).copy(), blp.numpy(np.float32, (S, max(n, 1))).copy())


def _want_ids(l64, n):
    """the model's list: value descending, id ascending (a stable sort), -1 behind the vocabulary"""
    order = np.argsort(-l64, axis=1, kind="stable")[:, :n]
    return np.pad(order, ((0, 0), (0, n - order.shape[1])), constant_values=-1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_CASES = {}


def _case(S, V, D):
    if (S, V, D) not in _CASES:
        xn, W = hm.exact_case(S, V, D)
        _CASES[(S, V, D)] = (xn, W, hm.logits16(xn, W))
    return _CASES[(S, V, D)]


@pytest.mark.parametrize("n", [1, 5, 20])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("V", [7, 129, 1000])
@pytest.mark.parametrize("S", [1, 129])
def test_lists_against_the_host_model(S, V, D, n):
    xn, W, l64 = _case(S, V, D)
    want = _want_ids(l64, n)
    tiles = (V + hm.BV - 1) // hm.BV
    for splits in ((1, 3) if V == 1000 else (1, )) + (tiles + 1, ):
        t = hm.targets(S, V, hm.split_ranges(V, splits), seed=splits)
        rc, lp, lse, top1, ids, lps = _run(xn, W, t, n, splits)
        assert rc == 0, _L().lib().gq_last_error()
        assert np.array_equal(ids, want), (splits, np.argwhere(ids != want)[:4])
        listed = want >= 0
        vals = np.take_along_axis(l64, np.maximum(want, 0), axis=1).astype(np.float32)
        want_lps = np.where(listed, vals - lse[:, None], np.float32(-np.inf)).astype(np.float32)
        assert np.array_equal(_bits(lps), _bits(want_lps)), splits
        hit = listed & (want == t[:, None])  # (a negative target matches no id: its row still has its list)
        assert np.array_equal(_bits(lps[hit]), _bits(np.broadcast_to(lp[:, None], lps.shape)[hit]))
        assert np.array_equal(top1, want[:, 0])
        rc0, lp0, lse0, top0 = plain_run(xn, W, t, splits)
        assert rc0 == 0 and np.array_equal(_bits(lp), _bits(lp0)) and np.array_equal(_bits(lse), _bits(lse0)) and np.array_equal(top1, top0)
        again = _run(xn, W, t, n, splits)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again[1:], (lp, lse, top1, ids, lps)))


def test_a_nan_logit_is_never_listed():
    S, V, D, n, row, tok = 20, 300, 64, 5, 3, 17
    xn, W = hm.exact_case(S, V, D, seed=1)
    l64 = hm.logits16(xn, W)
    t = hm.targets(S, V, hm.split_ranges(V, 2))
    clean = _run(xn, W, t, n, 2)
    assert clean[0] == 0 and np.array_equal(clean[4], _want_ids(l64, n))
    bad = xn.copy()
    bad[row, 5] = np.nan  # the row's logits are all NaN: nothing to list; every other row is what it was
    rc, lp, lse, top1, ids, lps = _run(bad, W, t, n, 2)
    assert rc == 0 and (ids[row] == -1).all() and np.isneginf(lps[row]).all()
    keep = np.arange(S) != row
    assert np.array_equal(ids[keep], clean[4][keep]) and np.array_equal(_bits(lps[keep]), _bits(clean[5][keep]))
    bad = W.copy()
    bad[tok, 9] = np.nan  # one token's logit is NaN in every row: the lists are the model's without it (lse, and so the values, are NaN)
    rc, lp, lse, top1, ids, lps = _run(xn, bad, t, n, 2)
    rest = _want_ids(np.delete(l64, tok, axis=1), n)
    assert rc == 0 and np.array_equal(ids, rest + (rest >= tok))
    assert np.isnan(lps).all()


def test_refusals_write_nothing():
    L = _L()
    xn, W, _ = _case(129, 129, 64)
    t = np.zeros(129, dtype=np.int32)
    for n, splits, cut, want in ((0, 1, 0, L.GQ_EINVAL), (21, 1, 0, L.GQ_EINVAL), (5, 2, 4, L.GQ_EINVAL)):
        rc, *outs = _run(xn, W, t, n, splits, ws_cut=cut)
        assert rc == want and all(_poisoned(o) for o in outs), (n, splits, cut, rc)
    rc, *outs = _run(np.zeros((5, 96), dtype=np.float16), np.zeros((40, 96), dtype=np.float16), np.zeros(5, dtype=np.int32), 5, 1)
    assert rc == L.GQ_ENOTSUP and all(_poisoned(o) for o in outs)
    assert L.lib().gq_head_nll_topn_ws_bytes(15, 128, 64, 2, 5) == (2 * 15 * 5 + 15 + 2 * 15 * 5 * 2) * 4
    assert L.lib().gq_head_nll_topn_ws_bytes(15, 128, 64, 2, 21) == 0
