"""GPU: the int8 scoring head gq_head_nll_i8 / gq_head_nll_i8_topn (csrc/head_nll.hip, the Q8 instances) through the C ABI on guard-banded,
poisoned buffers (tests/guarded.py), against the float64 host model of tests/head_nll_model.py on the logits
    hm.logits16(xn, q * scale[:, None])        logit = fp16(scale[v] * sum_k xn[k] q[v][k])

  same logits   q = 8 W, scale = 1 / 8 on the exact family: the logits are the fp16 head's numbers and everything behind them is shared, so
                logprob / lse / top1 equal gq_head_nll's on (xn, W) BIT FOR BIT for every `splits` -- only the operand path differs.
  per-row scale xn in {-1, 0, 1} / 4, codes uniform over -128 .. 127, scale[v] = 2^-(6 + v % 4): every partial sum is a multiple of 1 / 4
                below 2^24 steps and the scale a power of two, so scale * acc is exact in fp32 and the one fp16 rounding is the model's.
                top1 exactly, |lse - f64| and |logprob - f64| <= 4 x REF_ERR (test_head_nll_gpu.py says why), a target -1 row is +0.0.
                Row v, v % 4 and the lane map 16 a + 4 g + r do not line up: a wrong byte order, a wrong sign of -128 or a scale from
                the wrong row or tile shows here.
  round-off     xn = randn, codes uniform over -127 .. 127, scale[v] = (0.15 / 127) (1 + (v % 7) / 8): 2 ulp16(max |logit| of the row) on
                logprob and lse (a summation order moves a logit by one fp16 step; the fp32 scale multiply adds none), top1 on the rows
                whose float64 top-two gap is at least 2 ulp16 (RandomState(5000) leaves out 0 of 70 and 0 of 129 rows; the cap is 10 %).
  top-n         ids == the model's stable order, log-probabilities within 4 x REF_ERR, logprob / lse / top1 bit-equal to gq_head_nll_i8's.
  refusals      D = 96 GQ_ENOTSUP, a NULL scale and a short workspace GQ_EINVAL; every output still poisoned.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import head_nll_model as hm  # noqa: E402
from guarded import Guards, ptr  # noqa: E402

BOUND = 4.0 * hm.REF_ERR
IDS = ["S%d-V%d-D%d" % c for c in hm.EXACT_SHAPES]


def _L():
    from guidedquant_amd import _lib
    return _lib


def _run(xn, W, scale, target, splits, n=0, ws_cut=0, null_scale=False):
    """one call of gq_head_nll[_i8][_topn] (scale None: the fp16 entries; n: the top-n ones): (rc, logprob, lse, top1[, ids, lps])"""
    L, lib = _L(), _L().lib()
    S, V, D = xn.shape[0], W.shape[0], xn.shape[1]
    nws = int(lib.gq_head_nll_topn_ws_bytes(S, V, D, splits, n) if n else lib.gq_head_nll_ws_bytes(S, V, D, splits))
    g = Guards()
    head = [g.inp("xn", xn).ptr(), g.inp("W", W).ptr()]
    if scale is not None:
        head.append(None if null_scale else g.inp("scale", scale).ptr())
    out = {k: g.out(k, 4 * S) for k in ("logprob", "lse", "top1")}
    lists = [g.out("top_ids", 4 * S * n), g.out("top_lps", 4 * S * n)] if n else []
    bws = g.out("ws", max(nws - ws_cut, 4))
    entry = getattr(lib, "gq_head_nll" + ("_i8" if scale is not None else "") + ("_topn" if n else ""))
    rc = entry(*head, g.inp("target", np.asarray(target, dtype=np.int32)).ptr(), S, V, D, out["logprob"].ptr(), out["lse"].ptr(), out["top1"].ptr(),
               *([n] + [b.ptr() for b in lists] if n else []), splits, bws.ptr(), max(nws - ws_cut, 0), None)
    g.check()
    res = (rc, out["logprob"].numpy(np.float32).copy(), out["lse"].numpy(np.float32).copy(), out["top1"].numpy(np.int32).copy())
    return res + ((lists[0].numpy(np.int32, (S, n)).copy(), lists[1].numpy(np.float32, (S, n)).copy()) if n else ())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _poisoned(*arrays):
    return all(bool((a.view(np.uint8) == 0x7E).all()) for a in arrays)


def _splits_of(V):
    return (0, 1, 2, 3, (V + hm.BV - 1) // hm.BV + 1)


_ROWSCALE = {}


def _rowscale(S, V, D):
    """the per-row-scale family and its float64 logits, made once per shape"""
    if (S, V, D) not in _ROWSCALE:
        xn, _ = hm.exact_case(S, V, D)
        q = np.random.RandomState(4000).randint(-128, 128, size=(V, D)).astype(np.int8)
        scale = (2.0**-(6 + np.arange(V) % 4)).astype(np.float32)
        _ROWSCALE[(S, V, D)] = (xn, q, scale, hm.logits16(xn, q.astype(np.float64) * scale[:, None]))
    return _ROWSCALE[(S, V, D)]


@pytest.mark.parametrize("S,V,D", hm.EXACT_SHAPES, ids=IDS)
def test_same_logits_as_the_fp16_head(S, V, D):
    xn, W = hm.exact_case(S, V, D)
    q, scale = (8.0 * W.astype(np.float32)).astype(np.int8), np.full(V, 0.125, dtype=np.float32)
    assert np.array_equal(q.astype(np.float32) / 8.0, W.astype(np.float32))
    for n, splits in enumerate(_splits_of(V)):
        t = hm.targets(S, V, hm.split_ranges(V, max(splits, 1)), seed=n)
        want, got = _run(xn, W, None, t, splits), _run(xn, q, scale, t, splits)
        assert want[0] == 0 and got[0] == 0, _L().lib().gq_last_error()
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[1:], want[1:])), splits


@pytest.mark.parametrize("S,V,D", hm.EXACT_SHAPES, ids=IDS)
def test_full_code_range_and_row_scales(S, V, D):
    xn, q, scale, l64 = _rowscale(S, V, D)
    for n, splits in enumerate(_splits_of(V)):
        t = hm.targets(S, V, hm.split_ranges(V, max(splits, 1)), seed=n)
        lse, lp, top1 = hm.model(l64, t)
        rc, glp, glse, gtop = _run(xn, q, scale, t, splits)
        assert rc == 0, _L().lib().gq_last_error()
        e_lse, e_lp = np.abs(glse.astype(np.float64) - lse).max(), np.abs(glp.astype(np.float64) - lp).max()
        print("S%d V%d D%d splits %d: |dlse| %.3e  |dlogprob| %.3e  (bound %.3e)" % (S, V, D, splits, e_lse, e_lp, BOUND))
        assert np.array_equal(gtop.astype(np.int64), top1), (splits, np.flatnonzero(gtop != top1)[:8])
        assert (glp[t < 0] == 0.0).all() and not np.signbit(glp[t < 0]).any()
        assert e_lse <= BOUND and e_lp <= BOUND, (splits, e_lse, e_lp)


@pytest.mark.parametrize("S,V,D", [(70, 2088, 256), (129, 4104, 512)])
def test_roundoff_family(S, V, D):
    r = np.random.RandomState(5000)
    xn, q = r.randn(S, D).astype(np.float16), r.randint(-127, 128, size=(V, D)).astype(np.int8)
    scale = ((0.15 / 127.0) * (1.0 + (np.arange(V) % 7) / 8.0)).astype(np.float32)
    l64 = hm.logits16(xn, q.astype(np.float64) * scale[:, None])
    srt = np.sort(l64, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) >= 2.0 * hm.ulp16(srt[:, -1])
    print("top1 compared on %d of %d rows" % (clear.sum(), S))
    assert clear.mean() >= 0.9
    tol = 2.0 * hm.ulp16(np.abs(l64).max(axis=1))
    for n, splits in enumerate((0, 3)):
        t = hm.targets(S, V, hm.split_ranges(V, max(splits, 1)), seed=n)
        lse, lp, top1 = hm.model(l64, t)
        rc, glp, glse, gtop = _run(xn, q, scale, t, splits)
        assert rc == 0, _L().lib().gq_last_error()
        d = np.abs(glp.astype(np.float64) - lp)
        print("S%d V%d D%d splits %d: worst |dlogprob| / (2 ulp16) %.3f" % (S, V, D, splits, (d / tol).max()))
        assert (d <= tol).all(), (splits, (d / tol).max())
        assert (np.abs(glse.astype(np.float64) - lse) <= tol).all()
        assert np.array_equal(gtop[clear].astype(np.int64), top1[clear])
        assert (glp[t < 0] == 0.0).all()


@pytest.mark.parametrize("n", [1, 20])
@pytest.mark.parametrize("S,V,D", [(16, 129, 192), (65, 2088, 256)])
def test_topn_lists(S, V, D, n):
    xn, q, scale, l64 = _rowscale(S, V, D)
    want = np.argsort(-l64, axis=1, kind="stable")[:, :n]
    for splits in (0, 3):
        t = hm.targets(S, V, hm.split_ranges(V, max(splits, 1)), seed=splits)
        lse64 = hm.model(l64, t)[0]
        rc, lp, lse, top1, ids, lps = _run(xn, q, scale, t, splits, n=n)
        assert rc == 0, _L().lib().gq_last_error()
        assert np.array_equal(ids, want), (splits, np.argwhere(ids != want)[:4])
        assert np.abs(lps.astype(np.float64) - (np.take_along_axis(l64, want, axis=1) - lse64[:, None])).max() <= BOUND
        plain = _run(xn, q, scale, t, splits)
        assert plain[0] == 0 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((lp, lse, top1), plain[1:]))


def test_refusals_write_nothing():
    L = _L()
    t = np.zeros(5, dtype=np.int32)
    for n in (0, 5):
        rc, *outs = _run(np.zeros((5, 96), dtype=np.float16), np.zeros((40, 96), dtype=np.int8), np.ones(40, dtype=np.float32), t, 1, n=n)
        assert rc == L.GQ_ENOTSUP and _poisoned(*outs), n
        xn, q, scale = np.zeros((5, 64), dtype=np.float16), np.zeros((128, 64), dtype=np.int8), np.ones(128, dtype=np.float32)
        rc, *outs = _run(xn, q, scale, t, 2, n=n, null_scale=True)
        assert rc == L.GQ_EINVAL and _poisoned(*outs), n
        rc, *outs = _run(xn, q, scale, t, 2, n=n, ws_cut=4)
        assert rc == L.GQ_EINVAL and _poisoned(*outs), n
