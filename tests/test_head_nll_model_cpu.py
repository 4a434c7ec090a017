"""CPU: the host model of the scoring head (tests/head_nll_model.py) and the premises the GPU test of gq_head_nll rests on.

  * the model is torch's cross entropy on float64 logits (reduction="none"), its top1 torch's argmax;
  * the EXACT family is exact: for xn in {-1, 0, 1} / 4 and W in {-2 .. 2} / 8 the fp32 product of torch, the float64 product and
    the fp16 roundings of both are the same numbers, so a kernel that accumulates in fp32 in ANY order must produce the model's
    logits bit for bit -- and a share of the rows has tied maxima, so the lowest-id rule is exercised;
  * REF_ERR, the error of torch's own fp32 cross entropy / logsumexp against float64 on those logits, is what the GPU test's bound
    (4 x REF_ERR) is derived from: measured 9.55e-7 over the shapes below (the largest at (129, 4104, 512)), asserted here.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import head_nll_model as hm  # noqa: E402

from head_nll_model import EXACT_SHAPES, REF_ERR  # noqa: E402


def test_model_is_cross_entropy_on_float64_logits():
    import torch.nn.functional as F
    r = np.random.RandomState(0)
    logits = np.round(r.randn(37, 301) * 3.0, 2)
    logits[5, 17] = logits[5].max()  # a tie: two columns hold the largest
    logits[5, 200] = logits[5].max()
    t = r.randint(0, 301, size=37)
    t[3] = -1
    lse, lp, top1 = hm.model(logits, t)
    ce = F.cross_entropy(torch.from_numpy(logits), torch.from_numpy(np.maximum(t, 0)), reduction="none").numpy()
    keep = t >= 0
    assert np.abs(-ce[keep] - lp[keep]).max() < 1e-12
    assert lp[3] == 0.0
    assert np.abs(lse - torch.logsumexp(torch.from_numpy(logits), 1).numpy()).max() < 1e-12
    assert np.array_equal(top1, logits.argmax(1)) and top1[5] == min(np.flatnonzero(logits[5] == logits[5].max()))


@pytest.mark.parametrize("S,V,D", [(70, 2088, 256), (129, 4104, 512), (1, 40, 64)])
def test_exact_family_is_exact_and_has_ties(S, V, D):
    xn, W = hm.exact_case(S, V, D)
    p64 = xn.astype(np.float64) @ W.astype(np.float64).T
    p32 = torch.from_numpy(xn).float() @ torch.from_numpy(W).float().T
    l64 = hm.logits16(xn, W)
    assert np.array_equal(p32.numpy().astype(np.float64), p64)  # fp32 accumulation loses nothing
    assert np.array_equal(p64, l64)  # nor does the rounding to fp16
    assert np.array_equal(p32.half().double().numpy(), l64)
    assert np.array_equal(p64 * 32.0, np.round(p64 * 32.0))  # multiples of 1 / 32
    tied = ((l64 == l64.max(1)[:, None]).sum(1) > 1)
    assert tied.any(), "no tied maximum: the lowest-id rule would go untested"
    if S == 1:
        assert tied[0]


def test_reference_error_of_fp32_torch():
    import torch.nn.functional as F
    worst = 0.0
    for S, V, D in EXACT_SHAPES:
        xn, W = hm.exact_case(S, V, D)
        l64 = hm.logits16(xn, W)
        t = hm.targets(S, V, hm.split_ranges(V, 3))
        lse, lp, _ = hm.model(l64, t)
        l32 = torch.from_numpy(l64).float()
        ce = F.cross_entropy(l32, torch.from_numpy(np.maximum(t, 0)).long(), reduction="none").double().numpy()
        e = max(np.abs(np.where(t >= 0, -ce, 0.0) - lp).max(), np.abs(torch.logsumexp(l32, 1).double().numpy() - lse).max())
        print("(%d, %d, %d): torch fp32 against float64 %.3e" % (S, V, D, e))
        worst = max(worst, e)
    assert worst <= REF_ERR, worst


def test_targets_cover_the_edges():
    V = 2088
    edges = hm.split_ranges(V, 3)
    assert edges == [(0, 768), (768, 1536), (1536, 2088)]
    assert hm.split_ranges(129, 3) == [(0, 128), (128, 129), (129, 129)]  # (a split without a column)
    t = hm.targets(64, V, edges)
    for v in (0, V - 1, -1, 767, 768, 1535, 1536):
        assert v in t
    assert ((t >= -1) & (t < V)).all()


def test_ulp16():
    assert hm.ulp16(1.0) == 2.0**-10 and hm.ulp16(5.3) == 2.0**-8 and hm.ulp16(30000.0) == 16.0
