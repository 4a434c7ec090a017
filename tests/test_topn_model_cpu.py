"""CPU: tests/topn_model.py, the host model of the top-n alternatives, checked against torch and against hand-built order cases.
(a) on random logits without ties its ids are torch.topk's and its log-probabilities agree with a float64 log_softmax within the grant
    lp_raw has against float64 (tests/test_sampler_lp_gpu.py: 4 * max(ref_err, ulp32(|lse|)), topn_model.grant);
(b) hand-built orders: equal values list the lower id first, +0 above -0 whatever the ids, -inf entries are listed with -inf, NaN logits of
    both signs are left out, a vocabulary shorter than n is filled with -1 / -inf;
(c) the log-probability is lp_raw's expression: two subtractions against (M, L), not one against their sum;
(d) the row rule;
(e) every fault the model can inject is seen by one of these checks."""
import numpy as np
import pytest

import sampler_model as sm
import topn_model as tm

torch = pytest.importorskip("torch")


def _no_ties(V, seed):
    """V distinct fp16 values in random order"""
    rng = np.random.default_rng(seed)
    bits = rng.permutation(np.arange(0x2000, 0x4C00, dtype=np.uint16))[:V]  # positive normals up to 16
    x = bits.view(np.float16).copy()
    x[rng.random(V) < 0.5] *= np.float16(-1)
    assert np.unique(x.astype(np.float32)).size == V
    return x


def _b(*bits):
    return np.array(bits, dtype=np.uint16).view(np.float16)


def _ids(x, n, fault=None):
    return tm.top_n(x, n, *tm.lse_pair(x), fault=fault)[0].tolist()


@pytest.mark.parametrize("V,n", [(1000, 1), (1000, 5), (5000, 20), (21, 20)])
def test_ids_are_torch_topk_and_logprobs_float64_within_lp_raws_grant(V, n):
    x = _no_ties(V, V + n)
    ids, lps = tm.top_n(x, n, *tm.lse_pair(x))
    t = torch.from_numpy(x.astype(np.float64))
    want = torch.topk(t, n)
    assert ids.tolist() == want.indices.tolist()
    ref = torch.log_softmax(t, dim=0)[want.indices].numpy()
    g = tm.grant(x)
    assert 0 < g < 1e-4
    assert np.abs(lps.astype(np.float64) - ref).max() <= g
    ids64, lps64 = tm.top_n64(x, n)
    assert ids64.tolist() == ids.tolist() and np.abs(lps64 - ref).max() < 1e-12


def test_equal_values_list_the_lower_id_first():
    x = np.full(40, 1.5, dtype=np.float16)
    assert _ids(x, 5) == [0, 1, 2, 3, 4]
    x[[7, 30]] = 2.0
    x[3] = -1.0
    assert _ids(x, 6) == [7, 30, 0, 1, 2, 4]
    assert _ids(x, 6, fault="tie_to_higher_id") != _ids(x, 6)


def test_plus_zero_sorts_directly_above_minus_zero():
    x = _b(0x8000, 0x0000, 0x8000, 0x0000, 0x8001, 0x0001)  # -0 +0 -0 +0 -tiny +tiny
    assert _ids(x, 6) == [5, 1, 3, 0, 2, 4]
    assert _ids(x, 6, fault="zeros_equal") == [5, 0, 1, 2, 3, 4]
    _, lps = tm.top_n(x, 6, *tm.lse_pair(x))
    assert lps[1] == lps[3] == lps[2]  # (as values the zeros are equal)


def test_minus_inf_entries_are_listed_with_minus_inf():
    x = _b(0xFC00, 0x3C00, 0xFC00, 0x4000)  # -inf 1 -inf 2
    ids, lps = tm.top_n(x, 4, *tm.lse_pair(x))
    assert ids.tolist() == [3, 1, 0, 2]
    assert np.isfinite(lps[:2]).all() and (lps[2:] == -np.inf).all()


def test_nan_logits_of_both_signs_are_not_listed():
    x = _b(0x7E00, 0x3C00, 0xFE00, 0x7C01, 0xFFFF, 0xC000)  # NaN 1 -NaN NaN -NaN -2
    assert _ids(x, 4) == [1, 5, -1, -1]
    assert _ids(x, 4, fault="nan_listed") != _ids(x, 4)
    assert _ids(_b(0x7E00, 0xFE00), 2) == [-1, -1]


def test_a_vocabulary_shorter_than_n_is_filled():
    x = _b(0x3C00, 0x4000, 0x3800)
    ids, lps = tm.top_n(x, 5, *tm.lse_pair(x))
    assert ids.tolist() == [1, 0, 2, -1, -1] and ids.dtype == np.int32 and lps.dtype == np.float32
    assert np.isfinite(lps[:3]).all() and (lps[3:] == -np.inf).all()
    assert _ids(x, 5, fault="short_filled_with_0") == [1, 0, 2, 0, 0]
    for n in (0, 21):
        with pytest.raises(AssertionError, match="GQ_EINVAL"):
            tm.top_n(x, n, 0.0, 0.0)


def test_the_logprob_is_lp_raws_two_subtractions():
    # v = 1, M = 2^12, L = 2^-13 + 2^-20: (v - M) = -4095 exactly, -4095 - L rounds on 2^-12 spacing; M + L rounds L away first
    M, L = np.float32(4096.0), np.float32(2.0**-13 + 2.0**-20)
    x = _b(0x3C00)
    _, lps = tm.top_n(x, 1, M, L)
    assert lps[0] == np.float32(np.float32(np.float32(1.0) - M) - L)
    assert lps[0] != tm.top_n(x, 1, M, L, fault="one_subtraction")[1][0]
    # the pair a host forms: the exact maximum, the log-sum of the rest
    x = sm.profile("gauss", 3000)
    M, L = tm.lse_pair(x)
    assert M == x.astype(np.float32).max() and L >= 0.0


def test_the_row_rule():
    assert tm.row(None, 4) == 0 and tm.row(None, 0) is None
    assert tm.row(0, 4) == 1 and tm.row(2, 4) == 3 and tm.row(3, 4) is None and tm.row(-1, 4) == 0 and tm.row(-2, 4) is None
    assert tm.row(2, 4, fault="row_p") == 2


def test_every_fault_is_listed():
    import inspect
    src = inspect.getsource(tm)
    for f in tm.FAULTS:
        assert src.count('"%s"' % f) >= 2, f
