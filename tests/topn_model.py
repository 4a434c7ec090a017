"""Host model of the top-n alternatives gq_sample_topk_lp_topn / gq_sample_full_topn leave next to a draw (include/gq_hip.h), in numpy.
Like tests/sampler_lp_model.py it restates the CONTRACT, not the kernels: no slices, candidates or workspaces appear here.

One step
  row       i = p + 1 with p = *pos_io before the draw's increment (the index seq_out and lp_raw use); pos_io NULL: i = 0.  The two rows are
            written when i < cap, nothing else is touched (`row`)
  order     the RAW order: the fp16 logit descending AS A BIT PATTERN (sampler_model.order_key: -0 directly below +0), the token id
            ascending among equal patterns; a NaN of either sign is not listed (`raw_order`).  Nothing but the logits enters: no ban list,
            no token set, no penalty, no temperature, no filter -- the model has no such arguments
  ids[j]    the first n tokens of the order; -1 from the first place the vocabulary cannot fill
  lps[j]    fl32(fl32(v - M) - L), v the fp16 logit widened to fp32, (M, L) the two fp32 numbers lp_raw of the step is taken against
            (its maximum and its log of the sum): lp_raw's own two subtractions, so a drawn token that is listed has lps[j] == lp_raw,
            bit for bit.  -inf for a place that holds -1.  (M, L) are INPUTS of `top_n`: a device run hands over the pair it formed
            (the test hook of the workspace), and the model says what ids and bits follow.  `lse_pair` is the host's own pair -- the exact
            maximum and the float64 log-sum rounded once -- for the comparison against float64 on the CPU
  grant     what lp_raw is granted against float64 (tests/test_sampler_lp_gpu.py): 4 * max(ref_err(logits), ulp32(|lse|)), ref_err the error
            of torch's CPU fp32 log_softmax on the same logits.  The list's entries are lp_raw's expression on other tokens of the same
            logits, so the same grant holds for every finite one (`grant`)
n is 1..MAX_N.  Logits with +inf or a NaN, or all -inf: the log-probabilities are the same expression's whatever it gives (lp_raw is
unspecified there); the ids are specified always.

`fault=` injects one deviation (FAULTS), for tests/test_topn_model_cpu.py only.
"""
import numpy as np

import sampler_lp_model as lp
import sampler_model as sm

MAX_N = 20
FAULTS = ("tie_to_higher_id", "zeros_equal", "nan_listed", "row_p", "one_subtraction", "short_filled_with_0")


def raw_order(logits, fault=None):
    """token ids in the raw order, NaN logits left out"""
    bits = np.ascontiguousarray(logits, dtype=np.float16).view(np.uint16)
    key = sm.order_key(bits)
    if fault == "zeros_equal":  # ordered as VALUES: -0 == +0, the id decides
        key = np.where(bits == 0x8000, sm.order_key(np.uint16(0)), key)
    ids = np.arange(bits.size, dtype=np.int64)
    if fault != "nan_listed":
        live = (bits & 0x7FFF) <= 0x7C00
        ids, key = ids[live], key[live]
    return ids[np.lexsort((ids if fault != "tie_to_higher_id" else -ids, -key))]


def lse_pair(logits):
    """(M, L) as fp32 numbers formed on the host: the exact maximum and the float64 log of sum exp(v - M), rounded once"""
    v = np.ascontiguousarray(logits, dtype=np.float16).astype(np.float64)
    M = v.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(M), np.float32(np.log(np.exp(v - M).sum()))


def top_n(logits, n, M, L, fault=None):
    """(ids int32 [n], lps float32 [n]) of one step"""
    assert 1 <= n <= MAX_N, "GQ_EINVAL"
    x = np.ascontiguousarray(logits, dtype=np.float16)
    order = raw_order(x, fault)[:n]
    ids = np.full(n, 0 if fault == "short_filled_with_0" else -1, dtype=np.int32)
    lps = np.full(n, -np.inf, dtype=np.float32)
    ids[:order.size] = order
    v = x[order].astype(np.float32)
    M, L = np.float32(M), np.float32(L)
    with np.errstate(invalid="ignore", over="ignore"):
        if fault == "one_subtraction":  # v - lse with lse = fl32(M + L): one rounding of the sum in place of lp_raw's two differences
            lps[:order.size] = v - np.float32(M + L)
        else:
            lps[:order.size] = (v - M).astype(np.float32) - L
    return ids, lps


def row(pos, cap, fault=None):
    """the row a step at position `pos` (None: no pos_io) writes, or None"""
    i = 0 if pos is None else pos + (0 if fault == "row_p" else 1)
    return i if 0 <= i < cap else None


def top_n64(logits, n):
    """float64 reference of a list: (ids, lps) with lps = v - lse64 over all logits, -inf / -1 where the vocabulary cannot fill"""
    x = np.ascontiguousarray(logits, dtype=np.float16)
    order = raw_order(x)[:n]
    ids = np.full(n, -1, dtype=np.int64)
    lps = np.full(n, -np.inf, dtype=np.float64)
    ids[:order.size] = order
    lps[:order.size] = x[order].astype(np.float64) - lp.lse64(x.astype(np.float32))
    return ids, lps


def grant(logits):
    """lp_raw's grant against float64 on these logits: 4 * max(ref_err, ulp32(|lse|)) (tests/test_sampler_lp_gpu.py: FACTOR, _bound)"""
    x32 = np.ascontiguousarray(logits, dtype=np.float16).astype(np.float32)
    return 4.0 * max(lp.ref_err(x32), lp.ulp32(lp.lse64(x32)))
