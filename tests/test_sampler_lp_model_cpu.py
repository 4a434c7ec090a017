"""CPU: the host model of gq_sample_topk_lp's two outputs (tests/sampler_lp_model.py), and the export / argument checks of the entry.

(a) every fault of sampler_lp_model.FAULTS moves at least one number of at least one committed case by more than 1e-3 (the model is
    teacher-forced with the contract's own tokens -- sampler_rep_model.run -- as a device run would force it);
(b) sum_t exp(lp_raw_t) = 1 over a vocabulary; a single candidate gives exactly 0; an empty candidate set gives NaN; a slot at or past
    lp_cap is not written; -inf logits contribute nothing;
(c) ref_err is a small positive number on the profiles, 0 on one value;
(d) `_lib.EXPORTS` and include/gq_hip.h both name gq_sample_topk_lp, the library exports it and refuses bad arguments without a GPU.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import sampler_lp_model as lp
import sampler_model as sm
import sampler_rep_model as rm

# the committed cases each fault must show on (every one is a case of the GPU test as well)
FAULT_CASES = {
    "raw_without_banned": ("ban_argmax", "sup_argmax", "sup_ban_active"),
    "raw_penalised": ("values_rp1.3", "cut_k32"),
    "slot_p": ("v300_p", "ban_expires"),
    "drawn_no_temperature": ("v4096", "v32000_q32_p"),
    "drawn_no_nucleus": ("v300_p", "sup_nucleus_embed"),
    "drawn_over_vocab": ("v32000", "values_rp1.3"),
}


@functools.lru_cache(maxsize=None)
def _tokens(name):
    """the contract's own draws of a case (sampler_rep_model.run; rp = 1 and no sets for a case of sampler_model)"""
    c = lp.CASE_BY_NAME[name]
    x, kw = lp.case_args(c)
    r = rm.run(x, c.n, c.top_k, c.T, c.top_p, c.seed, c.counter, c.pos0, kw["ban"], c.seq_cap, kw.get("rp", 1.0), kw.get("seen0", ()), kw.get("suppress", ()))
    return r.tokens


def _model(name, fault=None, lp_cap=None):
    c = lp.CASE_BY_NAME[name]
    x, kw = lp.case_args(c)
    return lp.run(x, _tokens(name), lp_cap=c.pos0 + c.n + 2 if lp_cap is None else lp_cap, fault=fault, **kw)


def _differs(a, b):
    if set(a.raw) != set(b.raw):
        return True
    for s in a.raw:
        for x, y in ((a.raw[s], b.raw[s]), (a.drawn[s], b.drawn[s])):
            if np.isnan(x) != np.isnan(y) or (not np.isnan(x) and abs(x - y) > 1e-3):
                return True
    return False


def test_the_fault_list_is_covered():
    assert set(FAULT_CASES) == set(lp.FAULTS)
    assert all(n in lp.CASE_BY_NAME for names in FAULT_CASES.values() for n in names)


@pytest.mark.parametrize("fault", lp.FAULTS)
def test_every_fault_is_caught_by_a_committed_case(fault):
    caught = [n for n in FAULT_CASES[fault] if _differs(_model(n), _model(n, fault=fault))]
    assert caught, fault
    # and the unfaulted model is a function of its inputs
    n = FAULT_CASES[fault][0]
    assert not _differs(_model(n), _model(n))


def test_raw_logprobs_sum_to_one():
    for prof, V in (("gauss", 300), ("quant", 4096), ("ten_finite", 32000), ("negsub", 4096)):
        x = sm.profile(prof, V).astype(np.float64)
        assert abs(np.exp(x - lp.lse64(x)).sum() - 1.0) <= 1e-12, prof
    # through run(): both tokens of a two-token vocabulary, whatever the ban and the penalty do to the draw
    x = np.array([0.5, -1.25], dtype=np.float16)
    r = lp.run(x, [0, 1], top_k=2, T=0.7, rp=1.3, seen0=(0, ), lp_cap=8)
    assert abs(np.exp(r.raw[1]) + np.exp(r.raw[2]) - 1.0) <= 1e-12
    assert abs(np.exp(r.drawn[1]) + np.exp(lp.run(x, [1], top_k=2, T=0.7, rp=1.3, seen0=(0, ), lp_cap=8).drawn[1]) - 1.0) <= 1e-6
    # a -inf logit contributes 0
    y = np.array([0.5, -np.inf, -1.25], dtype=np.float16)
    assert lp.run(y, [0], top_k=3, T=1.0, lp_cap=8).raw[1] == pytest.approx(r.raw[1], abs=1e-15)


def test_single_candidate_empty_set_and_the_slots():
    x = sm.profile("gauss", 300)
    top = int(sm.candidates(x, 1)[0])
    r = lp.run(x, [top] * 3, top_k=1, T=1.0, pos=4, lp_cap=7)
    assert sorted(r.drawn) == [5, 6] and all(v == 0.0 for v in r.drawn.values())  # (slot 7 = lp_cap: not written)
    assert [d.slot for d in r.draws] == [5, 6, None]
    assert all(np.isfinite(v) and v < 0 for v in r.raw.values())
    # greedy with a unique maximum: the temperature leaves one candidate that matters, the kept set is still top_k wide
    g = lp.run(x, [top], top_k=50, T=0.0, lp_cap=4)
    assert g.drawn[1] <= 0.0 and g.drawn[1] > -1e-30 and len(g.draws[0].ids) == 50
    # everything suppressed: the token is EMPTY_TOKEN, both numbers are NaN, the slot is written
    e = lp.run(x, [lp.EMPTY_TOKEN], top_k=50, T=1.0, suppress=range(300), lp_cap=4)
    assert np.isnan(e.raw[1]) and np.isnan(e.drawn[1])
    # a nucleus on the threshold is not decided; one far from it is
    c = sm.CASE_BY_NAME["equal_k2_p_half"]
    assert not any(d.decided for d in _model(c.name).draws)
    assert all(d.decided for d in _model("v300_p").draws)
    assert not lp.specified(np.array([1.0, np.inf], dtype=np.float16)) and not lp.specified(np.array([-np.inf] * 3, dtype=np.float16))
    assert lp.specified(sm.profile("ten_finite", 300))


def test_ref_err_is_the_fp32_softmax_error():
    pytest.importorskip("torch")
    assert lp.ref_err(np.array([1.5], dtype=np.float16)) == 0.0
    for prof, V in (("gauss", 4096), ("quant", 32000), ("ten_finite", 32000)):
        e = lp.ref_err(sm.profile(prof, V))
        assert 0.0 < e < 1e-4, (prof, e)
    assert lp.ulp32(12.0) == 2.0**-20 and lp.ulp32(-1.0) == 2.0**-23


def test_exports_header_and_argument_checks_without_a_gpu():
    from guidedquant_amd import _lib
    assert "gq_sample_topk_lp" in _lib.EXPORTS
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gq_hip.h")
    assert "int gq_sample_topk_lp(" in open(header).read()
    L = _lib.lib()
    assert hasattr(L, "gq_sample_topk_lp") and _lib.SAMPLER_LP_WS == 2 * sm.BLOCKS
    buf = (ctypes.c_int * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # (host memory: every call below is refused before anything is launched)

    def call(V=300, top_k=50, rp=1.05, seen=p, ws=p, raw=p, drawn=p):
        return L.gq_sample_topk_lp(p, V, top_k, 1.0, 1.0, 7, p, p, p, p, p, p, None, None, 0, None, None, 0, None, rp, seen, None, ws, raw, drawn, 4, None)

    assert call(ws=None) == _lib.GQ_EINVAL and b"lp_ws" in L.gq_last_error()
    assert call(ws=None, raw=None, top_k=65) == _lib.GQ_ENOTSUP  # (lp_drawn alone needs no workspace: refused for top_k only)
    assert call(top_k=65) == _lib.GQ_ENOTSUP and call(V=262145) == _lib.GQ_ENOTSUP
    assert call(raw=None, drawn=None, top_k=65) == _lib.GQ_ENOTSUP
    assert call(rp=0.0) == _lib.GQ_EINVAL and call(rp=float("inf")) == _lib.GQ_EINVAL and call(rp=1.05, seen=None) == _lib.GQ_EINVAL
