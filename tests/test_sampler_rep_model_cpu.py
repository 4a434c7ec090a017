"""CPU: the host model of gq_sample_topk_rep (tests/sampler_rep_model.py), the exports and argument checks of the two new entry points,
and the routing of repetition_penalty / suppress_tokens on the HF surface.

(a) with rp = 1 and no sets the model IS sampler_model.run, token for token, on every committed `ex` / `p` case of sampler_model.CASES;
(b) every fault of sampler_rep_model.FAULTS changes at least one decided draw of at least one committed case (the faulted model is
    teacher-forced with the contract's own tokens, as a device run would be);
(c) the model alone leaves at most 5 % of a case's draws and 2 % of all draws undecided -- the caps of the existing sampler tests,
    conditions on the cases, not measurements -- and no nucleus threshold closer than 1e-5 to a cumulative sum;
(d) libgq_hip.so exports both symbols and refuses bad arguments without a GPU;
(e) _route_request, asked as generate() asks it (sampler_processors=True), accepts a penalty and a flat suppress list and still declines
    the rest; the two-argument form answers as it always did.
"""
import ctypes
import functools

import numpy as np
import pytest

import sampler_model as sm
import sampler_rep_model as rm


@functools.lru_cache(maxsize=None)
def _run(name):
    return rm.case_run(rm.CASE_BY_NAME[name])


@pytest.mark.parametrize("name", [c.name for c in sm.CASES if c.entry in ("ex", "p")])
def test_without_penalty_and_sets_the_model_is_the_old_model(name):
    c = sm.CASE_BY_NAME[name]
    x, ban = sm.case_inputs(c)
    old = sm.run(x, c.n, c.top_k, c.T, c.top_p, c.seed, c.counter, c.pos0, ban, c.seq_cap)
    new = rm.run(x, c.n, c.top_k, c.T, c.top_p, c.seed, c.counter, c.pos0, ban, c.seq_cap, rp=1.0)
    assert np.array_equal(old.tokens, new.tokens)
    assert np.array_equal(old.undecided, new.undecided)
    assert all(sorted(a.tolist()) == sorted(b.tolist()) for a, b in zip(old.admissible, new.admissible))
    assert (old.counter, old.pos, old.tok, old.seq) == (new.counter, new.pos, new.tok, new.seq)
    assert np.array_equal(new.seen, rm.token_set(new.tokens, c.V))
    i = int(np.argmax(new.undecided)) if new.undecided.any() else 0
    for t in new.admissible[i]:
        assert old.margin_to(i, int(t)) == pytest.approx(new.margin_to(i, int(t)), rel=1e-12, abs=0)


def test_token_set_layout():
    w = rm.token_set([0, 31, 32, 32, 299, 300, -1, 10**6], 300)
    assert w.dtype == np.uint32 and w.size == 10
    assert w[0] == 0x80000001 and w[1] == 1 and w[9] == 1 << (299 & 31) and int(w[2:9].sum()) == 0
    assert np.array_equal(rm.token_set([5], 300, base=w), w | np.where(np.arange(10) == 0, np.uint32(32), np.uint32(0)))


def test_the_penalty_formula():
    v = np.array([3.0, -2.0, 0.0, -0.0, np.inf, -np.inf, 2.0**-24, -2.0**-24], dtype=np.float16).astype(np.float32)
    for rp in rm.RPS:
        s = rm.penalised(v, rp)
        r = np.float32(rp)
        assert s.dtype == np.float32
        assert s[0] == np.float32(3.0) / r and s[1] == np.float32(-2.0) * r and s[4] == np.inf and s[5] == -np.inf
        assert s[2] == 0 and not np.signbit(s[2]) and s[3] == 0 and np.signbit(s[3])  # (-0 is not < 0: divided, and stays -0)
        assert s[6] == np.float32(2.0**-24) / r and s[7] == np.float32(-2.0**-24) * r
    # 1 / 1.05 in fp32 is no fp16 value, and a true division differs from the product with the reciprocal somewhere on the fp16 grid
    assert np.float32(np.float16(rm.penalised(np.float32([1.0]), 1.05)[0])) != rm.penalised(np.float32([1.0]), 1.05)[0]
    grid = np.arange(0x0400, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    assert (grid / np.float32(1.05) != grid * (np.float32(1.0) / np.float32(1.05))).any()
    assert rm.image32(np.float32([-0.0]))[0] + 1 == rm.image32(np.float32([0.0]))[0]


def test_the_cases_are_what_their_names_say():
    lo, hi = rm._LO, rm._HI
    s = float(np.float32(1.0) / np.float32(1.05))
    assert lo < s < hi and float(np.nextafter(np.float16(lo), np.float16(2))) == hi
    r = _run("between_fp16_k2")
    assert r.candidates0.tolist() == [20, 10]  # (the fp16 neighbour above, then the penalised token; the neighbour below is cut)
    assert _run("between_fp16_greedy").tokens.tolist()[:2] == [20, 10]
    assert _run("tie_seen_lower").tokens[0] == 40 and _run("tie_seen_higher").tokens[0] == 40  # (the lower id, seen or not)
    for k in (1, 32, 33, 64):  # the penalised arg-max is out, token number k + 1 of the plain order is in
        c = rm.CASE_BY_NAME["cut_k%d" % k]
        plain = sm.candidates(rm.case_logits(c), 64 if k == 64 else k + 1)
        top = np.lexsort((np.arange(c.V), -sm.order_key(rm.case_logits(c).view(np.uint16))))[:k + 1]
        assert plain[0] == top[0]
        assert _run(c.name).candidates0.tolist() == top[1:].tolist()
    for name in ("state_v300", "state_v131073"):
        assert _run(name).tokens.tolist() == list(range(300)) and not _run(name).undecided.any()
    assert set(_run("sup_all_but_one").tokens.tolist()) == {137}
    assert set(_run("layout_sup_v1").tokens.tolist()) == {rm.EMPTY_TOKEN} and not _run("layout_sup_v1").seen.any()
    assert set(_run("layout_sup_v2").tokens.tolist()) == {1}
    for c in rm.CASES:
        x, seen0, suppress, ban = rm.case_inputs(c)
        assert not set(_run(c.name).tokens.tolist()) & set(suppress), c.name
    assert _run("values_plus_inf").tokens.tolist() == [7] * 16
    assert {c.V for c in rm.CASES} >= {1, 2, 33, 300, 4096, 131072, 131073, 151936, 262144}
    assert max(rm.layout_ids(151936)) == 151935 and 131072 in rm.layout_ids(151936) and {0, 31, 32} <= set(rm.layout_ids(151936))
    assert all(c.n <= (300 if c.V > 32000 else 1000) for c in rm.CASES)


@pytest.mark.parametrize("fault", rm.FAULTS)
def test_every_fault_changes_a_decided_draw(fault):
    hit = []
    for c in rm.CASES:
        good = _run(c.name)
        bad = rm.case_run(c, forced=good.tokens, fault=fault)
        dec = ~good.undecided
        if (bad.tokens[dec] != good.tokens[dec]).any():
            hit.append(c.name)
            break
    assert hit, fault


def test_teacher_forcing_with_the_models_own_tokens_changes_nothing():
    for name in ("values_rp1.3", "sup_ban_expires", "cut_k33"):
        good = _run(name)
        again = rm.case_run(rm.CASE_BY_NAME[name], forced=good.tokens)
        assert np.array_equal(good.tokens, again.tokens) and np.array_equal(good.seen, again.seen) and good.seq == again.seq


def test_undecided_share_and_nucleus_boundaries():
    tot = und = 0
    for c in rm.CASES:
        r = _run(c.name)
        assert float(r.undecided.mean()) <= 0.05, (c.name, float(r.undecided.mean()))
        assert r.boundary_dist >= 1e-5, (c.name, r.boundary_dist)
        tot += c.n
        und += int(r.undecided.sum())
    assert und <= 0.02 * tot, (und, tot)


def test_exports_and_argument_checks_without_a_gpu():
    from guidedquant_amd import _lib
    L = _lib.lib()
    for name in ("gq_token_set_build", "gq_sample_topk_rep"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    buf = (ctypes.c_int * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # (host memory: every call below is refused before anything is launched)

    def call(V=300, top_k=50, rp=1.05, seen=p):
        return L.gq_sample_topk_rep(p, V, top_k, 1.0, 1.0, 7, p, p, p, p, p, p, None, None, 0, None, None, 0, None, rp, seen, None, None)

    assert call(rp=0.0) == _lib.GQ_EINVAL and call(rp=float("nan")) == _lib.GQ_EINVAL and call(rp=-1.0) == _lib.GQ_EINVAL
    assert call(rp=float("inf")) == _lib.GQ_EINVAL
    assert call(rp=1.05, seen=None) == _lib.GQ_EINVAL
    assert call(top_k=65) == _lib.GQ_ENOTSUP and call(V=262145) == _lib.GQ_ENOTSUP
    assert b"repetition_penalty" in L.gq_last_error() or call(rp=0.0) and b"repetition_penalty" in L.gq_last_error()
    assert L.gq_token_set_build(None, 0, 300, None, 1, None) == _lib.GQ_EINVAL
    assert L.gq_token_set_build(None, 3, 300, p, 1, None) == _lib.GQ_EINVAL
    assert L.gq_token_set_build(None, 0, 300, p, 0, None) == 0  # (nothing to do: no launch)


def test_route_request_takes_a_penalty_and_a_suppress_list(tmp_path):
    pytest.importorskip("transformers")
    import torch
    from ap_helpers import tiny_hf_anyprec_checkpoint
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    tiny_hf_anyprec_checkpoint(tmp_path)
    m = AnyPrecisionForCausalLM.from_quantized(str(tmp_path), device="cpu")
    ids = torch.tensor([[3, 17, 5]])
    req, why = m._route_request((ids, ), dict(max_new_tokens=4, repetition_penalty=1.05, suppress_tokens=[3, 7]), sampler_processors=True)
    assert why is None and req["repetition_penalty"] == 1.05 and req["suppress_tokens"] == (3, 7)
    req, why = m._route_request((ids, ), dict(max_new_tokens=4))
    assert why is None and req["repetition_penalty"] == 1.0 and req["suppress_tokens"] == ()
    # the two-argument form: what a caller without the token sets can serve, as before
    assert m._route_request((ids, ), dict(max_new_tokens=4, repetition_penalty=1.05))[0] is None
    assert m._route_request((ids, ), dict(max_new_tokens=4, suppress_tokens=[3]))[0] is None
    V = m.config.vocab_size
    for kw in (dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
               dict(suppress_tokens=[[3, 7]]), dict(suppress_tokens=[V]), dict(suppress_tokens=[-1]), dict(suppress_tokens=[1.5]),
               dict(no_repeat_ngram_size=2), dict(begin_suppress_tokens=[3])):
        req, why = m._route_request((ids, ), dict(max_new_tokens=4, **kw), sampler_processors=True)
        assert req is None and why, kw
    # from the generation config, as the published Qwen2.5-Instruct one carries it
    keep = m.model.generation_config
    try:
        import types
        m.model.generation_config = types.SimpleNamespace(repetition_penalty=1.05, top_k=20, top_p=0.8, temperature=0.7, do_sample=True, suppress_tokens=[5])
        req, why = m._route_request((ids, ), dict(max_new_tokens=4), sampler_processors=True)
        assert why is None and (req["repetition_penalty"], req["top_k"], req["top_p"], req["temperature"], req["suppress_tokens"]) == (1.05, 20, 0.8, 0.7, (5, ))
        m.model.generation_config = types.SimpleNamespace(no_repeat_ngram_size=2)
        assert m._route_request((ids, ), dict(max_new_tokens=4), sampler_processors=True)[0] is None
        m.model.generation_config = types.SimpleNamespace(suppress_tokens=[[1, 2]])
        assert m._route_request((ids, ), dict(max_new_tokens=4), sampler_processors=True)[0] is None
    finally:
        m.model.generation_config = keep
