"""CPU: the host side of frequency_penalty / presence_penalty / logit_bias -- FusedSampler's validation, state and entry-point rule with a
stub in place of the library (tests/test_fused_sampler_cpu.py's), the C entries' refusals on host memory (refused before anything is
launched), and AnyPrecisionForCausalLM.generate's handling of the keywords on a host model: what it refuses, and that they never reach
transformers' generate."""
import ctypes
import itertools

import pytest

torch = pytest.importorskip("torch")

V = 70  # (3 words of 32 bits)


class _Stub:
    """every entry point returns 0 and is noted as (name, arguments)"""

    def __init__(self):
        self.calls = []

    def gq_sample_full_ws_bytes(self, vocab):
        return 4096

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def stub(monkeypatch):
    from guidedquant_amd import _lib
    s = _Stub()
    monkeypatch.setattr(_lib, "_lib", s)
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: None)
    return s


def _sampler(top_k=8, **kw):
    from guidedquant_amd.fused_sampler import FusedSampler
    return FusedSampler(V, "cpu", top_k, **dict(dict(top_p=0.9, temperature=0.7, seed=11), **kw))


def _launch(s):
    io = [torch.zeros(1, dtype=torch.int32) for _ in range(3)]
    logits = torch.zeros(V, dtype=torch.float16)
    s.launch(logits, *io)
    return logits, io


def _adj_of(arg):
    """the GqSampleAdjust a ctypes.byref argument points at"""
    return arg._obj


NEUTRAL = (dict(), dict(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None), dict(frequency_penalty=None, presence_penalty=None, logit_bias={}),
           dict(frequency_penalty=0, presence_penalty=-0.0))


@pytest.mark.parametrize("top_k", [8, 0])
@pytest.mark.parametrize("penalty,suppress,logprobs,top_n", [(p, s, l, n) for p, s, l in itertools.product((False, True), repeat=3) for n in ((0, 3) if l else (0, ))])
def test_neutral_arguments_make_the_old_calls(stub, top_k, penalty, suppress, logprobs, top_n):
    common = dict(seq_capacity=16 if logprobs else 0, repetition_penalty=1.3 if penalty else 1.0, suppress_tokens=[3, 69] if suppress else (), logprobs=logprobs,
                  top_logprobs=top_n)
    logs = []
    for kw in NEUTRAL:
        del stub.calls[:]
        s = _sampler(top_k, **common, **kw)
        assert not s.adjusted and s.bias_set is s.bias is s.out_set is s.out_count is None
        s.reset_generated()
        s.count_generated([1, 2])
        s.clear_warmup()
        built = [c[0] for c in stub.calls]
        del stub.calls[:]
        _launch(s)
        (name, args), = stub.calls
        logs.append((built, name, len(args)))
    assert all(entry == logs[0] for entry in logs), logs
    want = ("gq_sample_full" + ("_topn" if top_n else "")) if top_k == 0 else \
        ("gq_sample_topk_lp_topn" if top_n else "gq_sample_topk_lp" if logprobs else "gq_sample_topk_rep" if penalty or suppress else "gq_sample_topk_p")
    assert logs[0][1] == want and "gq_token_bias_build" not in logs[0][0]


@pytest.mark.parametrize("top_k,entry", [(8, "gq_sample_topk_adj"), (1, "gq_sample_topk_adj"), (64, "gq_sample_topk_adj"), (0, "gq_sample_full_adj"),
                                         (None, "gq_sample_full_adj"), (65, "gq_sample_full_adj")])
@pytest.mark.parametrize("active", [("fp", ), ("pp", ), ("bias", ), ("fp", "pp", "bias")])
@pytest.mark.parametrize("logprobs,top_n", [(False, 0), (True, 0), (True, 5)])
def test_any_of_the_three_selects_the_adjusted_entry(stub, top_k, entry, active, logprobs, top_n):
    kw = dict(frequency_penalty=0.5 if "fp" in active else 0.0, presence_penalty=-0.25 if "pp" in active else 0.0,
              logit_bias={"3": 1.5, 69: -2.0, 0: 0.0} if "bias" in active else None)
    s = _sampler(top_k, seq_capacity=16 if logprobs else 0, repetition_penalty=1.3, suppress_tokens=[4], logprobs=logprobs, top_logprobs=top_n, **kw)
    counted, biased = "fp" in active or "pp" in active, "bias" in active
    assert s.adjusted and s.full == (entry == "gq_sample_full_adj")
    # state only when asked for
    assert (s.bias_set is not None) == (s.bias is not None) == biased and (s.out_set is not None) == (s.out_count is not None) == counted
    words = (V + 31) // 32
    if biased:
        assert s.bias_set.shape == (words, ) and s.bias_set.dtype == torch.int32 and s.bias.shape == (V, ) and s.bias.dtype == torch.float32
        assert s.logit_bias == {3: 1.5, 69: -2.0, 0: 0.0}
    if counted:
        assert s.out_set.shape == (words, ) and s.out_count.shape == (V, ) and s.out_count.dtype == torch.int32
    built = [c for c in stub.calls if c[0] == "gq_token_bias_build"]
    assert len(built) == (1 if biased else 0)
    if biased:  # (ids, values, n, vocab, bias_set, bias, stream): one launch, in the constructor
        assert built[0][1][2:6] == (3, V, s.bias_set.data_ptr(), s.bias.data_ptr())
    del stub.calls[:]
    logits, (tok, pos, nxt) = _launch(s)
    (name, args), = stub.calls
    assert name == entry
    lp = (s.lp_raw.data_ptr(), s.lp_drawn.data_ptr(), 16) if logprobs else (None, None, 0)
    topn = (top_n, s.top_ids.data_ptr(), s.top_lps.data_ptr(), s.topn_ws.data_ptr()) if top_n else (0, None, None, None)
    tail = (tok.data_ptr(), pos.data_ptr(), nxt.data_ptr(), s.ban.data_ptr(), s.seq.data_ptr() if logprobs else None, 16 if logprobs else 0, None, None, 0, None,
            1.3, s.seen.data_ptr(), s.suppress.data_ptr())
    if s.full:
        assert args[:-2] == (logits.data_ptr(), V, int(top_k or 0), 0.9, 0.0, 0.7, 11, s.counter.data_ptr(), s.ws.data_ptr(), 4096) + tail + lp + topn
    else:
        assert args[:-2] == (logits.data_ptr(), V, top_k, 0.9, 0.7, 11, s.counter.data_ptr(), s.work_val.data_ptr(), s.work_idx.data_ptr()) + tail \
            + (s.lp_ws.data_ptr() if logprobs else None, ) + lp + topn
    assert args[-1] is None
    a = _adj_of(args[-2])
    assert (a.frequency_penalty, a.presence_penalty) == (kw["frequency_penalty"], kw["presence_penalty"])
    assert (a.bias_set, a.bias) == ((s.bias_set.data_ptr(), s.bias.data_ptr()) if biased else (None, None))
    assert (a.out_set, a.out_count) == ((s.out_set.data_ptr(), s.out_count.data_ptr()) if counted else (None, None))
    assert a is s._adj  # (the struct lives as long as the sampler: a captured launch has read it by then, a later one reads it again)


def test_request_state_helpers(stub):
    s = _sampler(frequency_penalty=0.5, repetition_penalty=1.2, seq_capacity=8)
    s.out_set.fill_(7)
    s.out_count.fill_(3)
    s.seen.fill_(5)
    s.set_history([1, 2, 3])  # (unchanged: the prompt does not count)
    assert (s.out_set == 7).all() and (s.out_count == 3).all()
    s.reset_generated()
    assert not s.out_set.any() and not s.out_count.any() and (s.seen == 5).all()
    s.out_set.fill_(7)
    s.out_count.fill_(3)
    s.clear_warmup()
    assert not s.out_set.any() and not s.out_count.any() and not s.seen.any()
    del stub.calls[:]
    s.count_generated(torch.tensor([[5]]))
    s.count_generated([5, 69])
    assert s.out_count[5] == 2 and s.out_count[69] == 1 and int(s.out_count.sum()) == 3
    assert [(n, a[1:5]) for n, a in stub.calls] == [("gq_token_set_build", (1, V, s.out_set.data_ptr(), 0)), ("gq_token_set_build", (2, V, s.out_set.data_ptr(), 0))]
    only_bias = _sampler(logit_bias={1: 1.0})
    only_bias.reset_generated()  # (no count: nothing happens)
    only_bias.count_generated([1])
    only_bias.clear_warmup()


def test_every_validation_error(stub):
    inf, nan = float("inf"), float("nan")
    for name in ("frequency_penalty", "presence_penalty"):
        for bad in (inf, -inf, nan, "0.5", True, [1.0], 1e39):
            with pytest.raises(ValueError, match=name + " must be a finite number"):
                _sampler(**{name: bad})
        assert getattr(_sampler(**{name: -1.5}), name) == -1.5  # (negative penalties are served)
    for bad, what in (([(1, 2.0)], "must be a dict"), ("x", "must be a dict"), ({-1: 1.0}, "outside"), ({V: 1.0}, "outside"), ({"70": 1.0}, "outside"),
                      ({1: inf}, "finite"), ({1: nan}, "finite"), ({1: 1e39}, "finite"), ({1: None}, "no \\(token id, number\\) pair"), ({"a": 1.0}, "no \\(token id"),
                      ({1.5: 1.0}, "no \\(token id"), ({True: 1.0}, "no \\(token id"), ({1: "x"}, "no \\(token id"), ({1: 1.0, "1": 2.0}, "listed twice")):
        with pytest.raises(ValueError, match="logit_bias.*" + what):
            _sampler(logit_bias=bad)
    # the 32-candidate workspace serves the draw alone
    for kw in (dict(frequency_penalty=0.1), dict(presence_penalty=0.1), dict(logit_bias={1: 1.0})):
        with pytest.raises(ValueError, match="32 candidates"):
            _sampler(**dict(dict(top_p=1.0, candidates=32), **kw))
    assert _sampler(top_p=1.0, candidates=32, frequency_penalty=0.0, logit_bias={}).narrow
    assert stub.calls == []


def test_exports_and_refusals_without_a_gpu():
    from guidedquant_amd import _lib
    L = _lib.lib()
    for name in ("gq_token_bias_build", "gq_sample_topk_adj", "gq_sample_full_adj"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    buf = (ctypes.c_int * 64)(*([0x7E7E7E7E] * 64))
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = L.gq_sample_full_ws_bytes(300)
    ws = (ctypes.c_char * (need + 16))(*([0x7E] * (need + 16)))
    wsp = ctypes.c_void_p((ctypes.addressof(ws) + 15) & ~15)
    inf, nan = float("inf"), float("nan")

    def topk(adj, top_n=0, V=300, top_k=8):
        return L.gq_sample_topk_adj(p, V, top_k, 1.0, 1.0, 7, p, p, p, p, p, p, None, None, 0, None, None, 0, None, 1.0, None, None, p, p, p, 4, top_n, p, p, p,
                                    ctypes.byref(adj) if adj is not None else None, None)

    def full(adj, top_n=0, V=300, top_k=0):
        return L.gq_sample_full_adj(p, V, top_k, 1.0, 0.0, 1.0, 7, p, wsp, need, p, p, p, None, None, 0, None, None, 0, None, 1.0, None, None, p, p, 4, top_n, p, p, p,
                                    ctypes.byref(adj) if adj is not None else None, None)
    A = _lib.GqSampleAdjust
    for call in (topk, full):
        for adj in (A(inf, 0.0, None, None, p, p), A(0.0, -inf, None, None, p, p), A(nan, 0.0, None, None, p, p), A(0.0, nan, p, p, p, p),  # not finite
                    A(0.0, 0.0, p, None, None, None), A(0.0, 0.0, None, p, None, None), A(0.0, 0.0, None, None, p, None), A(0.0, 0.0, None, None, None, p),  # half a pair
                    A(0.5, 0.0, None, None, None, None), A(0.0, -0.5, p, p, None, None)):  # a penalty without out_set
            assert call(adj) == _lib.GQ_EINVAL, (call.__name__, adj.frequency_penalty, adj.presence_penalty, adj.bias_set, adj.bias, adj.out_set, adj.out_count)
            assert L.gq_last_error()
        # then the refusals of the entry without the suffix, with its codes -- with an adjustment and without one
        for adj in (A(0.5, 0.5, p, p, p, p), None, A(0.0, 0.0, None, None, None, None)):
            assert call(adj, V=262145) == _lib.GQ_ENOTSUP
            assert call(adj, top_n=21) == _lib.GQ_EINVAL and call(adj, top_n=-1) == _lib.GQ_EINVAL
        assert topk(A(0.5, 0.5, p, p, p, p), top_k=65) == _lib.GQ_ENOTSUP and full(A(0.5, 0.5, p, p, p, p), top_k=-1) == _lib.GQ_EINVAL
    for a in ((p, p, 2, 300, None, p), (p, p, 2, 300, p, None), (None, p, 2, 300, p, p), (p, None, 2, 300, p, p), (p, p, 2, 0, p, p)):
        assert L.gq_token_bias_build(*a, None) == _lib.GQ_EINVAL
    assert all(b == 0x7E for b in ws.raw) and all(v == 0x7E7E7E7E for v in buf), "a refused call wrote something"


IDS = torch.tensor([[3, 17, 5]])


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    pytest.importorskip("transformers")
    from ap_helpers import tiny_hf_anyprec_checkpoint
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    path = tmp_path_factory.mktemp("tiny")
    tiny_hf_anyprec_checkpoint(path)
    return AnyPrecisionForCausalLM.from_quantized(str(path), device="cpu")


def test_route_request_does_not_know_the_keywords(model):
    """they are popped by `generate`: a caller that hands them to `_route_request` is told they lie outside the fused routes"""
    for k, v in (("frequency_penalty", 0.5), ("presence_penalty", 0.5), ("logit_bias", {1: 1.0})):
        assert k not in model._ROUTE_KW
        req, why = model._route_request((IDS, ), {"max_new_tokens": 4, k: v}, sampler_processors=True, full_sampler=True)
        assert req is None and k in why


def test_generate_pops_the_keywords_and_refuses_on_the_host(model, monkeypatch):
    seen = []
    monkeypatch.setattr(model.model, "generate", lambda *a, **k: seen.append(dict(k)) or IDS)
    base = dict(max_new_tokens=3, do_sample=False, pad_token_id=0)
    # neutral values are the call without the keywords: transformers' generate runs on a host model, and never sees them
    for kw in (dict(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None), dict(frequency_penalty=None, logit_bias={}), dict(presence_penalty=0)):
        assert model.generate(IDS, **base, **kw) is IDS
        assert len(seen) == 1 and not {"frequency_penalty", "presence_penalty", "logit_bias"} & set(seen[0]) and seen[0]["max_new_tokens"] == 3
        del seen[:]
    prec = model.precision
    for kw, name in ((dict(frequency_penalty=0.5), "frequency_penalty"), (dict(presence_penalty=-0.5), "presence_penalty"), (dict(logit_bias={"5": 2.0}), "logit_bias"),
                     (dict(presence_penalty=0.5, logit_bias={5: 2.0}), "presence_penalty"), (dict(frequency_penalty=0.5, presence_penalty=0.5), "frequency_penalty")):
        # a host model: route 1 needs the GPU -- refused under the keyword's name, not dropped; native=False and capture=True as well
        for route in (dict(), dict(native=True), dict(native=False), dict(capture=True), dict(precision=2), dict(do_sample=True, top_k=100), dict(num_beams=2)):
            with pytest.raises(ValueError, match="^" + name + ": "):
                model.generate(IDS, **dict(base, **route), **kw)
            assert model.precision == prec
    for kw, what in ((dict(frequency_penalty=float("inf")), "frequency_penalty must be a finite number"), (dict(presence_penalty="x"), "presence_penalty must be"),
                     (dict(logit_bias={10**6: 1.0}), "logit_bias: token id 1000000 is outside"), (dict(logit_bias=[1]), "logit_bias must be a dict"),
                     (dict(logit_bias={1: float("nan")}), "finite")):
        with pytest.raises(ValueError, match=what):
            model.generate(IDS, **base, **kw)
    assert seen == []


def test_decode_graph_refuses_the_keywords_without_native_sampling():
    """the torch-sampling graph never applies them: ValueError before anything is captured"""
    from guidedquant_amd.generate import DecodeGraph

    class _NoNative:
        def native_ready(self):
            return False
    for kw in (dict(frequency_penalty=0.5), dict(presence_penalty=0.5), dict(logit_bias={1: 1.0})):
        for native in (False, True):  # (True on a model without the fused step is the torch-sampling graph as well)
            with pytest.raises(ValueError, match="frequency_penalty / presence_penalty / logit_bias are served by the fused sampler only"):
                DecodeGraph(_NoNative(), "cpu", native_sampling=native, temperature=0.8, top_k=8, **kw)
