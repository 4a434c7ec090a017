"""CPU: the host side of top_logprobs -- FusedSampler's validation, tensors and entry-point rule with a stub in place of the library
(tests/test_fused_sampler_cpu.py's), and AnyPrecisionForCausalLM.generate's handling of the keyword on a host model: what it refuses,
and that it never reaches transformers' generate."""
import pytest

torch = pytest.importorskip("torch")

V = 70


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
    s.launch(torch.zeros(V, dtype=torch.float16), *io)


@pytest.mark.parametrize("top_k,entry", [(8, "gq_sample_topk_lp"), (0, "gq_sample_full")])
def test_entry_point_and_tensors(stub, top_k, entry):
    from guidedquant_amd import _lib
    plain = _sampler(top_k, seq_capacity=16, logprobs=True)
    zero = _sampler(top_k, seq_capacity=16, logprobs=True, top_logprobs=0)
    for s in (plain, zero):  # n = 0, the default: what it called, nothing allocated
        assert s.top_logprobs == 0 and s.top_ids is s.top_lps is s.topn_ws is None
        _launch(s)
    (name0, args0), (name1, args1) = stub.calls
    assert name0 == name1 == entry and len(args0) == len(args1)
    del stub.calls[:]
    s = _sampler(top_k, seq_capacity=16, logprobs=True, top_logprobs=5)
    assert s.top_logprobs == 5 and s.top_ids.shape == s.top_lps.shape == (16, 5) and s.top_ids.dtype == torch.int32 and s.top_lps.dtype == torch.float32
    assert s.top_ids.is_contiguous() and s.top_lps.is_contiguous() and s.topn_ws.numel() * 8 == _lib.TOPN_WS_BYTES == 16 + 128 * 20 * 8
    _launch(s)
    (name, args), = stub.calls
    assert name == entry + "_topn" and len(args) == len(args0) + 4
    assert args[-5:] == (5, s.top_ids.data_ptr(), s.top_lps.data_ptr(), s.topn_ws.data_ptr(), None)
    assert args[-6] == 16 and args[-8] == s.lp_raw.data_ptr()  # (.., lp_raw, lp_drawn, lp_cap, then the four)


def test_validation(stub):
    for n in (-1, 21, 1.5, "5", True):
        with pytest.raises((ValueError, TypeError)):
            _sampler(seq_capacity=16, logprobs=True, top_logprobs=n)
    with pytest.raises(ValueError, match="top_logprobs needs the log-probabilities"):
        _sampler(seq_capacity=16, top_logprobs=5)
    with pytest.raises(ValueError, match="seq_capacity"):
        _sampler(logprobs=True, top_logprobs=5)
    for n in (1, 20):
        assert _sampler(seq_capacity=4, logprobs=True, top_logprobs=n).top_ids.shape == (4, n)
    assert _sampler(seq_capacity=4, logprobs=True, top_logprobs=None).top_logprobs == 0
    assert stub.calls == []


def test_generate_pops_the_keyword_and_refuses_on_the_host(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    from ap_helpers import tiny_hf_anyprec_checkpoint
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM, GenerateLogprobsOutput
    tiny_hf_anyprec_checkpoint(tmp_path)
    m = AnyPrecisionForCausalLM.from_quantized(str(tmp_path), device="cpu")
    ids = torch.tensor([[3, 17, 5]])
    seen = []
    monkeypatch.setattr(m.model, "generate", lambda *a, **k: seen.append(dict(k)) or ids)
    base = dict(max_new_tokens=3, do_sample=False, pad_token_id=0)
    # None is the call without the keyword: transformers' generate runs on a host model, and never sees it
    assert m.generate(ids, top_logprobs=None, **base) is ids
    assert len(seen) == 1 and "top_logprobs" not in seen[0] and "output_logprobs" not in seen[0] and seen[0]["max_new_tokens"] == 3
    del seen[:]
    prec = m.precision
    for kw in (dict(top_logprobs=5), dict(top_logprobs=5, output_logprobs=False), dict(top_logprobs=0, output_logprobs=True),
               dict(top_logprobs=21, output_logprobs=True), dict(top_logprobs=1.5, output_logprobs=True),
               dict(top_logprobs=5, output_logprobs=True),                   # (a host model: route 1 needs the GPU -- refused, not dropped)
               dict(top_logprobs=5, output_logprobs=True, native=False), dict(top_logprobs=5, output_logprobs=True, capture=True),
               dict(top_logprobs=5, output_logprobs=True, precision=2)):
        with pytest.raises(ValueError):
            m.generate(ids, **dict(base, **kw))
        assert m.precision == prec
    assert seen == []
    # the output type: both fields None (and no keys) unless given
    out = GenerateLogprobsOutput(sequences=ids, logprobs=torch.zeros(1, 3), sampled_logprobs=torch.zeros(1, 3))
    assert list(out.keys()) == ["sequences", "logprobs", "sampled_logprobs"] and out.top_logprobs is None and out.top_logprobs_ids is None
    out = GenerateLogprobsOutput(sequences=ids, logprobs=torch.zeros(1, 3), sampled_logprobs=torch.zeros(1, 3), top_logprobs_ids=torch.zeros(1, 3, 2, dtype=torch.long),
                                 top_logprobs=torch.zeros(1, 3, 2))
    assert list(out.keys())[3:] == ["top_logprobs_ids", "top_logprobs"]
