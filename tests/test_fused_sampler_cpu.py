"""CPU: the rule by which guidedquant_amd.fused_sampler.FusedSampler picks the sampler's C entry point, which optional tensors it
allocates, and what it refuses -- with a stub in place of the library that only records the calls (no kernel runs, no GPU)."""
import itertools

import pytest

torch = pytest.importorskip("torch")

V = 70  # (3 words of 32 bits)


class _Stub:
    """every entry point returns 0 and is noted as (name, arguments)"""

    def __init__(self):
        self.calls = []

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


def _sampler(**kw):
    from guidedquant_amd.fused_sampler import FusedSampler
    return FusedSampler(V, "cpu", 8, **dict(dict(top_p=0.9, temperature=0.7, seed=11), **kw))


def _launch(s):
    io = [torch.zeros(1, dtype=torch.int32) for _ in range(3)]
    logits = torch.zeros(V, dtype=torch.float16)
    s.launch(logits, *io)
    return logits, io


@pytest.mark.parametrize("penalty,suppress,logprobs", list(itertools.product((False, True), repeat=3)))
def test_entry_point_and_optional_tensors(stub, penalty, suppress, logprobs):
    s = _sampler(seq_capacity=16 if logprobs else 0, repetition_penalty=1.3 if penalty else 1.0, suppress_tokens=[3, 69] if suppress else (),
                 logprobs=logprobs)
    sets = penalty or suppress
    # what exists: the four words every draw needs, and nothing else unless it was asked for
    assert s.counter.shape == (1, ) and s.ban.shape == (6, ) and s.work_val.shape == s.work_idx.shape == (128 * 64, )
    assert (s.seen is not None) == sets and (s.suppress is not None) == suppress and (s.seq is not None) == logprobs
    assert all((t is not None) == logprobs for t in (s.lp_ws, s.lp_raw, s.lp_drawn))
    if sets:
        assert s.seen.shape == ((V + 31) // 32, ) and s.seen.dtype == torch.int32
    # the suppress list is built once, in the constructor; nothing else is launched there
    assert [c[0] for c in stub.calls] == (["gq_token_set_build"] if suppress else [])
    if suppress:
        assert stub.calls[0][1][1:5] == (2, V, s.suppress.data_ptr(), 1)
    del stub.calls[:]
    logits, (tok, pos, nxt) = _launch(s)
    (name, args), = stub.calls
    assert name == ("gq_sample_topk_lp" if logprobs else "gq_sample_topk_rep" if sets else "gq_sample_topk_p")
    common = (logits.data_ptr(), V, 8, 0.9, 0.7, 11, s.counter.data_ptr(), s.work_val.data_ptr(), s.work_idx.data_ptr(), tok.data_ptr(), pos.data_ptr(),
              nxt.data_ptr(), s.ban.data_ptr(), s.seq.data_ptr() if logprobs else None, 16 if logprobs else 0, None, None, 0, None)
    rep = (1.3 if penalty else 1.0, s.seen.data_ptr() if sets else None, s.suppress.data_ptr() if suppress else None)
    lp = (s.lp_ws.data_ptr(), s.lp_raw.data_ptr(), s.lp_drawn.data_ptr(), 16) if logprobs else ()
    assert args == common + (rep if sets or logprobs else ()) + lp + (None, )


def test_a_plain_request_with_a_sequence_store_and_the_embedding_fold_stays_on_p(stub):
    s = _sampler(seq_capacity=9)
    emb, x, ssq = torch.zeros(V, 8, dtype=torch.float16), torch.zeros(8, dtype=torch.float16), torch.zeros(1024)
    io = [torch.zeros(1, dtype=torch.int32) for _ in range(3)]
    s.launch(torch.zeros(V, dtype=torch.float16), *io, emb, x, 8, ssq)
    (name, args), = stub.calls
    assert name == "gq_sample_topk_p" and args[13:19] == (s.seq.data_ptr(), 9, emb.data_ptr(), x.data_ptr(), 8, ssq.data_ptr())
    assert s.seen is s.suppress is s.lp_ws is s.lp_raw is s.lp_drawn is None


def test_a_workspace_of_32_candidates_makes_the_narrow_call(stub):
    s = _sampler(top_p=1.0, candidates=32)
    assert s.work_val.shape == s.work_idx.shape == (128 * 32, )
    nxt = torch.zeros(1, dtype=torch.int32)
    logits = torch.zeros(V, dtype=torch.float16)
    s.launch(logits, None, None, nxt)
    assert stub.calls == [("gq_sample_topk", (logits.data_ptr(), V, 8, 0.7, 11, s.counter.data_ptr(), s.work_val.data_ptr(), s.work_idx.data_ptr(), None, None,
                                              nxt.data_ptr(), None))]
    for extra in (dict(seq_capacity=4), dict(repetition_penalty=1.1), dict(suppress_tokens=[1]), dict(top_p=0.5)):
        with pytest.raises(ValueError, match="32 candidates"):
            _sampler(**dict(dict(top_p=1.0, candidates=32), **extra))


def test_the_two_refusals(stub):
    for rp in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="repetition_penalty must be finite and > 0"):
            _sampler(repetition_penalty=rp)
    with pytest.raises(ValueError, match="logprobs=True needs seq_capacity > 0"):
        _sampler(logprobs=True)
    assert stub.calls == []


def test_request_state_helpers(stub):
    s = _sampler(repetition_penalty=1.2, seq_capacity=8)
    s.set_ban([5, 6], 3)
    assert s.ban.tolist() == [2, 3, 5, 6, 0, 0]
    s.reseed(torch.tensor([41], dtype=torch.int32))
    assert s.counter.tolist() == [41]
    s.reseed(0)
    assert s.counter.tolist() == [0]
    s.set_history([1, 2, 3])
    s.build_set(s.seen, torch.tensor([4]), clear=False)
    assert [(n, a[1:5]) for n, a in stub.calls] == [("gq_token_set_build", (3, V, s.seen.data_ptr(), 1)), ("gq_token_set_build", (1, V, s.seen.data_ptr(), 0))]
    s.seen.fill_(7)
    s.clear_warmup()
    assert not s.seen.any()
    plain = _sampler()
    del stub.calls[:]
    plain.set_history([1, 2])  # (no set: nothing happens)
    plain.clear_warmup()
    assert stub.calls == []
