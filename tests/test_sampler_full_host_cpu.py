"""CPU: the host side of the whole-vocabulary sampler -- the C ABI's exports and refusals (host memory: refused before anything is
launched), `_route_request` with and without the `full_sampler` flag, and FusedSampler's choice of entry point for every configuration
(a stub in place of the library, as tests/test_fused_sampler_cpu.py)."""
import ctypes
import itertools
import types

import pytest

torch = pytest.importorskip("torch")

V = 70


def test_exports_and_refusals_without_a_gpu():
    from guidedquant_amd import _lib
    L = _lib.lib()
    for name in ("gq_sample_full", "gq_sample_full_ws_bytes"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    need = L.gq_sample_full_ws_bytes(300)
    assert need > 24 and L.gq_sample_full_ws_bytes(262144) >= need and L.gq_sample_full_ws_bytes(262145) == 0 and L.gq_sample_full_ws_bytes(1) > 24
    ws = (ctypes.c_char * (need + 16))(*([0x7E] * (need + 16)))
    base = ctypes.addressof(ws)
    wsp = ctypes.c_void_p((base + 15) & ~15)
    buf = (ctypes.c_int * 16)(*([0x7E7E7E7E] * 16))
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(V=300, top_k=0, top_p=1.0, min_p=0.0, rp=1.0, seen=None, ws=wsp, ws_bytes=need, logits=p, counter=p, nt=p, x_out=None, table=None, dim=0, ssq=None):
        return L.gq_sample_full(logits, V, top_k, top_p, min_p, 1.0, 7, counter, ws, ws_bytes, p, p, nt, None, None, 0, table, x_out, dim, ssq, rp, seen, None,
                                None, None, 0, None)
    assert call(V=262145) == _lib.GQ_ENOTSUP
    for kw in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0001), dict(top_p=float("nan")), dict(min_p=-0.01), dict(min_p=1.5),
               dict(min_p=float("nan")), dict(rp=1.05), dict(rp=0.0), dict(rp=float("inf")), dict(rp=float("nan"), seen=p), dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(ws=None), dict(logits=None), dict(counter=None), dict(nt=None), dict(ssq=p), dict(x_out=p, dim=8), dict(x_out=p, table=p, dim=12)):
        assert call(**kw) == _lib.GQ_EINVAL, kw
    assert L.gq_last_error()
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


# the requests tests/test_host_logic_cpu.py asks about, with the answers they always had (served or not)
OLD_REQUESTS = [
    (dict(max_new_tokens=4), True), (dict(max_new_tokens=4, do_sample=True, top_k=50), True), (dict(max_new_tokens=4, do_sample=True, top_k=64, top_p=0.9), True),
    (dict(max_new_tokens=4, do_sample=True, top_k=100), False), (dict(max_new_tokens=4, do_sample=True, top_k=0), False),
    (dict(max_new_tokens=4, do_sample=True, top_k=65), False), (dict(max_new_tokens=4, do_sample=True, min_p=0.05), False),
    (dict(max_new_tokens=4, num_beams=2), False), (dict(max_new_tokens=4, do_sample=True, top_p=0.0), False), (dict(max_new_tokens=4, typical_p=0.5), False),
]


@pytest.mark.parametrize("kw,served", OLD_REQUESTS)
def test_route_request_old_forms_answer_as_before(model, kw, served):
    for extra in (dict(), dict(sampler_processors=True)):
        req, why = model._route_request((IDS, ), dict(kw), **extra)
        assert (req is not None) == served and (why is None) == served, (kw, extra, why)
        if served:
            assert req["min_p"] == 0.0 and 1 <= req["top_k"] <= 64


def test_route_request_old_forms_decline_a_config_without_top_k(model):
    keep = model.model.generation_config
    try:
        model.model.generation_config = types.SimpleNamespace(do_sample=True, top_k=None, top_p=0.95, temperature=0.8)  # (transformers-4 style: None = off)
        assert model._route_request((IDS, ), dict(max_new_tokens=4))[0] is None
        assert model._route_request((IDS, ), dict(max_new_tokens=4), True)[0] is None
        req, why = model._route_request((IDS, ), dict(max_new_tokens=4), sampler_processors=True, full_sampler=True)
        assert why is None and (req["top_k"], req["top_p"], req["temperature"], req["min_p"]) == (0, 0.95, 0.8, 0.0)
        model.model.generation_config = types.SimpleNamespace(do_sample=True, min_p=0.05)
        assert model._route_request((IDS, ), dict(max_new_tokens=4), sampler_processors=True)[0] is None
        req, why = model._route_request((IDS, ), dict(max_new_tokens=4), sampler_processors=True, full_sampler=True)
        assert why is None and req["min_p"] == 0.05 and req["top_k"] == 50
        model.model.generation_config = types.SimpleNamespace(do_sample=True, min_p=1.5)
        assert model._route_request((IDS, ), dict(max_new_tokens=4), sampler_processors=True, full_sampler=True)[0] is None
    finally:
        model.model.generation_config = keep


def test_route_request_with_the_flag(model):
    def ask(**kw):
        return model._route_request((IDS, ), dict(max_new_tokens=4, do_sample=True, **kw), sampler_processors=True, full_sampler=True)
    req, why = ask(top_k=0, top_p=0.9)
    assert why is None and (req["top_k"], req["top_p"], req["min_p"]) == (0, 0.9, 0.0)
    req, why = ask(min_p=0.05)
    assert why is None and (req["top_k"], req["min_p"]) == (50, 0.05)
    req, why = ask(min_p=1.0, top_k=0, repetition_penalty=1.1, suppress_tokens=[5])
    assert why is None and (req["top_k"], req["min_p"], req["repetition_penalty"], req["suppress_tokens"]) == (0, 1.0, 1.1, (5, ))
    for kw in (dict(top_k=100), dict(top_k=65), dict(min_p=1.5), dict(min_p=-0.1), dict(min_p="x"), dict(top_k=-3), dict(top_k=0, temperature=0.0), dict(typical_p=0.5)):
        req, why = ask(**kw)
        assert req is None and why, kw
    # greedy: no warper applies, whatever min_p says
    req, why = model._route_request((IDS, ), dict(max_new_tokens=4, min_p=0.3), sampler_processors=True, full_sampler=True)
    assert why is None and (req["top_k"], req["min_p"], req["do_sample"]) == (1, 0.0, False)


# ------------------------------------------------------------------------------------------------ FusedSampler
class _Stub:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 4096 if name == "gq_sample_full_ws_bytes" else 0
        return call


@pytest.fixture
def stub(monkeypatch):
    from guidedquant_amd import _lib
    s = _Stub()
    monkeypatch.setattr(_lib, "_lib", s)
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: None)
    return s


def _sampler(top_k, **kw):
    from guidedquant_amd.fused_sampler import FusedSampler
    return FusedSampler(V, "cpu", top_k, **dict(dict(top_p=0.9, temperature=0.7, seed=11), **kw))


def _launch(s):
    io = [torch.zeros(1, dtype=torch.int32) for _ in range(3)]
    logits = torch.zeros(V, dtype=torch.float16)
    s.launch(logits, *io)
    return logits, io


@pytest.mark.parametrize("top_k,min_p,penalty,suppress,logprobs",
                         [(k, mp, *r) for (k, mp) in ((None, 0.0), (0, 0.0), (65, 0.0), (200, 0.0), (8, 0.05), (0, 0.1)) for r in itertools.product((False, True), repeat=3)])
def test_full_configurations_call_gq_sample_full(stub, top_k, min_p, penalty, suppress, logprobs):
    s = _sampler(top_k, min_p=min_p, seq_capacity=16 if logprobs else 0, repetition_penalty=1.3 if penalty else 1.0, suppress_tokens=[3, 69] if suppress else (),
                 logprobs=logprobs)
    assert s.full and s.work_val is None and s.work_idx is None and s.lp_ws is None and s.ws.numel() * 8 == 4096
    sets = penalty or suppress
    assert (s.seen is not None) == sets and (s.suppress is not None) == suppress and (not sets or s.seen.shape == ((V + 31) // 32, ))
    assert [c[0] for c in stub.calls] == ["gq_sample_full_ws_bytes"] + (["gq_token_set_build"] if suppress else [])
    del stub.calls[:]
    logits, (tok, pos, nxt) = _launch(s)
    (name, args), = stub.calls
    assert name == "gq_sample_full"
    assert args == (logits.data_ptr(), V, int(top_k or 0), 0.9, min_p, 0.7, 11, s.counter.data_ptr(), s.ws.data_ptr(), 4096, tok.data_ptr(), pos.data_ptr(), nxt.data_ptr(),
                    s.ban.data_ptr(), s.seq.data_ptr() if logprobs else None, 16 if logprobs else 0, None, None, 0, None, 1.3 if penalty else 1.0, s.seen.data_ptr() if sets else None,
                    s.suppress.data_ptr() if suppress else None, s.lp_raw.data_ptr() if logprobs else None, s.lp_drawn.data_ptr() if logprobs else None,
                    16 if logprobs else 0, None)


@pytest.mark.parametrize("top_k", [1, 8, 32, 33, 64])
@pytest.mark.parametrize("penalty,suppress,logprobs", list(itertools.product((False, True), repeat=3)))
def test_old_configurations_keep_their_entry_point_and_arguments(stub, top_k, penalty, suppress, logprobs):
    s = _sampler(top_k, seq_capacity=16 if logprobs else 0, repetition_penalty=1.3 if penalty else 1.0, suppress_tokens=[3, 69] if suppress else (), logprobs=logprobs)
    sets = penalty or suppress
    assert not s.full and s.ws is None and s.min_p == 0.0 and s.work_val.shape == s.work_idx.shape == (128 * 64, )
    assert (s.seen is not None) == sets and [c[0] for c in stub.calls] == (["gq_token_set_build"] if suppress else [])
    del stub.calls[:]
    logits, (tok, pos, nxt) = _launch(s)
    (name, args), = stub.calls
    assert name == ("gq_sample_topk_lp" if logprobs else "gq_sample_topk_rep" if sets else "gq_sample_topk_p")
    common = (logits.data_ptr(), V, top_k, 0.9, 0.7, 11, s.counter.data_ptr(), s.work_val.data_ptr(), s.work_idx.data_ptr(), tok.data_ptr(), pos.data_ptr(),
              nxt.data_ptr(), s.ban.data_ptr(), s.seq.data_ptr() if logprobs else None, 16 if logprobs else 0, None, None, 0, None)
    rep = (1.3 if penalty else 1.0, s.seen.data_ptr() if sets else None, s.suppress.data_ptr() if suppress else None)
    lp = (s.lp_ws.data_ptr(), s.lp_raw.data_ptr(), s.lp_drawn.data_ptr(), 16) if logprobs else ()
    assert args == common + (rep if sets or logprobs else ()) + lp + (None, )


def test_refusals(stub):
    for kw in (dict(top_k=None), dict(top_k=0), dict(top_k=65), dict(top_k=8, min_p=0.1)):
        with pytest.raises(ValueError, match="32 candidates"):
            _sampler(**dict(dict(top_p=1.0, candidates=32), **kw))
    for mp in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_p"):
            _sampler(8, min_p=mp)
    with pytest.raises(ValueError, match="top_k"):
        _sampler(-1)
    assert stub.calls == []
