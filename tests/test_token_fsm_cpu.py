"""CPU: guidedquant_amd/token_fsm.py -- the canonical CSR form, the two constructors, every validation message, the host walk -- the numpy
model of the mask rows (tests/token_fsm_model.py) against `allowed()` for every state, and the refusals of FusedSampler(token_fsm=),
DecodeGraph(token_fsm=), generate(token_fsm=) and the C entries that need no GPU."""
import ctypes

import numpy as np
import pytest

import token_fsm_model as fm
from guidedquant_amd.token_fsm import TokenFSM

torch = pytest.importorskip("torch")

V = 70  # (3 words of 32 bits)


def test_canonical_csr_form():
    edges = [(2, 5, 0), (0, 9, 1), (0, 3, 2), (2, 1, -1), (1, 69, 2), (0, 64, 0)]
    f = TokenFSM(3, edges, default_next=[-1, -1, 1], start=0)
    assert f.row_ptr.tolist() == [0, 3, 4, 6] and f.edge_tok.tolist() == [3, 9, 64, 69, 1, 5] and f.edge_next.tolist() == [2, 1, 0, 2, -1, 0]
    assert f.default_next.tolist() == [-1, -1, 1] and (f.n_states, f.start) == (3, 0)
    for a in (f.row_ptr, f.edge_tok, f.edge_next, f.default_next):
        assert a.dtype == np.int32 and not a.flags.writeable
    # the form does not depend on the order of the edges, nor on their container; the key is the content's
    g = TokenFSM(3, iter(reversed(edges)), default_next=(-1, -1, 1))
    assert all(np.array_equal(a, b) for a, b in zip(fm.csr(f), fm.csr(g))) and f.key() == g.key()
    assert TokenFSM(3, edges, default_next=[-1, -1, 1], start=2).key() != f.key()
    assert TokenFSM(3, edges[:-1] + [(0, 64, 1)], default_next=[-1, -1, 1]).key() != f.key()
    # no edge at all: one free-text state
    free = TokenFSM(1, [], default_next=[0])
    assert free.row_ptr.tolist() == [0, 0] and free.edge_tok.size == 0 and free.allowed(0, 5).tolist() == [0, 1, 2, 3, 4]


def test_allowed_step_walk():
    f = TokenFSM(3, [(0, 3, 2), (0, 9, 1), (1, 69, 2), (2, 1, -1), (2, 5, 0)], default_next=[-1, -1, 1], vocab_size=V)
    assert f.allowed(0).tolist() == [3, 9] and f.allowed(1).tolist() == [69]
    assert f.allowed(2).tolist() == [t for t in range(V) if t != 1] and f.allowed(2, 4).tolist() == [0, 2, 3]
    assert f.allowed(0).dtype == np.int64
    assert (f.step(0, 3), f.step(0, 9), f.step(0, 4), f.step(2, 1), f.step(2, 5), f.step(2, 68)) == (2, 1, -1, -1, 0, 1)
    assert f.walk([]) == 0 and f.walk([9, 69, 5]) == 0 and f.walk([3, 40], None) == 1 and f.walk([69], state=1) == 2
    assert f.walk(torch.tensor([9, 69])) == 2
    with pytest.raises(ValueError, match=r"token 1 \(number 1 of the walk\) is forbidden in state 2"):
        f.walk([3, 1, 5])
    with pytest.raises(ValueError, match="state 3 is outside"):
        f.allowed(3)
    unbound = TokenFSM(1, [(0, 1, -1)], default_next=[0])
    with pytest.raises(ValueError, match="allowed\\(\\) needs vocab_size"):
        unbound.allowed(0)


def test_from_index():
    f = TokenFSM.from_index({0: {5: 1, 7: 2}, 1: {6: 2}, 2: {2: 2}}, start=0)
    assert f.n_states == 3 and f.row_ptr.tolist() == [0, 2, 3, 4] and f.edge_tok.tolist() == [5, 7, 6, 2] and f.edge_next.tolist() == [1, 2, 2, 2]
    assert (f.default_next == -1).all() and f.walk([5, 6, 2, 2]) == 2
    assert TokenFSM.from_index({4: {1: 4}}, start=4).n_states == 5  # (states 0..3 exist and are not reachable)
    with pytest.raises(ValueError, match="state 3 is reachable from state 0 and allows no token"):
        TokenFSM.from_index({0: {5: 3}})  # (a final state without an entry is a dead end: the index has to say what follows)
    for bad in ({}, [], {0: [1]}):
        with pytest.raises(ValueError, match="from_index"):
            TokenFSM.from_index(bad)


def test_from_choices():
    eos = [68, 69]
    # shared prefixes (10 11 12 / 10 11 13), one choice that is a prefix of another (10 / 10 11 12), a lone one, a duplicate
    f = TokenFSM.from_choices([[10, 11, 12], [10, 11, 13], [10], [20, 21], [20, 21]], eos, vocab_size=V)
    end = f.n_states - 1
    assert f.n_states == 8 and f.start == 0 and (f.default_next == -1).all()
    assert f.allowed(0).tolist() == [10, 20]
    s10 = f.step(0, 10)
    assert f.allowed(s10).tolist() == [11, 68, 69]  # (a complete choice AND the prefix of another: EOS or the continuation)
    s11 = f.step(s10, 11)
    assert f.allowed(s11).tolist() == [12, 13]
    for last in (12, 13):
        done = f.step(s11, last)
        assert f.allowed(done).tolist() == eos and all(f.step(done, e) == end for e in eos)  # (after a complete choice only EOS)
    assert f.allowed(f.walk([20])).tolist() == [21] and f.allowed(f.walk([20, 21])).tolist() == eos
    # the EOS tail: the absorbing state allows only EOS and stays
    assert f.allowed(end).tolist() == eos and all(f.step(end, e) == end for e in eos) and f.walk([10, 68, 69, 68, 68]) == end
    for bad, what in (([], "at least one choice"), ([[]], "at least one token"), ([[1, 68]], "holds the EOS id 68")):
        with pytest.raises(ValueError, match=what):
            TokenFSM.from_choices(bad, eos)
    for bad in ([], None):
        with pytest.raises(ValueError, match="at least one EOS id"):
            TokenFSM.from_choices([[1]], bad)


def test_every_validation_message():
    ok = [(0, 1, 1), (1, 2, 0)]
    for kw, what in ((dict(n_states=0), "n_states must be >= 1"), (dict(n_states=2.5), "n_states must be an integer"), (dict(n_states=True), "n_states must be an integer"),
                     (dict(start=2), r"start state 2 is outside \[0, 2\)"), (dict(start=-1), "start state -1 is outside"),
                     (dict(default_next=[-1]), "default_next has 1 entries for 2 states"), (dict(default_next=[-1, 2]), r"default_next\[1\] = 2 is neither -1 nor a state"),
                     (dict(default_next=[-2, 0]), r"default_next\[0\] = -2"),
                     (dict(edges=ok + [(2, 1, 0)]), r"edge \(2, 1, 0\): state 2 is outside \[0, 2\)"), (dict(edges=ok + [(-1, 1, 0)]), "state -1 is outside"),
                     (dict(edges=ok + [(0, 5, 2)]), r"edge \(0, 5, 2\): next state 2 is outside \[-1, 2\)"), (dict(edges=ok + [(0, 5, -2)]), "next state -2 is outside"),
                     (dict(edges=ok + [(0, -1, 1)]), r"token id -1 is outside \[0, 2\^31\)"), (dict(edges=ok + [(0, "1", 1)]), "an edge's token must be an integer"),
                     (dict(edges=ok + [(0, 1.5, 1)]), "an edge's token must be an integer"),
                     (dict(edges=ok + [(1, 2, 1)]), r"\(state 1, token 2\) is listed twice"), (dict(edges=ok + [(0, 1, -1)]), r"\(state 0, token 1\) is listed twice"),
                     # dead ends: nothing allowed by default and no allowing edge -- only when reachable from start
                     (dict(edges=[(0, 1, 1)]), "state 1 is reachable from state 0 and allows no token"),
                     (dict(edges=[(0, 1, 1), (1, 2, -1)]), "state 1 is reachable"), (dict(edges=[], default_next=[1, -1]), "state 1 is reachable"),
                     (dict(edges=[]), "state 0 is reachable from state 0 and allows no token"),
                     # the part that needs the vocabulary
                     (dict(vocab_size=2), r"state 1: token id 2 is outside \[0, 2\)"), (dict(vocab_size=0), "vocab_size must be >= 1"),
                     (dict(edges=[(0, 0, -1), (0, 1, -1)], default_next=[0, -1], vocab_size=2), "state 0 is reachable from state 0 and allows no token"),
                     (dict(vocab_size=V, max_mask_bytes=23), "the masks of 2 states over 70 tokens take 24 bytes, more than max_mask_bytes = 23")):
        args = dict(dict(n_states=2, edges=ok), **kw)
        with pytest.raises(ValueError, match="^token_fsm: .*" + what):
            TokenFSM(**args)
    assert TokenFSM(2, [(0, 1, 0)]).n_states == 2  # (state 1 allows nothing and is not reachable: no mistake)
    f = TokenFSM(2, ok, vocab_size=V, max_mask_bytes=24)
    assert f.vocab_size == V and f.check(V) == 24 and f.check(128256, 1 << 20) == 2 * 16032
    assert TokenFSM(1, [], default_next=[0]).check(128256) == 16032  # (16 KB per state at 128256 tokens)
    with pytest.raises(ValueError, match="take 268455840 bytes, more than max_mask_bytes = 268435456"):
        TokenFSM(16745, [], default_next=[0] * 16745).check(128256)  # (the default limit: 256 MiB)


MACHINES = {
    "mixed": lambda: TokenFSM(3, [(0, 3, 2), (0, 9, 1), (1, 69, 2), (2, 1, -1), (2, 5, 0), (2, 64, -1)], default_next=[-1, -1, 1]),
    "choices": lambda: TokenFSM.from_choices([[10, 11, 12], [10, 11, 13], [10], [0, 31, 32, 63, 64]], [68, 69]),
    "free": lambda: TokenFSM(1, [], default_next=[0]),
    "chain": lambda: TokenFSM(*fm.chain_machine([0, 31, 32, 63, 64, 69])),
}


@pytest.mark.parametrize("name", list(MACHINES))
@pytest.mark.parametrize("with_base", [False, True])
def test_mask_model_against_allowed(name, with_base):
    f = MACHINES[name]()
    base_ids = [9, 12, 69] if with_base else []
    base = np.zeros(fm.words(V), dtype=np.uint32)
    for t in base_ids:
        base[t >> 5] |= np.uint32(1 << (t & 31))
    rows = fm.mask_rows(*fm.csr(f), V, base if with_base else None)
    assert rows.shape == (f.n_states, 3) and rows.dtype == np.uint32
    for s in range(f.n_states):
        assert fm.row_allowed(rows[s], V).tolist() == [t for t in f.allowed(s, V).tolist() if t not in base_ids], (name, s)
        assert rows[s, -1] >> np.uint32(V & 31) == np.uint32(0xFFFFFFFF) >> np.uint32(V & 31), "the bits at and past V in the last word are set"
        for t in list(range(V)) + [-1, V, fm.EMPTY_TOKEN]:  # the transition: TokenFSM.step, with -1 / no token leaving the state as it is
            want = f.step(s, t) if 0 <= t < V else -1
            assert fm.step(*fm.csr(f), V, s, t) == (want if want >= 0 else s), (name, s, t)


# ------------------------------------------------------------------------------------------------ FusedSampler on a stub library
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


@pytest.mark.parametrize("top_k,entry", [(8, "gq_sample_topk_fsm"), (64, "gq_sample_topk_fsm"), (0, "gq_sample_full_fsm"), (None, "gq_sample_full_fsm"), (65, "gq_sample_full_fsm")])
@pytest.mark.parametrize("adjusted", [False, True])
def test_a_machine_selects_the_fsm_entry(stub, top_k, entry, adjusted):
    f = MACHINES["choices"]()
    s = _sampler(top_k, token_fsm=f, suppress_tokens=[4], **(dict(frequency_penalty=0.5) if adjusted else {}))
    (name, args), = [c for c in stub.calls if c[0] == "gq_token_fsm_build"]  # one launch, in the constructor, with the suppress list as the base
    assert args[4:8] == (f.n_states, V, s.suppress.data_ptr(), s.fsm_masks.data_ptr()) and args[:4] == tuple(t.data_ptr() for t in s.fsm_tables)
    assert s.fsm_masks.shape == (f.n_states, 3) and s.fsm_masks.dtype == torch.int32 and s.fsm_state.shape == (1, ) and int(s.fsm_state) == f.start
    assert [t.tolist() for t in s.fsm_tables] == [a.tolist() for a in fm.csr(f)]
    del stub.calls[:]
    _launch(s)
    (name, args), = stub.calls
    assert name == entry and args[-1] is None
    g = args[-2]._obj
    assert g is s._fsm and (g.masks, g.words_per_state, g.n_states, g.state) == (s.fsm_masks.data_ptr(), 3, f.n_states, s.fsm_state.data_ptr())
    assert (g.row_ptr, g.edge_tok, g.edge_next, g.default_next) == tuple(t.data_ptr() for t in s.fsm_tables)
    assert (args[-3]._obj is s._adj) if adjusted else (args[-3] is None)
    # without a machine: the calls the sampler made, and no state
    del stub.calls[:]
    plain = _sampler(top_k, suppress_tokens=[4], **(dict(frequency_penalty=0.5) if adjusted else {}))
    assert plain.token_fsm is plain.fsm_masks is plain.fsm_state is plain.fsm_tables is None
    plain.reset_fsm()
    plain.advance_fsm([1, 2])
    plain.clear_warmup()
    assert "gq_token_fsm_build" not in [c[0] for c in stub.calls]
    del stub.calls[:]
    _launch(plain)
    assert stub.calls[0][0] == (entry.replace("_fsm", "_adj") if adjusted else "gq_sample_full" if plain.full else "gq_sample_topk_rep")


def test_request_state_helpers(stub):
    f = MACHINES["choices"]()
    s = _sampler(token_fsm=f)
    assert int(s.fsm_state) == 0
    s.advance_fsm([10])
    assert int(s.fsm_state) == f.walk([10])
    s.advance_fsm(torch.tensor([[11, 12]]))  # (from where the last advance left the machine)
    assert int(s.fsm_state) == f.walk([10, 11, 12])
    with pytest.raises(ValueError, match="token 5 .* is forbidden in state"):
        s.advance_fsm([5])
    s.reset_fsm()
    assert int(s.fsm_state) == 0
    s.reset_fsm(3)
    assert int(s.fsm_state) == 3
    s.fsm_state.fill_(5)  # (what warm-up and capture-time draws do)
    s.clear_warmup()
    assert int(s.fsm_state) == 0
    with pytest.raises(ValueError, match="state %d is outside" % f.n_states):
        s.reset_fsm(f.n_states)


def test_fused_sampler_refusals(stub):
    f = MACHINES["choices"]()
    with pytest.raises(ValueError, match="^token_fsm: a workspace of 32 candidates"):
        _sampler(top_p=1.0, candidates=32, token_fsm=f)
    with pytest.raises(ValueError, match="token_fsm must be a guidedquant_amd.token_fsm.TokenFSM, not dict"):
        _sampler(token_fsm={0: {1: 0}})
    with pytest.raises(ValueError, match=r"token_fsm: state 0: token id 70 is outside \[0, 70\)"):
        _sampler(token_fsm=TokenFSM(1, [(0, 70, 0)]))
    with pytest.raises(ValueError, match="^token_fsm: state 1 allows no token that suppress_tokens leaves"):
        _sampler(token_fsm=TokenFSM(2, [(0, 1, 1), (1, 2, 0), (1, 3, 0)]), suppress_tokens=[2, 3])
    assert stub.calls == []


def test_exports_and_refusals_without_a_gpu():
    from guidedquant_amd import _lib
    L = _lib.lib()
    for name in ("gq_token_fsm_build", "gq_sample_topk_fsm", "gq_sample_full_fsm"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    buf = (ctypes.c_int * 64)(*([0x7E7E7E7E] * 64))
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = L.gq_sample_full_ws_bytes(300)
    ws = (ctypes.c_char * (need + 16))(*([0x7E] * (need + 16)))
    wsp = ctypes.c_void_p((ctypes.addressof(ws) + 15) & ~15)

    def topk(fsm, adj=None, V=300, top_k=8, top_n=0):
        return L.gq_sample_topk_fsm(p, V, top_k, 1.0, 1.0, 7, p, p, p, p, p, p, None, None, 0, None, None, 0, None, 1.0, None, None, p, p, p, 4, top_n, p, p, p,
                                    ctypes.byref(adj) if adj is not None else None, ctypes.byref(fsm) if fsm is not None else None, None)

    def full(fsm, adj=None, V=300, top_k=0, top_n=0):
        return L.gq_sample_full_fsm(p, V, top_k, 1.0, 0.0, 1.0, 7, p, wsp, need, p, p, p, None, None, 0, None, None, 0, None, 1.0, None, None, p, p, 4, top_n, p, p, p,
                                    ctypes.byref(adj) if adj is not None else None, ctypes.byref(fsm) if fsm is not None else None, None)
    F, A = _lib.GqTokenFsm, _lib.GqSampleAdjust
    W = 10  # ceil(300 / 32)
    good = F(p, W, 2, p, p, p, p, p)
    for call in (topk, full):
        for fsm in (F(None, W, 2, p, p, p, p, p), F(p, W, 2, None, p, p, p, p), F(p, W, 2, p, p, None, p, p), F(p, W, 2, p, p, p, None, p), F(p, W, 2, p, p, p, p, None),  # a NULL table
                    F(p, W, 0, p, p, p, p, p), F(p, W - 1, 2, p, p, p, p, p), F(p, W + 1, 2, p, p, p, p, p)):  # no state; a stride that is not the vocabulary's
            assert call(fsm) == _lib.GQ_EINVAL and b"fsm: " in L.gq_last_error()
        # the adjustment's refusals come first, then the entry's own, with their codes -- with a machine and without one
        assert call(good, A(float("inf"), 0.0, None, None, p, p)) == _lib.GQ_EINVAL and b"frequency_penalty" in L.gq_last_error()
        for fsm in (good, None):
            assert call(fsm, V=262145) == (_lib.GQ_ENOTSUP if fsm is None else _lib.GQ_EINVAL)  # (with a machine the stride is wrong first)
            assert call(fsm, top_n=21) == _lib.GQ_EINVAL and call(fsm, top_n=-1) == _lib.GQ_EINVAL
        assert call(F(p, 8193, 2, p, p, p, p, p), V=262145) == _lib.GQ_ENOTSUP
    assert topk(good, top_k=65) == _lib.GQ_ENOTSUP and full(good, top_k=-1) == _lib.GQ_EINVAL
    for a in ((None, p, p, p, 2, 300, None, p), (p, p, None, p, 2, 300, None, p), (p, p, p, None, 2, 300, None, p), (p, p, p, p, 2, 300, None, None),
              (p, p, p, p, 0, 300, None, p), (p, p, p, p, 2, 0, None, p)):
        assert L.gq_token_fsm_build(*a, None) == _lib.GQ_EINVAL and b"gq_token_fsm_build" in L.gq_last_error()
    assert all(b == 0x7E for b in ws.raw) and all(v == 0x7E7E7E7E for v in buf), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------ generate() and DecodeGraph on the host
IDS = torch.tensor([[3, 17, 5]])


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    pytest.importorskip("transformers")
    from ap_helpers import tiny_hf_anyprec_checkpoint
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    path = tmp_path_factory.mktemp("tiny")
    tiny_hf_anyprec_checkpoint(path)
    return AnyPrecisionForCausalLM.from_quantized(str(path), device="cpu")


def test_generate_pops_the_keyword_and_refuses_on_the_host(model, monkeypatch):
    seen = []
    monkeypatch.setattr(model.model, "generate", lambda *a, **k: seen.append(dict(k)) or IDS)
    base = dict(max_new_tokens=3, do_sample=False, pad_token_id=0)
    assert model.generate(IDS, **base, token_fsm=None) is IDS  # None is the call without the keyword, and never reaches transformers
    assert len(seen) == 1 and "token_fsm" not in seen[0]
    del seen[:]
    assert "token_fsm" not in model._ROUTE_KW
    f = TokenFSM.from_choices([[1, 2], [3]], [0])
    prec = model.precision
    # a host model: route 1 needs the GPU -- refused under the keyword's name, never dropped; native=False and capture=True as well
    for route in (dict(), dict(native=True), dict(native=False), dict(capture=True), dict(precision=2), dict(num_beams=2), dict(min_new_tokens=2),
                  dict(frequency_penalty=0.5)):
        with pytest.raises(ValueError, match="^token_fsm: "):
            model.generate(IDS, **dict(base, **route), token_fsm=f)
        assert model.precision == prec
    for route in (dict(native=False), dict(capture=True)):
        with pytest.raises(ValueError, match=r"^token_fsm: served by the fused decode model only \(not with native=False or capture=True\)"):
            model.generate(IDS, **dict(base, **route), token_fsm=f)
    with pytest.raises(ValueError, match="^token_fsm: must be a guidedquant_amd.token_fsm.TokenFSM, not dict"):
        model.generate(IDS, **base, token_fsm={0: {1: 0}})
    vocab = int(model.config.vocab_size)
    with pytest.raises(ValueError, match=r"^token_fsm: state 0: token id %d is outside \[0, %d\)" % (vocab, vocab)):
        model.generate(IDS, **base, token_fsm=TokenFSM(1, [(0, vocab, 0)]))
    assert seen == []


def test_decode_graph_refuses_the_machine_without_native_sampling():
    from guidedquant_amd.generate import DecodeGraph

    class _NoNative:
        def native_ready(self):
            return False
    for native in (False, True):  # (True on a model without the fused step is the torch-sampling graph as well)
        with pytest.raises(ValueError, match="^token_fsm: served by the fused sampler only"):
            DecodeGraph(_NoNative(), "cpu", native_sampling=native, temperature=0.8, top_k=8, token_fsm=MACHINES["chain"]())
