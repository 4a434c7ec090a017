"""GPU, model level: token_fsm on the fused decode route -- `DecodeGraph(token_fsm=)` and `AnyPrecisionForCausalLM.generate(token_fsm=)` -- on
the tiny random-init Llama of tests/sampler_calls.py (D = 512, 2 layers, V = 384).  The kernels are pinned by tests/test_token_fsm_gpu.py;
here: the machine walks inside a captured multi-step graph across replay boundaries, the state is the start state behind the constructor
and at the start of every request, a sampled request always returns one of the choices followed by EOS, a greedy request equals a host loop
over the same decoder's step logits masked with `allowed()`, the refusals, and a request without the keyword makes the recorded calls."""
import json
import os

import numpy as np
import pytest

import sampler_calls as sc
import token_fsm_model as fm
from guidedquant_amd.token_fsm import TokenFSM

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

V = sc.SMALL["vocab_size"]
EOS = sc.EOS


@pytest.fixture(scope="module")
def llama():
    m = sc._hf_model()
    with torch.no_grad():  # (from_config_random draws N(0, 0.02) embeddings: scaled up so that the logits have margins)
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    return m


def _decoder(m):
    dec = m.native_decoder(4)
    m._evict("graph")
    dec.setup_caches(1, 64)
    return dec


@pytest.mark.parametrize("kw", [dict(temperature=0.9, top_k=50, top_p=0.9), dict(temperature=0.9, top_k=0, min_p=0.01)], ids=["top_k_50", "whole_vocabulary"])
def test_a_chain_is_emitted_across_replay_boundaries(llama, kw):
    from guidedquant_amd.generate import DecodeGraph
    m, steps = llama, 30
    chain = [0, 31, 32, 383, 7, 7, 100, 200, 64, 63, 5, 300, 1]  # (13 states against 10 steps per replay: every replay begins elsewhere)
    f = TokenFSM(*fm.chain_machine(chain), start=2)
    g = DecodeGraph(_decoder(m), m.device, native_sampling=True, fold_embed=True, seq_capacity=65, steps_per_replay=10, token_fsm=f, **kw)
    try:
        s = g.sampler
        assert s.token_fsm is f and int(s.fsm_state) == 2, "the warm-up and capture-time draws moved the machine: the constructor leaves the start state"
        for request in range(2):
            g.seq.zero_()
            g.rng_counter.fill_(5 + request)
            g.set_token(7, 0)
            g.set_history([7])
            g.reset_fsm()
            for _ in range(steps // g.steps_per_replay):
                g.step()
            torch.cuda.synchronize()
            assert g.seq[1:steps + 1].cpu().tolist() == [chain[(2 + i) % len(chain)] for i in range(steps)], request
            assert int(s.fsm_state) == (2 + steps) % len(chain)
        g.reset_fsm(5)
        g.step_one()  # (the single-step graph over the same state)
        torch.cuda.synchronize()
        assert int(g.next_tok) == chain[5] and int(s.fsm_state) == 6
    finally:
        g.close()


def test_a_sampled_request_returns_one_of_the_choices_and_eos(llama):
    m = llama
    ids = torch.tensor([sc.PROMPT], device=m.device)
    T = ids.shape[1]
    choices = [[10, 11, 12], [10, 11, 13], [10], [200, 31, 32, 383], [5]]
    f = TokenFSM.from_choices(choices, [EOS])
    want = {tuple(c) + (EOS, ) for c in choices}
    got = set()
    for seed in range(20):  # (every request starts in the start state again: one decoder, one cached graph)
        torch.manual_seed(seed)
        out = m.generate(ids, token_fsm=f, do_sample=True, temperature=1.5, top_k=50, max_new_tokens=8, eos_token_id=EOS, pad_token_id=0)
        assert out[0, :T].tolist() == sc.PROMPT
        assert tuple(out[0, T:].tolist()) in want, (seed, out[0, T:].tolist())
        got.add(tuple(out[0, T:].tolist()))
    assert len([k for k in m._native_cache if k[0] == "graph"]) == 1, "an equal machine is one sampler: the decoder keys it on the content"
    # the whole-vocabulary sampler, and an equal machine built again
    again = TokenFSM.from_choices(choices, [EOS])
    for seed in range(5):
        torch.manual_seed(seed)
        out = m.generate(ids, token_fsm=again, do_sample=True, temperature=1.5, top_k=0, max_new_tokens=8, eos_token_id=EOS, pad_token_id=0, native=True)
        assert tuple(out[0, T:].tolist()) in want, (seed, out[0, T:].tolist())


def test_a_greedy_request_equals_the_host_loop_over_masked_logits(llama):
    m, new = llama, 12
    ids = torch.tensor([[7]], device=m.device)
    kw = dict(max_new_tokens=new, pad_token_id=0, do_sample=False, native=True)
    plain = m.generate(ids, **kw)[0, 1:].tolist()
    rng = np.random.default_rng(3)
    # three states: a listed set, everything but some exceptions (the unconstrained run's tokens among them), a listed set again
    listed = [sorted(set(rng.choice(V, size=40, replace=False).tolist()) - {plain[0]}) for _ in range(2)]  # (the first token has to differ)
    f = TokenFSM(3, [(0, t, 1) for t in listed[0]] + [(1, t, -1) for t in sorted(set(plain))] + [(1, 0, 0)] * (0 not in plain) + [(2, t, 0) for t in listed[1]],
                 default_next=[-1, 2, -1])
    out = m.generate(ids, token_fsm=f, **kw)[0, 1:].tolist()
    dec = m.native_decoder(4)
    tok, pos, s, host = torch.tensor([7], dtype=torch.int32, device=m.device), torch.zeros(1, dtype=torch.int32, device=m.device), f.start, []
    with torch.inference_mode():
        for i in range(new):
            logits = dec.decode_native(tok, pos).float().cpu().numpy().reshape(-1)
            masked = np.full(V, -np.inf, dtype=np.float32)
            allow = f.allowed(s, V)
            masked[allow] = logits[allow]
            t = int(np.argmax(masked))  # (the first of equal maxima: the lowest id)
            host.append(t)
            s = f.step(s, t)
            tok.fill_(t)
            pos.add_(1)
    assert out == host and f.walk(out) == s
    assert out != plain
    assert m.generate(ids, **kw)[0, 1:].tolist() == plain, "a request without the keyword is not what it was"


def test_refusals(llama):
    from guidedquant_amd.fused_sampler import FusedSampler
    from guidedquant_amd.generate import DecodeGraph
    m = llama
    ids = torch.tensor([sc.PROMPT], device=m.device)
    kw = dict(max_new_tokens=4, pad_token_id=0)
    f = TokenFSM.from_choices([[10, 11], [5]], [EOS])
    for route in (dict(native=False), dict(capture=True)):
        with pytest.raises(ValueError, match=r"^token_fsm: served by the fused decode model only \(not with native=False or capture=True\)"):
            m.generate(ids, token_fsm=f, **kw, **route)
    for route in (dict(num_beams=2), dict(do_sample=True, top_k=100)):  # (requests route 1 declines)
        with pytest.raises(ValueError, match="^token_fsm: "):
            m.generate(ids, token_fsm=f, **kw, **route)
    with pytest.raises(ValueError, match="^token_fsm: not served together with min_new_tokens > 0"):
        m.generate(ids, token_fsm=f, min_new_tokens=2, eos_token_id=EOS, **kw)
    with pytest.raises(ValueError, match=r"^token_fsm: state 0: token id 384 is outside \[0, 384\)"):
        m.generate(ids, token_fsm=TokenFSM(1, [(0, V, 0)]), **kw)
    with pytest.raises(ValueError, match="^token_fsm: must be a guidedquant_amd.token_fsm.TokenFSM"):
        m.generate(ids, token_fsm={0: {1: 0}}, **kw)
    dec = _decoder(m)
    with pytest.raises(ValueError, match="^token_fsm: served by the fused sampler only"):  # (the torch-sampling graph)
        DecodeGraph(dec, m.device, native_sampling=False, temperature=0.8, top_k=8, token_fsm=f)
    with pytest.raises(ValueError, match="^token_fsm: a workspace of 32 candidates"):
        FusedSampler(V, m.device, 8, candidates=32, token_fsm=f)


@pytest.mark.parametrize("name", ["graph_suppress", "route1_plain"])
def test_without_the_keyword_the_routes_make_the_recorded_calls(name):
    with open(os.path.join(os.path.dirname(__file__), "golden", "sampler_calls.json")) as fh:
        want = json.load(fh)["configs"][name]
    got = json.loads(json.dumps(sc.record(name)))
    assert got == want
