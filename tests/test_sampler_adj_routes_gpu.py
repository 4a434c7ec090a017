"""GPU, model level: frequency_penalty / presence_penalty / logit_bias on the fused decode route -- `DecodeGraph(...)` and
`AnyPrecisionForCausalLM.generate(...)` -- on the tiny random-init Llama of tests/sampler_calls.py (D = 512, 2 layers, V = 384).  The kernels
are pinned by tests/test_sampler_adj_gpu.py and tests/test_sampler_full_adj_gpu.py; here: the counts feed back inside a captured multi-step
graph, generate equals the DecodeGraph run with the same settings, the counts start over with every request, the bias decides a greedy
draw, the refusals, and a request without the keywords is what it was."""
import numpy as np
import pytest

import sampler_calls as sc

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

V = sc.SMALL["vocab_size"]


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


def _run_graph(g, steps, first=7):
    g.seq.zero_()
    g.ban.zero_()
    g.rng_counter.fill_(5)
    g.set_token(first, 0)
    g.set_history([first])
    g.reset_generated()
    for _ in range(steps // g.steps_per_replay):
        g.step()
    torch.cuda.synchronize()
    return g.seq[1:steps + 1].cpu().tolist()


@pytest.mark.parametrize("kw", [dict(temperature=0.9, top_k=50, top_p=0.9, repetition_penalty=1.2), dict(temperature=0.9, top_k=0, min_p=0.01)],
                         ids=["top_k_50", "whole_vocabulary"])
def test_one_and_four_steps_per_replay_draw_the_same_tokens_and_leave_the_same_counts(llama, kw):
    from guidedquant_amd.generate import DecodeGraph
    m, steps = llama, 24
    dec = _decoder(m)
    adj = dict(frequency_penalty=0.75, presence_penalty=0.5, logit_bias={3: 2.0, "40": -1.5, 383: 0.25})
    got = {}
    for spr in (0, 1, 4):  # (0: the run without the three arguments; its first token is then biased out of the other two)
        if spr == 1:
            adj["logit_bias"][got[0][0][0]] = -50.0
        g = DecodeGraph(dec, m.device, native_sampling=True, fold_embed=True, seq_capacity=65, steps_per_replay=max(spr, 1), **kw, **(adj if spr else {}))
        try:
            s = g.sampler
            assert s.adjusted == bool(spr) and (s.out_count is not None) == bool(spr)
            if spr:  # the constructor's warm-up and capture draws are gone: the counts are empty
                assert not s.out_set.any() and not s.out_count.any()
            toks = _run_graph(g, steps)
            got[spr] = (toks, s.out_count.cpu().numpy().copy() if spr else None, s.out_set.cpu().numpy().copy() if spr else None)
        finally:
            g.close()
    assert got[1][0] == got[4][0], "a four-step replay draws other tokens than single steps: the counts do not feed back inside the graph"
    assert np.array_equal(got[1][1], got[4][1]) and np.array_equal(got[1][2], got[4][2])
    # the device's counts are the tally of the tokens it stored
    want = np.bincount(np.asarray(got[1][0]), minlength=V)
    assert np.array_equal(got[1][1], want) and int(want.sum()) == steps
    bits = np.unpackbits(got[1][2].view(np.uint8), bitorder="little")[:V]
    assert np.array_equal(bits.astype(bool), want > 0)
    assert got[0][0][0] not in got[1][0], "the bias changes nothing"


def test_generate_equals_the_decode_graph_and_a_second_request_starts_over(llama):
    from guidedquant_amd.generate import DecodeGraph
    m, new = llama, 24
    ids = torch.tensor([[7]], device=m.device)
    kw = dict(max_new_tokens=new, pad_token_id=0, do_sample=False, native=True)
    plain = m.generate(ids, **kw)[0, 1:].tolist()
    out = m.generate(ids, presence_penalty=1.5, frequency_penalty=0.25, **kw)[0, 1:].tolist()
    again = m.generate(ids, presence_penalty=1.5, frequency_penalty=0.25, **kw)[0, 1:].tolist()
    assert out == again, "the counts of the first request leaked into the second"
    assert out != plain or len(set(plain)) == new  # (a greedy run that repeats a token cannot survive the penalty unchanged)
    # a penalty no logit survives: no generated token comes twice (greedy, 24 of 384 tokens); the prompt's token is not counted and may
    huge = m.generate(ids, presence_penalty=1.0e4, **kw)[0, 1:].tolist()
    assert len(set(huge)) == new
    assert m.generate(ids, **kw)[0, 1:].tolist() == plain, "a request without the keywords is not what it was"
    dec = _decoder(m)
    g = DecodeGraph(dec, m.device, native_sampling=True, fold_embed=True, seq_capacity=65, steps_per_replay=8, temperature=0.0, top_k=1,
                    presence_penalty=1.5, frequency_penalty=0.25)
    try:
        assert _run_graph(g, new) == out
    finally:
        g.close()


def test_a_bias_decides_the_greedy_draw(llama):
    m, new = llama, 12
    ids = torch.tensor([sc.PROMPT], device=m.device)
    T = ids.shape[1]
    kw = dict(max_new_tokens=new, pad_token_id=0, do_sample=False)
    plain = m.generate(ids, **kw)[0, T:].tolist()
    t = 123
    assert m.generate(ids, logit_bias={t: 100.0}, **kw)[0, T:].tolist() == [t] * new
    assert m.generate(ids, logit_bias={str(t): 100.0}, native=True, **kw)[0, T:].tolist() == [t] * new
    first = plain[0]
    out = m.generate(ids, logit_bias={first: -100.0}, **kw)[0, T:].tolist()
    assert out and first not in out  # (the run may end at the config's EOS)
    # the unprocessed distribution's numbers stay raw: the first step's logprobs row is the one of the request without the bias
    a = m.generate(ids, output_logprobs=True, top_logprobs=3, **kw)
    b = m.generate(ids, output_logprobs=True, top_logprobs=3, logit_bias={first: -100.0}, **kw)
    assert torch.equal(a.top_logprobs_ids[0, 0], b.top_logprobs_ids[0, 0]) and torch.equal(a.top_logprobs[0, 0].view(torch.int32), b.top_logprobs[0, 0].view(torch.int32))
    assert int(a.top_logprobs_ids[0, 0, 0]) == first and int(b.sequences[0, T]) != first
    assert m.generate(ids, **kw)[0, T:].tolist() == plain


def test_refusals(llama):
    from guidedquant_amd.generate import DecodeGraph
    m = llama
    ids = torch.tensor([sc.PROMPT], device=m.device)
    kw = dict(max_new_tokens=4, pad_token_id=0)
    for adj, name in ((dict(frequency_penalty=0.5), "frequency_penalty"), (dict(presence_penalty=0.5), "presence_penalty"), (dict(logit_bias={1: 1.0}), "logit_bias")):
        for route in (dict(native=False), dict(capture=True), dict(do_sample=True, top_k=100), dict(num_beams=2)):
            with pytest.raises(ValueError, match="^" + name + ": "):
                m.generate(ids, **kw, **route, **adj)
        dec = _decoder(m)
        with pytest.raises(ValueError, match="served by the fused sampler only"):  # (the torch-sampling graph)
            DecodeGraph(dec, m.device, native_sampling=False, temperature=0.8, top_k=8, **adj)
    with pytest.raises(ValueError, match="logit_bias: token id 384 is outside"):
        m.generate(ids, logit_bias={V: 1.0}, **kw)
