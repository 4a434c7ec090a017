"""GPU, model level: repetition_penalty and suppress_tokens on the fused routes of AnyPrecisionForCausalLM.generate.

A tiny Llama (D = 512, 3 layers, V = 512, as tests/test_hf_routes_gpu.py builds it) and a tiny Qwen2 whose generation config carries
repetition_penalty = 1.05 like the published Qwen2.5-Instruct one.  The plain generate() of the Qwen2 model must take route 1 (before:
transformers' generate on the module tree); route 1 is checked against transformers' RepetitionPenaltyLogitsProcessor applied on the
CPU to the logits of every step, route 2 against route 3, and the set must be rebuilt per request on a cached graph.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

_NAMES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
PROMPT = [3, 17, 5, 60, 2, 9]


def _long_prompt(shift=0, n=160):
    """n distinct ids, a third of the vocabulary of 512: a greedy continuation of a random model seldom repeats itself within a few dozen
    tokens, so the penalty has to find its tokens in the PROMPT -- with these, every step's arg-max is a seen token one time in three"""
    return [(i * 37 + 11 + shift * 101) % 512 for i in range(n)]


def _model(cfg, seed=5):
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=torch.device("cuda:0"), seed=seed)
    with torch.no_grad():  # (from_config_random draws N(0, 0.02) embeddings: scaled up so that the logits have margins)
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    return m


def _llama(seed=5):
    return _model(transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2,
                                           vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False), seed)


def _qwen2(seed=5):
    m = _model(transformers.Qwen2Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2,
                                        vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-6, tie_word_embeddings=False), seed)
    m.model.generation_config.repetition_penalty = 1.05
    return m


@pytest.fixture(scope="module")
def llama():
    return _llama()


def _ids(m, prompt=PROMPT):
    return torch.tensor([prompt], device=m.device)


def _hf_penalty(rp, seq, scores):
    """transformers' processor on the CPU (a true division there) over fp32 scores [V]"""
    proc = transformers.RepetitionPenaltyLogitsProcessor(penalty=float(rp))
    return proc(torch.tensor([list(seq)], dtype=torch.long), scores.detach().float().cpu().view(1, -1).clone())[0].numpy()


def test_the_published_qwen25_generation_config_takes_the_fused_route():
    m = _qwen2()
    ids = _ids(m)
    out = m.generate(ids, max_new_tokens=24, pad_token_id=0)
    assert ("decoder", 2) in m._native_cache and any(k[0] == "graph" and 1.05 in k for k in m._native_cache), list(m._native_cache)
    assert out.shape == (1, len(PROMPT) + 24) and out.dtype == ids.dtype and torch.equal(out[:, :len(PROMPT)], ids)
    again = m.generate(ids, max_new_tokens=24, pad_token_id=0, native=True)  # (raised ValueError("native=True: repetition_penalty") before)
    assert torch.equal(out, again)
    with pytest.raises(ValueError, match="native=True"):
        m.generate(ids, max_new_tokens=4, no_repeat_ngram_size=2, native=True)


def test_route_1_is_transformers_processor_on_every_steps_logits(llama):
    m, rp, new = llama, 1.3, 24
    for shift in range(3):  # (the first prompt whose continuation the penalty changes; all three are checked against the processor)
        ids = _ids(m, _long_prompt(shift))
        T = ids.shape[1]
        plain = m.generate(ids, max_new_tokens=new, do_sample=False, pad_token_id=0)
        out = m.generate(ids, max_new_tokens=new, do_sample=False, repetition_penalty=rp, pad_token_id=0)
        assert ("decoder", 2) in m._native_cache and out.shape == (1, T + new)
        _replay_against_the_processor(m, out, T, new, rp)
        if not torch.equal(out, plain):
            break
    assert not torch.equal(out, plain), "the penalty changed nothing: the comparison would show nothing"


def _replay_against_the_processor(m, out, T, new, rp):
    dec = m._native_cache[("decoder", 2)]
    seq = out[0].tolist()
    ids32 = out[0].to(torch.int32)
    with torch.no_grad():
        dec.prefill_native(ids32[:T - 1], torch.arange(0, T - 1, device=m.device, dtype=torch.int32), start=0)
        for p in range(T - 1, T + new - 1):  # the step at position p draws token p + 1 from the history seq[:p + 1]
            logits = dec.decode_native(ids32[p:p + 1], torch.tensor([p], device=m.device, dtype=torch.int32)).view(-1).clone()
            s = _hf_penalty(rp, seq[:p + 1], logits)
            want = int(np.flatnonzero(s == s.max())[0])
            assert seq[p + 1] == want, (p, seq[p + 1], want, float(s[seq[p + 1]]), float(s[want]))


def test_route_2_against_route_3(llama):
    m, rp, new = llama, 1.3, 16
    ids = _ids(m, _long_prompt())
    T = ids.shape[1]
    cap = m.generate(ids, max_new_tokens=new, do_sample=False, repetition_penalty=rp, pad_token_id=0, capture=True, native=False)
    assert any(k[0] == "cap" and rp in k for k in m._native_cache)
    ref = m.generate(ids, max_new_tokens=new, do_sample=False, repetition_penalty=rp, pad_token_id=0, native=False)
    assert cap.shape == ref.shape == (1, T + new)
    diff = torch.nonzero(cap[0] != ref[0]).view(-1)
    if diff.numel():
        # torch on the GPU divides by a Python scalar as a product with the reciprocal: equal up to a near tie.  The first differing
        # position is accepted only if the two tokens' scores behind transformers' processor are within 4 ulp of fp32 (1 for the
        # reciprocal form plus the roundings); nothing behind it is compared
        p = int(diff[0])
        assert p >= T
        with torch.no_grad():
            logits = m.model(ref[:, :p]).logits[0, -1]
        s = _hf_penalty(rp, ref[0, :p].tolist(), logits)
        a, b = np.float32(s[int(cap[0, p])]), np.float32(s[int(ref[0, p])])
        ulp = np.spacing(np.float32(max(abs(a), abs(b))))
        print("route 2 / route 3 differ at %d: scores %.9g %.9g, %.2f ulp" % (p, a, b, abs(float(a) - float(b)) / float(ulp)))
        assert abs(float(a) - float(b)) <= 4 * float(ulp), (p, a, b)


def test_replay_forms_and_the_set_the_constructor_leaves(llama):
    from guidedquant_amd.generate import DecodeGraph
    m = llama
    dec = m.native_decoder(2)
    m._evict("graph")
    dec.setup_caches(1, 256)
    outs = []
    for spr in (8, 1):
        g = DecodeGraph(dec, m.device, native_sampling=True, fold_embed=True, seq_capacity=257, temperature=0.0, top_k=1, steps_per_replay=spr,
                        repetition_penalty=1.3, suppress_tokens=[11, 400])
        try:
            assert not bool((g.seen != 0).any()), "the warm-up draws are still in the seen set"
            want = np.zeros(16, dtype=np.uint32)
            want[11 >> 5] |= 1 << (11 & 31)
            want[400 >> 5] |= 1 << (400 & 31)
            assert np.array_equal(g.suppress.cpu().numpy().view(np.uint32), want)
            g.seq.zero_()
            g.ban.zero_()
            g.set_token(7, 0)
            g.set_history([7])
            assert int(g.seen.cpu().numpy().view(np.uint32)[0]) == 1 << 7
            for _ in range(24 // spr):
                g.step()
            torch.cuda.synchronize()
            outs.append(g.seq[1:25].tolist())
            bits = g.seen.cpu().numpy().view(np.uint32)
            assert {t for t in range(512) if bits[t >> 5] >> (t & 31) & 1} == set(outs[-1]) | {7}
        finally:
            g.close()
    assert outs[0] == outs[1] and not {11, 400} & set(outs[0])
    with pytest.raises(ValueError, match="repetition_penalty"):
        DecodeGraph(dec, m.device, native_sampling=False, temperature=0.0, top_k=1, repetition_penalty=1.3)
    with pytest.raises(ValueError, match="suppress_tokens"):
        DecodeGraph(dec, m.device, native_sampling=False, temperature=0.0, top_k=1, suppress_tokens=[3])


def test_two_requests_on_one_cached_graph_rebuild_the_set(llama):
    m = llama
    prompts = (_long_prompt(0), _long_prompt(1, n=100))  # (different lengths: one cached graph serves both)
    kw = dict(max_new_tokens=20, do_sample=False, repetition_penalty=1.3, pad_token_id=0)
    m._evict("graph")
    got = [m.generate(_ids(m, p), **kw) for p in prompts]
    assert sum(1 for k in m._native_cache if k[0] == "graph") == 1
    for p, g in zip(prompts, got):
        fresh = _llama()  # (the same seed: the same weights)
        assert torch.equal(fresh.generate(_ids(fresh, p), **kw), g), p
        fresh._drop_native()
    # and route 2 the same way
    m._evict("cap")
    kw2 = dict(max_new_tokens=6, do_sample=False, repetition_penalty=1.3, pad_token_id=0, capture=True, native=False)
    a = [m.generate(_ids(m, p), **kw2) for p in ([3, 17, 5, 60, 2, 9], [9, 2, 60, 5, 17, 3])]
    b = m.generate(_ids(m, [3, 17, 5, 60, 2, 9]), **kw2)
    assert sum(1 for k in m._native_cache if k[0] == "cap") == 1 and torch.equal(a[0], b)


def test_a_sampled_request_is_reproducible(llama):
    m = llama
    kw = dict(max_new_tokens=24, do_sample=True, repetition_penalty=1.05, top_k=20, top_p=0.8, temperature=0.7, pad_token_id=0)
    torch.manual_seed(3)
    a = m.generate(_ids(m), **kw)
    torch.manual_seed(3)
    b = m.generate(_ids(m), **kw)
    torch.manual_seed(4)
    c = m.generate(_ids(m), **kw)
    assert torch.equal(a, b) and a.shape == c.shape == (1, len(PROMPT) + 24)
    assert any(k[0] == "graph" and k[-2] == 1.05 and 20 in k for k in m._native_cache), "not served by the fused route"


def test_suppress_tokens(llama):
    m = llama
    ids = _ids(m)
    T = ids.shape[1]
    plain = m.generate(ids, max_new_tokens=16, do_sample=False, pad_token_id=0)
    first = int(plain[0, T])
    sup = sorted({first, int(plain[0, T + 1])})
    out = m.generate(ids, max_new_tokens=16, do_sample=False, pad_token_id=0, suppress_tokens=sup)
    assert any(k[0] == "graph" and k[-1] == tuple(sup) for k in m._native_cache), "not served by the fused route"
    assert int(out[0, T]) != first and not set(sup) & set(out[0, T:].tolist())
    cap = m.generate(ids, max_new_tokens=8, do_sample=False, pad_token_id=0, capture=True, native=False, suppress_tokens=sup)
    assert not set(sup) & set(cap[0, T:].tolist())
    with pytest.raises(ValueError, match="suppress_tokens"):
        m.generate(ids, max_new_tokens=4, native=True, suppress_tokens=[[1, 2]])
