"""GPU, model level: per-token log-probabilities from the fused decode route -- `DecodeGraph(logprobs=True)` and
`AnyPrecisionForCausalLM.generate(output_logprobs=True)`.

The tiny Llama of tests/test_repetition_penalty_routes_gpu.py (D = 512, 3 layers, V = 512, embeddings x 25, head x 10; the helper is
restated here).  DecodeGraph: after every step the step's logits are read from the decoder's native state and both numbers of that
position are checked against tests/sampler_lp_model.py with the bounds of tests/test_sampler_lp_gpu.py -- 4 * max(ref_err, ulp32(|lse|)),
ref_err taken on the step's own logits / kept candidates; an eight-step replay must leave the same bits.  generate: shapes, signs, the
EOS cut, the cache key, the fp8 cache, and the refusals.

Printed, not asserted: `logprobs` against `score(sequences)["logprobs"][T - 1:]` -- the prompt pass and the decode step round
differently (DESIGN.md section 4 has the first measurement).
"""
import numpy as np
import pytest

import sampler_lp_model as lp

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

_NAMES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
PROMPT = [3, 17, 5, 60, 2, 9]
SAMPLED = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.7, repetition_penalty=1.3)


def _llama(seed=5):
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2,
                                   vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=torch.device("cuda:0"), seed=seed)
    with torch.no_grad():  # (from_config_random draws N(0, 0.02) embeddings: scaled up so that the logits have margins)
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    return m


@pytest.fixture(scope="module")
def llama():
    return _llama()


def _ids(m, prompt=PROMPT):
    return torch.tensor([prompt], device=m.device)


def _bound(values32, lse):
    return 4.0 * max(lp.ref_err(values32), lp.ulp32(lse))


def _start(g, counter=5):
    g.seq.zero_()
    g.ban.zero_()
    g.rng_counter.fill_(counter)
    g.lp_raw.fill_(float("nan"))
    g.lp_drawn.fill_(float("nan"))
    g.set_token(7, 0)
    g.set_history([7])


@pytest.mark.parametrize("kw", [dict(temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=1.3), dict(temperature=0.0, top_k=1)], ids=["sampled", "greedy"])
def test_decode_graph_every_step_against_the_model(llama, kw):
    from guidedquant_amd.generate import DecodeGraph
    m, steps = llama, 24
    dec = m.native_decoder(2)
    m._evict("graph")
    dec.setup_caches(1, 256)
    rp = kw.get("repetition_penalty", 1.0)
    g = DecodeGraph(dec, m.device, native_sampling=True, fold_embed=True, seq_capacity=257, steps_per_replay=1, logprobs=True, **kw)
    try:
        assert g.lp_raw.shape == g.lp_drawn.shape == (257, ) and g.lp_raw.dtype == g.lp_drawn.dtype == torch.float32
        _start(g)
        history, worst, left_out = [7], [0.0, 0.0], 0
        for p in range(steps):
            g.step()
            torch.cuda.synchronize()
            logits = dec._native_state()["logits"].view(-1).cpu().numpy().view(np.float16)[:512].copy()
            tok = int(g.seq[p + 1])
            assert lp.specified(logits)
            d = lp.run(logits, [tok], top_k=kw["top_k"], T=kw["temperature"], top_p=kw.get("top_p", 1.0), pos=p, rp=rp, seen0=history, lp_cap=257).draws[0]
            got_raw, got_drawn = float(g.lp_raw[p + 1]), float(g.lp_drawn[p + 1])
            assert d.slot == p + 1
            b = _bound(logits.astype(np.float32), d.lse_raw)
            worst[0] = max(worst[0], abs(got_raw - d.raw) / b)
            assert abs(got_raw - d.raw) <= b, (p, tok, got_raw, d.raw, b)
            if kw["top_k"] == 1:
                assert got_drawn == 0.0
            elif d.decided:
                assert d.member, (p, tok)
                b = _bound(d.a, d.lse_drawn)
                worst[1] = max(worst[1], abs(got_drawn - d.drawn) / b)
                assert abs(got_drawn - d.drawn) <= b, (p, tok, got_drawn, d.drawn, b)
            else:
                left_out += 1
            history.append(tok)
        assert torch.isnan(g.lp_raw[steps + 1:]).all() and torch.isnan(g.lp_raw[:1]).all(), "a slot outside the run was written"
        print("DecodeGraph %s: worst |lp_raw - model| / bound %.3f, worst |lp_drawn - model| / bound %.3f, %d draws with an undecided nucleus"
              % (kw, worst[0], worst[1], left_out))
        one = (g.seq[:steps + 1].clone(), g.lp_raw[:steps + 1].clone(), g.lp_drawn[:steps + 1].clone())
    finally:
        g.close()
    g8 = DecodeGraph(dec, m.device, native_sampling=True, fold_embed=True, seq_capacity=257, steps_per_replay=8, logprobs=True, **kw)
    try:
        _start(g8)
        for _ in range(steps // 8):
            g8.step()
        torch.cuda.synchronize()
        assert torch.equal(g8.seq[:steps + 1], one[0])
        for a, b in ((g8.lp_raw, one[1]), (g8.lp_drawn, one[2])):
            assert torch.equal(a[1:steps + 1].view(torch.int32), b[1:].view(torch.int32)), "an eight-step replay leaves other bits than single steps"
        assert torch.isnan(g8.lp_raw[steps + 1:]).all()
    finally:
        g8.close()


def test_decode_graph_refuses_logprobs_without_the_fused_sampler_or_a_sequence_store(llama):
    from guidedquant_amd.generate import DecodeGraph
    m = llama
    dec = m.native_decoder(2)
    m._evict("graph")
    dec.setup_caches(1, 256)
    with pytest.raises(ValueError, match="logprobs"):
        DecodeGraph(dec, m.device, native_sampling=False, seq_capacity=16, temperature=0.0, top_k=1, logprobs=True)
    with pytest.raises(ValueError, match="logprobs"):
        DecodeGraph(dec, m.device, native_sampling=True, fold_embed=True, seq_capacity=0, temperature=0.0, top_k=1, logprobs=True)
    g = DecodeGraph(dec, m.device, native_sampling=True, fold_embed=True, seq_capacity=16, temperature=0.0, top_k=1)  # (the default allocates nothing)
    try:
        assert g.lp_raw is None and g.lp_drawn is None and g._lp_ws is None and g.logprobs is False
    finally:
        g.close()


def _graph_keys(m):
    return [k for k in m._native_cache if k[0] == "graph"]


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_generate_output_logprobs(llama, mode):
    m, new = llama, 24
    kw = dict(max_new_tokens=new, pad_token_id=0, **(SAMPLED if mode == "sampled" else dict(do_sample=False)))
    ids = _ids(m)
    T = ids.shape[1]
    m._evict("graph")
    torch.manual_seed(3)
    plain = m.generate(ids, **kw)
    assert torch.is_tensor(plain)
    plain_keys = _graph_keys(m)
    torch.manual_seed(3)
    out = m.generate(ids, output_logprobs=True, **kw)
    assert isinstance(out, transformers.utils.ModelOutput) and list(out.keys()) == ["sequences", "logprobs", "sampled_logprobs"]
    assert torch.equal(out.sequences, plain) and out.sequences.dtype == plain.dtype
    keys = _graph_keys(m)
    assert len(keys) == 1 and keys != plain_keys and ("logprobs", True) in keys[0] and ("logprobs", True) not in plain_keys[0]
    for t in (out.logprobs, out.sampled_logprobs):
        assert t.shape == (1, new) and t.dtype == torch.float32 and bool(torch.isfinite(t).all()) and bool((t <= 0).all())
    if mode == "greedy":
        assert bool((out.sampled_logprobs == 0.0).all())
    # against the prompt pass: printed, not asserted
    sc = m.score(out.sequences)["logprobs"][T - 1:].float().cpu()
    diff = (out.logprobs[0].cpu() - sc).abs()
    print("generate(%s): |logprobs - score(sequences)| max %.3e, mean %.3e over %d tokens" % (mode, float(diff.max()), float(diff.mean()), new))
    # EOS: an id from the plain run's continuation cuts all three at the same place
    eos = int(plain[0, T + 6])
    torch.manual_seed(3)
    cut_plain = m.generate(ids, eos_token_id=eos, **kw)
    torch.manual_seed(3)
    cut = m.generate(ids, eos_token_id=eos, output_logprobs=True, **kw)
    n = cut_plain.shape[1] - T
    assert 1 <= n <= 7 and int(cut_plain[0, -1]) == eos and torch.equal(cut.sequences, cut_plain)
    assert cut.logprobs.shape == cut.sampled_logprobs.shape == (1, n)
    assert torch.equal(cut.logprobs, out.logprobs[:, :n]) and torch.equal(cut.sampled_logprobs, out.sampled_logprobs[:, :n])
    # a second, shorter request on the cached graph returns its own values: those of a graph captured for it alone
    short = _ids(m, [9, 2, 60])
    kw2 = dict(kw, max_new_tokens=10)
    torch.manual_seed(4)
    b = m.generate(short, output_logprobs=True, **kw2)
    assert _graph_keys(m) == keys and b.logprobs.shape == (1, 10) and b.sequences.shape == (1, 13)
    m._evict("graph")
    torch.manual_seed(4)
    fresh = m.generate(short, output_logprobs=True, **kw2)
    assert torch.equal(b.sequences, fresh.sequences) and torch.equal(b.logprobs, fresh.logprobs) and torch.equal(b.sampled_logprobs, fresh.sampled_logprobs)
    assert not torch.equal(b.logprobs, out.logprobs[:, :10])


def test_generate_output_logprobs_with_an_fp8_cache_and_the_refusals(llama):
    m = llama
    ids = _ids(m)
    out = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0, kv_cache_dtype="fp8", output_logprobs=True)
    assert out.sequences.shape == (1, len(PROMPT) + 12)
    for t in (out.logprobs, out.sampled_logprobs):
        assert t.shape == (1, 12) and bool(torch.isfinite(t).all()) and bool((t <= 0).all())
    for kw in (dict(native=False), dict(capture=True), dict(capture=True, native=False), dict(num_beams=2)):
        with pytest.raises(ValueError, match="output_logprobs"):
            m.generate(ids, max_new_tokens=4, do_sample=False, pad_token_id=0, output_logprobs=True, **kw)
    # without the keyword nothing changed: a tensor, and `output_logprobs=False` is the plain call
    assert torch.is_tensor(m.generate(ids, max_new_tokens=4, do_sample=False, pad_token_id=0, output_logprobs=False))
