"""GPU, model level: the whole-vocabulary sampler (gq_sample_full) behind `DecodeGraph` and behind `AnyPrecisionForCausalLM.generate`.

DecodeGraph, on the tiny Llama of tests/test_decode_logprobs_gpu.py (D = 512, 3 layers, V = 512; the helper is restated here):
`native_sampling=True, fold_embed=True, steps_per_replay=10, seq_capacity=..., logprobs=True` with top_k=None / top_p=0.9 and with
top_k=200 / min_p=0.05 / a penalty -- 40 tokens through multi-step replays equal 40 single `step_one` steps from the same seed, bit for bit in
the tokens and in both log-probabilities; native sampling stays native; min_p on the torch-sampling path raises.

HF surface, on the tiny Any-Precision checkpoint of ap_helpers: `generate(do_sample=True, top_k=0, top_p=0.9, native=True)` and
`generate(do_sample=True, min_p=0.1, native=True, output_logprobs=True)` (both raise on the commit before this sampler) return
[1, T + new], are reproducible under torch.manual_seed, also with an fp8 cache; `sampled_logprobs` is sampler_full_model's number for the
drawn tokens, from the logits of a SECOND decoder pass over the returned sequence.  `generate` keeps no logits, and a second pass may
round a logit one fp16 ulp away, so that check is a coarse one (2^-4: it tells a wrong candidate set, a missing temperature or filter);
the tight bound on lp_drawn -- G_MASS + 4 ulp, on the logits of the drawing step itself -- is the DecodeGraph test's
(`test_last_step_against_the_model...`) and, per case, tests/test_sampler_full_gpu.py's."""
import numpy as np
import pytest

import sampler_full_model as fm
import sampler_lp_model as lp
from ap_helpers import tiny_hf_anyprec_checkpoint

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

_NAMES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]


@pytest.fixture(scope="module")
def llama():
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2,
                                   vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=torch.device("cuda:0"), seed=5)
    with torch.no_grad():
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(4.0)
    return m


def _start(g, counter=5):
    g.seq.zero_()
    g.ban.zero_()
    g.rng_counter.fill_(counter)
    g.lp_raw.fill_(float("nan"))
    g.lp_drawn.fill_(float("nan"))
    g.set_token(7, 0)
    g.set_history([7])


@pytest.mark.parametrize("kw", [dict(temperature=0.8, top_k=None, top_p=0.9), dict(temperature=0.9, top_k=200, min_p=0.05, repetition_penalty=1.3)],
                         ids=["no_top_k_nucleus", "k200_min_p_penalty"])
def test_multi_step_replays_equal_single_steps(llama, kw):
    from guidedquant_amd.generate import DecodeGraph
    m, steps = llama, 40
    dec = m.native_decoder(2)
    m._evict("graph")
    dec.setup_caches(1, 256)
    g = DecodeGraph(dec, m.device, native_sampling=True, fold_embed=True, seq_capacity=257, steps_per_replay=10, logprobs=True, **kw)
    try:
        assert g.native_sampling and g.fold_embed and g.steps_per_replay == 10 and g.sampler.full and g.work_val is None
        _start(g)
        for _ in range(steps):
            g.step_one()
        torch.cuda.synchronize()
        one = (g.seq[:steps + 1].clone(), g.lp_raw[:steps + 1].clone(), g.lp_drawn[:steps + 1].clone())
        assert int(g.pos) == steps and len(set(one[0][1:].tolist())) > 4, "the draws do not vary"
        assert bool(torch.isfinite(one[1][1:]).all()) and bool(torch.isfinite(one[2][1:]).all()) and bool((one[2][1:] <= 0).all())
        _start(g)
        for _ in range(steps // 10):
            g.step()
        torch.cuda.synchronize()
        assert torch.equal(g.seq[:steps + 1], one[0])
        for a, b in ((g.lp_raw, one[1]), (g.lp_drawn, one[2])):
            assert torch.equal(a[1:steps + 1].view(torch.int32), b[1:].view(torch.int32)), "a ten-step replay leaves other bits than single steps"
        assert torch.isnan(g.lp_raw[steps + 1:]).all()
        if kw.get("repetition_penalty"):
            seen = np.zeros(512, dtype=bool)
            seen[[7] + one[0][1:].tolist()] = True
            assert np.array_equal(np.unpackbits(g.seen.cpu().numpy().view(np.uint8), bitorder="little")[:512].astype(bool), seen)
    finally:
        g.close()


def test_last_step_against_the_model_and_the_torch_path_refuses_min_p(llama):
    """one step's numbers against sampler_full_model, from the logits the step left in the decoder's state"""
    from guidedquant_amd.generate import DecodeGraph
    m = llama
    dec = m.native_decoder(2)
    m._evict("graph")
    dec.setup_caches(1, 256)
    with pytest.raises(ValueError, match="min_p"):
        DecodeGraph(dec, m.device, native_sampling=False, temperature=0.8, top_k=50, min_p=0.05)
    g = DecodeGraph(dec, m.device, native_sampling=True, fold_embed=True, seq_capacity=257, logprobs=True, temperature=0.8, top_k=200, top_p=0.9, min_p=0.02)
    try:
        _start(g, counter=11)
        for p in range(6):
            g.step()
            torch.cuda.synchronize()
            logits = dec._native_state()["logits"].view(-1).cpu().numpy().view(np.float16)[:512].copy()
            tok = int(g.seq[p + 1])
            r = fm.run(logits, 1, 200, 0.8, 0.9, 0.02, seed=g.seed, counter=11 + p, pos=p, seq_cap=257, forced=[tok])
            assert tok in r.admissible[0].tolist() and (bool(r.undecided[0]) or tok == int(r.tokens[0])), (p, tok, r.tokens[0])
            if r.n_lo[0] == r.n_hi[0]:
                want = r.lp_drawn[p + 1]
                assert abs(float(g.lp_drawn[p + 1]) - want) <= fm.G_MASS + 4 * lp.ulp32(max(abs(want), 1.0)), (p, float(g.lp_drawn[p + 1]), want)
            v32 = logits.astype(np.float32)
            assert abs(float(g.lp_raw[p + 1]) - r.lp_raw[p + 1]) <= 4 * max(lp.ref_err(v32), lp.ulp32(lp.lse64(v32)))
    finally:
        g.close()


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    path = tmp_path_factory.mktemp("tiny_ap")
    tiny_hf_anyprec_checkpoint(path, D=512, I=1024, H=8, KV=2, V=256)
    return AnyPrecisionForCausalLM.from_quantized(str(path))


def test_generate_without_top_k_and_with_min_p(tiny):
    m = tiny
    ids = torch.tensor([[3, 17, 5, 60, 2]], device=m.device)
    T, new = ids.shape[1], 20
    calls = (dict(top_k=0, top_p=0.9), dict(min_p=0.1, output_logprobs=True), dict(top_k=0, min_p=0.05, kv_cache_dtype="fp8", output_logprobs=True))
    for extra in calls:
        kw = dict(max_new_tokens=new, min_new_tokens=new, do_sample=True, temperature=1.0, pad_token_id=0, native=True, **extra)  # (EOS banned: the ban list)
        torch.manual_seed(21)
        a = m.generate(ids, **kw)
        b = m.generate(ids, **kw)
        torch.manual_seed(21)
        a2 = m.generate(ids, **kw)
        sa, sb, sa2 = [(o.sequences if "output_logprobs" in extra else o) for o in (a, b, a2)]
        assert sa.shape == (1, T + new) and torch.equal(sa[:, :T], ids) and int(sa.max()) < 256
        assert torch.equal(sa, sa2) and not torch.equal(sa, sb), extra
        if "output_logprobs" in extra:
            assert a.logprobs.shape == a.sampled_logprobs.shape == (1, new)
            assert torch.equal(a.logprobs, a2.logprobs) and torch.equal(a.sampled_logprobs, a2.sampled_logprobs)
            assert bool(torch.isfinite(a.logprobs).all()) and bool((a.sampled_logprobs <= 0).all()) and bool((a.sampled_logprobs >= a.logprobs - 1e-4).all())
    # the whole-vocabulary sampler ran: the cached graphs carry it
    graphs = [v for k, v in m._native_cache.items() if k[0] == "graph"]
    assert graphs and all(g.sampler.full for g in graphs)
    # top_k above 64 stays declined on this surface
    with pytest.raises(ValueError):
        m.generate(ids, max_new_tokens=4, do_sample=True, top_k=100, native=True)
    with pytest.raises(ValueError):
        m.generate(ids, max_new_tokens=4, do_sample=True, top_k=0, native=False, capture=True)


def test_sampled_logprobs_are_the_models_number(tiny):
    """min_p = 0.1 over the default top_k = 50: every generated token's sampled_logprobs against sampler_full_model on the logits of the step
    that drew it (the fused decoder stepped again over the returned sequence, one token at a time)"""
    m = tiny
    ids = torch.tensor([[3, 17, 5, 60, 2]], device=m.device)
    T, new = ids.shape[1], 24
    torch.manual_seed(5)
    out = m.generate(ids, max_new_tokens=new, min_new_tokens=new, do_sample=True, temperature=0.9, min_p=0.1, pad_token_id=0, native=True, output_logprobs=True)
    seq = out.sequences[0].to(torch.int32)
    dec = m.native_decoder(m.precision)
    compared = 0
    eos = m.model.generation_config.eos_token_id
    eos = [] if eos is None else ([int(eos)] if isinstance(eos, int) else [int(e) for e in eos])
    ban = (len(eos), T - 1 + new, tuple(eos) + (0, ) * (4 - len(eos)))  # (min_new_tokens: EOS cannot be drawn)
    with torch.inference_mode():
        pre, pos = seq[:T - 1], torch.arange(0, T - 1, device=m.device, dtype=torch.int32)
        if dec.prefill_ready(pre):  # (the prompt as `generate` runs it)
            dec.prefill_native(pre, pos, start=0)
        else:
            dec(pre.view(1, -1), pos)
        for p in range(T - 1, T + new - 1):
            dec.decode_native(seq[p:p + 1], torch.tensor([p], device=m.device, dtype=torch.int32))
            x = dec._native_state()["logits"].view(-1).cpu().numpy().view(np.float16)[:256].copy()
            tok = int(seq[p + 1])
            # the second pass may leave logits one fp16 ulp (2^-6 below 16) from the drawing step's: a draw is compared where the candidate
            # count does not depend on it -- the same count with the min_p threshold moved by e^(+-2^-5)
            rs = [fm.run(x, 1, 50, 0.9, 1.0, mp, forced=[tok], pos=p, seq_cap=p + 3, ban=ban) for mp in (0.1, 0.1 * np.exp(-2.0**-5), 0.1 * np.exp(2.0**-5))]
            r = rs[0]
            if len({int(q.n[0]) for q in rs}) != 1 or r.n_lo[0] != r.n_hi[0] or not np.isfinite(r.lp_drawn[p + 1]):
                continue
            compared += 1
            got = float(out.sampled_logprobs[0, p - (T - 1)])
            # (one fp16 ulp of a logit moves a log-probability by at most 2^-6 / T twice over -- a wrong candidate set moves it by far more)
            assert abs(got - r.lp_drawn[p + 1]) <= 2.0**-4 + fm.G_MASS, (p, tok, got, r.lp_drawn[p + 1])
    assert compared >= new // 3
