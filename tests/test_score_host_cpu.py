"""No GPU: the scoring surface of AnyPrecisionForCausalLM -- `score`, `perplexity`, `loglikelihood` -- on the module tree (the route a
CPU model takes), against the module forward's own `labels=` loss and the reference's perplexity formula
(any_precision/evaluate/eval.py:205-226), plus the named errors."""
import math

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

VOCAB = 128


@pytest.fixture(scope="module")
def wrapper():
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                  vocab_size=VOCAB, max_position_embeddings=64, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    return AnyPrecisionForCausalLM.from_config_random(hf, device="cpu")


@pytest.fixture(scope="module")
def stream():
    return torch.randint(0, VOCAB, (50, ), generator=torch.Generator().manual_seed(3))


def test_score_is_the_module_forwards_labels_loss(wrapper, stream):
    ids = stream[:17]
    r = wrapper.score(ids)
    assert r["logprobs"].shape == (16, ) and r["logprobs"].dtype == torch.float32 and r["greedy"].shape == (16, ) and r["greedy"].dtype == torch.bool
    assert bool((r["logprobs"] < 0).all())
    with torch.no_grad():
        out = wrapper.model(input_ids=ids.view(1, -1), labels=ids.view(1, -1))
    assert r["nll"] == pytest.approx(float(out.loss), rel=1e-5, abs=1e-6)
    assert r["nll"] == pytest.approx(float(-r["logprobs"].double().mean()), abs=1e-12)
    assert torch.equal(r["greedy"], out.logits[0, :-1].float().argmax(-1) == ids[1:])
    # [1, T] is the same request; native=False too
    r2 = wrapper.score(ids.view(1, -1), native=False)
    assert torch.equal(r2["logprobs"], r["logprobs"]) and torch.equal(r2["greedy"], r["greedy"])


def test_perplexity_is_the_reference_formula_and_drops_the_tail(wrapper, stream):
    p = wrapper.perplexity(stream, chunk_size=16)  # 50 tokens: three chunks, two tokens dropped
    assert len(p["nll_per_chunk"]) == 3
    by_hand = [wrapper.score(stream[i * 16:(i + 1) * 16])["nll"] for i in range(3)]
    assert p["nll_per_chunk"] == by_hand
    assert p["ppl"] == pytest.approx(math.exp(sum(by_hand) / 3), rel=1e-12)
    # the reference's loop itself: outputs.loss per chunk, exp of the mean of the stack
    with torch.no_grad():
        losses = [wrapper.model(input_ids=stream[None, i * 16:(i + 1) * 16], labels=stream[None, i * 16:(i + 1) * 16]).loss for i in range(3)]
    assert p["ppl"] == pytest.approx(float(torch.exp(torch.stack(losses).mean())), rel=1e-5)
    assert wrapper.perplexity(stream[:48], chunk_size=16) == p  # (the tail changed nothing)
    with pytest.raises(ValueError, match="whole chunk"):
        wrapper.perplexity(stream[:15], chunk_size=16)
    with pytest.raises(ValueError, match="1-D"):
        wrapper.perplexity(stream.view(1, -1), chunk_size=16)


def test_loglikelihood_covers_the_continuation_only(wrapper, stream):
    ctx, cont = stream[:9], stream[9:14]
    ll, greedy = wrapper.loglikelihood(ctx, cont)
    r = wrapper.score(stream[:14])
    assert ll == pytest.approx(float(r["logprobs"][8:].double().sum()), abs=1e-12)  # logprobs[8] scores token 9, the continuation's first
    assert greedy == bool(r["greedy"][8:].all())
    assert isinstance(ll, float) and isinstance(greedy, bool)
    # a one-token context and a one-token continuation
    ll1, _ = wrapper.loglikelihood(stream[:1], stream[1:2])
    assert ll1 == pytest.approx(float(wrapper.score(stream[:2])["logprobs"][0]), abs=1e-12)


def test_errors(wrapper, stream, monkeypatch):
    with pytest.raises(ValueError, match="token ids must lie in"):
        wrapper.score(torch.tensor([3, VOCAB, 5]))
    with pytest.raises(ValueError, match="token ids must lie in"):
        wrapper.score(torch.tensor([3, -1, 5]))
    with pytest.raises(ValueError, match="continuation"):
        wrapper.loglikelihood(stream[:4], stream[:0])
    with pytest.raises(ValueError, match="at least two tokens"):
        wrapper.score(stream[:1])
    with pytest.raises(ValueError, match="one sequence"):
        wrapper.score(stream[:8].view(2, 4))
    with pytest.raises(ValueError, match="native=True: the fused routes need the GPU"):
        wrapper.score(stream[:8], native=True)
    with pytest.raises(ValueError, match="kv_cache_dtype='fp8': the fused routes need the GPU"):
        wrapper.score(stream[:8], kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        wrapper.score(stream[:8], kv_cache_dtype="fp4")
    prec = wrapper.precision
    with pytest.raises(ValueError):
        wrapper.score(stream[:1], precision=2)
    assert wrapper.precision == prec


def test_a_bad_score_head_switch_is_named(monkeypatch):
    """GQ_SCORE_HEAD is read by Transformer.score_native in front of every launch: anything but auto / 0 / 1 raises like GQ_PREFILL_ATTN"""
    from guidedquant_amd.model import ModelArgs, Transformer
    m = Transformer(torch.float16, ModelArgs(dim=256, n_head=4, n_local_heads=2, n_layer=1, vocab_size=64, intermediate_size=512, block_size=64,
                                             model_name="llama-tiny")).eval()
    m.setup_caches(1, 16)
    monkeypatch.setattr(Transformer, "prefill_ready", lambda self, idx: True)  # (the switch is checked before anything touches the GPU)
    monkeypatch.setenv("GQ_SCORE_HEAD", "2")
    with pytest.raises(ValueError, match="GQ_SCORE_HEAD='2': auto, 0 or 1"):
        m.score_native(torch.tensor([1, 2, 3]))


def test_sharded_decoders_decline():
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    for cls in (TensorParallelDecoder, PipelinedDecoder):
        with pytest.raises(NotImplementedError, match="scoring"):
            cls.score_native(object())
