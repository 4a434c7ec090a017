"""No GPU: `AnyPrecisionForCausalLM.score_many` / `loglikelihood_many` off the fused route -- a CPU model loops over `score`, native=True
raises instead of falling back -- and the named errors."""
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


def _seqs():
    g = torch.Generator().manual_seed(4)
    return [torch.randint(0, VOCAB, (n, ), generator=g) for n in (17, 2, 9)]


def test_a_cpu_model_loops_over_score(wrapper):
    seqs = _seqs()
    one = [wrapper.score(s) for s in seqs]
    for kw in (dict(), dict(native=False), dict(pack_tokens=16)):
        many = wrapper.score_many(seqs, **kw)
        assert len(many) == 3
        for a, b in zip(many, one):
            assert torch.equal(a["logprobs"], b["logprobs"]) and torch.equal(a["greedy"], b["greedy"]) and a["nll"] == b["nll"]
    assert torch.equal(wrapper.score_many([seqs[0].view(1, -1)])[0]["logprobs"], one[0]["logprobs"])  # ([1, T] is the same request)
    assert wrapper.score_many([]) == []


def test_loglikelihood_many_is_loglikelihood_per_pair(wrapper):
    seqs = _seqs()
    pairs = [(seqs[0][:12], seqs[0][12:]), (seqs[1][:1], seqs[1][1:]), (seqs[2][:1], seqs[2][1:])]
    got = wrapper.loglikelihood_many(pairs)
    assert got == [wrapper.loglikelihood(c, t) for c, t in pairs]
    assert all(isinstance(ll, float) and isinstance(g, bool) for ll, g in got)


def test_named_errors(wrapper):
    seqs = _seqs()
    with pytest.raises(ValueError, match="native=True: the fused routes need the GPU"):
        wrapper.score_many(seqs, native=True)
    with pytest.raises(ValueError, match="native=True"):
        wrapper.loglikelihood_many([(seqs[0][:3], seqs[0][3:])], native=True)
    with pytest.raises(ValueError, match=r"token ids must lie in \[0, 128\)"):
        wrapper.score_many([seqs[0], torch.tensor([1, VOCAB])])
    with pytest.raises(ValueError, match="at least two tokens"):
        wrapper.score_many([torch.tensor([5])])
    with pytest.raises(ValueError, match="token ids"):
        wrapper.score_many([torch.tensor([0.5, 1.0])])
    with pytest.raises(ValueError, match="pack_tokens"):
        wrapper.score_many(seqs, pack_tokens=1)
    with pytest.raises(ValueError, match="at least one token each"):
        wrapper.loglikelihood_many([(seqs[0], seqs[0][:0])])
    prev = wrapper.precision
    wrapper.score_many(seqs[:1], precision=prev)
    assert wrapper.precision == prev
