"""CPU: the host side of `score(..., ref_precision=)` -- the torch form of the KL head (native_prompt.kl_rows) against float64, the
module-tree route on a tiny random Any-Precision parent (2 and 3 bits), and the combinations the keyword declines."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_torch_form_matches_float64():
    from guidedquant_amd.native_prompt import kl_rows
    g = torch.Generator().manual_seed(0)
    lp, lq = (4 * torch.randn(37, 301, generator=g)).half(), (4 * torch.randn(37, 301, generator=g)).half()
    lq[5] = lp[5]
    kl, tp, tq = kl_rows(lp, lq, rows=16)  # (three row blocks)
    p64, q64 = torch.log_softmax(lp.double(), -1), torch.log_softmax(lq.double(), -1)
    want = (p64.exp() * (p64 - q64)).sum(-1)
    # fp32 log_softmax and a 301-term fp32 sum of terms bounded by max |logp - logq|: (V + 16) 2^-23 (1 + that), as for the kernel
    bound = (301 + 16) * 2.0**-23 * (1 + (p64 - q64).abs().amax(-1))
    assert kl.dtype == torch.float32 and bool(((kl.double() - want).abs() <= bound).all()) and float(kl[5]) == 0.0
    assert torch.equal(tp.long(), lp.float().argmax(-1)) and torch.equal(tq.long(), lq.float().argmax(-1))


@pytest.fixture(scope="module")
def parent():
    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                  vocab_size=128, max_position_embeddings=64, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=3, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    return AnyPrecisionForCausalLM.from_config_random(hf, device="cpu")


IDS = torch.tensor([3, 17, 5, 99, 0, 64, 127, 8, 21])


def test_score_with_ref_precision_on_the_module_tree(parent):
    m = parent
    plain = m.score(IDS, precision=2)
    assert set(plain) == {"logprobs", "greedy", "nll"}
    r = m.score(IDS, precision=2, ref_precision=3)
    assert set(r) == {"logprobs", "greedy", "nll", "kl", "kl_mean", "top1_agree"} and m.precision == max(m.precisions)
    assert torch.equal(r["logprobs"], plain["logprobs"]) and torch.equal(r["greedy"], plain["greedy"]) and r["nll"] == plain["nll"]
    assert r["kl"].shape == (8, ) and r["kl"].dtype == torch.float32 and r["top1_agree"].shape == (8, ) and r["top1_agree"].dtype == torch.bool
    assert isinstance(r["kl_mean"], float) and r["kl_mean"] == pytest.approx(float(r["kl"].double().mean())) and r["kl_mean"] > 0.0
    same = m.score(IDS, precision=2, ref_precision=2)
    assert bool((same["kl"] == 0.0).all()) and bool(same["top1_agree"].all()) and same["kl_mean"] == 0.0


def test_declined_combinations_raise(parent):
    m = parent
    for call in (lambda: m.score(IDS, ref_precision=5),
                 lambda: m.score(IDS, ref_precision=True),
                 lambda: m.score(IDS, ref_precision=3, top_logprobs=3),
                 lambda: m.score(IDS, ref_precision=3, lm_head_dtype="int8"),
                 lambda: m.perplexity(IDS, chunk_size=4, ref_precision=3),
                 lambda: m.loglikelihood(IDS[:5], IDS[5:], ref_precision=3),
                 lambda: m.score_many([IDS], ref_precision=3),
                 lambda: m.loglikelihood_many([(IDS[:5], IDS[5:])], ref_precision=3)):
        with pytest.raises(ValueError, match="ref_precision: "):
            call()
    with pytest.raises(ValueError, match="native=True"):  # (keeps raising where it raises)
        m.score(IDS, ref_precision=3, native=True)
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    for cls in (TensorParallelDecoder, PipelinedDecoder):
        with pytest.raises(NotImplementedError, match="scoring is not implemented"):
            cls.score_native(None, IDS, ref_hidden=None)
