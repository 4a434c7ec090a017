"""No GPU: `model.fp8_row_quantize` (kv_cache_dtype="fp8_row") on hand-picked rows, and the refusals.  The exponent equals the rule in float64;
every element the clamp does not reach (|x| <= 448 * 2^e) meets e4m3's round-to-nearest bounds at the scale 2^e, |x - deq| <= 2^-4 |x| for
|x| >= 2^(e - 6) and <= 2^(e - 10) below; a magnitude above 448 * 2^7 = 57344 (e would be 8) saturates there: pinned on the 65504 row."""
import math

import pytest

torch = pytest.importorskip("torch")

HD = 64


def _row(amax_bits, seed):
    """head_dim fp16 values with the largest magnitude at `amax_bits`: the rest spread over 20 binades below it, signs mixed"""
    g = torch.Generator().manual_seed(seed)
    amax = torch.tensor([amax_bits], dtype=torch.int16).view(torch.float16).float()
    x = (amax * torch.rand(HD, generator=g) * 2.0 ** -torch.randint(0, 20, (HD,), generator=g).float()).half()
    x = torch.where(x.float().abs() < amax, x, torch.zeros_like(x)) * (1 - 2 * torch.randint(0, 2, (HD,), generator=g)).half()
    x[seed % HD] = -amax.half() if seed % 2 else amax.half()
    return x


def _bits(v):
    return int(torch.tensor([v]).half().view(torch.int16))


ROWS = {"zero": torch.zeros(HD).half(), "subnormals": (torch.arange(HD) * 16 + 1).to(torch.int16).view(torch.float16),
        "65504": _row(_bits(65504.0), 5), "inf": _row(_bits(3.0), 6), "nan": _row(_bits(0.3), 7)}
ROWS["inf"][2], ROWS["inf"][9], ROWS["nan"][4] = float("inf"), float("-inf"), float("nan")
for k in (-15, -9, 0, 7):  # amax exactly at 448 * 2^k, one fp16 step above and below
    for name, step in (("at", 0), ("above", 1), ("below", -1)):
        ROWS["%s-448*2^%d" % (name, k)] = _row(_bits(448.0 * 2.0**k) + step, 40 + k)


@pytest.mark.parametrize("name", list(ROWS))
def test_exponent_and_error_bounds_of_a_row(name):
    from guidedquant_amd.model import fp8_row_quantize, fp8_row_scale
    x = ROWS[name]
    codes, byte = fp8_row_quantize(x.view(1, HD))
    xd = x.double()
    finite = torch.isfinite(xd)
    amax = float(xd[finite].abs().max())
    want = max(-15, min(7, math.ceil(math.log2(amax / 448.0)))) if amax > 0 else -15
    e = int(byte) - 127
    assert e == want, (name, e, want, amax)
    deq = (codes.view(torch.float8_e4m3fn).float() * fp8_row_scale(byte)[..., None]).view(HD)
    inf, nan = torch.isinf(xd), torch.isnan(xd)
    assert torch.equal(deq[~nan].half().float(), deq[~nan])  # the read rule's product is an fp16 value
    assert torch.equal(deq[inf], torch.sign(x[inf]).float() * 448.0 * 2.0**e) and bool(torch.isnan(deq[nan]).all())
    over = finite & (xd.abs() > 448.0 * 2.0**e)  # (only where e is clamped at 7)
    assert bool(over.any()) == (name in ("65504", "above-448*2^7")) and torch.equal(deq[over].abs(), torch.full_like(deq[over], 57344.0))
    ok, err = finite & ~over, (xd - deq.double()).abs()
    big = xd.abs() >= 2.0 ** (e - 6)
    assert bool((err[ok & big] <= 2.0**-4 * xd.abs()[ok & big]).all()) and bool((err[ok & ~big] <= 2.0 ** (e - 10)).all()), name


def _tiny():
    from guidedquant_amd.model import ModelArgs, Transformer
    return Transformer(torch.float32, ModelArgs(dim=256, n_head=4, n_local_heads=2, n_layer=2, vocab_size=64, intermediate_size=512, block_size=64,
                                                model_name="llama-tiny")).eval()


def test_routes_that_do_not_serve_the_format_say_so():
    from guidedquant_amd import model as gm
    from guidedquant_amd.generate import load_model
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    m = _tiny()
    with pytest.raises(ValueError, match="kv_cache_dtype='fp8_col': None, 'fp16' or 'fp8'.*fp8_row"):
        m.setup_caches(1, 8, kv_cache_dtype="fp8_col")
    m.setup_caches(1, 8, kv_cache_dtype="fp8_row")
    with pytest.raises(ValueError, match="set_kv_scales: an fp8_row cache has no per-head scales"):
        m.set_kv_scales(torch.ones(2, 2), torch.ones(2, 2))
    with pytest.raises(NotImplementedError, match="fp8_row KV cache: tensor-parallel"):
        TensorParallelDecoder(m, None, 0, 2, 4)
    with pytest.raises(NotImplementedError, match="fp8_row KV cache: layer-pipelined"):
        PipelinedDecoder(m, 0, 1, range(0, 2), n_seq=1, max_new_tokens=4)
    gm.transformer_configs["qtip-test"] = dict(model_name="llama-qtip-test", block_size=64, vocab_size=128, n_layer=1, n_head=4, dim=256, intermediate_size=512,
                                               n_local_heads=2)
    try:
        q = load_model("qtip-test", "cpu", "qtip", 2, random_init=True)
    finally:
        del gm.transformer_configs["qtip-test"]
    with pytest.raises(NotImplementedError, match="fp8_row KV cache: QTIP"):
        q.setup_caches(1, 8, kv_cache_dtype="fp8_row")

    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                  vocab_size=128, max_position_embeddings=64, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(hf, device="cpu")
    ids = torch.tensor([[3, 17, 5]])
    with pytest.raises(ValueError, match="kv_cache_dtype='fp8_row': the fused routes need the GPU"):
        m.generate(ids, max_new_tokens=2, do_sample=False, kv_cache_dtype="fp8_row")
    m._adapter = object()  # (any adapter: the refusal comes before it is looked at)
    with pytest.raises(ValueError, match="lora: the adapter is served by the fused decode model with an fp16 cache only"):
        m.score(ids, kv_cache_dtype="fp8_row")
