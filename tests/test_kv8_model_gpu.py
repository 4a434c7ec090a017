"""GPU: the fp8 (e4m3) KV cache through the model -- `setup_caches(1, 256, kv_cache_dtype="fp8")` on the six tiny models of
tests/test_prefill_chunked_gpu.py (built the same way here), the fused HIP route (`prefill_native`, `decode_native`, a captured
`DecodeGraph`, `generate(kv_cache_dtype="fp8")`) against the module forward over the SAME fp8 cache (`KVCache.update` stores by the write
rule and hands back the dequantised rows: the torch restatement of the feature).

Criterion: the form of test_prefill_chunked_gpu._close -- element-wise error against max|logit| (E) and relative norm (R).
Measured on MI355X, largest over the six models, the prompt passes (S = 70 in chunks of 32, S = 17) and 8 decode steps each:
    scales 1.0:               E = 4.74e-3, R = 4.74e-3   (window8, a decode step; the prompt passes stay below 1.2e-3 / 5e-4)
    the non-trivial scales:   E = 7.38e-3, R = 8.61e-3   (window8; the module forward rounds code * scale to fp16, the kernels keep fp32)
(the fp16 decode step against its module forward is held to 2e-2 of max|logit| in tests/test_decode_gpu.py: SDPA's fp16 arithmetic against
the kernels' fp32.)
Bounds: max(the fp16 file's 1e-2 / 3e-3, 2 x measured) -- the margin is for a cache code that flips where the two routes' fp32 sums
differ by an ulp.  What keeps the bounds meaningful: they stay below HALF the deviation between the fp8-cache and the fp16-cache module
forwards on the same inputs (printed and asserted per model; measured 7.5e-2 ... 1.1e-1 element-wise, 5.6e-2 ... 6.4e-2 norm-wise against
bounds of 1.48e-2 / 1.72e-2), so a route that ignored the cache format would fail."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CACHE = 256
CHUNK = 32
MEASURED_E, MEASURED_R = 7.38e-3, 8.61e-3  # the largest deviations measured (see the docstring)
E_BOUND, R_BOUND = max(1e-2, 2 * MEASURED_E), max(3e-3, 2 * MEASURED_R)


def _dev():
    return torch.device("cuda:0")


def _tiny(bits, name, hd=None, **extra):
    """the tiny models of test_decode_gpu._tiny_model / test_prefill_chunked_gpu._variant: the same widths, seeds and norm weights"""
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    d = _dev()
    dim = 8 * hd if hd else 512
    cfg = ModelArgs(block_size=256, vocab_size=1024, n_layer=2, n_head=8, dim=dim, intermediate_size=1024, n_local_heads=2, rope_base=500000,
                    model_name=name, **extra)
    m = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=bits, device=d)).to(device=d, dtype=torch.float16)
    random_init_(m, seed=bits, lut_std=0.05)
    g = torch.Generator(device=d)
    g.manual_seed(1)
    for b in m.layers:
        b.input_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
        b.post_attention_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
        if cfg.qk_norm:
            b.attention.q_norm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.head_dim, device=d, generator=g)).half())
            b.attention.k_norm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.head_dim, device=d, generator=g)).half())
    m.norm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
    return m.eval()


_BUILD = {
    "llama-2bit": lambda: _tiny(2, "llama-test", hd=64),
    "llama-4bit": lambda: _tiny(4, "llama-test", hd=64),
    "qwen3": lambda: _tiny(2, "qwen3-test", qk_norm=True, head_dim=64),
    "qwen2": lambda: _tiny(2, "qwen2-test", attn_bias=True),
    "window8": lambda: _tiny(2, "mistral-test", layer_windows=(8, 8)),
    "window24": lambda: _tiny(2, "mistral-test", layer_windows=(None, 24)),
}
_models = {}


def _inputs(m, S):
    d = _dev()
    g = torch.Generator(device=d).manual_seed(S)
    return torch.randint(0, m.config.vocab_size, (1, S + 8), dtype=torch.int32, device=d, generator=g), torch.arange(S + 8, dtype=torch.int32, device=d)


def _model(kind):
    """the model with an fp8 cache, and the fp16-cache module forward's logits on the S = 70 inputs (taken before the switch)"""
    if kind not in _models:
        m = _BUILD[kind]()
        m.setup_caches(1, CACHE)
        idx, pos = _inputs(m, 70)
        with torch.no_grad():
            ref16 = m(idx[:, :70], pos[:70]).float().clone()
        k16 = m.layers[0].attention.kv_cache.k_cache
        m.setup_caches(1, CACHE, kv_cache_dtype="fp8")
        assert m.kv_cache_dtype == "fp8" and m.max_seq_length == CACHE and m.native_ready() and m.kv8_unserved() is None
        kc = m.layers[0].attention.kv_cache
        assert kc.k_cache.dtype == torch.float8_e4m3fn and kc.k_cache.data_ptr() != k16.data_ptr() and kc.k_cache.shape == (1, 2, CACHE, m.config.head_dim)
        _models[kind] = (m, ref16)
    return _models[kind]


def _zero(m):
    for b in m.layers:
        b.attention.kv_cache.k_cache.view(torch.uint8).zero_()
        b.attention.kv_cache.v_cache.view(torch.uint8).zero_()


def _dev_of(got, want):
    scale = want.abs().max().item()
    return (got - want).abs().max().item() / scale, ((got - want).norm() / want.norm()).item()


_worst = [0.0, 0.0]


def _close(got, want, what):
    e, r = _dev_of(got, want)
    _worst[0], _worst[1] = max(_worst[0], e), max(_worst[1], r)
    print("%s: max|logit| %.3f  element-wise %.3e  norm-wise %.3e   (bounds %.3e / %.3e; worst so far %.3e / %.3e)" % (
        what, want.abs().max().item(), e, r, E_BOUND, R_BOUND, _worst[0], _worst[1]))
    assert torch.isfinite(got).all()
    assert e <= E_BOUND, (what, e)
    assert r <= R_BOUND, (what, r)


def _run(m, kind, S, chunk, decode, tag):
    """prompt pass against the module forward, rows >= S untouched, then 8 decode steps step by step over the same history"""
    idx, pos = _inputs(m, S)
    _zero(m)
    with torch.no_grad():
        want = m(idx[:, :S], pos[:S]).float().clone()
    _zero(m)
    with torch.no_grad():
        got = m.prefill_native(idx[:, :S], pos[:S], start=0, last_only=False, chunk=chunk).float().clone()
    assert m.last_prefill_plan["attn"] == ["hip-kv8"] * len(m.layers) and len(m.last_prefill_plan["chunks"]) == -(-S // chunk)
    _close(got, want, "%s %s prompt S=%d" % (kind, tag, S))
    for b in m.layers:
        for c in (b.attention.kv_cache.k_cache, b.attention.kv_cache.v_cache):
            assert bool((c.view(torch.uint8)[:, :, S:] == 0).all()), "rows behind the prompt were written"
    for t in range(S, S + 8):  # the module forward first, then the fused step over the same rows < t (each writes row t itself)
        with torch.no_grad():
            want = m(idx[:, t:t + 1], pos[t:t + 1]).float().clone()
            got = decode(idx[0, t:t + 1], pos[t:t + 1]).float().clone()
        _close(got.view(-1), want.view(-1), "%s %s step %d" % (kind, tag, t))
    for b in m.layers:
        assert bool((b.attention.kv_cache.k_cache.view(torch.uint8)[:, :, S + 8:] == 0).all())


@pytest.mark.parametrize("kind", list(_BUILD))
def test_fused_route_matches_the_module_forward_over_an_fp8_cache(kind, monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m, ref16 = _model(kind)
    one = torch.ones(len(m.layers), m.config.n_local_heads)
    m.set_kv_scales(one, one)
    # the condition that keeps the bounds meaningful: the cache format moves the logits by more than twice the bounds
    idx, pos = _inputs(m, 70)
    _zero(m)
    with torch.no_grad():
        ref8 = m(idx[:, :70], pos[:70]).float()
    e16, r16 = _dev_of(ref8, ref16)
    print("%s: fp8-cache vs fp16-cache module forward: element-wise %.3e  norm-wise %.3e" % (kind, e16, r16))
    assert E_BOUND < 0.5 * e16 and R_BOUND < 0.5 * r16, (e16, r16)
    _run(m, kind, 70, CHUNK, m.decode_native, "scale 1")
    _run(m, kind, 17, CHUNK, m.decode_native, "scale 1")


@pytest.mark.parametrize("kind", ["llama-2bit", "qwen3", "qwen2", "window8"])
def test_new_scales_reach_a_captured_graph_without_a_new_capture(kind, monkeypatch):
    from guidedquant_amd.generate import DecodeGraph
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m, _ = _model(kind)
    d = _dev()
    one = torch.ones(len(m.layers), m.config.n_local_heads)
    m.set_kv_scales(one, one)
    graph = DecodeGraph(m, d, temperature=0.0, top_k=32)
    gen, bound = m._alloc_gen, graph._signature()
    try:
        i = torch.arange(len(m.layers) * m.config.n_local_heads, dtype=torch.float32).view(len(m.layers), -1)
        m.set_kv_scales(0.37 + 0.11 * i, 2.9 - 0.3 * i)  # no powers of two, different per layer and head
        assert m._alloc_gen == gen and graph._signature() == bound  # nothing was re-allocated: the graph stays bound
        kc = m.layers[1].attention.kv_cache
        assert torch.allclose(kc.k_inv * kc.k_scale, torch.ones_like(kc.k_scale), rtol=1e-6) and float(kc.v_scale[1]) == pytest.approx(2.9 - 0.9)

        def replay(tok, pos):
            graph.set_token(tok, pos)
            graph.step(advance=False)
            return m._native_state()["logits"]
        _run(m, kind, 17, CHUNK, replay, "scales set")
    finally:
        graph.close()
        m.set_kv_scales(one, one)


def _hf_tiny():
    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                                  vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(hf, device=_dev(), seed=5)
    with torch.no_grad():
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    return m


def test_generate_with_an_fp8_cache_and_back(monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    m = _hf_tiny()
    d = m.device
    ids = torch.randint(0, 512, (1, 20), device=d, generator=torch.Generator(device=d).manual_seed(3))
    plain = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0)
    dec = m._native_cache[("decoder", 2)]
    assert dec.kv_cache_dtype == "fp16" and plain.shape == (1, 32)
    out = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0, kv_cache_dtype="fp8")
    assert out.shape == (1, 32) and torch.equal(out[:, :20], ids)
    assert dec.kv_cache_dtype == "fp8" and dec.layers[0].attention.kv_cache.k_cache.dtype == torch.float8_e4m3fn
    assert dec.last_prefill_plan["attn"] == ["hip-kv8"] * len(dec.layers)
    assert sum(1 for k in m._native_cache if k[0] == "graph") == 1
    # the same 12 tokens by hand: the prompt but for its last token through the prompt pass, then greedy decode_native steps
    ids32 = ids.view(-1).to(torch.int32)
    for b in dec.layers:
        b.attention.kv_cache.k_cache.view(torch.uint8).zero_()
        b.attention.kv_cache.v_cache.view(torch.uint8).zero_()
    with torch.no_grad():
        dec.prefill_native(ids32[:19], torch.arange(19, device=d, dtype=torch.int32), start=0)
        tok, hand = ids32[19:20], []
        for t in range(19, 31):
            logits = dec.decode_native(tok, torch.tensor([t], dtype=torch.int32, device=d))
            tok = logits.view(-1).float().argmax().to(torch.int32).view(1)
            hand.append(int(tok))
    assert out[0, 20:].tolist() == hand
    # a plain generate afterwards: an fp16 cache again, and the tokens it gave before
    again = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0)
    assert dec.kv_cache_dtype == "fp16" and dec.layers[0].attention.kv_cache.k_cache.dtype == torch.float16
    assert torch.equal(again, plain)
    # native_decoder(kv_cache_dtype=) hands the decoder back with caches of that dtype
    assert m.native_decoder(2, kv_cache_dtype="fp8") is dec and dec.kv_cache_dtype == "fp8"
    with pytest.raises(ValueError, match="kv_cache_dtype='fp8'"):
        m.generate(ids, max_new_tokens=4, do_sample=False, pad_token_id=0, kv_cache_dtype="fp8", native=False)
    with pytest.raises(ValueError, match="kv_cache_dtype='fp8'"):  # (beams: a request the fused route does not serve)
        m.generate(ids, max_new_tokens=4, num_beams=2, do_sample=False, pad_token_id=0, kv_cache_dtype="fp8")
