"""GPU: the chunked prompt pass (`Transformer.prefill_native(..., chunk=)`, guidedquant_amd/native_prompt.py) with the HIP prompt attention
(gq_attn_prefill) and with SDPA, against the module forward; a cache beyond MASK_TABLE_MAX rows; `generate()` on a long-for-its-chunk
prompt.  Tolerances: tests/test_prefill_native_gpu.py's (max error <= 1e-2 max|logit|, relative norm <= 3e-3, caches <= 1e-2 of their max)."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CHUNK = 16
CACHE = 80


def _variant(bits, name, **extra):
    """`test_decode_gpu._tiny_model` with another block layout: the same widths, seeds and norm weights"""
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    d = torch.device("cuda:0")
    cfg = ModelArgs(block_size=256, vocab_size=1024, n_layer=2, n_head=8, dim=512, intermediate_size=1024, n_local_heads=2, rope_base=500000,
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
    "llama-2bit": lambda: __import__("test_decode_gpu")._tiny_model(2, hd=64),
    "llama-4bit": lambda: __import__("test_decode_gpu")._tiny_model(4, hd=64),
    "qwen3": lambda: _variant(2, "qwen3-test", qk_norm=True, head_dim=64),
    "qwen2": lambda: _variant(2, "qwen2-test", attn_bias=True),
    "window8": lambda: _variant(2, "mistral-test", layer_windows=(8, 8)),
    "window24": lambda: _variant(2, "mistral-test", layer_windows=(None, 24)),
}
_models, _wants = {}, {}


def _model(kind):
    if kind not in _models:
        m = _BUILD[kind]()
        m.setup_caches(1, CACHE)
        assert m.native_ready()
        _models[kind] = m
    return _models[kind]


def _zero(m):
    for b in m.layers:
        b.attention.kv_cache.k_cache.zero_()
        b.attention.kv_cache.v_cache.zero_()


def _want(kind, S):
    """the module forward's logits and caches, once per (model, S)"""
    if (kind, S) not in _wants:
        m = _model(kind)
        d = torch.device("cuda:0")
        g = torch.Generator(device=d).manual_seed(S)
        idx = torch.randint(0, m.config.vocab_size, (1, S), dtype=torch.int32, device=d, generator=g)
        pos = torch.arange(S, dtype=torch.int32, device=d)
        _zero(m)
        with torch.no_grad():
            want = m(idx, pos).float()
        kw = [b.attention.kv_cache.k_cache.clone() for b in m.layers]
        vw = [b.attention.kv_cache.v_cache.clone() for b in m.layers]
        _wants[(kind, S)] = (idx, pos, want, kw, vw)
    return _wants[(kind, S)]


def _close(got, want):
    scale = want.abs().max().item()
    err, rel = (got - want).abs().max().item(), ((got - want).norm() / want.norm()).item()
    print("max|logit| %.3f  element-wise %.3e  norm-wise %.3e" % (scale, err, rel))
    assert torch.isfinite(got).all()
    assert err <= 1e-2 * scale, (err, scale)
    assert rel <= 3e-3, rel


@pytest.mark.parametrize("attn", ["1", "0"])
@pytest.mark.parametrize("S", [70, 17])
@pytest.mark.parametrize("kind", list(_BUILD))
def test_chunked_pass_matches_module_forward(kind, S, attn, monkeypatch):
    from guidedquant_amd.model import prefill_chunks
    m = _model(kind)
    idx, pos, want, kw, vw = _want(kind, S)
    monkeypatch.setenv("GQ_PREFILL_ATTN", attn)
    _zero(m)
    with torch.no_grad():
        got = m.prefill_native(idx, pos, start=0, last_only=False, chunk=CHUNK).float()
        plan = m.last_prefill_plan
        last = m.prefill_native(idx, pos, start=0, last_only=True, chunk=CHUNK).float()
    torch.cuda.synchronize()
    assert plan["chunks"] == prefill_chunks(S, CHUNK) and len(plan["chunks"]) == -(-S // CHUNK) and plan["chunks"][-1][1] in (6, 1)
    assert plan["attn"] == ["hip" if attn == "1" else "sdpa"] * len(m.layers)
    assert got.shape == want.shape and last.shape == (1, 1, m.config.vocab_size)
    _close(got, want)
    assert (last[0, 0] - got[0, -1]).abs().max().item() <= 2e-3 * want.abs().max().item()
    for i, b in enumerate(m.layers):
        kc, vc = b.attention.kv_cache.k_cache, b.attention.kv_cache.v_cache
        assert (kc.float() - kw[i].float()).abs().max().item() <= 1e-2 * kw[i].float().abs().max().item()
        assert (vc.float() - vw[i].float()).abs().max().item() <= 1e-2 * vw[i].float().abs().max().item()
        assert bool((kc[:, :, S:] == 0).all()) and bool((vc[:, :, S:] == 0).all())  # only the prompt's positions were written


def test_default_switches_leave_a_short_prompt_on_sdpa_and_chunk_a_long_one(monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    monkeypatch.delenv("GQ_PREFILL_CHUNK", raising=False)
    m = _model("llama-2bit")
    idx, pos, want, _, _ = _want("llama-2bit", 70)
    _zero(m)
    with torch.no_grad():
        got = m.prefill_native(idx, pos, start=0, last_only=False).float()
    assert m.last_prefill_plan == dict(chunks=[(0, 70)], attn=["sdpa"] * len(m.layers))  # S <= chunk: what it always launched
    _close(got, want)
    # the chunk from the environment; auto takes the kernel inside a chunked pass
    monkeypatch.setenv("GQ_PREFILL_CHUNK", "32")
    _zero(m)
    with torch.no_grad():
        got = m.prefill_native(idx, pos, start=0, last_only=False).float()
    assert m.last_prefill_plan == dict(chunks=[(0, 32), (32, 32), (64, 6)], attn=["hip"] * len(m.layers))
    _close(got, want)
    monkeypatch.setenv("GQ_PREFILL_ATTN", "maybe")
    with pytest.raises(ValueError):
        m.prefill_native(idx, pos, start=0)


def test_a_cache_beyond_the_table_limit_serves_a_prompt_of_its_length(monkeypatch):
    import test_decode_gpu
    from guidedquant_amd.model import MASK_TABLE_MAX
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    monkeypatch.delenv("GQ_PREFILL_CHUNK", raising=False)
    d = torch.device("cuda:0")
    m = test_decode_gpu._tiny_model(2, hd=64)
    rows, S = 16392, 16390
    assert rows > MASK_TABLE_MAX
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.setup_caches(1, rows)
    assert m.max_seq_length == rows and getattr(m, "causal_mask", None) is None and not getattr(m, "window_masks", None)
    assert m.native_ready()
    g = torch.Generator(device=d).manual_seed(7)
    idx = torch.randint(0, m.config.vocab_size, (S, ), dtype=torch.int32, device=d, generator=g)
    pos = torch.arange(S, dtype=torch.int32, device=d)
    with torch.no_grad():
        hip = m.prefill_native(idx, pos, start=0).float().clone()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print("peak memory above the model: %.1f MB" % (grown / 1e6))
    assert grown < rows * rows  # one bool table of the cache's size: 268 MB
    assert m.last_prefill_plan == dict(chunks=[(0, 4096), (4096, 4096), (8192, 4096), (12288, 4096), (16384, 6)], attn=["hip"] * len(m.layers))
    # the last chunk alone over the same caches, through SDPA with the mask rows built from its positions
    monkeypatch.setenv("GQ_PREFILL_ATTN", "0")
    with torch.no_grad():
        sdpa = m.prefill_native(idx[16384:], pos[16384:], start=16384).float()
    assert m.last_prefill_plan == dict(chunks=[(16384, 6)], attn=["sdpa"] * len(m.layers))
    _close(hip, sdpa)


def test_generate_reaches_the_chunked_pass(monkeypatch):
    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                                  vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(hf, device=torch.device("cuda:0"), seed=5)
    with torch.no_grad():
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
    d = m.device
    g = torch.Generator(device=d).manual_seed(3)
    ids = torch.randint(0, 512, (1, 50), device=d, generator=g)
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    monkeypatch.setenv("GQ_PREFILL_CHUNK", str(CHUNK))
    out = m.generate(ids, max_new_tokens=4, do_sample=False, pad_token_id=0)
    assert ("decoder", 2) in m._native_cache and out.shape == (1, 54) and torch.equal(out[:, :50], ids)  # the fused route
    dec = m._native_cache[("decoder", 2)]
    # (the prompt but for its last token fills the caches: 49 tokens, a one-token tail)
    assert dec.last_prefill_plan == dict(chunks=[(0, 16), (16, 16), (32, 16), (48, 1)], attn=["hip"] * len(dec.layers))
    ids32, pos = ids.view(-1).to(torch.int32), torch.arange(50, device=d, dtype=torch.int32)
    with torch.no_grad():
        chunked = dec.prefill_native(ids32, pos, start=0).float().clone()
        assert len(dec.last_prefill_plan["chunks"]) == 4
        monkeypatch.delenv("GQ_PREFILL_CHUNK")
        whole = dec.prefill_native(ids32, pos, start=0).float().clone()
        assert dec.last_prefill_plan == dict(chunks=[(0, 50)], attn=["sdpa"] * len(dec.layers))
    _close(chunked, whole)
