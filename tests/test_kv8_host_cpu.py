"""No GPU: the host side of the fp8 (e4m3) KV cache -- `KVCache.update` against the host model of the write rule (clamp, tie and flush
cases included), `Transformer.set_kv_scales` validation, `setup_caches` re-allocating on a dtype change, the byte offsets of a batch
slot for both dtypes, and the named errors of the routes that do not serve the format."""
import pytest

torch = pytest.importorskip("torch")

import kv8_model as k8  # noqa: E402


def _tiny(**extra):
    from guidedquant_amd.model import ModelArgs, Transformer
    kw = dict(dim=256, n_head=4, n_local_heads=2, n_layer=2, vocab_size=64, intermediate_size=512, block_size=64, model_name="llama-tiny")
    kw.update(extra)
    return Transformer(torch.float32, ModelArgs(**kw)).eval()


def test_update_stores_by_the_write_rule_and_returns_the_dequantised_rows():
    from guidedquant_amd.model import KVCache
    c = KVCache(1, 8, 2, 64, torch.float16, "cpu", fp8=True)
    assert c.k_cache.dtype == torch.float8_e4m3fn and c.k_cache.element_size() == 1 and c.k_cache.shape == (1, 2, 8, 64)
    for name in ("k_scale", "v_scale", "k_inv", "v_inv"):
        assert getattr(c, name).dtype == torch.float32 and getattr(c, name).tolist() == [1.0, 1.0]
    # the cases of the rule at scale 1: 449 -> 448 (behind the clamp only), ties 17 -> 16 and 19 -> 20, 2^-10 -> 0, 1.5 * 2^-10 -> 2^-9
    x = torch.zeros(1, 2, 1, 64, dtype=torch.float16)
    cases = [449.0, -449.0, 60000.0, 17.0, 19.0, 2.0**-10, 1.5 * 2.0**-10, -2.0**-11, 448.0, 1.0]
    want = [448.0, -448.0, 448.0, 16.0, 20.0, 0.0, 2.0**-9, -0.0, 448.0, 1.0]
    x[0, :, 0, :len(cases)] = torch.tensor(cases).half()
    k, v = c.update(torch.tensor([3], dtype=torch.int32), x, x)
    assert k.dtype == torch.float16 and k.shape == (1, 2, 8, 64)
    assert k[0, 1, 3, :len(cases)].tolist() == want and v[0, 0, 3, :len(cases)].tolist() == want
    assert bool((c.k_cache.view(torch.uint8)[:, :, [0, 1, 2, 4, 5, 6, 7]] == 0).all())
    # scales that are no powers of two, random rows at several positions: byte for byte the host model
    c.set_scales(torch.tensor([0.37, 2.9]), torch.tensor([1.3, 0.051]))
    assert torch.equal(c.k_inv, torch.reciprocal(c.k_scale)) and torch.equal(c.v_inv, torch.reciprocal(c.v_scale))
    g = torch.Generator().manual_seed(0)
    kx = (torch.randn(1, 2, 3, 64, generator=g) * torch.tensor([600.0, 1.0, 2.0**-11])[None, None, :, None]).half()
    vx = torch.randn(1, 2, 3, 64, generator=g).half()
    pos = torch.tensor([0, 7, 2], dtype=torch.int32)
    k, v = c.update(pos, kx, vx)
    for cache, x16, inv, scale, out in ((c.k_cache, kx, c.k_inv, c.k_scale, k), (c.v_cache, vx, c.v_inv, c.v_scale, v)):
        codes = k8.quantize(x16[0], inv[:, None, None])
        assert torch.equal(cache.view(torch.uint8)[0][:, pos.long()], codes)
        assert torch.equal(out[0][:, pos.long()], (k8.TABLE[codes.long()] * scale[:, None, None]).half())
    assert int((kx.float().abs() * c.k_inv[None, :, None, None] > 448).sum()) > 0  # (some values clamped)


def test_an_fp16_cache_is_what_it_was():
    from guidedquant_amd.model import KVCache
    c = KVCache(1, 8, 2, 64, torch.float16, "cpu")
    assert sorted(c.state_dict()) == ["k_cache", "v_cache"] and c.k_cache.dtype == torch.float16
    x = torch.randn(1, 2, 1, 64).half()
    k, v = c.update(torch.tensor([5], dtype=torch.int32), x, x)
    assert k.data_ptr() == c.k_cache.data_ptr() and torch.equal(k[:, :, 5:6], x)


def test_setup_caches_reallocates_on_a_dtype_change_only():
    m = _tiny()
    m.setup_caches(1, 32)
    assert m.kv_cache_dtype == "fp16"
    k16, gen = m.layers[0].attention.kv_cache.k_cache, m._alloc_gen
    m.setup_caches(1, 16)                          # suffices: nothing happens
    m.setup_caches(1, 16, kv_cache_dtype="fp16")   # the default by name
    assert m.layers[0].attention.kv_cache.k_cache is k16 and m._alloc_gen == gen
    m.setup_caches(1, 16, kv_cache_dtype="fp8")    # the size suffices, the dtype differs
    kc = m.layers[0].attention.kv_cache
    assert m.kv_cache_dtype == "fp8" and kc.k_cache.dtype == torch.float8_e4m3fn and kc.fp8 and m._alloc_gen > gen and m._native is None
    k8c, gen = kc.k_cache, m._alloc_gen
    m.setup_caches(1, 8, kv_cache_dtype="fp8")
    assert m.layers[0].attention.kv_cache.k_cache is k8c and m._alloc_gen == gen
    m.setup_caches(1, 8)                           # None is the default dtype: fp16 again
    assert m.kv_cache_dtype == "fp16" and m.layers[0].attention.kv_cache.k_cache.dtype == torch.float32  # (the model's own dtype)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        m.setup_caches(1, 8, kv_cache_dtype="int4")


def test_the_module_forward_runs_over_an_fp8_cache():
    m = _tiny()
    idx = torch.randint(0, 64, (1, 9), generator=torch.Generator().manual_seed(1))
    pos = torch.arange(9, dtype=torch.int32)
    m.setup_caches(1, 16)
    with torch.no_grad():
        want = m(idx, pos)
    m.setup_caches(1, 16, kv_cache_dtype="fp8")
    with torch.no_grad():
        got = m(idx, pos)
    rel = float((got - want).norm() / want.norm())
    assert 0.0 < rel < 0.2, rel  # (three mantissa bits: close, and not the same)


def test_set_kv_scales_validation():
    m = _tiny()
    one = torch.ones(2, 2)
    with pytest.raises(ValueError, match="fp8"):
        m.set_kv_scales(one, one)  # no caches yet
    m.setup_caches(1, 8)
    with pytest.raises(ValueError, match="fp8"):
        m.set_kv_scales(one, one)  # an fp16 cache
    m.setup_caches(1, 8, kv_cache_dtype="fp8")
    gen = m._alloc_gen
    ptrs = [b.attention.kv_cache.k_scale.data_ptr() for b in m.layers]
    m.set_kv_scales(torch.tensor([[0.5, 0.37], [2.9, 1.0]]), torch.tensor([[1.0, 2.0], [3.0, 4.0]]))
    kc = m.layers[1].attention.kv_cache
    assert kc.k_scale.tolist() == pytest.approx([2.9, 1.0]) and kc.v_scale.tolist() == [3.0, 4.0]
    assert torch.equal(kc.k_inv, torch.reciprocal(kc.k_scale)) and torch.equal(kc.v_inv, torch.reciprocal(kc.v_scale))
    assert m._alloc_gen == gen and ptrs == [b.attention.kv_cache.k_scale.data_ptr() for b in m.layers]  # in place: no re-capture
    for bad in (torch.ones(2, 3), torch.ones(4), torch.tensor([[1.0, 0.0], [1.0, 1.0]]), torch.tensor([[1.0, -2.0], [1.0, 1.0]]),
                torch.tensor([[1.0, float("inf")], [1.0, 1.0]]), torch.tensor([[float("nan"), 1.0], [1.0, 1.0]])):
        with pytest.raises(ValueError, match="set_kv_scales"):
            m.set_kv_scales(bad, one)
        with pytest.raises(ValueError, match="set_kv_scales"):
            m.set_kv_scales(one, bad)
    assert kc.k_scale.tolist() == pytest.approx([2.9, 1.0])  # a refused call changed nothing


def test_slot_offsets_follow_the_element_size():
    from guidedquant_amd.native_step import kv_slot_bytes
    assert kv_slot_bytes(8, 4096, 128, 2) == 8 * 4096 * 128 * 2 and kv_slot_bytes(8, 4096, 128, 1) == 8 * 4096 * 128
    assert kv_slot_bytes(2, 40, 64, 1) * 2 == kv_slot_bytes(2, 40, 64, 2)
    # against the caches themselves: slot s of a [batch][n_kv_head][max_seq][head_dim] tensor begins at that many bytes
    m = _tiny()
    for kv, es in (("fp16", 4), ("fp8", 1)):  # (an fp32 model: the fp16-named default is the model's own dtype, 4 bytes)
        m.setup_caches(3, 16, kv_cache_dtype=kv)
        kc = m.layers[0].attention.kv_cache.k_cache
        assert kc.element_size() == es
        assert kc[2].data_ptr() - kc.data_ptr() == 2 * kv_slot_bytes(2, 16, 64, kc.element_size())


def test_routes_that_do_not_serve_the_format_say_so():
    from guidedquant_amd import model as gm
    from guidedquant_amd.generate import load_model
    from guidedquant_amd.pipeline import PipelinedDecoder
    from guidedquant_amd.tp import TensorParallelDecoder
    gm.transformer_configs["qtip-test"] = dict(model_name="llama-qtip-test", block_size=64, vocab_size=128, n_layer=1, n_head=4, dim=256, intermediate_size=512,
                                               n_local_heads=2)
    try:
        q = load_model("qtip-test", "cpu", "qtip", 2, random_init=True)
    finally:
        del gm.transformer_configs["qtip-test"]
    with pytest.raises(NotImplementedError, match="fp8 KV cache"):
        q.setup_caches(1, 8, kv_cache_dtype="fp8")
    assert q.kv_cache_dtype == "fp16" and not q.cache_initialized
    m = _tiny()
    m.setup_caches(1, 8, kv_cache_dtype="fp8")
    with pytest.raises(NotImplementedError, match="fp8 KV cache"):
        TensorParallelDecoder(m, None, 0, 2, 4)
    with pytest.raises(NotImplementedError, match="fp8 KV cache"):
        PipelinedDecoder(m, 0, 1, range(0, 2), n_seq=1, max_new_tokens=4)
    assert m.kv_cache_dtype == "fp8"  # (neither switched the caches back)
    assert "Any-Precision" in m.kv8_unserved()  # (nn.Linear layers: the module forward serves it, the fused route does not)
    assert "head_dim" in _tiny(head_dim=32).kv8_unserved()


def test_generate_with_fp8_on_a_cpu_model_raises():
    transformers = pytest.importorskip("transformers")
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    hf = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                  vocab_size=128, max_position_embeddings=64, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    hf.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(hf, device="cpu")
    ids = torch.tensor([[3, 17, 5]])
    with pytest.raises(ValueError, match="kv_cache_dtype='fp8': the fused routes need the GPU"):
        m.generate(ids, max_new_tokens=2, do_sample=False, kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        m.generate(ids, max_new_tokens=2, do_sample=False, kv_cache_dtype="fp4")
    out = m.generate(ids, max_new_tokens=2, do_sample=False, kv_cache_dtype="fp16")  # the default by name: popped, never reaches transformers
    assert out.shape == (1, 5)
