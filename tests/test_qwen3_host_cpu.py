"""CPU: the model description of Qwen3 checkpoints (explicit head_dim, per-head q / k RMSNorm) -- the Python forward against
transformers' own Qwen3ForCausalLM, the dispatch of `model_args_from_hf_config` on `model_type`, the geometry of the fused decoder
AnyPrecisionForCausalLM builds from a Qwen3 config, and the loud decline of every architecture the fused route does not serve."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
import torch.nn as nn  # noqa: E402

_NAMES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]


def _anyprec(cfg):
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    return cfg


def _hf_qwen3(hd, D=256, H=4, KV=2, I=512, V=320, Lr=2):
    cfg = transformers.Qwen3Config(hidden_size=D, intermediate_size=I, num_hidden_layers=Lr, num_attention_heads=H, num_key_value_heads=KV,
                                   head_dim=hd, vocab_size=V, max_position_embeddings=64, rms_norm_eps=1e-6, tie_word_embeddings=False,
                                   attention_bias=False)
    cfg._attn_implementation = "eager"
    torch.manual_seed(11 + hd)
    hf = transformers.Qwen3ForCausalLM(cfg).to(torch.float32).eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in hf.parameters():  # (more contrast than the default init: O(1) logits)
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / p.shape[1]**0.5))
        for n, p in hf.named_parameters():
            if n.endswith("norm.weight") or "layernorm" in n:  # q_norm / k_norm far from 1, like real checkpoints: a dropped or swapped weight shows
                p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
    return cfg, hf


@pytest.mark.parametrize("hd", [64, 128])
def test_python_forward_matches_transformers_qwen3(hd):
    """fp32 on both sides, the same dense weights: a 12-token prompt, then three single-token steps.  Bound 1e-4 * max|logit| (operation
    order only; dropping the norm moves logits by O(1)).  Measured maximum: 1.2e-6 * max|logit| (head_dim 64), 9.3e-7 (128)."""
    from guidedquant_amd.hf_loader import model_args_from_hf_config
    from guidedquant_amd.model import Transformer
    cfg, hf = _hf_qwen3(hd)
    args = model_args_from_hf_config(cfg.to_dict())
    assert args.head_dim == hd and args.qk_norm and args.norm_eps == 1e-6
    m = Transformer(torch.float32, args, linear_class=nn.Linear).eval()
    sd = hf.state_dict()
    with torch.no_grad():
        m.tok_embeddings.weight.copy_(sd["model.embed_tokens.weight"])
        m.output.weight.copy_(sd["lm_head.weight"])
        m.norm.weight.copy_(sd["model.norm.weight"])
        for i, b in enumerate(m.layers):
            p = f"model.layers.{i}."
            b.attention.wqkv.weight.copy_(torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], dim=0))
            b.attention.wo.weight.copy_(sd[p + "self_attn.o_proj.weight"])
            b.attention.q_norm.weight.copy_(sd[p + "self_attn.q_norm.weight"])
            b.attention.k_norm.weight.copy_(sd[p + "self_attn.k_norm.weight"])
            b.feed_forward.w1w3.weight.copy_(torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], dim=0))
            b.feed_forward.w2.weight.copy_(sd[p + "mlp.down_proj.weight"])
            b.input_layernorm.weight.copy_(sd[p + "input_layernorm.weight"])
            b.post_attention_layernorm.weight.copy_(sd[p + "post_attention_layernorm.weight"])
    assert m.layers[0].attention.wo.in_features == 4 * hd
    m.setup_caches(1, 16)
    ids = torch.tensor([[3, 17, 5, 60, 2, 9, 100, 311, 7, 7, 42, 1, 250, 19, 8]])
    with torch.no_grad():
        want = hf(ids).logits[0].float()  # [15, V]: causal, so row t is what a step at position t sees
        got = [m(ids[:, :12].to(torch.int32), torch.arange(12, dtype=torch.int32))[0]]
        for t in range(12, 15):
            got.append(m(ids[:, t:t + 1].to(torch.int32), torch.tensor([t], dtype=torch.int32))[0])
        got = torch.cat(got, dim=0).float()
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print("head_dim %d: max |logit| %.3f, max deviation %.3e (%.2e of it)" % (hd, scale, err, err / scale))
    assert scale > 0.5
    assert err <= 1e-4 * scale, (err, scale)
    # the norm matters at this scale: without it the logits move by O(1) of their magnitude
    for b in m.layers:
        b.attention.qk_norm = False
    with torch.no_grad():
        off = m(ids[:, :12].to(torch.int32), torch.arange(12, dtype=torch.int32))[0].float()
    assert (off - want[:12]).abs().max().item() > 1e-2 * scale


def test_model_args_dispatch_on_model_type():
    from guidedquant_amd.hf_loader import model_args_from_hf_config as f
    from guidedquant_amd.model import ModelArgs
    q = f(transformers.Qwen3Config(hidden_size=512, num_attention_heads=8, num_key_value_heads=2, head_dim=128, num_hidden_layers=2,
                                   intermediate_size=1024, vocab_size=512, rms_norm_eps=1e-6).to_dict())
    assert (q.head_dim, q.qk_norm, q.n_head, q.n_local_heads, q.dim, q.norm_eps) == (128, True, 8, 2, 512, 1e-6)
    # a Qwen3 config.json as transformers 4 writes it: base frequency at the top level
    q4 = f(dict(model_type="qwen3", hidden_size=4096, num_attention_heads=32, num_key_value_heads=8, head_dim=128, num_hidden_layers=36, intermediate_size=12288,
                vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=40960, use_sliding_window=False, sliding_window=None))
    assert (q4.head_dim, q4.qk_norm, q4.rope_base, q4.block_size) == (128, True, 1000000.0, 40960)
    # Llama dicts (no model_type, or "llama") resolve exactly as before: head_dim derived, no qk_norm, the same name rule
    d = dict(vocab_size=1000, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2, hidden_size=512, intermediate_size=1024,
             rope_theta=500000.0, rms_norm_eps=1e-5, max_position_embeddings=4096, _name_or_path="/ckpt/Llama-3-tiny-w2")
    want = ModelArgs(block_size=4096, vocab_size=1000, n_layer=3, n_head=8, dim=512, intermediate_size=1024, n_local_heads=2, rope_base=500000.0,
                     norm_eps=1e-5, rope_scaling=None, model_name="Llama-3-tiny-w2")
    assert f(d) == want and f(dict(d, model_type="llama")) == want and want.head_dim == 64 and not want.qk_norm
    assert f(dict(d, _name_or_path="/ckpt/w2-run7")).model_name == "llama-w2-run7"
    sc = dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192)
    assert f(dict(d, rope_scaling=sc)).rope_scaling == sc
    # Mistral: the Llama block with its own head_dim; only when no sliding window bites
    mi = f(transformers.MistralConfig(hidden_size=512, num_attention_heads=8, num_key_value_heads=2, head_dim=128, num_hidden_layers=2, intermediate_size=1024,
                                      vocab_size=512, sliding_window=None).to_dict())
    assert (mi.head_dim, mi.qk_norm) == (128, False)
    assert f(transformers.MistralConfig(sliding_window=4096, max_position_embeddings=4096).to_dict()).head_dim == 128
    declined = [
        transformers.Gemma3TextConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64, num_hidden_layers=2, intermediate_size=512, vocab_size=512),
        transformers.PhiConfig(hidden_size=256, num_attention_heads=4, num_hidden_layers=2, intermediate_size=512, vocab_size=512),
        transformers.MistralConfig(sliding_window=1024, max_position_embeddings=4096),
        transformers.Qwen3Config(num_hidden_layers=2, layer_types=["full_attention", "sliding_attention"], use_sliding_window=True, sliding_window=128, max_window_layers=1),
    ]
    for c in declined:
        with pytest.raises(NotImplementedError, match=c.model_type.split("_")[0]):
            f(c.to_dict())
    for mt in ("opt", "qwen2", "qwen3_moe", "phi3"):
        with pytest.raises(NotImplementedError, match=mt):
            f(dict(d, model_type=mt))


def test_model_args_keep_an_explicit_head_dim():
    from guidedquant_amd.model import ModelArgs
    assert ModelArgs(dim=512, n_head=8).head_dim == 64 and not ModelArgs(dim=512, n_head=8).qk_norm
    a = ModelArgs(dim=512, n_head=8, n_local_heads=2, head_dim=128, qk_norm=True)
    assert a.head_dim == 128 and a.qk_norm
    assert ModelArgs.from_name("Qwen/Qwen3-8B").head_dim == 128 and ModelArgs.from_name("Qwen/Qwen3-8B").qk_norm
    assert ModelArgs.from_name("meta-llama/Meta-Llama-3.1-8B").head_dim == 128 and not ModelArgs.from_name("meta-llama/Meta-Llama-3.1-8B").qk_norm


def test_fused_decoder_of_a_qwen3_checkpoint_has_its_geometry():
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg = _anyprec(transformers.Qwen3Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                                            head_dim=128, vocab_size=512, max_position_embeddings=256, tie_word_embeddings=False))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device="cpu")
    dec = m.native_decoder(2)
    assert dec.config.head_dim == 128 and dec.config.qk_norm
    l0, at = m.get_model_layers()[0], dec.layers[0].attention
    assert at.wqkv.out_features == at.wqkv.qweight.shape[1] == 1536 and at.wqkv.in_features == 512
    assert at.wo.in_features == 1024 and at.wo.qweight.shape == (2, 512, 32)
    assert at.q_norm.weight.shape == (128, ) and at.q_norm.eps == cfg.rms_norm_eps
    assert at.q_norm.weight.data_ptr() == l0.self_attn.q_norm.weight.data_ptr()
    assert at.k_norm.weight.data_ptr() == l0.self_attn.k_norm.weight.data_ptr()
    assert dec.layers[0].attention.wo.qweight.data_ptr() == l0.self_attn.o_proj.qweight.data_ptr()
    sd = dec.state_dict()
    assert "layers.1.attention.q_norm.weight" in sd and "layers.1.attention.k_norm.weight" in sd
    dec.load_state_dict(sd, strict=True)
    dec.setup_caches(1, 16)
    assert dec.layers[0].attention.kv_cache.k_cache.shape == (1, 2, 16, 128) and dec.rope_cos.shape == (16, 128)
    # the converter carries the per-head norms through under the decoder's keys
    from guidedquant_amd.convert import convert_anyprec_fuse
    fused = convert_anyprec_fuse({k: v for k, v in m.model.state_dict().items() if "rotary_emb" not in k}, 2, n_layer=2)
    assert set(fused) == set(sd) and all(fused[k].shape == sd[k].shape for k in sd)
    # the module tree gets its planes back from a decoder with head_dim != dim / n_head (native=True's release, undone)
    m._drop_native()
    dec = m.native_decoder(2, release_planes=True)
    assert l0.self_attn.q_proj.qweight.numel() == 0 and m._released is not None
    m._restore_module_tree()
    assert l0.self_attn.q_proj.qweight.shape == (2, 1024, 16) and l0.self_attn.k_proj.qweight.shape == (2, 256, 16) and l0.mlp.up_proj.qweight.shape == (2, 1024, 16)


def test_architectures_without_a_fused_form_are_declined_loudly():
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg = _anyprec(transformers.Gemma3TextConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                                 head_dim=64, vocab_size=512, max_position_embeddings=256))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device="cpu")
    with pytest.raises(NotImplementedError, match="gemma3"):
        m.native_decoder(2)
    assert m._native_decoder_or_none(2) is None and "gemma3" in m._no_native_reason
    ids = torch.tensor([[3, 17, 5]])
    with pytest.raises(ValueError, match="native=True"):
        m.generate(ids, max_new_tokens=2, do_sample=False, native=True)
    out = m.generate(ids, max_new_tokens=3, do_sample=False)  # the plain call falls through to transformers
    assert out.shape == (1, 6) and ("decoder", 2) not in m._native_cache


def test_tensor_parallel_decoder_declines_qk_norm():
    from guidedquant_amd.model import ModelArgs, Transformer
    from guidedquant_amd.tp import TensorParallelDecoder
    with torch.device("meta"):
        m = Transformer(torch.float16, ModelArgs(dim=256, n_head=4, n_local_heads=2, head_dim=64, qk_norm=True, n_layer=1, vocab_size=64,
                                                 intermediate_size=512, model_name="qwen3-tiny"))
    with pytest.raises(NotImplementedError, match="QK-norm"):
        TensorParallelDecoder(m, None, 0, 2, 8)
