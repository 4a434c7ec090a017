"""CPU: the model description of Qwen2 / Qwen2.5 checkpoints (a bias on q_proj / k_proj / v_proj) -- `model_args_from_hf_config` on a
Qwen2 config, the converter's fused `wqkv.bias`, the geometry of the fused decoder AnyPrecisionForCausalLM builds from a Qwen2 config,
the Python forward against transformers' own Qwen2ForCausalLM, and what stays declined."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
import torch.nn as nn  # noqa: E402

_NAMES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]

# a Qwen2.5-7B config.json as transformers 4 writes it (the fields the loader reads)
QWEN25_7B = dict(model_type="qwen2", hidden_size=3584, num_attention_heads=28, num_key_value_heads=4, num_hidden_layers=28, intermediate_size=18944,
                 vocab_size=152064, rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=32768, use_sliding_window=False, sliding_window=131072,
                 max_window_layers=28, tie_word_embeddings=False, _name_or_path="/ckpt/Qwen2.5-7B-w2")


def test_model_args_of_a_qwen2_config():
    from guidedquant_amd.hf_loader import model_args_from_hf_config as f
    from guidedquant_amd.model import ModelArgs
    a = f(QWEN25_7B)
    assert a == ModelArgs(block_size=32768, vocab_size=152064, n_layer=28, n_head=28, dim=3584, intermediate_size=18944, n_local_heads=4, head_dim=128,
                          rope_base=1000000.0, norm_eps=1e-6, rope_scaling=None, model_name="Qwen2.5-7B-w2", attn_bias=True)
    assert a.attn_bias and not a.qk_norm and a.head_dim == 3584 // 28  # (no head_dim in the config: hidden_size / num_attention_heads)
    # the table entry is the same geometry
    t = ModelArgs.from_name("Qwen/Qwen2.5-7B")
    assert (t.dim, t.n_layer, t.n_head, t.n_local_heads, t.head_dim, t.intermediate_size, t.vocab_size, t.rope_base, t.norm_eps, t.attn_bias, t.qk_norm) == \
        (3584, 28, 28, 4, 128, 18944, 152064, 1000000, 1e-6, True, False)
    # a head_dim of the config's own wins; a directory name without the model type gets it in front
    assert f(dict(QWEN25_7B, head_dim=64)).head_dim == 64
    assert f(dict(QWEN25_7B, _name_or_path="/ckpt/run7")).model_name == "qwen2-run7"
    # a config object of the installed transformers (base frequency under rope_parameters or at the top level, by version)
    q = f(transformers.Qwen2Config(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=1024, vocab_size=512,
                                   rms_norm_eps=1e-6).to_dict())
    assert (q.head_dim, q.attn_bias, q.qk_norm, q.n_head, q.n_local_heads, q.dim, q.norm_eps, q.rope_base) == (128, True, False, 4, 2, 512, 1e-6, 10000.0)
    rp = f({k: v for k, v in dict(QWEN25_7B, rope_parameters=dict(rope_theta=500000.0, rope_type="default")).items() if k != "rope_theta"})
    assert rp.rope_base == 500000.0 and rp.rope_scaling is None
    # other model types keep their meaning: no bias flag on Llama / Qwen3, and Qwen3 with attention_bias stays declined
    d = dict(vocab_size=1000, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2, hidden_size=512, intermediate_size=1024)
    assert not f(d).attn_bias and not f(dict(d, model_type="qwen3", head_dim=64)).attn_bias
    with pytest.raises(NotImplementedError, match="attention_bias"):
        f(dict(d, model_type="qwen3", head_dim=64, attention_bias=True))
    for mt in ("qwen2_moe", "qwen2_vl", "opt"):
        with pytest.raises(NotImplementedError, match=mt):
            f(dict(d, model_type=mt))


def test_qwen2_with_a_sliding_window_is_declined():
    from guidedquant_amd.hf_loader import model_args_from_hf_config as f
    with pytest.raises(NotImplementedError, match="qwen2: use_sliding_window"):
        f(dict(QWEN25_7B, use_sliding_window=True))
    with pytest.raises(NotImplementedError, match="qwen2: layer_types"):
        f(dict(QWEN25_7B, layer_types=["full_attention"] * 27 + ["sliding_attention"]))
    c = transformers.Qwen2Config(num_hidden_layers=3, use_sliding_window=True, sliding_window=128, max_window_layers=1)
    with pytest.raises(NotImplementedError, match="qwen2"):
        f(c.to_dict())
    assert f(dict(QWEN25_7B, layer_types=["full_attention"] * 28)).attn_bias
    # a dict that names the model type but states neither field is not a Qwen2 config.json: declined, not taken for a dense model
    bare = {k: v for k, v in QWEN25_7B.items() if k != "use_sliding_window"}
    with pytest.raises(NotImplementedError, match="qwen2: the config states neither"):
        f(bare)
    assert f(dict(bare, layer_types=["full_attention"] * 28)).attn_bias


def _hf_keyed(n_layer=2, D=64, H=2, KV=1, hd=32, inter=96, bias=True, seed=0):
    """an HF-keyed Any-Precision state dict (2 planes, lut2 / lut3)"""
    g = torch.Generator().manual_seed(seed)
    sd = {"model.embed_tokens.weight": torch.randn(50, D, generator=g).to(torch.bfloat16), "lm_head.weight": torch.randn(50, D, generator=g).half(),
          "model.norm.weight": torch.ones(D).half()}
    widths = dict(q=(H * hd, D), k=(KV * hd, D), v=(KV * hd, D), o=(D, H * hd), gate=(inter, D), up=(inter, D), down=(D, inter))
    for i in range(n_layer):
        p = f"model.layers.{i}."
        sd[p + "input_layernorm.weight"] = torch.ones(D).half()
        sd[p + "post_attention_layernorm.weight"] = torch.ones(D).half()
        for n, (N, K) in widths.items():
            q = p + ("self_attn." if n in "qkvo" else "mlp.") + n + "_proj."
            sd[q + "qweight"] = torch.randint(-2**31, 2**31 - 1, (3, N, K // 32), dtype=torch.int32, generator=g)
            sd[q + "lut2"] = torch.randn(N, 4, generator=g).float()
            sd[q + "lut3"] = torch.randn(N, 8, generator=g).float()
            if bias and n in "qkv":
                sd[q + "bias"] = torch.randn(N, generator=g).to(torch.bfloat16)
    return sd


def test_converter_fuses_the_biases_in_q_k_v_order():
    from guidedquant_amd.convert import convert_anyprec_fuse
    sd = _hf_keyed()
    out = convert_anyprec_fuse(sd, 2)
    for i in range(2):
        b = out[f"layers.{i}.attention.wqkv.bias"]
        want = torch.cat([sd[f"model.layers.{i}.self_attn.{n}_proj.bias"].half() for n in "qkv"])
        assert b.dtype == torch.float16 and b.shape == (128, ) and b.is_contiguous() and torch.equal(b, want)
        assert out[f"layers.{i}.attention.wqkv.qweight"].shape == (2, 128, 2)
    assert not any("_proj" in k for k in out)
    # a bias-free dict converts to exactly what it converted to before: the same keys in the same order, the same tensors
    plain = {k: v for k, v in sd.items() if not k.endswith(".bias")}
    free = convert_anyprec_fuse(plain, 2)
    assert list(free) == [k for k in out if not k.endswith(".bias")] and not any(k.endswith(".bias") for k in free)
    assert all(torch.equal(free[k], out[k]) and free[k].dtype == out[k].dtype for k in free)
    # biases where no served block layout has one, or on some of q / k / v only
    for name in ("self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"):
        with pytest.raises(ValueError, match="bias"):
            convert_anyprec_fuse(dict(sd, **{f"model.layers.1.{name}.bias": torch.zeros(64).half()}), 2)
    with pytest.raises(ValueError, match="bias"):
        convert_anyprec_fuse({k: v for k, v in sd.items() if k != "model.layers.0.self_attn.k_proj.bias"}, 2)


def test_converted_qwen2_state_dict_loads_into_the_fused_model():
    from guidedquant_amd.hf_loader import anyprec_state_dict_to_transformer
    sd = _hf_keyed()
    cfg = dict(model_type="qwen2", hidden_size=64, num_attention_heads=2, num_key_value_heads=1, num_hidden_layers=2, intermediate_size=96, vocab_size=50,
               rms_norm_eps=1e-6, max_position_embeddings=64, use_sliding_window=False)
    m = anyprec_state_dict_to_transformer(sd, cfg, 2, device="cpu")
    at = m.layers[1].attention
    assert m.config.attn_bias and at.wo.bias is None and m.layers[1].feed_forward.w2.bias is None and m.layers[1].feed_forward.w1w3.bias is None
    assert torch.equal(at.wqkv.bias, torch.cat([sd[f"model.layers.1.self_attn.{n}_proj.bias"].half() for n in "qkv"]))


def _anyprec(cfg):
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    return cfg


def test_fused_decoder_of_a_qwen2_checkpoint_carries_the_bias():
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    from guidedquant_amd.convert import convert_anyprec_fuse
    cfg = _anyprec(transformers.Qwen2Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                                            vocab_size=512, max_position_embeddings=256, tie_word_embeddings=False))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device="cpu")
    l0 = m.get_model_layers()[0]
    assert l0.self_attn.q_proj.bias is not None and l0.self_attn.o_proj.bias is None
    dec = m.native_decoder(2)
    at = dec.layers[0].attention
    assert dec.config.attn_bias and dec.config.head_dim == 64 and at.wqkv.out_features == 768
    want = torch.cat([l0.self_attn.q_proj.bias, l0.self_attn.k_proj.bias, l0.self_attn.v_proj.bias])
    assert at.wqkv.bias.dtype == torch.float16 and torch.equal(at.wqkv.bias, want) and at.wqkv.bias.data_ptr() != l0.self_attn.q_proj.bias.data_ptr()
    assert at.wo.bias is None and dec.layers[0].feed_forward.w1w3.bias is None and dec.layers[0].feed_forward.w2.bias is None
    sd = dec.state_dict()
    assert "layers.1.attention.wqkv.bias" in sd and "layers.1.attention.wo.bias" not in sd
    dec.load_state_dict(sd, strict=True)
    fused = convert_anyprec_fuse({k: v for k, v in m.model.state_dict().items() if "rotary_emb" not in k}, 2, n_layer=2)
    assert set(fused) == set(sd) and all(fused[k].shape == sd[k].shape for k in sd)
    assert torch.equal(fused["layers.0.attention.wqkv.bias"], want)
    # the release of the planes and their restoration leave the module tree's biases alone
    m._drop_native()
    m.native_decoder(2, release_planes=True)
    assert l0.self_attn.q_proj.qweight.numel() == 0 and l0.self_attn.q_proj.bias.shape == (512, )
    m._restore_module_tree()
    assert l0.self_attn.q_proj.qweight.shape == (2, 512, 16) and torch.equal(torch.cat([l0.self_attn.q_proj.bias, l0.self_attn.k_proj.bias, l0.self_attn.v_proj.bias]), want)
    # a bias anywhere else has no fused form
    m._drop_native()
    o = m.get_model_layers()[1].self_attn.o_proj
    o.bias = torch.zeros(o.out_features, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="biased linears"):
        m.native_decoder(2)
    assert m._native_decoder_or_none(2) is None and "biased linears" in m._no_native_reason


def _hf_qwen2(hd, D=256, KV=2, inter=512, V=320, Lr=2):
    cfg = transformers.Qwen2Config(hidden_size=D, intermediate_size=inter, num_hidden_layers=Lr, num_attention_heads=D // hd, num_key_value_heads=KV,
                                   vocab_size=V, max_position_embeddings=64, rms_norm_eps=1e-6, tie_word_embeddings=False)
    cfg._attn_implementation = "eager"
    torch.manual_seed(11 + hd)
    hf = transformers.Qwen2ForCausalLM(cfg).to(torch.float32).eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in hf.parameters():  # (more contrast than the default init: O(1) logits)
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / p.shape[1]**0.5))
        for n, p in hf.named_parameters():
            if n.endswith("norm.weight") or "layernorm" in n:
                p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
            if n.endswith("proj.bias"):  # (the default init leaves them zero: a dropped or mis-ordered bias would not show)
                p.copy_(torch.randn(p.shape, generator=g))
    return cfg, hf


@pytest.mark.parametrize("hd", [64, 128])
def test_python_forward_matches_transformers_qwen2(hd):
    """fp32 on both sides, the same dense weights and biases: a 12-token prompt, then three single-token steps.  The bound is the one
    tests/test_qwen3_host_cpu.py sets, 1e-4 * max|logit| (operation order only; a dropped bias moves logits by O(1e-2) of their
    magnitude and more).  Measured maximum: 1.2e-6 * max|logit| (head_dim 64), 4.3e-6 (128)."""
    from guidedquant_amd.hf_loader import model_args_from_hf_config
    from guidedquant_amd.model import Transformer
    cfg, hf = _hf_qwen2(hd)
    args = model_args_from_hf_config(cfg.to_dict())
    assert args.head_dim == hd and args.attn_bias and not args.qk_norm and args.norm_eps == 1e-6
    m = Transformer(torch.float32, args, linear_class=nn.Linear).eval()
    sd = hf.state_dict()
    assert not any(k.endswith(("o_proj.bias", "gate_proj.bias", "up_proj.bias", "down_proj.bias")) for k in sd)
    with torch.no_grad():
        m.tok_embeddings.weight.copy_(sd["model.embed_tokens.weight"])
        m.output.weight.copy_(sd["lm_head.weight"])
        m.norm.weight.copy_(sd["model.norm.weight"])
        for i, b in enumerate(m.layers):
            p = f"model.layers.{i}."
            b.attention.wqkv.weight.copy_(torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], dim=0))
            b.attention.wqkv.bias.copy_(torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], dim=0))
            b.attention.wo.weight.copy_(sd[p + "self_attn.o_proj.weight"])
            b.feed_forward.w1w3.weight.copy_(torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], dim=0))
            b.feed_forward.w2.weight.copy_(sd[p + "mlp.down_proj.weight"])
            b.input_layernorm.weight.copy_(sd[p + "input_layernorm.weight"])
            b.post_attention_layernorm.weight.copy_(sd[p + "post_attention_layernorm.weight"])
            assert b.attention.wo.bias is None and b.feed_forward.w1w3.bias is None and b.feed_forward.w2.bias is None
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
    # the bias matters at this scale: with k's and v's exchanged (the same widths) the logits move by far more than the bound
    with torch.no_grad():
        for b in m.layers:
            q, k, v = b.attention.wqkv.bias.split([args.n_head * hd, args.n_local_heads * hd, args.n_local_heads * hd])
            b.attention.wqkv.bias.copy_(torch.cat([q, v, k]))
        off = m(ids[:, :12].to(torch.int32), torch.arange(12, dtype=torch.int32))[0].float()
    assert (off - want[:12]).abs().max().item() > 1e-2 * scale


def test_tensor_parallel_decoder_declines_a_biased_model():
    from guidedquant_amd.model import ModelArgs, Transformer
    from guidedquant_amd.tp import TensorParallelDecoder
    with torch.device("meta"):
        m = Transformer(torch.float16, ModelArgs(dim=256, n_head=4, n_local_heads=2, attn_bias=True, n_layer=1, vocab_size=64, intermediate_size=512,
                                                 model_name="qwen2-tiny"))
    assert m.layers[0].attention.wqkv.bias is not None and m.layers[0].attention.wo.bias is None
    with pytest.raises(NotImplementedError, match="bias"):
        TensorParallelDecoder(m, None, 0, 2, 8)
