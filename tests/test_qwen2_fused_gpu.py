"""GPU, model level: an Any-Precision Qwen2 / Qwen2.5 checkpoint (a bias on q_proj / k_proj / v_proj) on the fused HIP route -- the plain
`generate()` lands there and agrees with transformers' own Qwen2 module tree; the decode step at the Qwen2.5-7B widths agrees with the
module forward on every GEMV route; a captured DecodeGraph replays what the eager step computes; and what the fused route does not
serve (a bias on o_proj, tensor-parallel decode of a biased model, sliding-window layers) is declined, not decoded wrongly.
The sibling of tests/test_qwen3_fused_gpu.py, with its bounds."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

TOL = 2e-2  # of max|logit|: tests/test_decode_default_gpu.py:16
_NAMES = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]


def _mode(m):
    from guidedquant_amd import _lib
    _lib.check(_lib.lib().gq_set_ap_mode(m), "gq_set_ap_mode")


@pytest.fixture(autouse=True)
def _restore():
    yield
    _mode(-1)


def _hf_model(cfg, seed=5):
    """`test_qwen3_fused_gpu._hf_model` for Qwen2: 2-bit planes only, embeddings / lm_head scaled for margins, and the q / k / v biases
    overwritten with seeded values of std 1 (from_config_random draws every other tensor at std 0.02: a bias that small would not show)"""
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=torch.device("cuda:0"), seed=seed)
    g = torch.Generator(device=m.device)
    g.manual_seed(seed + 1)
    with torch.no_grad():
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
        for layer in m.get_model_layers():
            for n in ("q_proj", "k_proj", "v_proj"):
                b = getattr(layer.self_attn, n).bias
                assert b is not None and b.dtype == torch.float16
                b.copy_(torch.randn(b.shape, device=m.device, generator=g).half())
            assert layer.self_attn.o_proj.bias is None
    return m


def _tiny_qwen2(hd, seed=5):
    """hidden 512 as 8 / 2 heads of 64 or 4 / 2 heads of 128 (Qwen2Config has no head_dim of its own: hidden_size / num_attention_heads)"""
    heads = 512 // hd
    return _hf_model(transformers.Qwen2Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=heads, num_key_value_heads=2,
                                              vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-6, tie_word_embeddings=False), seed)


@pytest.mark.parametrize("hd", [64, 128])
def test_plain_generate_of_a_qwen2_checkpoint_takes_the_fused_route(hd):
    m = _tiny_qwen2(hd)
    d = m.device
    assert type(m.get_model_layers()[0]).__name__ == "Qwen2DecoderLayer"
    ids = torch.tensor([[3, 17, 5, 60, 2, 9]], device=d)
    eager = m.generate(ids, max_new_tokens=24, do_sample=False, native=False, pad_token_id=0)
    fused = m.generate(ids, max_new_tokens=24, do_sample=False, pad_token_id=0)
    assert ("decoder", 2) in m._native_cache and fused.shape == eager.shape == (1, 30) and fused.dtype == ids.dtype
    dec = m._native_cache[("decoder", 2)]
    assert dec.config.attn_bias and dec.config.head_dim == hd and dec.native_ready()
    at0, hf0 = dec.layers[0].attention, m.get_model_layers()[0].self_attn
    assert torch.equal(at0.wqkv.bias, torch.cat([hf0.q_proj.bias, hf0.k_proj.bias, hf0.v_proj.bias])) and at0.wo.bias is None
    agree = float((fused[0, 6:] == eager[0, 6:]).float().mean())
    print("head_dim %d: agreement %.3f" % (hd, agree))
    assert torch.equal(fused[0, :7], eager[0, :7]) and agree >= 0.8, (agree, fused, eager)  # the Llama criterion, test_hf_routes_gpu.py:114-115
    # logits of the last prompt position: the HIP prompt pass and a decode step behind it, against transformers' module tree
    with torch.no_grad():
        want = m.model(ids).logits[0, -1].float()
        ids32 = ids.view(-1).to(torch.int32)
        T = ids32.numel()
        assert dec.prefill_ready(ids32)
        got_p = dec.prefill_native(ids32, torch.arange(T, device=d, dtype=torch.int32), start=0).float().view(-1).clone()
        dec.prefill_native(ids32[:T - 1], torch.arange(T - 1, device=d, dtype=torch.int32), start=0)
        got_d = dec.decode_native(ids32[T - 1:], torch.tensor([T - 1], device=d, dtype=torch.int32)).float().view(-1).clone()
    torch.cuda.synchronize()
    scale = want.abs().max().item()
    for name, got in (("prefill_native", got_p), ("decode_native", got_d)):
        err, rel = (got - want).abs().max().item(), ((got - want).norm() / want.norm()).item()
        print("head_dim %d %s: max|logit| %.3f  element-wise %.3e  norm-wise %.3e" % (hd, name, scale, err, rel))
        assert torch.isfinite(got).all()
        assert err <= TOL * scale, (name, err, scale)
        assert rel <= 5e-3, (name, rel)
    # and the bias is in it: the decoder holds the original biases (a tensor of its own); with every q / k / v bias of the module tree
    # negated, the module tree's logits leave the fused ones by more than twice what the right biases are allowed
    with torch.no_grad():
        for layer in m.get_model_layers():
            for n in ("q_proj", "k_proj", "v_proj"):
                getattr(layer.self_attn, n).bias.neg_()
        negated = m.model(ids).logits[0, -1].float()
    for name, got in (("prefill_native", got_p), ("decode_native", got_d)):
        moved = ((got - negated).norm() / negated.norm()).item()
        print("head_dim %d %s: against the negated biases norm-wise %.3e" % (hd, name, moved))
        assert moved > 2 * 5e-3, (name, moved)


def _wide_model(bits, n_layer=2, seed=0):
    """the Qwen2.5-7B widths (hidden 3584, MLP 18944, 28 / 4 heads of 128, vocab 152064), like test_qwen3_fused_gpu._wide_model;
    random_init_ draws the wqkv bias (std 1, a few k entries 30 times that)"""
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    d = torch.device("cuda:0")
    cfg = ModelArgs(block_size=8192, vocab_size=152064, n_layer=n_layer, n_head=28, dim=3584, intermediate_size=18944, n_local_heads=4, head_dim=128,
                    rope_base=1000000, norm_eps=1e-6, attn_bias=True, model_name="Qwen2.5-7B-2layers")
    m = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=bits, device=d))
    m = m.to(device=d, dtype=torch.float16)
    random_init_(m, seed=seed + bits)
    g = torch.Generator(device=d)
    g.manual_seed(1)
    for b in m.layers:
        b.input_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
        b.post_attention_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
        bias = b.attention.wqkv.bias.float()
        assert b.attention.wo.bias is None and 0.5 < bias.std().item() and 8.0 < bias[3584:3584 + 512].abs().max().item() < 200.0
    m.norm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
    m.tok_embeddings.weight.data.mul_(25.0)
    m.output.weight.data.mul_(4.0)
    return m.eval()


@pytest.mark.parametrize("bits", [2, 3, 4, 5])
def test_decode_at_qwen25_7b_widths_matches_the_module_forward(bits, monkeypatch):
    """`test_decode_at_qwen3_8b_widths_matches_the_module_forward` for the biased layer: ten positions, the module forward in exact mode as
    the yardstick (APLinear adds the bias there; anchored to transformers by the test above), the same bounds and the same token list;
    every AP-GEMV launch of the step on the route a dry dispatch names.  K = 3584 and 18944 are no multiples of 1024 and 18944 sits
    beside the 16384 K-split threshold: whichever family serves them holds the bound."""
    from guidedquant_amd import _lib
    d = torch.device("cuda:0")
    m = _wide_model(bits)
    m.setup_caches(1, 32)
    assert m.native_ready()
    L = _lib.lib()
    routes = []
    real = L.gq_anyprec_gemv_fused_ho

    def recording(*a):
        rc = real(*a)
        routes.append((int(a[4]), int(a[5])) + _lib.ap_last_route() + (int(a[12] or 0), ))
        return rc

    toks = [128000, 17, 90000, 3, 3, 512, 44, 1023, 127999, 5]  # (the token list of the Llama test)
    ref = []
    with torch.no_grad():
        _mode(1)
        for p, t in enumerate(toks):
            lg = m(torch.tensor([[t]], dtype=torch.int32, device=d), torch.tensor([p], dtype=torch.int32, device=d))
            ref.append(lg.float().view(-1).clone())
        ref_k = [b.attention.kv_cache.k_cache.clone() for b in m.layers]
        ref_v = [b.attention.kv_cache.v_cache.clone() for b in m.layers]
        for b in m.layers:
            b.attention.kv_cache.k_cache.zero_()
            b.attention.kv_cache.v_cache.zero_()
        _mode(0)
        monkeypatch.setattr(L, "gq_anyprec_gemv_fused_ho", recording)
        for name in ("gq_anyprec_gemv_qkv_rope", "gq_anyprec_gemv_qkv_rope_ho", "gq_anyprec_gemv_qkv_rope_attn", "gq_anyprec_gemv_fused"):
            monkeypatch.setattr(L, name, lambda *a, _n=name: pytest.fail("a biased layer launched " + _n))
        for p, t in enumerate(toks):
            lg = m.decode_native(torch.tensor([t], dtype=torch.int32, device=d), torch.tensor([p], dtype=torch.int32, device=d))
            torch.cuda.synchronize()
            a, r = lg.float().view(-1), ref[p]
            assert torch.isfinite(a).all()
            scale, err = r.abs().max().item(), (a - r).abs().max().item()
            rel = ((a - r).norm() / r.norm()).item()
            print("bits %d pos %d: element-wise %.3e of %.3f  norm-wise %.3e" % (bits, p, err, scale, rel))
            assert err <= TOL * scale, (p, err, scale)
            assert rel <= (5e-3 if bits == 2 else 7.5e-3), (p, bits, rel)  # (tests/test_decode_default_gpu.py:87)
        monkeypatch.undo()
    n = len(toks)
    for i, b in enumerate(m.layers):
        dk = (b.attention.kv_cache.k_cache[:, :, :n].float() - ref_k[i][:, :, :n].float()).abs().max().item()
        dv = (b.attention.kv_cache.v_cache[:, :, :n].float() - ref_v[i][:, :, :n].float()).abs().max().item()
        assert dk <= TOL * ref_k[i][:, :, :n].float().abs().max().item(), (i, dk)
        assert dv <= TOL * ref_v[i][:, :, :n].float().abs().max().item(), (i, dv)
    # the launches of one step, in order: (wqkv, wo, w1w3, w2) per layer -- the real route equals the dry one, and the wqkv launch never
    # takes the RoPE-epilogue kernel (it would rotate the unbiased q / k)
    from dispatch_table import EPI_RESIDUAL, EPI_SILU_PAIRS
    assert len(routes) == n * 2 * 4
    forms = (("wqkv", 4608, 3584, True, 0), ("wo", 3584, 3584, False, EPI_RESIDUAL), ("w1w3", 37888, 3584, True, EPI_SILU_PAIRS),
             ("w2", 3584, 18944, False, EPI_RESIDUAL))
    seen = set()
    for i, (N, K, fam, launches, variant, ws_bytes) in enumerate(routes):
        name, wN, wK, norm, epi = forms[i % 4]
        assert (N, K) == (wN, wK), (i, N, K)
        assert fam not in ("none", "stream-qkv-rope"), (name, fam)
        assert (fam, launches, variant) == _lib.ap_plan_route(N, K, bits, 1, norm, epi, ws_bytes), (name, fam)
        if bits == 5:
            assert fam == "wide", (name, fam)
        seen.add((name, fam, launches))
    print("bits %d routes: %s" % (bits, sorted(seen)))


def test_decode_graph_replay_equals_the_eager_step_on_a_biased_model():
    from guidedquant_amd.generate import DecodeGraph
    m = _tiny_qwen2(128, seed=7)
    d = m.device
    dec = m.native_decoder(2)
    dec.setup_caches(1, 64)
    assert dec.native_ready() and dec.config.attn_bias
    n = 16
    eager, t = [], 3
    with torch.no_grad():
        for p in range(n):
            lg = dec.decode_native(torch.tensor([t], dtype=torch.int32, device=d), torch.tensor([p], dtype=torch.int32, device=d))
            t = int(lg.float().view(-1).argmax().item())
            eager.append(t)
    for b in dec.layers:
        b.attention.kv_cache.k_cache.zero_()
        b.attention.kv_cache.v_cache.zero_()
    g = DecodeGraph(dec, d, native_sampling=True, temperature=0.0, top_k=32, seq_capacity=65, steps_per_replay=1)
    g.set_token(3, 0)
    for _ in range(n):
        g.step()
    torch.cuda.synchronize()
    assert g.seq[1:n + 1].tolist() == eager and int(g.pos.item()) == n
    assert len(set(eager)) > 4  # not a fixed point
    g.close() if hasattr(g, "close") else None


def test_what_the_biased_route_does_not_serve_is_declined():
    from guidedquant_amd.hf_loader import model_args_from_hf_config
    from guidedquant_amd.tp import TensorParallelDecoder
    m = _tiny_qwen2(64)
    ids = torch.tensor([[3, 17, 5, 60, 2, 9]], device=m.device)
    # tensor-parallel decode of a biased model
    with pytest.raises(NotImplementedError, match="bias"):
        TensorParallelDecoder(m.native_decoder(2), None, 0, 2, 8)
    # a Qwen2 tree with a bias on o_proj: no fused form, `native=True` says so, the plain call goes to transformers
    m._drop_native()
    o = m.get_model_layers()[1].self_attn.o_proj
    o.bias = torch.zeros(o.out_features, dtype=torch.float16, device=m.device)
    with pytest.raises(ValueError, match="native=True"):
        m.generate(ids, max_new_tokens=4, do_sample=False, native=True, pad_token_id=0)
    assert "biased linears" in m._no_native_reason
    plain = m.generate(ids, max_new_tokens=4, do_sample=False, pad_token_id=0)
    assert plain.shape == (1, 10) and not any(k[0] == "decoder" for k in m._native_cache)
    # a qwen2 config with sliding-window layers
    cfg = transformers.Qwen2Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2,
                                   vocab_size=512, use_sliding_window=True, sliding_window=128, max_window_layers=1).to_dict()
    with pytest.raises(NotImplementedError, match="qwen2"):
        model_args_from_hf_config(cfg)
