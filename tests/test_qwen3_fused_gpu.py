"""GPU, model level: an Any-Precision Qwen3 checkpoint (explicit head_dim, per-head q / k RMSNorm in front of the rotation) on the
fused HIP route -- the plain `generate()` lands there and agrees with transformers' own Qwen3 module tree; the decode step at the
Qwen3-8B widths agrees with the module forward on every GEMV route; a captured DecodeGraph replays what the eager step computes; and
what the fused route does not serve (Gemma3, tensor-parallel decode of a QK-norm model) is declined, not decoded wrongly."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

from dispatch_table import EPI_RESIDUAL, EPI_SILU_PAIRS, ROUTES  # noqa: E402

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
    """`test_hf_routes_gpu._single_precision_model` for another architecture: 2-bit planes only, embeddings / lm_head scaled for margins,
    and q_norm / k_norm weights far from 1 (from_config_random sets every norm weight to ones)"""
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg.anyprec = dict(seed_precision=2, parent_precision=2, group_count=1, arch_config=dict(module_names=_NAMES, model_name="model", layers_name="layers"))
    m = AnyPrecisionForCausalLM.from_config_random(cfg, device=torch.device("cuda:0"), seed=seed)
    g = torch.Generator(device=m.device)
    g.manual_seed(seed + 1)
    with torch.no_grad():
        m.model.model.embed_tokens.weight.mul_(25.0)
        m.model.lm_head.weight.mul_(10.0)
        for layer in m.get_model_layers():
            for n in ("q_norm", "k_norm"):
                w = getattr(layer.self_attn, n, None)
                if w is not None:
                    w.weight.copy_((1 + 0.3 * torch.randn(w.weight.shape, device=m.device, generator=g)).half())
    return m


def _tiny_qwen3(hd, seed=5):
    return _hf_model(transformers.Qwen3Config(hidden_size=512, intermediate_size=1024, num_hidden_layers=3, num_attention_heads=8, num_key_value_heads=2,
                                              head_dim=hd, vocab_size=512, max_position_embeddings=256, rms_norm_eps=1e-6, tie_word_embeddings=False), seed)


@pytest.mark.parametrize("hd", [64, 128])
def test_plain_generate_of_a_qwen3_checkpoint_takes_the_fused_route(hd):
    m = _tiny_qwen3(hd)
    d = m.device
    assert type(m.get_model_layers()[0]).__name__ == "Qwen3DecoderLayer"
    ids = torch.tensor([[3, 17, 5, 60, 2, 9]], device=d)
    eager = m.generate(ids, max_new_tokens=24, do_sample=False, native=False, pad_token_id=0)
    fused = m.generate(ids, max_new_tokens=24, do_sample=False, pad_token_id=0)
    assert ("decoder", 2) in m._native_cache and fused.shape == eager.shape == (1, 30) and fused.dtype == ids.dtype
    dec = m._native_cache[("decoder", 2)]
    assert dec.config.qk_norm and dec.config.head_dim == hd and dec.native_ready()
    assert dec.layers[0].attention.q_norm.weight.data_ptr() == m.get_model_layers()[0].self_attn.q_norm.weight.data_ptr()
    agree = float((fused[0, 6:] == eager[0, 6:]).float().mean())
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
    # and the norm is in it: with the weights of q_norm and k_norm swapped the fused logits leave the module tree's by more than twice
    # what the right weights are allowed (measured: 8e-2 at head_dim 64, 4e-2 at 128)
    with torch.no_grad():
        for layer in m.get_model_layers():
            a, b = layer.self_attn.q_norm.weight, layer.self_attn.k_norm.weight
            t = a.clone()
            a.copy_(b)
            b.copy_(t)
        moved = dec.prefill_native(ids32, torch.arange(T, device=d, dtype=torch.int32), start=0).float().view(-1)
    assert ((moved - want).norm() / want.norm()).item() > 2 * 5e-3


def _wide_model(bits, n_layer=2, seed=0):
    """the Qwen3-8B widths (hidden 4096, MLP 12288, 32 / 8 heads of 128, vocab 151936), like test_decode_default_gpu._model"""
    from guidedquant_amd.APLinear import APLinear
    from guidedquant_amd.generate import random_init_
    from guidedquant_amd.model import ModelArgs, Transformer
    d = torch.device("cuda:0")
    cfg = ModelArgs(block_size=8192, vocab_size=151936, n_layer=n_layer, n_head=32, dim=4096, intermediate_size=12288, n_local_heads=8, head_dim=128,
                    rope_base=1000000, norm_eps=1e-6, qk_norm=True, model_name="Qwen3-8B-2layers")
    m = Transformer(torch.float16, cfg, linear_class=APLinear, linear_kwargs=dict(bitwidth=bits, device=d))
    m = m.to(device=d, dtype=torch.float16)
    random_init_(m, seed=seed + bits)
    g = torch.Generator(device=d)
    g.manual_seed(1)
    for b in m.layers:
        b.input_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
        b.post_attention_layernorm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
        b.attention.q_norm.weight.data.copy_((1 + 0.3 * torch.randn(cfg.head_dim, device=d, generator=g)).half())
        b.attention.k_norm.weight.data.copy_((1 + 0.3 * torch.randn(cfg.head_dim, device=d, generator=g)).half())
    m.norm.weight.data.copy_((1 + 0.1 * torch.randn(cfg.dim, device=d, generator=g)).half())
    m.tok_embeddings.weight.data.mul_(25.0)
    m.output.weight.data.mul_(4.0)
    return m.eval()


@pytest.mark.parametrize("bits", [2, 3, 4, 5])
def test_decode_at_qwen3_8b_widths_matches_the_module_forward(bits, monkeypatch):
    """`test_default_mode_decode_at_8b_widths_matches_torch_forward` for the QK-norm layer: ten positions, the module forward in exact mode
    as the yardstick (anchored to transformers by the test above), the same bounds and the same token list; every AP-GEMV launch of the
    step on its route.  Measured at 2 bits: norm-wise 2.1e-3 .. 3.5e-3 over the ten positions (bound 5e-3).  The yardstick is noisy at
    this bound: with 151000 as the first token, position 0 -- attention over one key, where the norm cannot act -- reads 6.0e-3 with
    qk_norm and 6.0e-3 with it switched off; against a dense fp32 twin the exact-mode module forward is 5.2e-3 off there, the fused step
    1.5e-3 (profiles/qwen3_fused_route.json, `decode_8b_widths`)."""
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
        routes.append((int(a[4]), int(a[5])) + _lib.ap_last_route())
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
        for p, t in enumerate(toks):
            lg = m.decode_native(torch.tensor([t], dtype=torch.int32, device=d), torch.tensor([p], dtype=torch.int32, device=d))
            torch.cuda.synchronize()
            a, r = lg.float().view(-1), ref[p]
            assert torch.isfinite(a).all()
            scale, err = r.abs().max().item(), (a - r).abs().max().item()
            rel = ((a - r).norm() / r.norm()).item()
            print("bits %d pos %d: element-wise %.3e of %.3f  norm-wise %.3e" % (bits, p, err, scale, rel))
            assert err <= TOL * scale, (p, err, scale)
            assert rel <= (5e-3 if bits == 2 else 7.5e-3), (p, bits, rel)
        monkeypatch.undo()
    n = len(toks)
    for i, b in enumerate(m.layers):
        dk = (b.attention.kv_cache.k_cache[:, :, :n].float() - ref_k[i][:, :, :n].float()).abs().max().item()
        dv = (b.attention.kv_cache.v_cache[:, :, :n].float() - ref_v[i][:, :, :n].float()).abs().max().item()
        assert dk <= TOL * ref_k[i][:, :, :n].float().abs().max().item(), (i, dk)
        assert dv <= TOL * ref_v[i][:, :, :n].float().abs().max().item(), (i, dv)
    # the launches of one step, in order: (wqkv, wo, w1w3, w2) per layer -- the real route equals the dry one, the wqkv launch never
    # takes the RoPE-epilogue kernel (it would rotate un-normalised values), and the shapes shared with Llama-3.1-8B take its routes
    assert len(routes) == n * 2 * 4
    forms = (("wqkv", 6144, 4096, True, 0), ("wo", 4096, 4096, False, EPI_RESIDUAL), ("w1w3", 24576, 4096, True, EPI_SILU_PAIRS),
             ("w2", 4096, 12288, False, EPI_RESIDUAL))
    for i, (N, K, fam, launches, variant) in enumerate(routes):
        name, wN, wK, norm, epi = forms[i % 4]
        assert (N, K) == (wN, wK), (i, N, K)
        assert fam != "stream-qkv-rope", (name, fam)
        assert (fam, launches, variant) == _lib.ap_plan_route(N, K, bits, 1, norm, epi, 0), (name, fam)
        if bits == 5:
            assert fam == "wide", (name, fam)
        elif name in ("wqkv", "wo"):
            assert fam == ROUTES[("8B", bits)][name], (name, fam)


@pytest.mark.parametrize("spr", [1, 8])
def test_decode_graph_replay_equals_the_eager_step_on_a_qk_norm_model(spr):
    from guidedquant_amd.generate import DecodeGraph
    m = _tiny_qwen3(128, seed=7)
    d = m.device
    dec = m.native_decoder(2)
    dec.setup_caches(1, 64)
    assert dec.native_ready()
    n = 40
    eager, t = [], 3
    with torch.no_grad():
        for p in range(n):
            lg = dec.decode_native(torch.tensor([t], dtype=torch.int32, device=d), torch.tensor([p], dtype=torch.int32, device=d))
            t = int(lg.float().view(-1).argmax().item())
            eager.append(t)
    for b in dec.layers:
        b.attention.kv_cache.k_cache.zero_()
        b.attention.kv_cache.v_cache.zero_()
    g = DecodeGraph(dec, d, native_sampling=True, temperature=0.0, top_k=32, seq_capacity=65, steps_per_replay=spr)
    g.set_token(3, 0)
    for _ in range(n // spr):
        g.step()
    torch.cuda.synchronize()
    assert g.seq[1:n + 1].tolist() == eager and int(g.pos.item()) == n
    assert len(set(eager)) > 4  # not a fixed point
    g.close() if hasattr(g, "close") else None


def test_gemma3_is_handed_to_transformers_and_tensor_parallel_declines_qk_norm():
    m = _hf_model(transformers.Gemma3TextConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                                head_dim=64, vocab_size=512, max_position_embeddings=256, tie_word_embeddings=False))
    ids = torch.tensor([[3, 17, 5, 60, 2, 9]], device=m.device)
    plain = m.generate(ids, max_new_tokens=12, do_sample=False, pad_token_id=0)
    assert not any(k[0] == "decoder" for k in m._native_cache)
    assert torch.equal(plain, m.generate(ids, max_new_tokens=12, do_sample=False, native=False, pad_token_id=0))
    with pytest.raises(ValueError, match="gemma3"):
        m.generate(ids, max_new_tokens=4, do_sample=False, native=True, pad_token_id=0)
    from guidedquant_amd.tp import TensorParallelDecoder
    q = _tiny_qwen3(64)
    with pytest.raises(NotImplementedError, match="QK-norm"):
        TensorParallelDecoder(q.native_decoder(2), None, 0, 2, 8)


def test_a_vocabulary_beyond_the_fused_sampler_is_handed_to_transformers():
    """the captured step ends in the fused sampler (at most 131072 logits): a larger vocabulary -- Qwen3's published one is 151936 -- must
    not reach it through `generate()`; the decoder itself (decode_native: the 8B-width test above runs at 151936) stays available"""
    from guidedquant_amd._lib import SAMPLER_MAX_VOCAB
    m = _hf_model(transformers.Qwen3Config(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                                           head_dim=64, vocab_size=SAMPLER_MAX_VOCAB + 512, max_position_embeddings=256, rms_norm_eps=1e-6,
                                           tie_word_embeddings=False))
    ids = torch.tensor([[3, 17, 5, 60, 2, 9]], device=m.device)
    plain = m.generate(ids, max_new_tokens=8, do_sample=False, pad_token_id=0)
    assert not any(k[0] == "graph" for k in m._native_cache)
    assert torch.equal(plain, m.generate(ids, max_new_tokens=8, do_sample=False, native=False, pad_token_id=0))
    with pytest.raises(ValueError, match="vocabulary"):
        m.generate(ids, max_new_tokens=4, do_sample=False, native=True, pad_token_id=0)
    assert m.native_decoder(2).config.vocab_size == SAMPLER_MAX_VOCAB + 512
