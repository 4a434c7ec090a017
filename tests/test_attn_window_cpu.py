"""CPU: the host side of sliding-window layers -- the mask the module forward and the prompt pass hand a windowed layer
(model.window_mask) against transformers' own overlay, how hf_loader resolves a config's layers to ModelArgs.layer_windows (only when asked:
the one-argument call keeps declining), and the row ranges of a window launch as tests/test_attn_window_gpu.py states them."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

import attn_probes as ap  # noqa: E402


@pytest.mark.parametrize("W", [1, 2, 16, 40, 100])
def test_mask_builder_equals_transformers_overlay_on_the_causal_mask(W):
    from transformers import masking_utils as mu
    from guidedquant_amd.model import window_mask
    n = 40
    overlay = mu.sliding_window_overlay(W)
    want = torch.tensor([[bool(mu.causal_mask_function(0, 0, q, kv)) and bool(overlay(0, 0, q, kv)) for kv in range(n)] for q in range(n)])
    got = window_mask(n, W)
    assert got.dtype == torch.bool and torch.equal(got, want)
    assert int(got.sum(1).max()) == min(W, n) and bool(got.diagonal().all())
    if W >= n:  # a window the grid never outgrows is the causal mask
        assert torch.equal(got, window_mask(n, None)) and torch.equal(got, torch.tril(torch.ones(n, n, dtype=torch.bool)))


_SMALL = dict(hidden_size=512, intermediate_size=1024, num_attention_heads=8, num_key_value_heads=2, vocab_size=512)


def _resolve(cfg):
    from guidedquant_amd.hf_loader import model_args_from_hf_config
    return model_args_from_hf_config(cfg.to_dict(), sliding_window=True)


def _declines(cfg):
    from guidedquant_amd.hf_loader import model_args_from_hf_config
    with pytest.raises(NotImplementedError):
        model_args_from_hf_config(cfg.to_dict())


def test_mistral_as_published_resolves_to_a_window_on_every_layer():
    cfg = transformers.MistralConfig(num_hidden_layers=4, sliding_window=4096, max_position_embeddings=32768, **_SMALL)
    a = _resolve(cfg)
    assert a.layer_windows == (4096,) * 4 and a.block_size == 32768 and not a.qk_norm and not a.attn_bias
    _declines(cfg)


def test_qwen2_windows_start_at_max_window_layers():
    cfg = transformers.Qwen2Config(num_hidden_layers=4, use_sliding_window=True, sliding_window=8, max_window_layers=2, **_SMALL)
    assert cfg.to_dict().get("layer_types") in (None, ["full_attention", "full_attention", "sliding_attention", "sliding_attention"])
    a = _resolve(cfg)
    assert a.layer_windows == (None, None, 8, 8) and a.attn_bias
    _declines(cfg)
    # the same without the resolved layer_types (an older config.json): from use_sliding_window / max_window_layers
    d = cfg.to_dict()
    d.pop("layer_types", None)
    from guidedquant_amd.hf_loader import model_args_from_hf_config
    assert model_args_from_hf_config(d, sliding_window=True).layer_windows == (None, None, 8, 8)
    with pytest.raises(NotImplementedError):
        model_args_from_hf_config(d)


def test_qwen3_layer_types_are_taken_as_they_are():
    lt = ["sliding_attention", "full_attention", "sliding_attention"]
    cfg = transformers.Qwen3Config(num_hidden_layers=3, layer_types=lt, sliding_window=16, use_sliding_window=True, head_dim=64, **_SMALL)
    a = _resolve(cfg)
    assert a.layer_windows == (16, None, 16) and a.qk_norm and a.head_dim == 64
    _declines(cfg)


def test_a_window_the_context_never_outgrows_is_no_window():
    for cfg in (transformers.MistralConfig(num_hidden_layers=2, sliding_window=4096, max_position_embeddings=4096, **_SMALL),
                transformers.MistralConfig(num_hidden_layers=2, sliding_window=8192, max_position_embeddings=4096, **_SMALL),
                transformers.Qwen2Config(num_hidden_layers=2, use_sliding_window=True, sliding_window=512, max_window_layers=0,
                                         max_position_embeddings=256, **_SMALL)):
        assert _resolve(cfg).layer_windows is None
    # and a model without sliding-window layers is what it was
    from guidedquant_amd.hf_loader import model_args_from_hf_config
    plain = transformers.Qwen2Config(num_hidden_layers=2, **_SMALL).to_dict()
    assert model_args_from_hf_config(plain, sliding_window=True) == model_args_from_hf_config(plain)
    assert model_args_from_hf_config(plain).layer_windows is None


def test_an_unknown_layer_type_still_raises():
    from guidedquant_amd.hf_loader import model_args_from_hf_config
    d = transformers.Qwen3Config(num_hidden_layers=2, **_SMALL).to_dict()
    d["layer_types"] = ["full_attention", "chunked_attention"]
    d["sliding_window"] = 16
    for kw in (dict(sliding_window=True), {}):
        with pytest.raises(NotImplementedError, match="layer_types"):
            model_args_from_hf_config(d, **kw)


def test_model_args_keep_one_window_per_layer():
    from guidedquant_amd.model import ModelArgs
    assert ModelArgs(n_layer=2, model_name="llama-x").layer_windows is None
    assert ModelArgs(n_layer=2, model_name="llama-x", layer_windows=[None, None]).layer_windows is None
    assert ModelArgs(n_layer=2, model_name="llama-x", layer_windows=[None, 4]).layer_windows == (None, 4)
    for bad in ([4], [0, 4]):
        with pytest.raises(AssertionError):
            ModelArgs(n_layer=2, model_name="llama-x", layer_windows=bad)


def test_module_forward_hands_each_layer_its_own_mask():
    """a two-layer fp32 model on the CPU, layer 1 with W = 3: its logits equal those of a forward whose layer-1 attention is masked by
    hand, and differ from the model without the window"""
    from guidedquant_amd.model import ModelArgs, Transformer, window_mask
    torch.manual_seed(0)
    kw = dict(block_size=32, vocab_size=64, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128, model_name="llama-tiny")
    m = Transformer(torch.float32, ModelArgs(layer_windows=(None, 3), **kw)).eval()
    full = Transformer(torch.float32, ModelArgs(**kw)).eval()
    full.load_state_dict(m.state_dict())
    m.setup_caches(1, 16)
    full.setup_caches(1, 16)
    assert set(m.window_masks) == {3} and full.window_masks == {} and torch.equal(m.window_masks[3], window_mask(16, 3))
    idx, pos = torch.randint(0, 64, (1, 10)), torch.arange(10)
    with torch.no_grad():
        got, plain = m(idx, pos), full(idx, pos)
        # by hand: the blocks of `full`, layer 1 with the window mask
        x = full.tok_embeddings(idx)
        x = full.layers[0](x, pos, full.causal_mask[None, None, pos], full.rope_cos, full.rope_sin)
        x = full.layers[1](x, pos, window_mask(16, 3)[None, None, pos], full.rope_cos, full.rope_sin)
        want = full.output(full.norm(x))
    assert torch.allclose(got, want, atol=1e-6, rtol=0)
    assert float((got - plain)[0, 4:].abs().max()) > 1e-3 and torch.allclose(got[0, :3], plain[0, :3], atol=1e-6, rtol=0)


def test_windowed_geometry_covers_the_window_exactly_once():
    """the row ranges of a window launch as the GPU test states them (attn_probes.geometry at n - 1, shifted by lo): the blocks' ranges
    tile [lo, pos] -- each row in exactly one -- for every (W, pos, n_split) the shift-identity test launches"""
    import test_attn_window_gpu as tw
    seen = 0
    for hd in (64, 128):
        P = ap.geometry(hd, 0, 1).PASS
        for W, max_seq, poss in tw.window_cases(hd):
            assert (max_seq - W) % 2 == 1
            for pos in poss:
                for ns in tw.SPLITS:
                    lo, n, splits = tw.window_geometry(hd, pos, ns, W)
                    assert 0 <= lo <= pos and n == min(W, pos + 1) and lo == max(0, pos + 1 - W)
                    count = [0] * (pos + 2)
                    for a, b in splits:
                        assert a >= lo and (a - lo) % P == 0
                        for t in range(a, min(b, pos + 2)):
                            count[t] += 1
                    assert count[:lo] == [0] * lo and count[lo:pos + 1] == [1] * n and count[pos + 1] == 0, (hd, W, pos, ns)
                    assert (len(splits) == 1) == (ns == 1 or n <= 2 * P)
                    seen += 1
    assert seen >= 2 * 7 * 4 * 4
